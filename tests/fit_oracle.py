"""ORACLE for tests/test_fit.py (test infrastructure only): the tube fit of csrc/fit.hip, restated on its own in numpy.

The pair, the frame and the moments are float32, operation by operation (numpy rounds every float32 operation and never contracts):
  ab = b - a; dot(u, w) = (ux*wx + uy*wy) + uz*wz; k = the coordinate with the smallest |ab_k| (strict comparisons from 0 on);
  cross(u, w) = (uy*wz - uz*wy, uz*wx - ux*wz, ux*wy - uy*wx); e1 = normalise(cross(ab, unit_k)); e2 = normalise(cross(ab, e1));
  normalise(x) = x / sqrt(dot(x, x)).
  A point enters when its tube is in [0, m), it is finite, q = dot(p - a, ab) / dot(ab, ab) has 0 <= q <= 1,
  r = (1 - q)*r1 + q*r2, v = (a + q*ab) - p, rho = sqrt(dot(v, v)) > 0, and max_relative < 0 or |rho - r| <= max_relative * r.
  w = (-v) / rho, c = dot(w, e1), s = dot(w, e2); per tube the count and the sums of fix(x) = rint(min(max(x * 2^24, -2^40), 2^40))
  of c*c, c*s, s*s, c, s, rho*c, rho*s, rho, rho*rho (min / max that drop a NaN, as fminf / fmaxf do).
The solve is float64 (`solve`): numpy's own linear solver on the 3x3 normal equations, the eigenvalue in closed form.
"""
from __future__ import annotations

import numpy as np

F = np.float32
FIX = F(2.0 ** 24)
CLAMP = F(2.0 ** 40)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(u, w):
    return np.stack([u[..., 1] * w[..., 2] - u[..., 2] * w[..., 1], u[..., 2] * w[..., 0] - u[..., 0] * w[..., 2],
                     u[..., 0] * w[..., 1] - u[..., 1] * w[..., 0]], axis=-1)


def _normalise(x):
    with np.errstate(all="ignore"):
        return x / np.sqrt(_dot(x, x))[..., None]


def frames(a, b):
    """(ab, e1, e2) float32 [m,3]."""
    a, b = np.asarray(a, F).reshape(-1, 3), np.asarray(b, F).reshape(-1, 3)
    ab = b - a
    mag = np.abs(ab)
    k = np.zeros(len(ab), np.int64)
    least = mag[:, 0].copy()
    with np.errstate(invalid="ignore"):
        one = mag[:, 1] < least
        k[one], least[one] = 1, mag[one, 1]
        k[mag[:, 2] < least] = 2
    unit = np.zeros_like(ab)
    unit[np.arange(len(ab)), k] = F(1)
    with np.errstate(all="ignore"):
        e1 = _normalise(_cross(ab, unit))
        e2 = _normalise(_cross(ab, e1))
    assert e1.dtype == F and e2.dtype == F
    return ab, e1, e2


def fix(x):
    with np.errstate(all="ignore"):
        q = np.fmin(np.fmax(np.asarray(x, F) * FIX, -CLAMP), CLAMP)
    return np.rint(q.astype(np.float64)).astype(np.int64)


def moments(pts, tube, a, b, r1, r2, max_relative=0.5):
    """int64 [m,10] and the boolean [n] of the points that entered."""
    pts, a, b = np.asarray(pts, F).reshape(-1, 3), np.asarray(a, F).reshape(-1, 3), np.asarray(b, F).reshape(-1, 3)
    r1, r2, tube = np.asarray(r1, F).reshape(-1), np.asarray(r2, F).reshape(-1), np.asarray(tube, np.int64).reshape(-1)
    n, m = len(pts), len(a)
    out = np.zeros((m, 10), np.int64)
    ok = (tube >= 0) & (tube < m) & np.isfinite(pts).all(1) if n else np.zeros(0, bool)
    if not ok.any():
        return out, ok
    ab, e1, e2 = frames(a, b)
    idx = np.flatnonzero(ok)
    t, p = tube[idx], pts[idx]
    one = F(1)
    with np.errstate(all="ignore"):
        q = _dot(p - a[t], ab[t]) / _dot(ab[t], ab[t])
        inside = (q >= 0) & (q <= 1)
        r = (one - q) * r1[t] + q * r2[t]
        v = (a[t] + q[:, None] * ab[t]) - p
        rho = np.sqrt(_dot(v, v))
        res = rho - r
        keep = inside & (rho > 0)
        if max_relative >= 0:
            keep &= np.abs(res) <= F(max_relative) * r
        w = (-v) / rho[:, None]
        c, s = _dot(w, e1[t]), _dot(w, e2[t])
        assert c.dtype == F and rho.dtype == F and q.dtype == F
        terms = [c * c, c * s, s * s, c, s, rho * c, rho * s, rho, rho * rho]
    ok[idx[~keep]] = False
    t = t[keep]
    np.add.at(out[:, 0], t, 1)
    for k, x in enumerate(terms):
        np.add.at(out[:, k + 1], t, fix(x[keep]))
    return out, ok


def solve(mom, a, b, min_points=8, min_spread=0.01):
    """float64 [m,8]: N, R, offset (3), rms, spread, status -- from the integer moments."""
    mom = np.asarray(mom, np.int64).reshape(-1, 10)
    _, e1, e2 = frames(a, b)
    out = np.zeros((len(mom), 8))
    for g, M in enumerate(mom):
        N = float(M[0])
        out[g, 0] = N
        if M[0] < min_points or M[0] <= 0:
            continue
        Scc, Scs, Sss, Sc, Ss, Src, Srs, Sr, Srr = (float(x) / 2.0 ** 24 for x in M[1:])
        cov = np.array([[Scc, Scs], [Scs, Sss]]) / N - np.outer([Sc / N, Ss / N], [Sc / N, Ss / N])
        spread = 0.5 * (cov[0, 0] + cov[1, 1]) - np.sqrt((0.5 * (cov[0, 0] - cov[1, 1])) ** 2 + cov[0, 1] ** 2)
        x, status = np.array([0.0, 0.0, Sr / N]), 1.0
        rhs = np.array([Src, Srs, Sr])
        if spread >= min_spread:
            try:
                full = np.linalg.solve(np.array([[Scc, Scs, Sc], [Scs, Sss, Ss], [Sc, Ss, N]]), rhs)
            except np.linalg.LinAlgError:
                full = np.full(3, np.nan)
            if np.isfinite(full).all():
                x, status = full, 2.0
        out[g, 1] = x[2]
        if status == 2.0:
            out[g, 2:5] = x[0] * e1[g].astype(np.float64) + x[1] * e2[g].astype(np.float64)
        out[g, 5] = np.sqrt(max(Srr - float(x @ rhs), 0.0) / N)
        out[g, 6] = spread
        out[g, 7] = status
    return out


def fit(pts, tube, a, b, r1, r2, max_relative=0.5, min_points=8, min_spread=0.01):
    mom, _ = moments(pts, tube, a, b, r1, r2, max_relative)
    return mom, solve(mom, a, b, min_points, min_spread)
