"""ORACLE for tests/test_segment.py (test infrastructure only): the segmentation of csrc/segment.hip, every pair of a cloud.

A float32 numpy restatement of the pair expression, written from its definition (include/smarttree_hip.h):
ab = b - a; dot = (x*x' + y*y') + z*z'; t = clip01(dot(ap, ab) / dot(ab, ab)), t = 0 for a zero-length tube; q = a + t*ab;
r = (1 - t)*r1 + t*r2; v = q - p; residual = sqrt(dot(v, v)) - r; score = |residual|.  numpy rounds every float32 operation and
never contracts.  A tube with a non-finite value and a NaN score never win, a non-finite point gets no tube; the winner is the
minimum of (score bits, index); a best score > max_distance is unassigned (-1, +inf, 0, NaN).

`check64` evaluates the same pairs in float64 and asserts that the float32 winner is the float64 minimiser wherever the two best
float32 scores lie further apart than `gap` (1e-5: two orders above the rounding of a score between points and tubes a few metres
from the origin; callers that move the scene kilometres away pass the gap that goes with those coordinates).
"""
from __future__ import annotations

import numpy as np

F = np.float32
FIX = F(2.0 ** 24)
CLAMP = F(2.0 ** 62)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def pairs(p, a, b, r1, r2, dtype=F):
    """(v [n,m,3], r [n,m], residual [n,m]) of every pair in `dtype`."""
    one, zero = dtype(1), dtype(0)
    p, a, b, r1, r2 = (np.asarray(x, dtype) for x in (p, a, b, r1, r2))
    ab = b - a
    ab2 = _dot(ab, ab)
    with np.errstate(all="ignore"):
        t = _dot(p[:, None, :] - a[None], ab[None]) / ab2[None]
        t = np.where(t < zero, zero, np.where(t > one, one, t))
        t = np.where(ab2[None] == zero, zero, t).astype(dtype)
        q = a[None] + t[..., None] * ab[None]
        r = (one - t) * r1[None] + t * r2[None]
        v = q - p[:, None, :]
        res = np.sqrt(_dot(v, v)) - r
    assert v.dtype == dtype and res.dtype == dtype
    return v, r, res


def fix(x):
    """llrintf(x * 2^24) with the scaled value clamped to +-2^62 (round half to even, as the default rounding mode does)."""
    q = np.minimum(np.maximum(np.asarray(x, F) * FIX, -CLAMP), CLAMP)
    return np.rint(q.astype(np.float64)).astype(np.int64)


def segment(pts, a, b, r1, r2, pt_off=None, tube_off=None, max_distance=None, check64=True, gap=1e-5, chunk=512):
    pts, a, b = np.asarray(pts, F).reshape(-1, 3), np.asarray(a, F).reshape(-1, 3), np.asarray(b, F).reshape(-1, 3)
    r1, r2 = np.asarray(r1, F).reshape(-1), np.asarray(r2, F).reshape(-1)
    n, m = len(pts), len(a)
    pt_off = [0, n] if pt_off is None else [int(x) for x in pt_off]
    tube_off = [0, m] if tube_off is None else [int(x) for x in tube_off]
    tube = np.full(n, -1, np.int32)
    residual = np.full(n, np.inf, F)
    vec = np.zeros((n, 3), F)
    rad = np.full(n, np.nan, F)
    ok_tube = np.isfinite(a).all(1) & np.isfinite(b).all(1) & np.isfinite(r1) & np.isfinite(r2)
    for s in range(len(pt_off) - 1):
        t0, t1 = tube_off[s], tube_off[s + 1]
        if t1 == t0:
            continue
        for c0 in range(pt_off[s], pt_off[s + 1], chunk):
            c1 = min(c0 + chunk, pt_off[s + 1])
            p = pts[c0:c1]
            v, r, res = pairs(p, a[t0:t1], b[t0:t1], r1[t0:t1], r2[t0:t1])
            score = np.abs(res)
            live = ok_tube[None, t0:t1] & ~np.isnan(score) & np.isfinite(p).all(1)[:, None]
            key = np.where(live, score.view(np.uint32).astype(np.int64), np.int64(1) << 40)
            w = key.argmin(1)  # the first minimum: the lowest index among equal bits
            rows = np.arange(len(p))
            found = live[rows, w]
            if check64 and live.any():
                with np.errstate(all="ignore"):
                    s64 = np.abs(pairs(p, a[t0:t1], b[t0:t1], r1[t0:t1], r2[t0:t1], np.float64)[2])
                s64 = np.where(live, s64, np.inf)
                s32 = np.where(live, score, F(np.inf))
                two = np.partition(s32, 1, axis=1)[:, :2] if s32.shape[1] > 1 else np.concatenate([s32, np.full_like(s32, np.inf)], 1)
                with np.errstate(invalid="ignore"):
                    clear = found & np.isfinite(two[:, 0]) & ((two[:, 1] - two[:, 0]) > gap)
                assert np.array_equal(s64.argmin(1)[clear], w[clear]), "the float32 winner is not the float64 minimiser"
            keep = found if max_distance is None else found & (score[rows, w] <= F(max_distance))
            idx = rows[keep]
            tube[c0 + idx] = (t0 + w[keep]).astype(np.int32)
            residual[c0 + idx] = res[idx, w[keep]]
            vec[c0 + idx] = v[idx, w[keep]]
            rad[c0 + idx] = r[idx, w[keep]]
    tally = np.zeros((m, 3), np.int64)
    won = tube >= 0
    np.add.at(tally[:, 0], tube[won], 1)
    np.add.at(tally[:, 1], tube[won], fix(np.abs(residual[won])))
    np.add.at(tally[:, 2], tube[won], fix(residual[won]))
    return {"tube": tube, "residual": residual, "vec": vec, "rad": rad, "tally": tally}
