"""ORACLE for tests/test_skeleton_eval.py (test infrastructure only -- never imported by the product path).

numpy restatement of csrc/skeleton_eval.hip in float32 with the kernel's operation order:
  sampling  v = b - a, len = sqrt((vx*vx + vy*vy) + vz*vz), n = ceil(float64(len) / spacing), 0 for a zero / non-finite len;
            sample k < n: f = float32(k) / float32(n), point a + v*f, radius r1 + (r2 - r1)*f.
  matching  dot(u,w) = (ux*wx + uy*wy) + uz*wz; inv = 1 / dot(ab,ab) (0 where dot(ab,ab) == 0); t = dot(ap,ab) * inv,
            t = t > 0 ? t : 0 (NaN -> 0), t = t < 1 ? t : 1; q = a + t*ab; d2 = dot(q - p, q - p); first minimum over the
            tubes with d2 < +inf (NaN / inf never win; none: idx = -1, dist = +inf, tube_rad = NaN);
            dist = sqrt(d2), tube_rad = (1 - t)*r1 + t*r2; hit j: idx >= 0 and dist <= thr[j] * ref (float32 product).
"""
from __future__ import annotations

import numpy as np

F32 = np.float32


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def sample_tubes(a, b, r1, r2, spacing):
    """-> (count [m] int32, off [m] int32, pts [N,3], rad [N], tube_of [N] int32)."""
    a, b = np.asarray(a, F32).reshape(-1, 3), np.asarray(b, F32).reshape(-1, 3)
    r1, r2 = np.asarray(r1, F32).reshape(-1), np.asarray(r2, F32).reshape(-1)
    v = (b - a).astype(F32)
    with np.errstate(invalid="ignore", over="ignore"):
        length = np.sqrt(_dot(v, v)).astype(F32)
        live = np.isfinite(length) & (length > 0)
        count = np.where(live, np.ceil(np.where(live, length, 0).astype(np.float64) / float(spacing)), 0.0).astype(np.int64)
    off = np.cumsum(count) - count
    tube_of = np.repeat(np.arange(len(a)), count)
    k = np.arange(len(tube_of)) - off[tube_of]
    f = (k.astype(F32) / count[tube_of].astype(F32)).astype(F32)
    pts = (a[tube_of] + (v[tube_of] * f[:, None]).astype(F32)).astype(F32)
    rad = (r1[tube_of] + ((r2 - r1).astype(F32)[tube_of] * f).astype(F32)).astype(F32)
    return count.astype(np.int32), off.astype(np.int32), pts, rad, tube_of.astype(np.int32)


def match(pts, rad, a, b, r1, r2, thr, ref_mode, chunk: int = 1024):
    """-> dict(dist, idx (int32), tube_rad, hits (int64 [T]), terms = the float32 terms of the four sums (for idx >= 0))."""
    pts, rad = np.asarray(pts, F32).reshape(-1, 3), np.asarray(rad, F32).reshape(-1)
    a, b = np.asarray(a, F32).reshape(-1, 3), np.asarray(b, F32).reshape(-1, 3)
    r1, r2, thr = np.asarray(r1, F32).reshape(-1), np.asarray(r2, F32).reshape(-1), np.asarray(thr, F32).reshape(-1)
    n = len(pts)
    ab = (b - a).astype(F32)
    with np.errstate(all="ignore"):
        ab2 = _dot(ab, ab).astype(F32)
        inv = np.where(ab2 == 0, F32(0), F32(1) / np.where(ab2 == 0, F32(1), ab2)).astype(F32)
    dist, idx, trad = np.empty(n, F32), np.empty(n, np.int32), np.empty(n, F32)
    for s in range(0, n, chunk):
        p = pts[s:s + chunk, None, :]
        with np.errstate(all="ignore"):
            t = (_dot((p - a[None]).astype(F32), ab[None]) * inv[None]).astype(F32)
            t = np.where(t > 0, t, F32(0)).astype(F32)
            t = np.where(t < 1, t, F32(1)).astype(F32)
            q = (a[None] + (t[..., None] * ab[None]).astype(F32)).astype(F32)
            v = (q - p).astype(F32)
            d2 = _dot(v, v).astype(F32)
            key = np.where(d2 < np.inf, d2, np.inf)  # NaN and inf never win
            best = key.argmin(1)  # first minimum
            rows = np.arange(len(best))
            none = ~(key[rows, best] < np.inf)
            tb = t[rows, best]
            r = (((F32(1) - tb) * r1[best]).astype(F32) + (tb * r2[best]).astype(F32)).astype(F32)
            dist[s:s + chunk] = np.where(none, F32(np.inf), np.sqrt(d2[rows, best]).astype(F32))
            idx[s:s + chunk] = np.where(none, -1, best)
            trad[s:s + chunk] = np.where(none, F32(np.nan), r)
    ok = idx >= 0
    ref = trad if ref_mode else rad
    with np.errstate(all="ignore"):
        hits = np.array([int((ok & (dist <= (th * ref).astype(F32))).sum()) for th in thr], np.int64)
        e = np.abs(rad - trad).astype(F32)
        terms = np.stack([dist[ok], e[ok], (e / ref).astype(F32)[ok], np.ones(int(ok.sum()), F32)], 0)
    return {"dist": dist, "idx": idx, "tube_rad": trad, "hits": hits, "terms": terms}
