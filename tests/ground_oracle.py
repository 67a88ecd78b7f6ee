"""Oracle of the terrain calls (csrc/ground.hip), restated from include/smarttree_hip.h on its own: numpy, the index and weight arithmetic in
float32 in the header's order, the morphology a plain loop over the window's offsets on the ordered bits, the blend in float64."""
import numpy as np

F = np.float32
ORD_POS_INF = np.uint32(0xff800000)


def f2ord(x):
    u = np.ascontiguousarray(x, F).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def ord2f(o):
    o = np.ascontiguousarray(o, np.uint32)
    return np.where(o & np.uint32(0x80000000), o & np.uint32(0x7fffffff), ~o).astype(np.uint32).view(F)


def plan_axes(up):
    return (1 if up == 0 else 0), (1 if up == 2 else 2)


def takes_part(pts):
    return np.isfinite(pts).all(1)


def _clouds(n, seg_off):
    off = [0, n] if seg_off is None else [int(v) for v in seg_off]
    return list(zip(off[:-1], off[1:]))


def _quotient(p, o, cell):
    with np.errstate(all="ignore"):
        return ((p.astype(F) - F(o)).astype(F) / F(cell)).astype(F)


def extent(pts, seg_off=None, cell=0.5, up=1):
    """(origin float32 [S,2], dims int32 [S,2])."""
    a, b = plan_axes(up)
    origin, dims = [], []
    for lo, hi in _clouds(len(pts), seg_off):
        p = pts[lo:hi][takes_part(pts[lo:hi])]
        if not len(p):
            origin.append([np.inf, np.inf])
            dims.append([0, 0])
            continue
        o = [ord2f(f2ord(p[:, k]).min().reshape(1))[0] for k in (a, b)]
        origin.append(o)
        dims.append([int(np.floor(_quotient(p[:, k], o[j], cell)).max()) + 1 for j, k in enumerate((a, b))])
    return np.asarray(origin, F).reshape(-1, 2), np.asarray(dims, np.int32).reshape(-1, 2)


def _window(keys, w, pad, reduce):
    A, B = keys.shape
    big = np.full((A + 2 * w, B + 2 * w), pad, np.uint32)
    big[w:w + A, w:w + B] = keys
    out = np.full((A, B), pad, np.uint32)
    for da in range(2 * w + 1):
        for db in range(2 * w + 1):
            out = reduce(out, big[da:da + A, db:db + B])
    return out


def raster(pts, origin, dims, cell=0.5, up=1):
    """Z float32 [A,B] of one cloud: the ordered minimum per cell, +inf without points."""
    a, b = plan_axes(up)
    A, B = int(dims[0]), int(dims[1])
    z = np.full(A * B, ORD_POS_INF, np.uint32)
    p = pts[takes_part(pts)]
    if len(p) and A * B:
        fa, fb = np.floor(_quotient(p[:, a], origin[0], cell)), np.floor(_quotient(p[:, b], origin[1], cell))
        ok = (fa >= 0) & (fa < A) & (fb >= 0) & (fb < B)
        idx = fa[ok].astype(np.int64) * B + fb[ok].astype(np.int64)
        np.minimum.at(z, idx, f2ord(p[ok, up]))
    return ord2f(z).reshape(A, B)


def open_raster(z, w, dh):
    """(surface float32 [A,B], flags uint8 [A,B]) from the raster of minima."""
    z = z.copy()
    flags = np.isposinf(z).astype(np.uint8)
    for wk, dk in zip(w, dh):
        wk = int(wk)
        e = _window(f2ord(z), wk, ORD_POS_INF, np.minimum)
        finite = np.where(e < ORD_POS_INF, e, np.uint32(0))
        o = _window(finite, wk, np.uint32(0), np.maximum)
        o = np.where(o == 0, F(np.inf), ord2f(np.where(o == 0, ORD_POS_INF, o)))
        with np.errstate(invalid="ignore"):
            hit = (z - o).astype(F) > F(dk)
        flags[hit] |= 2
        z = np.where(hit, o, z).astype(F)
    return z, flags


def model(pts, seg_off=None, cell=0.5, up=1, w=(1,), dh=(0.5,)):
    """origin, dims, cell_off int64 [S+1], surface float32 [cells], flags uint8 [cells]."""
    origin, dims = extent(pts, seg_off, cell, up)
    surface, flags = [np.zeros(0, F)], [np.zeros(0, np.uint8)]
    for k, (lo, hi) in enumerate(_clouds(len(pts), seg_off)):
        s, f = open_raster(raster(pts[lo:hi], origin[k], dims[k], cell, up), w, dh)
        surface.append(s.reshape(-1))
        flags.append(f.reshape(-1))
    cell_off = np.concatenate([[0], np.cumsum(dims[:, 0].astype(np.int64) * dims[:, 1])]).astype(np.int64)
    return origin, dims, cell_off, np.concatenate(surface), np.concatenate(flags)


def height(q, origin, dims, surface, cell=0.5, up=1, tol=0.2):
    """(height float64 [m], is_ground uint8 [m], ground float64 [m], scale float64 [m]) of queries against ONE cloud's raster
    `surface` [A,B]; scale = max(1, |p_up|, largest |sample|), what the tolerance of `height` is relative to."""
    a, b = plan_axes(up)
    A, B = int(dims[0]), int(dims[1])
    m = len(q)
    h, g, is_ground, scale = np.full(m, np.nan), np.full(m, np.nan), np.zeros(m, np.uint8), np.ones(m)
    if not A * B or not m:
        return h, is_ground, g, scale
    s = surface.reshape(A, B)
    with np.errstate(all="ignore"):
        clamp = lambda f, n: np.nan_to_num(np.minimum(np.maximum(f, F(0)), F(n - 1)), nan=0.0).astype(np.int64)
        qa, qb = _quotient(q[:, a], origin[0], cell), _quotient(q[:, b], origin[1], cell)
        own = s[clamp(np.floor(qa), A), clamp(np.floor(qb), B)]
        ok = takes_part(q) & np.isfinite(own)
        pu = q[:, up].astype(F)
        is_ground[ok] = ((pu - own).astype(F) <= F(tol))[ok]
        fa, fb = (qa - F(0.5)).astype(F), (qb - F(0.5)).astype(F)
        a0, b0 = np.floor(fa), np.floor(fb)
        ta, tb = (fa - a0).astype(F).astype(np.float64), (fb - b0).astype(F).astype(np.float64)
        i0, i1, j0, j1 = clamp(a0, A), clamp((a0 + F(1)).astype(F), A), clamp(b0, B), clamp((b0 + F(1)).astype(F), B)
        smp = [np.where(np.isfinite(v), v, own).astype(np.float64) for v in (s[i0, j0], s[i0, j1], s[i1, j0], s[i1, j1])]
        s0, s1 = smp[0] + tb * (smp[1] - smp[0]), smp[2] + tb * (smp[3] - smp[2])
        blend = s0 + ta * (s1 - s0)
        g[ok] = blend[ok]
        h[ok] = (pu.astype(np.float64) - blend)[ok]
        big = np.maximum.reduce([np.ones(m), np.abs(pu.astype(np.float64))] + [np.abs(v) for v in smp])
        scale[ok] = big[ok]
    return h, is_ground, g, scale
