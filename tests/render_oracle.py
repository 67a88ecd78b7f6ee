"""numpy restatement of the renderer (csrc/render.hip).  Every function takes `dtype`: np.float64 is the oracle, np.float32 mirrors the
kernels' float32 order of operations (numpy rounds a float32 expression once per operation, no contraction).  Both take the float32
inputs the kernels take.

Definitions (stated here once; the header comment of render.hip says the same):
  camera     row of 16: R (9, row-major), t (3), fx, fy, cx, cy.  xc = ((R00 px + R01 py) + R02 pz) + tx, yc, zc likewise.
             Culled: !(zc > near) or a non-finite coordinate.  u = (fx xc)/zc + cx, v = (fy yc)/zc + cy.  Pixel centres are integers.
  point      nearest pixel (floor(u + 0.5), floor(v + 0.5)); with rp = max(point_px/2, (fx r)/zc) > 0.5 (and rp rp within float32)
             also the pixel centres of [ceil(u-rp), floor(u+rp)] x [ceil(v-rp), floor(v+rp)] with dx dx + dy dy <= rp rp.  Depth zc.
  segment    ends clipped to z = near (radius interpolated), projected with pixel radii max((fx r)/z, min_px/2); for a pixel centre q:
             s = clamp(dot(q-a', b'-a')/|b'-a'|^2, 0, 1) (0 if degenerate), d = |q - (a' + s(b'-a'))|, rp = pa + s(pb-pa), covered iff
             d <= rp, depth = max(near, zx (1 - (rp/fx) sqrt(max(0, 1 - (d/rp)^2)))) with 1/zx = (1-s)/za + s/zb.
  frame      per pixel the smallest (depth, id); ids count through the items in order.  Background: depth +inf, id -1, white.
  colour     uniform | float rgb | class through cmap (outside: black) | scalar through the 5-stop ramp | int id through st_hash64.
  shading    shade = exp(-strength sum_nb max(0, log2 z - log2 z_nb)) over (x-e, x+e, y-e, y+e) inside the image and not background.
  byte       floor(clamp(c, 0, 1) 255 + 0.5).
"""
import numpy as np

FLT_MAX = float(np.finfo(np.float32).max)
UNIFORM, RGB, CLASS, SCALAR, ID = 0, 1, 2, 3, 4
RAMP = np.array([[0, 0, 1], [0, 1, 1], [0, 1, 0], [1, 1, 0], [1, 0, 0]], dtype=np.float64)


def _finite(x):
    with np.errstate(invalid="ignore"):
        return np.abs(x) <= FLT_MAX


def to_camera(cam, xyz, f):
    """Camera-space coordinates (dtype f) of float32 points under one camera row (float32 [16])."""
    c = np.asarray(cam, dtype=np.float32).astype(f)
    p = np.asarray(xyz, dtype=np.float32).reshape(-1, 3).astype(f)
    with np.errstate(all="ignore"):
        out = [((c[3 * r] * p[:, 0] + c[3 * r + 1] * p[:, 1]) + c[3 * r + 2] * p[:, 2]) + c[9 + r] for r in range(3)]
    assert all(o.dtype == f for o in out)
    return out


def project_points(cam, xyz, near, f):
    """(u, v, zc, ok) of every point; ok = drawn (not culled before the viewport test)."""
    c = np.asarray(cam, dtype=np.float32).astype(f)
    xc, yc, zc = to_camera(cam, xyz, f)
    with np.errstate(all="ignore"):
        ok = (zc > f(np.float32(near))) & _finite(xc) & _finite(yc) & _finite(zc)
        u = (c[12] * xc) / zc + c[14]
        v = (c[13] * yc) / zc + c[15]
        ok &= _finite(u) & _finite(v)
    return u, v, zc, ok


def point_radius_px(cam, zc, radius, point_px, f):
    c = np.asarray(cam, dtype=np.float32).astype(f)
    half = f(np.float32(point_px)) * f(0.5)
    if radius is None:
        return np.full(zc.shape, half, dtype=f)
    with np.errstate(all="ignore"):
        return np.fmax(half, (c[12] * np.asarray(radius, dtype=np.float32).astype(f)) / zc)


def point_candidates(cam, xyz, radius, point_px, H, W, near, f):
    """Every (pixel, depth, point) a point cloud offers to one view, and per point its margin: the distance in pixels to the nearest
    decision boundary (a pixel boundary for the nearest-pixel rule, a disc's edge for every pixel centre around it)."""
    u, v, zc, ok = project_points(cam, xyz, near, f)
    n = u.shape[0]
    rp = point_radius_px(cam, zc, radius, point_px, f)
    u, v, rp = (np.where(ok, a, f(0)) for a in (u, v, rp))
    bu, bv = np.floor(u + f(0.5)), np.floor(v + f(0.5))
    margin = np.full(n, np.inf)
    fr = lambda a: np.abs((a + f(0.5)) - np.round(a + f(0.5))).astype(np.float64)
    margin[ok] = np.minimum(fr(u), fr(v))[ok]
    with np.errstate(all="ignore"):
        disc = ok & (rp > f(0.5)) & _finite(rp * rp)  # a radius whose square leaves float32 draws no disc
    reach = int(min(np.ceil(rp[disc].max()) + 1, max(H, W))) if disc.any() else 0
    x0, x1, y0, y1 = np.ceil(u - rp), np.floor(u + rp), np.ceil(v - rp), np.floor(v + rp)
    pix, dep, idx = [], [], []
    for oy in range(-reach, reach + 1):
        for ox in range(-reach, reach + 1):
            i, j = bu + f(ox), bv + f(oy)
            dx, dy = i - u, j - v
            d2 = dx * dx + dy * dy
            cov = disc & (i >= x0) & (i <= x1) & (j >= y0) & (j <= y1) & (d2 <= rp * rp)
            if ox == 0 and oy == 0:
                cov = ok.copy()
            else:
                edge = np.abs(np.sqrt(d2.astype(np.float64)) - rp.astype(np.float64))
                margin[disc] = np.minimum(margin[disc], edge[disc])
            cov &= (i >= 0) & (i < W) & (j >= 0) & (j < H)
            k = np.flatnonzero(cov)
            pix.append(j[k].astype(np.int64) * W + i[k].astype(np.int64))
            dep.append(zc[k])
            idx.append(k)
    cat = lambda parts, dt: np.concatenate(parts) if parts else np.zeros(0, dt)
    return cat(pix, np.int64), cat(dep, f), cat(idx, np.int64), margin


def segment_setup(cam, a, b, r1, r2, min_px, H, W, near, f):
    """Clipped, projected ends of every segment under one camera: dict of arrays (dtype f) and `ok`."""
    c = np.asarray(cam, dtype=np.float32).astype(f)
    nr = f(np.float32(near))
    xa, ya, za = to_camera(cam, a, f)
    xb, yb, zb = to_camera(cam, b, f)
    ra, rb = (np.asarray(r, dtype=np.float32).reshape(-1).astype(f) for r in (r1, r2))
    with np.errstate(all="ignore"):
        ok = np.ones(xa.shape[0], dtype=bool)
        for x in (xa, ya, za, xb, yb, zb, ra, rb):
            ok &= _finite(x)
        a_in, b_in = za > nr, zb > nr
        ok &= a_in | b_in
        ta = (nr - za) / (zb - za)
        tb = (nr - zb) / (za - zb)
        ca, cb = ok & ~a_in, ok & a_in & ~b_in
        xa2, ya2, ra2, za2 = (np.where(ca, p + ta * (q - p), p) for p, q in ((xa, xb), (ya, yb), (ra, rb), (za, zb)))
        za2 = np.where(ca, nr, za2)
        xb2, yb2, rb2, zb2 = (np.where(cb, p + tb * (q - p), p) for p, q in ((xb, xa), (yb, ya), (rb, ra), (zb, za)))
        zb2 = np.where(cb, nr, zb2)
        half = f(np.float32(min_px)) * f(0.5)
        S = dict(ua=(c[12] * xa2) / za2 + c[14], va=(c[13] * ya2) / za2 + c[15], ub=(c[12] * xb2) / zb2 + c[14],
                 vb=(c[13] * yb2) / zb2 + c[15], pa=np.fmax((c[12] * ra2) / za2, half), pb=np.fmax((c[12] * rb2) / zb2, half), za=za2, zb=zb2)
        for k in ("ua", "va", "ub", "vb", "pa", "pb"):
            ok &= _finite(S[k])
        for k in S:
            S[k] = np.where(ok, S[k], f(1))
        S["x0"] = np.fmax(np.ceil(np.fmin(S["ua"] - S["pa"], S["ub"] - S["pb"])), f(0))
        S["x1"] = np.fmin(np.floor(np.fmax(S["ua"] + S["pa"], S["ub"] + S["pb"])), f(W - 1))
        S["y0"] = np.fmax(np.ceil(np.fmin(S["va"] - S["pa"], S["vb"] - S["pb"])), f(0))
        S["y1"] = np.fmin(np.floor(np.fmax(S["va"] + S["pa"], S["vb"] + S["pb"])), f(H - 1))
        ok &= (S["x0"] <= S["x1"]) & (S["y0"] <= S["y1"])
    S["ok"], S["fx"], S["near"], S["H"], S["W"] = ok, c[12], nr, H, W
    assert all(S[k].dtype == f for k in ("ua", "pa", "za", "x0"))
    return S


def segment_pixels(S, k, f):
    """Segment k over its clipped box: (pixel x, pixel y, covered, depth, |d - rp|) as flat arrays."""
    x0, x1, y0, y1 = (int(S[n][k]) for n in ("x0", "x1", "y0", "y1"))
    if f == np.float64:  # one pixel more on every side (inside the viewport): the float32 box may round the other way, and such a
        x0, y0, x1, y1 = max(x0 - 1, 0), max(y0 - 1, 0), min(x1 + 1, S["W"] - 1), min(y1 + 1, S["H"] - 1)  # pixel must count as an edge
    yy, xx = np.mgrid[y0:y1 + 1, x0:x1 + 1]
    xx, yy = xx.reshape(-1), yy.reshape(-1)
    qx, qy = xx.astype(f), yy.astype(f)
    ua, va, ub, vb, pa, pb, za, zb = (S[n][k] for n in ("ua", "va", "ub", "vb", "pa", "pb", "za", "zb"))
    with np.errstate(all="ignore"):
        ex, ey = ub - ua, vb - va
        l2 = ex * ex + ey * ey
        s = np.zeros(qx.shape, dtype=f)
        if l2 > 0:
            s = ((qx - ua) * ex + (qy - va) * ey) / l2
            s = np.where(s > 0, np.where(s < 1, s, f(1)), f(0))
        dx, dy = qx - (ua + s * ex), qy - (va + s * ey)
        d = np.sqrt(dx * dx + dy * dy)
        rp = pa + s * (pb - pa)
        cov = d <= rp
        zx = f(1) / ((f(1) - s) / za + s / zb)
        kk = np.where(rp > 0, d / np.where(rp > 0, rp, f(1)), f(0))
        depth = np.fmax(S["near"], zx * (f(1) - (rp / S["fx"]) * np.sqrt(np.fmax(f(0), f(1) - kk * kk))))
        cov &= depth <= FLT_MAX
    assert depth.dtype == f and s.dtype == f
    return xx, yy, cov, depth, np.abs(d.astype(np.float64) - rp.astype(np.float64))


def render(items, cams, H, W, near=0.01, point_px=1.0, min_px=1.0, dtype=np.float64, detail=False):
    """The frame: {"depth": dtype [V,H,W] (+inf background), "ids": int32 [V,H,W] (-1)}.  items: dicts with kind "points" (xyz,
    optional radius) or "segments" (a, b, r1, r2), plus their colour source for `resolve`.  detail=True adds "runner" (the smallest
    depth offered by ANOTHER id, +inf if none) and "edge" (bool: some segment's coverage boundary passes within 1e-3 px)."""
    f = dtype
    cams = np.asarray(cams, dtype=np.float32).reshape(-1, 16)
    V = cams.shape[0]
    depth = np.full((V, H * W), np.inf, dtype=f)
    ids = np.full((V, H * W), -1, dtype=np.int64)
    runner = np.full((V, H * W), np.inf, dtype=f)
    edge = np.zeros((V, H * W), dtype=bool)

    def offer(v, pix, dep, idn):
        """Merge candidates (one id per pixel at most within a call is NOT assumed)."""
        order = np.lexsort((idn, dep, pix))
        pix, dep, idn = pix[order], dep[order], idn[order]
        first = np.ones(pix.shape[0], dtype=bool)
        first[1:] = pix[1:] != pix[:-1]
        if detail and pix.shape[0]:
            second = ~first
            second[1:] &= first[:-1]  # the second entry of a pixel's run: its smallest depth of another candidate
            other = np.full(H * W, np.inf, dtype=f)
            other[pix[second]] = dep[second]
        p, d, i = pix[first], dep[first], idn[first]
        cur_d, cur_i = depth[v, p], ids[v, p]
        win = (d < cur_d) | ((d == cur_d) & ((cur_i < 0) | (i < cur_i)))
        if detail and pix.shape[0]:
            loser = np.where(win, cur_d, d)  # whoever loses the pixel may be the new runner-up
            runner[v, p] = np.minimum(runner[v, p], loser)
            runner[v] = np.minimum(runner[v], other)
        depth[v, p[win]], ids[v, p[win]] = d[win], i[win]

    base = 0
    for it in items:
        if it["kind"] == "points":
            n = np.asarray(it["xyz"]).reshape(-1, 3).shape[0]
            for v in range(V):
                pix, dep, idx, _ = point_candidates(cams[v], it["xyz"], it.get("radius"), point_px, H, W, near, f)
                offer(v, pix, dep, idx + base)
        else:
            n = np.asarray(it["a"]).reshape(-1, 3).shape[0]
            for v in range(V):
                S = segment_setup(cams[v], it["a"], it["b"], it["r1"], it["r2"], min_px, H, W, near, f)
                for k in np.flatnonzero(S["ok"]):
                    xx, yy, cov, dep, gap = segment_pixels(S, k, f)
                    pix = yy.astype(np.int64) * W + xx
                    edge[v, pix[gap < 1e-3]] = True
                    offer(v, pix[cov], dep[cov], np.full(int(cov.sum()), base + k, dtype=np.int64))
        base += n
    out = {"depth": depth.reshape(V, H, W), "ids": ids.reshape(V, H, W).astype(np.int32)}
    if detail:
        out["runner"], out["edge"] = runner.reshape(V, H, W), edge.reshape(V, H, W)
    return out


def hash64(k):
    k = np.asarray(k, dtype=np.uint64)
    with np.errstate(over="ignore"):
        k = k ^ (k >> np.uint64(33))
        k = k * np.uint64(0xFF51AFD7ED558CCD)
        k = k ^ (k >> np.uint64(33))
        k = k * np.uint64(0xC4CEB9FE1A85EC53)
        k = k ^ (k >> np.uint64(33))
    return k


def item_colours(it, f):
    """float colours [n,3] (dtype f) of an item's ids."""
    n = np.asarray(it["xyz"] if it["kind"] == "points" else it["a"]).reshape(-1, 3).shape[0]
    mode = it.get("mode", UNIFORM)
    if mode == UNIFORM:
        return np.tile(np.asarray(it.get("rgb", (0, 0, 0)), dtype=np.float32).astype(f), (n, 1))
    if mode == RGB:
        return np.asarray(it["data"], dtype=np.float32).reshape(-1, 3).astype(f)
    if mode == CLASS:
        cm = np.asarray(it["cmap"], dtype=np.float32).reshape(-1, 3).astype(f)
        cl = np.asarray(it["data"]).astype(np.int64).reshape(-1)
        inside = (cl >= 0) & (cl < cm.shape[0])
        return np.where(inside[:, None], cm[np.where(inside, cl, 0)], f(0))
    if mode == SCALAR:
        x = np.asarray(it["data"], dtype=np.float32).reshape(-1).astype(f)
        lo, hi = f(np.float32(it["lo"])), f(np.float32(it["hi"]))
        with np.errstate(all="ignore"):
            t = (x - lo) / (hi - lo)
            t = np.where(t > 0, np.where(t < 1, t, f(1)), f(0))
        x4 = t * f(4)
        s = np.minimum(x4.astype(np.int64), 3)
        fr = x4 - s.astype(f)
        stop = RAMP.astype(f)
        return stop[s] + fr[:, None] * (stop[s + 1] - stop[s])
    if mode == ID:
        h = hash64(np.asarray(it["data"]).astype(np.int64).reshape(-1).astype(np.uint64) + np.uint64(1))
        byte = lambda sh: (np.uint64(64) + ((h >> np.uint64(sh)) & np.uint64(127))).astype(f) / f(255)
        return np.stack([byte(8), byte(24), byte(40)], axis=1)
    raise ValueError(mode)


def to8(c, f):
    with np.errstate(invalid="ignore"):
        c = np.where(c > 0, np.where(c < 1, c, f(1)), f(0))
    return np.floor(c * f(255) + f(0.5)).astype(np.uint8)


def _shift(a, dy, dx, fill):
    """b[v, y, x] = a[v, y + dy, x + dx], `fill` outside the image."""
    out = np.full_like(a, fill)
    H, W = a.shape[1:3]
    y0, y1, x0, x1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
    if y0 < y1 and x0 < x1:
        out[:, y0:y1, x0:x1] = a[:, y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return out


def resolve(frame, items, edl_strength=0.0, edl_px=1, dtype=np.float64, unrounded=False):
    """uint8 [V,H,W,3] of a frame of `render` (same dtype).  unrounded=True: the float channel values before `to8` instead."""
    f = dtype
    depth, ids = frame["depth"].astype(f), frame["ids"]
    V, H, W = ids.shape
    table = np.concatenate([item_colours(it, f) for it in items] or [np.zeros((0, 3), dtype=f)])
    hit = ids >= 0
    col = np.ones((V, H, W, 3), dtype=f)
    col[hit] = table[ids[hit]]
    if edl_strength > 0:
        e = int(edl_px)
        with np.errstate(all="ignore"):
            lz = np.log2(np.where(hit, depth, f(1)))
        acc = np.zeros((V, H, W), dtype=f)
        for dy, dx in ((0, -e), (0, e), (-e, 0), (e, 0)):  # a neighbour outside the image or on the background adds nothing
            acc = acc + np.where(_shift(hit, dy, dx, False), np.fmax(f(0), lz - _shift(lz, dy, dx, f(0))), f(0))
        shade = np.exp(-f(np.float32(edl_strength)) * acc)
        col = np.where(hit[..., None], col * shade[..., None], col)
    assert col.dtype == f
    if unrounded:
        return col
    out = to8(col, f)
    out[~hit] = 255
    return out
