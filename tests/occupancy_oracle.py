"""Numpy oracle of the beam tally (csrc/occupancy.hip).  Two statements of the same thing:

`walk32`: the kernel's walk restated in float32, operation for operation (the head of csrc/occupancy.hip), vectorised over the beams
with one numpy step per cell of the walk.  The kernel must give these very integers.

`brute64`: an independent float64 statement by brute force -- a slab test of every beam against every cell, no walk, no grid
traversal, no tie rule -- from which two-sided bounds on the tallies follow (tau = 1e-4 cell):
  enter_strict / enter_loose: beams whose free chord in the cell exceeds tau / whose free part [0, f] comes within tau (Euclidean)
    of the cell's box;
  behind_loose: returns whose part beyond the return, [f, inf), comes within tau of the box; behind_strict: those whose chord
    beyond the return exceeds tau AND whose free part does not come within tau of the box (a cell the free part reaches holds, or
    touches, the return: it is the hit cell or its neighbour across a face, and the hit cell gets no `behind`);
  chord: the float64 free chord per beam and cell; free_total: the free length inside the grid's box.
"""
import numpy as np

F = np.float32
INF32 = F(np.inf)
FLT_MAX = F(3.4028234e38)


def _arrays(origins, origin_idx, dir, rng):
    return (np.asarray(origins, F).reshape(-1, 3), np.asarray(origin_idx, np.int64).reshape(-1), np.asarray(dir, F).reshape(-1, 3),
            np.asarray(rng, F).reshape(-1))


def good_beams(origins, origin_idx, dir, rng):
    """(good [R] bool, o [R,3] float32): the kernel's BAD rule."""
    S = len(origins)
    idx_ok = (origin_idx >= 0) & (origin_idx < S)
    o = origins[np.where(idx_ok, origin_idx, 0)] if S else np.zeros((len(rng), 3), F)
    with np.errstate(invalid="ignore", over="ignore"):
        xx, yy, zz = dir[:, 0] * dir[:, 0], dir[:, 1] * dir[:, 1], dir[:, 2] * dir[:, 2]
        ww = xx + yy
        ww = ww + zz
        good = idx_ok & np.isfinite(o).all(1) & np.isfinite(dir).all(1) & (rng >= 0) & (ww >= F(0.998)) & (ww <= F(1.002))
    return good, o


def _axis32(v, lo, cell, dim):
    with np.errstate(invalid="ignore", over="ignore"):
        c = v - lo
        c = c / cell
        c = np.floor(c)
        c = np.fmin(np.fmax(c, F(0)), F(dim - 1))
    return c.astype(np.int64)


def _exit32(i, lo, cell, o, w):
    plane = np.where(w > 0, i + 1, i).astype(F) * cell
    plane = lo + plane
    plane = plane - o
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        e = plane / w
    return np.where(w == 0, INF32, e).astype(F)


def q32(d, cell):
    with np.errstate(over="ignore"):
        t = np.fmax(d, F(0))
        t = t / cell
        t = t * F(65536.0)
        t = np.fmin(t, F(4294967296.0))
    return np.rint(t).astype(np.uint64)


def walk32(origins, origin_idx, dir, rng, lo, cell, dim, max_range=np.inf, behind=True):
    """The kernel's integers for one grid: enter, hit, behind (uint32, shaped dim), path (uint64), hit_cell [R] int32, n_bad,
    n_outside."""
    origins, origin_idx, dir, rng = _arrays(origins, origin_idx, dir, rng)
    lo, cell, max_range = np.asarray(lo, F).reshape(3), F(cell), F(max_range)
    dx, dy, dz = (int(d) for d in dim)
    n, R = dx * dy * dz, len(rng)
    tally = {k: np.zeros(n, np.uint64) for k in ("enter", "hit", "behind", "path")}
    hit_cell = np.full(R, -1, np.int32)
    good, o_all = good_beams(origins, origin_idx, dir, rng)
    rows = np.flatnonzero(good)
    o, w, r = o_all[rows], dir[rows], rng[rows]
    hi = lo + np.asarray([dx, dy, dz], F) * cell
    sa, sb, inside = np.zeros(len(rows), F), np.full(len(rows), INF32), np.ones(len(rows), bool)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for k in range(3):
            zero = w[:, k] == 0
            inside &= ~zero | ((o[:, k] >= lo[k]) & (o[:, k] <= hi[k]))
            u, v = lo[k] - o[:, k], hi[k] - o[:, k]
            u = u / w[:, k]
            v = v / w[:, k]
            sa = np.where(zero, sa, np.fmax(sa, np.fmin(u, v)))
            sb = np.where(zero, sb, np.fmin(sb, np.fmax(u, v)))
        touch = inside & (sa <= sb) & (sa <= FLT_MAX)
        ret = (r <= FLT_MAX) & (r <= max_range)
        f = np.fmin(r, max_range)
        early = f < sa
        active = touch & ~(early & (~ret | (not behind)))
        free = ~early
        p = sa[:, None] * w
        p = o + p
    ix, iy, iz = (_axis32(p[:, k], lo[k], cell, d) for k, d in enumerate((dx, dy, dz)))
    s_in, steps = sa.copy(), 0
    while active.any():
        a = np.flatnonzero(active)
        ex = _exit32(ix[a], lo[0], cell, o[a, 0], w[a, 0])
        ey = _exit32(iy[a], lo[1], cell, o[a, 1], w[a, 1])
        ez = _exit32(iz[a], lo[2], cell, o[a, 2], w[a, 2])
        out = np.fmin(np.fmin(ex, ey), ez)
        e = np.fmin(out, sb[a])
        c = (ix[a] * dy + iy[a]) * dz + iz[a]
        fr = free[a]
        with np.errstate(invalid="ignore"):
            m = np.fmin(e, f[a])
            d = m - s_in[a]
        q = q32(d, cell)
        np.add.at(tally["enter"], c[fr], 1)
        np.add.at(tally["path"], c[fr], q[fr])
        np.add.at(tally["behind"], c[~fr], 1)
        stop = fr & (f[a] <= e)
        h = stop & ret[a]
        np.add.at(tally["hit"], c[h], 1)
        hit_cell[rows[a[h]]] = c[h]
        free[a[h]] = False
        alive = ~(stop & ~ret[a]) & ~(h & (not behind)) & (out < sb[a])
        sx = ex == out
        sy = ~sx & (ey == out)
        sz = ~sx & ~sy
        ix[a] += np.where(alive & sx, np.where(w[a, 0] > 0, 1, -1), 0)
        iy[a] += np.where(alive & sy, np.where(w[a, 1] > 0, 1, -1), 0)
        iz[a] += np.where(alive & sz, np.where(w[a, 2] > 0, 1, -1), 0)
        alive &= (ix[a] >= 0) & (ix[a] < dx) & (iy[a] >= 0) & (iy[a] < dy) & (iz[a] >= 0) & (iz[a] < dz)
        s_in[a] = out
        steps += 1
        alive &= steps <= dx + dy + dz
        active[a] = alive
    shape = (dx, dy, dz)
    return {"enter": tally["enter"].astype(np.uint32).reshape(shape), "hit": tally["hit"].astype(np.uint32).reshape(shape),
            "behind": tally["behind"].astype(np.uint32).reshape(shape), "path": tally["path"].reshape(shape), "hit_cell": hit_cell,
            "n_bad": int((~good).sum()), "n_outside": int((~touch).sum())}


def walk32_grids(origins, origin_idx, dir, rng, grids, beam_off, max_range=np.inf, behind=True):
    """`walk32` per grid of a call: a list of results, and the call's two counters summed."""
    origins, origin_idx, dir, rng = _arrays(origins, origin_idx, dir, rng)
    out = [walk32(origins, origin_idx[b0:b1], dir[b0:b1], rng[b0:b1], lo, cell, dim, max_range, behind)
           for (lo, cell, dim), b0, b1 in zip(grids, beam_off[:-1], beam_off[1:])]
    return out, sum(o["n_bad"] for o in out), sum(o["n_outside"] for o in out)


# ------------------------------------------------------------------------------------------------------- float64 ---
def _intervals(o, w, lo_planes, hi_planes):
    """[R, n] parameter intervals of the lines o + s w inside the slabs [lo_planes[j], hi_planes[j]] of one axis."""
    o, w = o[:, None], w[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        u, v = (lo_planes[None] - o) / w, (hi_planes[None] - o) / w
    t0, t1 = np.minimum(u, v), np.maximum(u, v)
    zero = w == 0
    within = (o >= lo_planes[None]) & (o <= hi_planes[None])
    t0 = np.where(zero, np.where(within, -np.inf, np.inf), t0)
    t1 = np.where(zero, np.where(within, np.inf, -np.inf), t1)
    return t0, t1


def _cells(o, w, lo, cell, dim, pad):
    """[R, n_cells] interval of every line in every cell's box inflated by `pad` on every side."""
    per = []
    for k in range(3):
        planes = lo[k] + np.arange(dim[k] + 1, dtype=np.float64) * cell
        per.append(_intervals(o[:, k], w[:, k], planes[:-1] - pad, planes[1:] + pad))
    R = len(o)
    t0 = np.maximum(np.maximum(per[0][0][:, :, None, None], per[1][0][:, None, :, None]), per[2][0][:, None, None, :])
    t1 = np.minimum(np.minimum(per[0][1][:, :, None, None], per[1][1][:, None, :, None]), per[2][1][:, None, None, :])
    return t0.reshape(R, -1), t1.reshape(R, -1)


def box_distance(p, blo, bhi):
    """Euclidean distance of points [.,3] from boxes [.,3]."""
    return np.linalg.norm(np.maximum(np.maximum(blo - p, p - bhi), 0.0), axis=-1)


def cell_box(c, lo, cell, dim):
    """(lo, hi) float64 [.,3] of cells by index."""
    c = np.asarray(c, np.int64)
    ijk = np.stack([c // (dim[1] * dim[2]), (c // dim[2]) % dim[1], c % dim[2]], axis=-1).astype(np.float64)
    blo = np.asarray(lo, np.float64) + ijk * float(cell)
    return blo, blo + float(cell)


def _near(o, w, s0, s1, blo, bhi, tau):
    """Does the piece [s0, s1] of each line come within tau of its box?  The distance from a convex set is convex along a line:
    a golden-section search, then the end points as well."""
    a, b = s0.copy(), np.minimum(s1, s0 + 1e9)  # (a piece that runs to infinity: the box is far nearer than that)
    g = (np.sqrt(5.0) - 1.0) / 2.0
    dist = lambda s: box_distance(o + s[:, None] * w, blo, bhi)
    best = np.minimum(dist(a), dist(b))
    for _ in range(120):
        c, d = b - g * (b - a), a + g * (b - a)
        fc, fd = dist(c), dist(d)
        left = fc < fd
        b, a = np.where(left, d, b), np.where(left, a, c)
        best = np.minimum(best, np.minimum(fc, fd))
    return best <= tau


def brute64(origins, origin_idx, dir, rng, lo, cell, dim, max_range=np.inf, tau=None):
    """The float64 statement (behind counted: the `behind` flag on).  Bad beams take no part."""
    origins, origin_idx, dir, rng = _arrays(origins, origin_idx, dir, rng)
    good, o32 = good_beams(origins, origin_idx, dir, rng)
    lo, cell = np.asarray(lo, F).astype(np.float64), float(F(cell))
    dim = tuple(int(d) for d in dim)
    tau = 1e-4 * cell if tau is None else tau
    rows = np.flatnonzero(good)
    o, w, r = o32[rows].astype(np.float64), dir[rows].astype(np.float64), rng[rows].astype(np.float64)
    ret = np.isfinite(r) & (r <= max_range)
    f = np.minimum(r, float(max_range))
    n = dim[0] * dim[1] * dim[2]
    t0, t1 = _cells(o, w, lo, cell, dim, 0.0)
    fcol = f[:, None]
    chord = np.maximum(np.minimum(t1, fcol) - np.maximum(t0, 0.0), 0.0)
    chord = np.where(t1 >= t0, chord, 0.0)
    chord_behind = np.where(ret[:, None] & (t1 >= t0), np.maximum(t1 - np.maximum(np.maximum(t0, 0.0), fcol), 0.0), 0.0)
    i0, i1 = _cells(o, w, lo, cell, dim, tau)
    blo_all, bhi_all = cell_box(np.arange(n), lo, cell, dim)

    def loose(s0, s1, sure):
        """pairs whose piece [s0, s1] comes within tau of the cell: `sure` ones at once, the other candidates by search"""
        cand = (s1 >= s0) & ~sure
        b, c = np.nonzero(cand)
        out = sure.copy()
        if len(b):
            out[b, c] = _near(o[b], w[b], s0[b, c], s1[b, c], blo_all[c], bhi_all[c], tau)
        return out

    free_lo, free_hi = np.maximum(i0, 0.0), np.minimum(i1, fcol)
    enter_loose = loose(free_lo, free_hi, chord > 0.0)
    beh_lo = np.maximum(np.maximum(i0, 0.0), fcol)
    behind_loose = loose(np.where(ret[:, None], beh_lo, np.inf), np.where(ret[:, None], i1, -np.inf), chord_behind > 0.0)
    behind_strict = (chord_behind > tau) & ~enter_loose
    # the grid's box
    per = [_intervals(o[:, k], w[:, k], np.asarray([lo[k]]), np.asarray([lo[k] + dim[k] * cell])) for k in range(3)]
    ta = np.maximum(np.maximum(per[0][0], per[1][0]), per[2][0])[:, 0]
    tb = np.minimum(np.minimum(per[0][1], per[1][1]), per[2][1])[:, 0]
    free_len = np.where(tb >= ta, np.maximum(np.minimum(tb, f) - np.maximum(ta, 0.0), 0.0), 0.0)
    with np.errstate(invalid="ignore"):
        point = o + np.where(ret, r, 0.0)[:, None] * w
    shape = dim
    return {"rows": rows, "ret": ret, "point": point, "chord": chord, "tau": tau,
            "enter_strict": (chord > tau).sum(0).reshape(shape), "enter_loose": enter_loose.sum(0).reshape(shape),
            "behind_strict": behind_strict.sum(0).reshape(shape), "behind_loose": behind_loose.sum(0).reshape(shape),
            "chord_sum": chord.sum(0).reshape(shape), "free_total": float(free_len.sum()),
            "grid_lo": lo, "grid_hi": lo + np.asarray(dim, np.float64) * cell}
