"""TEST ORACLE for csrc/scan.hip, written on its own in numpy: the surface of a tube, the first hit of a ray, the noise draw.

Two statements of the same surface:
* `cast(..., dtype=np.float64)`: the definition, solved from the scanner's own position -- no moved origin, no box rule;
* `cast(..., dtype=np.float32, kernel_order=True)`: the kernel's operation order (origin moved to the closest approach of the tube's
  midpoint, the roots through q = -(B + sign(B) sqrt(disc)), the box rule), every operation rounded to float32 by numpy.
All rays against all tubes at once ([R, M] arrays), so keep R * M modest.

Surface of tube (a, b, r1, r2): |p - (a + clip01(t) ab)| = r(clip01(t)), t = dot(p - a, ab) / dot(ab, ab): a frustum's side for
0 <= t <= 1, the sphere r1 about a where t <= 0, the sphere r2 about b where t >= 1; dot(ab, ab) == 0: the sphere r1 about a.
A tube with a non-finite value or a negative radius is never hit.  Hit of a ray: the smallest root s in [smin, smax], ties to the
lowest tube.
"""
import numpy as np

INF = np.inf


def _dot(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def _quad(A, B, C):
    """Roots of A s^2 + 2 B s + C = 0 as (q / A, C / q), q = -(B + copysign(sqrt(disc), B)); NaN where disc < 0."""
    with np.errstate(all="ignore"):
        disc = B * B - A * C
        ok = disc >= 0
        q = -(B + np.copysign(np.sqrt(np.where(ok, disc, 0)), B))
        nan = np.array(np.nan, dtype=disc.dtype)
        return np.where(ok, q / A, nan), np.where(ok, C / q, nan)


def tube_s(o, w, a, b, r1, r2, smin, smax, dtype=np.float64, kernel_order=False):
    """[R, M] in `dtype`: the smallest valid root of every ray on every tube, +inf where there is none.  o [R,3] (or [3]), w [R,3],
    smin, smax scalars or [R]."""
    T = dtype
    o = np.broadcast_to(np.asarray(o, T).reshape(-1, 3), np.asarray(w).shape)
    ox, oy, oz = (np.asarray(o[:, k], T)[:, None] for k in range(3))
    wx, wy, wz = (np.asarray(w, T)[:, k][:, None] for k in range(3))
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    with np.errstate(invalid="ignore"):
        ok_tube = np.isfinite(a).all(1) & np.isfinite(b).all(1) & np.isfinite(r1) & np.isfinite(r2) & (np.asarray(r1) >= 0) & (np.asarray(r2) >= 0)
    ax, ay, az = (a[:, k].astype(T)[None, :] for k in range(3))
    # the record is formed in float32 by the kernel (ab = b - a rounded once); the definition takes the same tube
    ab = (b - a).astype(np.float32) if kernel_order else (b.astype(T) - a.astype(T))
    bx, by, bz = (ab[:, k].astype(T)[None, :] for k in range(3))
    r1, r2 = np.asarray(r1), np.asarray(r2)  # float32 as the kernel is given them (float64 only for the grazing test's inflation)
    ra, rb = r1.astype(T)[None, :], r2.astype(T)[None, :]
    smin, smax = (np.asarray(v, T).reshape(-1, 1) for v in (smin, smax))
    with np.errstate(all="ignore"):
        ab2 = _dot(bx, by, bz, bx, by, bz)
        ww = _dot(wx, wy, wz, wx, wy, wz)
        if kernel_order:
            half = T(0.5)
            midx, midy, midz = ax + half * bx, ay + half * by, az + half * bz
            s0 = _dot(midx - ox, midy - oy, midz - oz, wx, wy, wz)
            mx, my, mz = (ox + s0 * wx) - ax, (oy + s0 * wy) - ay, (oz + s0 * wz) - az
        else:
            s0 = np.zeros((1, 1), T)
            mx, my, mz = ox - ax, oy - ay, oz - az
        rmax = np.maximum(ra, rb)
        e = rmax + T(2.0 ** -10) * (np.maximum(np.maximum(np.abs(bx), np.abs(by)), np.abs(bz)) + rmax)
        zero = ab2 == 0
        safe_ab2 = np.where(zero, T(1), ab2)
        t0 = np.where(zero, T(0), _dot(mx, my, mz, bx, by, bz) / safe_ab2)
        t1 = np.where(zero, T(0), _dot(wx, wy, wz, bx, by, bz) / safe_ab2)
        best = np.full(np.broadcast(ox, ax).shape, INF, T)

        def offer(sp, piece):
            nonlocal best
            t = t0 + sp * t1
            if piece == 0:
                t_ok = zero | (t <= 0)
            elif piece == 1:
                t_ok = ~zero & (t >= 0) & (t <= 1)
            else:
                t_ok = ~zero & (t >= 1)
            s = (s0 + sp) + T(0)
            good = t_ok & (s >= smin) & (s <= smax)
            if kernel_order:
                x, y, z = mx + sp * wx, my + sp * wy, mz + sp * wz
                for c, d in ((x, bx), (y, by), (z, bz)):
                    good &= (c >= np.minimum(T(0), d) - e) & (c <= np.maximum(T(0), d) + e)
            best = np.where(good & (s < best), s, best)

        for root in _quad(ww + 0 * ab2, _dot(mx, my, mz, wx, wy, wz), _dot(mx, my, mz, mx, my, mz) - ra * ra):
            offer(root, 0)
        nx, ny, nz = mx - bx, my - by, mz - bz
        for root in _quad(ww + 0 * ab2, _dot(nx, ny, nz, wx, wy, wz), _dot(nx, ny, nz, nx, ny, nz) - rb * rb):
            offer(root, 2)
        px, py, pz = mx - t0 * bx, my - t0 * by, mz - t0 * bz
        qx, qy, qz = wx - t1 * bx, wy - t1 * by, wz - t1 * bz
        dr = rb - ra
        R = ra + t0 * dr
        D = t1 * dr
        for root in _quad(_dot(qx, qy, qz, qx, qy, qz) - D * D, _dot(px, py, pz, qx, qy, qz) - R * D, _dot(px, py, pz, px, py, pz) - R * R):
            offer(root, 1)
    best[:, ~ok_tube] = INF
    return best


def cast(o, w, a, b, r1, r2, smin, smax, dtype=np.float64, kernel_order=False, inflate=0.0):
    """dict(range [R] (+inf: no hit), tube [R] (-1), second [R]: the runner-up tube's s (+inf)).  `inflate`: radii r -> r + inflate *
    (1e-4 r + 1e-6) first (float64 only; for the grazing test)."""
    r1, r2 = np.asarray(r1, np.float32), np.asarray(r2, np.float32)
    if inflate:
        with np.errstate(invalid="ignore"):
            r1 = np.where(r1 >= 0, np.maximum(r1.astype(np.float64) + inflate * (1e-4 * r1 + 1e-6), 0), r1)
            r2 = np.where(r2 >= 0, np.maximum(r2.astype(np.float64) + inflate * (1e-4 * r2 + 1e-6), 0), r2)
        s = tube_s(o, w, a, b, r1, r2, smin, smax)
    else:
        s = tube_s(o, w, a, b, r1, r2, smin, smax, dtype, kernel_order)
    R, M = s.shape
    if M == 0:
        return {"range": np.full(R, INF, dtype), "tube": np.full(R, -1, np.int32), "second": np.full(R, INF, dtype)}
    tube = np.argmin(s, axis=1)  # the first minimum: ties to the lowest tube
    rng = s[np.arange(R), tube]
    rest = s.copy()
    rest[np.arange(R), tube] = INF
    return {"range": rng, "tube": np.where(np.isfinite(rng), tube, -1).astype(np.int32), "second": rest.min(axis=1)}


def grazing(o, w, a, b, r1, r2, smin, smax, base=None):
    """[R] bool: rays whose float64 outcome changes under radii inflated or deflated by 1e-4 r + 1e-6 m: hit against miss, or a
    range moved by more than 1 mm."""
    base = cast(o, w, a, b, r1, r2, smin, smax) if base is None else base
    out = np.zeros(len(base["range"]), bool)
    for sign in (1.0, -1.0):
        other = cast(o, w, a, b, r1, r2, smin, smax, inflate=sign)
        h0, h1 = np.isfinite(base["range"]), np.isfinite(other["range"])
        with np.errstate(invalid="ignore"):
            out |= (h0 != h1) | (h0 & h1 & (np.abs(base["range"] - other["range"]) > 1e-3))
    return out


def directions(az, el, position=None):
    """float64 [n_az * n_el, 3]: the beams of a window az = (start, step, count), el likewise, whose parameters are rounded to
    float32 first (what the kernel is given), ray k = i * n_el + j."""
    f = lambda v: float(np.float32(v))
    i, j = np.meshgrid(np.arange(int(az[2])), np.arange(int(el[2])), indexing="ij")
    a = f(az[0]) + i.reshape(-1) * f(az[1])
    e = f(el[0]) + j.reshape(-1) * f(el[1])
    return np.stack([np.cos(e) * np.cos(a), np.cos(e) * np.sin(a), np.sin(e)], axis=1)


def pair(p, a, b, r1, r2, dtype=np.float64):
    """st_tube.h's pair of points p [n,3] with their own tubes (rows of a, b, r1, r2 [n]): (vector q - p [n,3], residual [n]);
    t = 0 for a zero-length tube."""
    T = dtype
    p, a = np.asarray(p, T), np.asarray(a, np.float32).astype(T)
    ab = (np.asarray(b, np.float32) - np.asarray(a, np.float32)).astype(T) if T is np.float32 else np.asarray(b, np.float32).astype(T) - a
    ab2 = _dot(ab[:, 0], ab[:, 1], ab[:, 2], ab[:, 0], ab[:, 1], ab[:, 2])
    d = p - a
    with np.errstate(all="ignore"):
        t = np.where(ab2 == 0, T(0), np.clip(_dot(d[:, 0], d[:, 1], d[:, 2], ab[:, 0], ab[:, 1], ab[:, 2]) / np.where(ab2 == 0, T(1), ab2), 0, 1))
    q = a + t[:, None] * ab
    v = q - p
    r = (T(1) - t) * np.asarray(r1, np.float32).astype(T) + t * np.asarray(r2, np.float32).astype(T)
    return v, np.sqrt(_dot(v[:, 0], v[:, 1], v[:, 2], v[:, 0], v[:, 1], v[:, 2])) - r


def philox_normal(k, seed, dtype=np.float64):
    """The first Box-Muller normal of words 0, 1 of Philox4x32-10, key = seed (low, high), counter = (k, 0, 0, 0), k [n]."""
    mask = np.uint64(0xFFFFFFFF)
    c = [np.asarray(k, np.uint64) & mask] + [np.zeros(len(k), np.uint64) for _ in range(3)]
    seed = int(seed) & ((1 << 64) - 1)
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & mask, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & mask]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & mask, (k1 + np.uint64(0xBB67AE85)) & mask
    T = dtype
    u1 = ((c[0] >> np.uint64(8)) + np.uint64(1)).astype(T) * T(2.0 ** -24)
    u2 = ((c[1] >> np.uint64(8)) + np.uint64(1)).astype(T) * T(2.0 ** -24)
    return np.sqrt(T(-2.0) * np.log(u1)) * np.cos(T(2.0 * np.pi) * u2)
