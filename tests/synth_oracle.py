"""TEST INFRASTRUCTURE: numpy restatement of csrc/synthetic.hip (st_synth_points_seg), written from the draw table in that file's
header comment.  Integer decisions (class, segment, tip, branch id) are exact; the float outputs are evaluated in `dtype`:
float64 is the reference, float32 (plain numpy operations, no fused multiply-add) is the restatement whose distance from the
float64 one sets the tests' bound."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter [n,4], key (k0, k1) -> [n,4] uint32."""
    c = [np.asarray(counter, dtype=np.uint64)[:, j] & MASK for j in range(4)]
    k0, k1 = np.uint64(int(key[0]) & 0xFFFFFFFF), np.uint64(int(key[1]) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & MASK]
        k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
    return np.stack(c, axis=1).astype(np.uint32)


def draw_words(n, seed):
    """Blocks 0 and 1 of the points 0 .. n-1 of a tree: two [n,4] uint32 arrays."""
    seed = int(seed) & ((1 << 64) - 1)
    key = (seed & 0xFFFFFFFF, seed >> 32)
    ctr = np.zeros((n, 4), dtype=np.uint64)
    ctr[:, 0] = np.arange(n, dtype=np.uint64)
    d = philox4x32_10(ctr, key)
    ctr[:, 1] = 1
    return d, philox4x32_10(ctr, key)


def _uniform(w, dtype):
    return (w >> np.uint32(8)).astype(dtype) * dtype(2.0 ** -24)


def _normal_pair(wa, wb, dtype):
    u1 = ((wa >> np.uint32(8)).astype(np.uint64) + 1).astype(dtype) * dtype(2.0 ** -24)
    u2 = ((wb >> np.uint32(8)).astype(np.uint64) + 1).astype(dtype) * dtype(2.0 ** -24)
    m = np.sqrt(dtype(-2.0) * np.log(u1))
    phi = dtype(2.0 * np.pi) * u2
    return m * np.cos(phi), m * np.sin(phi)


def sample_tree(table, n, seed, fol_thr, noise, sigma, dtype=np.float64, tab0=0):
    """One tree's points: dict(xyz, medial_vector [n,3] in `dtype`; class_l [n] float32; branch_ids, segment [n] int32; t,
    radius [n] and surface [n,3] of the branch points in `dtype`, NaN for foliage)."""
    d, e = draw_words(n, seed)
    n_tips, fol_thr = len(table.tips), int(fol_thr)
    foliage = np.zeros(n, dtype=bool) if n_tips == 0 else ((d[:, 0] < np.uint32(fol_thr)) | (fol_thr == 0xFFFFFFFF))
    nx, ny = _normal_pair(e[:, 0], e[:, 1], dtype)
    nz, _ = _normal_pair(e[:, 2], e[:, 3], dtype)
    normal = np.stack([nx, ny, nz], axis=1)
    xyz = np.zeros((n, 3), dtype=dtype)
    mv = np.zeros((n, 3), dtype=dtype)
    seg = np.full(n, -1, dtype=np.int32)
    bid = np.full(n, -1, dtype=np.int32)
    t_out, r_out, surf = np.full(n, np.nan, dtype), np.full(n, np.nan, dtype), np.full((n, 3), np.nan, dtype)
    f = np.flatnonzero(foliage)
    if len(f):
        tip = table.tips[(d[f, 1] % np.uint32(n_tips)).astype(np.int64)].astype(dtype)
        xyz[f] = tip + dtype(sigma) * normal[f]
    b = np.flatnonzero(~foliage)
    if len(b):
        j = np.minimum(np.searchsorted(table.cdf, d[b, 1], side="right"), len(table.cdf) - 1)  # first cdf[j] > w, else the last
        a, bb, ra, rb = (x[j].astype(dtype) for x in (table.a, table.b, table.ra, table.rb))
        u, v = table.u[j].astype(dtype), table.v[j].astype(dtype)
        t = _uniform(d[b, 2], dtype)
        theta = dtype(2.0 * np.pi) * _uniform(d[b, 3], dtype)
        q = np.cos(theta)[:, None] * u + np.sin(theta)[:, None] * v
        r = ra * (dtype(1.0) - t) + rb * t
        p = a + t[:, None] * (bb - a)
        s = p + r[:, None] * q
        xyz[b] = s + dtype(noise) * normal[b]
        mv[b] = -(r[:, None] * q)
        seg[b] = (tab0 + j).astype(np.int32)
        bid[b] = table.branch[j]
        t_out[b], r_out[b], surf[b] = t, r, s
    return {"xyz": xyz, "medial_vector": mv, "class_l": foliage.astype(np.float32), "branch_ids": bid, "segment": seg, "t": t_out,
            "radius": r_out, "surface": surf}


def sample_batch(tables, counts, seeds, fol_thr, noise, sigma, dtype=np.float64):
    """The batched call: every key of sample_tree concatenated over the trees (segment indexes the batched table)."""
    parts, tab0 = [], 0
    for tb, n, s, th, ns, sg in zip(tables, counts, seeds, fol_thr, noise, sigma):
        parts.append(sample_tree(tb, int(n), s, th, ns, sg, dtype, tab0))
        tab0 += len(tb.ra)
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
