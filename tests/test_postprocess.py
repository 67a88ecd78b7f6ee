"""st_post_process (prune / repair / smooth on the device, csrc/postprocess.hip) against oracle/pipeline_oracle.py on synthetic
branch tables of every size class of the kernel: a lane per branch (<= 1024 branches in a tree), the loop over branches in LDS
(<= 8192), the tables in global memory (more), and several trees in one call.  Reference: data_types/tree.py:73-134,164-176.

Every comparison is bit for bit (kernel and oracle share one float32 operation order).  Each case also asserts, FROM THE ORACLE
ALONE, that the path it was written for was taken (a tube index >= 64, a real tie, a NaN score, a branch smoothed only because
of the prepended point ...), so a case cannot decay into an easy one unnoticed."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import pipeline_oracle as po
from smart_tree_amd import _lib
from smart_tree_amd.skeleton.skeletonize import DeviceSkeleton

F32 = np.float32
G = F32(2.0 ** -6)  # the exact grid: small multiples of it keep every float32 operation of the tube score exact


def _random_tree(rng, nb, first_len=40, len_range=(2, 14), parents="random", grid=None):
    """Branch hierarchy with parent id < child id (or outside [0, nb)); a child starts near a random vertex of its parent.
    parents: "random" | "chain" (b - 1) | "comb" (a chain with a side twig per link) | "invalid" (as random, but branches
    1, 2, 3 and one in twenty of the others hang under -1 / nb / nb + 7).  grid: coordinates and radii rounded to its multiples."""
    branches = []
    for b in range(nb):
        n = int(rng.integers(*len_range)) if b else first_len
        if b == 0:
            parent, origin = -1, np.zeros(3, np.float32)
        else:
            if parents == "chain":
                near = parent = b - 1
            elif parents == "comb":  # odd ids: the chain (1 <- 3 <- 5 ...), even ids: a twig on the chain link before it
                near = parent = max(b - 2, 0) if b % 2 else b - 1
            else:
                parent = int(rng.integers(0, b)) if rng.random() < 0.9 else int(rng.integers(max(0, b - 4), b))  # deep chains too
                near = parent
                if parents == "invalid" and (b <= 3 or rng.random() < 0.05):
                    parent = (-1, nb, nb + 7)[b - 1 if b <= 3 else int(rng.integers(0, 3))]
            pv = branches[near][1]
            origin = pv[int(rng.integers(0, len(pv)))] + rng.normal(0, 0.01, 3).astype(np.float32)
        step = rng.normal(0, 1, 3)
        step = (0.03 * step / np.linalg.norm(step)).astype(np.float32)
        xyz = (origin + np.arange(1, n + 1, dtype=np.float32)[:, None] * step + rng.normal(0, 0.004, (n, 3))).astype(np.float32)
        # a few very short / thin branches so that prune removes some (and their whole sub-hierarchy)
        scale = 0.05 if rng.random() < 0.05 else 1.0
        xyz = (origin + (xyz - origin) * np.float32(scale)).astype(np.float32)
        rad = rng.uniform(0.004 if rng.random() < 0.05 else 0.012, 0.05, n).astype(np.float32)
        if grid is not None:
            xyz, rad = (np.round(xyz / grid) * grid).astype(np.float32), (np.round(rad / grid) * grid).astype(np.float32)
        branches.append((parent, xyz, rad))
    return branches


def _device_skeleton(trees, device, seg=None):
    tree_off, parent, start, length, xyz, rad = [0], [], [], [], [np.zeros((0, 3), np.float32)], [np.zeros(0, np.float32)]
    slot = 0
    for branches in trees:
        for par, bx, br in branches:
            parent.append(par)
            start.append(slot)
            length.append(len(bx))
            xyz.append(np.concatenate([bx[:1], bx]))  # slot start[k]: reserved for the connection point (pre-filled, tree.py:92)
            rad.append(np.concatenate([br[:1], br]))
            slot += len(bx) + 1
        tree_off.append(len(parent))
    i32 = lambda a: torch.tensor(a, dtype=torch.int32, device=device)
    return DeviceSkeleton(i32(tree_off), i32(parent), i32(start), i32(length),
                          torch.from_numpy(np.concatenate(xyz)).to(device), torch.from_numpy(np.concatenate(rad)).to(device),
                          None if seg is None else i32(seg))


def _oracle(trees, prune=None, repair=False, smooth=None, seg=None, trace=None):
    """po.post_process of the same tables, once per cloud (only skeleton 0 OF A CLOUD is pruned).  prune = (min_radius, min_length)."""
    ref = [po.OTree(t, {b: po.OBranch(b, par, bx.copy(), br.reshape(-1, 1).copy()) for b, (par, bx, br) in enumerate(branches)})
           for t, branches in enumerate(trees)]
    seg = [0, len(trees)] if seg is None else seg
    for c in range(len(seg) - 1):
        cloud = ref[seg[c]: seg[c + 1]]
        po.post_process(cloud, prune is not None and bool(cloud) and bool(cloud[0].branches), *(prune or (0.0, 0.0)), repair,
                        smooth is not None, smooth or 1, trace=trace)
    return ref


def _device(trees, device, prune=None, repair=False, smooth=None, seg=None):
    """The same steps on the device: exactly the subset wanted, in the order DeviceSkeleton defers (prune, repair, smooth)."""
    sk = _device_skeleton(trees, device, seg)
    if prune is not None:
        sk.prune(min_radius=prune[0], min_length=prune[1])
    if repair:
        sk.repair()
    if smooth is not None:
        sk.smooth(kernel_size=smooth)
    assert sk._trees is None  # still deferred: reading .skeletons runs st_post_process, not the host fall-back
    return sk


def _same(got, ref):
    """Ids, parents, xyz, radii (values and the [m,1] / [m] quirk of smooth) of every tree, bit for bit, NaN equal to NaN."""
    assert len(got) == len(ref)
    for g, r in zip(got, ref):
        gb, rb = g.branches, r.branches
        assert list(gb.keys()) == list(rb.keys())
        if not rb:
            continue
        assert [b.parent_id for b in gb.values()] == [b.parent_id for b in rb.values()]
        assert [tuple(b.xyz.shape) for b in gb.values()] == [b.xyz.shape for b in rb.values()]
        assert [tuple(b.radii.shape) for b in gb.values()] == [b.radii.shape for b in rb.values()]
        np.testing.assert_array_equal(np.concatenate([b.xyz.numpy() for b in gb.values()]), np.concatenate([b.xyz for b in rb.values()]))
        np.testing.assert_array_equal(np.concatenate([b.radii.numpy().reshape(-1) for b in gb.values()]),
                                      np.concatenate([b.radii.reshape(-1) for b in rb.values()]))


def _chosen_tube(pt, parent):
    """Index of the tube nearest_tube_offset takes its projection from, and every tube's score."""
    i, score, _ = po.nearest_tube(pt, parent)
    return i, score


@pytest.mark.parametrize("sizes", [(300,), (1500,), (9000,), (700, 1, 40, 1100, 3)])
def test_post_process_matches_the_oracle(backend, sizes):
    rng = np.random.default_rng(len(sizes) * 1000 + sizes[0])
    trees = [_random_tree(rng, nb) for nb in sizes]
    sk = _device_skeleton(trees, backend)
    sk.prune(min_radius=0.01, min_length=0.02)
    sk.repair()
    sk.smooth(kernel_size=5)
    ref = [po.OTree(t, {b: po.OBranch(b, par, bx.copy(), br.reshape(-1, 1).copy()) for b, (par, bx, br) in enumerate(branches)})
           for t, branches in enumerate(trees)]
    po.post_process(ref, True, 0.01, 0.02, True, True, 5)
    got = sk.skeletons
    assert len(got) == len(ref)
    pruned = 0
    for g, r in zip(got, ref):
        assert list(g.branches.keys()) == list(r.branches.keys())
        for k, rb in r.branches.items():
            gb = g.branches[k]
            assert gb.parent_id == rb.parent_id
            np.testing.assert_array_equal(gb.xyz.numpy(), rb.xyz)
            np.testing.assert_array_equal(gb.radii.numpy(), rb.radii)
    pruned = sizes[0] - len(ref[0].branches)
    assert 0 < pruned < sizes[0]  # the case exercises the keep chain (only skeleton 0 is pruned: tree.py:164-168)
    assert all(len(r.branches) == nb for r, nb in zip(ref[1:], sizes[1:]))


# ---------------------------------------------------------------------------------- 64-lane chunk loops ---
def _polyline(rng, origin, steps, jitter=0.004):
    d = rng.normal(0, 1, 3)
    d = d / np.linalg.norm(d)
    along = np.cumsum(np.asarray(steps, np.float64))
    return (np.asarray(origin) + along[:, None] * d + rng.normal(0, jitter, (len(steps), 3))).astype(np.float32)


def test_long_branches_cross_the_64_lane_chunks(backend):
    """Branches of 63 / 64 / 65 / 127 / 128 / 129 / 300 segments: the second and third chunk of k_pp_branch's length sum and
    tube scan and of k_pp_smooth's stride, with children whose nearest tube has an index >= 64 (>= 128 on the root)."""
    rng = np.random.default_rng(7)
    rad = lambda n: rng.uniform(0.012, 0.05, n).astype(np.float32)
    branches = [(-1, _polyline(rng, np.zeros(3), [0.03] * 301), rad(301))]
    segs = (63, 64, 65, 127, 128, 129)
    for k, ns in enumerate(segs):  # inner branches under the root, near its tubes 70, 100, ...
        steps = [0.03] * (ns + 1)
        if ns == 127:
            steps = [1e-4] * (ns + 1)  # 127 segments of 0.1 mm: shorter than min_length, pruned by length
        if ns == 129:
            steps = [1e-4] * ns + [0.03]  # kept only by its LAST segment (third chunk of the sum)
        origin = branches[0][1][70 + 30 * k] + rng.normal(0, 0.01, 3)
        branches.append((0, _polyline(rng, origin, steps, 0.004 if steps[0] > 1e-3 else 1e-5), rad(ns + 1)))
    long_ids = list(range(len(branches)))
    for p in long_ids:  # children near the far end and at the chunk boundaries of every long branch
        pv = branches[p][1]
        for at in sorted({62, 63, 64, 65, 66, 126, 127, 128, 129, 130, len(pv) - 2, len(pv) - 1} & set(range(len(pv)))):
            n = int(rng.integers(2, 7))
            branches.append((p, _polyline(rng, pv[at] + rng.normal(0, 0.01, 3), [0.03] * n), rad(n)))
            if rng.random() < 0.5:  # and a grandchild
                branches.append((len(branches) - 1, _polyline(rng, branches[-1][1][-1] + rng.normal(0, 0.01, 3), [0.03] * 3), rad(3)))
    trees = [branches, _random_tree(rng, 30, first_len=140, len_range=(2, 90))]  # tree 1: not pruned, long branches too
    kw = dict(prune=(0.01, 0.02), repair=True, smooth=5)
    trace = []
    ref = _oracle(trees, trace=trace, **kw)
    chosen = {(t, b): (prep, i) for t, b, prep, i, _ in trace}
    assert any(i >= 64 and not prep for (t, b), (prep, i) in chosen.items())  # straight from k_pp_branch's key
    assert any(i >= 64 and prep for (t, b), (prep, i) in chosen.items())  # through the j -> j + 1 shift
    assert any(i >= 128 for prep, i in chosen.values())
    assert 4 not in ref[0].branches and 6 in ref[0].branches and all(b in ref[0].branches for b in (0, 1, 2, 3, 5))
    assert po.branch_length(po.OBranch(0, 0, branches[6][1][:129], None)) < F32(0.02)  # 128 segments alone would not keep it
    _same(_device(trees, backend, **kw).skeletons, ref)


# ------------------------------------------------------------------------------------ exact ties, NaN ---
def _grid_branch(parent, pts, r):
    pts = np.asarray(pts, np.float32) * G
    return parent, pts, np.full(len(pts), F32(r) * G, np.float32)


def _tie_tree(rng, nb):
    """Branch ids: 0 R root (L-shaped at its end); 1 P (b); 2 C child of P: tie between P's connection-point tube and tube 1;
    3 Q L-shaped, 4 D child of Q: tie between two tubes of the extracted path of a repaired parent; 5 E child of R: tie under an
    unrepaired parent; 6 A child of R: projects on the shared vertex of two tubes (a); 7 N with a repeated vertex, 8 NC its
    child, 9 NG its grandchild (c); 10 M with two repeated vertices, 11 MD its child (d); then unrelated padding."""
    b = [_grid_branch(-1, [(0, 0, 0), (16, 0, 0), (32, 0, 0), (48, 0, 0), (64, 0, 0), (64, 16, 0), (64, 32, 0)], 4),
         _grid_branch(0, [(16, 8, 0), (24, 8, 0), (32, 8, 0)], 2),
         _grid_branch(1, [(20, 4, 0), (20, 4, 8)], 1),
         _grid_branch(0, [(40, 8, 0), (48, 8, 0), (48, 16, 0), (48, 24, 0)], 2),
         _grid_branch(3, [(44, 12, 0), (44, 12, 8)], 1),
         _grid_branch(0, [(56, 8, 0), (56, 8, 8)], 1),
         _grid_branch(0, [(32, 8, 8), (32, 8, 16)], 1),
         _grid_branch(0, [(8, -8, 0), (8, -16, 0), (8, -16, 0), (8, -24, 0)], 2),
         _grid_branch(7, [(12, -12, 0), (20, -12, 0)], 1),
         _grid_branch(8, [(16, -14, 0), (16, -14, 8)], 1),
         _grid_branch(0, [(24, -8, 0), (24, -16, 0), (24, -16, 0), (24, -24, 0), (24, -24, 0), (24, -32, 0)], 2),
         _grid_branch(10, [(28, -20, 0), (36, -20, 0)], 1)]
    while len(b) < nb:  # padding: random grid branches anywhere below (children of the special branches change nothing in them)
        n = int(rng.integers(2, 5))
        pts = rng.integers(-40, 80, 3) + np.cumsum(rng.integers(1, 6, (n, 3)), axis=0)
        b.append(_grid_branch(int(rng.integers(0, len(b))), pts, int(rng.integers(1, 5))))
    return b


@pytest.mark.parametrize("nb", [40, 1100])  # a lane per branch / the strided level loop
@pytest.mark.parametrize("steps", ["repair", "all"])
def test_ties_take_the_first_tube_and_nan_wins(backend, nb, steps):
    trees = [_tie_tree(np.random.default_rng(nb), nb)]
    kw = dict(repair=True) if steps == "repair" else dict(prune=(float(G), float(G)), repair=True, smooth=2)
    trace = []
    ref = _oracle(trees, trace=trace, **kw)
    t = {b: (prep, i, score) for _, b, prep, i, score in trace}
    r = ref[0].branches
    xyz0 = lambda k: (r[k].xyz[0] / G).tolist()
    # (a) the shared vertex of tubes 1 and 2 of R: equal scores, the lower index
    assert t[6][:2] == (False, 1) and t[6][2][1] == t[6][2][2] == t[6][2].min() and xyz0(6) == [32, 0, 0]
    # two DIFFERENT projections with equal scores under an unrepaired parent: tube 3, not tube 4 (which would give (64, 8, 0))
    assert t[5][:2] == (False, 3) and t[5][2][3] == t[5][2][4] == t[5][2].min() and xyz0(5) == [56, 0, 0]
    # the same on the extracted path of a repaired parent (tubes 1 and 2 after the shift)
    assert t[4][:2] == (True, 1) and t[4][2][1] == t[4][2][2] == t[4][2].min() and xyz0(4) == [44, 8, 0]
    # (b) the connection-point tube (index 0 after the shift) against tube 1
    assert xyz0(1) == [16, 0, 0]
    assert t[2][:2] == (True, 0) and t[2][2][0] == t[2][2][1] == t[2][2].min() and xyz0(2) == [16, 4, 0]
    # (c) the 0/0 tube wins over finite scores, the connection point is NaN, and the grandchild takes the NaN tube from it
    assert t[8][:2] == (True, 2) and np.isnan(t[8][2][2]) and np.isfinite(np.delete(t[8][2], 2)).all() and np.isnan(r[8].xyz[0]).all()
    assert t[9][:2] == (True, 0) and np.isnan(t[9][2][0]) and np.isfinite(t[9][2][1:]).all() and np.isnan(r[9].xyz[0]).all()
    # (d) two NaN tubes: the first
    assert t[11][:2] == (True, 2) and np.isnan(t[11][2][[2, 4]]).all() and np.isfinite(t[11][2][[0, 1, 3, 5]]).all()
    assert _chosen_tube(trees[0][5][1][0], po.OBranch(0, -1, trees[0][0][1], trees[0][0][2]))[0] == 3
    _same(_device(trees, backend, **kw).skeletons, ref)


def test_prune_thresholds_at_equality(backend):
    """`<` on both thresholds (tree.py:113-116): a length of exactly min_length and an initial radius of exactly min_radius stay,
    one grid step less goes -- with everything below it."""
    seg = lambda parent, x, lens, r: (parent, (np.array([[x, 8 + sum(lens[:i]), 0] for i in range(len(lens) + 1)], np.float32) * G),
                                      np.asarray(r, np.float32) * G)
    b = [_grid_branch(-1, [(0, 0, 0), (32, 0, 0), (64, 0, 0), (96, 0, 0)], 4),
         seg(0, 8, [8, 8], [4, 4, 4]),    # 1: length 16 G == min_length: kept
         seg(0, 24, [8, 7], [4, 4, 4]),   # 2: 15 G: pruned
         seg(0, 40, [16, 16], [2, 9, 1]),  # 3: initial radius max(2, 1) G == min_radius: kept
         seg(0, 56, [16, 16], [1, 9, 1]),  # 4: 1 G: pruned
         seg(0, 72, [16, 16], [1, 1, 2]),  # 5: the LAST radius carries it: kept
         seg(1, 8, [32], [4, 4]), seg(2, 24, [32], [4, 4]), seg(3, 40, [32], [4, 4]), seg(4, 56, [32], [4, 4]),  # 6..9: children
         seg(7, 24, [64], [4, 4])]        # 10: grandchild of 2
    b = [(p, x + (np.array([0, 40, 0], np.float32) * G if k >= 6 else 0), r) for k, (p, x, r) in enumerate(b)]
    trees = [b, b]  # the same table as tree 1, which nobody prunes
    for kw in (dict(prune=(float(2 * G), float(16 * G))), dict(prune=(float(2 * G), float(16 * G)), repair=True, smooth=2)):
        ref = _oracle(trees, **kw)
        assert po.branch_length(po.OBranch(1, 0, b[1][1], None)) == 16 * G and po.branch_length(po.OBranch(2, 0, b[2][1], None)) == 15 * G
        assert list(ref[0].branches) == [0, 1, 3, 5, 6, 8] and len(ref[1].branches) == len(b)
        _same(_device(trees, backend, **kw).skeletons, ref)


# ----------------------------------------------------------------------------------------------- flags ---
@pytest.mark.parametrize("flags", [(p, r, s) for p in (0, 1) for r in (0, 1) for s in (0, 1)])
def test_every_flag_combination(backend, flags):
    rng = np.random.default_rng(400)
    trees = [_random_tree(rng, 400), _random_tree(rng, 60, first_len=9)]
    kw = dict(prune=(0.01, 0.02) if flags[0] else None, repair=bool(flags[1]), smooth=5 if flags[2] else None)
    ref = _oracle(trees, **kw)
    assert (len(ref[0].branches) < 400) == bool(flags[0]) and len(ref[1].branches) == 60
    dims = {b.radii.ndim for t in ref for b in t.branches.values()}
    assert dims == ({1, 2} if flags[2] else {2})  # [m] once smoothed, [m,1] otherwise (and for branches too short to smooth)
    _same(_device(trees, backend, **kw).skeletons, ref)


# ------------------------------------------------------------------------------------ smoothing window ---
@pytest.mark.parametrize("repair", [False, True])
def test_smoothing_window(backend, repair):
    """Odd and even kernels, kernel 1, and the `len > kernel` decision at len = k - 1, k, k + 1 -- on the extracted path (roots,
    orphans, repair off) and on the path with the prepended connection point (len == k is smoothed only because of it)."""
    rng = np.random.default_rng(11)
    for k in (1, 2, 4, 5, 11, 64):
        lens = sorted({max(2, k - 1), max(2, k), k + 1, 2 * k + 3, 200})
        b = [(-1, _polyline(rng, np.zeros(3), [0.03] * 200), rng.uniform(0.012, 0.05, 200).astype(np.float32))]
        for n in lens:
            for parent in (0, -1):  # under the root / an orphan (not repaired)
                origin = b[0][1][int(rng.integers(0, 200))] + rng.normal(0, 0.01, 3)
                b.append((parent, _polyline(rng, origin, [0.03] * n), rng.uniform(0.012, 0.05, n).astype(np.float32)))
        trees = [b, b[:1]]
        ref = _oracle(trees, repair=repair, smooth=k)
        r = ref[0].branches
        by_len = {(len(x), par): i for i, (par, x, _) in enumerate(b) if i}
        if k >= 2:
            assert r[by_len[(k, -1)]].radii.ndim == 2  # len == kernel: left alone ...
            assert r[by_len[(k, 0)]].radii.ndim == (1 if repair else 2)  # ... unless repair made it one longer
            assert r[by_len[(k, 0)]].radii.shape[0] == k + (1 if repair else 0)
            assert r[by_len[(k + 1, -1)]].radii.ndim == 1
        if k >= 3:
            assert r[by_len[(k - 1, 0)]].radii.ndim == 2
        _same(_device(trees, backend, repair=repair, smooth=k).skeletons, ref)


# --------------------------------------------------------------------------------------- size classes ---
@pytest.mark.parametrize("nb", [1, 2, 1024, 1025, 8192, 8193])
def test_size_class_boundaries(backend, nb):
    rng = np.random.default_rng(nb)
    trees = [_random_tree(rng, nb, first_len=4, len_range=(2, 5)), _random_tree(rng, 3, first_len=4, len_range=(2, 5))]
    kw = dict(prune=(0.01, 0.02) if nb > 2 else (10.0, 10.0), repair=True, smooth=2)  # nb <= 2: nothing passes its own tests
    ref = _oracle(trees, **kw)
    if nb <= 2:
        assert list(ref[0].branches) == [0]  # the root always stays (tree.py:101-103,120)
    else:
        assert 0 < len(ref[0].branches) < nb
    _same(_device(trees, backend, **kw).skeletons, ref)


# ---------------------------------------------------------------------------------------------- depth ---
def _thin(branches, b):
    out = list(branches)
    out[b] = (out[b][0], out[b][1], np.full_like(out[b][2], 0.001))  # fails its own radius test
    return out


@pytest.mark.parametrize("nb,parents", [(1024, "chain"), (3001, "chain"), (9001, "chain"), (1500, "comb"), (801, "comb")])
def test_deep_hierarchies(backend, nb, parents):
    """Keep chain and level loop as deep as the table is long (every size class), kept whole and cut near the top.  Branches of
    2-3 vertices: the emulator's time is the level count times a 1024-fiber barrier (9001: 17 s there, 0.6 s on the device)."""
    rng = np.random.default_rng(nb)
    whole = _random_tree(rng, nb, first_len=3, len_range=(2, 4), parents=parents)
    whole = [(p, x, np.maximum(r, F32(0.012))) for p, x, r in whole]
    kw = dict(prune=(0.01, 0.0), repair=True, smooth=2)
    trace = []
    ref = _oracle([whole], trace=trace, **kw)
    assert len(ref[0].branches) == nb and len(trace) == nb - 1
    _same(_device([whole], backend, **kw).skeletons, ref)
    cut = _thin(whole, 5)
    ref = _oracle([cut], **kw)
    assert list(ref[0].branches) == [0, 1, 2, 3, 4]  # everything else hangs under branch 5
    _same(_device([cut], backend, **kw).skeletons, ref)


@pytest.mark.parametrize("backend", [pytest.param("hip", marks=pytest.mark.gpu)], indirect=True)
def test_depth_beyond_32767(backend):
    """A chain of 33 000 two-vertex branches: the level loop of the global-table path runs 32 999 times (it used to stop at level
    32 767 and leave the rest unrepaired, which this case showed on the emulator before the fix).  On the device only: the
    emulator pays a 1024-fiber barrier per level and needs 52 s for it (measured; it passes there)."""
    nb = 33000
    rng = np.random.default_rng(33)
    pts = np.cumsum(rng.normal(0, 0.02, (nb + 1, 3)), axis=0).astype(np.float32)
    rad = rng.uniform(0.012, 0.05, (nb, 2)).astype(np.float32)
    chain = [(b - 1, pts[b: b + 2] + np.float32(0.004), rad[b]) for b in range(nb)]
    kw = dict(prune=(0.01, 0.0), repair=True, smooth=2)
    trace = []
    ref = _oracle([chain], trace=trace, **kw)
    assert len(ref[0].branches) == nb and len(trace) == nb - 1 and all(b.xyz.shape[0] == 3 for b in list(ref[0].branches.values())[1:])
    _same(_device([chain], backend, **kw).skeletons, ref)


# --------------------------------------------------------------------------- parents outside the tree ---
@pytest.mark.parametrize("nb", [120, 1300])
def test_parents_outside_the_tree(backend, nb):
    rng = np.random.default_rng(nb + 1)
    tree = _random_tree(rng, nb, parents="invalid")
    assert [tree[b][0] for b in (1, 2, 3)] == [-1, nb, nb + 7]
    outside = {b for b, (p, _, _) in enumerate(tree) if b and not 0 <= p < nb}
    below = set(outside)
    for b, (p, _, _) in enumerate(tree):
        if p in below:
            below.add(b)
    assert len(below) > len(outside) + 3  # they have descendants
    for t in ([tree], [tree[:4], tree]):  # as the pruned tree 0 / as a tree nobody prunes
        kw = dict(prune=(0.01, 0.02), repair=True, smooth=5)
        ref = _oracle(t, **kw)
        if len(t) == 1:
            assert not below & set(ref[0].branches)  # orphans: the whole sub-hierarchy goes
        _same(_device(t, backend, **kw).skeletons, ref)
    trace = []
    ref = _oracle([tree], repair=True, trace=trace)
    r = ref[0].branches
    assert all(r[b].xyz.shape[0] == tree[b][1].shape[0] for b in outside)  # not repaired ...
    under = [(b, prep) for _, b, prep, _, _ in trace if tree[b][0] in outside]
    assert under and not any(prep for _, prep in under)  # ... and their children are repaired against the extracted path
    _same(_device([tree], backend, repair=True).skeletons, ref)


# ---------------------------------------------------------------------------------------- batched form ---
def _with_prunable_subtree(tree):
    tree = _thin(tree, 1)
    tree[2] = (1, tree[2][1], tree[2][2])
    return tree


def _cloud_layout(rng, n_clouds):
    """Tree sizes per cloud: clouds without trees first, in the middle and last (n_clouds > 3), a tree without branches between
    two others, several trees in a cloud."""
    sizes = []
    for c in range(n_clouds):
        if c in (0, n_clouds // 2, n_clouds - 1):
            sizes.append([])
        else:
            sizes.append([int(rng.integers(4, 30))] + [0 if k == 1 and c % 2 else int(rng.integers(1, 12)) for k in range(1, 1 + c % 4)])
    if n_clouds <= 3:
        sizes = [[30, 0, 12]] if n_clouds == 1 else [[20, 0, 9], [], [15, 7]]
    return sizes


@pytest.mark.parametrize("n_clouds", [1, 3, 5, 64])
def test_batched_clouds(backend, n_clouds):
    rng = np.random.default_rng(n_clouds)
    sizes = _cloud_layout(rng, n_clouds)
    trees, seg = [], [0]
    for cloud in sizes:
        for k, nb in enumerate(cloud):
            t = _random_tree(rng, nb, first_len=12, len_range=(2, 9)) if nb else []
            trees.append(_with_prunable_subtree(t) if k == 0 else t)
        seg.append(len(trees))
    kw = dict(prune=(0.01, 0.02), repair=True, smooth=3)
    ref = _oracle(trees, seg=seg, **kw)
    sk = _device(trees, backend, seg=seg, **kw)
    parts = sk.split()
    assert len(parts) == n_clouds
    for c, part in enumerate(parts):
        cloud = ref[seg[c]: seg[c + 1]]
        if cloud:
            assert 1 not in cloud[0].branches and 2 not in cloud[0].branches  # the first tree of EVERY cloud is pruned
            assert all(len(r.branches) == nb for r, nb in zip(cloud[1:], sizes[c][1:]))  # and no other
        _same(part.skeletons, cloud)
    _same(sk.skeletons, ref)


def test_batched_call_refusals(backend):
    """More than 64 clouds, and smoothing without a kernel size: refused with a message before anything is launched."""
    L = _lib.lib()
    tree = _random_tree(np.random.default_rng(0), 3, first_len=4, len_range=(2, 5))
    tree_off, parent, start, length, xyz, rad = _device_skeleton([tree], backend)._dev
    B, before = parent.shape[0], xyz.clone()
    u8 = lambda: torch.zeros(B, dtype=torch.uint8, device=backend)
    keep, repaired, smoothed, rad_out = u8(), u8(), u8(), torch.zeros_like(rad)
    depth = torch.zeros(B, dtype=torch.int32, device=backend)
    first = torch.zeros(65, dtype=torch.int32, device=backend)

    def call(do_smooth, kernel, n_first):
        return L.st_post_process_seg(1, _lib.ptr(tree_off), _lib.ptr(parent), _lib.ptr(start), _lib.ptr(length), _lib.ptr(xyz),
                                     _lib.ptr(rad), _lib.ptr(rad_out), _lib.ptr(keep), _lib.ptr(repaired), _lib.ptr(smoothed),
                                     _lib.ptr(depth), 1, 0.01, 0.02, 1, do_smooth, kernel, _lib.ptr(first), n_first, _lib.stream(backend))

    for args, word in (((1, 5, 65), "64 clouds"), ((1, 0, 1), "kernel_size")):
        assert call(*args) != 0
        assert word in L.st_last_error().decode()
        if backend.type == "cuda":
            torch.cuda.synchronize()
        assert torch.equal(xyz, before) and not rad_out.any() and not keep.any()
    assert call(1, 5, 64) == 0 and call(0, 0, 1) == 0  # the limits themselves are accepted
    if backend.type == "cuda":
        torch.cuda.synchronize()
    assert not torch.equal(xyz, before)


# ----------------------------------------------------------------------------------------------- sweep ---
SWEEP_SEEDS = (1000, 1001, 1002, 1003)
_sweep_cache = {}


def _sweep_case(seed):
    """About 300 small trees of every parent policy in 60 clouds of one call, under one random setting; the oracle's result and
    the outcomes that occurred in it.  Computed once per seed and shared (nothing changes it)."""
    if seed in _sweep_cache:
        return _sweep_cache[seed]
    rng = np.random.default_rng(seed)
    trees = []
    for _ in range(300):
        nb = int(rng.integers(1, 41))
        policy = ("random", "chain", "comb", "invalid")[int(rng.integers(0, 4))]
        trees.append(_random_tree(rng, nb, first_len=int(rng.integers(2, 91)), len_range=(2, 91) if rng.random() < 0.2 else (2, 12),
                                  parents=policy, grid=F32(2.0 ** -9) if rng.random() < 0.2 else None))
    seg = list(range(0, 301, 5))
    flags = (1, 1, 1) if seed == SWEEP_SEEDS[0] else tuple(int(v) for v in rng.integers(0, 2, 3))
    k = int(rng.integers(1, 13))
    kw = dict(prune=(float(rng.uniform(0.005, 0.02)), float(rng.uniform(0.01, 0.1))) if flags[0] else None, repair=bool(flags[1]),
              smooth=k if flags[2] else None)
    trace, seen = [], set()
    ref = _oracle(trees, seg=seg, trace=trace, **kw)
    for t, tree in enumerate(trees):
        if kw["prune"] and t % 5 == 0:
            for b, (p, x, r) in enumerate(tree):
                if b and b not in ref[t].branches:
                    short = po.branch_length(po.OBranch(b, p, x, r)) < F32(kw["prune"][1])
                    thin = max(r[0], r[-1]) < F32(kw["prune"][0])
                    seen.update({"length"} if short else set(), {"radius"} if thin else set(), set() if short or thin else {"orphan"})
        if kw["smooth"]:
            seen.update("smoothed" if b.radii.ndim == 1 else "too short to smooth" for b in ref[t].branches.values())
    seen.update("under a repaired parent, tube 0" if prep and i == 0 else "under a repaired parent" if prep else
                "under an unrepaired parent" for _, _, prep, i, _ in trace)
    _sweep_cache[seed] = (trees, seg, kw, ref, seen)
    return _sweep_cache[seed]


@pytest.mark.parametrize("seed", SWEEP_SEEDS)
def test_seeded_sweep(backend, seed):
    trees, seg, kw, ref, _ = _sweep_case(seed)
    for c, part in enumerate(_device(trees, backend, seg=seg, **kw).split()):
        _same(part.skeletons, ref[seg[c]: seg[c + 1]])


def test_seeded_sweep_reaches_every_outcome():
    """Counted on the oracle's side alone: the seeds were chosen so that every outcome of the three steps occurs."""
    seen = set().union(*(_sweep_case(seed)[4] for seed in SWEEP_SEEDS))
    assert seen == {"length", "radius", "orphan", "smoothed", "too short to smooth", "under a repaired parent, tube 0",
                    "under a repaired parent", "under an unrepaired parent"}
    assert len({tuple(sorted((k, v is not None and v is not False) for k, v in _sweep_case(seed)[2].items())) for seed in SWEEP_SEEDS}) > 1
