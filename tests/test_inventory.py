"""Tree measurements (csrc/tree_tally.hip, smart_tree_amd/inventory.py).

The tally is compared for exact equality with tests/inventory_oracle.py (float32 cell arithmetic in the header's order, Python sets for
the distinct cells); the skeleton metrics with the oracle's tube-by-tube float64 sums at 1e-9 relative and with closed forms.  Each
scene is the smallest that reaches one way the kernel can go wrong; one oracle run per scene, shared and read-only.
"""
import functools
import math

import numpy as np
import pytest
import torch

from smart_tree_amd import _lib
from smart_tree_amd import inventory as I
from smart_tree_amd.data_types.branch import BranchSkeleton
from smart_tree_amd.data_types.cloud import Cloud
from smart_tree_amd.data_types.flat import FlatSkeletons
from smart_tree_amd.data_types.tree import DisjointTreeSkeleton, TreeSkeleton

import inventory_oracle as io

F = np.float32


def _t(x, dev, dtype=None):
    if x is None:
        return None
    return torch.from_numpy(np.array(x)).to(dev) if dtype is None else torch.as_tensor(np.array(x), dtype=dtype, device=dev)


def _run(dev, pts, tree, n_trees, cls=None, n_classes=1, **kw):
    res = I.tree_tally(_t(pts, dev), _t(tree, dev, torch.int32), n_trees, _t(cls, dev, torch.uint8), n_classes, **kw)
    return {k: v.cpu().numpy() for k, v in res.items()}


def _assert_tally(got, want):
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
        if k == "box":
            np.testing.assert_array_equal(got[k].view(np.uint32), want[k].view(np.uint32))
        else:
            np.testing.assert_array_equal(got[k], want[k], err_msg=k)


# -------------------------------------------------------------------------------------------- scenes ---
@functools.lru_cache(maxsize=None)
def _scene(name):
    """(pts, tree, n_trees, cls, n_classes, keywords)."""
    rng = np.random.default_rng(17)
    cls, n_classes, kw = None, 1, {}
    if name == "one_point":
        pts, tree, T = np.array([[0.3, -1.5, 2.0]], F), np.zeros(1, np.int32), 1
    elif name == "one_cell":  # 20 000 points of one tree inside one cell: every lane wants the same slot
        pts, tree, T = (5.0 + rng.uniform(0.0, 0.09, size=(20000, 3))).astype(F), np.zeros(20000, np.int32), 1
        pts[0] = 5.0  # the box's corner, so that no point reaches the next cell
        kw = dict(cell=0.1)
    elif name == "own_cells":  # 50 000 points, each in a plan cell and a volume cell of its own: the set at its worst-case fill
        i = np.arange(50000)
        pts = np.stack([(i % 250) * 0.01, ((i * 7) % 100) * 0.01, (i // 250) * 0.01], axis=1).astype(F)
        pts, tree, T = pts[rng.permutation(50000)], np.zeros(50000, np.int32), 1
        kw = dict(cell=0.001, layers=64)
    elif name == "many_trees":  # 700 trees interleaved among 3 000 points: more in a workgroup than any LDS table holds
        pts, tree, T = rng.normal(size=(3000, 3)).astype(F), (np.arange(3000) % 700).astype(np.int32), 700
        cls, n_classes = (np.arange(3000) % 3).astype(np.uint8), 3
        kw = dict(cell=0.25, layers=8)
    elif name == "multiples":  # exact multiples of the cell above and below zero, the minimum negative
        k = rng.integers(-8, 9, size=(400, 3))
        k[0], k[1] = -8, 8
        pts, tree, T = (k * 0.125).astype(F), np.zeros(400, np.int32), 1
        kw = dict(cell=0.125, layers=32)
    elif name == "tall":  # taller than the layers: the last one collects what is above it
        pts = np.stack([rng.uniform(0, 0.3, 600), rng.uniform(0, 1.0, 600), rng.uniform(0, 0.3, 600)], axis=1).astype(F)
        pts[0], pts[1] = 0.0, (0.3, 1.0, 0.3)
        tree, T = np.zeros(600, np.int32), 1
        kw = dict(cell=0.1, layers=4)
    elif name == "ignored":  # NaN / inf coordinates, tree ids outside the trees, classes outside the classes
        pts, tree, T = rng.uniform(-2, 2, size=(5000, 3)).astype(F), rng.integers(-2, 5, size=5000).astype(np.int32), 3
        pts[::7, 0], pts[3::11, 1], pts[5::13, 2] = np.nan, np.inf, -np.inf
        cls, n_classes = rng.integers(0, 4, size=5000).astype(np.uint8), 2
        kw = dict(cell=0.2, layers=16)
    elif name == "forest":  # a few trees of different sizes, in runs and mixed, two workgroups
        pts = rng.normal(size=(4099, 3)).astype(F) * F(3.0)
        tree, T = np.where(np.arange(4099) < 2500, 0, rng.integers(0, 5, size=4099)).astype(np.int32), 5
        kw = dict(cell=0.3, layers=12)
    else:
        raise KeyError(name)
    for x in (pts, tree, cls):
        if x is not None:
            x.setflags(write=False)
    return pts, tree, T, cls, n_classes, kw


@functools.lru_cache(maxsize=None)
def _scene_oracle(name, up=1):
    pts, tree, T, cls, n_classes, kw = _scene(name)
    want = io.tally(pts, tree, T, cls, n_classes, up=up, **kw)
    for v in want.values():
        v.setflags(write=False)
    return want


SCENES = ("one_point", "one_cell", "own_cells", "many_trees", "multiples", "tall", "ignored", "forest")


# ---------------------------------------------------------------------------------------- 1: the tally ---
@pytest.mark.parametrize("name", SCENES)
def test_tally_equals_the_oracle(backend, name):
    pts, tree, T, cls, n_classes, kw = _scene(name)
    want = _scene_oracle(name)
    got = _run(backend, pts, tree, T, cls, n_classes, **kw)
    _assert_tally(got, want)
    box, counts, area, profile = (got[k] for k in ("box", "counts", "area_cells", "profile"))
    if name == "one_point":
        assert box[0].tolist() == [F(0.3), F(-1.5), F(2.0)] * 2 and counts.tolist() == [[1]] and area.tolist() == [1]
        assert profile[0, 0] == 1 and profile.sum() == 1
    elif name == "one_cell":
        assert counts.tolist() == [[20000]] and area.tolist() == [1] and profile[0, 0] == 1 and profile.sum() == 1
    elif name == "own_cells":
        assert area.tolist() == [50000] and profile.sum() == 50000
    elif name == "many_trees":
        assert (np.unique(tree[:2048]).size == 700) and (counts.sum(1) > 0).all() and counts.shape == (700, 3) and (counts > 0).all()
    elif name == "multiples":  # index = k + 8, whatever the sign of the coordinate
        k = np.rint(pts / F(0.125)).astype(int) + 8
        assert box[0].tolist() == [-1.0] * 3 + [1.0] * 3
        assert area[0] == len({(a, c) for a, _, c in k.tolist()}) and profile.sum() == len({tuple(r) for r in k.tolist()})
        assert profile[0].tolist() == [len({tuple(r) for r in k.tolist() if r[1] == j}) for j in range(17)] + [0] * 15
    elif name == "tall":
        triples = {tuple(r) for r in np.floor(pts / F(0.1)).astype(int).tolist()}  # (min = 0)
        assert profile.sum() == len(triples) and profile[0, 3] == len({r for r in triples if r[1] >= 3}) > profile[0, 2] > 0
    elif name == "ignored":
        ok = io.takes_part(pts, tree, T, cls, n_classes)
        assert 0 < ok.sum() < 0.5 * len(pts) and counts.sum() == ok.sum() and (counts > 0).all() and np.isfinite(box).all()
        # the second class splits the counts and not the cells
        one = _run(backend, pts[ok], tree[ok], T, **kw)
        np.testing.assert_array_equal(one["counts"][:, 0], counts.sum(1))
        for k in ("box", "area_cells", "profile"):
            np.testing.assert_array_equal(one[k], got[k])


def test_nothing_to_tally(backend):
    pts, tree, T, cls, n_classes, kw = _scene("forest")
    empty = {"box": np.tile(np.array([np.inf] * 3 + [-np.inf] * 3, F), (T, 1)), "counts": np.zeros((T, 1), np.int64),
             "area_cells": np.zeros(T, np.int64), "profile": np.zeros((T, 12), np.int64)}
    _assert_tally(_run(backend, pts[:0], tree[:0], T, **kw), empty)                         # n = 0
    _assert_tally(_run(backend, pts, np.full(len(pts), -1, np.int32), T, **kw), empty)      # every point without a tree
    none = _run(backend, pts, tree, 0, **kw)                                                # no trees
    assert none["box"].shape == (0, 6) and none["counts"].shape == (0, 1) and none["profile"].shape == (0, 12)
    # n = 0 through the C call: outputs that held something are filled
    L = _lib.lib()
    box = torch.full((T, 6), 7.0, dtype=torch.float32, device=backend)
    ints = [torch.full(s, 77, dtype=torch.int64, device=backend) for s in ((T, 1), (T,), (T, 12))]
    ws = _lib.workspace(L.st_tree_tally_workspace_bytes(0, T, 12), backend)
    _lib.check(L.st_tree_tally(None, 0, None, None, 1, T, 1, 0.3, 12, _lib.ptr(box), *[_lib.ptr(t) for t in ints], _lib.ptr(ws), ws.numel(),
                               _lib.stream(backend)))
    _assert_tally({"box": box.cpu().numpy(), "counts": ints[0].cpu().numpy(), "area_cells": ints[1].cpu().numpy(), "profile": ints[2].cpu().numpy()}, empty)


@pytest.mark.parametrize("up", [0, 1, 2])
def test_vertical_axis(backend, up):
    pts, tree, T, cls, n_classes, kw = _scene("forest")
    got = _run(backend, pts, tree, T, up=up, **kw)
    _assert_tally(got, _scene_oracle("forest", up))
    perm = {0: [1, 0, 2], 1: [0, 1, 2], 2: [0, 2, 1]}[up]  # the vertical axis to the middle, the horizontal ones in their order
    turned = io.tally(np.ascontiguousarray(pts[:, perm]), tree, T, up=1, **kw)
    np.testing.assert_array_equal(got["area_cells"], turned["area_cells"])
    np.testing.assert_array_equal(got["profile"], turned["profile"])
    np.testing.assert_array_equal(got["box"][:, perm + [3 + p for p in perm]], turned["box"])
    if up != 1:
        assert not np.array_equal(got["profile"], _scene_oracle("forest", 1)["profile"])


def test_outputs_are_optional_and_runs_identical(backend):
    pts, tree, T, cls, n_classes, kw = _scene("forest")
    want = _scene_oracle("forest")
    for outputs in (("area_cells",), ("profile",), ("box", "counts"), ("counts", "profile")):
        got = _run(backend, pts, tree, T, outputs=outputs, **kw)
        _assert_tally(got, {k: want[k] for k in outputs})
    for name in ("own_cells", "many_trees"):
        pts, tree, T, cls, n_classes, kw = _scene(name)
        _assert_tally(_run(backend, pts, tree, T, cls, n_classes, **kw), _run(backend, pts, tree, T, cls, n_classes, **kw))


@functools.lru_cache(maxsize=None)
def _handfuls():
    """For n = 1..64 and three seeds: n points in cells of their own (uniform in a 10 m cube, 1 cm cells), on one tree and dealt over
    three, with the oracle's answer.  The cell set is at its smallest here (16 to 256 slots) and at its fullest: 2 n keys."""
    cases = []
    for seed in range(3):
        for n in range(1, 65):
            rng = np.random.default_rng(1000 * seed + n)
            pts = rng.uniform(0.0, 10.0, size=(n, 3)).astype(F)
            for T in (1, 3):
                tree = (np.arange(n) % T).astype(np.int32)
                want = io.tally(pts, tree, T, cell=0.01, layers=64)
                assert want["area_cells"].sum() == n and want["profile"].sum() == n  # every point in a cell of its own, in both families
                cases.append((pts, tree, T, want))
    return cases


def test_handfuls_of_points_in_cells_of_their_own(backend):
    """A key must find a slot however small the set is: no distinct cell may be taken for one already there."""
    for pts, tree, T, want in _handfuls():
        _assert_tally(_run(backend, pts, tree, T, cell=0.01, layers=64), want)


def test_refusals(backend):
    L = _lib.lib()
    pts, tree, T, _, _, _ = _scene("forest")
    n = 512
    tp, tt, tc = _t(pts[:n], backend), _t(tree[:n], backend), torch.zeros(n, dtype=torch.uint8, device=backend)
    box = torch.full((T, 6), -7.0, dtype=torch.float32, device=backend)
    ints = [torch.full(s, -7, dtype=torch.int64, device=backend) for s in ((T, 2), (T,), (T, 12))]
    ws = _lib.workspace(L.st_tree_tally_workspace_bytes(n, T, 12), backend)

    def call(n=n, T=T, layers=12, up=1, cell=0.3, n_classes=2, pts=tp, tree=tt, ws_bytes=None):
        return L.st_tree_tally(_lib.ptr(pts), n, _lib.ptr(tree), _lib.ptr(tc), n_classes, T, up, cell, layers, _lib.ptr(box),
                               *[_lib.ptr(t) for t in ints], _lib.ptr(ws), ws.numel() if ws_bytes is None else ws_bytes, _lib.stream(backend))

    cases = {"points": dict(n=1 << 31), "negative points": dict(n=-1), "trees": dict(T=1 << 21), "negative trees": dict(T=-1),
             "no layers": dict(layers=0), "layers": dict(layers=4097), "up": dict(up=3), "negative up": dict(up=-1),
             "zero cell": dict(cell=0.0), "negative cell": dict(cell=-0.1), "nan cell": dict(cell=float("nan")),
             "inf cell": dict(cell=float("inf")), "no classes": dict(n_classes=0), "classes": dict(n_classes=256),
             "no points array": dict(pts=None), "no tree array": dict(tree=None), "workspace": dict(ws_bytes=64)}
    for what, kw in cases.items():
        rc = call(**kw)
        assert rc == (-2 if what == "workspace" else -1), what
        text = L.st_last_error().decode()
        assert text.startswith("tree_tally:") and len(text) > 20, what
    assert "workspace too small" in L.st_last_error().decode()
    assert (box.cpu().numpy() == -7).all() and all((t.cpu().numpy() == -7).all() for t in ints)  # nothing launched, nothing written
    Q = L.st_tree_tally_workspace_bytes
    assert Q(1 << 31, 3, 8) == -1 and Q(5, 1 << 21, 8) == -1 and Q(5, 3, 0) == -1 and Q(5, 3, 4097) == -1 and Q(-1, 3, 8) == -1
    assert Q(0, 0, 1) >= 0 and Q((1 << 31) - 1, (1 << 21) - 1, 4096) >= 32 * ((1 << 31) - 1)  # the worst case: 2 keys per point, half full
    assert call() == 0 and ints[0].cpu().numpy().sum() == n and L.st_version() >= 114
    with pytest.raises(_lib.StError, match="cell size"):
        I.tree_tally(tp, tt, T, cell=0.0)
    with pytest.raises(ValueError):
        I.tree_tally(tp, tt[:5], T)


# --------------------------------------------------------------------------------------- 2: host metrics ---
def _branch(bid, parent, xyz, radii):
    return BranchSkeleton(bid, parent, torch.tensor(xyz, dtype=torch.float32), torch.tensor(radii, dtype=torch.float32).reshape(-1, 1))


def _hand_tree(tree_id=0, top=3.0, shift=(0.0, 0.0, 0.0)):
    """A trunk of two frusta along y, a perpendicular branch along x from its middle, a grandchild along z, an orphan."""
    s = np.asarray(shift)
    at = lambda rows: (np.asarray(rows, np.float64) + s).tolist()
    return TreeSkeleton(tree_id, {0: _branch(0, -1, at([[0, 0, 0], [0, 1, 0], [0, top, 0]]), [0.25, 0.125, 0.0625]),
                                  1: _branch(1, 0, at([[0, 2, 0], [1, 2, 0], [2, 2, 0]]), [0.0625, 0.03125, 0.03125]),
                                  2: _branch(2, 1, at([[1, 2, 0], [1, 2, 1]]), [0.03125, 0.015625]),
                                  5: _branch(5, 99, at([[0, 3, 0], [0.5, 3.5, 0]]), [0.03125, 0.03125])})


def _frustum(h, r1, r2):
    return math.pi * h * (r1 * r1 + r1 * r2 + r2 * r2) / 3.0, math.pi * (r1 + r2) * math.sqrt(h * h + (r1 - r2) ** 2)


def _oracle_input(tree: TreeSkeleton):
    return [(k, b.parent_id, b.xyz.numpy().astype(np.float64), b.radii.numpy().reshape(-1).astype(np.float64)) for k, b in tree.branches.items()]


def _no_points(T, layers=8):
    return (np.tile(np.array([np.inf] * 3 + [-np.inf] * 3, F), (T, 1)), np.zeros((T, 1), np.int64), np.zeros(T, np.int64),
            np.zeros((T, layers), np.int64))


def test_branch_metrics_by_hand():
    tree = _hand_tree()
    flat = FlatSkeletons([tree])
    rows, orphans = I.branch_table(flat, points=np.array([40.0, 30.0, 20.0, 10.0]))
    col = lambda name: rows[:, I.BRANCH_COLUMNS.index(name)]
    assert rows.shape == (4, 14) and col("branch").tolist() == [0, 1, 2, 5] and col("parent").tolist() == [-1, 0, 1, 99]
    assert col("order").tolist() == [0, 1, 2, 0] and orphans.tolist() == [[0, 0, 5]] and col("tubes").tolist() == [2, 2, 1, 1]
    assert col("points").tolist() == [40, 30, 20, 10] and (col("cloud") == 0).all() and (col("tree") == 0).all()
    v0, a0 = np.add(_frustum(1.0, 0.25, 0.125), _frustum(2.0, 0.125, 0.0625))
    v1, a1 = np.add(_frustum(1.0, 0.0625, 0.03125), _frustum(1.0, 0.03125, 0.03125))
    v2, a2 = _frustum(1.0, 0.03125, 0.015625)
    np.testing.assert_allclose(col("volume")[:3], [v0, v1, v2], rtol=1e-12)
    np.testing.assert_allclose(col("area")[:3], [a0, a1, a2], rtol=1e-12)
    np.testing.assert_allclose(col("length"), [3.0, 2.0, 1.0, math.sqrt(0.5)], rtol=1e-12)
    np.testing.assert_allclose(col("mean_radius")[:2], [(1 * 0.1875 + 2 * 0.09375) / 3, (0.046875 + 0.03125) / 2], rtol=1e-12)
    assert col("base_radius").tolist() == [0.25, 0.0625, 0.03125, 0.03125] and col("tip_radius").tolist() == [0.0625, 0.03125, 0.015625, 0.03125]
    np.testing.assert_allclose(col("angle")[1:3], [90.0, 90.0], rtol=1e-12)
    assert np.isnan(col("angle")[0]) and np.isnan(col("angle")[3])
    # against the oracle's tube-by-tube sums
    per, o_orphans = io.branches(_oracle_input(tree))
    assert o_orphans == [5]
    for k, bid in enumerate([0, 1, 2, 5]):
        for name in ("order", "tubes", "length", "volume", "area", "mean_radius", "base_radius", "tip_radius", "angle"):
            np.testing.assert_allclose(col(name)[k], per[bid][name], rtol=1e-9, err_msg=f"{bid} {name}")


def test_tree_metrics_by_hand():
    tall, short = _hand_tree(0), _hand_tree(1, top=1.25, shift=(5.0, -2.0, 0.0))
    sk = DisjointTreeSkeleton([tall, short])
    flat = FlatSkeletons([sk])
    assert flat.tree_rows.tolist() == [[0, 0], [0, 1]]
    rows, _ = I.branch_table(flat)
    box, counts, area, profile = _no_points(2)
    trees = I.tree_table(flat, rows, box, counts, area, profile, 0.1)
    cols = I.tree_columns(1)
    assert trees.shape == (2, len(cols)) and cols[:4] == ("cloud", "tree", "points", "points_class_0") and cols[-1] == "dbh"
    g = lambda r, name: trees[r, cols.index(name)]
    # no points: the base is the lowest tube end; 1.3 m above it the trunk's second tube is at t = 0.15
    assert g(0, "base") == 0.0 and g(1, "base") == -2.0 and g(0, "points") == 0 and np.isnan(g(0, "height")) and np.isnan(g(0, "crown_width"))
    np.testing.assert_allclose(g(0, "dbh"), 2 * (0.125 + 0.15 * (0.0625 - 0.125)), rtol=1e-12)
    assert np.isnan(g(1, "dbh"))  # a trunk of 1.25 m never reaches breast height
    assert g(0, "branches") == 4 and g(0, "max_order") == 2 and g(0, "trunk_length") == 3.0 and g(1, "trunk_length") == 1.25
    assert g(0, "crown_area") == 0 and g(0, "crown_volume") == 0 and np.isnan(g(0, "widest_layer_height"))
    vol = rows[:4, I.BRANCH_COLUMNS.index("volume")]
    np.testing.assert_allclose([g(0, f"volume_order_{k}") for k in range(4)], [vol[0] + vol[3], vol[1], vol[2], 0.0], rtol=1e-12)
    np.testing.assert_allclose(g(0, "wood_volume"), vol.sum(), rtol=1e-12)
    np.testing.assert_allclose(g(0, "length"), 6.0 + math.sqrt(0.5), rtol=1e-12)
    # with points: the tallies set base, height, crown; DBH follows the points' base
    box[0] = [-1.0, -0.5, -2.0, 1.5, 3.25, 1.0]
    counts[0], area[0], profile[0, 2], profile[0, 5] = 100, 7, 4, 9
    trees = I.tree_table(flat, rows, box, counts, area, profile, 0.1)
    assert g(0, "base") == -0.5 and g(0, "height") == 3.75 and g(0, "crown_width") == 3.0 and g(0, "points") == 100 == g(0, "points_class_0")
    np.testing.assert_allclose([g(0, "crown_area"), g(0, "crown_volume"), g(0, "widest_layer_height")], [7 * 0.01, 13 * 0.001, 0.55], rtol=1e-12)
    np.testing.assert_allclose(g(0, "dbh"), 2 * (0.25 + 0.8 * (0.125 - 0.25)), rtol=1e-12)  # 0.8 m up the first tube
    for r, tree in enumerate((tall, short)):
        want, _, _ = io.tree(_oracle_input(tree), box[r], counts[r], area[r], profile[r], 0.1)
        for name, value in want.items():
            np.testing.assert_allclose(g(r, name), value, rtol=1e-9, err_msg=f"{r} {name}")
    # another vertical axis and breast height reach the walk
    lying = I.tree_table(flat, rows, *_no_points(2), 0.1, breast_height=0.5, up=0)
    assert lying[0, cols.index("base")] == 0.0 and np.isnan(lying[0, cols.index("dbh")])  # along x the trunk stays at 0: no crossing of 0.5
    lying = I.tree_table(flat, rows, *_no_points(2), 0.1, breast_height=0.0, up=0)
    assert lying[0, cols.index("dbh")] == 0.5  # and at its own level the first tube's first radius


# ------------------------------------------------------------------------------- 3: measure_trees ---
def _surface_points(tree: TreeSkeleton, n, seed):
    """n points on the tubes' surfaces (float32), and a class per point."""
    rng = np.random.default_rng(seed)
    a, b, r1, r2 = [], [], [], []
    for br in tree.branches.values():
        x, r = br.xyz.numpy().astype(np.float64), br.radii.numpy().reshape(-1).astype(np.float64)
        a.append(x[:-1]); b.append(x[1:]); r1.append(r[:-1]); r2.append(r[1:])
    a, b, r1, r2 = (np.concatenate(v) for v in (a, b, r1, r2))
    j = rng.integers(len(a), size=n)
    t = rng.uniform(0.0, 1.0, size=(n, 1))
    axis = (b[j] - a[j]) / np.linalg.norm(b[j] - a[j], axis=1, keepdims=True)
    u = rng.normal(size=(n, 3))
    u -= (u * axis).sum(1, keepdims=True) * axis
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    pts = a[j] + t * (b[j] - a[j]) + ((1 - t) * r1[j, None] + t * r2[j, None]) * u
    return pts.astype(F), (rng.uniform(size=n) < 0.3).astype(F).reshape(-1, 1)


@functools.lru_cache(maxsize=None)
def _batch_case():
    """Three clouds: two trees side by side, a cloud whose skeleton is empty, one tree."""
    two = DisjointTreeSkeleton([_hand_tree(0), _hand_tree(1, top=2.5, shift=(6.0, 0.5, 1.0))])
    one = DisjointTreeSkeleton([_hand_tree(0, top=4.0, shift=(-1.0, 0.25, 0.0))])
    none = DisjointTreeSkeleton([TreeSkeleton(0, {})])
    p0 = np.concatenate([_surface_points(two.skeletons[0], 2500, 1)[0], _surface_points(two.skeletons[1], 1700, 2)[0]])
    c0 = np.concatenate([_surface_points(two.skeletons[0], 2500, 1)[1], _surface_points(two.skeletons[1], 1700, 2)[1]])
    order = np.random.default_rng(5).permutation(len(p0))
    p2, c2 = _surface_points(one.skeletons[0], 3001, 3)
    p1 = np.random.default_rng(6).normal(size=(300, 3)).astype(F)
    return [(p0[order], c0[order], two), (p1, np.zeros((300, 1), F), none), (p2, c2, one)]


def _assert_inventory_equal(x, y):
    assert x.tree_columns == y.tree_columns and x.cell == y.cell and x.n_clouds == y.n_clouds
    np.testing.assert_array_equal(x.trees.view(np.uint64), y.trees.view(np.uint64))
    np.testing.assert_array_equal(x.branches.view(np.uint64), y.branches.view(np.uint64))
    np.testing.assert_array_equal(x.profile, y.profile)
    np.testing.assert_array_equal(x.orphans, y.orphans)


def test_batch_equals_the_single_calls(backend, tmp_path):
    from smart_tree_amd.segmentation import segment_cloud

    case = _batch_case()
    clouds = [Cloud(xyz=_t(p, backend), class_l=_t(c, backend)) for p, c, _ in case]
    skeletons = [s for _, _, s in case]
    singles = [I.measure_trees(c, s, cell=0.125, layers=24) for c, s in zip(clouds, skeletons)]
    batch = I.measure_trees(Cloud.collate(clouds), skeletons, cell=0.125, layers=24)
    assert len(batch) == 3 and batch.n_clouds == 3 and batch.trees[:, 0].tolist() == [0, 0, 2] and batch.trees[:, 1].tolist() == [0, 1, 0]
    assert batch.profile.shape == (3, 24) and batch.branches.shape == (12, 14) and batch.orphans.tolist() == [[0, 0, 5], [0, 1, 5], [2, 0, 5]]
    for one, part in zip(singles, batch.split()):
        _assert_inventory_equal(part, one)
    assert len(singles[1]) == 0 and singles[1].trees.shape == (0, len(I.tree_columns(1))) and singles[1].profile.shape == (0, 24)
    # the rows against the oracle on the ids the segmentation gave, and against the points themselves
    p0, c0, two = case[0]
    seg = segment_cloud(clouds[0], two)
    tree_id = seg.tree_id.cpu().numpy()
    assert (tree_id >= 0).all() and set(tree_id.tolist()) == {0, 1}
    want = io.tally(p0, tree_id, 2, c0.reshape(-1).astype(np.uint8), 2, cell=0.125, layers=24)
    inv = singles[0]
    assert inv.tree_columns == I.tree_columns(2)
    np.testing.assert_array_equal(inv.profile, want["profile"])
    np.testing.assert_array_equal(np.stack([inv.column("points_class_0"), inv.column("points_class_1")], 1), want["counts"])
    np.testing.assert_array_equal(inv.column("crown_area"), want["area_cells"] * 0.125 ** 2)
    for r in range(2):
        mine = p0[tree_id == r].astype(np.float64)
        assert inv.column("height")[r] == mine[:, 1].max() - mine[:, 1].min() and inv.column("base")[r] == mine[:, 1].min()
        assert inv.column("crown_width")[r] == max(np.ptp(mine[:, 0]), np.ptp(mine[:, 2])) and inv.column("points")[r] == len(mine)
        rows, _, _ = io.tree(_oracle_input(two.skeletons[r]), want["box"][r], want["counts"][r], want["area_cells"][r], want["profile"][r], 0.125)
        for name, value in rows.items():
            np.testing.assert_allclose(inv.column(name)[r], value, rtol=1e-9, err_msg=f"{r} {name}")
    assert 0.2 < inv.column("dbh")[0] < 0.5 and inv.branch_column("points").sum() == len(p0)
    # a segmentation the caller holds is the one used; the kinds of skeleton agree; a round trip through the files
    again = I.measure_trees(clouds[0], two, segmentation=seg, cell=0.125, layers=24)
    _assert_inventory_equal(again, inv)
    lone = I.measure_trees(clouds[2].xyz, case[2][2].skeletons[0], cell=0.125, layers=24)
    np.testing.assert_array_equal(lone.profile, singles[2].profile)
    assert lone.tree_columns == I.tree_columns(1) and lone.column("points")[0] == singles[2].column("points")[0]
    batch.save(tmp_path / "deep" / "inv")
    assert sorted(p.name for p in (tmp_path / "deep" / "inv").iterdir()) == ["branches.csv", "inventory.json", "trees.csv"]
    _assert_inventory_equal(I.TreeInventory.load(tmp_path / "deep" / "inv"), batch)
    _assert_inventory_equal(I.TreeInventory.load(tmp_path / "deep" / "inv" / "inventory.json"), batch)
    lines = (tmp_path / "deep" / "inv" / "trees.csv").read_text().splitlines()
    assert lines[0].split(",") == list(batch.tree_columns) and len(lines) == 4
    assert float(lines[1].split(",")[batch.tree_columns.index("wood_volume")]) == batch.column("wood_volume")[0]
    assert len((tmp_path / "deep" / "inv" / "branches.csv").read_text().splitlines()) == 13
    # labels that are no class (negative, NaN, above 254) keep their points out of the tree altogether
    labels = c0.copy()
    labels[::5], labels[1::5], labels[2::5] = -1.0, np.nan, 255.0
    part = I.measure_trees(Cloud(xyz=clouds[0].xyz, class_l=_t(labels, backend)), two, segmentation=seg, cell=0.125, layers=24)
    kept = np.arange(len(p0)) % 5 >= 3
    some = io.tally(p0[kept], tree_id[kept], 2, c0.reshape(-1).astype(np.uint8)[kept], 2, cell=0.125, layers=24)
    np.testing.assert_array_equal(part.profile, some["profile"])
    np.testing.assert_array_equal(np.stack([part.column("points_class_0"), part.column("points_class_1")], 1), some["counts"])
    assert part.column("points").sum() == kept.sum() and part.column("base")[0] == p0[kept & (tree_id == 0), 1].min()
    with pytest.raises(ValueError):
        I.measure_trees(Cloud.collate(clouds), skeletons[0])
    with pytest.raises(ValueError):
        I.measure_trees(clouds[0], two, cell=0.0)


def test_generated_tree_end_to_end(backend):
    from smart_tree_amd.dataset.synthetic import generate_trees
    from smart_tree_amd.segmentation import segment_cloud

    cloud, (truth,) = generate_trees([3], 6000, foliage_fraction=0.0, noise=0.002, max_depth=2, device=torch.device(backend))
    seg = segment_cloud(cloud, truth)
    inv = I.measure_trees(cloud, truth, segmentation=seg)
    xyz, tree_id = cloud.xyz.cpu().numpy(), seg.tree_id.cpu().numpy()
    assert len(inv) == 1 and (tree_id == 0).mean() > 0.99
    cls = None if cloud.class_l is None else cloud.class_l.cpu().numpy().reshape(-1).clip(0, 255).astype(np.uint8)
    want = io.tally(xyz, tree_id, 1, cls, 255)
    np.testing.assert_array_equal(inv.profile, want["profile"])
    assert inv.column("crown_area")[0] == want["area_cells"][0] * 0.1 * 0.1 and inv.column("points")[0] == want["counts"].sum() == (tree_id == 0).sum()
    up = xyz[tree_id == 0, 1].astype(np.float64)
    assert inv.column("height")[0] == up.max() - up.min() > 0 and inv.column("base")[0] == up.min()
    assert inv.column("crown_volume")[0] == want["profile"].sum() * 0.1 * 0.1 * 0.1 and inv.column("wood_volume")[0] > 0
    per, _ = io.branches(_oracle_input(truth))
    np.testing.assert_allclose(inv.column("wood_volume")[0], sum(m["volume"] for m in per.values()), rtol=1e-9)
    np.testing.assert_allclose(inv.branch_column("order"), [per[int(b)]["order"] for b in inv.branch_column("branch")])
    assert "cloud 0 tree 0: height" in I.summary(inv)


# ------------------------------------------------------------------------------------- 4: Pipeline and CLI ---
def _exact_pipeline(dev, trees, **kw):
    """The real pipeline with the network replaced by the exact medial vectors of seeded synthetic trees."""
    from smart_tree_amd.dataset.augmentations import AugmentationPipeline, CentreCloud
    from smart_tree_amd.pipeline import Pipeline
    from smart_tree_amd.skeleton.skeletonize import Skeletonizer

    class Exact:
        def __init__(self):
            self.by_size = {len(x): mv for x, mv in trees}
            self.by_size[sum(len(x) for x, _ in trees)] = np.concatenate([mv for _, mv in trees])

        def forward(self, cloud):
            n = len(cloud)
            return Cloud(xyz=cloud.xyz, rgb=cloud.rgb, medial_vector=_t(self.by_size[n], dev), class_l=torch.zeros((n, 1), device=dev),
                         seg_off=cloud.seg_off)

    sk = Skeletonizer(K=16, min_connection_length=0.02, minimum_graph_vertices=32, device=dev)
    sk.block_threads = 128 if dev.type == "cpu" else 0
    return Pipeline(AugmentationPipeline([CentreCloud()]), Exact(), sk, repair_skeletons=True, smooth_skeletons=True, smooth_kernel_size=11,
                    prune_skeletons=True, min_skeleton_radius=0.01, min_skeleton_length=0.02, device=dev, **kw)


@functools.lru_cache(maxsize=None)
def _tree_cloud(seed, n):
    from smart_tree_amd.synthetic import sample_tree_cloud

    c = sample_tree_cloud(n, seed=seed, scale=0.5, max_depth=2, noise=0.0)
    xyz, mv = np.ascontiguousarray(c["xyz"]), np.ascontiguousarray(c["medial_vector"])
    xyz.setflags(write=False)
    mv.setflags(write=False)
    return xyz, mv


_cloud = lambda dev, xyz: Cloud(xyz=_t(xyz, dev), rgb=torch.zeros((len(xyz), 3), device=dev))


def test_pipeline_measures_its_trees(backend, tmp_path, capsys):
    from smart_tree_amd.dataset.augmentations import CentreCloud
    from smart_tree_amd.segmentation import segment_cloud
    from smart_tree_amd.util.file import save_cloud, save_skeleton_npz

    trees = [_tree_cloud(2, 1700), _tree_cloud(7, 1500)]
    off = _exact_pipeline(backend, trees[:1], save_outputs=True, save_path=tmp_path / "off")
    np.random.seed(11)
    off.process_cloud(cloud=_cloud(backend, trees[0][0]))
    assert off.last_inventory is None and off.last_segmentation is None
    names = {"inventory.json", "trees.csv", "branches.csv"}
    assert not names & {p.name for p in (tmp_path / "off").iterdir()}
    pipe = _exact_pipeline(backend, trees, measure_trees=True, inventory_cell=0.05, inventory_layers=64, save_outputs=True, save_path=tmp_path / "on")
    np.random.seed(11)
    skeleton = pipe.process_cloud(cloud=_cloud(backend, trees[0][0]))
    inv = pipe.last_inventory
    assert pipe.last_segmentation is None and len(inv) >= 1 and inv.cell == 0.05 and inv.profile.shape[1] == 64
    assert {p.name for p in (tmp_path / "on").iterdir()} == names | {p.name for p in (tmp_path / "off").iterdir()}
    _assert_inventory_equal(I.TreeInventory.load(tmp_path / "on"), inv)
    # what the pipeline measured is measure_trees of the preprocessed cloud and the skeleton it returned
    centred = CentreCloud()(_cloud(backend, trees[0][0]))
    want = I.measure_trees(centred, skeleton, cell=0.05, layers=64)
    _assert_inventory_equal(inv, want)
    seg = segment_cloud(centred, skeleton)
    assert inv.column("points").sum() == (seg.tree_id >= 0).sum().item() > 1000 and (inv.column("height") > 0).any()
    # with segment_cloud on, its segmentation is the one measured
    both = _exact_pipeline(backend, trees, measure_trees=True, segment_cloud=True, inventory_cell=0.05, inventory_layers=64)
    both.process_cloud(cloud=_cloud(backend, trees[0][0]))
    _assert_inventory_equal(both.last_inventory, inv)
    # a batch of two: one call, the clouds' parts equal the single runs
    pipe.save_outputs = False
    pipe.process_cloud(cloud=_cloud(backend, trees[1][0]))
    second = pipe.last_inventory
    parts = pipe.process_clouds([_cloud(backend, x) for x, _ in trees])
    assert len(parts) == 2 and pipe.last_inventory.n_clouds == 2
    for one, part in zip((inv, second), pipe.last_inventory.split()):
        _assert_inventory_equal(part, one)
    # the command line on a saved cloud and the flat skeleton file, from the RAW cloud
    save_cloud(tmp_path / "raw.npz", _cloud(torch.device("cpu"), trees[0][0]))
    save_skeleton_npz(tmp_path / "sk.npz", skeleton)
    capsys.readouterr()
    cli = I.main([f"cloud={tmp_path / 'raw.npz'}", f"skeleton={tmp_path / 'sk.npz'}", f"out={tmp_path / 'cli'}", "centre=true", "cell=0.05",
                  "layers=64", f"device={backend}"])
    assert sorted(p.name for p in (tmp_path / "cli").iterdir()) == sorted(names)
    np.testing.assert_array_equal(cli.profile, inv.profile)
    np.testing.assert_array_equal(cli.trees[:, 2:].view(np.uint64), inv.trees[:, 2:].view(np.uint64))  # (the file's tree column is the tree's id)
    text = capsys.readouterr().out
    assert text.count("height") == len(inv) and "dbh" in text and "branches" in text
    with pytest.raises(SystemExit):
        I.main(["cloud=x.npz"])
    with pytest.raises(SystemExit):
        I.main(["cloud=x.npz", "skeleton=y.npz", "out=z", "colour=red"])
