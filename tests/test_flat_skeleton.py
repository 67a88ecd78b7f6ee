"""The one flat table of skeletons (`data_types/flat.py`) and the two helpers the entry points share: every consumer sees the same
branches, tubes and tree numbers, in the same order, whichever kind of skeleton it was given."""
import numpy as np
import pytest
import torch

from smart_tree_amd import inventory as I
from smart_tree_amd import refine as R
from smart_tree_amd import segmentation as S
from smart_tree_amd.config import cloud_command
from smart_tree_amd.data_types.branch import BranchSkeleton
from smart_tree_amd.data_types.cloud import Cloud
from smart_tree_amd.data_types.flat import FlatSkeletons, points_and_skeletons
from smart_tree_amd.data_types.tree import DisjointTreeSkeleton, TreeSkeleton
from smart_tree_amd.evaluate import load_any_skeleton
from smart_tree_amd.evaluation import skeleton_owners, skeleton_tubes
from smart_tree_amd.util.file import load_cloud, save_skeleton_npz

F = np.float32


def _branch(_id, parent, xyz, radii, column=True):
    br = BranchSkeleton(_id, parent, torch.tensor(xyz, dtype=torch.float32).reshape(-1, 3), torch.tensor(radii, dtype=torch.float32).reshape(-1, 1))
    if not column:
        br.radii = br.radii.reshape(-1)  # as `smooth` leaves them
    return br


def _two_trees():
    """Tree 0 (its own id 4): a trunk of three vertices, a branch of one vertex, a branch of two with radii [n].  Tree 1 (id 9): a
    branch without vertices and one of four."""
    first = TreeSkeleton(4, {0: _branch(0, -1, [[0, 0, 0], [0, 1, 0], [0.1, 2, 0]], [0.3, 0.25, 0.2]),
                             1: _branch(1, 0, [[0, 1, 0]], [0.1]),
                             2: _branch(2, 0, [[0, 1, 0], [1, 1.5, 0.25]], [0.07, 0.05], column=False)})
    second = TreeSkeleton(9, {0: _branch(0, -1, [], []),
                              3: _branch(3, 0, [[5, 0, 0], [5, 1, 0.5], [5.5, 2, 1], [6, 3, 1]], [0.2, 0.15, 0.1, 0.03])})
    return DisjointTreeSkeleton([first, second])


def _object_tubes(skeleton):
    tubes = skeleton.to_tubes()
    stack = lambda parts, shape: np.stack([p.numpy().reshape(shape) for p in parts]) if parts else np.zeros((0,) + shape, F)
    return (stack([t.a for t in tubes], (3,)), stack([t.b for t in tubes], (3,)), stack([t.r1 for t in tubes], ()), stack([t.r2 for t in tubes], ()))


# ------------------------------------------------------------------------------------------- 1: the three kinds ---
def test_the_three_kinds_give_one_table(tmp_path):
    both = _two_trees()
    save_skeleton_npz(tmp_path / "both.npz", both)
    file = load_any_skeleton(tmp_path / "both.npz")
    assert file["branches"].tolist() == [[4, 0, -1, 0, 3], [4, 1, 0, 3, 1], [4, 2, 0, 4, 2], [9, 0, -1, 6, 0], [9, 3, 0, 6, 4]]
    owners = [[0, 0, -1, 2], [0, 1, 0, 0], [0, 2, 0, 1], [1, 0, -1, 0], [1, 3, 0, 3]]
    in_file = [[4, 0, -1, 2], [4, 1, 0, 0], [4, 2, 0, 1], [9, 0, -1, 0], [9, 3, 0, 3]]
    for skeleton, obj, want in ((both, both, owners), (both.skeletons[0], both.skeletons[0], owners[:3]), (file, both, in_file)):
        flat = FlatSkeletons([skeleton])
        assert flat.xyz.dtype == np.float64 and flat.radii.dtype == np.float64 and flat.rows.dtype == np.int64
        assert np.column_stack([flat.rows[:, [1, 2, 3]], flat.tubes_of_row]).tolist() == want == skeleton_owners(skeleton).tolist()
        assert (flat.rows[:, 0] == 0).all() and flat.tube_off.tolist() == [0, sum(w[3] for w in want)]
        assert flat.tube_first.tolist() == np.concatenate([[0], np.cumsum([w[3] for w in want])]).tolist()
        got, views = flat.tubes(), skeleton_tubes(skeleton)
        for g, v, t in zip(got, views, _object_tubes(obj)):
            assert g.dtype == np.float64 and v.dtype == torch.float32 and t.dtype == F
            assert g.shape == t.shape and g.astype(F).tobytes() == t.tobytes() == v.numpy().tobytes()
            assert np.array_equal(g, t.astype(np.float64))  # float64 holds the float32 input exactly
    # what the objects carry besides: the trees' own ids, the shape of the radii, and a tree object without branches
    flat = FlatSkeletons([both])
    assert flat.label.tolist() == [4, 4, 4, 9, 9] and flat.column.tolist() == [True, True, False, True, True] and flat.trees == [[(0, 4), (1, 9)]]
    assert flat.tree_rows.tolist() == [[0, 0], [0, 1]] and flat.tree_of_branch.tolist() == [0, 0, 0, 1, 1]
    empty = FlatSkeletons([DisjointTreeSkeleton([TreeSkeleton(2, {})]), both.skeletons[1]])
    assert empty.trees == [[(0, 2)], [(0, 9)]] and empty.rows[:, 0].tolist() == [1, 1] and empty.tube_off.tolist() == [0, 0, 3]
    back = empty.rebuild(*empty.float32())
    assert [[(t._id, list(t.branches)) for t in sk.skeletons] for sk in back] == [[(2, [])], [(9, [0, 3])]]
    with pytest.raises(TypeError, match="segment_cloud: a TreeSkeleton"):
        FlatSkeletons([3.0], "segment_cloud")


# ---------------------------------------------------------------------------------- 2: a gapped, interleaved file ---
def _gapped_file():
    """Flat arrays whose trees are 7, 3, 7: a trunk of three vertices, another tree's trunk of two, the first tree's side branch."""
    xyz = np.array([[0, 0, 0], [0, 1, 0], [0, 2, 0], [3, 0, 0], [3, 1, 0], [0, 1, 0], [1, 1.5, 0]], F)
    radii = np.array([0.1, 0.1, 0.08, 0.08, 0.06, 0.05, 0.05], F)
    return {"branches": np.array([[7, 0, -1, 0, 3], [3, 0, -1, 3, 2], [7, 1, 0, 5, 2]]), "xyz": xyz, "radii": radii}


ROWS = [[0, 7, 0], [0, 3, 0], [0, 7, 1]]


def test_every_walk_lists_the_same_rows_in_the_same_order():
    file = _gapped_file()
    flat = FlatSkeletons([file])
    assert skeleton_owners(file)[:, :2].tolist() == [r[1:] for r in ROWS] and flat.rows[:, :3].tolist() == ROWS
    refined, fit = R.refine_skeleton(np.zeros((5, 3)), file, iterations=0)  # no iteration: no kernel
    assert fit.branches[:, :3].tolist() == ROWS and I.branch_table(flat)[0][:, :3].tolist() == ROWS
    assert fit.tube_off.tolist() == [0, 4] == flat.tube_off.tolist() and len(fit.tubes) == skeleton_tubes(file)[0].shape[0] == 4
    assert flat.tree_rows.tolist() == [[0, 7], [0, 3]] and flat.tree_of_branch.tolist() == [0, 1, 0]
    assert [t._id for t in refined.skeletons] == [7, 3] and [list(t.branches) for t in refined.skeletons] == [[0, 1], [0]]
    for tree, branch, parent, o, n in ((0, 0, -1, 0, 3), (1, 0, -1, 3, 2), (0, 1, 0, 5, 2)):
        got = refined.skeletons[tree].branches[branch]
        assert got.xyz.numpy().tobytes() == file["xyz"][o:o + n].tobytes() and got.radii.numpy().tobytes() == file["radii"][o:o + n].tobytes()
        assert got.radii.shape == (n, 1) and got.parent_id == parent


# ------------------------------------------------------------------------------- 3: the three features, one order ---
def _points_on_tubes(file, n, seed=5):
    """n points on the surfaces of the file's tubes, the same number on each (the last takes the remainder)."""
    a, b, r1, r2 = (t.numpy().astype(np.float64) for t in skeleton_tubes(file))
    rng = np.random.default_rng(seed)
    tube = np.minimum(np.arange(n) * len(a) // n, len(a) - 1)
    t, phi = rng.uniform(0.1, 0.9, n), rng.uniform(0, 2 * np.pi, n)
    d = (b - a)[tube]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    u = np.cross(d, [0.0, 0.0, 1.0])  # every tube of the file lies in the plane z = 0
    r = r1[tube] + t * (r2[tube] - r1[tube])
    return (a[tube] + t[:, None] * (b - a)[tube] + r[:, None] * (np.cos(phi)[:, None] * u + np.sin(phi)[:, None] * [0.0, 0.0, 1.0])).astype(F)


def test_segmentation_fit_and_inventory_agree_row_by_row(backend):
    file = _gapped_file()
    pts = torch.from_numpy(_points_on_tubes(file, 200)).to(backend)
    flat = FlatSkeletons([file])
    seg = S.segment_cloud(pts, file)
    _, fit = R.refine_skeleton(pts, file, iterations=1)
    inv = I.measure_trees(pts, file)
    want = [r + [p] for r, p in zip(ROWS, (-1, -1, 0))]
    assert seg.branches[:, :4].tolist() == want and fit.branches[:, :4].tolist() == want and inv.branches[:, :4].tolist() == want
    assert inv.trees[:, :2].tolist() == [[0, 7], [0, 3]]
    # the fit's tubes are in the segmentation's order: the points of a branch's tubes are the branch's points
    per_branch = np.add.reduceat(fit.tubes[:, 0], flat.tube_first[:-1])
    print("points per tube", fit.tubes[:, 0].tolist(), "status", fit.tubes[:, 7].tolist(), "per branch", fit.branches[:, 6].tolist())
    assert per_branch.tolist() == fit.branches[:, 6].tolist() and per_branch.sum() > 0
    assert seg.branches[:, 5].tolist() == per_branch.tolist()  # and they are the points the segmentation counted there


# ---------------------------------------------------------------------------------------- 4: the shared prologue ---
def test_points_and_skeletons():
    sk = _two_trees()
    xyz = np.arange(12, dtype=np.float64).reshape(4, 3)
    for name, call in (("segment_cloud", S.segment_cloud), ("refine_skeleton", R.refine_skeleton), ("measure_trees", I.measure_trees)):
        with pytest.raises(ValueError, match=rf"^{name}: 2 skeleton\(s\) for 1 cloud\(s\); a collated Cloud takes a list, one per cloud$"):
            call(xyz, [sk, sk])
        with pytest.raises(ValueError, match=rf"^{name}: 1 skeleton\(s\) for 2 cloud\(s\)"):
            call(Cloud.collate([Cloud(xyz=torch.zeros(3, 3)), Cloud(xyz=torch.ones(2, 3))]), sk)
    batch = Cloud.collate([Cloud(xyz=torch.zeros(3, 3)), Cloud(xyz=torch.ones(2, 3))])
    pts, seg_off, skeletons, many, n_clouds = points_and_skeletons(batch, (sk, sk.skeletons[0]), None, "caller")
    assert pts.shape == (5, 3) and seg_off.tolist() == [0, 3, 5] and skeletons == [sk, sk.skeletons[0]] and many and n_clouds == 2
    pts, seg_off, skeletons, many, n_clouds = points_and_skeletons(xyz, sk, "cpu", "caller")
    assert pts.dtype == torch.float32 and pts.is_contiguous() and pts.tolist() == xyz.tolist() and pts.device.type == "cpu"
    assert seg_off is None and skeletons == [sk] and not many and n_clouds == 1


# ------------------------------------------------------------------------------------------ 5: the shared command ---
@pytest.mark.parametrize("module", (S, R, I), ids=("segmentation", "refine", "inventory"))
def test_cloud_command(module, tmp_path):
    usage = module.USAGE
    assert usage.startswith(f"usage: python -m {module.__name__} cloud=")
    with pytest.raises(SystemExit) as unknown:
        module.main(["cloud=x.npz", "skeleton=y.npz", "out=z", "colour=red"])
    assert str(unknown.value) == usage + "  (unknown: colour)"
    for args in (["cloud=x.npz", "skeleton=y.npz"], ["cloud=x.npz", "out=z"], ["skeleton=y.npz", "out=z"], []):
        with pytest.raises(SystemExit) as missing:
            module.main(args)
        assert str(missing.value) == usage
    xyz = np.random.default_rng(2).uniform(-1, 3, (50, 3)).astype(F)
    np.savez(tmp_path / "cloud.npz", xyz=xyz, rgb=np.zeros_like(xyz))
    args = [f"cloud={tmp_path / 'cloud.npz'}", "skeleton=y.npz", "out=z", "device=cpu"]
    cfg, dev, cloud = cloud_command(args, module.DEFAULTS, usage)
    assert dev == torch.device("cpu") and cloud.xyz.numpy().tobytes() == xyz.tobytes() and cfg["skeleton"] == "y.npz" and cfg["centre"] is False
    assert set(cfg) == set(module.DEFAULTS) and module.DEFAULTS["cloud"] is None  # the module's defaults are not written to
    cfg, dev, centred = cloud_command(args + ["centre=true"], module.DEFAULTS, usage)
    lo, hi = centred.xyz.min(0).values, centred.xyz.max(0).values
    assert cfg["centre"] is True and abs(float(lo[1])) < 1e-6 and abs(float(lo[0] + hi[0])) < 1e-5 and abs(float(lo[2] + hi[2])) < 1e-5
    assert torch.allclose(centred.xyz - centred.xyz[0], load_cloud(tmp_path / "cloud.npz").xyz - torch.from_numpy(xyz[0]), atol=1e-6)
