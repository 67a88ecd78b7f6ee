"""Synthetic trees generated on the device (csrc/synthetic.hip, smart_tree_amd/dataset/synthetic.py, dataset/generate.py, the
`config=training_synthetic` run) against tests/synth_oracle.py: the random stream and every integer output bit for bit, the
float outputs to the float32-restatement bound of DESIGN.md section 7 item 7, then the label geometry, the skeleton, the dataset
and the commands."""
import ctypes
import json
import math

import numpy as np
import pytest
import torch

import synth_oracle as so
from smart_tree_amd import _lib
from smart_tree_amd.dataset import synthetic as S
from smart_tree_amd.synthetic import grow_tree

INT_KEYS = ("class_l", "segment", "branch_ids")
FLOAT_KEYS = ("xyz", "medial_vector")

# (trees, points per tree, max_depth, foliage fraction per tree)
BATCHES = {
    "one_point": (1, [1], 0, [0.0]),
    "one_tree": (1, [257], 2, [0.3]),
    "straddle": (3, [100, 0, 613], 3, [0.0, 0.5, 1.0]),
    "many": (64, [40] * 64, 1, [0.25] * 64),
}
_CASES = {}


def _case(name, noise=0.002, scale=1.0):
    """Tables, arguments and both oracle evaluations of a batch: computed once, shared, never modified."""
    key = (name, noise, scale)
    if key not in _CASES:
        B, counts, depth, fol = BATCHES[name]
        seeds = [(0x9E3779B97F4A7C15 * (s + 1) + 12345) & ((1 << 64) - 1) for s in range(B)]  # both key halves in use
        tables = [S.segment_table(grow_tree(s & 0xFFFFFFFF, scale, depth)) for s in seeds]
        args = (tables, counts, seeds, [S.foliage_threshold(f) for f in fol], [noise] * B, [0.08 * scale] * B)
        o64, o32 = so.sample_batch(*args, dtype=np.float64), so.sample_batch(*args, dtype=np.float32)
        for o in (o64, o32):
            for v in o.values():
                v.setflags(write=False)
        _CASES[key] = (args, o64, o32)
    return _CASES[key]


def _bound(o64, o32, key, rows=slice(None)):
    """max(1e-6 m, 4 x the float32 restatement's distance from the float64 oracle)."""
    if o64[key][rows].size == 0:
        return 1e-6
    return max(1e-6, 4.0 * float(np.abs(o32[key][rows].astype(np.float64) - o64[key][rows]).max()))


def _np(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


# ------------------------------------------------------------------------------------------------ 1. random stream ---
PHILOX_KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@pytest.mark.parametrize("counter,key,want", PHILOX_KAT)
def test_philox_known_answers(backend, counter, key, want):
    c, k, out = (ctypes.c_uint32 * 4)(*counter), (ctypes.c_uint32 * 2)(*key), (ctypes.c_uint32 * 4)()
    _lib.lib().st_synth_philox(c, k, out)
    assert tuple(out) == want
    assert tuple(int(x) for x in so.philox4x32_10(np.asarray([counter]), key)[0]) == want


# ------------------------------------------------------------------------------------- 2. / 3. against the oracle ---
@pytest.mark.parametrize("name", list(BATCHES))
def test_outputs_against_the_oracle(backend, name):
    args, o64, o32 = _case(name)
    res, pt_off, tab_off = S.synth_points(*args, backend)
    got = _np(res)
    for k in INT_KEYS:  # bit exact
        np.testing.assert_array_equal(got[k], o64[k], err_msg=k)
        np.testing.assert_array_equal(o32[k], o64[k], err_msg=k)
    for k in FLOAT_KEYS:
        err, bound = float(np.abs(got[k].astype(np.float64) - o64[k]).max()), _bound(o64, o32, k)
        print(f"{name} {backend} {k}: max error {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (k, err, bound)
    B, counts, _, fol = BATCHES[name]
    assert pt_off.tolist() == np.concatenate([[0], np.cumsum(counts)]).tolist()
    for s in range(B):
        cls = got["class_l"][pt_off[s]:pt_off[s + 1]]
        seg = got["segment"][pt_off[s]:pt_off[s + 1]]
        if fol[s] == 0.0:
            assert not cls.any()  # a threshold of 0: no foliage
        if fol[s] == 1.0:
            assert cls.all() and len(cls) > 0  # fraction 1: only foliage
        assert ((seg[cls == 0] >= tab_off[s]) & (seg[cls == 0] < tab_off[s + 1])).all() and (seg[cls == 1] == -1).all()
    if name == "one_tree":
        assert 0 < got["class_l"].sum() < 257 and len(np.unique(got["segment"])) > 5
    if name == "straddle":
        assert pt_off[1] == pt_off[2] == 100 and (got["segment"][:100] < tab_off[1]).all()
    # null outputs: the others unchanged; a second call: the same bits
    only, _, _ = S.synth_points(*args, backend, outputs={"medial_vector": None, "class_l": None, "branch_ids": None, "segment": None})
    assert only["medial_vector"] is None and torch.equal(only["xyz"], res["xyz"])
    again, _, _ = S.synth_points(*args, backend)
    assert all(torch.equal(again[k], res[k]) for k in res)


def test_no_tips_means_no_foliage(backend):
    (tables, counts, seeds, _, noise, sigma), _, _ = _case("one_tree")
    bare = [S.SegmentTable(**{**tables[0].__dict__, "tips": np.zeros((0, 3), np.float32)})]
    res, _, _ = S.synth_points(bare, counts, seeds, [0xFFFFFFFF], noise, sigma, backend)
    assert not res["class_l"].any() and (res["segment"] >= 0).all()


# ------------------------------------------------------------------------------------------------ 4. label geometry ---
def test_label_geometry(backend):
    n, depth, scale = 20_000, 3, 1.0
    table = S.segment_table(grow_tree(11, scale, depth))
    run = lambda noise: _np(S.synth_points([table], [n], [11], [S.foliage_threshold(0.3)], [noise], [0.08], backend)[0])
    clean, noisy = run(0.0), run(0.002)
    args = ([table], [n], [11], [S.foliage_threshold(0.3)], [0.0], [0.08])
    o64, o32 = so.sample_batch(*args, dtype=np.float64), so.sample_batch(*args, dtype=np.float32)
    branch = clean["class_l"] == 0
    bound = _bound(o64, o32, "xyz") + _bound(o64, o32, "medial_vector")  # the checks add the two outputs
    seg = clean["segment"][branch]
    a, b = table.a[seg].astype(np.float64), table.b[seg].astype(np.float64)
    ra, rb = table.ra[seg].astype(np.float64), table.rb[seg].astype(np.float64)
    xyz, mv = clean["xyz"][branch].astype(np.float64), clean["medial_vector"][branch].astype(np.float64)
    ab = b - a
    t = ((xyz + mv - a) * ab).sum(1) / (ab * ab).sum(1)
    off_axis = np.linalg.norm(xyz + mv - (a + t[:, None] * ab), axis=1)
    rad_err = np.abs(np.linalg.norm(mv, axis=1) - (ra * (1 - t) + rb * t))
    ortho = np.abs((mv * ab).sum(1) / np.linalg.norm(ab, axis=1))
    print(f"{backend}: off axis {off_axis.max():.3e}, radius {rad_err.max():.3e}, orthogonality {ortho.max():.3e}, bound {bound:.3e}; "
          f"t in [{t.min():.4f}, {t.max():.4f}], {int(branch.sum())} branch points")
    assert 0.6 * n < branch.sum() < 0.8 * n
    assert t.min() >= -bound and t.max() <= 1 + bound
    assert off_axis.max() <= bound and rad_err.max() <= bound and ortho.max() <= bound
    assert (clean["branch_ids"][branch] == table.branch[seg]).all()
    fol = ~branch
    assert not clean["medial_vector"][fol].any() and (clean["branch_ids"][fol] == -1).all() and (clean["segment"][fol] == -1).all()
    # the same stream with noise: the classes and segments stay, the displacement is the noise
    for k in INT_KEYS:
        np.testing.assert_array_equal(noisy[k], clean[k])
    np.testing.assert_array_equal(noisy["medial_vector"], clean["medial_vector"])
    np.testing.assert_array_equal(noisy["xyz"][fol], clean["xyz"][fol])
    delta = noisy["xyz"][branch].astype(np.float64) - xyz
    m = int(branch.sum())
    print(f"noise: mean {delta.mean(0)}, std {delta.std(0)}, standard error {0.002 / math.sqrt(m):.3e}")
    assert (np.abs(delta.mean(0)) <= 5 * 0.002 / math.sqrt(m)).all()
    assert np.abs(delta.std(0) / 0.002 - 1).max() < 0.05
    spread = clean["xyz"][fol].astype(np.float64) - table.tips[(so.draw_words(n, 11)[0][fol, 1] % len(table.tips)).astype(int)]
    assert np.abs(spread.std(0) / 0.08 - 1).max() < 0.05


# ----------------------------------------------------------------------------------------------------- 5. refusals ---
def _raw_call(backend, tab_off, tip_off, pt_off, B, n_out=64):
    """st_synth_points_seg with the offsets as given; returns (rc, outputs) with the outputs filled with a sentinel before."""
    table = S.segment_table(grow_tree(1, 1.0, 1))
    dev = lambda x: torch.from_numpy(x).to(backend)
    rows, cdf, tips = dev(table.rows()), dev(table.cdf.view(np.int32)), dev(table.tips)
    outs = [torch.full((n_out, 3), -7.0, device=backend), torch.full((n_out, 3), -7.0, device=backend),
            torch.full((n_out,), -7.0, device=backend), torch.full((n_out,), -7, dtype=torch.int32, device=backend),
            torch.full((n_out,), -7, dtype=torch.int32, device=backend)]
    i32 = lambda v: np.asarray(v, dtype=np.int32)
    tab_off, tip_off, pt_off = i32(tab_off), i32(tip_off), i32(pt_off)
    seeds, thr = np.zeros(max(B, 1), np.uint64), np.zeros(max(B, 1), np.uint32)
    ns = np.zeros(max(B, 1), np.float32)
    h = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    rc = _lib.lib().st_synth_points_seg(_lib.ptr(rows), h(tab_off), _lib.ptr(cdf), _lib.ptr(tips), h(tip_off), h(pt_off), B, h(seeds),
                                        h(thr), h(ns), h(ns), *[_lib.ptr(o) for o in outs], _lib.stream(backend))
    if backend.type == "cuda":
        torch.cuda.synchronize()
    return rc, outs


@pytest.mark.parametrize("what", ["too_many", "decreasing", "negative", "no_segments"])
def test_refusals_write_nothing(backend, what):
    S_, T_ = 3, 2  # grow_tree(1, max_depth=1): 3 or 4 segments; the offsets below stay inside the table either way
    if what == "too_many":
        off = list(range(66))
        rc, outs = _raw_call(backend, [0] * 66, [0] * 66, off, 65, n_out=65)
        text = "trees per call"
    elif what == "decreasing":
        rc, outs = _raw_call(backend, [0, 1, 2], [0, 1, 2], [0, 40, 30], 2)
        text = "decreasing offset"
    elif what == "negative":
        rc, outs = _raw_call(backend, [-1, 1], [0, 1], [0, 10], 1)
        text = "negative offset"
    else:
        rc, outs = _raw_call(backend, [0, S_, S_], [0, T_, T_], [0, 10, 20], 2)
        text = "points and no segments"
    assert rc != 0
    with pytest.raises(_lib.StError, match=text):
        _lib.check(rc)
    for o in outs:
        assert bool((o == -7).all())
    if what == "too_many":
        args = _case("one_point")[0]
        with pytest.raises(_lib.StError, match="trees per call"):
            S.synth_points(args[0] * 65, [1] * 65, [0] * 65, [0] * 65, [0.0] * 65, [0.0] * 65, backend)
        with pytest.raises(ValueError, match="at most 64"):
            S.generate_trees(list(range(65)), 1, max_depth=0, device=backend)


# ----------------------------------------------------------------------------------------------------- 6. skeleton ---
def test_tree_skeleton_structure():
    segs = grow_tree(seed=3, max_depth=3)
    sk = S.tree_skeleton(segs, tree_id=5)
    branch, branch_parent, members = S.segment_branches(segs)
    assert sk._id == 5 and sorted(sk.branches) == list(range(len(members))) and sk.branches[0].parent_id == -1
    assert sorted(j for m in members for j in m) == list(range(len(segs.a)))  # every segment in exactly one branch
    assert list(dict.fromkeys(branch.tolist())) == list(range(len(members)))  # ids in first-appearance order
    parent = S.segment_parents(segs)
    assert parent[0] == -1 and (parent[1:] < np.arange(1, len(parent))).all() and (segs.depth[parent[1:]] == segs.depth[1:] - 1).all()
    np.testing.assert_array_equal(segs.a[1:], segs.b[parent[1:]])  # a child starts where its parent ends
    for bid, b in sk.branches.items():
        assert len(b) == len(members[bid]) + 1 and b.radii.shape == (len(b), 1) and b.xyz.dtype == torch.float32
        if bid:
            assert b.parent_id < bid  # parents precede children
            assert (sk.branches[b.parent_id].xyz == b.xyz[0]).all(1).any()  # the first vertex is a vertex of the parent
            assert float(b.radii[0]) == np.float32(segs.ra[members[bid][0]])
    total = float(np.linalg.norm(segs.b - segs.a, axis=1).sum())
    assert float(sk.length) == pytest.approx(total, rel=1e-5)
    table = S.segment_table(segs)
    np.testing.assert_array_equal(table.branch, branch)
    assert table.cdf.dtype == np.uint32 and table.cdf[-1] == 0xFFFFFFFF and (np.diff(table.cdf.astype(np.int64)) >= 0).all()
    area = np.pi * (segs.ra + segs.rb) * np.linalg.norm(segs.b - segs.a, axis=1)
    np.testing.assert_array_equal(table.cdf[:-1], np.floor(4294967296.0 * np.cumsum(area)[:-1] / area.sum()).astype(np.uint32))
    assert len(table.tips) == int(segs.is_tip.sum()) and table.rows().shape == (len(segs.a), 16)
    assert np.abs((table.u * table.v).sum(1)).max() < 1e-6 and np.abs(np.linalg.norm(table.u, axis=1) - 1).max() < 1e-6


def test_ground_truth_against_itself_is_perfect(backend):
    from smart_tree_amd.evaluation import evaluate_skeleton

    sk = S.tree_skeleton(grow_tree(seed=3, max_depth=3))
    r = evaluate_skeleton(sk, sk, spacing=0.01, device=backend)
    assert len(r["f1"]) == 10 and r["f1"] == [1.0] * 10 and r["auc"] == 1.0


def test_segment_labels_land_on_the_nearest_tube(backend):
    """Depth 0 (one tube, no junction), noise 0, t in [0.2, 0.8]: the projection on the tube is the label's axis point."""
    from smart_tree_amd.util.queries import pts_to_nearest_tube

    n = 2000
    cloud, (sk,) = S.generate_trees([21], n, noise=0.0, max_depth=0, device=backend)
    table = S.segment_table(grow_tree(21, 1.0, 0))
    args = ([table], [n], [21], [0], [0.0], [0.08])
    o64, o32 = so.sample_batch(*args, dtype=np.float64), so.sample_batch(*args, dtype=np.float32)
    keep = torch.from_numpy((o64["t"] >= 0.2) & (o64["t"] <= 0.8)).to(backend)
    assert 0.5 * n < int(keep.sum()) < 0.7 * n and len(sk.branches) == 1
    vec, idx, rad = pts_to_nearest_tube(cloud.xyz[keep], sk.to_tubes())
    err = float((vec.norm(dim=1) - rad).abs().max())
    bound = _bound(o64, o32, "xyz")
    print(f"{backend}: | |vector| - radius | {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    assert float((vec - cloud.medial_vector[keep]).abs().max()) <= bound + _bound(o64, o32, "medial_vector")


def test_nearest_labels(backend):
    """labels="nearest": the branch points' vectors come from st_points_to_nearest_tube on the noised points; everything else is
    the "segment" cloud."""
    from smart_tree_amd.util.queries import nearest_tube_device

    kw = dict(noise=0.002, foliage_fraction=0.3, max_depth=2, device=backend)
    seg_cloud, _ = S.generate_trees([5, 6], [700, 300], labels="segment", **kw)
    near, _ = S.generate_trees([5, 6], [700, 300], labels="nearest", **kw)
    assert torch.equal(near.xyz, seg_cloud.xyz) and torch.equal(near.class_l, seg_cloud.class_l)
    assert near.seg_off.tolist() == [0, 700, 1000]
    fol = near.class_l.view(-1) == 1
    assert not near.medial_vector[fol].any()
    for s, (lo, hi) in enumerate(((0, 700), (700, 1000))):
        t = S.segment_table(grow_tree((5, 6)[s], 1.0, 2))
        sel = (~fol[lo:hi]).nonzero().view(-1) + lo
        want, _, _ = nearest_tube_device(near.xyz[sel], *[torch.from_numpy(x).to(backend) for x in (t.a, t.b, t.ra, t.rb)])
        assert torch.equal(near.medial_vector[sel], want)
    diff = (near.medial_vector - seg_cloud.medial_vector)[~fol].norm(dim=1)
    assert 0 < float(diff.median()) < 0.01  # the noise moved the labels by about its size


# ------------------------------------------------------------------------------------------------------ 7. dataset ---
FEATS = (["xyz"], ["radius", "direction", "class_l"])
TREE = dict(n_points=3000, scale=0.6, noise=0.002, foliage_fraction=0.3, max_depth=2)


@pytest.fixture
def emu(request, monkeypatch):
    """The CPU build of the kernels, for the checks that are about host logic."""
    monkeypatch.setattr(_lib, "_LIB", request.getfixturevalue("emu_lib"))
    monkeypatch.setattr(_lib, "_ALLOW_HOST_POINTERS", True)
    return torch.device("cpu")


def _same_item(a, b):
    (ia, ta), ca, ma, na = a
    (ib, tb), cb, mb, nb = b
    return torch.equal(ia, ib) and torch.equal(ta, tb) and torch.equal(ca, cb) and torch.equal(ma, mb) and na == nb


def test_dataset_items_match_tree_dataset(backend, tmp_path):
    from smart_tree_amd.dataset.dataset import TreeDataset
    from smart_tree_amd.util.file import save_cloud

    ds = S.SyntheticTreeDataset(0.05, "validation", 3, *FEATS, seed=4, device=backend, **TREE)
    assert len(ds) == 3
    item = ds[1]
    save_cloud(tmp_path / "tree.npz", ds.cloud(1))
    (tmp_path / "split.json").write_text(json.dumps({"train": [], "validation": ["tree.npz"], "test": []}))
    ref = TreeDataset(0.05, tmp_path / "split.json", tmp_path, "validation", *FEATS, device=backend)[0]
    (inp, tgt), coords, mask, name = item
    (rinp, rtgt), rcoords, rmask, _ = ref
    assert name == f"synthetic_validation_{S.item_seed(4, 'validation', 1, 0)}"
    for got, want in ((inp, rinp), (tgt, rtgt), (coords, rcoords), (mask, rmask)):
        assert got.dtype == want.dtype and got.shape == want.shape and got.device == want.device
        assert torch.equal(got, want)
    assert inp.shape[1] == 3 and tgt.shape[1] == 5 and coords.shape[1] == 4 and 100 < inp.shape[0] < 3000
    assert set(tgt[:, 4].unique().tolist()) == {0.0, 1.0}
    with pytest.raises(IndexError):
        ds[3]
    with pytest.raises(ValueError, match="mode"):
        S.SyntheticTreeDataset(0.05, "validate", 3, *FEATS)


def test_dataset_determinism(emu):
    make = lambda mode, seed=4: S.SyntheticTreeDataset(0.05, mode, 2, *FEATS, seed=seed, device=emu, **TREE)
    val, train, twin = make("validation"), make("train"), make("train")
    v0, t0 = val[0], train[0]
    assert not _same_item(t0, train[1]) and t0[3] != v0[3]
    for ds in (val, train, twin):
        ds.set_epoch(1)
    assert _same_item(val[0], v0)  # validation trees are fixed
    t1 = train[0]
    assert not _same_item(t1, t0) and t1[3] != t0[3]  # fresh trees in a new epoch
    assert _same_item(twin[0], t1)  # the same arguments: the same bits
    train.set_epoch(0)
    assert _same_item(train[0], t0)
    assert not _same_item(make("train", seed=5)[0], t0)
    seeds = {S.item_seed(4, m, i, e) for m in S.MODES for i in range(8) for e in range(4)}
    assert len(seeds) == 96 and all(0 <= s < 2 ** 63 for s in seeds)


# --------------------------------------------------------------------------------------------- 8. command and run ---
def test_generate_command_feeds_dataset_and_evaluate(backend, tmp_path, capsys):
    from smart_tree_amd import evaluate
    from smart_tree_amd.dataset import generate
    from smart_tree_amd.dataset.dataset import TreeDataset
    from smart_tree_amd.util.file import load_cloud, load_skeleton

    out = tmp_path / "trees"
    res = generate.main([f"out={out}", "trees=4", "points=3000", "max_depth=2", "seed=10", "split=[0.5,0.25,0.25]", f"device={backend}"])
    split = json.loads((out / "split.json").read_text())
    assert split == res["split"] == {"train": ["tree_10.npz", "tree_11.npz"], "validation": ["tree_12.npz"], "test": ["tree_13.npz"]}
    c = load_cloud(out / "tree_12.npz")
    assert len(c) == 3000 and c.rgb.shape == (3000, 3) and c.medial_vector.shape == (3000, 3) and c.class_l.shape == (3000, 1)
    assert c.branch_ids.shape == (3000, 1) and 0.2 < float(c.class_l.mean()) < 0.4
    again, _ = S.generate_trees([12], 3000, foliage_fraction=0.3, max_depth=2, device=backend)  # a tree does not depend on its batch
    assert torch.equal(again.xyz.cpu(), c.xyz)
    ds = TreeDataset(0.05, out / "split.json", out, "train", *FEATS, device=backend)
    (inp, tgt), coords, mask, name = ds[1]
    assert len(ds) == 2 and name == "tree_11.npz" and inp.shape[1] == 3 and tgt.shape[1] == 5 and coords.shape[0] == inp.shape[0]
    sk = load_skeleton(out / "tree_10_skeleton.npz")
    assert len(sk.branches) == len(S.tree_skeleton(grow_tree(10, 1.0, 2)).branches)
    r = evaluate.main([f"pred={out / 'tree_10_skeleton.npz'}", f"gt={out / 'tree_10_skeleton.npz'}", "spacing=0.02",
                       f"out={tmp_path / 'm.json'}", f"device={backend}"])
    assert r["trees"]["tree_10_skeleton"]["f1"] == [1.0] * 10
    with pytest.raises(SystemExit):
        generate.main(["trees=4"])


def _run_args(run_dir, device, **kw):
    a = {"config": "training_synthetic", "num_epoch": 2, "batch_size": 2, "train_trees": 2, "validation_trees": 1, "test_trees": 1,
         "points": 1500, "scale": 0.6, "max_depth": 2, "voxel_size": 0.05, "fp16": False, "capture_output": 0, "device": device,
         "run_dir": run_dir}
    a.update(kw)
    return [f"{k}={v}" for k, v in a.items()]


def test_synthetic_training_run_and_resume(backend, tmp_path):
    from smart_tree_amd.model import train as T
    from smart_tree_amd.model.tracker import read_metrics

    whole, part = tmp_path / "whole", tmp_path / "part"
    T.main(_run_args(whole, backend))
    lines = read_metrics(whole / "metrics.jsonl")
    assert [r["epoch"] for r in lines] == [0, 1]
    assert all(math.isfinite(v) for r in lines for v in r["train"].values())
    assert lines[0]["train"] != lines[1]["train"]
    assert lines[0]["validation"].keys() == lines[0]["train"].keys() == {"radius", "direction", "class_l", "total"}
    T.main(_run_args(part, backend, num_epoch=1))
    assert len(read_metrics(part / "metrics.jsonl")) == 1
    T.main(_run_args("elsewhere", backend, resume=part))
    resumed = read_metrics(part / "metrics.jsonl")
    assert len(resumed) == 2 and resumed[0]["train"] == lines[0]["train"]
    assert resumed[1]["train"] == lines[1]["train"] and resumed[1]["validation"] == lines[1]["validation"]


def test_config_selection_and_required_keys(tmp_path):
    from smart_tree_amd import config as C
    from smart_tree_amd.model import train as T

    with pytest.raises(ValueError, match="directory and json_path not set: pass directory=... json_path=..."):
        T.load_training_config([])
    with pytest.raises(ValueError, match="no bundled configuration"):
        T.load_training_config(["config=nope"])
    cfg = T.load_training_config(["config=training_synthetic", "device=cpu", "points=1234", "train_trees=5"])
    assert "directory" not in cfg and "json_path" not in cfg
    sets = [C.instantiate(cfg[f"{m}_dataset"]) for m in S.MODES]
    assert all(isinstance(ds, S.SyntheticTreeDataset) for ds in sets) and [ds.mode for ds in sets] == list(S.MODES)
    assert [len(ds) for ds in sets] == [5, 8, 8] and sets[0].tree_args["n_points"] == 1234 and sets[0].voxel_size == 0.01
    raw, base = C.load_yaml(T.CONF.parent / "training_synthetic.yaml"), C.load_yaml(T.CONF)
    same = [k for k in base if k not in ("directory", "json_path", "train_dataset", "validation_dataset", "test_dataset")]
    assert all(raw[k] == base[k] for k in same)  # the same run
    # a configuration that still refers to a key must be given it
    (tmp_path / "config.yaml").write_text("directory: ???\njson_path: ???\nx: ${json_path}\ndevice: cpu\n")
    with pytest.raises(ValueError, match="^train-smart-tree: json_path not set"):
        T.load_training_config([f"resume={tmp_path}"])
