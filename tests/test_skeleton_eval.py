"""Skeleton evaluation (csrc/skeleton_eval.hip, smart_tree_amd/evaluation, smart_tree_amd/evaluate.py) against
tests/eval_oracle.py: sampling and matching bit for bit, the tally exactly (hits) or to float64 re-association (sums),
then properties of the metrics and the command line."""
import json
import math

import numpy as np
import pytest
import torch

import eval_oracle as eo
from smart_tree_amd import _lib
from smart_tree_amd.data_types.branch import BranchSkeleton
from smart_tree_amd.data_types.tree import DisjointTreeSkeleton, TreeSkeleton
from smart_tree_amd.data_types.tube import sample_tubes, sample_tubes_device, sample_tubes_host
from smart_tree_amd.evaluation import DEFAULT_THRESHOLDS, evaluate_skeleton, match, skeleton_tubes
from smart_tree_amd.synthetic import grow_tree

THR10 = [0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 1.0]


def _tubes(m, seed, special=False):
    rng = np.random.RandomState(seed)
    a = (rng.rand(m, 3) * 4).astype(np.float32)
    b = (a + rng.normal(0, 0.15, (m, 3))).astype(np.float32)
    r1 = (0.01 + 0.1 * rng.rand(m)).astype(np.float32)
    r2 = (r1 * (0.7 + 0.3 * rng.rand(m))).astype(np.float32)
    if special and m >= 3:
        b[0] = a[0]  # zero length: no samples; a point for the matcher
        b[m // 2] = a[m // 2] + np.float32([0.0, 0.004, 0.0])  # shorter than the spacing: one sample
        b[m - 1, 1] = np.nan  # NaN end point: no samples, never a winner
    return a, b, r1, r2


def _dev(backend, *arrays):
    return [torch.from_numpy(np.array(x)).to(backend) for x in arrays]  # a copy: the shared cases are read-only


# ------------------------------------------------------------------------------------------------ 1. sampling ---
@pytest.mark.parametrize("m,spacing,special", [(1, 0.01, False), (37, 0.01, True), (1300, 0.01, True)])
def test_sampling_bit_exact(backend, m, spacing, special):
    a, b, r1, r2 = _tubes(m, seed=m, special=special)
    count, off, pts, rad, tube_of = eo.sample_tubes(a, b, r1, r2, spacing)
    gp, gr, gt, gc, go = sample_tubes_device(*_dev(backend, a, b, r1, r2), spacing)
    np.testing.assert_array_equal(gc.cpu().numpy(), count)
    np.testing.assert_array_equal(go.cpu().numpy(), off)
    np.testing.assert_array_equal(gt.cpu().numpy(), tube_of)
    np.testing.assert_array_equal(gp.cpu().numpy(), pts)
    np.testing.assert_array_equal(gr.cpu().numpy(), rad)
    if special:
        assert count[0] == 0 and count[m - 1] == 0 and count[m // 2] == 1
        assert off[1] == off[0] == 0 and off[m - 1] == count[:m - 1].sum() == len(pts)
    if m == 1300:
        assert 15000 < len(pts) < 40000


def test_sampling_refuses_bad_spacing(backend):
    a, b, r1, r2 = _dev(backend, *_tubes(5, seed=1))
    for spacing in (0.0, -0.01, float("nan")):
        with pytest.raises(_lib.StError, match="spacing must be > 0"):
            sample_tubes_device(a, b, r1, r2, spacing)
    assert b"spacing" in _lib.lib().st_last_error()


def test_sampling_refuses_two_to_the_31_samples(backend):
    a, b, r1, r2 = _dev(backend, *_tubes(5, seed=1))
    with pytest.raises(_lib.StError, match="2\\^31"):
        sample_tubes_device(a, b, r1, r2, 1e-11)


# ------------------------------------------------------------------------------------------------ 2. matching ---
_CASES = {}


def _match_case(n, m):
    """(samples, tubes, oracle results per (ref_mode, T)): computed once, shared, never modified."""
    if (n, m) not in _CASES:
        a, b, r1, r2 = _tubes(m, seed=n + m)
        rng = np.random.RandomState(n)
        # samples near the tubes, so that every threshold has hits and misses
        pick = rng.randint(0, m, n)
        f = rng.rand(n, 1).astype(np.float32)
        pts = (a[pick] + f * (b[pick] - a[pick]) + rng.normal(0, 0.05, (n, 3))).astype(np.float32)
        rad = (0.01 + 0.1 * rng.rand(n)).astype(np.float32)
        if m == 37:
            b[11] = a[11]  # a zero-length tube behaves as the point a
            pts[5] = a[11] + np.float32([1e-3, 0, 0])  # and wins for a sample next to it
            pts[7, 2] = np.nan  # a NaN sample: idx -1, in no hit, not in sums[3]
        for arr in (pts, rad, a, b, r1, r2):
            arr.setflags(write=False)
        ref = {(mode, len(thr)): eo.match(pts, rad, a, b, r1, r2, thr, mode) for mode in (0, 1) for thr in ([0.5], THR10)}
        _CASES[(n, m)] = (pts, rad, a, b, r1, r2, ref)
    return _CASES[(n, m)]


@pytest.mark.parametrize("T", [1, 10])
@pytest.mark.parametrize("ref_mode", [0, 1])
# (513, 512), (511, 513): the tubes end on an LDS tile edge and one past it; 513 samples cross the workgroup edge at 512, an odd
# count leaves the last lane's second sample dead
@pytest.mark.parametrize("n,m", [(1, 1), (701, 37), (3000, 1300), (513, 512), (511, 513)])
def test_match_bit_exact(backend, n, m, ref_mode, T):
    pts, rad, a, b, r1, r2, ref = _match_case(n, m)
    want = ref[(ref_mode, T)]
    thr = [0.5] if T == 1 else THR10
    dev = _dev(backend, pts, rad, a, b, r1, r2)
    got = match(*dev, thr, ref_mode)
    np.testing.assert_array_equal(got["idx"].cpu().numpy(), want["idx"])
    np.testing.assert_array_equal(got["dist"].cpu().numpy(), want["dist"])
    np.testing.assert_array_equal(got["tube_rad"].cpu().numpy(), want["tube_rad"])
    hits, sums = got["hits"].cpu().numpy(), got["sums"].cpu().numpy()
    print(f"n={n} m={m} ref_mode={ref_mode} hits={hits.tolist()} sums={sums.tolist()}")
    np.testing.assert_array_equal(hits, want["hits"])
    exact = want["terms"].astype(np.float64).sum(1)  # float64 sum of the oracle's float32 terms
    assert sums[3] == exact[3] == (want["idx"] >= 0).sum()
    np.testing.assert_allclose(sums, exact, rtol=1e-10, atol=0)
    # null per-sample outputs: the same tally; a second call: the same bits
    bare = match(*dev, thr, ref_mode, per_sample=False)
    again = match(*dev, thr, ref_mode)
    assert torch.equal(bare["tally"], got["tally"]) and torch.equal(again["tally"], got["tally"])
    if m == 37:
        assert want["idx"][5] == 11 and want["idx"][7] == -1
        assert math.isinf(want["dist"][7]) and math.isnan(want["tube_rad"][7])
        assert sums[3] == n - 1
        if T == 10:
            assert 0 < hits[0] < hits[-1] < n  # thresholds separate; the NaN sample is in no hit
    if m == 1300:
        assert (want["idx"] >= 512).any() and (want["idx"] < 512).any()  # winners in more than one LDS tile


def test_match_first_minimum_wins_across_a_tile_edge(backend):
    """512 tubes twice over: tube j + 512 is exactly as far as tube j and sits one LDS tile later; the first must win."""
    pts, rad, a, b, r1, r2, _ = _match_case(300, 512)
    a, b, r1, r2 = (np.concatenate([x, x]) for x in (a, b, r1, r2))
    want = eo.match(pts, rad, a, b, r1, r2, THR10, 1)
    assert (want["idx"] >= 0).all() and (want["idx"] < 512).all()
    got = match(*_dev(backend, pts, rad, a, b, r1, r2), THR10, 1)
    np.testing.assert_array_equal(got["idx"].cpu().numpy(), want["idx"])
    np.testing.assert_array_equal(got["dist"].cpu().numpy(), want["dist"])
    np.testing.assert_array_equal(got["tube_rad"].cpu().numpy(), want["tube_rad"])
    np.testing.assert_array_equal(got["hits"].cpu().numpy(), want["hits"])


def test_match_argument_checks(backend):
    pts, rad, a, b, r1, r2, _ = _match_case(1, 1)
    dev = _dev(backend, pts, rad, a, b, r1, r2)
    with pytest.raises(_lib.StError, match="thresholds"):
        match(*dev, [0.1] * 33, 0)
    with pytest.raises(_lib.StError, match="ref_mode"):
        match(*dev, [0.1], 2)
    with pytest.raises(_lib.StError, match="tubes"):
        match(dev[0], dev[1], dev[2][:0], dev[3][:0], dev[4][:0], dev[5][:0], [0.1], 0)
    empty = match(dev[0][:0], dev[1][:0], *dev[2:], THR10, 0)  # n == 0: a zeroed tally, nothing else launched
    assert not empty["tally"].cpu().numpy().any()


# ------------------------------------------------------------------------------------------ 3. metric properties ---
def _segments_tree(seed, max_depth=4):
    """grow_tree segments as a TreeSkeleton: one branch of four tubes per segment."""
    seg = grow_tree(seed, max_depth=max_depth)
    branches = {}
    for i in range(len(seg.a)):
        f = np.linspace(0.0, 1.0, 5)[:, None]
        xyz = (seg.a[i] + f * (seg.b[i] - seg.a[i])).astype(np.float32)
        radii = (seg.ra[i] + f * (seg.rb[i] - seg.ra[i])).astype(np.float32)
        branches[i] = BranchSkeleton(i, i - 1, torch.from_numpy(xyz), torch.from_numpy(radii))
    return TreeSkeleton(0, branches)


def test_skeleton_against_itself_is_perfect(backend):
    tree = _segments_tree(3)
    r = evaluate_skeleton(tree, tree, spacing=0.01, device=backend)
    assert r["thresholds"] == list(DEFAULT_THRESHOLDS) == THR10
    assert r["n_pred"] == r["n_gt"] > 1000
    assert r["precision"] == [1.0] * 10 and r["recall"] == [1.0] * 10 and r["f1"] == [1.0] * 10 and r["auc"] == 1.0
    assert r["mean_distance_pred_to_gt"] < 1e-5 and r["mean_distance_gt_to_pred"] < 1e-5
    # the first sample of a child branch IS the parent's end point: the parent's tube (lower index) wins at distance 0 with
    # its own end radius, of which the child's is 0.6 .. 0.9 (grow_tree); every other sample meets its own radius to rounding
    assert r["radius_rel_error"] <= 0.4 * len(tree) / r["n_pred"] + 1e-5
    assert r["pred_length"] == r["gt_length"] == pytest.approx(float(tree.length), rel=1e-5)


def test_shifted_tube_steps_from_zero_to_one(backend):
    R = 0.05
    line = lambda x: BranchSkeleton(0, -1, torch.tensor([[x, 0.0, 0.0], [x, 1.0, 0.0]]), torch.full((2, 1), R))
    gt, pred = TreeSkeleton(0, {0: line(0.0)}), TreeSkeleton(0, {0: line(0.35 * R)})
    r = evaluate_skeleton(pred, gt, spacing=0.01, device=backend)
    want = [0.0, 0.0, 0.0] + [1.0] * 7
    assert r["precision"] == want and r["recall"] == want and r["f1"] == want
    assert r["n_pred"] == r["n_gt"] == 100
    assert r["mean_distance_pred_to_gt"] == pytest.approx(0.35 * R, rel=1e-5)
    assert r["auc"] == pytest.approx((0.05 + 0.6) / 0.9, rel=1e-12)  # trapezoid: half a step up, then six full ones
    one = evaluate_skeleton(pred, gt, spacing=0.01, thresholds=[0.5], device=backend)
    assert one["f1"] == [1.0] and one["auc"] == 1.0


def test_half_the_branches_keeps_precision(backend):
    gt = _segments_tree(5)
    kept = {k: v for k, v in gt.branches.items() if k % 2 == 0}
    pred = TreeSkeleton(0, kept)
    r = evaluate_skeleton(pred, gt, spacing=0.01, device=backend)
    assert r["precision"] == [1.0] * 10
    count = eo.sample_tubes(*[t.numpy() for t in skeleton_tubes(gt)], 0.01)[0]
    per_branch = count.reshape(-1, 4).sum(1)  # four tubes per branch, in branch order
    share = per_branch[::2].sum() / per_branch.sum()
    assert r["n_pred"] == per_branch[::2].sum() and r["n_gt"] == per_branch.sum()
    assert share <= r["recall"][0] < 1.0
    assert all(x <= y for x, y in zip(r["recall"], r["recall"][1:]))


def test_empty_prediction_and_empty_ground_truth(backend):
    gt = _segments_tree(1, max_depth=2)
    for empty in (TreeSkeleton(0, {}), DisjointTreeSkeleton([])):
        r = evaluate_skeleton(empty, gt, spacing=0.01, device=backend)
        assert r["n_pred"] == 0 and r["n_gt"] > 0 and r["auc"] == 0.0
        assert r["precision"] == r["recall"] == r["f1"] == [0.0] * 10
        assert all(math.isnan(r[k]) for k in ("mean_distance_pred_to_gt", "mean_distance_gt_to_pred", "radius_rel_error"))
        with pytest.raises(ValueError):
            evaluate_skeleton(gt, empty, spacing=0.01, device=backend)


# ---------------------------------------------------------------------------- 4. sample_skeleton and the host path ---
def test_sample_skeleton_and_host_path(backend):
    tree = _segments_tree(2, max_depth=3)
    a, b, r1, r2 = skeleton_tubes(tree)
    kp, kr = sample_tubes_device(*[t.to(backend) for t in (a, b, r1, r2)], 0.02)[:2]
    sp, sr = tree.sample_skeleton(0.02)
    assert sp.shape == kp.shape and sp.shape[0] > 300
    np.testing.assert_allclose(sp.numpy(), kp.cpu().numpy(), rtol=0, atol=1e-6)
    np.testing.assert_allclose(sr.numpy(), kr.cpu().numpy(), rtol=0, atol=1e-6)
    dp, dr = DisjointTreeSkeleton([tree, tree]).sample_skeleton(0.02)
    assert torch.equal(dp, torch.cat([sp, sp])) and torch.equal(dr, torch.cat([sr, sr]))
    # the host expression against the kernel on tubes with the degenerate ones
    ta = _tubes(37, seed=37, special=True)
    host = sample_tubes_host(*[torch.from_numpy(x) for x in ta], 0.01)
    kern = sample_tubes_device(*_dev(backend, *ta), 0.01)
    for h, k in zip(host, kern):
        assert h.shape == k.shape
        np.testing.assert_allclose(h.numpy(), k.cpu().numpy(), rtol=0, atol=1e-6)
    hp, hr = sample_tubes(tree.to_tubes(), 0.02)  # a list of Tube on the host takes the host path
    assert torch.equal(hp, sp) and torch.equal(hr, sr)
    with pytest.raises(ValueError):
        sample_tubes_host(*[torch.from_numpy(x) for x in ta], 0.0)


# ------------------------------------------------------------------------------------------------------ 5. CLI ---
def test_cli_pairs_by_stem_and_matches_the_function(backend, tmp_path, capsys):
    from smart_tree_amd import evaluate
    from smart_tree_amd.util.file import save_skeleton, save_skeleton_npz

    gts = {"oak": _segments_tree(1, max_depth=3), "elm": _segments_tree(2, max_depth=3)}
    preds = {}
    for name, gt in gts.items():
        save_skeleton(gt, tmp_path / "gt" / f"{name}.npz")
        moved = {k: BranchSkeleton(b._id, b.parent_id, b.xyz + torch.tensor([0.01, 0.0, 0.0]), b.radii) for k, b in gt.branches.items()
                 if k % 3 != 1}
        preds[name] = DisjointTreeSkeleton([TreeSkeleton(0, moved)])
    save_skeleton_npz(tmp_path / "pred" / "oak.npz", preds["oak"])  # the flat file the pipeline writes
    save_skeleton(preds["elm"].skeletons[0], tmp_path / "pred" / "elm.npz")  # the reference layout
    save_skeleton(gts["oak"], tmp_path / "gt" / "lonely.npz")  # no partner: reported and skipped
    out = tmp_path / "metrics.json"
    res = evaluate.main([f"pred={tmp_path / 'pred'}", f"gt={tmp_path / 'gt'}", "spacing=0.02", "thresholds=[0.25,0.5,1.0]",
                         f"out={out}", f"device={backend}"])
    text = capsys.readouterr().out
    assert "lonely" in text and "skipped" in text
    assert sorted(res["trees"]) == ["elm", "oak"] and res["skipped"] == ["lonely"]
    saved = json.loads(out.read_text())
    for name in gts:
        want = evaluate_skeleton(preds[name], gts[name], spacing=0.02, thresholds=[0.25, 0.5, 1.0], device=backend)
        assert res["trees"][name] == want == saved["trees"][name]
        assert 0.0 < want["recall"][-1] < 1.0 and name in text
    for key in ("auc", "radius_rel_error", "n_gt"):
        assert res["mean"][key] == pytest.approx(np.mean([res["trees"][n][key] for n in gts]))
    assert res["mean"]["f1"] == pytest.approx(np.mean([res["trees"][n]["f1"] for n in gts], axis=0).tolist())
    # a single pair of files
    one = evaluate.main([f"pred={tmp_path / 'pred' / 'oak.npz'}", f"gt={tmp_path / 'gt' / 'oak.npz'}", "spacing=0.02",
                         "thresholds=[0.25,0.5,1.0]", f"out={tmp_path / 'one.json'}", f"device={backend}"])
    assert one["trees"]["oak"] == res["trees"]["oak"]


# ------------------------------------------------------------------------------------------- 6. on the card only ---
@pytest.mark.gpu
def test_match_at_evaluation_size():
    """2e5 samples against 4000 tubes (8e8 pairs): a random subset bit for bit against the oracle, and the hits equal to
    the counts recomputed in torch from the returned distances and radii."""
    dev = torch.device("cuda:0")
    n, m = 200_000, 4000
    a, b, r1, r2 = _tubes(m, seed=9)
    rng = np.random.RandomState(4)
    pick = rng.randint(0, m, n)
    pts = (a[pick] + rng.rand(n, 1).astype(np.float32) * (b[pick] - a[pick]) + rng.normal(0, 0.03, (n, 3))).astype(np.float32)
    rad = (0.01 + 0.1 * rng.rand(n)).astype(np.float32)
    t = lambda x: torch.from_numpy(x).to(dev)
    thr = torch.tensor(THR10, dtype=torch.float32, device=dev)
    sub = np.random.RandomState(0).choice(n, 2000, replace=False)
    for mode in (0, 1):
        got = match(t(pts), t(rad), t(a), t(b), t(r1), t(r2), THR10, mode)
        want = eo.match(pts[sub], rad[sub], a, b, r1, r2, THR10, mode)
        np.testing.assert_array_equal(got["idx"].cpu().numpy()[sub], want["idx"])
        np.testing.assert_array_equal(got["dist"].cpu().numpy()[sub], want["dist"])
        np.testing.assert_array_equal(got["tube_rad"].cpu().numpy()[sub], want["tube_rad"])
        ref = got["tube_rad"] if mode else t(rad)
        counts = ((got["dist"][None, :] <= thr[:, None] * ref[None, :]) & (got["idx"] >= 0)[None, :]).sum(1)
        assert torch.equal(counts, got["hits"])
        assert 0 < int(counts[0]) < int(counts[-1]) <= n
        assert float(got["sums"][3]) == n
        assert float(got["sums"][0]) == pytest.approx(float(got["dist"].double().sum()), rel=1e-10)
