"""Per-point prediction metrics (csrc/prediction_metrics.hip, smart_tree_amd/evaluation/prediction.py, `eval_epoch(metrics=)`,
the run's `prediction_metrics` key, `python -m smart_tree_amd.model.evaluate`) against tests/metrics_oracle.py: every integer
bit for bit, every sum to max(1e-6, 4 x the float32 mirror's own error) relative to the float64 oracle; then the special rows,
determinism and segment independence, the empty cases, the refusals, the derived figures, and the three places that use them."""
import ctypes
import functools
import json
import math

import numpy as np
import pytest
import torch

import metrics_oracle as mo
from smart_tree_amd import _lib
from smart_tree_amd.evaluation import PredictionTally, derive_metrics, prediction_tally, segment_offsets
from smart_tree_amd.model import loss as L

# every boundary a power-of-two tile up to 4096 can have, and an empty segment
LENGTHS = (0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097)
SEG_OFF = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)
THR = (0.1, 0.25, 0.5, 1.0)
EDGES = (0.005, 0.01, 0.02, 0.05, 0.1)
NETWORK = (3, [8, 16, 32], [8, 8, 4, 1], [8, 8, 4, 3], [8, 8, 4, 2])
LOSS_FN = functools.partial(L.compute_loss, radius_loss_fn=L.L1Loss, direction_loss_fn=L.cosine_similarity_loss,
                            class_loss_fn=L.focal_loss, target_radius_log=True, vector_class=0)
_INPUTS, _ORACLES = {}, {}


def _inputs(C):
    """About 22k rows of plausible predictions for the 17 segments: built once per class count, shared, never modified.  Logits
    lie on a grid of 1/64 (two logits are bit-equal, some on purpose, or 1/64 apart); rows that land within 1e-3 relative of a
    threshold or a bin edge are moved off it, and the oracle's margin condition is asserted."""
    if C not in _INPUTS:
        rng = np.random.default_rng(100 + C)
        n = int(SEG_OFF[-1])
        r_gt = np.exp(rng.uniform(np.log(0.003), np.log(0.2), n)).astype(np.float32)
        q = rng.normal(size=(n, 3))
        q /= np.linalg.norm(q, axis=1, keepdims=True)
        targets = np.concatenate([r_gt[:, None], q, rng.integers(0, C, n)[:, None]], axis=1).astype(np.float32)
        radius = (np.log(r_gt) + rng.normal(0, 0.3, n)).astype(np.float32)[:, None]
        direction = ((q + rng.normal(0, 0.3, (n, 3))) * rng.uniform(0.5, 2.0, (n, 1))).astype(np.float32)
        class_l = (np.round(rng.normal(0, 2, (n, C)) * 64) / 64 + 0.0).astype(np.float32)  # + 0.0: no -0.0
        class_l[::37, 1] = class_l[::37, 0]  # ties: the first largest wins
        class_l[5::41, C - 1] = class_l[5::41].max(1)
        for _ in range(8):
            bad = mo.margin_violations(radius, direction, class_l, targets, True, THR, EDGES, rel=1e-3)
            if not bad.any():
                break
            radius[bad, 0] += np.float32(0.03)
            targets[bad, 0] *= np.float32(1.01)
        mo.assert_margins(radius, direction, class_l, targets, True, THR, EDGES)
        mask = rng.random(n) < 0.7
        arrays = dict(radius=radius, direction=direction, class_l=class_l, targets=targets, mask=mask)
        for a in arrays.values():
            a.setflags(write=False)
        _INPUTS[C] = arrays
    return _INPUTS[C]


def _oracles(C, masked, vector_class):
    key = (C, masked, vector_class)
    if key not in _ORACLES:
        a = _inputs(C)
        args = (a["radius"], a["direction"], a["class_l"], a["targets"], a["mask"] if masked else None, SEG_OFF.tolist(), vector_class,
                True, THR, EDGES)
        _ORACLES[key] = (mo.evaluate(*args, dtype=np.float64), mo.evaluate(*args, dtype=np.float32))
    return _ORACLES[key]


def _tally(a, device, rows=slice(None), masked=True, **kw):
    t = lambda x: torch.from_numpy(np.array(x[rows])).to(device)
    preds = {"radius": t(a["radius"]), "direction": t(a["direction"]), "class_l": t(a["class_l"])}
    kw.setdefault("thresholds", THR)
    kw.setdefault("radius_edges", EDGES)
    return prediction_tally(preds, t(a["targets"]), t(a["mask"]) if masked else None, **kw)


def _sum_error(got, o64, o32):
    """(largest relative error of a sum against the float64 oracle, whether every sum is within its bound)."""
    scale = np.maximum(np.abs(o64), 1e-300)
    err = np.abs(got - o64) / scale
    bound = np.maximum(1e-6, 4.0 * np.abs(o32 - o64) / scale)
    return float(err.max()), bool((err <= bound).all())


def _same_metrics(a, b):
    return json.dumps(a, sort_keys=True) == json.dumps(b, sort_keys=True)  # NaN == NaN


# ---------------------------------------------------------------------------------------------------- 1. the oracle ---
@pytest.mark.parametrize("vector_class", [0, None])
@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("C", [2, 3])
def test_parity_with_the_oracle(backend, C, masked, vector_class):
    o64, o32 = _oracles(C, masked, vector_class)
    got = _tally(_inputs(C), backend, masked=masked, seg_off=SEG_OFF, vector_class=vector_class)
    assert got.n_seg == len(LENGTHS) and got.ints.dtype == torch.int64 and got.sums.dtype == torch.float64
    ints, sums = got.ints.cpu().numpy(), got.sums.cpu().numpy()
    np.testing.assert_array_equal(o32["ints"], o64["ints"])  # the margins hold: both evaluations decide alike
    np.testing.assert_array_equal(ints, o64["ints"])
    err, ok = _sum_error(sums, o64["sums"], o32["sums"])
    print(f"{backend} C={C} mask={masked} vector_class={vector_class}: largest sum error {err:.3e} relative "
          f"(float32 mirror: {_sum_error(o32['sums'], o64['sums'], o32['sums'])[0]:.3e})")
    assert ok, err
    assert ints[0].sum() == 0 and not sums[0].any()  # the empty segment
    cc = C * C
    assert (ints[:, :cc].sum(1) == ints[:, cc + 3] - ints[:, cc]).all()  # confusion entries = rows - bad_class
    assert int(ints[:, cc + 1].sum()) > 5000 and (ints[:, cc + 4 + len(THR):].sum(1) == ints[:, cc + 1]).all()


# --------------------------------------------------------------------------------------------------- 2. special rows ---
def test_special_rows(backend):
    C, nan = 2, float("nan")
    thr = (0.1, 0.25, 0.5, 2.0)  # not 1.0: a zero predicted direction misses by exactly the target radius
    n = 24
    rng = np.random.default_rng(7)
    q = rng.normal(size=(n, 3))
    targets = np.concatenate([np.full((n, 1), 0.03), q, np.zeros((n, 1))], axis=1).astype(np.float32)
    targets[1::2, 4] = 1.0
    radius = np.full((n, 1), math.log(0.035), dtype=np.float32)
    direction = (q + rng.normal(0, 0.2, (n, 3))).astype(np.float32)
    class_l = (np.round(rng.normal(0, 2, (n, C)) * 64) / 64 + 0.0).astype(np.float32)
    class_l[0] = [nan, 5.0]   # a NaN logit in the first position: predicted 0
    class_l[1] = [5.0, nan]   # in a later one: predicted 1
    class_l[2] = [nan, nan]   # the first NaN
    class_l[3] = [1.5, 1.5]   # bit-equal: the first
    targets[4, 4], targets[5, 4], targets[6, 4], targets[7, 4] = -1.0, float(C), nan, 1.9  # 1.9 truncates to 1
    targets[8, 0] = 0.0       # zero target radius: dr / r_gt is infinite
    targets[9, 0] = nan
    direction[10] = 0.0       # a zero predicted direction: p^ = 0, finite
    targets[11, 1:4] = 0.0    # a zero target direction
    radius[12, 0] = 100.0     # expf overflows
    a = dict(radius=radius, direction=direction, class_l=class_l, targets=targets, mask=np.ones(n, dtype=bool))
    mo.assert_margins(radius, direction, class_l, targets, True, thr, EDGES)
    args = (radius, direction, class_l, targets, None, None, None, True, thr, EDGES)
    o64, o32 = mo.evaluate(*args, dtype=np.float64), mo.evaluate(*args, dtype=np.float32)
    got = _tally(a, backend, masked=False, thresholds=thr)
    ints, sums = got.ints.cpu().numpy(), got.sums.cpu().numpy()
    cc = C * C
    assert ints[0, cc:cc + 4].tolist() == [3, n - 6, 3, n]  # bad_class, vector_rows, bad_vector, rows
    np.testing.assert_array_equal(ints, o64["ints"])
    np.testing.assert_array_equal(o32["ints"], o64["ints"])
    assert np.isfinite(sums).all()
    err, ok = _sum_error(sums, o64["sums"], o32["sums"])
    assert ok, err
    first = _tally(a, backend, rows=slice(0, 4), masked=False)  # targets 0, 1, 0, 1; predictions 0, 1, 0, 0
    assert first.ints[0, :cc].tolist() == [2, 0, 1, 1]
    m = got.metrics()
    assert m["counts"] == {"rows": n, "vector_rows": n - 6, "bad_class": 3, "bad_vector": 3}
    assert all(math.isfinite(m[k]) for k in ("radius_mae", "radius_rel_error", "direction_angle_deg", "medial_error", "medial_rel_error"))


# ------------------------------------------------------------------------- 3. determinism and segment independence ---
def test_determinism_and_segment_independence(backend):
    C = 3
    a = _inputs(C)
    kw = dict(vector_class=0)
    first = _tally(a, backend, seg_off=SEG_OFF, **kw)
    again = _tally(a, backend, seg_off=SEG_OFF, **kw)
    assert torch.equal(first.ints, again.ints) and torch.equal(first.sums.view(torch.int64), again.sums.view(torch.int64))
    for s, (lo, hi) in enumerate(zip(SEG_OFF[:-1], SEG_OFF[1:])):
        alone = _tally(a, backend, rows=slice(int(lo), int(hi)), **kw)
        assert alone.n_seg == 1
        assert torch.equal(alone.ints[0], first.ints[s]), s
        assert torch.equal(alone.sums[0].view(torch.int64), first.sums[s].view(torch.int64)), s
        assert torch.equal(first.segment(s).ints, alone.ints)
    total = first.total()
    ints, sums = first.ints.cpu().numpy(), first.sums.cpu().numpy()
    acc = sums[0].copy()
    for s in range(1, len(LENGTHS)):
        acc = acc + sums[s]
    assert total.n_seg == 1
    np.testing.assert_array_equal(total.ints.cpu().numpy()[0], ints.sum(0))
    np.testing.assert_array_equal(total.sums.cpu().numpy()[0].view(np.int64), acc.view(np.int64))
    assert _same_metrics(first.metrics(), total.metrics())
    both = total + total  # a one-segment tally adds to another
    assert torch.equal(both.ints, 2 * total.ints)
    with pytest.raises(ValueError, match="segment"):
        first + total
    with pytest.raises(ValueError, match="parameters"):
        total + _tally(a, backend, rows=slice(0, 10), vector_class=None)


# ------------------------------------------------------------------------------------------------------ 4. empty cases ---
@pytest.mark.parametrize("what", ["no_rows", "all_masked"])
def test_empty_cases(backend, what):
    a = _inputs(2)
    if what == "no_rows":
        got = _tally(a, backend, rows=slice(0, 0), vector_class=0)
    else:
        a = {**a, "mask": np.zeros_like(a["mask"])}
        got = _tally(a, backend, rows=slice(0, 5000), seg_off=[0, 100, 100, 5000], vector_class=0)
    assert not got.ints.any() and not got.sums.any()
    m = got.metrics()
    assert m["counts"] == {"rows": 0, "vector_rows": 0, "bad_class": 0, "bad_vector": 0}
    for k in ("accuracy", "miou", "radius_mae", "radius_rel_error", "direction_angle_deg", "medial_error", "medial_rel_error"):
        assert math.isnan(m[k]), k
    assert all(math.isnan(v) for v in m["within"] + m["iou"] + m["by_radius"]["medial_rel_error"])
    assert m["confusion"] == [[0, 0], [0, 0]] and m["by_radius"]["count"] == [0] * 6


# -------------------------------------------------------------------------------------------------------- 5. refusals ---
REFUSALS = {
    "classes": (dict(C=17), "classes"),
    "thresholds": (dict(thr=[0.1] * 17), "thresholds"),
    "bins": (dict(edges=[0.001 * (k + 1) for k in range(16)]), "radius edges"),
    "segments": (dict(seg_off=[0] * 65 + [8]), "segments per call"),
    "target_cols": (dict(target_cols=4), "columns"),
    "edges_not_ascending": (dict(edges=[0.01, 0.01]), "strictly ascend"),
    "edge_not_finite": (dict(edges=[0.01, float("inf")]), "not finite"),
    "nan_threshold": (dict(thr=[0.5, float("nan")]), "NaN"),
    "offsets_decrease": (dict(seg_off=[0, 6, 4, 8]), "decreasing"),
    "offsets_start": (dict(seg_off=[1, 8]), "start at 0"),
    "offsets_end": (dict(seg_off=[0, 7]), "end at n"),
    "null_input": (dict(null="direction"), "null input"),
    "workspace": (dict(ws_bytes=8), "workspace too small"),
}


@pytest.mark.parametrize("what", list(REFUSALS))
def test_refusals_write_nothing(backend, what):
    over, text = REFUSALS[what]
    n, C = 8, over.get("C", 2)
    dev = lambda x: torch.from_numpy(x).to(backend)
    tens = {"radius": dev(np.zeros(n, np.float32)), "direction": dev(np.ones((n, 3), np.float32)),
            "class_l": dev(np.zeros((n, C), np.float32)), "targets": dev(np.ones((n, 5), np.float32))}
    if "null" in over:
        tens[over["null"]] = None
    thr = np.asarray(over.get("thr", THR), dtype=np.float32)
    edges = np.asarray(over.get("edges", EDGES), dtype=np.float32)
    off = np.asarray(over["seg_off"], dtype=np.int64) if "seg_off" in over else None
    n_seg = len(off) - 1 if off is not None else 1
    ints = torch.full((64 * 400,), -7, dtype=torch.int64, device=backend)
    sums = torch.full((64 * 64,), -7.0, dtype=torch.float64, device=backend)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=backend)
    h = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    lib = _lib.lib()
    rc = lib.st_prediction_metrics(_lib.ptr(tens["radius"]), _lib.ptr(tens["direction"]), _lib.ptr(tens["class_l"]), C,
                                   _lib.ptr(tens["targets"]), over.get("target_cols", 5), None, n, h(off), n_seg, 0, 1, h(thr), len(thr),
                                   h(edges), len(edges), _lib.ptr(ints), _lib.ptr(sums), _lib.ptr(ws), over.get("ws_bytes", ws.numel()),
                                   _lib.stream(backend))
    if backend.type == "cuda":
        torch.cuda.synchronize()
    assert rc != 0
    with pytest.raises(_lib.StError, match=text):
        _lib.check(rc)
    assert bool((ints == -7).all()) and bool((sums == -7.0).all())
    if what == "classes":  # the wrapper reports the library's reason
        with pytest.raises(_lib.StError, match="classes"):
            prediction_tally({"radius": tens["radius"], "direction": tens["direction"], "class_l": tens["class_l"]}, tens["targets"])
    if what == "workspace":
        assert lib.st_prediction_metrics_workspace_bytes(n, 1, 6) > 8
        assert lib.st_prediction_metrics_tally_ints(2, 4, 6) == 4 + 4 + 4 + 6 and lib.st_prediction_metrics_tally_sums(6) == 17
        assert lib.st_prediction_metrics_tally_ints(17, 4, 6) == -1 and lib.st_version() >= 108


# --------------------------------------------------------------------------------------------- 6. metrics() on the CPU ---
def test_metrics_from_a_hand_written_record():
    conf = [[5, 1, 0], [2, 3, 1], [0, 0, 0]]  # class 2 never a target; predicted once
    ints = [v for row in conf for v in row] + [2, 10, 1, 15] + [2, 5] + [4, 6, 0]
    sums = [0.05, 2.0, 10 * math.pi / 6, 0.1, 5.0] + [1.0, 1.0, 0.0] + [2.0, 3.0, 0.0]
    m = derive_metrics(ints, sums, 3, (0.5, 1.0), (0.01, 0.02))
    assert m["accuracy"] == 8 / 12
    assert m["iou"] == [5 / 8, 3 / 7, 0.0] and m["miou"] == pytest.approx((5 / 8 + 3 / 7 + 0.0) / 3)
    assert m["precision"] == [5 / 7, 3 / 4, 0.0] and m["recall"][:2] == [5 / 6, 3 / 6] and math.isnan(m["recall"][2])
    assert m["radius_mae"] == 0.005 and m["radius_rel_error"] == 0.2 and m["direction_angle_deg"] == pytest.approx(30.0)
    assert m["medial_error"] == 0.01 and m["medial_rel_error"] == 0.5
    assert m["within"] == [0.2, 0.5] and m["thresholds"] == [0.5, 1.0]
    assert m["by_radius"]["edges"] == [0.01, 0.02] and m["by_radius"]["count"] == [4, 6, 0]
    assert m["by_radius"]["radius_rel_error"][:2] == [0.25, 1 / 6] and m["by_radius"]["medial_rel_error"][:2] == [0.5, 0.5]
    assert math.isnan(m["by_radius"]["radius_rel_error"][2]) and math.isnan(m["by_radius"]["medial_rel_error"][2])
    assert m["counts"] == {"rows": 15, "vector_rows": 10, "bad_class": 2, "bad_vector": 1} and m["confusion"] == conf
    none = derive_metrics([0] * 9 + [0] * 4 + [0, 0] + [0] * 3, [0.0] * 11, 3, (0.5, 1.0), (0.01, 0.02))
    assert math.isnan(none["miou"]) and math.isnan(none["accuracy"]) and math.isnan(none["medial_error"])
    with pytest.raises(ValueError, match="record"):
        derive_metrics(ints[:-1], sums, 3, (0.5, 1.0), (0.01, 0.02))
    assert segment_offsets(torch.tensor([0, 0, 2, 2, 2])) == [0, 2, 2, 5] and segment_offsets(torch.zeros(0)) == [0]
    with pytest.raises(ValueError, match="contiguous"):
        segment_offsets(torch.tensor([0, 1, 0]))


# ------------------------------------------------------------------------------------------------------ 7. eval_epoch ---
TREE = dict(n_points=1500, scale=0.6, noise=0.002, foliage_fraction=0.3, max_depth=2)


def _loader(device, trees=2, batch_size=2):
    from smart_tree_amd.dataset.synthetic import SyntheticTreeDataset
    from smart_tree_amd.model.sparse import batch_collate

    ds = SyntheticTreeDataset(0.05, "validation", trees, ["xyz"], ["radius", "direction", "class_l"], seed=3, device=device, **TREE)
    return torch.utils.data.DataLoader(ds, batch_size=batch_size, collate_fn=batch_collate)


def _model(device):
    from smart_tree_amd.model.trainable import TrainableSmartTree

    torch.manual_seed(0)
    return TrainableSmartTree(*NETWORK).to(device).train()


@torch.no_grad()
def _direct_tally(loader, net, device, per_tree=False, **kw):
    """The model's outputs tallied batch by batch with prediction_tally itself."""
    from smart_tree_amd.model.sparse import sparse_from_batch

    net.eval()
    out = []
    for (feats, targets), coords, mask, names in loader:
        preds = net.forward(sparse_from_batch(feats.float(), coords, device=device))
        seg = segment_offsets(coords[:, 0]) if per_tree else None
        out.append((names, prediction_tally(preds, targets.to(device).float(), mask.to(device), seg_off=seg, **kw)))
    net.train()
    return out


def test_eval_epoch_metrics(backend):
    from smart_tree_amd.model import train as T

    net = _model(backend)
    plain = T.eval_epoch(_loader(backend), net, LOSS_FN, backend)
    assert set(plain) == {"radius", "direction", "class_l"}
    got = T.eval_epoch(_loader(backend), net, LOSS_FN, backend, metrics={})
    assert set(got) == {"radius", "direction", "class_l", "metrics"} and {k: got[k] for k in plain} == plain
    (_, want), = _direct_tally(_loader(backend), net, backend, vector_class=0, target_radius_log=True)
    assert _same_metrics(got["metrics"], want.metrics())
    m = got["metrics"]
    assert m["counts"]["rows"] > 200 and 0 < m["counts"]["vector_rows"] < m["counts"]["rows"] and len(m["confusion"]) == 2
    assert m["thresholds"] == [0.1, 0.25, 0.5, 1.0] and math.isfinite(m["medial_error"])
    # keywords of the dict win over the loss's; two batches add
    every = T.eval_epoch(_loader(backend, batch_size=1), net, LOSS_FN, backend, metrics={"vector_class": None, "thresholds": [0.5]})["metrics"]
    parts = [t for _, t in _direct_tally(_loader(backend, batch_size=1), net, backend, vector_class=None, thresholds=[0.5])]
    assert len(parts) == 2 and _same_metrics(every, (parts[0] + parts[1]).metrics())
    assert every["counts"]["vector_rows"] + every["counts"]["bad_vector"] == every["counts"]["rows"] == m["counts"]["rows"]


# ------------------------------------------------------------------------------------------- 8. / 9. run and command ---
def _run_args(run_dir, device, **kw):
    a = {"config": "training_synthetic", "num_epoch": 2, "batch_size": 2, "train_trees": 2, "validation_trees": 2, "test_trees": 2,
         "points": 1500, "scale": 0.6, "max_depth": 2, "voxel_size": 0.05, "fp16": False, "capture_output": 0, "device": device,
         "lr": 0.01, "run_dir": run_dir, "validation_dataset.augmentation": "null", "test_dataset.augmentation": "null"}  # no random crop
    a.update(kw)
    return [f"{k}={v}" for k, v in a.items()]


def test_run_and_command(backend, tmp_path, capsys):
    from smart_tree_amd import config as C
    from smart_tree_amd.model import evaluate as E
    from smart_tree_amd.model import train as T
    from smart_tree_amd.model.tracker import read_metrics

    run, plain = tmp_path / "run", tmp_path / "plain"
    T.main(_run_args(run, backend, prediction_metrics="true"))
    T.main(_run_args(plain, backend, num_epoch=1))
    assert all("validation_metrics" not in r and "test_metrics" not in r for r in read_metrics(plain / "metrics.jsonl"))
    assert "prediction_metrics" not in (plain / "config.yaml").read_text()
    lines = read_metrics(run / "metrics.jsonl")
    assert [r["epoch"] for r in lines] == [0, 1]
    drop = lambda r: {k: v for k, v in r.items() if k not in ("seconds", "validation_metrics", "test_metrics")}
    assert drop(read_metrics(plain / "metrics.jsonl")[0]) == drop(lines[0])  # the losses and the best are untouched
    cfg = T.load_training_config(_run_args(run, backend))
    rows = {split: sum(int(mask.sum()) for _, _, mask, _ in C.instantiate(cfg[f"{split}_data_loader"])) for split in ("validation", "test")}
    for r in lines:
        for split in ("validation", "test"):
            m = r[f"{split}_metrics"]
            assert sum(sum(row) for row in m["confusion"]) == rows[split] == m["counts"]["rows"] and m["counts"]["bad_class"] == 0
            assert len(m["confusion"]) == 2 and len(m["within"]) == 4
    assert lines[0]["validation_metrics"] != lines[1]["validation_metrics"] and lines[1]["validation_metrics"]["counts"]["vector_rows"] > 0
    # a mapping of keywords is accepted as an override
    T.main(_run_args(tmp_path / "kw", backend, num_epoch=1, prediction_metrics="{thresholds: [0.5], vector_class: null}"))
    m = read_metrics(tmp_path / "kw" / "metrics.jsonl")[0]["validation_metrics"]
    assert m["thresholds"] == [0.5] and m["counts"]["vector_rows"] + m["counts"]["bad_vector"] == m["counts"]["rows"]

    # the command, on both kinds of weights file
    capsys.readouterr()
    weights = run / "smart-tree_model_weights.pt"
    args = [a for a in _run_args("unused", backend) if not a.startswith(("num_epoch", "run_dir"))]
    res = E.main(args + [f"weights={run / 'last.pt'}", f"out={tmp_path / 'm.json'}", "split=validation"])
    printed = capsys.readouterr().out.strip().splitlines()
    net = C.instantiate(cfg["model"]).to(backend)
    net.load_state_dict(torch.load(run / "last.pt", weights_only=True)["model"])
    torch.manual_seed(42)
    (names, want), = _direct_tally(C.instantiate(cfg["validation_data_loader"]), net, backend, per_tree=True, vector_class=0,
                                   target_radius_log=True)
    assert list(res["trees"]) == [str(n) for n in names] and len(names) == 2
    for s, name in enumerate(names):
        assert _same_metrics(res["trees"][str(name)], want.segment(s).metrics())
    assert _same_metrics(res["total"], want.total().metrics())
    assert _close(res["total"], lines[1]["validation_metrics"])  # last.pt is the model after epoch 1; other tiles, other last bits
    assert _same_metrics(json.loads((tmp_path / "m.json").read_text()), res)
    assert len(printed) == 3 and all("miou" in ln and "medial error" in ln and "within 0.5 r" in ln for ln in printed)
    if weights.is_file():
        best = E.main(args + [f"weights={weights}", "out=null"])
        assert len(best["trees"]) == 2 and best["total"]["counts"]["rows"] == rows["test"]
    with pytest.raises(SystemExit, match="usage: python -m smart_tree_amd.model.evaluate.*unknown: no_such_key"):
        E.main(args + [f"weights={weights}", "no_such_key=1"])
    with pytest.raises(SystemExit, match="usage"):
        E.main(args)


# ------------------------------------------------------------------------------------------------- 10. two gloo ranks ---
def _rank_worker(rank, world, port, data, q):
    import os
    from pathlib import Path

    import torch.distributed as dist

    from smart_tree_amd.model import train as T
    from smart_tree_amd.model.sync_bn import convert_sync_batchnorm
    from test_data_parallel import _loader as tree_loader
    from test_data_parallel import _use_kernels

    device = torch.device("cpu")
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    _use_kernels(device)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        net = convert_sync_batchnorm(_model(device), dist.group.WORLD)
        q.put((rank, T.eval_epoch(tree_loader(Path(data), 2, device), net, LOSS_FN, device, group=dist.group.WORLD, metrics={})))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def _close(a, b, rel=1e-12):
    """Integers (and lists of them) exact, floats to `rel`, NaN equal to NaN."""
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_close(a[k], b[k], rel) for k in a)
    if isinstance(a, list):
        return len(a) == len(b) and all(_close(x, y, rel) for x, y in zip(a, b))
    if isinstance(a, float) and isinstance(b, float):
        return (math.isnan(a) and math.isnan(b)) or math.isclose(a, b, rel_tol=rel, abs_tol=0.0)
    return a == b


def test_two_gloo_ranks_equal_one_process(emu_lib, monkeypatch, tmp_path):
    """Two trees of one voxel extent (tests/test_data_parallel.py), one per rank, against one process given both: the same
    synchronised-BatchNorm modules in eval mode on both sides, so every prediction is the same float."""
    from smart_tree_amd.model import train as T
    from smart_tree_amd.model.sync_bn import convert_sync_batchnorm
    from test_data_parallel import _loader as tree_loader
    from test_data_parallel import _spawn, _write_trees

    monkeypatch.setattr(_lib, "_LIB", emu_lib)
    monkeypatch.setattr(_lib, "_ALLOW_HOST_POINTERS", True)
    device = torch.device("cpu")
    _write_trees(tmp_path, 2)
    net = convert_sync_batchnorm(_model(device), None)
    one = T.eval_epoch(tree_loader(tmp_path, 2, device), net, LOSS_FN, device, metrics={})["metrics"]
    ranks = _spawn(_rank_worker, 2, str(tmp_path))
    for out in ranks:
        assert _close(out["metrics"], one), (out["metrics"], one)
    assert one["counts"]["rows"] > 200
