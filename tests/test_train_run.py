"""The `train-smart-tree` run (smart_tree_amd/model/train.py `main`, conf/training.yaml): the config loader's interpolation and
`_partial_`, the bundled configuration, the stop policy on scripted losses, and end-to-end runs on the emulator and the MI355X
against a hand-written loop of train_epoch / eval_epoch, their files, captures, resume, fp16, and the weights feeding
`run-smart-tree`."""
import functools
import json
import math

import numpy as np
import pytest
import torch

from smart_tree_amd import config as C
from smart_tree_amd.model import loss as L
from smart_tree_amd.model import train as T
from smart_tree_amd.model.tracker import MetricsSink, Tracker, read_metrics
from smart_tree_amd.model.trainable import TrainableSmartTree

NETWORK = (3, [8, 16, 32], [8, 8, 4, 1], [8, 8, 4, 3], [8, 8, 4, 2])
LOSS_FN = functools.partial(L.compute_loss, radius_loss_fn=L.L1Loss, direction_loss_fn=L.cosine_similarity_loss,
                            class_loss_fn=L.focal_loss, target_radius_log=True, vector_class=0)
NAMES = ["tree_0.npz", "tree_1.npz"]
SPLITS = ("train", "validation", "test")


@pytest.fixture
def data(tmp_path):
    """Two synthetic trees as .npz and a split listing both for every mode (tests/test_train_step.py's _loader)."""
    from smart_tree_amd.synthetic import sample_tree_cloud

    d = tmp_path / "data"
    d.mkdir()
    for name, s in zip(NAMES, (1, 2)):
        c = sample_tree_cloud(6000, seed=s, scale=0.6, max_depth=3, foliage_fraction=0.3)
        np.savez(d / name, xyz=c["xyz"], rgb=c["rgb"], medial_vector=c["medial_vector"], class_l=c["class_l"])
    (d / "split.json").write_text(json.dumps({k: NAMES for k in SPLITS}))
    return d


def _args(data, run_dir, device, **kw):
    a = {"directory": data, "json_path": data / "split.json", "voxel_size": 0.05, "batch_size": 2, "device": device,
         "run_dir": run_dir, "fp16": False, "capture_output": 2, "num_epoch": 3}
    a.update(kw)
    return [f"{k}={v}" for k, v in a.items()]


# ---------------------------------------------------------------------------------------------------------------- config


def test_interpolation_partial_and_call_time_arguments():
    cfg = C.resolve({"x": 2, "node": {"_target_": "builtins.dict", "v": "${x}"}, "a": "${node}", "b": "${node}",
                     "text": "v${x}-${deep.k}", "deep": {"k": "${x}"}})
    assert cfg["a"] == {"_target_": "builtins.dict", "v": 2} and cfg["text"] == "v2-2" and cfg["deep"]["k"] == 2
    a, b = C.instantiate(cfg["a"], w=1), C.instantiate(cfg["b"])
    assert a == {"v": 2, "w": 1} and b == {"v": 2} and a is not b
    p = C.instantiate({"_target_": "builtins.pow", "_partial_": True, "exp": 3})
    assert isinstance(p, functools.partial) and p(2) == 8
    assert C.instantiate({"_target_": "math.sqrt", "_partial_": True}) is math.sqrt  # nothing to bind: the function itself
    with pytest.raises(KeyError, match="nope.k"):
        C.resolve({"a": {"b": "${nope.k}"}})
    with pytest.raises(KeyError, match="cycle.*a"):
        C.resolve({"a": "${b}", "b": "x${a}"})


def test_pipeline_config_unchanged():
    """run-smart-tree's loader reads pipeline.yaml as before: no interpolation, overrides as given."""
    import yaml

    from smart_tree_amd import cli

    raw = yaml.safe_load((T.CONF.parent / "pipeline.yaml").read_text())
    assert cli.load_config([]) == raw
    assert cli.instantiate is C.instantiate


def test_bundled_training_config(data):
    from smart_tree_amd.dataset.augmentations import RandomCubicCrop
    from smart_tree_amd.dataset.dataset import TreeDataset

    raw = C.load_yaml(T.CONF)
    for key, value in (("fp16", True), ("lr", 0.1), ("early_stop_epoch", 20), ("early_stop", True), ("lr_decay", True),
                       ("batch_size", 8), ("voxel_size", 0.01), ("capture_output", 1), ("device", "auto"),
                       ("run_name", "smart-tree"), ("resume", None), ("input_features", ["xyz"]),
                       ("target_features", ["radius", "direction", "class_l"])):
        assert raw[key] == value, key
    assert raw["run_dir"].startswith("outputs/") and "wandb" in raw
    cfg = T.load_training_config(_args(data, "unused", "cpu"))
    loaders = [C.instantiate(cfg[f"{s}_data_loader"]) for s in SPLITS]
    sets = [ld.dataset for ld in loaders]
    assert all(isinstance(ld, torch.utils.data.DataLoader) and ld.batch_size == 2 for ld in loaders)
    assert all(isinstance(ds, TreeDataset) and ds.voxel_size == 0.05 for ds in sets)
    assert [ds.mode for ds in sets] == list(SPLITS) and len({id(ds) for ds in sets}) == 3
    assert [ds.cache is not None for ds in sets] == [False, True, False]
    crops = [ds.augmentation.augmentations[0] for ds in sets]
    assert all(isinstance(c, RandomCubicCrop) and c.size == 4.0 for c in crops) and len({id(c) for c in crops}) == 3
    assert all(str(ds.device) == "cpu" for ds in sets)
    model = C.instantiate(cfg["model"])
    assert isinstance(model, TrainableSmartTree)
    opt = C.instantiate(cfg["optimizer"], params=model.parameters())
    assert isinstance(opt, torch.optim.Adam) and opt.param_groups[0]["lr"] == 0.1
    sched = C.instantiate(cfg["scheduler"], optimizer=opt)
    assert isinstance(sched, torch.optim.lr_scheduler.ReduceLROnPlateau) and sched.mode == "min"
    loss_fn = C.instantiate(cfg["loss_fn"])
    assert isinstance(loss_fn, functools.partial) and loss_fn.func is L.compute_loss
    assert loss_fn.keywords == LOSS_FN.keywords  # the fused HIP loss path's functions
    # a reference-style wandb block is accepted; device auto is decided
    cfg = T.load_training_config(_args(data, "unused", "auto") + ["wandb.entity=someone"])
    assert cfg["device"] == ("cuda:0" if torch.cuda.is_available() else "cpu")


@pytest.mark.parametrize("given", [["json_path=x.json"], ["directory=x"], []])
def test_missing_directory_or_json_path_is_named(given):
    with pytest.raises(ValueError) as e:
        T.load_training_config(given)
    for key in ("directory", "json_path"):
        assert (key in str(e.value)) == (not any(g.startswith(key) for g in given))


# ---------------------------------------------------------------------------------------------------------- stop policy


def test_stop_policy_on_scripted_losses():
    p = T.StopPolicy(early_stop_epoch=2)
    saved, ran = [], []
    for epoch, v in enumerate([3, 2, 2.5, 2.4, 1]):
        ran.append(epoch)
        d = p.update(v)
        assert d.step_scheduler
        if d.save_best:
            saved.append(epoch)
        if d.stop:
            break
    assert saved == [0, 1] and ran == [0, 1, 2, 3] and p.best == 2
    p = T.StopPolicy(early_stop_epoch=2, early_stop=False, lr_decay=False)
    decisions = [p.update(v) for v in [3, 2, 2.5, 2.4, 1]]
    assert not any(d.step_scheduler or d.stop for d in decisions) and [d.save_best for d in decisions] == [1, 1, 0, 0, 1]


@pytest.mark.parametrize("lr_decay", [True, False])
def test_run_loop_on_scripted_losses(data, tmp_path, monkeypatch, lr_decay):
    """The run's loop with train_epoch / eval_epoch scripted: the weights file holds epoch 1's parameters, epoch 4 never runs,
    the scheduler is stepped only with lr_decay, and capture_output=0 writes no captures."""
    val = iter([3, 3, 2, 2, 2.5, 2.5, 2.4, 2.4, 1, 1])  # validation then test, per epoch
    trained = []

    def train_epoch(loader, model, *a, **k):
        with torch.no_grad():
            next(model.parameters()).fill_(len(trained))  # mark the parameters with the epoch
        trained.append(1)
        return {"radius": 1.0, "direction": 1.0, "class_l": 1.0}

    monkeypatch.setattr(T, "train_epoch", train_epoch)
    monkeypatch.setattr(T, "eval_epoch", lambda *a, **k: {"radius": next(val), "direction": 0.0, "class_l": 0.0})
    run = tmp_path / "run"
    res = T.main(_args(data, run, "cpu", num_epoch=10, early_stop_epoch=2, capture_output=0, lr_decay=lr_decay))
    assert len(trained) == 4 and res["stopped"] and res["epochs"] == 4
    lines = read_metrics(run / "metrics.jsonl")
    assert [r["epoch"] for r in lines] == [0, 1, 2, 3] and [r["best"] for r in lines] == [3, 2, 2, 2]
    assert lines[2]["validation"] == {"radius": 2.5, "direction": 0.0, "class_l": 0.0, "total": 2.5}
    w = torch.load(run / "smart-tree_model_weights.pt", weights_only=True)
    assert float(next(iter(w.values())).flatten()[0]) == 1.0
    ck = torch.load(run / "last.pt", weights_only=True)
    assert ck["scheduler"]["last_epoch"] == (4 if lr_decay else 0) and ck["epochs_no_improve"] == 2 and ck["stopped"]
    assert not (run / "captures").exists()
    assert T.main(_args(data, run, "cpu", num_epoch=10, resume=run))["epochs"] == 4  # a stopped run stays stopped
    assert len(trained) == 4


def test_tracker_and_metrics_sink(tmp_path):
    t = Tracker()
    for v in (1.0, 2.0):
        t.update({"radius": torch.tensor(v), "direction": torch.tensor(2 * v), "class_l": torch.tensor(0.5)})
    assert (t.radius_loss, t.direction_loss, t.class_loss, t.total_loss) == (1.5, 3.0, 0.5, 5.0)
    sink = MetricsSink(tmp_path / "m.jsonl")
    t.log("Training", 0, sink)
    sink.log({"lr": 0.1}, step=0)
    t.log("Training", 1, sink)  # a new step commits the previous one
    sink.commit()
    lines = read_metrics(tmp_path / "m.jsonl")
    assert lines[0] == {"epoch": 0, "Training": t.as_dict(), "lr": 0.1} and lines[1]["epoch"] == 1
    sink.truncate(1)
    assert len(read_metrics(tmp_path / "m.jsonl")) == 1


def test_to_labelled_clds_slices_the_batch():
    from smart_tree_amd.model.helper import to_labelled_clds

    ids = torch.tensor([0, 0, 1, 1, 1])
    xyz = torch.arange(15.0).reshape(5, 3)
    out = {"radius": torch.zeros(5, 1), "direction": torch.ones(5, 3), "class_l": torch.tensor([[0, 1.0]] * 2 + [[1.0, 0]] * 3)}
    out["radius"][2] = math.log(2.0)
    a, b = to_labelled_clds(ids, xyz, None, out, None, ["x/a.npz", "b.npz"])
    assert torch.equal(a.xyz, xyz[:2]) and torch.equal(b.xyz, xyz[2:]) and a.filename.stem == "a" and a.rgb is None
    assert a.class_l.view(-1).tolist() == [1, 1] and b.class_l.view(-1).tolist() == [0, 0, 0]
    assert b.medial_vector[0].tolist() == [2.0, 2.0, 2.0] and b.medial_vector[1].tolist() == [1.0, 1.0, 1.0]


# ----------------------------------------------------------------------------------------------------------- end to end


def _hand_loop(data, device, epochs, capture, lr=0.1, fp16=False):
    """The reference's main written out with this package's pieces: seed 42, the three loaders, the model, Adam,
    ReduceLROnPlateau, one GradScaler; per epoch train, validation, test, the captures' passes over test and validation (they
    draw crops too), the scheduler and the best weights.  Returns (model, [(train, validation, test)], best state_dict,
    {split: {tree stem: input xyz of the capture pass}})."""
    from smart_tree_amd.dataset.augmentations import AugmentationPipeline, RandomCubicCrop
    from smart_tree_amd.dataset.dataset import TreeDataset
    from smart_tree_amd.model.sparse import batch_collate

    torch.manual_seed(42)
    torch.cuda.manual_seed_all(42)

    def loader(mode):
        ds = TreeDataset(0.05, data / "split.json", data, mode, ["xyz"], ["radius", "direction", "class_l"],
                         augmentation=AugmentationPipeline([RandomCubicCrop(4.0)]), cache=mode == "validation", device=device)
        return torch.utils.data.DataLoader(ds, batch_size=2, collate_fn=batch_collate)

    tr, va, te = loader("train"), loader("validation"), loader("test")
    net = TrainableSmartTree(*NETWORK).to(device).train()
    opt = torch.optim.Adam(net.parameters(), lr=lr)
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode="min")
    scaler = torch.amp.GradScaler(device.type, enabled=fp16)
    best, best_sd, lines, captured = math.inf, None, [], {}
    for epoch in range(epochs):
        t = T.train_epoch(tr, net, opt, LOSS_FN, device, fp16=fp16, scaler=scaler)
        v = T.eval_epoch(va, net, LOSS_FN, device, fp16=fp16)
        s = T.eval_epoch(te, net, LOSS_FN, device, fp16=fp16)
        if (epoch + 1) % capture == 0:
            for split, ld in (("test", te), ("validation", va)):
                for (feats, _), coords, _, names in ld:
                    for i, name in enumerate(names):
                        captured.setdefault(epoch, {}).setdefault(split, {})[name[:-4]] = feats[coords[:, 0] == i, :3].cpu()
        vt = v["radius"] + v["direction"] + v["class_l"]
        sched.step(vt)
        if vt < best:
            best, best_sd = vt, {k: x.detach().cpu().clone() for k, x in net.state_dict().items()}
        lines.append((t, v, s))
    return net, lines, best_sd, captured


def _assert_same_state(a, b):
    assert list(a) == list(b)
    for k in a:
        assert torch.equal(a[k].cpu(), b[k].cpu()), k


def test_run_end_to_end(backend, data, tmp_path):
    from smart_tree_amd.model.model import Smart_Tree
    from smart_tree_amd.util.file import load_cloud

    run = tmp_path / "run"
    T.main(_args(data, run, backend))
    assert (run / "config.yaml").is_file() and (run / "last.pt").is_file()
    saved_cfg = C.load_yaml(run / "config.yaml")
    assert saved_cfg["train_dataset"]["voxel_size"] == 0.05 and saved_cfg["device"] == str(backend)
    lines = read_metrics(run / "metrics.jsonl")
    assert [r["epoch"] for r in lines] == [0, 1, 2]
    assert all(math.isfinite(v) for r in lines for s in SPLITS for v in r[s].values())
    net, hand, best_sd, captured = _hand_loop(data, backend, 3, 2)
    for r, (t, v, s) in zip(lines, hand):  # bit-identical logged losses
        for split, means in zip(SPLITS, (t, v, s)):
            assert {k: r[split][k] for k in means} == means, (r["epoch"], split)
    ck = torch.load(run / "last.pt", weights_only=True)
    _assert_same_state(ck["model"], net.state_dict())
    w = torch.load(run / "smart-tree_model_weights.pt", weights_only=True)
    _assert_same_state(w, best_sd)
    TrainableSmartTree(*NETWORK).load_state_dict(w, strict=True)
    Smart_Tree(w, device=backend)
    assert sorted(p.name for p in (run / "captures").iterdir()) == ["epoch_1"]
    for split in ("validation", "test"):
        files = sorted((run / "captures" / "epoch_1" / split).iterdir())
        assert [f.name for f in files] == NAMES
        for f in files:
            c = load_cloud(f)
            xyz = captured[1][split][f.stem]
            assert torch.equal(c.xyz, xyz)  # one row per voxel: the capture pass's representative points
            assert c.medial_vector.shape == (len(xyz), 3) and c.class_l.shape == (len(xyz), 1)
            assert set(c.class_l.view(-1).tolist()) <= {0.0, 1.0}  # (medial vectors may overflow: exp of an lr=0.1 radius)


def _resume_matches(data, tmp_path, device, **kw):
    whole, part = tmp_path / "whole", tmp_path / "part"
    T.main(_args(data, whole, device, num_epoch=4, **kw))
    T.main(_args(data, part, device, num_epoch=2, **kw))
    assert len(read_metrics(part / "metrics.jsonl")) == 2
    T.main(_args(data, "elsewhere", device, num_epoch=4, resume=part, **kw))  # writes into part, not run_dir
    a, b = torch.load(whole / "last.pt", weights_only=True), torch.load(part / "last.pt", weights_only=True)
    _assert_same_state(a["model"], b["model"])
    drop = lambda r: {k: v for k, v in r.items() if k != "seconds"}
    la, lb = read_metrics(whole / "metrics.jsonl"), read_metrics(part / "metrics.jsonl")
    assert [drop(r) for r in la] == [drop(r) for r in lb] and len(lb) == 4
    assert a["scaler"] == b["scaler"] and a["best"] == b["best"]
    w = [p / "smart-tree_model_weights.pt" for p in (whole, part)]
    assert w[0].exists() == w[1].exists()  # no weights when no validation total was finite
    if w[0].exists():
        _assert_same_state(*(torch.load(p, weights_only=True) for p in w))
    return a


def test_resume_reproduces_the_uninterrupted_run(backend, data, tmp_path):
    _resume_matches(data, tmp_path, backend)


# ----------------------------------------------------------------------------------------------------------------- GPU


@pytest.mark.gpu
def test_fp16_run_and_resume(data, tmp_path):
    """At the default lr=0.1 no epoch's fp16 validation total of these two trees is finite (no weights file; measured, cause not
    traced); at lr=1e-2 every term is finite."""
    _resume_matches(data, tmp_path / "lr0.1", "cuda:0", fp16=True)
    ck = _resume_matches(data, tmp_path, "cuda:0", fp16=True, lr=1e-2)
    assert ck["scaler"]["scale"] > 0 and "_growth_tracker" in ck["scaler"]
    lines = read_metrics(tmp_path / "whole" / "metrics.jsonl")
    assert all(math.isfinite(v) for r in lines for s in SPLITS for v in r[s].values())


@pytest.mark.gpu
def test_long_run_lowers_the_loss_and_feeds_run_smart_tree(data, tmp_path):
    """30 float32 epochs at lr=1e-2 from seed 42, then the best weights as run-smart-tree's weights_path."""
    from smart_tree_amd import cli
    from smart_tree_amd.data_types.cloud import Cloud
    from smart_tree_amd.synthetic import sample_tree_cloud

    run = tmp_path / "run"
    T.main(_args(data, run, "cuda:0", num_epoch=30, lr=1e-2, capture_output=0))
    lines = read_metrics(run / "metrics.jsonl")
    first, last = lines[0]["train"]["total"], lines[-1]["train"]["total"]
    seconds = [r["seconds"] for r in lines]
    print(f"train total {first:.4f} -> {last:.4f} ({last / first:.3f}) over {len(lines)} epochs; "
          f"seconds per epoch: first {seconds[0]:.3f}, median {float(np.median(seconds)):.3f}")
    assert last <= 0.7 * first
    weights = run / "smart-tree_model_weights.pt"
    cfg = cli.load_config([f"pipeline.model_inference.weights_path={weights}", "pipeline.model_inference.voxel_size=0.05"])
    pipe = cli.instantiate(cfg["pipeline"])
    c = sample_tree_cloud(20000, seed=7, scale=0.6, max_depth=3, foliage_fraction=0.3)
    skeleton = pipe.process_cloud(cloud=Cloud.from_numpy(xyz=c["xyz"], rgb=c["rgb"]))
    print("skeletons:", len(skeleton.skeletons), "branches:", sum(len(t.branches) for t in skeleton.skeletons))
    assert hasattr(skeleton, "skeletons")
