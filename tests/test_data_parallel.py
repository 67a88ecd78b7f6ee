"""Data-parallel training (model/data_parallel.py, model/sync_bn.py, train.py `group=`): spawned gloo ranks, each loading the kernels
itself (the emulator on CPU, the HIP library on cuda:0 under -m gpu), against one process given the whole batch with torch BatchNorm.

Step: loss terms, gradients, the SGD-updated parameters and the running statistics equal the one-process step (gradients within
1e-4 of each tensor's max |g| against a one-rank group on the same module, TORCH_BN_GRAD_BAR against torch's BatchNorm1d);
parameters are bit-identical across ranks.  W = 3 over 2 trees leaves a rank without a tree.
Run: a 2-rank `run(cfg)` writes the one-process run's files, and resuming it after epoch 1 reproduces the uninterrupted run."""
import functools
import json
import math
import os
import socket
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from smart_tree_amd.model import loss as L

ROOT = Path(__file__).resolve().parents[1]
NETWORK = (3, [8, 16, 32], [8, 8, 4, 1], [8, 8, 4, 3], [8, 8, 4, 2])
LOSS_FN = functools.partial(L.compute_loss, radius_loss_fn=L.L1Loss, direction_loss_fn=L.cosine_similarity_loss,
                            class_loss_fn=L.focal_loss, target_radius_log=True, vector_class=0)
CHILD_TIMEOUT = 600


def _write_trees(d: Path, n: int):
    """n trees cut from one synthetic tree: tree k drops every (k + 2)-th point but keeps the six extreme points, so every tree has
    other rows but the same voxel extent.  The strided convolutions' output set depends on the batch's extent (spconv's
    spatial_shape, DESIGN.md "Training: data parallel"): only then are a shard's coarse levels those of the whole batch."""
    from smart_tree_amd.synthetic import sample_tree_cloud

    d.mkdir(parents=True, exist_ok=True)
    c = sample_tree_cloud(5000, seed=1, scale=0.6, max_depth=3, foliage_fraction=0.3)
    m = len(c["xyz"])
    extremes = np.concatenate([c["xyz"].argmin(0), c["xyz"].argmax(0)])
    names = []
    for k in range(n):
        keep = np.arange(m) % (k + 2) != 1
        keep[extremes] = True
        np.savez(d / f"tree_{k}.npz", **{key: c[key][keep] for key in ("xyz", "rgb", "medial_vector", "class_l")})
        names.append(f"tree_{k}.npz")
    (d / "split.json").write_text(json.dumps({"train": names, "validation": names, "test": names}))
    return names


def _loader(d: Path, n: int, device):
    from smart_tree_amd.dataset.dataset import TreeDataset
    from smart_tree_amd.model.sparse import batch_collate

    ds = TreeDataset(0.05, d / "split.json", d, "train", ["xyz"], ["radius", "direction", "class_l"], device=device)
    return torch.utils.data.DataLoader(ds, batch_size=n, collate_fn=batch_collate)


class _RecordingSGD(torch.optim.SGD):
    """SGD that keeps the gradients it steps with (after GradScaler's unscale) and whether it was stepped."""

    def step(self, closure=None):
        self.grads = [p.grad.detach().cpu().clone() for p in self.param_groups[0]["params"]]
        self.stepped = getattr(self, "stepped", 0) + 1
        return super().step(closure)


def _use_kernels(device):
    from smart_tree_amd import _lib

    if device.type == "cpu":
        import ctypes
        import sys

        sys.path.insert(0, str(ROOT / "tests" / "hipemu"))
        import build as emu_build

        _lib._LIB = _lib.declare(ctypes.CDLL(os.environ.get("SMARTTREE_EMU_LIB") or str(emu_build.build())))
        _lib._ALLOW_HOST_POINTERS = True
    else:
        _lib._LIB = None
        _lib.lib()


def _step(loader, device, group, fp16, steps=1):
    """Seed 0, the network, SGD(lr 0.1), `steps` train_epoch calls; the model's state after them."""
    from smart_tree_amd.model import train as T
    from smart_tree_amd.model.sync_bn import convert_sync_batchnorm
    from smart_tree_amd.model.trainable import TrainableSmartTree

    torch.manual_seed(0)
    net = TrainableSmartTree(*NETWORK).to(device).train()
    if group is not None:
        convert_sync_batchnorm(net, group)
    opt = _RecordingSGD(net.parameters(), lr=0.1)
    scaler = torch.amp.GradScaler(device.type, enabled=fp16) if fp16 else None
    means = [T.train_epoch(loader, net, opt, LOSS_FN, device, fp16=fp16, scaler=scaler, **({"group": group} if group else {}))
             for _ in range(steps)]
    return {"means": means, "grads": [g.numpy() for g in opt.grads], "stepped": getattr(opt, "stepped", 0),
            "state": {k: v.detach().cpu().numpy() for k, v in net.state_dict().items()},
            "scale": float(scaler.get_scale()) if scaler else None}


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _init(rank, world, port, device):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    if device.type == "cuda":
        torch.cuda.set_device(device)
    _use_kernels(device)
    dist.init_process_group("gloo", rank=rank, world_size=world)


def _step_worker(rank, world, port, data, n_trees, device, fp16, steps, q):
    device = torch.device(device)
    _init(rank, world, port, device)
    try:
        out = _step(_loader(Path(data), n_trees, device), device, dist.group.WORLD, fp16, steps)
        q.put((rank, out))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def _spawn(target, world, *args):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=target, args=(r, world, port, *args, q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        got = dict(q.get(timeout=CHILD_TIMEOUT) for _ in range(world))
    finally:
        for p in procs:
            p.join(timeout=CHILD_TIMEOUT)
            if p.is_alive():
                p.kill()
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    return [got[r] for r in range(world)]


def _compare(one, ranks, grad_tol, what):
    for out in ranks[1:]:  # replicas: bit-identical parameters and buffers
        for k in ranks[0]["state"]:
            assert np.array_equal(ranks[0]["state"][k], out["state"][k], equal_nan=True), (what, k)
    dp = ranks[0]
    for a, b in zip(one["means"], dp["means"]):
        for k in a:
            assert math.isclose(a[k], b[k], rel_tol=1e-5, abs_tol=1e-6), (what, k, a[k], b[k])
    worst = 0.0
    for i, (a, b) in enumerate(zip(one["grads"], dp["grads"])):
        scale = float(np.abs(a).max())
        err = float(np.abs(a - b).max())
        worst = max(worst, err / scale if scale else err)
        assert err <= grad_tol * max(scale, 1e-30), (what, i, err, scale)
    for k, a in one["state"].items():
        b = dp["state"][k]
        if a.dtype.kind == "f":
            assert np.allclose(a, b, rtol=1e-5, atol=grad_tol * 0.1 * max(float(np.abs(a).max()), 1.0)), (what, k)  # lr 0.1
        else:
            assert np.array_equal(a, b), (what, k)
    return worst


TORCH_BN_GRAD_BAR = 1e-2  # the new BatchNorm against torch's BatchNorm1d in the same one-process step: measured 6.5e-3 of max|g| on
# the emulator (the BatchNorm bias gradients: sums of dy that cancel, float64 in st_bn_backward_stats, float32 in torch)


def _step_equivalence(device, tmp_path):
    """The W-rank step against (a) one process with torch BatchNorm and (b) a one-rank group on the same module: the gradients
    within 1e-4 of each tensor's max |g| of (b), within TORCH_BN_GRAD_BAR of (a)."""
    for world, n_trees in ((2, 3), (3, 2)):  # 3 ranks over 2 trees: rank 2 owns none
        d = tmp_path / f"w{world}"
        _write_trees(d, n_trees)
        one = _step(_loader(d, n_trees, device), device, None, False)
        single_group = _spawn(_step_worker, 1, str(d), n_trees, str(device), False, 1)
        ranks = _spawn(_step_worker, world, str(d), n_trees, str(device), False, 1)
        worst_torch = _compare(one, ranks, TORCH_BN_GRAD_BAR, f"W={world} vs torch BatchNorm")
        worst = _compare(single_group[0], ranks, 1e-4, f"W={world} vs one rank")
        print(f"W={world}, {n_trees} trees: worst gradient difference {worst:.2e} of max|g| against a one-rank group, "
              f"{worst_torch:.2e} against torch BatchNorm")


def test_step_equals_one_process_step(backend, tmp_path):
    _step_equivalence(backend, tmp_path)


# Twice the largest gradient difference measured, W = 2 against a one-rank group after two AMP steps: 0.254 of max|g| on the MI355X,
# 8.8e-7 on the emulator.  The half convolutions' float32 sums split differently with the rows, and dy rounded to half amplifies
# that (the open AMP finding of DESIGN.md "Training: mixed precision": one AMP step is up to 0.44 of max|g64| from float64).
FP16_BAR = 0.51


def test_fp16_step_two_ranks_against_one_rank_group(backend, tmp_path):
    """Mixed precision: W = 2 against a one-rank group on the same (synchronised) module: the same scaler decisions, gradients within
    FP16_BAR of max |g| (both sides round to half at different row splits)."""
    d = tmp_path / "fp16"
    _write_trees(d, 2)
    one = _spawn(_step_worker, 1, str(d), 2, str(backend), True, 2)[0]
    two = _spawn(_step_worker, 2, str(d), 2, str(backend), True, 2)
    assert one["stepped"] == two[0]["stepped"] and one["scale"] == two[0]["scale"]
    for k in two[0]["state"]:
        assert np.array_equal(two[0]["state"][k], two[1]["state"][k], equal_nan=True), k
    worst = max(float(np.abs(a - b).max()) / max(float(np.abs(a).max()), 1e-30) for a, b in zip(one["grads"], two[0]["grads"]))
    print(f"fp16: W=2 vs one-rank group, worst gradient difference {worst:.2e} of max|g|")
    assert worst <= FP16_BAR


def test_refusals(backend):
    from smart_tree_amd.model import data_parallel as dp
    from smart_tree_amd.model import train as T
    from smart_tree_amd.model.trainable import TrainableSmartTree

    with pytest.raises(ValueError, match="dice_loss"):
        dp.check_loss_fn(functools.partial(L.compute_loss, radius_loss_fn=L.L1Loss, direction_loss_fn=L.cosine_similarity_loss,
                                           class_loss_fn=L.dice_loss))
    with pytest.raises(ValueError, match="foreign"):
        dp.check_loss_fn(lambda p, t, m: {})
    net = TrainableSmartTree(*NETWORK)
    with pytest.raises(ValueError, match="convert_sync_batchnorm"):
        T._data_parallel([], net, LOSS_FN, group=object())


# -------------------------------------------------------------------------------------------------------------------- run


def _args(data, run_dir, device, **kw):
    a = {"directory": data, "json_path": data / "split.json", "voxel_size": 0.05, "batch_size": 2, "device": device,
         "run_dir": run_dir, "fp16": False, "capture_output": 2, "num_epoch": 3}
    a.update(kw)
    return [f"{k}={v}" for k, v in a.items()]


def _run_worker(rank, world, port, data, out, device, q):
    from smart_tree_amd.model import train as T

    device = torch.device(device)
    _init(rank, world, port, device)
    try:
        data, out = Path(data), Path(out)
        T.run(T.load_training_config(_args(data, out / "whole", str(device))))
        T.run(T.load_training_config(_args(data, out / "part", str(device), num_epoch=1)))
        T.run(T.load_training_config(_args(data, "elsewhere", str(device), resume=out / "part")))
        q.put((rank, None))
    finally:
        dist.destroy_process_group()


def _same_state(a, b):
    assert list(a) == list(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_two_rank_run_and_resume(backend, tmp_path, monkeypatch):
    from smart_tree_amd import config as C
    from smart_tree_amd.model import train as T
    from smart_tree_amd.model.model import Smart_Tree
    from smart_tree_amd.model.tracker import read_metrics
    from smart_tree_amd.model.trainable import TrainableSmartTree

    data = tmp_path / "data"
    names = _write_trees(data, 2)
    monkeypatch.chdir(tmp_path)
    _spawn(_run_worker, 2, str(data), str(tmp_path), str(backend))
    whole, part = tmp_path / "whole", tmp_path / "part"
    lines = read_metrics(whole / "metrics.jsonl")
    assert [r["epoch"] for r in lines] == [0, 1, 2]
    assert all(math.isfinite(v) for r in lines for s in ("train", "validation", "test") for v in r[s].values())
    assert C.load_yaml(whole / "config.yaml")["world_size"] == 2
    w = torch.load(whole / "smart-tree_model_weights.pt", weights_only=True)
    TrainableSmartTree.from_state_dict(w)
    Smart_Tree(w, device=backend)
    for split in ("validation", "test"):
        assert sorted(f.name for f in (whole / "captures" / "epoch_1" / split).iterdir()) == names
    # resumed after epoch 1 == uninterrupted
    drop = lambda r: {k: v for k, v in r.items() if k != "seconds"}
    assert [drop(r) for r in read_metrics(part / "metrics.jsonl")] == [drop(r) for r in lines]
    a, b = torch.load(whole / "last.pt", weights_only=True), torch.load(part / "last.pt", weights_only=True)
    _same_state(a["model"], b["model"])
    assert a["world_size"] == 2 and len(a["rng_ranks"]) == 2
    # one rank cannot continue a 2-rank run
    with pytest.raises(ValueError, match="same number of ranks"):
        T.main(_args(data, "x", str(backend), num_epoch=4, resume=part))


@pytest.mark.gpu
def test_rccl_one_rank_group_step():
    """The RCCL (nccl backend) all-reduces of the synchronised BatchNorm, the loss and the gradients on a one-rank group on cuda:0:
    the step equals the one-process step."""
    dev = torch.device("cuda", 0)
    _use_kernels(dev)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    import tempfile

    with tempfile.TemporaryDirectory() as tmp:
        d = Path(tmp)
        _write_trees(d, 2)
        one = _step(_loader(d, 2, dev), dev, None, False)
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
        try:
            got = _step(_loader(d, 2, dev), dev, dist.group.WORLD, False)
            torch.cuda.synchronize()
        finally:
            dist.destroy_process_group()
    _compare(one, [got], 1e-4, "nccl W=1")
