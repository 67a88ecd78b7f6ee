"""Data-parallel training-step cost on one GPU: the step of tools/bench_train.py (noble-elevator-58 start, BASELINE.json configs[1]'s
1M-point synthetic tree at 2 cm, every block in one batch, Adam) with synchronised BatchNorm (model/sync_bn.py) on a one-rank nccl
(RCCL) group, against the same step with torch's BatchNorm1d.  Prints one JSON line:

  ms per step (median of the timed steps, CUDA events) for torch BatchNorm and for the data-parallel step (new BatchNorm kernels,
  the BatchNorm / loss / gradient all-reduces on a one-rank group), float32 and fp16;
  the BatchNorm kernels' share of the step: the four passes of every BatchNorm layer replayed on that layer's rows, summed;
  the all-reduces of one step timed on their own: 2 per BatchNorm layer ([sum|sumsq|n] and [sum dy|sum dy*xhat]), the loss
  counts and the flat gradient buffer.

A one-rank group measures what the new path costs, not how it scales: scaling across GPUs is unmeasured here.

    python tools/bench_train_dist.py [--steps 10] [--warmup 3] [--points 1000000] [--voxel 0.02]
"""
import argparse
import copy
import functools
import json
import os
import socket
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from oracle import unet_oracle as uo  # noqa: E402
from smart_tree_amd.data_types.cloud import Cloud  # noqa: E402
from smart_tree_amd.model import data_parallel as dp  # noqa: E402
from smart_tree_amd.model import loss as L  # noqa: E402
from smart_tree_amd.model import sync_bn as S  # noqa: E402
from smart_tree_amd.model.model_inference import SingleTreeInference  # noqa: E402
from smart_tree_amd.model.sparse import sparse_from_batch  # noqa: E402
from smart_tree_amd.model.trainable import TrainableSmartTree  # noqa: E402
from smart_tree_amd.synthetic import sample_tree_cloud  # noqa: E402

LOSS_FN = functools.partial(L.compute_loss, radius_loss_fn=L.L1Loss, direction_loss_fn=L.cosine_similarity_loss,
                            class_loss_fn=L.focal_loss, target_radius_log=True, vector_class=0)


def _events_ms(fn, reps):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def _batch(points, voxel, dev):
    c = sample_tree_cloud(points, seed=0)
    cloud = Cloud(xyz=torch.from_numpy(c["xyz"]).to(dev), rgb=torch.from_numpy(c["rgb"]).to(dev))
    cloud = Cloud(cloud.xyz - cloud.xyz.mean(0), cloud.rgb)
    block, buffer = 4.0, 0.4
    vb = SingleTreeInference(cloud, voxel, block, buffer).batch
    hint = (int(vb.block_centres.shape[0]), int(round((block + 2 * buffer) / voxel)) + 2)
    sp = sparse_from_batch(vb.feats[:, :3].contiguous(), vb.coords, device=dev, blk_seg=vb.blk_seg, n_seg=vb.n_seg, brick_hint=hint)
    n = sp.features.shape[0]
    g = torch.Generator().manual_seed(0)
    targets = torch.cat([torch.rand(n, 1, generator=g) * 0.19 + 0.01, torch.nn.functional.normalize(torch.randn(n, 3, generator=g)),
                         (torch.rand(n, 1, generator=g) < 0.4).float()], 1).to(dev)
    mask = vb.mask.to(dev).bool() if vb.mask is not None else None
    return sp, targets, mask


def _step_times(net, sp, targets, mask, fp16, group, steps, warmup):
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    scaler = torch.amp.GradScaler("cuda", enabled=fp16)
    times = []
    for step in range(warmup + steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        with torch.autocast("cuda", dtype=torch.float16, enabled=fp16):
            preds = net(sp)
            loss = LOSS_FN(preds, targets, mask) if group is None else dp.global_loss(LOSS_FN, preds, targets, mask, group)[0]
            total = sum(loss.values())
        scaler.scale(total).backward()
        if group is not None:
            dp.all_reduce_grads(net.parameters(), group)
        scaler.step(opt)
        scaler.update()
        opt.zero_grad()
        b.record()
        torch.cuda.synchronize()
        if step >= warmup:
            times.append(a.elapsed_time(b))
    return float(np.median(times))


def _bn_inputs(net, sp, fp16):
    rows = []
    hooks = [m.register_forward_pre_hook(lambda m, a: rows.append((m, a[0].detach().contiguous())))
             for m in net.modules() if isinstance(m, S.SyncBatchNorm)]
    with torch.autocast("cuda", dtype=torch.float16, enabled=fp16):
        net(sp)
    for h in hooks:
        h.remove()
    return rows


def _bn_kernel_ms(rows, reps):
    total = 0.0
    for m, x in rows:
        C = x.shape[1]
        dy = torch.randn_like(x)
        st = S.batch_stats(x)
        count = st[2 * C:].clone()
        mean = (st[:C] / count).float()
        invstd = torch.ones(C, device=x.device)
        sums = S.backward_stats(x, dy, mean, invstd)
        total += _events_ms(lambda: (S.batch_stats(x), S.apply(x, mean, invstd, m.weight, m.bias), S.backward_stats(x, dy, mean, invstd),
                                     S.backward_apply(x, dy, mean, invstd, m.weight, sums, count)), reps)
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--voxel", type=float, default=0.02)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    group = dist.group.WORLD
    try:
        sp, targets, mask = _batch(args.points, args.voxel, dev)
        base = TrainableSmartTree.from_state_dict(uo.load_weights(ROOT / "smart_tree_amd" / "model" / "weights" / "noble-elevator-58.npz"))
        out = {"voxels": int(sp.features.shape[0]), "world_size": 1, "backend": "nccl"}
        for fp16 in (False, True):
            tag = "fp16" if fp16 else "fp32"
            torch_bn = copy.deepcopy(base).to(dev).train()
            sync = S.convert_sync_batchnorm(copy.deepcopy(base), group).to(dev).train()
            t_torch = _step_times(torch_bn, sp, targets, mask, fp16, None, args.steps, args.warmup)
            t_sync = _step_times(sync, sp, targets, mask, fp16, group, args.steps, args.warmup)
            rows = _bn_inputs(sync, sp, fp16)
            bn_ms = _bn_kernel_ms(rows, args.reps)
            out[tag] = {"ms_per_step_torch_bn": t_torch, "ms_per_step_data_parallel": t_sync,
                        "overhead_ms": t_sync - t_torch, "bn_layers": len(rows),
                        "bn_rows": sorted({int(x.shape[0]) for _, x in rows}), "bn_kernels_ms": bn_ms,
                        "bn_kernels_share": bn_ms / t_sync}
        # the step's all-reduces on their own
        ar = []
        for m, x in rows:
            C = x.shape[1]
            ar += [torch.zeros(2 * C + 1, dtype=torch.float64, device=dev), torch.zeros(2 * C, dtype=torch.float64, device=dev)]
        small = _events_ms(lambda: [dist.all_reduce(t, group=group) for t in ar], args.reps)
        loss_vec = torch.zeros(5, dtype=torch.float64, device=dev)
        loss_ms = _events_ms(lambda: dist.all_reduce(loss_vec, group=group), args.reps)
        flat = torch.zeros(sum(p.numel() for p in base.parameters()), dtype=torch.float32, device=dev)
        grad_ms = _events_ms(lambda: dist.all_reduce(flat, group=group), args.reps)
        out["all_reduce"] = {"bn_count": len(ar), "bn_ms": small, "loss_ms": loss_ms, "grad_floats": int(flat.numel()),
                             "grad_ms": grad_ms, "per_step_ms": small + loss_ms + grad_ms}
        out["scaling"] = "unmeasured: one GPU, one-rank group"
        print(json.dumps(out))
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
