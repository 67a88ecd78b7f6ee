"""Training-step timing: TrainableSmartTree (noble-elevator-58 start) on one batch of BASELINE.json configs[1]'s cloud (1M-point
synthetic tree, 2 cm voxels, every block in one batch), Adam.  Prints one JSON line:

  ms per step split into forward (network + loss), backward and optimizer (CUDA events, mean over the timed steps);
  the weight-gradient family: every st_sparse_conv_wgrad call of one backward pass replayed and timed on its own, next to the
  forward of the same layer (st_sparse_conv_fwd, same tensors): time, the ratio wgrad / forward, and the fraction of the HBM peak at
  the forward's algorithmic bytes P * (Cin * 4 + 4) + n_out * Cout * 4 (P = live pairs; pointwise: P = n_out, no index bytes).

    python tools/bench_train.py [--steps 10] [--warmup 3] [--points 1000000] [--voxel 0.02] [--fp16]

--fp16: the AMP step (forward + loss under float16 autocast, backward of the scaled loss, GradScaler + Adam) on the same batch; the
family is then every st_sparse_conv_wgrad_h call next to the st_sparse_conv_h_fwd of the same layer (bytes at 2 per feature element).
"""
import argparse
import functools
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import unet_oracle as uo  # noqa: E402
from smart_tree_amd.data_types.cloud import Cloud  # noqa: E402
from smart_tree_amd.model import loss as L  # noqa: E402
from smart_tree_amd.model import sparse_grad as sg  # noqa: E402
from smart_tree_amd.model import sparse_ops as ops  # noqa: E402
from smart_tree_amd.model.model_inference import SingleTreeInference  # noqa: E402
from smart_tree_amd.model.sparse import sparse_from_batch  # noqa: E402
from smart_tree_amd.model.trainable import TrainableSmartTree  # noqa: E402
from smart_tree_amd.synthetic import sample_tree_cloud  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec (bench.py's constant)


def _events_ms(fn, reps):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--voxel", type=float, default=0.02)
    ap.add_argument("--reps", type=int, default=10, help="replays per wgrad / forward layer timing")
    ap.add_argument("--fp16", action="store_true", help="mixed precision: float16 autocast + GradScaler (half convolution kernels)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")

    c = sample_tree_cloud(args.points, seed=0)
    cloud = Cloud(xyz=torch.from_numpy(c["xyz"]).to(dev), rgb=torch.from_numpy(c["rgb"]).to(dev))
    cloud = Cloud(cloud.xyz - cloud.xyz.mean(0), cloud.rgb)
    block, buffer = 4.0, 0.4
    vb = SingleTreeInference(cloud, args.voxel, block, buffer).batch
    hint = (int(vb.block_centres.shape[0]), int(round((block + 2 * buffer) / args.voxel)) + 2)
    sp = sparse_from_batch(vb.feats[:, :3].contiguous(), vb.coords, device=dev, blk_seg=vb.blk_seg, n_seg=vb.n_seg, brick_hint=hint)
    n = sp.features.shape[0]
    g = torch.Generator().manual_seed(0)
    targets = torch.cat([torch.rand(n, 1, generator=g) * 0.19 + 0.01, torch.nn.functional.normalize(torch.randn(n, 3, generator=g)),
                         (torch.rand(n, 1, generator=g) < 0.4).float()], 1).to(dev)
    mask = vb.mask.to(dev).bool() if vb.mask is not None else None

    net = TrainableSmartTree.from_state_dict(uo.load_weights(ROOT / "smart_tree_amd" / "model" / "weights" / "noble-elevator-58.npz"))
    net = net.to(dev).train()
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    loss_fn = functools.partial(L.compute_loss, radius_loss_fn=L.L1Loss, direction_loss_fn=L.cosine_similarity_loss,
                                class_loss_fn=L.focal_loss, target_radius_log=True, vector_class=0)

    ev = lambda: torch.cuda.Event(enable_timing=True)
    phases = {"forward": [], "backward": [], "optimizer": []}
    scaler = torch.amp.GradScaler("cuda") if args.fp16 else None
    amp = lambda: torch.autocast("cuda", dtype=torch.float16, enabled=args.fp16)
    for step in range(args.warmup + args.steps):
        e0, e1, e2, e3 = ev(), ev(), ev(), ev()
        e0.record()
        with amp():
            loss = loss_fn(net(sp), targets, mask)
            total = sum(loss.values())
        e1.record()
        (scaler.scale(total) if args.fp16 else total).backward()
        e2.record()
        if args.fp16:
            scaler.step(opt)
            scaler.update()
        else:
            opt.step()
        opt.zero_grad()
        e3.record()
        torch.cuda.synchronize()
        if step >= args.warmup:
            phases["forward"].append(e0.elapsed_time(e1))
            phases["backward"].append(e1.elapsed_time(e2))
            phases["optimizer"].append(e2.elapsed_time(e3))
    ms = {k: float(np.mean(v)) for k, v in phases.items()}

    # the wgrad family: record the calls of one backward pass, replay each one on its own next to the layer's forward
    calls = []
    real = sg.conv_wgrad
    fwd = ops.sparse_conv_half if args.fp16 else ops.sparse_conv
    esz = 2 if args.fp16 else 4

    def recording(x0, x1, nbr, n_out, dy, K):
        if x0.element_size() == esz:  # (--fp16: the float32 convolution behind the direction head is not of the family)
            calls.append((x0, x1, nbr, n_out, dy, K))
        return real(x0, x1, nbr, n_out, dy, K)

    sg.conv_wgrad = recording
    try:
        with amp():
            total = sum(loss_fn(net(sp), targets, mask).values())
        total.backward()
    finally:
        sg.conv_wgrad = real
    opt.zero_grad()
    layers, tot_w, tot_f, tot_bytes = [], 0.0, 0.0, 0
    for x0, x1, nbr, n_out, dy, K in calls:
        cin = x0.shape[1] + (x1.shape[1] if x1 is not None else 0)
        cout = dy.shape[1]
        w = torch.randn(K, cin, cout, device=dev, dtype=x0.dtype)
        t_w = _events_ms(lambda: real(x0, x1, nbr, n_out, dy, K), args.reps)
        t_f = _events_ms(lambda: fwd(x0, w, nbr, n_out, x1=x1), args.reps)
        pairs = int((nbr >= 0).sum()) if nbr is not None else n_out
        nbytes = pairs * (cin * esz + (4 if nbr is not None else 0)) + n_out * cout * esz
        layers.append({"K": K, "cin": cin, "cout": cout, "n_out": n_out, "pairs": pairs, "wgrad_ms": round(t_w, 4),
                       "fwd_ms": round(t_f, 4), "ratio": round(t_w / t_f, 2), "wgrad_hbm_frac": round(nbytes / (t_w * 1e-3) / 1e9 / HBM_PEAK_GBS, 3)})
        tot_w, tot_f, tot_bytes = tot_w + t_w, tot_f + t_f, tot_bytes + nbytes
    out = {"metric": "train_step_fp16" if args.fp16 else "train_step", "voxels": n, "steps": args.steps, "warmup": args.warmup,
           "ms_per_step": round(sum(ms.values()), 3), "ms": {k: round(v, 3) for k, v in ms.items()},
           "loss_last": {k: float(v.detach()) for k, v in loss.items()},
           "wgrad": {"calls": len(calls), "ms_total": round(tot_w, 3), "fwd_ms_total_same_layers": round(tot_f, 3),
                     "ratio_total": round(tot_w / tot_f, 2), "hbm_frac": round(tot_bytes / (tot_w * 1e-3) / 1e9 / HBM_PEAK_GBS, 3),
                     "layers_over_2x_forward": sum(1 for l in layers if l["ratio"] > 2.0), "layers": layers},
           "timestamp": time.strftime("%Y-%m-%dT%H:%M:%S")}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
