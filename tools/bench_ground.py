"""Time the terrain calls (smart_tree_amd/terrain.py, csrc/ground.hip):
python tools/bench_ground.py [--points 1000000] [--set 20] [--repeats 9] [--cell 0.5] [--out profiles/ground_bench.json]

Input: a seeded 40 x 30 m plot made on the device -- terrain of slope 0.2 with 0.6 m and 0.4 m undulations and 1 cm noise under a
third of the points, 25 trunks with crowns and 30 shrubs in the rest -- alone and as a launch set of `--set` copies.

Recorded per size: each of the three calls alone (st_ground_extent, st_ground_model, st_ground_height through terrain.ground_extent /
ground_raster / ground_height: one call ended by a synchronise, and the time per call of `--chain` calls enqueued back to back between
two device events, which leaves the launch latency out), a whole `ground_model` (the read-back of the dimensions included), and the
yardstick, the raster and its opening as a torch expression on the same GPU: `scatter_reduce(amin)` for the per-cell minima and
`max_pool2d` on the negated and the plain raster for every window.  The script asserts that the yardstick and the kernels agree in
every bit of the surface and the flags.  Times are median / min / max in ms after a warm-up."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np
import torch
import torch.nn.functional as F

from smart_tree_amd import terrain as T
from smart_tree_amd.data_types.cloud import Cloud


def stats(ms):
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms)}


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return stats(ms)


def chained(fn, chain, warmup, repeats):
    """ms per call of `chain` calls enqueued back to back, between two device events."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(chain):
            fn()
        end.record()
        torch.cuda.synchronize()
        ms.append(start.elapsed_time(end) / chain)
    return stats(ms)


def plot(n, dev, seed=0):
    """[n,3] float32 on the device, up = 1."""
    g = torch.Generator(device=dev).manual_seed(seed)
    u = lambda *shape: torch.rand(*shape, generator=g, device=dev, dtype=torch.float64)
    terrain = lambda x, z: 0.2 * x + 0.6 * torch.sin(x / 6.0) + 0.4 * torch.cos(z / 4.0)
    n_ground = n // 3
    n_tree = (n - n_ground) * 9 // 10
    gx, gz = u(n_ground) * 40, u(n_ground) * 30
    parts = [torch.stack([gx, terrain(gx, gz) + 0.01 * torch.randn(n_ground, generator=g, device=dev, dtype=torch.float64), gz], 1)]
    for count, objects, spread, tall in ((n_tree, 25, 1.8, 12.0), (n - n_ground - n_tree, 30, 0.5, 1.0)):
        centre = torch.stack([2 + u(objects) * 36, 2 + u(objects) * 26], 1)
        which = torch.randint(objects, (count,), generator=g, device=dev)
        d = (u(count, 2) * 2 - 1) * spread * u(count, 1)
        x, z = centre[which, 0] + d[:, 0], centre[which, 1] + d[:, 1]
        parts.append(torch.stack([x, terrain(x, z) + u(count) * tall * (0.5 + u(objects)[which]), z], 1))
    pts = torch.cat(parts)
    return pts[torch.randperm(n, generator=g, device=dev)].float().contiguous()


def torch_model(pts, cell, w, dh, up=1):
    """(surface [A,B], flags [A,B]) of one cloud by the contract's rules in plain torch: the yardstick."""
    a, b = (1 if up == 0 else 0), (1 if up == 2 else 2)
    p = pts[torch.isfinite(pts).all(1)]
    plan = p[:, [a, b]]
    origin = plan.amin(0)
    # (the divisor as a device tensor: by a host scalar torch multiplies with the reciprocal, which rounds differently)
    q = torch.floor((plan - origin) / torch.tensor(cell, dtype=torch.float32, device=pts.device)).long()
    A, B = (int(v) for v in (q.amax(0) + 1).tolist())
    z = torch.full((A * B,), float("inf"), device=pts.device).scatter_reduce_(0, q[:, 0] * B + q[:, 1], p[:, up], "amin").reshape(1, 1, A, B)
    flags = torch.isinf(z).to(torch.uint8)
    for wk, dk in zip(w.tolist(), dh.tolist()):
        e = -F.max_pool2d(-z, 2 * wk + 1, stride=1, padding=wk)
        o = F.max_pool2d(torch.where(torch.isfinite(e), e, torch.full_like(e, float("-inf"))), 2 * wk + 1, stride=1, padding=wk)
        o = torch.where(torch.isinf(o), torch.full_like(o, float("inf")), o)
        hit = (z - o) > dk
        flags = flags | (hit.to(torch.uint8) * 2)
        z = torch.where(hit, o, z)
    return z.reshape(A, B), flags.reshape(A, B)


def measure(cloud, args, warmup, repeats):
    pts, seg_off = cloud.xyz, cloud.seg_off
    w, dh = T.windows(args.cell, args.max_window)
    model = T.ground_model(cloud, cell=args.cell, max_window=args.max_window)
    origin, dims, cell_off = model.origin, model.dims, model.cell_off
    out = {"points": int(pts.shape[0]), "clouds": cloud.n_seg, "cell": args.cell, "windows": w.tolist(), "thresholds": [float(v) for v in dh],
           "raster": dims[0].tolist(), "cells": int(cell_off[-1]), "ground_points": int(model.is_ground.sum()),
           "cells_not_ground": int((model.flags & 2).ne(0).sum()), "workspace_MB": T._lib.lib().st_ground_workspace_bytes(int(cell_off[-1])) / 2 ** 20}
    parts = cloud.split()
    for k in sorted({0, len(parts) - 1}):
        surface, flags = torch_model(parts[k].xyz, args.cell, w, dh)
        got_s, got_f = model.raster(k)
        assert torch.equal(got_s.view(torch.int32), surface.view(torch.int32)), f"the kernel and the torch expression differ in the surface of cloud {k}"
        assert torch.equal(got_f, flags), f"the kernel and the torch expression differ in the flags of cloud {k}"
    out["equals_torch"] = True
    again = T.ground_model(cloud, cell=args.cell, max_window=args.max_window)
    out["two_runs_identical"] = bool(torch.equal(again.surface.view(torch.int32), model.surface.view(torch.int32)) and torch.equal(again.flags, model.flags)
                                     and torch.equal(again.is_ground, model.is_ground))
    calls = {"extent": lambda: T.ground_extent(pts, seg_off, args.cell, 1),
             "model": lambda: T.ground_raster(pts, seg_off, origin, dims, cell_off, w, dh, args.cell, 1),
             "height": lambda: T.ground_height(pts, seg_off, origin, dims, cell_off, model.surface, args.cell, 1, 0.2)}
    for name, fn in calls.items():
        out[f"{name}_ms"] = timed(fn, warmup, repeats)
        out[f"{name}_chained_ms"] = chained(fn, args.chain, warmup, repeats)
    out["three_calls_chained_ms"] = sum(out[f"{name}_chained_ms"]["median"] for name in calls)
    out["ground_model_ms"] = timed(lambda: T.ground_model(cloud, cell=args.cell, max_window=args.max_window), warmup, repeats)
    yardstick = lambda: [torch_model(c.xyz, args.cell, w, dh) for c in parts]
    out["torch_ms"] = timed(yardstick, warmup, repeats)
    out["torch_chained_ms"] = chained(yardstick, max(args.chain // 4, 1), warmup, repeats)
    hip = out["extent_chained_ms"]["median"] + out["model_chained_ms"]["median"]  # what the yardstick computes: extent, raster, opening
    out["torch_over_hip_chained"] = out["torch_chained_ms"]["median"] / hip
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--set", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--chain", type=int, default=20)
    ap.add_argument("--cell", type=float, default=0.5)
    ap.add_argument("--max-window", dest="max_window", type=float, default=8.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_ground.py measures on the GPU"
    dev = torch.device("cuda:0")
    cloud = Cloud(xyz=plot(args.points, dev))
    res = {"device": torch.cuda.get_device_name(0), "points": args.points, "repeats": args.repeats, "warmup": args.warmup, "chain": args.chain,
           "what": "st_ground_extent / st_ground_model / st_ground_height through terrain.py; median, min, max in ms; *_ms: one call ended by a "
                   "synchronise, *_chained_ms: per call of `chain` calls between two device events; torch_*: extent, raster and opening by amin, "
                   "scatter_reduce(amin) and max_pool2d, one cloud after the other; torch_over_hip_chained: against extent + model"}
    res["one_cloud"] = measure(cloud, args, args.warmup, args.repeats)
    if args.set > 1:
        B, n = args.set, cloud.xyz.shape[0]
        batch = Cloud(xyz=cloud.xyz.repeat(B, 1), seg_off=torch.arange(B + 1, dtype=torch.int32, device=dev) * n)
        res["launch_set"] = measure(batch, args, 1, max(3, args.repeats // 2))
    print(json.dumps(res))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
