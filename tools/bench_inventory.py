"""Time the tree tally of a segmented cloud (smart_tree_amd/inventory.py, csrc/tree_tally.hip):
python tools/bench_inventory.py [--points 1000000] [--set 20] [--repeats 9] [--out profiles/inventory_bench.json]

Input: that of tools/bench_fit.py -- the seed-0 synthetic tree, centred as the pipeline centres it, and the skeleton the pipeline
gives for it on ground-truth medial vectors -- alone and as a launch set of `--set` copies, each against its own copy of the tubes.

Recorded per size: the tally alone (st_tree_tally through inventory.tree_tally: one call ended by a synchronise, and the time per
call of `--chain` calls enqueued back to back between two device events, which leaves the launch latency out), whole and with the
boxes and counts only; the tally beside the segmentation call it follows; a whole `measure_trees`
(segmentation included); and the yardstick, the same four outputs as a torch expression on the same GPU: `scatter_reduce` for the
boxes, `bincount` for the counts, `torch.unique` over packed 64-bit keys for the cells.  The script asserts that the yardstick and
the kernel agree.  Times are median / min / max in ms after a warm-up."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch

import bench
from smart_tree_amd import inventory as I
from smart_tree_amd import segmentation as S
from smart_tree_amd.data_types.cloud import Cloud
from smart_tree_amd.data_types.flat import FlatSkeletons
from smart_tree_amd.data_types.tree import DisjointTreeSkeleton
from smart_tree_amd.dataset.augmentations import CentreCloud
from smart_tree_amd.synthetic import sample_tree_cloud


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


def torch_tally(pts, tree, T, up, cell, layers):
    """The four outputs by the contract's rules in plain torch (one class): the yardstick."""
    ok = torch.isfinite(pts).all(1) & (tree >= 0) & (tree < T)
    p, t = pts[ok], tree[ok].long()
    idx = t[:, None].expand(-1, 3)
    lo = torch.full((T, 3), float("inf"), device=pts.device).scatter_reduce_(0, idx, p, "amin")
    hi = torch.full((T, 3), float("-inf"), device=pts.device).scatter_reduce_(0, idx, p, "amax")
    counts = torch.bincount(t, minlength=T)
    # (the divisor as a device tensor: by a host scalar torch multiplies with the reciprocal, which rounds differently)
    q = torch.floor((p - lo[t]) / torch.tensor(cell, dtype=torch.float32, device=pts.device)).clamp_(0, 16383).long()
    h0, h1 = (1 if up == 0 else 0), (1 if up == 2 else 2)
    plan = torch.unique((t << 28) | (q[:, h1] << 14) | q[:, h0])
    volume = torch.unique((t << 42) | (q[:, up] << 28) | (q[:, h1] << 14) | q[:, h0])
    area = torch.bincount(plan >> 28, minlength=T)
    layer = ((volume >> 28) & 16383).clamp_(max=layers - 1)
    profile = torch.bincount((volume >> 42) * layers + layer, minlength=T * layers).reshape(T, layers)
    return {"box": torch.cat([lo, hi], 1), "counts": counts.reshape(T, 1), "area_cells": area, "profile": profile}


def measure(cloud, skeletons, args, warmup, repeats):
    pts = cloud.xyz
    seg_fn = lambda: S.segment_cloud(cloud, skeletons, tally=False)
    seg = S.segment_cloud(cloud, skeletons)
    flat = FlatSkeletons(skeletons if isinstance(skeletons, list) else [skeletons])
    T = len(flat.tree_rows)
    rows_fn = lambda: I.point_rows(flat, seg.tree_id, cloud.seg_off, pts.device)
    row = rows_fn()
    kw = dict(up=1, cell=args.cell, layers=args.layers)
    tally = lambda: I.tree_tally(pts, row, T, **kw)
    res = tally()
    out = {"points": int(pts.shape[0]), "trees": T, "clouds": cloud.n_seg, "cell": args.cell, "layers": args.layers,
           "points_on_trees": int(res["counts"].sum()), "plan_cells": int(res["area_cells"].sum()), "volume_cells": int(res["profile"].sum()),
           "workspace_MB": I._lib.lib().st_tree_tally_workspace_bytes(int(pts.shape[0]), T, args.layers) / 2 ** 20}
    want = torch_tally(pts, row, T, **kw)
    for k in ("box", "counts", "area_cells", "profile"):
        assert torch.equal(res[k], want[k]), f"the kernel and the torch expression differ in {k}"
    out["equals_torch"] = True
    out["two_runs_identical"] = all(torch.equal(a, b) for a, b in zip(tally().values(), res.values()))
    out["tally_ms"] = timed(tally, warmup, repeats)
    out["tally_chained_ms"] = chained(tally, args.chain, warmup, repeats)
    out["tally_chained_GBps_of_16B_per_point_and_pass"] = 2 * 16.0 * pts.shape[0] / (out["tally_chained_ms"]["median"] * 1e-3) / 1e9
    out["box_and_counts_only_chained_ms"] = chained(lambda: I.tree_tally(pts, row, T, outputs=("box", "counts"), **kw), args.chain, warmup, repeats)
    out["point_rows_chained_ms"] = chained(rows_fn, args.chain, warmup, repeats)
    out["segment_ms"] = timed(seg_fn, warmup, repeats)
    out["segment_and_tally_ms"] = timed(lambda: I.tree_tally(pts, I.point_rows(flat, seg_fn().tree_id, cloud.seg_off, pts.device), T, **kw), warmup, repeats)
    out["measure_trees_ms"] = timed(lambda: I.measure_trees(cloud, skeletons, cell=args.cell, layers=args.layers), 1, max(3, repeats // 2))
    out["measure_trees_given_segmentation_ms"] = timed(lambda: I.measure_trees(cloud, skeletons, segmentation=seg, cell=args.cell, layers=args.layers),
                                                       1, max(3, repeats // 2))
    yardstick = lambda: torch_tally(pts, row, T, **kw)
    out["torch_ms"] = timed(yardstick, warmup, repeats)
    out["torch_chained_ms"] = chained(yardstick, max(args.chain // 4, 1), warmup, repeats)
    out["torch_over_hip_chained"] = out["torch_chained_ms"]["median"] / out["tally_chained_ms"]["median"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=bench.N_POINTS)
    ap.add_argument("--set", type=int, default=bench.REP_SET)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--chain", type=int, default=20)
    ap.add_argument("--cell", type=float, default=0.1)
    ap.add_argument("--layers", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_inventory.py measures on the GPU"
    dev = torch.device("cuda:0")
    c = sample_tree_cloud(args.points, seed=0)
    branch = bench.gt_branch_clouds(dev, [torch.from_numpy(c["xyz"])], [torch.from_numpy(c["medial_vector"])], bench.VOXEL)[0]
    pipe = bench.build_pipeline(dev)
    skeleton = pipe.skeletonizer.forward(branch)
    pipe.post_process(skeleton)
    skeleton = DisjointTreeSkeleton(list(skeleton.skeletons))
    cloud = CentreCloud()(Cloud(xyz=torch.from_numpy(c["xyz"]).to(dev)))
    cloud = Cloud(xyz=cloud.xyz.contiguous())
    res = {"device": torch.cuda.get_device_name(0), "points": args.points, "repeats": args.repeats, "warmup": args.warmup, "chain": args.chain,
           "what": "st_tree_tally through inventory.tree_tally; median, min, max in ms; *_ms: one call ended by a synchronise, "
                   "*_chained_ms: per call of `chain` calls between two device events; torch_*: the same outputs by scatter_reduce, "
                   "bincount and torch.unique over packed keys"}
    res["one_cloud"] = measure(cloud, skeleton, args, args.warmup, args.repeats)
    if args.set > 1:
        B, n = args.set, cloud.xyz.shape[0]
        batch = Cloud(xyz=cloud.xyz.repeat(B, 1), seg_off=torch.arange(B + 1, dtype=torch.int32, device=dev) * n)
        res["launch_set"] = measure(batch, [skeleton] * B, args, 1, max(3, args.repeats // 2))
    print(json.dumps(res))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
