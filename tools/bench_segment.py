"""Time the segmentation of a cloud by its skeleton (smart_tree_amd/segmentation.py, csrc/segment.hip):
python tools/bench_segment.py [--points 1000000] [--set 20] [--large-copies 32] [--repeats 7] [--out profiles/segment_bench.json]

Input: the seed-0 synthetic tree, centred as the pipeline centres it, and the skeleton the pipeline gives for it on ground-truth
medial vectors (bench.gt_branch_clouds, bench.build_pipeline).  Three sizes: the cloud alone, a launch set of `--set` copies (each
against its own copy of the tubes), and one cloud of `--large-copies` copies set side by side (points and tubes shifted together).

Recorded per size: the dense and the grid form with and without the tally, the grid's build (a one-point call: everything but
the query), the shells a point walked (mean, max) and the share of points that ended in the plain sweep; on the one-cloud input
also the parent's st_points_to_nearest_tube -- the yardstick -- and a sweep over the number of tubes at the full point count, from
which the crossover of `auto` is read.  Times are median / min / max in ms after a warm-up, every run ends in a device synchronise."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np
import torch

import bench
from smart_tree_amd import segmentation as S
from smart_tree_amd.data_types.cloud import Cloud
from smart_tree_amd.dataset.augmentations import CentreCloud
from smart_tree_amd.evaluation import skeleton_tubes
from smart_tree_amd.synthetic import sample_tree_cloud
from smart_tree_amd.util.queries import nearest_tube_device


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
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms)}


def measure(pts, tubes, pt_off, tube_off, warmup, repeats, dense=True):
    run = lambda form, tally, p=pts, po=pt_off: S.segment_points(p, *tubes, po, tube_off, None, form, tally)
    out = {"points": int(pts.shape[0]), "tubes": int(tubes[0].shape[0]), "clouds": 1 if pt_off is None else int(pt_off.shape[0]) - 1}
    if dense:
        out["dense_ms"] = timed(lambda: run("dense", True), warmup, repeats)
        out["dense_no_tally_ms"] = timed(lambda: run("dense", False), warmup, repeats)
    out["grid_ms"] = timed(lambda: run("grid", True), warmup, repeats)
    out["grid_no_tally_ms"] = timed(lambda: run("grid", False), warmup, repeats)
    one = pts[:1].contiguous() if pt_off is None else pts.index_select(0, pt_off[:-1].long())  # a point per cloud: the build alone
    one_off = None if pt_off is None else torch.arange(pt_off.shape[0], dtype=torch.int32, device=pts.device)
    out["grid_build_ms"] = timed(lambda: run("grid", False, one, one_off), warmup, repeats)
    res = run("grid", True)
    walked, shells, longest, swept = res["ws"][:32].view(torch.int64).tolist()
    out.update({"shells_mean": shells / max(walked, 1), "shells_max": longest, "swept_share": swept / max(int(pts.shape[0]), 1),
                "assigned": int((res["tube"] >= 0).sum()), "mean_abs_residual_m": float(res["residual"].abs().mean())})
    if dense:
        ref = run("dense", True)
        out["forms_identical"] = bool(all(torch.equal(res[k].view(torch.int32) if res[k].dtype == torch.float32 else res[k],
                                                      ref[k].view(torch.int32) if ref[k].dtype == torch.float32 else ref[k])
                                          for k in ("tube", "residual", "vec", "rad", "tally")))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=bench.N_POINTS)
    ap.add_argument("--set", type=int, default=bench.REP_SET)
    ap.add_argument("--large-copies", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_segment.py measures on the GPU"
    dev = torch.device("cuda:0")
    c = sample_tree_cloud(args.points, seed=0)
    branch = bench.gt_branch_clouds(dev, [torch.from_numpy(c["xyz"])], [torch.from_numpy(c["medial_vector"])], bench.VOXEL)[0]
    pipe = bench.build_pipeline(dev)
    skeleton = pipe.skeletonizer.forward(branch)
    pipe.post_process(skeleton)
    tubes = tuple(t.to(dev).contiguous() for t in skeleton_tubes(skeleton))
    pts = CentreCloud()(Cloud(xyz=torch.from_numpy(c["xyz"]).to(dev))).xyz.contiguous()
    m = int(tubes[0].shape[0])
    res = {"device": torch.cuda.get_device_name(0), "points": args.points, "tubes": m, "repeats": args.repeats, "warmup": args.warmup,
           "what": "st_segment_points_seg through segmentation.segment_points; median, min, max in ms, each run ended by a synchronise"}
    res["one_cloud"] = measure(pts, tubes, None, None, args.warmup, args.repeats)
    res["one_cloud"]["parent_nearest_tube_ms"] = timed(lambda: nearest_tube_device(pts, *tubes), args.warmup, args.repeats)
    res["one_cloud"]["auto_ms"] = timed(lambda: S.segment_points(pts, *tubes, form="auto"), args.warmup, args.repeats)
    sweep = []
    for k in sorted({min(x, m) for x in (64, 128, 256, 512, 1024, 2048, 4096, m)}):
        sub = tuple(t[:k].contiguous() for t in tubes)
        sweep.append({"tubes": k, "dense_ms": timed(lambda: S.segment_points(pts, *sub, form="dense"), 1, max(3, args.repeats // 2)),
                      "dense_no_tally_ms": timed(lambda: S.segment_points(pts, *sub, form="dense", tally=False), 1, max(3, args.repeats // 2)),
                      "grid_ms": timed(lambda: S.segment_points(pts, *sub, form="grid"), 1, max(3, args.repeats // 2))})
    step = float(pts[:, 0].max() - pts[:, 0].min()) + 1.0
    for K in (2, 4, 8):  # more tubes than the tree has: copies of it set aside, the points stay
        sub = (torch.cat([tubes[0] + torch.tensor([k * step, 0.0, 0.0], device=dev) for k in range(K)]),
               torch.cat([tubes[1] + torch.tensor([k * step, 0.0, 0.0], device=dev) for k in range(K)]), tubes[2].repeat(K), tubes[3].repeat(K))
        sweep.append({"tubes": K * m, "dense_ms": timed(lambda: S.segment_points(pts, *sub, form="dense"), 1, 3),
                      "grid_ms": timed(lambda: S.segment_points(pts, *sub, form="grid"), 1, 3)})
    res["tube_sweep"] = sweep
    if args.set > 1:
        B = args.set
        off = lambda k: torch.arange(B + 1, dtype=torch.int32, device=dev) * k
        res["launch_set"] = measure(pts.repeat(B, 1), tuple(t.repeat(*([B] + [1] * (t.dim() - 1))) for t in tubes), off(pts.shape[0]),
                                    off(m), 1, max(3, args.repeats // 2))
    if args.large_copies > 1:
        K = args.large_copies
        shift = torch.zeros((K, 1, 3), device=dev)
        shift[:, 0, 0] = torch.arange(K, device=dev, dtype=torch.float32) * step
        big = (pts.unsqueeze(0) + shift).reshape(-1, 3).contiguous()
        big_tubes = ((tubes[0].unsqueeze(0) + shift).reshape(-1, 3).contiguous(), (tubes[1].unsqueeze(0) + shift).reshape(-1, 3).contiguous(),
                     tubes[2].repeat(K), tubes[3].repeat(K))
        res["large_cloud"] = {"copies": K, **measure(big, big_tubes, None, None, 1, 3)}
    print(json.dumps(res))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
