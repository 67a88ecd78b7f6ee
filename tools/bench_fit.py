"""Time the tube fit of a skeleton to its points (smart_tree_amd/refine.py, csrc/fit.hip):
python tools/bench_fit.py [--points 1000000] [--set 20] [--repeats 9] [--out profiles/fit_bench.json]

Input: that of tools/bench_segment.py -- the seed-0 synthetic tree, centred as the pipeline centres it, and the skeleton the pipeline
gives for it on ground-truth medial vectors -- alone and as a launch set of `--set` copies, each against its own copy of the tubes.

Recorded per size: the fit pass alone (st_fit_tubes through refine.fit_tubes: one call ended by a synchronise, and the time per
call of `--chain` calls enqueued back to back between two device events, which leaves the launch latency out), with the points in
the cloud's order and sorted by tube (a scan's spatial order against the generator's random one: how often the LDS table helps);
the pass beside the segmentation call it follows; a whole `refine_skeleton` of two iterations; and the yardstick, the same ten sums
as float64 `index_add_` calls in torch.  Times are median / min / max in ms after a warm-up."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch

import bench
from smart_tree_amd import refine as R
from smart_tree_amd import segmentation as S
from smart_tree_amd.data_types.cloud import Cloud
from smart_tree_amd.data_types.tree import DisjointTreeSkeleton
from smart_tree_amd.dataset.augmentations import CentreCloud
from smart_tree_amd.evaluation import skeleton_tubes
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


def torch_terms(pts, tube, a, b, r1, r2, max_relative=0.5):
    """(tube of every entering point, the nine float64 terms [9,k]) by the contract's rules in plain torch -- the yardstick's input."""
    ok = tube >= 0
    t = tube.clamp(min=0).long()
    ab = b[t] - a[t]
    q = ((pts - a[t]) * ab).sum(1) / (ab * ab).sum(1)
    r = (1 - q) * r1[t] + q * r2[t]
    v = a[t] + q[:, None] * ab - pts
    rho = v.norm(dim=1)
    ok = ok & (q >= 0) & (q <= 1) & (rho > 0) & ((rho - r).abs() <= max_relative * r)
    k = ab.abs().argmin(1)
    unit = torch.nn.functional.one_hot(k, 3).to(ab.dtype)
    e1 = torch.nn.functional.normalize(torch.cross(ab, unit, dim=1), dim=1)
    e2 = torch.nn.functional.normalize(torch.cross(ab, e1, dim=1), dim=1)
    w = -v / rho[:, None]
    c, s = (w * e1).sum(1).double(), (w * e2).sum(1).double()
    rho = rho.double()
    terms = torch.stack([c * c, c * s, s * s, c, s, rho * c, rho * s, rho, rho * rho])
    return t[ok], terms[:, ok].contiguous()


def measure(pts, tubes, pt_off, tube_off, skeletons, cloud, args, warmup, repeats):
    m = int(tubes[0].shape[0])
    seg = lambda: S.segment_points(pts, *tubes, pt_off, tube_off, None, "auto", tally=False, outputs=("tube",))
    tube = seg()["tube"]
    out = {"points": int(pts.shape[0]), "tubes": m, "clouds": 1 if pt_off is None else int(pt_off.shape[0]) - 1}
    fit = lambda p=pts, t=tube: R.fit_tubes(p, t, *tubes)
    res = R.fit_tubes(pts, tube, *tubes, moments=True)
    out["points_used"] = int(res["moments"][:, 0].sum())
    out["status_share"] = [float((res["fit"][:, 7] == k).double().mean()) for k in (0, 1, 2)]
    out["fit_ms"] = timed(fit, warmup, repeats)
    out["fit_chained_ms"] = chained(fit, args.chain, warmup, repeats)
    out["fit_chained_GBps_of_16B_per_point"] = 16.0 * pts.shape[0] / (out["fit_chained_ms"]["median"] * 1e-3) / 1e9
    order = torch.sort(tube.long(), stable=True).indices  # the same points, neighbours on the same tube
    p_sorted, t_sorted = pts.index_select(0, order).contiguous(), tube.index_select(0, order).contiguous()
    out["fit_sorted_by_tube_chained_ms"] = chained(lambda: fit(p_sorted, t_sorted), args.chain, warmup, repeats)
    out["sorted_moments_identical"] = bool(torch.equal(R.fit_tubes(p_sorted, t_sorted, *tubes, moments=True)["moments"], res["moments"]))
    out["segment_ms"] = timed(seg, warmup, repeats)
    out["segment_and_fit_ms"] = timed(lambda: fit(pts, seg()["tube"]), warmup, repeats)
    out["refine_two_iterations_ms"] = timed(lambda: R.refine_skeleton(cloud, skeletons, iterations=2), 1, max(3, repeats // 2))
    # the yardstick: ten float64 index_add_ calls (float atomics: other bits in every run)
    idx, terms = torch_terms(pts, tube, *tubes)
    ones = torch.ones(idx.shape[0], dtype=torch.float64, device=pts.device)

    def yardstick():
        sums = torch.zeros((10, m), dtype=torch.float64, device=pts.device)
        sums[0].index_add_(0, idx, ones)
        for k in range(9):
            sums[k + 1].index_add_(0, idx, terms[k])
        return sums

    out["torch_index_add_ms"] = timed(yardstick, warmup, repeats)
    out["torch_index_add_chained_ms"] = chained(yardstick, max(args.chain // 4, 1), warmup, repeats)
    sums = yardstick()
    mom = res["moments"].double()
    out["torch_points"] = int(sums[0].sum())
    out["torch_sum_rho_rel_diff"] = float((sums[8].sum() - mom[:, 8].sum() / 2.0 ** 24).abs() / sums[8].sum().clamp(min=1e-30))
    out["torch_two_runs_identical"] = bool(torch.equal(yardstick(), sums))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=bench.N_POINTS)
    ap.add_argument("--set", type=int, default=bench.REP_SET)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--chain", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_fit.py measures on the GPU"
    dev = torch.device("cuda:0")
    c = sample_tree_cloud(args.points, seed=0)
    branch = bench.gt_branch_clouds(dev, [torch.from_numpy(c["xyz"])], [torch.from_numpy(c["medial_vector"])], bench.VOXEL)[0]
    pipe = bench.build_pipeline(dev)
    skeleton = pipe.skeletonizer.forward(branch)
    pipe.post_process(skeleton)
    skeleton = DisjointTreeSkeleton(list(skeleton.skeletons))
    tubes = tuple(t.to(dev).contiguous() for t in skeleton_tubes(skeleton))
    cloud = CentreCloud()(Cloud(xyz=torch.from_numpy(c["xyz"]).to(dev)))
    pts = cloud.xyz.contiguous()
    m = int(tubes[0].shape[0])
    res = {"device": torch.cuda.get_device_name(0), "points": args.points, "tubes": m, "repeats": args.repeats, "warmup": args.warmup,
           "chain": args.chain, "what": "st_fit_tubes through refine.fit_tubes; median, min, max in ms; *_ms: one call ended by a synchronise, "
                                        "*_chained_ms: per call of `chain` calls between two device events"}
    res["one_cloud"] = measure(pts, tubes, None, None, skeleton, Cloud(xyz=pts), args, args.warmup, args.repeats)
    if args.set > 1:
        B = args.set
        off = lambda k: torch.arange(B + 1, dtype=torch.int32, device=dev) * k
        batch = Cloud(xyz=pts.repeat(B, 1), seg_off=off(pts.shape[0]))
        res["launch_set"] = measure(batch.xyz, tuple(t.repeat(*([B] + [1] * (t.dim() - 1))) for t in tubes), off(pts.shape[0]), off(m),
                                    [skeleton] * B, batch, args, 1, max(3, args.repeats // 2))
    print(json.dumps(res))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
