"""Time the bridging of components (Skeletonizer(connect_components=True), csrc/bridge.hip) on the ground-truth inputs of
`bench.py --full`: python tools/bench_bridge.py [--points 1000000] [--set 20] [--max-gap 0.3] [--repeats 7] [--out profiles/bridge_bench.json]

Input: the seed-0 synthetic tree, centred and voxelised at 2 cm as ModelInference does, its inner voxel representatives paired
with the generator's exact medial vectors (bench.gt_branch_clouds) -- with slabs cut out across its branches, so the medial
points fall into fragments.  Once as one cloud, once as a launch set of `--set` copies of it.

Recorded: `Skeletonizer.forward` (+ post_process, results on the host) with the feature off and on, the bridging call alone
(bridge_components on the components of the cut graph), its Boruvka rounds, the boundary set of round 1 and the trees before
and after.  Times are medians after a warm-up, every run ends in a device synchronise."""
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
from smart_tree_amd.data_types.cloud import Cloud
from smart_tree_amd.skeleton import graph as G
from smart_tree_amd.skeleton.filter import outlier_removal
from smart_tree_amd.synthetic import sample_tree_cloud


def cut_slabs(xyz, mv, slabs):
    """Drop the points whose axis point (xyz + medial vector) lies in one of the height intervals."""
    y = (xyz + mv)[:, 1]
    keep = np.ones(len(y), bool)
    for lo, hi in slabs:
        keep &= ~((y >= lo) & (y <= hi))
    return xyz[keep], mv[keep]


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


def measure(pipe_off, pipe_on, cloud, max_gap, warmup, repeats):
    def run(pipe):
        s = pipe.skeletonizer.forward(cloud)
        pipe.post_process(s)
        parts = s.split()  # materialise: device post-processing, one device-to-host copy
        return parts

    # the bridging call alone, on the components Skeletonizer.forward hands it
    sk = pipe_on.skeletonizer
    medial, radius = G.medial_points(cloud.xyz, cloud.medial_vector)
    keep = outlier_removal(medial, radius.unsqueeze(1), nb_points=8, seg_off=cloud.seg_off).nonzero().view(-1)
    seg_off = cloud.filter(keep, assume_sorted=True).seg_off
    medial, radius = medial.index_select(0, keep), radius.index_select(0, keep)
    graph = G.nn_graph(medial, radius.clamp(min=sk.min_connection_length), K=sk.K, seg_off=seg_off)
    comps = graph.connected_cugraph_components(minimum_vertices=sk.minimum_graph_vertices)
    out = {"graph_vertices": int(medial.shape[0]), "kept_vertices": int(comps.vert_order.shape[0]), "components": int(comps.n_components)}
    out["bridge_components_ms"] = timed(lambda: G.bridge_components(comps, medial, max_gap), warmup, repeats)
    out.update({k: G.last_bridge_stats[k] for k in ("rounds", "boundary", "bridges")})
    # off and on alternate: both see the same machine state
    off, on = [], []
    for i in range(warmup + repeats):
        for pipe, ms in ((pipe_off, off), (pipe_on, on)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            parts = run(pipe)
            torch.cuda.synchronize()
            if i >= warmup:
                ms.append((time.perf_counter() - t0) * 1e3)
            if i == 0:
                out["trees_on" if pipe is pipe_on else "trees_off"] = int(sum(len(p.skeletons) for p in parts))
                out["branches_on" if pipe is pipe_on else "branches_off"] = int(sum(len(t.branches) for p in parts for t in p.skeletons))
    for name, ms in (("forward_off_ms", off), ("forward_on_ms", on)):
        out[name] = {"median": statistics.median(ms), "min": min(ms), "max": max(ms)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=bench.N_POINTS)
    ap.add_argument("--set", type=int, default=bench.REP_SET)
    ap.add_argument("--max-gap", type=float, default=0.3)
    ap.add_argument("--slab", type=float, default=0.2, help="width of the slabs cut out (metres)")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_bridge.py measures on the GPU"
    dev = torch.device("cuda:0")
    c = sample_tree_cloud(args.points, seed=0)
    top = float((c["xyz"] + c["medial_vector"])[:, 1].max())
    slabs = [(f * top, f * top + args.slab) for f in (0.15, 0.40, 0.55, 0.70, 0.85)]  # the trunk once, the crown four times
    xyz, mv = cut_slabs(c["xyz"], c["medial_vector"], slabs)
    one = bench.gt_branch_clouds(dev, [torch.from_numpy(xyz)], [torch.from_numpy(mv)], bench.VOXEL)[0]
    pipe_off = bench.build_pipeline(dev)
    pipe_on = bench.build_pipeline(dev)
    pipe_on.skeletonizer.connect_components, pipe_on.skeletonizer.max_gap = True, float(args.max_gap)
    res = {"device": torch.cuda.get_device_name(0), "points": args.points, "voxel": bench.VOXEL, "max_gap": args.max_gap,
           "slabs": [[round(a, 3), round(b, 3)] for a, b in slabs], "repeats": args.repeats, "warmup": args.warmup,
           "what": "Skeletonizer.forward + post_process, results on the host; off / on alternate; median, min, max in ms"}
    res["one_cloud"] = measure(pipe_off, pipe_on, one, args.max_gap, args.warmup, args.repeats)
    if args.set > 1:
        batch = Cloud.collate([one] * args.set)
        res["launch_set"] = {"clouds": args.set, **measure(pipe_off, pipe_on, batch, args.max_gap, args.warmup, max(3, args.repeats // 2))}
    print(json.dumps(res))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
