"""Time of `st_scan_cast_seg` (csrc/scan.hip) on the GPU: the dense and the grid form, the tube count at which they cost the same
(what SC_AUTO_GRID_M should be), the grid's build against its cast, and `st_synth_points_seg`'s time per point for context.
Prints one JSON line and writes it to profiles/scan_bench.json (`--out`).

Device events around the call alone (resident tubes, fresh outputs), warm-up 2, median of 7, as tools/bench_synth.py.
* scenes          one depth-7 tree under 1, 3 and 8 scanners of about `--beams` beams each on a ring, and a batch of 64 trees with one
                  scanner of `--batch-beams` beams each: rays/s and hits/s of both forms
* auto_sweep      trees of depth 1 .. --max-depth (3 to 736 tubes at depth 7) under one scanner: dense_ms and grid_ms per tube count,
                  and the first count at which the grid wins
* call_overhead_ms  a dense call with a single beam on a 3-tube tree: the host's table, the output allocations, the put, scan and finish launches
                  and the read-back that every call pays whatever its form
* grid_build_ms   a grid call with a single beam minus call_overhead_ms: plan, pack, count, scan and fill; grid_cast_ms: the
                  one-scanner grid call minus the single-beam grid call.  grid_plan: the cell and the shape of that grid
* synth           st_synth_points_seg for the same number of points as one scanner has beams: ns per point
No GPU: the tool fails, it does not fall back.
"""
from __future__ import annotations

import argparse
import json
import math
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from smart_tree_amd import scan as SC  # noqa: E402
from smart_tree_amd.data_types.flat import FlatSkeletons  # noqa: E402
from smart_tree_amd.dataset import synthetic as S  # noqa: E402
from smart_tree_amd.synthetic import grow_tree  # noqa: E402


UP = 1  # the trees grow along y


def framed(scanners):
    return [SC.Scanner(tuple(SC.to_frame(np.asarray(s.position), s.up)), s.az, s.el, s.min_range, s.max_range, s.range_noise, s.seed)
            for s in scanners]


def ring(skeleton, n, beams, seed=0):
    """n scanners on the default ring whose windows hold about `beams` beams each."""
    box = SC.skeleton_box(skeleton)
    probe = SC.scanner_ring(n, 6.0, 1.5, box, 0.5, up=UP)
    step = 0.5 * math.sqrt(statistics.mean(s.n_rays for s in probe) / beams)
    return framed(SC.scanner_ring(n, 6.0, 1.5, box, step, up=UP, seed=seed))


def tubes_of(skeletons, dev):
    flat = FlatSkeletons(skeletons, "bench_scan")
    a, b, r1, r2 = flat.tubes(*flat.float32())
    a, b = SC.to_frame(a, UP), SC.to_frame(b, UP)  # scan_cast works in the scanners' frame
    a, b, r1, r2 = (torch.from_numpy(np.ascontiguousarray(t)).to(dev) for t in (a, b, r1, r2))
    off = torch.from_numpy(flat.tube_off.astype(np.int32)).to(dev) if len(skeletons) > 1 else None
    return a, b, r1, r2, off


def time_ms(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times)


def cast_ms(dev, skeletons, scanners, form, warmup, iters):
    """(median ms of scan_cast -- its launches and its one read-back of n_hits --, beams, hits, tubes, the last call's result)."""
    a, b, r1, r2, off = tubes_of(skeletons, dev)
    res = {}

    def call():
        res.update(SC.scan_cast(a, b, r1, r2, off, None, None, scanners, form, outputs=("xyz", "medial_vector", "class_l", "branch_ids", "segment")))

    ms = time_ms(call, warmup, iters)
    return ms, int(res["ray_off"][-1]), int(res["n_hits"]), int(a.shape[0]), res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--beams", type=int, default=1_000_000)
    ap.add_argument("--batch-beams", type=int, default=65_536)
    ap.add_argument("--max-depth", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--out", default=str(Path(__file__).resolve().parents[1] / "profiles" / "scan_bench.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_scan: needs the GPU (no CPU fallback; a CPU timing would say nothing)")
    dev = torch.device("cuda:0")
    result = {"beams_per_scanner": a.beams, "max_depth": a.max_depth, "warmup": a.warmup, "iters": a.iters,
              "device": torch.cuda.get_device_name(0), "scenes": {}, "auto_sweep": [], "timed": "scan_cast: launches and the read-back of n_hits"}
    tree = S.tree_skeleton(grow_tree(0, 1.0, a.max_depth))
    scenes = {f"1_tree_{n}_scanners": ([tree], [ring(tree, n, a.beams)]) for n in (1, 3, 8)}
    batch = [S.tree_skeleton(grow_tree(s, 1.0, a.max_depth), s) for s in range(64)]
    scenes["64_trees_1_scanner_each"] = (batch, [ring(sk, 1, a.batch_beams, seed=s) for s, sk in enumerate(batch)])
    for name, (skeletons, scanners) in scenes.items():
        row = {}
        for form in ("dense", "grid"):
            ms, beams, hits, m, _ = cast_ms(dev, skeletons, scanners, form, a.warmup, a.iters)
            row.update({"tubes": m, "beams": beams, "hits": hits, f"{form}_ms": round(ms, 3), f"{form}_rays_per_s": round(beams / (ms * 1e-3)),
                        f"{form}_hits_per_s": round(hits / (ms * 1e-3))})
        result["scenes"][name] = row
    crossover = None
    for depth in range(1, a.max_depth + 1):
        sk = S.tree_skeleton(grow_tree(0, 1.0, depth))
        sc = [ring(sk, 1, a.beams)]
        d_ms, beams, hits, m, _ = cast_ms(dev, [sk], sc, "dense", a.warmup, a.iters)
        g_ms = cast_ms(dev, [sk], sc, "grid", a.warmup, a.iters)[0]
        result["auto_sweep"].append({"depth": depth, "tubes": m, "beams": beams, "hits": hits, "dense_ms": round(d_ms, 3), "grid_ms": round(g_ms, 3)})
        if crossover is None and g_ms < d_ms:
            crossover = m
    result["grid_wins_from_tubes"] = crossover
    one = [[SC.Scanner(scenes["1_tree_1_scanners"][1][0][0].position, (0.0, 0.01, 1), (0.0, 0.01, 1))]]
    # single-beam calls are all host overhead and a few tiny launches: many more repeats than the big calls need
    # (on a 3-tube tree: a single lane sweeping the big table alone would take 0.75 ms, which no full call pays)
    overhead = cast_ms(dev, [S.tree_skeleton(grow_tree(0, 1.0, 1))], one, "dense", 10, 51)[0]
    build, _, _, _, res = cast_ms(dev, [tree], one, "grid", 10, 51)
    full = result["scenes"]["1_tree_1_scanners"]["grid_ms"]
    plan = SC.grid_plan(res["ws"])
    result["call_overhead_ms"], result["one_beam_grid_ms"] = round(overhead, 3), round(build, 3)
    result["grid_build_ms"], result["grid_cast_ms"] = round(build - overhead, 3), round(full - build, 3)
    result["grid_plan"] = {"cell": round(plan["cell"], 4), "dim": [int(x) for x in plan["dim"]], "sweep": plan["sweep"]}
    table = S.segment_table(grow_tree(0, 1.0, a.max_depth))
    outs = None

    def synth():
        nonlocal outs
        outs, _, _ = S.synth_points([table], [a.beams], [0], [0], [0.002], [0.08], dev, outputs=outs)

    s_ms = time_ms(synth, a.warmup, a.iters)
    result["synth"] = {"points": a.beams, "ms": round(s_ms, 4), "ns_per_point": round(s_ms * 1e6 / a.beams, 4)}
    line = json.dumps(result)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")
    return result


if __name__ == "__main__":
    main()
