"""Time `evaluate_skeleton` on a representative tree and compare its matching with the same matching written as a chunked
dense torch expression on the same device (the reference's style, smart_tree/util/queries.py:89-133, with the nearest-axis
criterion): python tools/bench_eval.py [--samples 200000] [--tubes 20000] [--repeats 9] [--out FILE.json]

Ground truth: `synthetic.grow_tree` segments, subdivided.  Prediction: the same segments subdivided differently and jittered by
a tenth of their radius.  Both matchings must agree to 1e-5 on every distance (asserted); times are medians after a warm-up."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np
import torch

from smart_tree_amd.data_types.tube import sample_tubes_device
from smart_tree_amd.evaluation import DEFAULT_THRESHOLDS, evaluate_skeleton, match
from smart_tree_amd.synthetic import grow_tree


def subdivide(seg, pieces, jitter, rng):
    """Every segment as `pieces` tubes; interior and end vertices moved by N(0, jitter * radius)."""
    f = np.linspace(0.0, 1.0, pieces + 1)[None, :, None]
    xyz = seg.a[:, None, :] + f * (seg.b - seg.a)[:, None, :]
    rad = seg.ra[:, None] + f[..., 0] * (seg.rb - seg.ra)[:, None]
    xyz = xyz + rng.normal(0.0, 1.0, xyz.shape) * (jitter * rad)[..., None]
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x.astype(np.float32)))
    return (t(xyz[:, :-1].reshape(-1, 3)), t(xyz[:, 1:].reshape(-1, 3)), t(rad[:, :-1].reshape(-1)), t(rad[:, 1:].reshape(-1)))


def dense_match(pts, a, b, r1, r2, chunk=4096):
    """Nearest axis per sample as a dense [chunk, M] torch expression: (dist, tube radius at the projection)."""
    ab = b - a
    ab2 = torch.einsum("md,md->m", ab, ab)
    dist, rad = [], []
    for s in range(0, pts.shape[0], chunk):
        p = pts[s:s + chunk]
        ap = p[:, None, :] - a[None]
        t = (torch.einsum("nmd,md->nm", ap, ab) / ab2).clip(0.0, 1.0)
        d2 = (a[None] + t[..., None] * ab[None] - p[:, None, :]).square().sum(2)
        best = d2.argmin(1, keepdim=True)
        tb = t.gather(1, best)[:, 0]
        dist.append(d2.gather(1, best)[:, 0].sqrt())
        rad.append((1 - tb) * r1[best[:, 0]] + tb * r2[best[:, 0]])
    return torch.cat(dist), torch.cat(rad)


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
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=200_000)
    ap.add_argument("--tubes", type=int, default=20_000)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_eval.py measures on the GPU"
    dev = torch.device("cuda:0")
    seg = grow_tree(seed=0, max_depth=7)
    pieces = max(1, round(args.tubes / len(seg.a)))
    rng = np.random.RandomState(0)
    gt = subdivide(seg, pieces, 0.0, rng)
    pred = subdivide(seg, pieces + 1, 0.1, rng)
    length = float(np.linalg.norm(seg.b - seg.a, axis=1).sum())
    spacing = length / args.samples
    g, p = [t.to(dev) for t in gt], [t.to(dev) for t in pred]
    g_pts, g_rad = sample_tubes_device(*g, spacing)[:2]
    p_pts, p_rad = sample_tubes_device(*p, spacing)[:2]
    thr = list(DEFAULT_THRESHOLDS)

    # agreement of the two matchings, both directions
    worst = 0.0
    for (pts, rad, tubes, mode) in ((g_pts, g_rad, p, 0), (p_pts, p_rad, g, 1)):
        got = match(pts, rad, *tubes, thr, mode)
        d_ref, r_ref = dense_match(pts, *tubes)
        err = float((got["dist"] - d_ref).abs().max())
        worst = max(worst, err)
        assert err <= 1e-5, f"distances differ from the dense expression by {err}"
        ref = r_ref if mode else rad
        hits_ref = (d_ref[None, :] <= torch.tensor(thr, device=dev)[:, None] * ref[None, :]).sum(1)
        print(f"ref_mode {mode}: max |dist - dense| = {err:.3g}; hits {got['hits'].tolist()} dense {hits_ref.tolist()}")

    def kernel_both():
        match(g_pts, g_rad, *p, thr, 0, per_sample=False)
        match(p_pts, p_rad, *g, thr, 1, per_sample=False)

    def dense_both():
        dense_match(g_pts, *p)
        dense_match(p_pts, *g)

    k_ms = timed(kernel_both, args.warmup, args.repeats)
    d_ms = timed(dense_both, args.warmup, args.repeats)
    e_ms = timed(lambda: evaluate_skeleton(pred, gt, spacing=spacing, device=dev), args.warmup, args.repeats)
    s_ms = timed(lambda: (sample_tubes_device(*g, spacing), sample_tubes_device(*p, spacing)), args.warmup, args.repeats)
    pairs = g_pts.shape[0] * p[0].shape[0] + p_pts.shape[0] * g[0].shape[0]
    metrics = evaluate_skeleton(pred, gt, spacing=spacing, device=dev)
    res = {"device": torch.cuda.get_device_name(0), "gt_tubes": g[0].shape[0], "pred_tubes": p[0].shape[0], "gt_samples": g_pts.shape[0],
           "pred_samples": p_pts.shape[0], "spacing": spacing, "pairs_both_directions": pairs, "repeats": args.repeats,
           "match_kernel_ms": {"median": k_ms[0], "min": k_ms[1], "max": k_ms[2]},
           "match_dense_torch_ms": {"median": d_ms[0], "min": d_ms[1], "max": d_ms[2]},
           "sampling_both_ms": {"median": s_ms[0], "min": s_ms[1], "max": s_ms[2]},
           "evaluate_skeleton_ms": {"median": e_ms[0], "min": e_ms[1], "max": e_ms[2]},
           "kernel_pairs_per_s": pairs / (k_ms[0] * 1e-3), "dense_pairs_per_s": pairs / (d_ms[0] * 1e-3),
           "speedup_of_matching": d_ms[0] / k_ms[0], "max_abs_distance_difference": worst,
           "auc": metrics["auc"], "f1": metrics["f1"]}
    print(json.dumps(res))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
