"""Time `st_prediction_metrics` against `st_loss_forward` (the yardstick: it reads the same rows) and against the same metrics
written as torch expressions on the device: python tools/bench_metrics.py [--rows 1000000 10000000] [--repeats 9] [--out FILE.json]

One process, C = 2, one segment, the run's loss selection (mask, vector_class = 0, log radius).  Every timing is a pair of device
events around one call after a warm-up of 2; reported as the median of the repeats with min and max.  The two C entry points are
called on preallocated buffers, so the interval holds the kernels (for the loss also its 64-byte read-back, which is part of that
call).  Bytes per row = (10 + C) * 4 + 1; the share is of the 6.3 TB/s a float4 copy reaches on an MI355X (HBM3E peak 8 TB/s)."""
import argparse
import ctypes
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np
import torch

from smart_tree_amd import _lib
from smart_tree_amd.evaluation.prediction import DEFAULT_RADIUS_EDGES, DEFAULT_THRESHOLDS, prediction_tally

ACHIEVABLE_HBM = 6.3e12  # bytes / s
C = 2


def make_rows(n, dev, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    r_gt = torch.exp(torch.empty(n).uniform_(float(np.log(0.003)), float(np.log(0.2)), generator=g))
    q = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=1)
    cls = (torch.rand(n, generator=g) < 0.3).float()
    targets = torch.cat([r_gt[:, None], q, cls[:, None]], 1)
    preds = {"radius": (r_gt.log() + 0.3 * torch.randn(n, generator=g))[:, None], "direction": q + 0.3 * torch.randn(n, 3, generator=g),
             "class_l": torch.randn(n, C, generator=g) + 2.0 * torch.stack([1 - cls, cls], 1)}
    mask = torch.rand(n, generator=g) < 0.9
    return {k: v.to(dev).contiguous() for k, v in preds.items()}, targets.to(dev).contiguous(), mask.to(dev)


def torch_metrics(preds, targets, mask, vector_class=0, thresholds=DEFAULT_THRESHOLDS, radius_edges=DEFAULT_RADIUS_EDGES):
    """The kernel's figures as torch expressions (no guard for non-finite rows: the benchmark's rows have none)."""
    dev = targets.device
    tc = targets[mask, 4].long()
    pc = preds["class_l"][mask].argmax(1)
    conf = torch.bincount(tc * C + pc, minlength=C * C)
    vec = mask & (targets[:, 4].long() == vector_class)
    r_gt, r_pred = targets[vec, 0], preds["radius"][vec, 0].exp()
    p, q = preds["direction"][vec], targets[vec, 1:4]
    u, h = p / p.norm(dim=1, keepdim=True).clamp_min(1e-8), q / q.norm(dim=1, keepdim=True).clamp_min(1e-8)
    dr = (r_pred - r_gt).abs()
    ang = (u * h).sum(1).clamp(-1.0, 1.0).acos()
    err = (r_pred[:, None] * u - r_gt[:, None] * h).norm(dim=1)
    sums = torch.stack([x.double().sum() for x in (dr, dr / r_gt, ang, err, err / r_gt)])
    within = (err[None, :] <= torch.tensor(thresholds, device=dev)[:, None] * r_gt[None, :]).sum(1)
    which = torch.bucketize(r_gt, torch.tensor(radius_edges, device=dev), right=True)
    nb = len(radius_edges) + 1
    bins = torch.bincount(which, minlength=nb)
    z = torch.zeros(nb, dtype=torch.float64, device=dev)
    return conf, sums, within, bins, z.index_add(0, which, (dr / r_gt).double()), z.index_add(0, which, (err / r_gt).double()), vec.sum()


def check_agreement(preds, targets, mask, T=len(DEFAULT_THRESHOLDS)):
    """The torch expressions agree with the kernel: counts exactly (the threshold counts up to an ulp of `err`), sums to float32
    rounding.  Returns the largest relative difference of a sum."""
    n = targets.shape[0]
    tally = prediction_tally(preds, targets, mask, vector_class=0)
    conf, t_sums, within, bins, b_dr, b_err, n_vec = torch_metrics(preds, targets, mask)
    ki, ks = tally.ints[0], tally.sums[0]
    assert torch.equal(ki[:C * C], conf) and int(ki[C * C + 1]) == int(n_vec) and int(ki[C * C + 2]) == 0
    assert torch.equal(ki[C * C + 4 + T:], bins), (ki[C * C + 4 + T:], bins)
    assert int((ki[C * C + 4:C * C + 4 + T] - within).abs().max()) <= max(2, n // 100_000), (ki[C * C + 4:C * C + 4 + T], within)
    rel = float(((ks - torch.cat([t_sums, b_dr, b_err])).abs() / ks.abs().clamp_min(1e-30)).max())
    assert rel < 1e-4, rel
    return rel


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        ms.append(t0.elapsed_time(t1))
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms)}


def bench(n, dev, warmup, repeats):
    L = _lib.lib()
    preds, targets, mask = make_rows(n, dev)
    m8 = mask.view(torch.uint8)
    thr, edges = np.asarray(DEFAULT_THRESHOLDS, np.float32), np.asarray(DEFAULT_RADIUS_EDGES, np.float32)
    T, NB = len(thr), len(edges) + 1
    ints = torch.empty(L.st_prediction_metrics_tally_ints(C, T, NB), dtype=torch.int64, device=dev)
    sums = torch.empty(L.st_prediction_metrics_tally_sums(NB), dtype=torch.float64, device=dev)
    ws = torch.empty(L.st_prediction_metrics_workspace_bytes(n, 1, NB), dtype=torch.uint8, device=dev)
    lws = torch.empty(L.st_loss_workspace_bytes(), dtype=torch.uint8, device=dev)
    out = (ctypes.c_double * 8)()
    host = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    p = _lib.ptr
    stream = _lib.stream(dev)

    def metrics():
        _lib.check(L.st_prediction_metrics(p(preds["radius"]), p(preds["direction"]), p(preds["class_l"]), C, p(targets), 5, p(m8), n,
                                           None, 1, 0, 1, host(thr), T, host(edges), len(edges), p(ints), p(sums), p(ws), ws.numel(),
                                           stream))

    def loss():
        _lib.check(L.st_loss_forward(p(preds["radius"]), p(preds["direction"]), p(preds["class_l"]), C, p(targets), 5, p(m8), n, 0, 1,
                                     out, p(lws), lws.numel(), stream))

    rel = check_agreement(preds, targets, mask, T)

    res = {"rows": n, "metrics_ms": timed(metrics, warmup, repeats), "loss_ms": timed(loss, warmup, repeats),
           "torch_expressions_ms": timed(lambda: torch_metrics(preds, targets, mask), warmup, repeats)}
    res["bytes"] = n * ((10 + C) * 4 + 1)
    for k in ("metrics", "loss"):
        res[f"{k}_bytes_per_s"] = res["bytes"] / (res[f"{k}_ms"]["median"] * 1e-3)
        res[f"{k}_share_of_achievable_hbm"] = res[f"{k}_bytes_per_s"] / ACHIEVABLE_HBM
    spread = max(res["metrics_ms"]["max"] - res["metrics_ms"]["min"], res["loss_ms"]["max"] - res["loss_ms"]["min"])
    res["metrics_minus_loss_ms"] = res["metrics_ms"]["median"] - res["loss_ms"]["median"]
    res["slower_than_loss_beyond_spread"] = res["metrics_minus_loss_ms"] > spread
    res["speedup_over_torch_expressions"] = res["torch_expressions_ms"]["median"] / res["metrics_ms"]["median"]
    res["max_rel_sum_difference_from_torch"] = rel
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=str(Path(__file__).resolve().parents[1] / "profiles" / "metrics_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_metrics.py measures on the GPU"
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "classes": C, "repeats": args.repeats, "warmup": args.warmup,
           "achievable_hbm_bytes_per_s": ACHIEVABLE_HBM, "sizes": [bench(n, dev, args.warmup, args.repeats) for n in args.rows]}
    print(json.dumps(res))
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
