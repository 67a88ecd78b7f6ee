"""Time of `dataset.synthetic.generate_trees` for 1, 20 and 64 trees of 1M points on the GPU, against the way the same clouds got
onto the device before it: `synthetic.sample_tree_cloud` on the host plus the upload.  Prints one JSON line.

Per batch size:
* generate_ms       whole call (host tree growth, table upload, the launch), host clock around a device synchronise, median
* kernel_ms         st_synth_points_seg alone on resident tables and outputs, device events, median
* write_gbps        36 bytes per point over kernel_ms; write_bound_fraction: that over the achievable HBM rate (6.3 TB/s; of the
                    8 TB/s peak: write_peak_fraction)
* host_sample_ms    sample_tree_cloud for every tree (one pass; it is seconds long) and upload_ms, the copies of its four arrays
No GPU: the tool fails, it does not fall back.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from smart_tree_amd import _lib  # noqa: E402
from smart_tree_amd.dataset import synthetic as S  # noqa: E402
from smart_tree_amd.synthetic import grow_tree, sample_tree_cloud  # noqa: E402

BYTES_PER_POINT = 36
HBM_ACHIEVABLE, HBM_PEAK = 6.3e12, 8.0e12


def kernel_ms(dev, B, n_points, depth, fraction, warmup, iters):
    tables = [S.segment_table(grow_tree(s, 1.0, depth)) for s in range(B)]
    out = {k: torch.empty(shape, dtype=dt, device=dev) for k, (shape, dt) in
           {"xyz": ((B * n_points, 3), torch.float32), "medial_vector": ((B * n_points, 3), torch.float32),
            "class_l": ((B * n_points,), torch.float32), "branch_ids": ((B * n_points,), torch.int32),
            "segment": ((B * n_points,), torch.int32)}.items()}
    off = lambda sizes: np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    tab_off, tip_off, pt_off = off([len(t.ra) for t in tables]), off([len(t.tips) for t in tables]), off([n_points] * B)
    rows = torch.from_numpy(np.concatenate([t.rows() for t in tables])).to(dev)
    cdf = torch.from_numpy(np.concatenate([t.cdf for t in tables]).view(np.int32)).to(dev)
    tips = torch.from_numpy(np.concatenate([t.tips for t in tables])).to(dev)
    seeds = np.arange(B, dtype=np.uint64)
    thr = np.full(B, S.foliage_threshold(fraction), dtype=np.uint32)
    noise, sigma = np.full(B, 0.002, np.float32), np.full(B, 0.08, np.float32)
    h = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    L = _lib.lib()

    def launch():
        _lib.check(L.st_synth_points_seg(_lib.ptr(rows), h(tab_off), _lib.ptr(cdf), _lib.ptr(tips), h(tip_off), h(pt_off), B, h(seeds),
                                         h(thr), h(noise), h(sigma), _lib.ptr(out["xyz"]), _lib.ptr(out["medial_vector"]),
                                         _lib.ptr(out["class_l"]), _lib.ptr(out["branch_ids"]), _lib.ptr(out["segment"]),
                                         _lib.stream(dev)))

    for _ in range(warmup):
        launch()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times), int(tab_off[-1])


def generate_ms(dev, B, n_points, depth, fraction, warmup, iters):
    times = []
    for it in range(warmup + iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        cloud, _ = S.generate_trees(list(range(B)), n_points, foliage_fraction=fraction, max_depth=depth, device=dev)
        torch.cuda.synchronize()
        if it >= warmup:
            times.append((time.perf_counter() - t0) * 1e3)
        del cloud
    return statistics.median(times)


def host_path_ms(dev, B, n_points, depth, fraction):
    sample = upload = 0.0
    for s in range(B):
        t0 = time.perf_counter()
        c = sample_tree_cloud(n_points, seed=s, foliage_fraction=fraction, max_depth=depth)
        t1 = time.perf_counter()
        on_dev = [torch.from_numpy(c[k]).to(dev) for k in ("xyz", "rgb", "medial_vector", "class_l")]
        torch.cuda.synchronize()
        upload += time.perf_counter() - t1
        sample += t1 - t0
        del on_dev
    return sample * 1e3, upload * 1e3


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--trees", type=int, nargs="+", default=[1, 20, 64])
    ap.add_argument("--max-depth", type=int, default=7)
    ap.add_argument("--foliage-fraction", type=float, default=0.3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--no-host-path", action="store_true", help="skip the sample_tree_cloud + upload comparison")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_synth: needs the GPU (no CPU fallback; a CPU timing would say nothing)")
    dev = torch.device("cuda:0")
    result = {"points_per_tree": a.points, "max_depth": a.max_depth, "foliage_fraction": a.foliage_fraction, "warmup": a.warmup,
              "iters": a.iters, "bytes_per_point": BYTES_PER_POINT, "device": torch.cuda.get_device_name(0), "batches": {}}
    for B in a.trees:
        k_ms, n_seg = kernel_ms(dev, B, a.points, a.max_depth, a.foliage_fraction, a.warmup, a.iters)
        g_ms = generate_ms(dev, B, a.points, a.max_depth, a.foliage_fraction, 1, min(a.iters, 3))
        rate = BYTES_PER_POINT * B * a.points / (k_ms * 1e-3)
        row = {"segments": n_seg, "kernel_ms": round(k_ms, 4), "generate_ms": round(g_ms, 2), "write_gbps": round(rate / 1e9, 1),
               "write_bound_fraction": round(rate / HBM_ACHIEVABLE, 4), "write_peak_fraction": round(rate / HBM_PEAK, 4),
               "points_per_second": round(B * a.points / (k_ms * 1e-3))}
        if not a.no_host_path:
            s_ms, u_ms = host_path_ms(dev, B, a.points, a.max_depth, a.foliage_fraction)
            row.update(host_sample_ms=round(s_ms, 1), upload_ms=round(u_ms, 2),
                       speedup_whole_call=round((s_ms + u_ms) / g_ms, 1))
        result["batches"][str(B)] = row
    print(json.dumps(result))
    return result


if __name__ == "__main__":
    main()
