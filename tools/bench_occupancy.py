"""Time of `st_beam_tally_seg` (csrc/occupancy.hip) on the GPU: the aggregated and the plain form, and for context a torch stand-in.
Prints one JSON line and writes it to profiles/occupancy_bench.json (`--out`).

Device events around the call alone (resident beams; the call's output allocations, zeroing, launches and its read-back of the
two counters are inside), warm-up 2, median of 7, as tools/bench_scan.py.
* scene     `scan_trees` on one depth-7 tree with leaves under 1, 3 and 8 scanners of `--step-deg` beams; the grid is
            `VoxelGrid.around` the returns with a margin of 0.2 m, at cells of 0.1 m and 0.05 m
* aggregated_ms / plain_ms   `beam_tally` with form="aggregated" / "plain".  Both results are compared in this very run: `same_bits`
            must be true (the tool fails otherwise)
* torch_ms  the stand-in: points every cell / 4 along every beam up to min(range, the far side of the grid), floored to cells and
            `bincount`ed.  It is APPROXIMATE -- it counts samples, not beams, it misses cells a beam clips by less than cell / 4,
            and it gives neither `hit`, `behind` nor a path length; it is here only to say what the obvious torch code costs
            (warm-up 1, median of 3: it is the slow one)
* default   the form "auto" resolves to must be the faster one on the 3-scanner case at 0.1 m: `default_is_faster_on_3_scanners`
No GPU: the tool fails, it does not fall back.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from smart_tree_amd import occupancy as OC  # noqa: E402
from smart_tree_amd.dataset import synthetic as S  # noqa: E402


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


def torch_stand_in(origins, idx, w, rng, grid, chunk=1 << 16):
    """Samples every cell / 4 along the beams inside the grid, counted per cell: an approximation of `enter` weighted by chord."""
    lo = torch.tensor(grid.lo, device=w.device)
    hi = torch.tensor(grid.hi, device=w.device)
    dim = torch.tensor(grid.dim, device=w.device)
    step = grid.cell / 4.0
    counts = torch.zeros(grid.n_cells, dtype=torch.int64, device=w.device)
    reach = float(torch.linalg.norm(hi - lo)) + float(torch.linalg.norm(origins - 0.5 * (lo + hi), dim=1).max())
    n_steps = int(reach / step) + 1
    s = torch.arange(n_steps, device=w.device, dtype=torch.float32) * step
    for first in range(0, w.shape[0], chunk):
        rows = slice(first, first + chunk)
        o = origins.index_select(0, idx[rows].long())
        for s0 in range(0, n_steps, 256):  # (a chunk of beams x 256 samples at a time: the whole product does not fit)
            ss = s[s0:s0 + 256]
            p = o[:, None, :] + ss[None, :, None] * w[rows][:, None, :]
            ok = (ss[None, :] <= rng[rows][:, None]) & ((p >= lo) & (p < hi)).all(2)
            c = torch.floor((p[ok] - lo) / grid.cell).long()
            c = torch.minimum(c.clamp_(min=0), dim - 1)
            counts += torch.bincount((c[:, 0] * grid.dim[1] + c[:, 1]) * grid.dim[2] + c[:, 2], minlength=grid.n_cells)
    return counts


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--step-deg", type=float, default=0.05)
    ap.add_argument("--max-depth", type=int, default=7)
    ap.add_argument("--leaves-per-tip", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--skip-torch", action="store_true")
    ap.add_argument("--out", default=str(Path(__file__).resolve().parents[1] / "profiles" / "occupancy_bench.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_occupancy: needs the GPU (no CPU fallback; a CPU timing would say nothing)")
    dev = torch.device("cuda:0")
    result = {"step_deg": a.step_deg, "max_depth": a.max_depth, "leaves_per_tip": a.leaves_per_tip, "warmup": a.warmup, "iters": a.iters,
              "device": torch.cuda.get_device_name(0), "cases": [],
              "timed": "beam_tally: output allocation, zeroing, launches and the read-back of the two counters",
              "torch_stand_in": "approximate: samples every cell/4 along the beams, bincount; no hit, behind or path"}
    for scanners in (1, 3, 8):
        cloud, _, extras = S.scan_trees([0], scanners, step_deg=a.step_deg, max_depth=a.max_depth, leaves_per_tip=a.leaves_per_tip,
                                        leaf_radius=0.03, range_noise=0.0, device=dev, beams=True)
        beams = (extras["origins"], extras["beam_scanner"], extras["beam_dir"], extras["beam_range"])
        for cell in (0.1, 0.05):
            grid = OC.VoxelGrid.around(cloud.xyz, cell, margin=0.2)
            got = {}

            def run(form):
                got[form] = OC.beam_tally(*beams, grid, form=form, hit_cell=True)

            row = {"scanners": scanners, "cell": cell, "beams": int(beams[3].shape[0]), "returns": len(cloud), "dim": list(grid.dim)}
            for form in ("aggregated", "plain"):
                row[f"{form}_ms"] = round(time_ms(lambda: run(form), a.warmup, a.iters), 4)
            x, y = got["aggregated"], got["plain"]
            row["same_bits"] = all(torch.equal(getattr(x, k), getattr(y, k)) for k in ("enter", "hit", "behind", "path", "hit_cell")) and \
                (x.n_bad, x.n_outside) == (y.n_bad, y.n_outside)
            row["cells_entered_total"] = int(x.enter.sum())
            row["steps_per_beam"] = round((int(x.enter.sum()) + int(x.behind.sum())) / max(row["beams"], 1), 1)
            fast = min(row["aggregated_ms"], row["plain_ms"])
            row["beams_per_s"] = round(row["beams"] / (fast * 1e-3))
            if not a.skip_torch:
                row["torch_ms"] = round(time_ms(lambda: torch_stand_in(*beams, grid), 1, 3), 3)
                row["kernel_not_slower_than_torch"] = fast <= row["torch_ms"]
            result["cases"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
            if not row["same_bits"]:
                raise SystemExit(f"bench_occupancy: the two forms differ on {row}")
    three = next(r for r in result["cases"] if r["scanners"] == 3 and r["cell"] == 0.1)
    result["faster_on_3_scanners"] = "aggregated" if three["aggregated_ms"] <= three["plain_ms"] else "plain"
    # what "auto" resolves to: the form whose time an auto call matches is not measurable apart; the library says it by its bits being
    # the same, so the default is read from the source's OC_AUTO_FORM
    src = (Path(__file__).resolve().parents[1] / "smart_tree_amd" / "csrc" / "occupancy.hip").read_text()
    auto = {"1": "aggregated", "2": "plain"}[src.split("#define OC_AUTO_FORM ")[1].split()[0]]
    result["auto_form"] = auto
    result["default_is_faster_on_3_scanners"] = auto == result["faster_on_3_scanners"]
    line = json.dumps(result)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")
    return result


if __name__ == "__main__":
    main()
