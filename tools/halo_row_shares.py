"""Dev script, CPU only: the share of every level's rows the decoder needs when only the inner voxels' outputs are kept -- the rule
of csrc/st_rule.h ("Which decoder rows ...") restated in numpy on the oracle's voxelisation of the benchmark trees.
python tools/halo_row_shares.py [seed ...]   (default: seeds 0 and 1 at 2 cm voxels, 4 m blocks, 0.4 m halo)
With trace files (tools/trace_one_batch.py output) as --parent / --candidate it also prints the per-layer duration ratios of the
decoder's kernels next to the shares, so that a layer that did not shrink with its rows is visible."""
import argparse
import re
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from oracle import unet_oracle as uo  # noqa: E402
from oracle import voxel_oracle as vo  # noqa: E402
from smart_tree_amd.synthetic import sample_tree_cloud  # noqa: E402

BASE = (0, 1, 2, 2)  # a[l]: base margin per level


def shares(seed, points=1_000_000, voxel=0.02, block=4.0, halo=0.4):
    c = sample_tree_cloud(points, seed=seed)
    v = vo.voxelize_cloud(vo.centre_cloud(c["xyz"]), c["rgb"], voxel, block, halo)
    coords, mask = v["coords"].astype(np.int64), v["mask"].astype(bool)
    nb = int(coords[:, 0].max()) + 1
    lo, hi = np.full((nb, 3), 2 ** 30), np.full((nb, 3), -1)
    np.minimum.at(lo, coords[mask, 0], coords[mask, 1:])
    np.maximum.at(hi, coords[mask, 0], coords[mask, 1:])
    out, level_coords = [], coords
    for level in range(4):
        b, cc = level_coords[:, 0], level_coords[:, 1:]
        blo, bhi = lo[b] >> level, (hi[b] + (1 << level) - 1) >> level
        margin = np.maximum(np.maximum(blo - cc, cc - bhi), 0).max(1)
        margin[(lo[b] > hi[b]).any(1)] = 10 ** 6
        out.append((len(level_coords), [float((margin <= BASE[level] + t).mean()) for t in range(3)]))
        if level < 3:
            level_coords = uo.strided_out_coords(level_coords.astype(np.int32)).astype(np.int64)
    return int(mask.sum()), out


def decoder_lines(path):
    """the folded decoder lines of a trace: from the first conv after the bottom level to k_heads"""
    rows = []
    for line in Path(path).read_text().splitlines():
        m = re.match(r"\s*[\d.]+ ms\s+\+gap\s+[-\d.]+ us\s+x(\d+)\s+([\d.]+) us\s+(.*)", line)
        if m and ("k_sparse_conv" in m.group(3) or "k_heads" in m.group(3) or "k_rb_move_rows" in m.group(3) or "k_bk_inner" in m.group(3)
                  or "k_bk_need" in m.group(3)):
            rows.append((m.group(3).strip(), int(m.group(1)), float(m.group(2))))
    return rows


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("seeds", nargs="*", type=int, default=[0, 1])
    ap.add_argument("--parent", nargs="*", default=[])
    ap.add_argument("--candidate", nargs="*", default=[])
    a = ap.parse_args()
    for seed in a.seeds:
        inner, levels = shares(seed)
        print(f"seed {seed}: level-0 rows {levels[0][0]}, inner {inner} ({inner / levels[0][0]:.3f})")
        for level, (n, s) in enumerate(levels):
            print(f"  L{level}: {n:8d} rows, margin <= a / a+1 / a+2 (a = {BASE[level]}): " + " / ".join(f"{x:.3f}" for x in s))
    for side, files in (("parent", a.parent), ("candidate", a.candidate)):
        for f in files:
            rows = decoder_lines(f)
            conv = sum(d for n, _, d in rows if "k_sparse_conv" in n)
            lists = sum(d for n, _, d in rows if "k_bk_inner" in n or "k_bk_need" in n)
            print(f"{side} {f}: conv family {conv:.1f} us, list kernels {lists:.1f} us, k_heads "
                  f"{sum(d for n, _, d in rows if 'k_heads' in n):.1f} us, row moves {sum(d for n, _, d in rows if 'k_rb_move' in n):.1f} us")
            for n, c, d in rows:
                print(f"    x{c:<2d} {d:8.1f} us  {n}")
