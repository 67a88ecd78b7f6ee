"""Dev script: time of the two rulebook builders (ops.brick_pyramid, ops.build_pyramid) on a bench cloud's voxels, device events.

    python tools/bench_pyramid.py [points=1000000] [voxel=0.02] [foliage_fraction=0] [clouds per launch set=1, or a list: 1,16]

One JSON line per launch-set size: the median and the spread of REPS calls after a warm-up.
"""
import json, sys
from pathlib import Path
ROOT = Path(__file__).resolve().parents[1]; sys.path.insert(0, str(ROOT))
import torch, numpy as np
import bench
from smart_tree_amd.data_types.cloud import Cloud
from smart_tree_amd.synthetic import sample_tree_cloud
from smart_tree_amd.dataset.dataset import voxelize_blocks
from smart_tree_amd.model import sparse_ops as ops
import ctypes as _ct, os as _os
from smart_tree_amd import _lib as _l
if _os.environ.get("ST_PROBE_LIB"):  # A/B aid: another build of the library (e.g. the previous revision's .so kept under _ab/)
    _l._LIB = _l.declare(_ct.CDLL(_os.environ["ST_PROBE_LIB"]))
dev = torch.device("cuda:0")
pipe = bench.build_pipeline(dev)
NPTS = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
VOX = float(sys.argv[2]) if len(sys.argv) > 2 else 0.02
FOL = float(sys.argv[3]) if len(sys.argv) > 3 else 0.0
BATCHES = [int(v) for v in sys.argv[4].split(",")] if len(sys.argv) > 4 else [1]  # clouds per launch set (Cloud.collate)
WARM, REPS = 3, 20
clouds = []
for b in range(max(BATCHES)):
    c = sample_tree_cloud(NPTS, seed=(3 if FOL else 0) + b, **({"foliage_fraction": FOL} if FOL else {}))
    clouds.append(Cloud(xyz=torch.from_numpy(c["xyz"]).to(dev), rgb=torch.from_numpy(c["rgb"]).to(dev)))
def times_us(fn):
    for _ in range(WARM): fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return {"median_us": round(float(np.median(out)), 1), "min_us": round(min(out), 1), "max_us": round(max(out), 1)}
for batch in BATCHES:
    cloud = pipe.preprocessing(Cloud.collate(clouds[:batch]) if batch > 1 else clouds[0])
    vb = voxelize_blocks(cloud.xyz, cloud.rgb, VOX, seg_off=cloud.seg_off)
    hint = (vb.block_centres.shape[0], int(round(4.8 / VOX)) + 2)  # as Smart_Tree.features sizes the bricks
    ordered = ops.move_rows(vb.coords, ops.spatial_order(vb.coords))  # the hash-table builders see Morton-ordered rows there
    got = ops.brick_pyramid(vb.coords, 3, *hint, vb.blk_seg, vb.n_seg)
    assert got is not None, "the brick pyramid cannot be sized for this input"
    line = {"lib": _os.environ.get("ST_PROBE_LIB", "built"), "points": NPTS, "voxel": VOX, "clouds": batch,
            "levels": [x.shape[0] for x in got[0].coords],
            "brick_pyramid": times_us(lambda: ops.brick_pyramid(vb.coords, 3, *hint, vb.blk_seg, vb.n_seg)),
            "build_pyramid": times_us(lambda: ops.build_pyramid(ordered, 3, vb.blk_seg, vb.n_seg))}
    print(json.dumps(line), flush=True)
