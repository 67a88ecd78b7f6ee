"""Time the offscreen renderer on the workload a capture is: python tools/bench_render.py [--points 1000000] [--views 8] [--width 1920]
[--height 1080] [--repeats 20] [--warmup 5] [--out FILE.json]

One synthetic labelled tree (`generate_trees`, 30 % foliage) and its ground-truth skeleton, a turntable of `views` cameras, three
passes, each a whole frame (clear, draw, resolve to rgb + depth + ids) through `Renderer.render`:
  points    the cloud coloured by class, one pixel per point
  lines     the medial vectors, one line per point
  skeleton  the skeleton's capsules over the cloud
and the points pass once more as a plain torch expression on the same device (project, pack an int64 key, `scatter_reduce(amin)`,
gather), whose ids are compared with the kernel's.  Every timing is a pair of events on the stream around one frame; reported as the
median of the repeats with min and max, and as points x views per second."""
import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch

from smart_tree_amd import render as R
from smart_tree_amd.dataset.synthetic import generate_trees

NEAR = 0.01


def torch_points(xyz, classes, cmap8, cams, H, W):
    """The points pass as torch expressions: rgb uint8 [V,H,W,3], ids int64 [V,H,W] (-1 background)."""
    n = xyz.shape[0]
    index = torch.arange(n, device=xyz.device)
    empty = torch.iinfo(torch.int64).max
    rgb, ids = [], []
    for c in cams:
        pc = xyz @ c[:9].view(3, 3).T + c[9:12]
        z = pc[:, 2]
        iu = torch.floor(c[12] * pc[:, 0] / z + c[14] + 0.5).long()
        iw = torch.floor(c[13] * pc[:, 1] / z + c[15] + 0.5).long()
        ok = (z > NEAR) & (iu >= 0) & (iu < W) & (iw >= 0) & (iw < H)
        key = (z.view(torch.int32).long() << 32) | index
        fb = torch.full((H * W,), empty, dtype=torch.int64, device=xyz.device)
        fb = fb.scatter_reduce(0, (iw * W + iu)[ok], key[ok], "amin")
        hit = fb != empty
        who = torch.where(hit, fb & 0xFFFFFFFF, torch.zeros_like(fb))
        img = torch.where(hit[:, None], cmap8[classes[who]], torch.full_like(cmap8[:1], 255))
        rgb.append(img.view(H, W, 3))
        ids.append(torch.where(hit, who, torch.full_like(who, -1)).view(H, W))
    return torch.stack(rgb), torch.stack(ids)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=str(Path(__file__).resolve().parents[1] / "profiles" / "render_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_render.py measures on the GPU"
    dev = torch.device("cuda:0")
    W, H, V, n = args.width, args.height, args.views, args.points

    cloud, skeletons = generate_trees([7], n, foliage_fraction=0.3, device=dev)
    cloud.seg_off = None
    cmap = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0))
    points = R.cloud_items(cloud, "class", cmap=cmap)
    lines = R.medial_vector_items(cloud)
    tubes = R.skeleton_items(skeletons[0], device=dev)
    cameras = R.turntable(V, points, W, H, elevation=0.3)
    cams = R.camera_rows(cameras, dev)
    r = R.Renderer(W, H, near=NEAR, shading=None)

    frames = {"points": lambda: r.render(points, cams), "lines": lambda: r.render(lines, cams),
              "skeleton": lambda: r.render(points + tubes, cams)}
    classes = cloud.class_l.view(-1).long()
    cmap8 = torch.tensor(cmap, device=dev).mul(255).add(0.5).floor().to(torch.uint8)
    expression = lambda: torch_points(cloud.xyz, classes, cmap8, cams, H, W)

    ours, (t_rgb, t_ids) = frames["points"](), expression()
    covered = ours["ids"] >= 0
    res = {"device": torch.cuda.get_device_name(0), "points": n, "views": V, "width": W, "height": H, "segments": {"lines": n, "skeleton": len(tubes[0])},
           "repeats": args.repeats, "warmup": args.warmup, "covered_pixel_share": float(covered.float().mean()),
           # matmul rounds the projection in another order than the kernel: a point on a pixel boundary may land next door
           "torch_ids_differ_share": float((t_ids != ours["ids"].long()).float().mean()),
           "torch_rgb_differ_share": float((t_rgb != ours["rgb"]).any(-1).float().mean())}
    assert res["torch_ids_differ_share"] < 1e-3, res
    for name, fn in frames.items():
        res[f"{name}_ms"] = timed(fn, args.warmup, args.repeats)
        res[f"{name}_point_views_per_s"] = n * V / (res[f"{name}_ms"]["median"] * 1e-3)
    res["torch_points_ms"] = timed(expression, args.warmup, args.repeats)
    res["points_speedup_over_torch"] = res["torch_points_ms"]["median"] / res["points_ms"]["median"]
    two = frames["skeleton"]()
    again = frames["skeleton"]()
    res["bit_identical_runs"] = bool(all(torch.equal(two[k], again[k]) for k in two))
    print(json.dumps(res))
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
