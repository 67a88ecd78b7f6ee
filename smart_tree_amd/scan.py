"""A virtual terrestrial laser scanner: skeletons ray-cast to occluded, labelled clouds (csrc/scan.hip).

`python -m smart_tree_amd.scan skeleton=<skeleton.npz> out=<.npz|.ply> [scanners=3] [radius=6] [height=1.5] [step_deg=0.05]
[range_noise=0.002] [seed=0] [form=auto] [device=cuda:0] [beams=<beams.npz>]` scans a saved skeleton from a ring of positions around
it and writes the cloud (`util.file.load_cloud` reads it back); with `beams=` also every beam of the scan, returned or not, as the
file `python -m smart_tree_amd.occupancy` reads.  Overrides are parsed by config.py, as for `segmentation` / `render`.

What `dataset.synthetic.generate_trees` cannot give: a cloud that sees one side of a stem from each position, thins out with the
square of the range and has shadows wherever a nearer branch stands in the way.  The surface of a tube is the zero set of the
point-to-tube residual the whole package uses (a frustum's side and the parts of the two end spheres outside it); a beam returns
its first hit in [min_range, max_range]; a beam that starts inside a tube returns that tube's far wall.  Not modelled: beam
divergence, multiple returns, intensity, drop-out, a ground surface, a moving platform.
"""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass, replace
from pathlib import Path
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .data_types.cloud import Cloud
from .data_types.flat import FlatSkeletons

FORMS = {"auto": 0, "dense": 1, "grid": 2}
MAX_SCANNERS = 4096  # ST_SCAN_MAX_SCANNERS
_M64 = (1 << 64) - 1


def to_frame(xyz, up: int):
    """Coordinates [..., 3] in the frame of a scanner that rotates about world axis `up`: the axes in the cyclic order
    (up + 1, up + 2, up), so that the frame's z is `up` -- a permutation, no rounding.  `from_frame` is its inverse."""
    return xyz[..., [(up + 1) % 3, (up + 2) % 3, up]]


def from_frame(xyz, up: int):
    return xyz[..., [(2 - up) % 3, (3 - up) % 3, (4 - up) % 3]]


@dataclass
class Scanner:
    """One scanner position (world coordinates) and its window of beams: beam (i, j) has azimuth az[0] + i az[1], elevation
    el[0] + j el[1] (radians); az[2] x el[2] beams, ray k = i el[2] + j.  The scanner rotates about world axis `up`: in its frame
    (`to_frame`) the direction is (cos el cos az, cos el sin az, sin el), so the pole of the window is `up` and beams are evenly
    spread around the horizon.  Ranges in metres; `range_noise` is the standard deviation of the normal draw that moves a hit
    along its beam."""
    position: Sequence[float]
    az: Tuple[float, float, int] = (0.0, math.radians(0.05), 0)
    el: Tuple[float, float, int] = (0.0, math.radians(0.05), 0)
    min_range: float = 0.05
    max_range: float = math.inf
    range_noise: float = 0.002
    seed: int = 0
    up: int = 2

    def __post_init__(self):
        if self.up not in (0, 1, 2):
            raise ValueError(f"Scanner: up must be 0, 1 or 2, got {self.up}")
        pos = [float(x) for x in np.asarray(self.position, dtype=np.float64).reshape(-1)]
        values = pos + [float(self.az[0]), float(self.az[1]), float(self.el[0]), float(self.el[1]), float(self.range_noise)]
        if len(pos) != 3 or not all(math.isfinite(v) and abs(v) <= 3.4028234e38 for v in values):
            raise ValueError(f"Scanner: position, angles and range_noise must be finite (got position={self.position}, az={self.az}, "
                             f"el={self.el}, range_noise={self.range_noise})")
        if math.isnan(self.min_range) or math.isnan(self.max_range) or self.min_range < 0 or self.max_range < self.min_range:
            raise ValueError(f"Scanner: 0 <= min_range <= max_range, got {self.min_range}, {self.max_range}")
        if int(self.az[2]) < 0 or int(self.el[2]) < 0:
            raise ValueError(f"Scanner: negative beam count ({self.az[2]} x {self.el[2]})")
        self.position = tuple(pos)

    @property
    def n_rays(self) -> int:
        return int(self.az[2]) * int(self.el[2])

    @staticmethod
    def towards(box_lo, box_hi, position, step_deg: float = 0.05, up: int = 2, **kw) -> "Scanner":
        """A window of `step_deg` beams that covers the box [box_lo, box_hi] seen from `position` by a scanner that rotates about
        `up`: the azimuths of its corners about the azimuth of its centre, and elevations bounded through the nearest and the
        farthest horizontal distance."""
        if up not in (0, 1, 2):
            raise ValueError(f"Scanner.towards: up must be 0, 1 or 2, got {up}")
        world = np.asarray(position, dtype=np.float64).reshape(3)
        lo, hi, p = (to_frame(np.asarray(v, dtype=np.float64).reshape(3), up) for v in (box_lo, box_hi, position))
        if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (hi >= lo).all()):
            raise ValueError(f"Scanner.towards: a finite box with hi >= lo, got {box_lo}, {box_hi}")
        if not (math.isfinite(step_deg) and step_deg > 0):
            raise ValueError(f"Scanner.towards: step_deg must be finite and > 0, got {step_deg}")
        step = math.radians(step_deg)
        corners = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])]) - p
        rho = np.hypot(corners[:, 0], corners[:, 1])
        near = np.hypot(*np.maximum(np.maximum(lo[:2] - p[:2], p[:2] - hi[:2]), 0.0))
        if near == 0.0:  # the scanner's vertical line passes through the box: every azimuth
            az0, az1 = -math.pi, math.pi
        else:
            centre = 0.5 * (lo + hi) - p
            azc = math.atan2(centre[1], centre[0])
            rel = np.arctan2(corners[:, 1], corners[:, 0]) - azc
            rel = (rel + math.pi) % (2 * math.pi) - math.pi
            az0, az1 = azc + rel.min(), azc + rel.max()
        z0, z1 = lo[2] - p[2], hi[2] - p[2]
        el0 = math.atan2(z0, near if z0 < 0 else rho.max())
        el1 = math.atan2(z1, near if z1 > 0 else rho.max())
        count = lambda a, b: int(math.floor((b - a) / step)) + 2
        return Scanner(tuple(world), (az0, step, count(az0, az1)), (el0, step, count(el0, el1)), up=up, **kw)


def scanner_ring(n: int, radius: float, height: float, box, step_deg: float = 0.05, up: int = 1, seed: int = 0, **kw) -> list:
    """`n` scanners evenly on a circle of `radius` about the box's centre, `height` above its lowest side along axis `up` (the
    package's trees grow along axis 1), each rotating about `up` with a window that covers `box` = (lo, hi).  Scanner k draws its
    noise with `seed + k`."""
    lo, hi = (np.asarray(v, dtype=np.float64).reshape(3) for v in box)
    h0, h1 = [k for k in range(3) if k != up]
    out = []
    for k in range(int(n)):
        phi = 2.0 * math.pi * k / max(int(n), 1)
        p = 0.5 * (lo + hi)
        p[h0] += radius * math.cos(phi)
        p[h1] += radius * math.sin(phi)
        p[up] = lo[up] + height
        out.append(Scanner.towards(lo, hi, p, step_deg, up=up, seed=int(seed) + k, **kw))
    return out


def scan_cast(a, b, r1, r2, tube_off, tube_class, tube_branch, scanners: Sequence[Sequence[Scanner]], form="auto",
              outputs=("dir", "range", "tube", "xyz", "medial_vector", "class_l", "branch_ids", "segment", "ray")) -> dict:
    """`st_scan_cast_seg` on device tensors: tubes a, b [m,3], r1, r2 [m], tube_off [B+1] (None: one cloud), tube_class [m] uint8,
    tube_branch [m] int32 (either may be None); `scanners`: per cloud a list of `Scanner`.  Returns the requested tensors -- per ray
    "dir", "range", "tube"; per hit, sliced to the hits after the call's one read-back, the others -- plus "n_hits" (int), "ray_off"
    (numpy int64 [S+1]), "scanner_cloud" (numpy int32 [S]) and "ws" (the call's workspace, for `grid_plan`).  Tubes and scanners are in
    the scanners' frame (`Scanner.up` = 2); `scan_skeletons` is the call that takes world coordinates."""
    L = _lib.lib()
    dev = a.device
    f = lambda t, shape: t.to(dev).float().reshape(shape).contiguous()
    a, b, r1, r2 = f(a, (-1, 3)), f(b, (-1, 3)), f(r1, (-1,)), f(r2, (-1,))
    m, nseg = a.shape[0], len(scanners)
    if tube_off is not None:
        tube_off = torch.as_tensor(tube_off).to(dev).to(torch.int32).contiguous()
        if tube_off.shape[0] != nseg + 1:
            raise ValueError(f"scan_cast: {nseg} lists of scanners for {tube_off.shape[0] - 1} cloud(s)")
    elif nseg != 1:
        raise ValueError("scan_cast: a batch needs the offsets of its tubes")
    if tube_class is not None:
        tube_class = tube_class.to(dev).to(torch.uint8).contiguous()
    if tube_branch is not None:
        tube_branch = tube_branch.to(dev).to(torch.int32).contiguous()
    flat = [(c, s) for c, per_cloud in enumerate(scanners) for s in per_cloud]
    if any(s.up != 2 for _, s in flat):
        raise ValueError("scan_cast works in the scanners' own frame (up = 2); scan_skeletons turns tubes and positions into it")
    S = len(flat)
    if S > MAX_SCANNERS:
        raise ValueError(f"scan_cast: at most {MAX_SCANNERS} scanners per call (got {S})")
    table = (_lib.StScanner * max(S, 1))()
    ray_off = np.zeros(S + 1, np.int64)
    for k, (c, s) in enumerate(flat):
        t = table[k]
        t.cloud, t.n_az, t.n_el, t.reserved = c, int(s.az[2]), int(s.el[2]), 0
        t.position[0], t.position[1], t.position[2] = s.position
        t.az0, t.daz, t.el0, t.del_ = float(s.az[0]), float(s.az[1]), float(s.el[0]), float(s.el[1])
        t.min_range, t.max_range, t.range_noise, t.seed = float(s.min_range), float(s.max_range), float(s.range_noise), int(s.seed) & _M64
        ray_off[k + 1] = ray_off[k] + s.n_rays
    R = int(ray_off[-1])
    shapes = {"dir": ((R, 3), torch.float32), "range": ((R,), torch.float32), "tube": ((R,), torch.int32),
              "xyz": ((R, 3), torch.float32), "medial_vector": ((R, 3), torch.float32), "class_l": ((R,), torch.float32),
              "branch_ids": ((R,), torch.int32), "segment": ((R,), torch.int32), "ray": ((R,), torch.int32)}
    out = {k: torch.empty(shape, dtype=dt, device=dev) if k in outputs else None for k, (shape, dt) in shapes.items()}
    n_hits = torch.zeros(1, dtype=torch.int64, device=dev)
    nbytes = L.st_scan_cast_workspace_bytes(R, m, S, nseg)
    if nbytes < 0:
        raise _lib.StError(f"scan_cast: {R} beams, {m} tubes, {S} scanners and {nseg} cloud(s) are outside what the call takes")
    ws = _lib.workspace(nbytes, dev)
    p = lambda t: _lib.ptr(t) if t is not None and t.numel() else None
    _lib.check(L.st_scan_cast_seg(p(a), p(b), p(r1), p(r2), m, p(tube_off) if nseg > 1 else None, nseg, p(tube_class), p(tube_branch),
                                  ctypes.cast(table, ctypes.c_void_p), S, ray_off.ctypes.data_as(ctypes.c_void_p),
                                  FORMS[form] if isinstance(form, str) else int(form), p(out["dir"]), p(out["range"]), p(out["tube"]),
                                  p(out["xyz"]), p(out["medial_vector"]), p(out["class_l"]), p(out["branch_ids"]), p(out["segment"]),
                                  p(out["ray"]), _lib.ptr(n_hits), _lib.ptr(ws), ws.numel(), _lib.stream(dev)))
    n = int(n_hits.item())  # the one read-back
    res = {k: (v if k in ("dir", "range", "tube") else v[:n]) for k, v in out.items() if v is not None}
    res.update(n_hits=n, ray_off=ray_off, ws=ws, scanner_cloud=np.asarray([c for c, _ in flat], np.int32))
    return res


def grid_plan(ws, cloud: int = 0) -> dict:
    """Diagnostics (tests, tools/bench_scan.py): the grid a grid-form `scan_cast` built for `cloud`, from the head of its workspace
    (csrc/scan.hip keeps the 64-byte plan records there and asserts their size): lo [3], cell, dim [3], sweep (1: no grid was
    usable and the cloud's tubes are swept one by one)."""
    rec = ws[64 * cloud:64 * cloud + 64].cpu().numpy()
    return {"lo": rec[:12].view(np.float32).copy(), "cell": float(rec[12:16].view(np.float32)[0]), "dim": rec[16:28].view(np.int32).copy(),
            "sweep": int(rec[28:32].view(np.int32)[0])}


def scan_skeletons(skeletons, scanners, leaves=None, form="auto", device=None, beams=False):
    """Scan a batch of clouds.  `skeletons`: one per cloud, anything `FlatSkeletons` takes (a `DisjointTreeSkeleton` gives mutual
    occlusion between its trees); `scanners`: per cloud a list of `Scanner`; `leaves`: per cloud None or (centres [L,3], radii [L]),
    spheres of class 1 that shadow and are hit like the wood.  Returns a batched `Cloud` (`xyz`, zero `rgb`, `medial_vector`,
    `class_l` [N,1], `branch_ids` [N,1] int32 with -1 on leaves, `seg_off`) and a dict per hit: `ray` (its index among the call's
    beams), `scanner` (its scanner's index in cloud-major order), `range` (un-noised), `segment` (the tube, in `FlatSkeletons`'
    order per cloud with the cloud's leaves behind its tubes, counted through the batch; `tube_off` [B+1] has each cloud's first),
    `dir` (the beam's unit direction, world coordinates).  All scanners of a call rotate about the same axis (`Scanner.up`): tubes,
    leaves and positions are permuted into that frame for the cast and the points back, which rounds nothing.
    `beams=True` adds every beam of the call, returned or not, for `occupancy.beam_tally`: `beam_dir` [R,3] (world coordinates),
    `beam_range` [R] (un-noised, +inf without a return), `beam_scanner` [R] int32 and `origins` [S,3] (the scanners' positions, world
    coordinates, cloud-major order)."""
    skeletons, scanners = list(skeletons), [list(s) for s in scanners]
    B = len(skeletons)
    if len(scanners) != B or (leaves is not None and len(leaves) != B):
        raise ValueError(f"scan_skeletons: {B} skeleton(s), {len(scanners)} list(s) of scanners"
                         + (f", {len(leaves)} leaf set(s)" if leaves is not None else "") + ": one of each per cloud")
    if not 1 <= B <= 64:
        raise ValueError(f"scan_skeletons: 1 .. 64 clouds per call (got {B})")
    dev = torch.device(device) if device is not None else torch.device("cuda:0")
    ups = {s.up for per_cloud in scanners for s in per_cloud}
    if len(ups) > 1:
        raise ValueError(f"scan_skeletons: the scanners of one call rotate about one axis, got up = {sorted(ups)}")
    up = ups.pop() if ups else 2
    scanners = [[replace(s, position=tuple(to_frame(np.asarray(s.position), up)), up=2) for s in per_cloud] for per_cloud in scanners]
    flat = FlatSkeletons(skeletons, "scan_skeletons")
    ta, tb, tr1, tr2 = flat.tubes(*flat.float32())
    ta, tb = to_frame(ta, up), to_frame(tb, up)
    branch_of_tube = np.repeat(flat.rows[:, 2], flat.tubes_of_row).astype(np.int32)
    parts = {k: [] for k in ("a", "b", "r1", "r2", "cls", "br")}
    off = [0]
    for c in range(B):
        t0, t1 = int(flat.tube_off[c]), int(flat.tube_off[c + 1])
        centres, radii = (np.zeros((0, 3), np.float32), np.zeros(0, np.float32)) if leaves is None or leaves[c] is None else \
            (to_frame(np.asarray(leaves[c][0], np.float32).reshape(-1, 3), up), np.asarray(leaves[c][1], np.float32).reshape(-1))
        if len(centres) != len(radii):
            raise ValueError(f"scan_skeletons: cloud {c} has {len(centres)} leaf centres and {len(radii)} radii")
        parts["a"] += [ta[t0:t1], centres]; parts["b"] += [tb[t0:t1], centres]
        parts["r1"] += [tr1[t0:t1], radii]; parts["r2"] += [tr2[t0:t1], radii]
        parts["cls"] += [np.zeros(t1 - t0, np.uint8), np.ones(len(radii), np.uint8)]
        parts["br"] += [branch_of_tube[t0:t1], np.full(len(radii), -1, np.int32)]
        off.append(off[-1] + (t1 - t0) + len(radii))
    cat = lambda k, dt: torch.from_numpy(np.ascontiguousarray(np.concatenate(parts[k]), dtype=dt)).to(dev)
    tube_off = np.asarray(off, np.int64)
    if tube_off[-1] >= 2 ** 31:
        raise ValueError(f"scan_skeletons: {tube_off[-1]} tubes do not fit the int32 offsets")
    res = scan_cast(cat("a", np.float32), cat("b", np.float32), cat("r1", np.float32), cat("r2", np.float32),
                    torch.from_numpy(tube_off.astype(np.int32)) if B > 1 else None, cat("cls", np.uint8), cat("br", np.int32), scanners, form,
                    outputs=("dir", "range", "xyz", "medial_vector", "class_l", "branch_ids", "segment", "ray"))
    ray = res["ray"].long()
    world = lambda t: from_frame(t, up).contiguous()
    ray_off = torch.from_numpy(res["ray_off"]).to(dev)
    scanner = torch.searchsorted(ray_off, ray, right=True) - 1 if len(res["ray_off"]) > 1 else torch.zeros_like(ray)
    # hits are in ray order and the scanners in cloud order: a cloud's hits are the ones of its scanners' beams
    first_ray = np.asarray([res["ray_off"][int(np.searchsorted(res["scanner_cloud"], c))] for c in range(B)] + [res["ray_off"][-1]], np.int64)
    seg_off = torch.searchsorted(res["ray"].long(), torch.from_numpy(first_ray).to(dev)).to(torch.int32)
    cloud = Cloud(world(res["xyz"]), torch.zeros_like(res["xyz"]), world(res["medial_vector"]), None, res["branch_ids"].view(-1, 1),
                  res["class_l"].view(-1, 1), seg_off=seg_off)
    extras = {"ray": res["ray"], "scanner": scanner.to(torch.int32), "range": res["range"].index_select(0, ray), "segment": res["segment"],
              "dir": world(res["dir"].index_select(0, ray)), "tube_off": tube_off, "ray_off": res["ray_off"]}
    if beams:
        n_rays = torch.from_numpy(np.diff(res["ray_off"])).to(dev)
        positions = np.asarray([s.position for per_cloud in scanners for s in per_cloud], np.float32).reshape(-1, 3)
        extras.update(beam_dir=world(res["dir"]), beam_range=res["range"], origins=world(torch.from_numpy(positions).to(dev)),
                      beam_scanner=torch.repeat_interleave(torch.arange(len(n_rays), dtype=torch.int32, device=dev), n_rays,
                                                           output_size=int(res["ray_off"][-1])))
    return cloud, extras


def skeleton_box(skeleton, leaves=None):
    """(lo, hi) float64 of a skeleton's tubes inflated by their radii, and of the leaf spheres."""
    flat = FlatSkeletons([skeleton], "skeleton_box")
    pts, rad = [flat.xyz], [flat.radii]
    if leaves is not None:
        pts.append(np.asarray(leaves[0], np.float64).reshape(-1, 3))
        rad.append(np.asarray(leaves[1], np.float64).reshape(-1))
    pts, rad = np.concatenate(pts), np.concatenate(rad)
    ok = np.isfinite(pts).all(1) & np.isfinite(rad)
    if not ok.any():
        raise ValueError("skeleton_box: no finite vertex")
    return (pts[ok] - rad[ok, None]).min(0), (pts[ok] + rad[ok, None]).max(0)


# ---------------------------------------------------------------------------------------------------------------- cli ---
DEFAULTS = {"skeleton": None, "out": None, "scanners": 3, "radius": 6.0, "height": 1.5, "step_deg": 0.05, "range_noise": 0.002,
            "seed": 0, "form": "auto", "device": "cuda:0", "beams": None}
USAGE = ("usage: python -m smart_tree_amd.scan skeleton=<skeleton.npz> out=<.npz|.ply> [scanners=3] [radius=6] [height=1.5] "
         "[step_deg=0.05] [range_noise=0.002] [seed=0] [form=auto|dense|grid] [device=] [beams=<beams.npz>]")


def main(argv=None) -> Cloud:
    import sys

    from .config import apply_overrides
    from .evaluate import load_any_skeleton
    from .util.file import save_cloud, write_ply_points

    cfg = apply_overrides(dict(DEFAULTS), argv if argv is not None else sys.argv[1:])
    unknown = sorted(set(cfg) - set(DEFAULTS))
    out = Path(str(cfg["out"]))
    if unknown or cfg["skeleton"] is None or cfg["out"] is None or out.suffix not in (".npz", ".ply") or str(cfg["form"]) not in FORMS:
        raise SystemExit(USAGE + (f"  (unknown: {', '.join(unknown)})" if unknown else ""))
    skeleton = load_any_skeleton(cfg["skeleton"])
    ring = scanner_ring(int(cfg["scanners"]), float(cfg["radius"]), float(cfg["height"]), skeleton_box(skeleton), float(cfg["step_deg"]),
                        seed=int(cfg["seed"]), range_noise=float(cfg["range_noise"]))
    cloud, extras = scan_skeletons([skeleton], [ring], form=str(cfg["form"]), device=cfg["device"], beams=cfg["beams"] is not None)
    cloud.seg_off = None
    if cfg["beams"] is not None:
        from .occupancy import save_beams
        save_beams(str(cfg["beams"]), extras["origins"], extras["beam_scanner"], extras["beam_dir"], extras["beam_range"])
    out.parent.mkdir(parents=True, exist_ok=True)
    if out.suffix == ".npz":
        save_cloud(out, cloud)
    else:
        write_ply_points(out, cloud.xyz.detach().cpu().numpy(), cloud.rgb.detach().cpu().numpy())
    beams = int(extras["ray_off"][-1])
    print(f"{len(cloud)} points from {beams} beams of {len(ring)} scanner(s) ({100.0 * len(cloud) / max(beams, 1):.1f} % returned) -> {out}")
    return cloud


if __name__ == "__main__":
    main()
