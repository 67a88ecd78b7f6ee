"""Offscreen rendering of clouds and skeletons on the device tensors the pipeline holds (csrc/render.hip).

`python -m smart_tree_amd.render cloud=<.npz|.ply> [skeleton=<.npz>] out=<.png|dir> [views=1] [width=1920] [height=1080]
[colour=rgb|class|radius|branch] [shading=edl|none] [point_px=1] [device=cuda:0]` writes one PNG (`views=1`, `out` a `.png`) or
`view_<k>.png` for a turntable of `views` cameras into the directory `out`.  Overrides are parsed by config.py, as for the
training run.

The reference draws through open3d's headless renderer (`o3d_abstractions/camera.py`); this module keeps its surface -- a
`Renderer(width, height)` whose `capture(items, camera_position, camera_up)` aims at the first item's centre -- over a
rasteriser of the project's own:

* `Camera` / `look_at` are `create_camera` + `update_camera_position` (camera.py:6-35): `cx = w/2 - 0.5`, rows `[right; cam_up; dir]`
  with `right = normalize(dir x up)`, `cam_up = dir x right`, and a translation by `-position`.
* an item is `PointItem(xyz, colour, radius=None)` or `SegmentItem(a, b, r1, r2, colour)`; a colour source is made by `rgb_colour`,
  `class_colour`, `scalar_colour`, `id_colour` or `uniform_colour`.  `cloud_items`, `medial_vector_items` and `skeleton_items` build
  them from a `Cloud` and from a skeleton.
* `Renderer.render(items, cameras)` returns `rgb` uint8 [V,H,W,3], `depth` float32 [V,H,W] and `ids` int32 [V,H,W] as device
  tensors; nothing is read back.  Ids count through the items in the order given; -1 is background.
* `write_png` needs the standard library only.
"""
from __future__ import annotations

import ctypes
import struct
import sys
import zlib
from dataclasses import dataclass
from pathlib import Path
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib

UNIFORM, RGB, CLASS, SCALAR, ID = 0, 1, 2, 3, 4  # ST_RENDER_* of include/smarttree_hip.h
MAX_ITEMS = 16
DEFAULT_CMAP = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0))  # the pipeline's default: branch red, foliage green
EDL_STRENGTH = 2.0


# ------------------------------------------------------------------------------------------------------------ cameras ---
@dataclass
class Camera:
    """A pinhole camera: `p_cam = R p + t`, +z forward; pixel (u, v) has its centre at the integer (u, v)."""
    R: np.ndarray  # [3,3] float64
    t: np.ndarray  # [3]
    fx: float
    fy: float
    cx: float
    cy: float
    width: int
    height: int

    @property
    def extrinsic(self) -> np.ndarray:
        m = np.eye(4)
        m[:3, :3], m[:3, 3] = self.R, self.t
        return m

    def row(self) -> np.ndarray:
        """The 16 float32 the kernels read: R (row-major), t, fx, fy, cx, cy."""
        return np.concatenate([self.R.reshape(-1), self.t, [self.fx, self.fy, self.cx, self.cy]]).astype(np.float32)


def look_at(position, target, up, width: int, height: int, fx: float = 575, fy: float = 575) -> Camera:
    """The reference's `create_camera` + `update_camera_position`."""
    position, target, up = (np.asarray(v, dtype=np.float64).reshape(3) for v in (position, target, up))
    d = target - position
    norm = np.linalg.norm(d)
    if not norm > 0:
        raise ValueError("look_at: the camera sits on its target")
    d = d / norm
    right = np.cross(d, up)
    rn = np.linalg.norm(right)
    if not rn > 1e-12:
        raise ValueError("look_at: `up` is parallel to the viewing direction")
    right = right / rn
    cam_up = np.cross(d, right)
    R = np.vstack((right, cam_up, d))
    return Camera(R, R @ (-position), float(fx), float(fy), width / 2.0 - 0.5, height / 2.0 - 0.5, int(width), int(height))


def camera_rows(cameras, device) -> torch.Tensor:
    """float32 [V,16] on `device`: what the kernels read (`Renderer.render` takes it in place of the Camera objects)."""
    rows = np.stack([c.row() for c in cameras]) if len(cameras) else np.zeros((0, 16), np.float32)
    return torch.from_numpy(rows).to(device)


def _item_points(items):
    """Every item's end points [n,3] and the world radius that goes with them [n] (device tensors)."""
    pts, rad = [], []
    for it in items:
        if isinstance(it, PointItem):
            pts.append(it.xyz)
            rad.append(it.radius if it.radius is not None else torch.zeros(it.xyz.shape[0], device=it.xyz.device))
        else:
            pts += [it.a, it.b]
            rad += [it.r1, it.r2]
    return pts, rad


def bounding_sphere(items):
    """(centre [3], radius) of a sphere around the items: the middle of their box, and the farthest point plus its radius.
    Non-finite points are left out.  One small read-back."""
    sel = []
    for p, r in zip(*_item_points(items)):
        p = p.float().reshape(-1, 3)
        ok = torch.isfinite(p).all(1)
        r = torch.nan_to_num(r.float().reshape(-1).to(p.device)[ok], nan=0.0, posinf=0.0, neginf=0.0).clamp_min(0)
        if bool(ok.any()):
            sel.append((p[ok], r))
    if not sel:
        return np.zeros(3), 1.0
    lo = torch.stack([p.min(0)[0] for p, _ in sel]).min(0)[0]
    hi = torch.stack([p.max(0)[0] for p, _ in sel]).max(0)[0]
    centre = (lo + hi) / 2
    far = max(float(((p - centre).norm(dim=1) + r).max()) for p, r in sel)
    return centre.double().cpu().numpy(), max(far, 1e-6)


def fit(items, direction, width: int, height: int, up=(0, 1, 0), fx: float = 575, fy: float = 575, margin: float = 1.05) -> Camera:
    """A camera looking along `direction` at the centre of the items' bounding sphere, backed off until the sphere fits the view:
    at distance d a sphere of radius r spans asin(r/d), which must stay inside the narrower half-angle of the image."""
    centre, radius = bounding_sphere(items)
    direction = np.asarray(direction, dtype=np.float64).reshape(3)
    direction = direction / np.linalg.norm(direction)
    tan_half = min((width / 2.0 - 1.0) / fx, (height / 2.0 - 1.0) / fy)
    if not tan_half > 0:
        raise ValueError(f"fit: a {width} x {height} image has no room for a view")
    sin_half = tan_half / np.sqrt(1.0 + tan_half * tan_half)
    dist = margin * radius / sin_half
    return look_at(centre - direction * dist, centre, up, width, height, fx, fy)


def turntable(n: int, items, width: int, height: int, up=(0, 1, 0), elevation: float = 0.0, fx: float = 575, fy: float = 575):
    """`n` cameras around the `up` axis through the items' centre, all at the fitting distance; `elevation` (radians) tilts them."""
    up_v = np.asarray(up, dtype=np.float64).reshape(3)
    up_v = up_v / np.linalg.norm(up_v)
    e0 = np.cross(up_v, [1.0, 0.0, 0.0] if abs(up_v[0]) < 0.9 else [0.0, 0.0, 1.0])
    e0 = e0 / np.linalg.norm(e0)
    e1 = np.cross(up_v, e0)
    cams = []
    for k in range(int(n)):
        ang = 2.0 * np.pi * k / int(n)
        out = np.cos(elevation) * (np.cos(ang) * e0 + np.sin(ang) * e1) + np.sin(elevation) * up_v  # from the centre to the camera
        cams.append(fit(items, -out, width, height, up=up, fx=fx, fy=fy))
    return cams


# -------------------------------------------------------------------------------------------------------------- items ---
@dataclass
class ColourSource:
    mode: int
    data: Optional[torch.Tensor] = None
    cmap: Optional[torch.Tensor] = None
    lo: float = 0.0
    hi: float = 1.0
    rgb: Sequence[float] = (0.0, 0.0, 0.0)


def uniform_colour(rgb) -> ColourSource:
    return ColourSource(UNIFORM, rgb=tuple(float(c) for c in rgb))


def rgb_colour(rgb: torch.Tensor) -> ColourSource:
    return ColourSource(RGB, data=rgb.float().reshape(-1, 3).contiguous())


def class_colour(classes: torch.Tensor, cmap=DEFAULT_CMAP) -> ColourSource:
    cm = torch.as_tensor(np.asarray(cmap, dtype=np.float32).reshape(-1, 3)).to(classes.device)
    return ColourSource(CLASS, data=classes.reshape(-1).to(torch.int32).contiguous(), cmap=cm.contiguous())


def scalar_colour(values: torch.Tensor, lo: float, hi: float) -> ColourSource:
    return ColourSource(SCALAR, data=values.float().reshape(-1).contiguous(), lo=float(lo), hi=float(hi))


def id_colour(ids: torch.Tensor) -> ColourSource:
    return ColourSource(ID, data=ids.reshape(-1).to(torch.int32).contiguous())


@dataclass
class PointItem:
    xyz: torch.Tensor  # [n,3]
    colour: ColourSource
    radius: Optional[torch.Tensor] = None  # [n] world radii: discs instead of pixels

    def __len__(self):
        return int(self.xyz.shape[0])


@dataclass
class SegmentItem:
    a: torch.Tensor  # [m,3]
    b: torch.Tensor
    r1: torch.Tensor  # [m]
    r2: torch.Tensor
    colour: ColourSource

    def __len__(self):
        return int(self.a.shape[0])


def cloud_items(cloud, colour: str = "rgb", cmap=DEFAULT_CMAP):
    """The cloud as one PointItem: colour="rgb" (its colours; black without), "class" (`class_l` through `cmap`), "radius"
    (|medial_vector| through the ramp, over its own range: one read-back) or "branch" (`branch_ids` through the hash)."""
    if colour == "rgb":
        src = rgb_colour(cloud.rgb) if cloud.rgb is not None else uniform_colour((0.0, 0.0, 0.0))
    elif colour == "class":
        if cloud.class_l is None:
            raise ValueError("cloud_items: colour='class' needs class_l")
        src = class_colour(cloud.class_l, cmap)
    elif colour == "radius":
        if cloud.medial_vector is None:
            raise ValueError("cloud_items: colour='radius' needs medial_vector")
        r = cloud.radius
        lo, hi = (float(r.min()), float(r.max())) if r.numel() else (0.0, 1.0)
        src = scalar_colour(r, lo, hi if hi > lo else lo + 1.0)
    elif colour == "branch":
        if cloud.branch_ids is None:
            raise ValueError("cloud_items: colour='branch' needs branch_ids")
        src = id_colour(cloud.branch_ids)
    else:
        raise ValueError(f"cloud_items: colour must be rgb, class, radius or branch, got {colour!r}")
    return [PointItem(cloud.xyz, src)]


def medial_vector_items(cloud, colour=(0.0, 0.0, 0.0)):
    """The line from every point to its medial point (the reference's `to_o3d_medial_vectors`), one pixel wide."""
    if cloud.medial_vector is None:
        raise ValueError("medial_vector_items: the cloud has no medial_vector")
    zero = torch.zeros(len(cloud), dtype=torch.float32, device=cloud.xyz.device)
    return [SegmentItem(cloud.xyz, cloud.medial_pts, zero, zero, uniform_colour(colour))]


def skeleton_items(skeleton, device=None):
    """The tubes of a `TreeSkeleton`, a `DisjointTreeSkeleton` or the flat arrays of `save_skeleton_npz` (in `skeleton_tubes`
    order), coloured by branch."""
    from .data_types.flat import FlatSkeletons
    from .evaluation import branch_key

    flat = FlatSkeletons([skeleton], "skeleton_items")
    a, b, r1, r2 = (torch.from_numpy(t) for t in flat.tubes(*flat.float32()))
    ids = np.repeat(branch_key(flat.rows[:, 1], flat.rows[:, 2]), flat.tubes_of_row).astype(np.int32)
    dev = torch.device(device) if device is not None else torch.device("cuda:0")
    f = lambda t: t.to(dev).float().contiguous()
    return [SegmentItem(f(a), f(b), f(r1).reshape(-1), f(r2).reshape(-1), id_colour(torch.from_numpy(ids).to(dev)))]


# ----------------------------------------------------------------------------------------------------------- renderer ---
def _count_matches(src: ColourSource, n: int, what: str) -> None:
    if src.mode != UNIFORM and (src.data is None or src.data.shape[0] != n):
        raise ValueError(f"{what}: the colour source has {None if src.data is None else src.data.shape[0]} entries for {n} ids")


class Renderer:
    """`Renderer(width, height).capture(items, camera_position, camera_up)` as in the reference; `render` for V cameras."""

    def __init__(self, width: int, height: int, fx: float = 575, fy: float = 575, shading: Optional[str] = "edl", point_px: float = 1.0,
                 near: float = 0.01):
        self.width, self.height, self.fx, self.fy = int(width), int(height), float(fx), float(fy)
        self.shading, self.point_px, self.near = shading, float(point_px), float(near)

    def render(self, items, cameras, shading="default", point_px: Optional[float] = None, min_px: float = 1.0, near: Optional[float] = None,
               edl_strength: float = EDL_STRENGTH, edl_px: int = 1, outputs=("rgb", "depth", "ids")) -> dict:
        items = list(items)
        if not torch.is_tensor(cameras):  # a [V,16] tensor of camera rows already on the device saves the upload
            cameras = [cameras] if isinstance(cameras, Camera) else list(cameras)
        shading = self.shading if shading == "default" else shading
        if shading not in (None, "none", "edl"):
            raise ValueError(f"render: shading must be 'edl' or None, got {shading!r}")
        if len(items) > MAX_ITEMS:
            raise ValueError(f"render: at most {MAX_ITEMS} items per frame (got {len(items)})")
        for c in ([] if torch.is_tensor(cameras) else cameras):
            if (c.width, c.height) != (self.width, self.height):
                raise ValueError(f"render: a {c.width} x {c.height} camera on a {self.width} x {self.height} renderer")
        L = _lib.lib()
        dev = (items[0].xyz if isinstance(items[0], PointItem) else items[0].a).device if items else \
            torch.device("cpu" if _lib._ALLOW_HOST_POINTERS else "cuda:0")
        V, H, W = (cameras.numel() // 16 if torch.is_tensor(cameras) else len(cameras)), self.height, self.width
        near = self.near if near is None else float(near)
        cams = cameras.to(dev).float().reshape(-1, 16).contiguous() if torch.is_tensor(cameras) else camera_rows(cameras, dev)
        nbytes = L.st_render_workspace_bytes(V, H, W)
        if nbytes < 0:
            raise _lib.StError(f"render: {V} view(s) of {W} x {H} are outside what the renderer takes")
        ws = _lib.workspace(nbytes, dev)
        stream = _lib.stream(dev)
        p = lambda t: _lib.ptr(t) if t is not None and t.numel() else None
        f = lambda t, shape: t.to(dev).float().reshape(shape).contiguous()
        _lib.check(L.st_render_clear(V, H, W, _lib.ptr(ws), ws.numel(), stream))
        table = (_lib.StRenderItem * max(len(items), 1))()
        keep = [cams, ws]  # tensors the enqueued kernels read
        base = 0
        for k, it in enumerate(items):
            n = len(it)
            src = it.colour
            _count_matches(src, n, f"render: item {k}")
            if isinstance(it, PointItem):
                xyz = f(it.xyz, (-1, 3))
                rad = f(it.radius, (-1,)) if it.radius is not None else None
                if rad is not None and rad.shape[0] != n:
                    raise ValueError(f"render: item {k} has {rad.shape[0]} radii for {n} points")
                keep += [xyz, rad]
                _lib.check(L.st_render_points(p(xyz), p(rad), n, base, self.point_px if point_px is None else float(point_px),
                                              _lib.ptr(cams), V, H, W, near, _lib.ptr(ws), ws.numel(), stream))
            elif isinstance(it, SegmentItem):
                a, b, r1, r2 = f(it.a, (-1, 3)), f(it.b, (-1, 3)), f(it.r1, (-1,)), f(it.r2, (-1,))
                if not (b.shape[0] == r1.shape[0] == r2.shape[0] == n):
                    raise ValueError(f"render: item {k}: a, b, r1 and r2 differ in length")
                keep += [a, b, r1, r2]
                _lib.check(L.st_render_segments(p(a), p(b), p(r1), p(r2), n, base, float(min_px), _lib.ptr(cams), V, H, W, near,
                                                _lib.ptr(ws), ws.numel(), stream))
            else:
                raise TypeError(f"render: item {k} is a {type(it).__name__}, not a PointItem or a SegmentItem")
            data = src.data.to(dev).contiguous() if src.data is not None else None
            cmap = src.cmap.to(dev).float().contiguous() if src.cmap is not None else None
            keep += [data, cmap]
            e = table[k]
            e.count, e.mode = n, src.mode
            e.n_classes = int(cmap.shape[0]) if cmap is not None else 0
            e.data, e.cmap = p(data), p(cmap)
            e.lo, e.hi = src.lo, src.hi
            e.rgb[0], e.rgb[1], e.rgb[2] = (float(c) for c in src.rgb)
            base += n
        out = {"rgb": torch.empty((V, H, W, 3), dtype=torch.uint8, device=dev) if "rgb" in outputs else None,
               "depth": torch.empty((V, H, W), dtype=torch.float32, device=dev) if "depth" in outputs else None,
               "ids": torch.empty((V, H, W), dtype=torch.int32, device=dev) if "ids" in outputs else None}
        _lib.check(L.st_render_resolve(ctypes.cast(table, ctypes.c_void_p), len(items), V, H, W,
                                       float(edl_strength) if shading == "edl" else 0.0, int(edl_px), p(out["rgb"]), p(out["depth"]),
                                       p(out["ids"]), _lib.ptr(ws), ws.numel(), stream))
        del keep  # freed blocks go back to the caching allocator, which hands them only to work enqueued LATER on this stream
        return {k: v for k, v in out.items() if v is not None}

    def camera(self, items, camera_position, camera_up) -> Camera:
        """The reference's aim: the target is the mean of the first item's points, the camera sits at target + camera_position."""
        items = list(items)
        first = items[0].xyz if isinstance(items[0], PointItem) else torch.cat([items[0].a, items[0].b])
        first = first[torch.isfinite(first).all(1)]  # an untrained network's medial points overflow
        if first.shape[0] == 0:
            raise ValueError("capture: the first item has no finite point, there is nothing to aim at")
        target = first.double().mean(0).cpu().numpy()
        return look_at(target + np.asarray(camera_position, dtype=np.float64), target, camera_up, self.width, self.height, self.fx, self.fy)

    def capture(self, items, camera_position, camera_up) -> np.ndarray:
        """uint8 [H,W,3] on the host (the reference returns an open3d image the caller turns into an array)."""
        items = list(items)
        out = self.render(items, [self.camera(items, camera_position, camera_up)], outputs=("rgb",))
        return out["rgb"][0].cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------- png ---
def write_png(path, image) -> None:
    """uint8 [H,W,3] (or [H,W]: grey) as an 8-bit PNG: signature, IHDR, one zlib stream of filter-0 rows in IDAT, IEND."""
    if torch.is_tensor(image):
        image = image.detach().cpu().numpy()
    image = np.ascontiguousarray(image)
    if image.dtype != np.uint8 or image.ndim not in (2, 3) or (image.ndim == 3 and image.shape[2] != 3) or 0 in image.shape:
        raise ValueError(f"write_png: a non-empty uint8 [H,W,3] or [H,W] image, got {image.dtype} {image.shape}")
    h, w = image.shape[:2]
    rows = np.zeros((h, 1 + w * (3 if image.ndim == 3 else 1)), dtype=np.uint8)  # a leading 0 per row: filter type None
    rows[:, 1:] = image.reshape(h, -1)

    def chunk(kind: bytes, body: bytes) -> bytes:
        return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xFFFFFFFF)

    data = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2 if image.ndim == 3 else 0, 0, 0, 0)) + \
        chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)) + chunk(b"IEND", b"")
    path = Path(path)
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_bytes(data)


# ---------------------------------------------------------------------------------------------------------------- cli ---
DEFAULTS = {"cloud": None, "skeleton": None, "out": None, "views": 1, "width": 1920, "height": 1080, "colour": "rgb", "shading": "edl",
            "point_px": 1, "device": "cuda:0"}


def main(argv=None) -> list:
    from .config import apply_overrides
    from .evaluate import load_any_skeleton
    from .util.file import load_cloud

    cfg = apply_overrides(dict(DEFAULTS), argv if argv is not None else sys.argv[1:])
    unknown = sorted(set(cfg) - set(DEFAULTS))
    if unknown or cfg["cloud"] is None or cfg["out"] is None:
        raise SystemExit("usage: python -m smart_tree_amd.render cloud=<.npz|.ply> [skeleton=<.npz>] out=<.png|dir> [views=1] [width=1920] "
                         "[height=1080] [colour=rgb|class|radius|branch] [shading=edl|none] [point_px=1] [device=]"
                         + (f"  (unknown: {', '.join(unknown)})" if unknown else ""))
    dev = torch.device(cfg["device"])
    views, out = int(cfg["views"]), Path(str(cfg["out"]))
    if views < 1:
        raise SystemExit("render: views must be at least 1")
    if views > 1 and out.suffix == ".png":
        raise SystemExit(f"render: {views} views need a directory for out=, not {out}")
    cloud = load_cloud(cfg["cloud"]).to_device(dev)
    items = cloud_items(cloud, colour=str(cfg["colour"]))
    if cfg["skeleton"] is not None:
        items += skeleton_items(load_any_skeleton(cfg["skeleton"]), device=dev)
    r = Renderer(int(cfg["width"]), int(cfg["height"]), shading=None if str(cfg["shading"]).lower() in ("none", "false", "off") else
                 str(cfg["shading"]), point_px=float(cfg["point_px"]))
    cams = turntable(views, items, r.width, r.height, elevation=0.3 if views > 1 else 0.0)
    rgb = r.render(items, cams, outputs=("rgb",))["rgb"].cpu().numpy()
    paths = [out] if out.suffix == ".png" else [out / f"view_{k}.png" for k in range(views)]
    for path, img in zip(paths, rgb):
        write_png(path, img)
        print(path)
    return paths


if __name__ == "__main__":
    main()
