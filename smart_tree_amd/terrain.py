"""Terrain: a ground raster under a cloud, which points are ground, and every point's height above it (csrc/ground.hip).

`python -m smart_tree_amd.terrain cloud=<.npz|.ply> out=<dir> [cell=0.5] [max_window=8] [slope=0.3] [initial_distance=0.15]
[max_distance=2.5] [ground_tolerance=0.2] [up=1] [normalise=false] [device=cuda:0]` writes `ground.npz`, `dtm.asc` and
`cloud_no_ground.npz` (the cloud without its ground points; with `normalise=true` its up-coordinate is the height above ground) and
prints the summary.  Overrides are parsed by config.py.

The reference's clouds hold trees only; a plot scan is half ground.  `ground_model` is a progressive morphological filter (Zhang et
al. 2003) on a raster of per-cell minima of the up-coordinate: windows of doubling half-width open the raster (a minimum, then a
maximum over the window), and a cell that stands more than the window's threshold above its opening is not ground and takes the
opening's value.  Three HIP calls (`st_ground_extent`, `st_ground_model`, `st_ground_height`; include/smarttree_hip.h states the
arithmetic), one read-back (the rasters' dimensions).  The rasters, the flags and `is_ground` are the same bits in every run, for a
batch and for its clouds alone.

Known limits: the cell minimum lies below the terrain by about slope x cell / 2 on a slope; an object wider than 2 x max_window
survives as ground; an overhang beyond the scanned ground cannot be resolved (there is no data under it); a hill top is cut by the
opening within the slope term of the thresholds.
"""
from __future__ import annotations

import sys
from dataclasses import dataclass, field
from pathlib import Path

import numpy as np
import torch

from . import _lib
from .data_types.cloud import Cloud

MAX_HALF_WIDTH = 32   # cells: the largest window of st_ground_model
MAX_SIDE = 16384      # cells per side of one raster
MAX_CELLS = 1 << 26   # cells per call
NODATA = -9999.0


def windows(cell, max_window=8.0, slope=0.3, initial_distance=0.15, max_distance=2.5):
    """(half-widths int32 [K] in cells, thresholds float32 [K]): 1, 2, 4, ... up to max(1, round(max_window / cell)) -- that last
    half-width closes the list when it is no power of two -- and dh[k] = min(max_distance, initial_distance + slope (w[k] - w[k-1])
    cell) with w[-1] = 0, in float64, rounded once."""
    if not (np.isfinite(cell) and cell > 0):
        raise ValueError(f"ground_model: the cell size must be finite and > 0 (got {cell})")
    if not (np.isfinite(max_window) and max_window >= 0) or max_window / cell > MAX_HALF_WIDTH:
        raise ValueError(f"ground_model: max_window / cell = {max_window / cell:g} is outside [0, {MAX_HALF_WIDTH}]: choose a larger cell "
                         f"(at least {max_window / MAX_HALF_WIDTH:g}) or a smaller max_window")
    last = max(1, int(round(max_window / cell)))
    w = [1]
    while w[-1] * 2 <= last:
        w.append(w[-1] * 2)
    if w[-1] < last:
        w.append(last)
    w = np.asarray(w, np.int64)
    dh = np.minimum(float(max_distance), float(initial_distance) + float(slope) * np.diff(w, prepend=0).astype(np.float64) * float(cell))
    return w.astype(np.int32), dh.astype(np.float32)


def _points(cloud, device):
    if isinstance(cloud, Cloud):
        xyz, seg_off = cloud.xyz, cloud.seg_off
    else:
        xyz, seg_off = (cloud if torch.is_tensor(cloud) else torch.tensor(np.asarray(cloud, np.float32))), None
    dev = torch.device(device) if device is not None else xyz.device
    pts = xyz.to(dev).float().reshape(-1, 3).contiguous()
    if seg_off is not None:
        seg_off = seg_off.to(dev).to(torch.int32).reshape(-1).contiguous()
        if seg_off.shape[0] < 2:
            raise ValueError("ground_model: seg_off holds no cloud")
    return pts, seg_off, dev


def _host_ptr(a: np.ndarray):
    return a.ctypes.data


def ground_extent(pts, seg_off=None, cell=0.5, up=1):
    """`st_ground_extent` on device tensors: (origin float32 [S,2], dims int32 [S,2]), both on the device."""
    L = _lib.lib()
    dev = pts.device
    S = 1 if seg_off is None else seg_off.shape[0] - 1
    origin = torch.empty((S, 2), dtype=torch.float32, device=dev)
    dims = torch.empty((S, 2), dtype=torch.int32, device=dev)
    ws = _lib.workspace(L.st_ground_workspace_bytes(0), dev)
    _lib.check(L.st_ground_extent(_lib.ptr(pts) if pts.numel() else None, pts.shape[0], _lib.ptr(seg_off), S, int(up), float(cell),
                                  _lib.ptr(origin), _lib.ptr(dims), _lib.ptr(ws), ws.numel(), _lib.stream(dev)))
    return origin, dims


def ground_raster(pts, seg_off, origin, dims, cell_off, w, dh, cell=0.5, up=1):
    """`st_ground_model` on device tensors with the host arrays dims int32 [S,2], cell_off int64 [S+1], w int32 [K], dh float32 [K]:
    (surface float32 [cells], flags uint8 [cells]) on the device."""
    L = _lib.lib()
    dev = pts.device
    dims, cell_off = np.ascontiguousarray(dims, np.int32), np.ascontiguousarray(cell_off, np.int64)
    w, dh = np.ascontiguousarray(w, np.int32), np.ascontiguousarray(dh, np.float32)
    if len(w) != len(dh):
        raise ValueError(f"ground_model: {len(w)} windows with {len(dh)} thresholds")
    S, cells = dims.shape[0], int(cell_off[-1])
    nbytes = L.st_ground_workspace_bytes(cells)
    if nbytes < 0:
        raise _lib.StError(f"ground_model: {cells} cells are more than a call takes (2^26): choose a larger cell")
    surface = torch.empty(max(cells, 0), dtype=torch.float32, device=dev)
    flags = torch.empty(max(cells, 0), dtype=torch.uint8, device=dev)
    ws = _lib.workspace(nbytes, dev)
    p = lambda t: _lib.ptr(t) if t is not None and t.numel() else None
    _lib.check(L.st_ground_model(p(pts), pts.shape[0], _lib.ptr(seg_off), S, int(up), float(cell), _lib.ptr(origin), _host_ptr(dims),
                                 _host_ptr(cell_off), len(w), _host_ptr(w), _host_ptr(dh), p(surface), p(flags), _lib.ptr(ws), ws.numel(),
                                 _lib.stream(dev)))
    return surface, flags


def ground_height(pts, seg_off, origin, dims, cell_off, surface, cell=0.5, up=1, tolerance=0.2):
    """`st_ground_height` on device tensors: (height float32 [m], is_ground uint8 [m], ground float32 [m]) on the device."""
    L = _lib.lib()
    dev = pts.device
    dims, cell_off = np.ascontiguousarray(dims, np.int32), np.ascontiguousarray(cell_off, np.int64)
    m = pts.shape[0]
    height = torch.empty(m, dtype=torch.float32, device=dev)
    is_ground = torch.empty(m, dtype=torch.uint8, device=dev)
    ground = torch.empty(m, dtype=torch.float32, device=dev)
    p = lambda t: _lib.ptr(t) if t is not None and t.numel() else None
    _lib.check(L.st_ground_height(p(pts), m, _lib.ptr(seg_off), dims.shape[0], int(up), float(cell), float(tolerance), _lib.ptr(origin),
                                  _host_ptr(dims), _host_ptr(cell_off), p(surface), p(height), p(is_ground), p(ground), _lib.stream(dev)))
    return height, is_ground, ground


@dataclass
class GroundModel:
    """`surface` float32 [cells] and `flags` uint8 [cells] (bit 0: no point in the cell, bit 1: not ground) on the device, the
    rasters of the clouds one behind the other: cloud k owns [cell_off[k], cell_off[k+1]) as a [dims[k,0], dims[k,1]] array over the
    plan axes a < b (the two that are not `up`), whose cell (0, 0) begins at `origin[k]`.  `origin` float32 [S,2] on the device;
    `dims` int32 [S,2] and `cell_off` int64 [S+1] on the host.  Per point of the cloud the model was made from: `is_ground` bool [n]
    and `height` float32 [n] above the blended surface (NaN where there is no terrain in reach); None after `load`."""
    surface: torch.Tensor
    flags: torch.Tensor
    origin: torch.Tensor
    dims: np.ndarray
    cell_off: np.ndarray
    cell: float
    up: int = 1
    is_ground: torch.Tensor = None
    height: torch.Tensor = None
    seg_off: torch.Tensor = None
    ground_tolerance: float = 0.2
    params: dict = field(default_factory=dict)

    @property
    def n_clouds(self) -> int:
        return int(self.dims.shape[0])

    def raster(self, cloud=0):
        """(surface [A,B], flags [A,B]) of one cloud: views."""
        a, b = int(self.cell_off[cloud]), int(self.cell_off[cloud + 1])
        shape = tuple(int(v) for v in self.dims[cloud])
        return self.surface[a:b].view(shape), self.flags[a:b].view(shape)

    def _query(self, xyz, cloud):
        if not 0 <= int(cloud) < self.n_clouds:
            raise ValueError(f"GroundModel: cloud {cloud} of {self.n_clouds}")
        dev = self.surface.device
        pts = (xyz if torch.is_tensor(xyz) else torch.tensor(np.asarray(xyz, np.float32))).to(dev).float().reshape(-1, 3).contiguous()
        a, b = int(self.cell_off[cloud]), int(self.cell_off[cloud + 1])
        return ground_height(pts, None, self.origin[cloud:cloud + 1].contiguous(), self.dims[cloud:cloud + 1], np.asarray([0, b - a], np.int64),
                             self.surface[a:b], self.cell, self.up, self.ground_tolerance)

    def height_at(self, xyz, cloud=0) -> torch.Tensor:
        """Height above ground of any positions [m,3] in the frame of `cloud`: float32 [m], NaN where there is no terrain."""
        return self._query(xyz, cloud)[0]

    def surface_at(self, xyz, cloud=0) -> torch.Tensor:
        """The terrain's up-coordinate under any positions [m,3]: float32 [m], NaN where there is no terrain."""
        return self._query(xyz, cloud)[2]

    def split(self) -> list:
        """The clouds of a batch, each as its own call gives it."""
        if self.n_clouds == 1:
            return [self]
        off = self.seg_off.tolist() if self.seg_off is not None and self.is_ground is not None else None
        out = []
        for k in range(self.n_clouds):
            a, b = int(self.cell_off[k]), int(self.cell_off[k + 1])
            pt = slice(off[k], off[k + 1]) if off is not None else None
            out.append(GroundModel(self.surface[a:b], self.flags[a:b], self.origin[k:k + 1], self.dims[k:k + 1].copy(), np.asarray([0, b - a], np.int64),
                                   self.cell, self.up, None if pt is None else self.is_ground[pt], None if pt is None else self.height[pt],
                                   None, self.ground_tolerance, dict(self.params)))
        return out

    def save(self, directory) -> None:
        """`ground.npz` (rasters, origin, dims, cell offsets, cell size, parameters) and one ESRI ASCII grid per cloud: `dtm.asc`, or
        `dtm_<k>.asc` for the clouds of a batch; columns run along a, rows along b from the far side down, NODATA_value where the
        surface is +inf."""
        directory = Path(directory)
        directory.mkdir(parents=True, exist_ok=True)
        np.savez(directory / "ground.npz", surface=self.surface.cpu().numpy(), flags=self.flags.cpu().numpy(), origin=self.origin.cpu().numpy(),
                 dims=self.dims, cell_off=self.cell_off, cell=np.float64(self.cell), up=np.int64(self.up),
                 ground_tolerance=np.float64(self.ground_tolerance), **{f"param_{k}": np.asarray(v) for k, v in self.params.items()})
        origin = self.origin.cpu().numpy()
        for k in range(self.n_clouds):
            name = "dtm.asc" if self.n_clouds == 1 else f"dtm_{k}.asc"
            grid = self.raster(k)[0].cpu().numpy()
            write_asc(directory / name, grid, origin[k], self.cell)

    @staticmethod
    def load(path, device="cpu") -> "GroundModel":
        """From `ground.npz` or the directory that holds it; the per-point fields are not stored."""
        path = Path(path)
        dev = torch.device(device)
        with np.load(path / "ground.npz" if path.is_dir() else path) as z:
            params = {k[len("param_"):]: (z[k].item() if z[k].ndim == 0 else z[k]) for k in z.files if k.startswith("param_")}
            return GroundModel(torch.from_numpy(z["surface"]).to(dev), torch.from_numpy(z["flags"]).to(dev), torch.from_numpy(z["origin"]).to(dev),
                               z["dims"].astype(np.int32), z["cell_off"].astype(np.int64), float(z["cell"]), int(z["up"]),
                               ground_tolerance=float(z["ground_tolerance"]), params=params)

    def summary(self) -> str:
        """One line per cloud."""
        lines = []
        off = self.seg_off.tolist() if self.seg_off is not None else None
        for k in range(self.n_clouds):
            surface, flags = (t.cpu().numpy() for t in self.raster(k))
            A, B = surface.shape
            known = np.isfinite(surface)
            line = (f"cloud {k}: {A} x {B} cells of {self.cell:g} m, {int((flags & 1).sum())} without points, {int((flags & 2).sum() // 2)} not ground, "
                    f"{int((~known).sum())} without terrain")
            if known.any():
                line += f", terrain {surface[known].min():.2f} to {surface[known].max():.2f} m"
            if self.is_ground is not None:
                pt = slice(off[k], off[k + 1]) if off is not None else slice(None)
                g, h = self.is_ground[pt], self.height[pt]
                n = int(g.shape[0])
                above = h[~g & ~torch.isnan(h)]
                line += f"; {int(g.sum())} of {n} points are ground"
                if above.numel():
                    line += f", the others reach {float(above.max()):.2f} m above it"
            lines.append(line)
        return "\n".join(lines)


def write_asc(path, grid, origin, cell) -> None:
    """An [A,B] raster as an ESRI ASCII grid: ncols = A along the first plan axis, nrows = B along the second, top row first."""
    A, B = grid.shape
    rows = np.where(np.isfinite(grid), grid, np.float32(NODATA)).T[::-1]
    head = [f"ncols {A}", f"nrows {B}", f"xllcorner {float(origin[0])!r}", f"yllcorner {float(origin[1])!r}", f"cellsize {float(cell)!r}",
            f"NODATA_value {NODATA:g}"]
    body = [" ".join(format(float(v), ".9g") for v in row) for row in rows]
    Path(path).write_text("\n".join(head + body) + "\n")


def read_asc(path):
    """(grid float32 [A,B] with +inf for NODATA, origin (a0, b0), cell) of a grid `write_asc` wrote."""
    lines = Path(path).read_text().splitlines()
    head = {k.lower(): v for k, v in (line.split() for line in lines[:6])}
    A, B, nodata = int(head["ncols"]), int(head["nrows"]), float(head["nodata_value"])
    rows = np.asarray([[float(v) for v in line.split()] for line in lines[6:6 + B]], np.float64).reshape(B, A)
    grid = np.where(rows == nodata, np.inf, rows).astype(np.float32)[::-1].T
    return np.ascontiguousarray(grid), (float(head["xllcorner"]), float(head["yllcorner"])), float(head["cellsize"])


def ground_model(cloud, cell=0.5, max_window=8.0, slope=0.3, initial_distance=0.15, max_distance=2.5, ground_tolerance=0.2, up=1,
                 device=None) -> GroundModel:
    """The terrain under `cloud` -- a `Cloud` (one, or a collated batch with `seg_off`: one raster per cloud, one set of calls) or
    [n,3] points.  `cell`: the raster's cell in metres; `max_window`: the half-width in metres of the largest window, more than
    half the width of the widest object to remove; `slope`, `initial_distance`, `max_distance`: the thresholds (`windows`);
    `ground_tolerance`: a point at most this far above its cell's surface is ground; `up`: the vertical axis."""
    if up not in (0, 1, 2):
        raise ValueError(f"ground_model: up is 0, 1 or 2 (got {up})")
    w, dh = windows(cell, max_window, slope, initial_distance, max_distance)
    if not np.isfinite(ground_tolerance):
        raise ValueError(f"ground_model: ground_tolerance must be finite (got {ground_tolerance})")
    pts, seg_off, dev = _points(cloud, device)
    if seg_off is not None and seg_off.shape[0] - 1 > _lib.lib().st_abi_entries(2):
        raise ValueError(f"ground_model: a call takes at most {_lib.lib().st_abi_entries(2)} clouds (got {seg_off.shape[0] - 1})")
    origin, dims_dev = ground_extent(pts, seg_off, cell, up)
    dims = dims_dev.cpu().numpy()  # the one read-back
    cells = dims[:, 0].astype(np.int64) * dims[:, 1].astype(np.int64)
    if dims.max(initial=0) > MAX_SIDE or cells.sum() > MAX_CELLS:
        raise ValueError(f"ground_model: rasters of {', '.join(f'{a} x {b}' for a, b in dims.tolist())} cells; a side takes at most {MAX_SIDE} and "
                         f"a call 2^26 cells: choose a larger cell than {cell:g}")
    cell_off = np.concatenate([[0], np.cumsum(cells)]).astype(np.int64)
    surface, flags = ground_raster(pts, seg_off, origin, dims, cell_off, w, dh, cell, up)
    height, is_ground, _ = ground_height(pts, seg_off, origin, dims, cell_off, surface, cell, up, ground_tolerance)
    params = {"max_window": float(max_window), "slope": float(slope), "initial_distance": float(initial_distance), "max_distance": float(max_distance),
              "windows": w, "thresholds": dh}
    return GroundModel(surface, flags, origin, dims, cell_off, float(cell), int(up), is_ground.bool(), height, seg_off, float(ground_tolerance), params)


# ---------------------------------------------------------------------------------------------------------------- cli ---
DEFAULTS = {"cloud": None, "out": None, "cell": 0.5, "max_window": 8.0, "slope": 0.3, "initial_distance": 0.15, "max_distance": 2.5,
            "ground_tolerance": 0.2, "up": 1, "normalise": False, "device": "cuda:0"}


def main(argv=None) -> GroundModel:
    from .config import apply_overrides
    from .util.file import load_cloud, save_cloud

    cfg = apply_overrides(dict(DEFAULTS), argv if argv is not None else sys.argv[1:])
    unknown = sorted(set(cfg) - set(DEFAULTS))
    if unknown or cfg["cloud"] is None or cfg["out"] is None:
        raise SystemExit("usage: python -m smart_tree_amd.terrain cloud=<.npz|.ply> out=<dir> [cell=0.5] [max_window=8] [slope=0.3] "
                         "[initial_distance=0.15] [max_distance=2.5] [ground_tolerance=0.2] [up=1] [normalise=false] [device=]"
                         + (f"  (unknown: {', '.join(unknown)})" if unknown else ""))
    dev = torch.device(cfg["device"])
    cloud = load_cloud(cfg["cloud"]).to_device(dev)
    model = ground_model(cloud, cell=float(cfg["cell"]), max_window=float(cfg["max_window"]), slope=float(cfg["slope"]),
                         initial_distance=float(cfg["initial_distance"]), max_distance=float(cfg["max_distance"]),
                         ground_tolerance=float(cfg["ground_tolerance"]), up=int(cfg["up"]), device=dev)
    out = Path(str(cfg["out"]))
    model.save(out)
    if str(cfg["normalise"]).lower() in ("true", "1", "yes", "on"):
        xyz = cloud.xyz.clone()
        xyz[:, model.up] = model.height
        cloud = cloud._map(lambda t: t)
        cloud.xyz = xyz
    save_cloud(out / "cloud_no_ground.npz", cloud.filter(~model.is_ground))
    print(model.summary())
    return model


if __name__ == "__main__":
    main()
