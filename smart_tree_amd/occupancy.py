"""Beam occupancy: what a scan saw, what it could not see, and plant area per voxel (csrc/occupancy.hip).

`python -m smart_tree_amd.occupancy beams=<beams.npz> out=<dir|.npz> [cell=0.1] [margin=0.2] [max_range=inf] [behind=true] [G=0.5]
[device=cuda:0]` walks the beams of a scan (`python -m smart_tree_amd.scan ... beams=<beams.npz>` writes them: `origins`,
`origin_idx`, `dir`, `range`, +inf where nothing came back) through a voxel grid around the returns and writes `occupancy.npz`:
the grid, the four tallies, the state of every cell and its plant-area density.  Overrides are parsed by config.py.

Per cell: `enter`, the beams that entered it while free; `hit`, the returns that ended in it; `behind`, the returns that ended
before it and would have passed; `path`, the free path spent in it in units of cell / 65536.  A cell no free beam entered but
some stopped beam would have is occluded: the scan says nothing about it, which is not the same as empty.  hit / path is the
Beer-Lambert contact frequency (1/m); divided by the projection function G it is the plant-area density (m^2 / m^3).  Not
modelled: beam divergence, partial and multiple returns, a G that varies with the beam's direction.
"""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass
from pathlib import Path
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib

FORMS = {"auto": 0, "aggregated": 1, "plain": 2}
MAX_GRIDS = 64
MAX_DIM = 1024
PATH_UNITS = 65536.0
STATES = ("unseen", "empty", "occupied", "occluded")


@dataclass
class VoxelGrid:
    """Cells of `cell` metres from corner `lo`, `dim` = (nx, ny, nz) of them; cell (x, y, z) covers lo + (x, y, z) cell .. + cell.
    The numbers are kept as float32, as the kernel reads them."""
    lo: Sequence[float]
    cell: float
    dim: Sequence[int]

    def __post_init__(self):
        lo = np.asarray(self.lo, dtype=np.float32).reshape(-1)
        dim = [int(d) for d in np.asarray(self.dim).reshape(-1)]
        cell = float(np.float32(self.cell))
        if len(lo) != 3 or len(dim) != 3 or not np.isfinite(lo).all() or not (math.isfinite(cell) and cell > 0):
            raise ValueError(f"VoxelGrid: a finite corner of 3 numbers and a finite cell > 0 (got lo={self.lo}, cell={self.cell})")
        if not all(1 <= d <= MAX_DIM for d in dim):
            raise ValueError(f"VoxelGrid: 1 .. {MAX_DIM} cells per axis (got {dim})")
        self.lo, self.cell, self.dim = tuple(float(v) for v in lo), cell, tuple(dim)

    @property
    def n_cells(self) -> int:
        return self.dim[0] * self.dim[1] * self.dim[2]

    @property
    def hi(self) -> tuple:
        """The far corner as the kernel forms it: lo + (float32)dim * cell."""
        return tuple(float(np.float32(l) + np.float32(d) * np.float32(self.cell)) for l, d in zip(self.lo, self.dim))

    @staticmethod
    def around(points, cell: float, margin: float = 0.0) -> "VoxelGrid":
        """The grid of `cell` metres that covers the finite points [N,3] and `margin` metres around them."""
        p = points.detach().cpu().numpy() if torch.is_tensor(points) else np.asarray(points)
        p = p.reshape(-1, 3).astype(np.float64)
        p = p[np.isfinite(p).all(1)]
        if len(p) == 0:
            raise ValueError("VoxelGrid.around: no finite point")
        lo, hi = p.min(0) - margin, p.max(0) + margin
        dim = np.floor((hi - lo) / cell).astype(np.int64) + 1
        if (dim > MAX_DIM).any():
            raise ValueError(f"VoxelGrid.around: {dim.tolist()} cells of {cell} m (at most {MAX_DIM} per axis); use a larger cell")
        return VoxelGrid(lo, cell, dim)

    def cell_of(self, xyz: torch.Tensor):
        """(index [N] int64 of the cell under each point, inside [N] bool): the kernel's first-cell rule, clamped; `inside` is false
        for a point outside the grid's box or not finite."""
        lo = torch.tensor(self.lo, dtype=torch.float32, device=xyz.device)
        hi = torch.tensor(self.hi, dtype=torch.float32, device=xyz.device)
        dim = torch.tensor(self.dim, dtype=torch.float32, device=xyz.device)
        p = xyz.float().reshape(-1, 3)
        inside = ((p >= lo) & (p <= hi)).all(1)
        c = torch.floor((p - lo) / self.cell)
        c = torch.minimum(torch.clamp(torch.nan_to_num(c, nan=0.0), min=0.0), dim - 1).long()
        return (c[:, 0] * self.dim[1] + c[:, 1]) * self.dim[2] + c[:, 2], inside


class BeamTally:
    """The tallies of one grid of a `beam_tally` call: device tensors `enter`, `hit`, `behind` (int64 views of the kernel's
    uint32, shaped `dim`) and `path` (int64, units of cell / 65536); `hit_cell` [beams of this grid] int32 when asked for.
    `n_bad` and `n_outside` are the call's counters (all grids), read back once."""

    def __init__(self, grid: VoxelGrid, enter, hit, behind, path, hit_cell, n_bad: int, n_outside: int):
        self.grid, self.enter, self.hit, self.behind, self.path, self.hit_cell = grid, enter, hit, behind, path, hit_cell
        self.n_bad, self.n_outside = int(n_bad), int(n_outside)

    def state(self) -> torch.Tensor:
        """uint8 per cell: 0 unseen, 1 empty (entered, no hit), 2 occupied (a hit), 3 occluded (never entered, some beam was
        stopped before it)."""
        s = torch.zeros_like(self.enter, dtype=torch.uint8)
        s[(self.enter > 0) & (self.hit == 0)] = 1
        s[self.hit > 0] = 2
        s[(self.enter == 0) & (self.hit == 0) & (self.behind > 0)] = 3
        return s

    def path_length(self) -> torch.Tensor:
        """Free path per cell in metres (float64)."""
        return self.path.double() / PATH_UNITS * self.grid.cell

    def attenuation(self, min_beams: int = 1) -> torch.Tensor:
        """Contact frequency hit / path length in 1/m (float64); NaN where fewer than `min_beams` free beams entered or no free
        path was spent."""
        length = self.path_length()
        ok = (self.enter >= int(min_beams)) & (length > 0)
        nan = torch.full_like(length, float("nan"))
        return torch.where(ok, self.hit.double() / torch.where(ok, length, torch.ones_like(length)), nan)

    def plant_area_density(self, G: float = 0.5, min_beams: int = 1) -> torch.Tensor:
        """attenuation / G in m^2 of plant area per m^3 (G: the mean projection of a unit of area onto the plane across the beam;
        0.5 for a spherical distribution of orientations)."""
        return self.attenuation(min_beams) / float(G)

    def plant_area_cells(self, G: float = 0.5, min_beams: int = 1) -> torch.Tensor:
        """Plant area per cell in m^2; 0 where the density is not known."""
        return torch.nan_to_num(self.plant_area_density(G, min_beams), nan=0.0) * self.grid.cell ** 3

    def plant_area(self, G: float = 0.5, min_beams: int = 1) -> float:
        """The grid's plant area in m^2: density times cell volume over the cells where the density is known."""
        return float(self.plant_area_cells(G, min_beams).sum())

    def plant_area_by_label(self, hit_cell, labels, n_labels: int, G: float = 0.5, min_beams: int = 1) -> torch.Tensor:
        """[n_labels] float64 m^2: every cell's plant area shared among the labels in proportion to its labelled returns.
        `hit_cell` [R] (the call's, -1 where a beam has none) and `labels` [R] (0 .. n_labels - 1, anything else: unlabelled) are
        per beam.  With `segment_cloud`'s tree column as the label of a return this is the leaf (plant) area per tree; the area
        of a cell none of whose returns is labelled is left out."""
        hit_cell, labels = hit_cell.reshape(-1).long(), labels.reshape(-1).long().to(hit_cell.device)
        if hit_cell.shape != labels.shape:
            raise ValueError(f"plant_area_by_label: {hit_cell.shape[0]} hit cells and {labels.shape[0]} labels")
        n, n_labels = self.grid.n_cells, int(n_labels)
        ok = (hit_cell >= 0) & (hit_cell < n) & (labels >= 0) & (labels < n_labels)
        key = hit_cell[ok] * n_labels + labels[ok]
        per = torch.bincount(key, minlength=n * n_labels).view(n, n_labels).double()
        total = per.sum(1, keepdim=True)
        share = torch.where(total > 0, per / torch.where(total > 0, total, torch.ones_like(total)), torch.zeros_like(per))
        return (share * self.plant_area_cells(G, min_beams).reshape(-1, 1)).sum(0)


def _dev_f32(t, dev, shape):
    t = torch.as_tensor(t) if not torch.is_tensor(t) else t
    return t.to(dev).float().reshape(shape).contiguous()


def beam_tally(origins, origin_idx, dir, range, grids, beam_off=None, max_range=math.inf, behind=True, form="auto", hit_cell=False):
    """`st_beam_tally_seg` on device tensors: `origins` [S,3]; per beam `origin_idx` [R], `dir` [R,3] (unit), `range` [R] (+inf: no
    return).  `grids`: one `VoxelGrid` or up to 64 of them with `beam_off` [G+1], the first beam of every grid.  Returns a
    `BeamTally` (a list of them for a list of grids) after the call's one read-back of its two counters."""
    single = isinstance(grids, VoxelGrid)
    grids = [grids] if single else list(grids)
    L = _lib.lib()
    dev = origins.device if torch.is_tensor(origins) else torch.device("cpu")
    origins = _dev_f32(origins, dev, (-1, 3))
    dir, range = _dev_f32(dir, dev, (-1, 3)), _dev_f32(range, dev, (-1,))
    origin_idx = torch.as_tensor(origin_idx).to(dev).to(torch.int32).reshape(-1).contiguous()
    R, S, G = range.shape[0], origins.shape[0], len(grids)
    if dir.shape[0] != R or origin_idx.shape[0] != R:
        raise ValueError(f"beam_tally: {R} ranges, {dir.shape[0]} directions, {origin_idx.shape[0]} origin indices")
    if not 1 <= G <= MAX_GRIDS:
        raise ValueError(f"beam_tally: 1 .. {MAX_GRIDS} grids per call (got {G})")
    if beam_off is None:
        if G != 1:
            raise ValueError("beam_tally: several grids need beam_off")
        beam_off = [0, R]
    beam_off = np.ascontiguousarray(np.asarray(beam_off.cpu() if torch.is_tensor(beam_off) else beam_off, dtype=np.int64).reshape(-1))
    if beam_off.shape[0] != G + 1:
        raise ValueError(f"beam_tally: {G} grid(s) and {beam_off.shape[0]} beam offsets")
    if isinstance(form, str) and form not in FORMS:
        raise ValueError(f"beam_tally: form is one of {sorted(FORMS)}, got {form!r}")
    table = (_lib.StVoxelGrid * G)()
    cells = [g.n_cells for g in grids]
    for t, g in zip(table, grids):
        t.lo[0], t.lo[1], t.lo[2] = g.lo
        t.dim[0], t.dim[1], t.dim[2] = g.dim
        t.cell, t.reserved = g.cell, 0
    total = int(sum(cells))
    if total >= 2 ** 31:
        raise ValueError(f"beam_tally: {total} cells in one call (fewer than 2^31)")
    counts = torch.empty((3, total), dtype=torch.int32, device=dev)  # enter, hit, behind: the kernel's uint32
    path = torch.empty(total, dtype=torch.int64, device=dev)
    cell_of_hit = torch.empty(R, dtype=torch.int32, device=dev) if hit_cell else None
    counters = torch.empty(2, dtype=torch.int32, device=dev)
    nbytes = L.st_beam_tally_workspace_bytes(R, G)
    if nbytes < 0:
        raise _lib.StError(f"beam_tally: {R} beams and {G} grid(s) are outside what the call takes")
    ws = _lib.workspace(nbytes, dev)
    p = lambda t: _lib.ptr(t) if t is not None and t.numel() else None
    _lib.check(L.st_beam_tally_seg(p(origins), S, p(origin_idx), p(dir), p(range), R, ctypes.cast(table, ctypes.c_void_p), G,
                                   beam_off.ctypes.data_as(ctypes.c_void_p), float(max_range), 1 if behind else 0,
                                   FORMS[form] if isinstance(form, str) else int(form), _lib.ptr(counts[0]), _lib.ptr(counts[1]),
                                   _lib.ptr(counts[2]), _lib.ptr(path), p(cell_of_hit), _lib.ptr(counters), _lib.ptr(ws), ws.numel(),
                                   _lib.stream(dev)))
    n_bad, n_outside = (int(v) & 0xFFFFFFFF for v in counters.tolist())  # the one read-back
    wide = counts.long() & 0xFFFFFFFF
    out, first = [], 0
    for k, g in enumerate(grids):
        rows = slice(first, first + cells[k])
        first += cells[k]
        out.append(BeamTally(g, wide[0, rows].view(g.dim), wide[1, rows].view(g.dim), wide[2, rows].view(g.dim), path[rows].view(g.dim),
                             cell_of_hit[int(beam_off[k]):int(beam_off[k + 1])] if hit_cell else None, n_bad, n_outside))
    return out[0] if single else out


def beams_from_points(xyz, origins, origin_idx):
    """For a real scan that records a scan position per point: the beams of its returns, (dir [N,3] float32, range [N] float32) from
    `origins[origin_idx]` to every point.  Such a scan has no misses, so cells are only ever entered on the way to a return."""
    origins = torch.as_tensor(origins).to(xyz.device)
    origin_idx = torch.as_tensor(origin_idx).to(xyz.device)
    d = xyz.double().reshape(-1, 3) - origins.double().reshape(-1, 3).index_select(0, origin_idx.reshape(-1).long())
    rng = torch.linalg.norm(d, dim=1)
    unit = d / torch.where(rng > 0, rng, torch.ones_like(rng)).unsqueeze(1)
    unit[rng == 0] = torch.tensor([1.0, 0.0, 0.0], dtype=torch.float64, device=xyz.device)  # a point on its scanner: any direction
    return unit.float(), rng.float()


def visibility_of_points(tally: BeamTally, xyz) -> torch.Tensor:
    """uint8 [N]: the state of the cell under each point (`BeamTally.state`); 0 for a point outside the grid."""
    xyz = torch.as_tensor(xyz).to(tally.enter.device)
    cell, inside = tally.grid.cell_of(xyz)
    s = tally.state().reshape(-1).index_select(0, cell)
    return torch.where(inside, s, torch.zeros_like(s))


# ---------------------------------------------------------------------------------------------------------------- cli ---
DEFAULTS = {"beams": None, "out": None, "cell": 0.1, "margin": 0.2, "max_range": math.inf, "behind": True, "G": 0.5, "device": "cuda:0"}
USAGE = ("usage: python -m smart_tree_amd.occupancy beams=<beams.npz> out=<dir|.npz> [cell=0.1] [margin=0.2] [max_range=inf] "
         "[behind=true] [G=0.5] [device=]")


def save_beams(path, origins, origin_idx, dir, range) -> None:
    """The file the occupancy command reads: origins [S,3] float32, origin_idx [R] int32, dir [R,3] float32, range [R] float32."""
    n = lambda t, dt: np.ascontiguousarray((t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)), dtype=dt)
    path = Path(path)
    path.parent.mkdir(parents=True, exist_ok=True)
    np.savez(path, origins=n(origins, np.float32).reshape(-1, 3), origin_idx=n(origin_idx, np.int32).reshape(-1),
             dir=n(dir, np.float32).reshape(-1, 3), range=n(range, np.float32).reshape(-1))


def main(argv=None) -> BeamTally:
    import sys

    from .config import apply_overrides

    cfg = apply_overrides(dict(DEFAULTS), argv if argv is not None else sys.argv[1:])
    unknown = sorted(set(cfg) - set(DEFAULTS))
    if unknown or cfg["beams"] is None or cfg["out"] is None:
        raise SystemExit(USAGE + (f"  (unknown: {', '.join(unknown)})" if unknown else ""))
    dev = torch.device(str(cfg["device"]))
    with np.load(str(cfg["beams"])) as z:
        missing = [k for k in ("origins", "origin_idx", "dir", "range") if k not in z]
        if missing:
            raise SystemExit(f"{cfg['beams']}: no {', '.join(missing)}  ({USAGE})")
        origins, origin_idx, dir, rng = (torch.from_numpy(np.ascontiguousarray(z[k])).to(dev) for k in ("origins", "origin_idx", "dir", "range"))
    back = torch.isfinite(rng)
    if not bool(back.any()):
        raise SystemExit(f"{cfg['beams']}: no beam returned, so there is nothing to put a grid around")
    points = origins.index_select(0, origin_idx[back].long()) + rng[back].unsqueeze(1) * dir[back]
    grid = VoxelGrid.around(points, float(cfg["cell"]), float(cfg["margin"]))
    behind = cfg["behind"] if isinstance(cfg["behind"], bool) else str(cfg["behind"]).lower() in ("1", "true", "yes")
    tally = beam_tally(origins, origin_idx, dir, rng, grid, max_range=float(cfg["max_range"]), behind=behind)
    state, G = tally.state(), float(cfg["G"])
    out = Path(str(cfg["out"]))
    out = out if out.suffix == ".npz" else out / "occupancy.npz"
    out.parent.mkdir(parents=True, exist_ok=True)
    n = lambda t: t.detach().cpu().numpy()
    np.savez(out, lo=np.asarray(grid.lo, np.float32), cell=np.float32(grid.cell), dim=np.asarray(grid.dim, np.int32),
             enter=n(tally.enter).astype(np.uint32), hit=n(tally.hit).astype(np.uint32), behind=n(tally.behind).astype(np.uint32),
             path=n(tally.path).astype(np.uint64), state=n(state), density=n(tally.plant_area_density(G)))
    counts = torch.bincount(state.reshape(-1).long(), minlength=4).tolist()
    print(f"{grid.n_cells} cells of {grid.cell:g} m ({grid.dim[0]} x {grid.dim[1]} x {grid.dim[2]}), {rng.shape[0]} beams "
          f"({tally.n_bad} bad, {tally.n_outside} outside the grid)")
    print("  ".join(f"{name}: {c}" for name, c in zip(STATES, counts)))
    print(f"plant area {tally.plant_area(G):.3f} m2 (G = {G:g}) -> {out}")
    return tally


if __name__ == "__main__":
    main()
