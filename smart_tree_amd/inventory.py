"""Measure trees: height, diameter at breast height, crown extent and wood volume per tree (csrc/tree_tally.hip).

`python -m smart_tree_amd.inventory cloud=<.npz|.ply> skeleton=<skeleton.npz> out=<dir> [cell=0.1] [layers=256] [breast_height=1.3]
[max_distance=] [centre=false] [device=cuda:0]` writes `inventory.json`, `trees.csv` and `branches.csv` and prints one line per tree.
`centre=true` runs `CentreCloud` first, as for `segmentation`.  Overrides are parsed by config.py.

The reference measures nothing: `BranchSkeleton.length` / `TreeSkeleton.length` are its only quantities.  `measure_trees` takes
what `segment_cloud` takes and answers per tree and per branch.  What depends on the points -- the tree's box, its points per class
and the distinct cells its crown occupies in plan and, by height layer, in volume -- is one HIP call over the points and the
per-point tree ids of the segmentation (`st_tree_tally`; include/smarttree_hip.h states the contract): integers and extrema, the
same bits in every run, for a batch and for its clouds alone.  What depends on the skeleton -- lengths, frustum volumes and areas,
branch orders, branching angles, the diameter at breast height -- is float64 arithmetic on the host over its few thousand tubes.

Known limits: the crown is every point segmented onto the tree (no crown-base detection: a trunk's cells count); crown area is
occupied cells, not a hull; `measure_trees` takes the classes 0..254 of `cloud.class_l`: a point whose class is negative (an
"unlabelled" -1), NaN or above 254 takes no part in its tree's box, counts and cells.
"""
from __future__ import annotations

import json
from dataclasses import dataclass, field
from pathlib import Path

import numpy as np
import torch

from . import _lib
from .data_types.cloud import Cloud
from .data_types.flat import FlatSkeletons, points_and_skeletons

TALLY_OUTPUTS = ("box", "counts", "area_cells", "profile")
MAX_CLASSES = 255
TREE_HEAD = ("cloud", "tree", "points")
TREE_TAIL = ("base", "height", "crown_width", "crown_area", "crown_volume", "widest_layer_height", "branches", "max_order", "length",
             "wood_volume", "wood_area", "volume_order_0", "volume_order_1", "volume_order_2", "volume_order_3", "trunk_length", "dbh")
BRANCH_COLUMNS = ("cloud", "tree", "branch", "parent", "order", "tubes", "length", "volume", "area", "mean_radius", "base_radius",
                  "tip_radius", "angle", "points")


def tree_tally(pts, tree, n_trees, cls=None, n_classes=1, up=1, cell=0.1, layers=256, outputs=TALLY_OUTPUTS) -> dict:
    """`st_tree_tally` on device tensors: pts [n,3] with the row `tree` [n] int32 of every point's tree among `n_trees`, and its
    class `cls` [n] uint8 (None: one class).  Returns the requested device tensors: "box" float32 [T,6], "counts" int64 [T,C],
    "area_cells" int64 [T], "profile" int64 [T,layers].  Nothing is read back."""
    L = _lib.lib()
    dev = pts.device
    pts = pts.to(dev).float().reshape(-1, 3).contiguous()
    tree = tree.to(dev).to(torch.int32).reshape(-1).contiguous()
    n, T = pts.shape[0], int(n_trees)
    if tree.shape[0] != n:
        raise ValueError(f"tree_tally: {n} points with {tree.shape[0]} tree ids")
    if cls is None:
        n_classes = 1
    else:
        cls = cls.to(dev).to(torch.uint8).reshape(-1).contiguous()
        if cls.shape[0] != n:
            raise ValueError(f"tree_tally: {n} points with {cls.shape[0]} classes")
    unknown = sorted(set(outputs) - set(TALLY_OUTPUTS))
    if unknown:
        raise ValueError(f"tree_tally: outputs are {', '.join(TALLY_OUTPUTS)} (got {', '.join(unknown)})")
    nbytes = L.st_tree_tally_workspace_bytes(n, T, int(layers))
    if nbytes < 0:
        raise _lib.StError(f"tree_tally: {n} points, {T} trees and {layers} layers are outside what the call takes")
    rows, C, Ly = max(T, 0), max(int(n_classes), 1), max(int(layers), 1)
    out = {"box": torch.empty((rows, 6), dtype=torch.float32, device=dev) if "box" in outputs else None,
           "counts": torch.empty((rows, C), dtype=torch.int64, device=dev) if "counts" in outputs else None,
           "area_cells": torch.empty(rows, dtype=torch.int64, device=dev) if "area_cells" in outputs else None,
           "profile": torch.empty((rows, Ly), dtype=torch.int64, device=dev) if "profile" in outputs else None}
    ws = _lib.workspace(nbytes, dev)
    p = lambda t: _lib.ptr(t) if t is not None and t.numel() else None
    _lib.check(L.st_tree_tally(p(pts), n, p(tree), p(cls), int(n_classes), T, int(up), float(cell), int(layers), p(out["box"]),
                               p(out["counts"]), p(out["area_cells"]), p(out["profile"]), _lib.ptr(ws), ws.numel(), _lib.stream(dev)))
    return {k: v for k, v in out.items() if v is not None}


# ------------------------------------------------------------------------------------------------ the skeleton, flat ---
def tree_lookup(flat: FlatSkeletons):
    """(table int32 [S + 1], base int64 [clouds], span int64 [clouds]): table[base[c] + t] is the row of tree t of cloud c among
    `flat.tree_rows` for 0 <= t < span[c], -1 for a tree id the skeleton does not hold; the last entry (-1) is what a point without
    a tree indexes."""
    if len(flat.tree_rows) and (flat.tree_rows[:, 1].min() < 0 or flat.tree_rows[:, 1].max() >= 1 << 24):
        raise ValueError("measure_trees: tree ids must be in [0, 2^24)")
    span = np.zeros(flat.n_clouds, np.int64)
    for c, t in flat.tree_rows.tolist():
        span[c] = max(span[c], t + 1)
    base = np.concatenate([[0], np.cumsum(span)]).astype(np.int64)
    table = np.full(int(base[-1]) + 1, -1, np.int32)
    for row, (c, t) in enumerate(flat.tree_rows.tolist()):
        table[base[c] + t] = row
    return table, base[:-1], span


# ------------------------------------------------------------------------------------------------ host metrics ---
def _segment_distance2(p, a, b):
    """Squared distance of point p to every segment a[i] -> b[i] (a zero-length segment is the point a)."""
    ab = b - a
    den = (ab * ab).sum(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        t = np.where(den > 0, ((p - a) * ab).sum(1) / den, 0.0)
    t = np.clip(t, 0.0, 1.0)
    v = a + t[:, None] * ab - p
    return (v * v).sum(1)


def branch_table(flat: FlatSkeletons, points=None):
    """(float64 [B,14], BRANCH_COLUMNS; orphans int64 [k,3] = cloud, tree, branch) of the skeletons in `flat`.
    order: a root is 0, a child its parent's plus 1; a branch whose parent is not in its tree counts as a root (and is an orphan when
    it names one: a parent id other than -1 and its own).  volume = sum pi h (r1^2 + r1 r2 + r2^2) / 3 and area = sum
    pi (r1 + r2) sqrt(h^2 + (r1 - r2)^2) over its tubes; mean_radius is length-weighted; angle: degrees between the first tube's
    direction and the direction of the parent's tube nearest to the branch's first point (ties to the lowest tube), NaN for roots."""
    rows, xyz, radii = flat.rows, flat.xyz, flat.radii
    B = len(rows)
    out = np.full((B, len(BRANCH_COLUMNS)), np.nan)
    orphans = []
    if not B:
        return out, np.zeros((0, 3), np.int64)
    out[:, :4] = rows[:, :4]
    tubes, start, first_tube = flat.tubes_of_row, flat.tube_start, flat.tube_first
    out[:, 5] = tubes
    owner = np.repeat(np.arange(B), tubes)
    d = xyz[start + 1] - xyz[start]
    h = np.sqrt((d * d).sum(1))
    r1, r2 = radii[start], radii[start + 1]
    total = lambda w: np.bincount(owner, weights=w, minlength=B)
    out[:, 6] = total(h)
    out[:, 7] = total(np.pi * h * (r1 * r1 + r1 * r2 + r2 * r2) / 3.0)
    out[:, 8] = total(np.pi * (r1 + r2) * np.sqrt(h * h + (r1 - r2) * (r1 - r2)))
    with np.errstate(invalid="ignore", divide="ignore"):
        out[:, 9] = np.where(out[:, 6] > 0, total(h * (r1 + r2) * 0.5) / out[:, 6], np.nan)
    has = rows[:, 5] > 0
    out[has, 10] = radii[rows[has, 4]]
    out[has, 11] = radii[rows[has, 4] + rows[has, 5] - 1]
    # orders: walk up to a branch whose order is known, or to a parent the tree does not hold
    index = {(c, t, b): k for k, (c, t, b) in enumerate(rows[:, :3].tolist())}
    parent_row = np.full(B, -1, np.int64)
    for k, (c, t, b, p) in enumerate(rows[:, :4].tolist()):
        j = index.get((c, t, p), -1) if p != b else -1
        parent_row[k] = j
        if j < 0 and p != -1 and p != b:
            orphans.append((c, t, b))
    order = np.full(B, -1, np.int64)
    for k in range(B):
        chain, j = [], k
        while j >= 0 and order[j] < 0 and j not in chain:
            chain.append(j)
            j = int(parent_row[j])
        depth = order[j] + 1 if j >= 0 and order[j] >= 0 else 0  # a cycle's first branch counts as a root as well
        for j in reversed(chain):
            order[j] = depth
            depth += 1
    out[:, 4] = order
    for k in range(B):
        j = int(parent_row[k])
        if j < 0 or tubes[k] < 1 or tubes[j] < 1:
            continue
        a, b = xyz[start[first_tube[j]:first_tube[j + 1]]], xyz[start[first_tube[j]:first_tube[j + 1]] + 1]
        near = int(np.argmin(_segment_distance2(xyz[rows[k, 4]], a, b)))
        u, w = d[first_tube[k]], b[near] - a[near]
        den = np.sqrt((u * u).sum()) * np.sqrt((w * w).sum())
        if den > 0:
            out[k, 12] = np.degrees(np.arccos(np.clip((u * w).sum() / den, -1.0, 1.0)))
    if points is not None:
        out[:, 13] = points
    return out, np.asarray(orphans, np.int64).reshape(-1, 3)


def radius_at_height(xyz, radii, level, up=1) -> float:
    """The radius of a branch where it first crosses the up-coordinate `level`, linear inside the tube; NaN when it never does."""
    for i in range(len(xyz) - 1):
        ua, ub = xyz[i, up], xyz[i + 1, up]
        if min(ua, ub) <= level <= max(ua, ub):
            t = (level - ua) / (ub - ua) if ub != ua else 0.0
            return float(radii[i] + t * (radii[i + 1] - radii[i]))
    return float("nan")


LEAF_AREA = "leaf_area_m2"  # the optional last column: measure_trees(..., plant_area=)


def tree_columns(n_classes: int) -> tuple:
    return TREE_HEAD + tuple(f"points_class_{k}" for k in range(n_classes)) + TREE_TAIL


def tree_table(flat: FlatSkeletons, branches, box, counts, area_cells, profile, cell, breast_height=1.3, up=1, ground_base=None):
    """float64 [T, 3 + C + 17] (`tree_columns(C)`) from the tallies (host arrays) and the branch table.  `ground_base` [T] (or None):
    the terrain under every tree's root; where it is finite it is the tree's base instead of its lowest point."""
    T, C = len(flat.tree_rows), counts.shape[1]
    cols = tree_columns(C)
    at = {name: k for k, name in enumerate(cols)}
    out = np.full((T, len(cols)), np.nan)
    h0, h1 = (1 if up == 0 else 0), (1 if up == 2 else 2)
    box = box.astype(np.float64)
    for r, (c, t) in enumerate(flat.tree_rows.tolist()):
        mine = np.flatnonzero(flat.tree_of_branch == r)
        n_pts = int(counts[r].sum())
        out[r, :3] = (c, t, n_pts)
        out[r, 3:3 + C] = counts[r]
        ends = np.concatenate([flat.xyz[o:o + n, up] for o, n in flat.rows[mine, 4:6].tolist()] or [np.zeros(0)])
        base = box[r, up] if n_pts else (ends.min() if len(ends) else np.nan)
        low = box[r, up]
        if ground_base is not None and np.isfinite(ground_base[r]):
            base = low = float(ground_base[r])
        out[r, at["base"]] = base
        if n_pts:
            out[r, at["height"]] = box[r, 3 + up] - low
            out[r, at["crown_width"]] = max(box[r, 3 + h0] - box[r, h0], box[r, 3 + h1] - box[r, h1])
        out[r, at["crown_area"]] = float(area_cells[r]) * cell * cell
        out[r, at["crown_volume"]] = float(profile[r].sum()) * cell * cell * cell
        if profile[r].any():
            out[r, at["widest_layer_height"]] = (int(np.argmax(profile[r])) + 0.5) * cell
        rows = branches[mine]
        out[r, at["branches"]] = len(mine)
        out[r, at["max_order"]] = rows[:, 4].max() if len(mine) else np.nan
        out[r, at["length"]], out[r, at["wood_volume"]], out[r, at["wood_area"]] = rows[:, 6].sum(), rows[:, 7].sum(), rows[:, 8].sum()
        for k in range(4):
            sel = rows[:, 4] == k if k < 3 else rows[:, 4] >= 3
            out[r, at[f"volume_order_{k}"]] = rows[sel, 7].sum()
        roots = mine[rows[:, 4] == 0]
        if len(roots):  # the root branch: the first of order 0
            o, n = flat.rows[roots[0], 4:6].tolist()
            out[r, at["trunk_length"]] = branches[roots[0], 6]
            out[r, at["dbh"]] = 2.0 * radius_at_height(flat.xyz[o:o + n], flat.radii[o:o + n], base + breast_height, up)
    return out


# ------------------------------------------------------------------------------------------------ the result ---
def _listed(a):
    """A float array as nested lists with None for NaN (JSON has no NaN)."""
    a = np.asarray(a, np.float64)
    return [[None if v != v else v for v in row] for row in a.tolist()]


def _array(rows, width):
    return np.asarray([[np.nan if v is None else v for v in row] for row in rows], np.float64).reshape(-1, width)


@dataclass
class TreeInventory:
    """`trees`: float64 [T, ...] on the host, one row per (cloud, tree) in `skeleton_owners` order, columns `tree_columns` (metres,
    m2, m3; see `tree_table`).  `branches`: float64 [B,14], BRANCH_COLUMNS.  `profile`: int64 [T, layers], the distinct occupied
    cells of every tree per height layer of `cell` metres above its lowest point.  `orphans`: int64 [k,3], the (cloud, tree, branch)
    whose parent id is not in their tree."""
    trees: np.ndarray
    branches: np.ndarray
    profile: np.ndarray
    cell: float
    tree_columns: tuple = ()
    orphans: np.ndarray = field(default_factory=lambda: np.zeros((0, 3), np.int64))
    breast_height: float = 1.3
    up: int = 1
    n_clouds: int = 1

    def __len__(self) -> int:
        return int(self.trees.shape[0])

    def column(self, name: str) -> np.ndarray:
        return self.trees[:, self.tree_columns.index(name)]

    def branch_column(self, name: str) -> np.ndarray:
        return self.branches[:, BRANCH_COLUMNS.index(name)]

    def split(self) -> list:
        """The clouds of a batch, each as its own call gives it (the class columns end at the cloud's own last class)."""
        first = len(TREE_HEAD)
        extra = tuple(self.tree_columns[-1:]) if tuple(self.tree_columns[-1:]) == (LEAF_AREA,) else ()
        C = len(self.tree_columns) - first - len(TREE_TAIL) - len(extra)
        out = []
        for k in range(self.n_clouds):
            sel = self.trees[:, 0] == k
            trees = self.trees[sel].copy()
            trees[:, 0] = 0
            keep = _used_classes(trees[:, first:first + C])
            trees = np.concatenate([trees[:, :first + keep], trees[:, first + C:]], axis=1)
            rows = self.branches[self.branches[:, 0] == k].copy()
            rows[:, 0] = 0
            orphans = self.orphans[self.orphans[:, 0] == k].copy()
            orphans[:, 0] = 0
            out.append(TreeInventory(trees, rows, self.profile[sel], self.cell, tree_columns(keep) + extra, orphans, self.breast_height, self.up))
        return out

    def save(self, directory) -> None:
        """`inventory.json` (everything; NaN as null), `trees.csv`, `branches.csv`."""
        directory = Path(directory)
        directory.mkdir(parents=True, exist_ok=True)
        doc = {"cell": self.cell, "layers": int(self.profile.shape[1]) if self.profile.ndim == 2 else 0, "breast_height": self.breast_height,
               "up": self.up, "clouds": self.n_clouds, "tree_columns": list(self.tree_columns), "branch_columns": list(BRANCH_COLUMNS), "trees": _listed(self.trees),
               "branches": _listed(self.branches), "profile": self.profile.tolist(), "orphans": self.orphans.tolist()}
        (directory / "inventory.json").write_text(json.dumps(doc) + "\n")
        for name, cols, table in (("trees.csv", self.tree_columns, self.trees), ("branches.csv", BRANCH_COLUMNS, self.branches)):
            lines = [",".join(cols)] + [",".join(format(v, ".17g") for v in row) for row in table.tolist()]
            (directory / name).write_text("\n".join(lines) + "\n")

    @staticmethod
    def load(path) -> "TreeInventory":
        """From `inventory.json` or the directory that holds it."""
        path = Path(path)
        doc = json.loads((path / "inventory.json" if path.is_dir() else path).read_text())
        cols = tuple(doc["tree_columns"])
        return TreeInventory(_array(doc["trees"], len(cols)), _array(doc["branches"], len(BRANCH_COLUMNS)),
                             np.asarray(doc["profile"], np.int64).reshape(-1, int(doc["layers"])), float(doc["cell"]), cols,
                             np.asarray(doc["orphans"], np.int64).reshape(-1, 3), float(doc["breast_height"]), int(doc["up"]), int(doc["clouds"]))


def _used_classes(counts) -> int:
    """Columns up to the last class that has a point (at least one)."""
    counts = np.asarray(counts)
    used = np.flatnonzero(counts.any(0)) if counts.ndim == 2 and len(counts) else np.zeros(0, np.int64)
    return int(used[-1]) + 1 if len(used) else 1


def point_rows(flat: FlatSkeletons, tree_id, seg_off=None, device=None) -> torch.Tensor:
    """int32 [n] on the device: the row among `flat.tree_rows` of every point's tree, from the segmentation's `tree_id` (the tree's
    id inside its cloud) and the cloud's tree offset; -1 for a point without a tree.  Nothing is read back."""
    dev = torch.device(device) if device is not None else tree_id.device
    table, base, span = tree_lookup(flat)
    tree_id = tree_id.to(dev).long().reshape(-1)
    n = tree_id.shape[0]
    if seg_off is not None:
        sizes = (seg_off[1:] - seg_off[:-1]).to(dev).long()
        per_point = lambda v: torch.repeat_interleave(torch.from_numpy(v).to(dev), sizes, output_size=n)
        slot, limit = tree_id + per_point(base), per_point(span)
    else:
        slot, limit = tree_id, int(span[0]) if len(span) else 0
    # a point without a tree, or with an id its cloud's skeleton does not reach, reads the table's last entry: -1
    slot = torch.where((tree_id >= 0) & (tree_id < limit), slot, torch.full_like(slot, len(table) - 1))
    return torch.from_numpy(table).to(dev).index_select(0, slot)


def root_positions(flat: FlatSkeletons, branches) -> np.ndarray:
    """float64 [T,3]: the first vertex of every tree's root branch (the first of order 0), NaN for a tree without one."""
    out = np.full((len(flat.tree_rows), 3), np.nan)
    for r in range(len(flat.tree_rows)):
        mine = np.flatnonzero(flat.tree_of_branch == r)
        roots = mine[(branches[mine, 4] == 0) & (flat.rows[mine, 5] > 0)]
        if len(roots):
            out[r] = flat.xyz[flat.rows[roots[0], 4]]
    return out


def measure_trees(cloud, skeleton, segmentation=None, cell=0.1, layers=256, breast_height=1.3, up=1, max_distance=None,
                  device=None, ground=None, plant_area=None) -> TreeInventory:
    """Every tree of `skeleton` measured on the points of `cloud` segmented onto it.  Takes what `segment_cloud` takes: a `Cloud` or
    [n,3] points with a `TreeSkeleton`, a `DisjointTreeSkeleton` or the flat arrays of `save_skeleton_npz`; a collated `Cloud` with a
    list of skeletons, one per cloud.  `segmentation`: the `CloudSegmentation` of these points and this skeleton when the caller has
    it (else `segment_cloud` runs here, with `max_distance`).  One tally call and one read-back for the whole batch.
    `ground`: the `terrain.GroundModel` of these clouds, in their frame.  A tree's `base` is then the terrain under the first vertex of
    its root branch (`ground.surface_at`), and `height` and the level of the DBH follow from it; where the terrain is unknown there
    (NaN) the base stays the tree's lowest point.  None changes nothing.
    `plant_area`: [n_trees] m2, one value per tree in `skeleton_owners` order -- what `occupancy.BeamTally.plant_area_by_label` gives
    for the tree rows of the returns (`point_rows`); it becomes the last column, `leaf_area_m2`.  None adds no column."""
    from .segmentation import segment_cloud

    pts, seg_off, skeletons, _, n_clouds = points_and_skeletons(cloud, skeleton, device, "measure_trees")
    dev, n = pts.device, pts.shape[0]
    class_l = cloud.class_l if isinstance(cloud, Cloud) else None
    if not (up in (0, 1, 2) and cell > 0 and np.isfinite(cell) and 1 <= int(layers) <= 4096):
        raise ValueError(f"measure_trees: up in 0..2, cell > 0 and 1 <= layers <= 4096 (got {up}, {cell}, {layers})")
    if segmentation is None:
        segmentation = segment_cloud(Cloud(xyz=pts, seg_off=seg_off) if seg_off is not None else pts, skeleton, max_distance=max_distance, device=dev)
    if len(segmentation) != n:
        raise ValueError(f"measure_trees: a segmentation of {len(segmentation)} points for a cloud of {n}")
    flat = FlatSkeletons(skeletons, "measure_trees")
    if len(flat.rows) != len(segmentation.branches):
        raise ValueError(f"measure_trees: a segmentation onto {len(segmentation.branches)} branches for a skeleton of {len(flat.rows)}")
    T = len(flat.tree_rows)
    row = point_rows(flat, segmentation.tree_id, seg_off if n_clouds > 1 else None, dev)
    cls = None
    if class_l is not None and class_l.shape[0] == n:
        # classes 0..254 as they are; a negative, NaN or larger label becomes 255, which the call leaves out (255 >= n_classes)
        label = class_l.to(dev).reshape(-1)
        cls = torch.where((label >= 0) & (label < MAX_CLASSES), label, torch.full_like(label, MAX_CLASSES)).to(torch.uint8)
    res = tree_tally(pts, row, T, cls, MAX_CLASSES if cls is not None else 1, up, cell, layers)
    C = res["counts"].shape[1]
    packed = torch.cat([res["counts"].reshape(-1), res["area_cells"], res["profile"].reshape(-1), res["box"].view(torch.int64).reshape(-1)])
    host = packed.cpu().numpy()  # the one read-back
    counts, host = host[:T * C].reshape(T, C), host[T * C:]
    area_cells, host = host[:T], host[T:]
    profile, host = host[:T * int(layers)].reshape(T, int(layers)).copy(), host[T * int(layers):]
    box = host.view(np.float32).reshape(T, 6)
    counts = counts[:, :_used_classes(counts)]
    branches, orphans = branch_table(flat, segmentation.branches[:, 5])
    ground_base = None
    if ground is not None:
        if ground.up != int(up) or ground.n_clouds != n_clouds:
            raise ValueError(f"measure_trees: a ground model of {ground.n_clouds} cloud(s) with up={ground.up} for {n_clouds} cloud(s) with up={up}")
        roots, ground_base = root_positions(flat, branches), np.full(T, np.nan)
        for c in range(n_clouds):
            sel = np.flatnonzero((flat.tree_rows[:, 0] == c) & np.isfinite(roots).all(1))
            if len(sel):
                ground_base[sel] = ground.surface_at(roots[sel].astype(np.float32), cloud=c).cpu().numpy()
    trees = tree_table(flat, branches, box, counts, area_cells, profile, float(cell), float(breast_height), int(up), ground_base)
    columns = tree_columns(counts.shape[1])
    if plant_area is not None:
        area = (plant_area.detach().cpu().numpy() if torch.is_tensor(plant_area) else np.asarray(plant_area)).astype(np.float64).reshape(-1)
        if area.shape[0] != T:
            raise ValueError(f"measure_trees: plant_area has {area.shape[0]} value(s) for {T} tree(s)")
        trees, columns = np.concatenate([trees, area[:, None]], axis=1), columns + (LEAF_AREA,)
    return TreeInventory(trees, branches, profile, float(cell), columns, orphans, float(breast_height), int(up), n_clouds)


def summary(inv: TreeInventory) -> str:
    """One line per tree."""
    at = {name: k for k, name in enumerate(inv.tree_columns)}
    lines = []
    for r in inv.trees:
        g = lambda name: r[at[name]]
        lines.append(f"cloud {int(g('cloud'))} tree {int(g('tree'))}: height {g('height'):.2f} m, dbh {g('dbh'):.3f} m, crown {g('crown_width'):.2f} m wide, "
                     f"{g('crown_area'):.2f} m2, {g('crown_volume'):.2f} m3, wood {g('wood_volume'):.4f} m3 in {int(g('branches'))} branches "
                     f"(order <= {int(g('max_order'))}), {int(g('points'))} points")
    return "\n".join(lines)


# ---------------------------------------------------------------------------------------------------------------- cli ---
DEFAULTS = {"cloud": None, "skeleton": None, "out": None, "cell": 0.1, "layers": 256, "breast_height": 1.3, "max_distance": None,
            "centre": False, "device": "cuda:0"}
USAGE = ("usage: python -m smart_tree_amd.inventory cloud=<.npz|.ply> skeleton=<skeleton.npz> out=<dir> [cell=0.1] [layers=256] "
         "[breast_height=1.3] [max_distance=] [centre=false] [device=]")


def main(argv=None) -> TreeInventory:
    from .config import cloud_command
    from .evaluate import load_any_skeleton

    cfg, dev, cloud = cloud_command(argv, DEFAULTS, USAGE)
    inv = measure_trees(cloud, load_any_skeleton(cfg["skeleton"]), cell=float(cfg["cell"]), layers=int(cfg["layers"]),
                        breast_height=float(cfg["breast_height"]),
                        max_distance=None if cfg["max_distance"] is None else float(cfg["max_distance"]), device=dev)
    inv.save(Path(str(cfg["out"])))
    print(summary(inv))
    return inv


if __name__ == "__main__":
    main()
