"""Labelled synthetic trees generated on the device (csrc/synthetic.hip: st_synth_points_seg), as a training dataset.

The reference's training set is an external download (the `synthetic-trees` link of its README).  Here a tree is grown on the
host by `smart_tree_amd.synthetic.grow_tree` (seeded, a few thousand tapered cylinders at most), turned into a segment table
and its ground-truth `TreeSkeleton`, and its points are sampled by one kernel launch for up to 64 trees: exact labels (class,
medial vector, branch id), no files, no upload of points.

* `tree_skeleton(segs, tree_id)`: the branches of a `grow_tree` result.
* `segment_table(segs)`: what the kernel reads of one tree.
* `generate_trees(seeds, n_points, ...)`: one batched `Cloud` plus the skeletons.
* `scan_trees(seeds, scanners, ...)`: the same trees seen by a ring of virtual laser scanners (smart_tree_amd/scan.py): one side
  of a stem per position, density falling with the range, shadows.
* `SyntheticTreeDataset`: `TreeDataset`'s item layout from trees generated on the fly, fresh ones every training epoch.
* `python -m smart_tree_amd.dataset.generate` writes a folder of them (dataset/generate.py).

The geometry model and the meaning of every label are `synthetic.sample_tree_cloud`'s; the random stream (Philox4x32-10 per
point) and the foliage draw (Bernoulli per point instead of an exact count and a permutation) are not, so the clouds differ
(DESIGN.md "Dataset: synthetic trees on the device").
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Sequence

import numpy as np
import torch

from .. import _lib
from ..data_types.branch import BranchSkeleton
from ..data_types.cloud import Cloud
from ..data_types.tree import TreeSkeleton
from ..synthetic import TreeSegments, _orthobasis, grow_tree
from .dataset import TreeDataset

MAX_TREES = 64  # trees per launch (ST_MAX_SEG)
MODES = ("train", "validation", "test")
_M64 = (1 << 64) - 1


# ------------------------------------------------------------------------------------------------------- host side ---
def segment_parents(segs: TreeSegments) -> np.ndarray:
    """Parent segment of every segment (-1 for the trunk).  `grow_tree` appends in depth-first pre-order, so the parent of
    segment j is the latest earlier segment one level up."""
    depth = np.asarray(segs.depth).astype(np.int64)
    parent = np.full(len(depth), -1, dtype=np.int64)
    latest = {}
    for j, d in enumerate(depth):
        if d > 0:
            parent[j] = latest[d - 1]
        latest[int(d)] = j
    return parent


def segment_branches(segs: TreeSegments):
    """(branch id [S], parent branch id per branch, segments per branch).  Segment 0 starts branch 0; a segment's first child
    in list order continues its parent's branch, every other child starts a new one whose parent is the parent segment's
    branch; ids are given in first-appearance order."""
    parent = segment_parents(segs)
    branch = np.zeros(len(parent), dtype=np.int32)
    has_child = np.zeros(len(parent), dtype=bool)
    branch_parent, members = [-1], [[0]]
    for j in range(1, len(parent)):
        p = parent[j]
        if not has_child[p]:
            has_child[p] = True
            branch[j] = branch[p]
            members[branch[j]].append(j)
        else:
            branch[j] = len(branch_parent)
            branch_parent.append(int(branch[p]))
            members.append([j])
    return branch, branch_parent, members


def tree_skeleton(segs: TreeSegments, tree_id: int = 0) -> TreeSkeleton:
    """The ground-truth skeleton: one BranchSkeleton per branch of `segment_branches`; vertices are segment end points (a new
    branch starts at its parent segment's end point, which is its own first segment's start), radii `ra` at a start and `rb`
    at an end."""
    _, branch_parent, members = segment_branches(segs)
    branches = {}
    for bid, (par, seg_ids) in enumerate(zip(branch_parent, members)):
        first = seg_ids[0]
        xyz = np.concatenate([segs.a[[first]], segs.b[seg_ids]]).astype(np.float32)
        radii = np.concatenate([segs.ra[[first]], segs.rb[seg_ids]]).astype(np.float32).reshape(-1, 1)
        branches[bid] = BranchSkeleton(bid, par, torch.from_numpy(xyz), torch.from_numpy(radii))
    return TreeSkeleton(tree_id, branches)


@dataclass
class SegmentTable:
    a: np.ndarray  # [S,3] float32
    b: np.ndarray  # [S,3] float32
    ra: np.ndarray  # [S] float32
    rb: np.ndarray  # [S] float32
    u: np.ndarray  # [S,3] float32: synthetic._orthobasis of the axis direction, computed in float64
    v: np.ndarray  # [S,3] float32
    branch: np.ndarray  # [S] int32
    tips: np.ndarray  # [T,3] float32 end points of the segments without children
    cdf: np.ndarray  # [S] uint32 selection table

    def rows(self) -> np.ndarray:
        """[S,16] float32: the kernel's row layout (ax ay az ra | bx by bz rb | ux uy uz branch bits | vx vy vz 0)."""
        out = np.zeros((len(self.ra), 16), dtype=np.float32)
        out[:, 0:3], out[:, 3] = self.a, self.ra
        out[:, 4:7], out[:, 7] = self.b, self.rb
        out[:, 8:11] = self.u
        out.view(np.int32)[:, 11] = self.branch
        out[:, 12:15] = self.v
        return out


def selection_table(area: np.ndarray) -> np.ndarray:
    """cdf[j] = floor(2^32 * sum(area[0..j]) / sum(area)) in float64, as uint32, the last entry forced to 0xFFFFFFFF."""
    area = np.asarray(area, dtype=np.float64)
    cum = np.cumsum(area)
    cdf = np.minimum(np.floor(cum / cum[-1] * 4294967296.0), 4294967295.0).astype(np.uint64).astype(np.uint32)
    cdf[-1] = 0xFFFFFFFF
    return cdf


def segment_table(segs: TreeSegments) -> SegmentTable:
    axis = segs.b - segs.a
    length = np.linalg.norm(axis, axis=1)
    u, v = _orthobasis(axis / length[:, None])
    area = np.pi * (segs.ra + segs.rb) * length
    f32 = lambda x: np.ascontiguousarray(x, dtype=np.float32)
    return SegmentTable(f32(segs.a), f32(segs.b), f32(segs.ra), f32(segs.rb), f32(u), f32(v), segment_branches(segs)[0],
                        f32(segs.b[segs.is_tip]).reshape(-1, 3), selection_table(area))


def foliage_threshold(fraction: float) -> int:
    """min(floor(fraction * 2^32), 2^32 - 1); the all-ones value means every point (the kernel's rule)."""
    if not 0.0 <= float(fraction) <= 1.0:
        raise ValueError(f"foliage_fraction must be in [0, 1], got {fraction}")
    return min(int(np.floor(float(fraction) * 4294967296.0)), 0xFFFFFFFF)


# ---------------------------------------------------------------------------------------------------------- kernel ---
def _per_tree(value, n, name):
    if np.ndim(value) == 0:
        return [value] * n
    if len(value) != n:
        raise ValueError(f"{name}: {len(value)} values for {n} trees")
    return list(value)


def synth_points(tables: Sequence[SegmentTable], n_points: Sequence[int], seeds: Sequence[int], fol_thr: Sequence[int],
                 noise: Sequence[float], foliage_sigma: Sequence[float], device, outputs=None):
    """One `st_synth_points_seg` launch over `tables`.  Returns dict(xyz, medial_vector, class_l, branch_ids, segment) of device
    tensors, and the int32 offsets (pt_off, tab_off) as numpy arrays.  `outputs`: tensors to write into instead of fresh ones
    (a key mapped to None leaves that output out)."""
    L = _lib.lib()
    dev = torch.device(device)
    B = len(tables)
    off = lambda sizes: np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64))])
    tab_off, tip_off, pt_off = off([len(t.ra) for t in tables]), off([len(t.tips) for t in tables]), off(n_points)
    if pt_off[-1] >= 2 ** 31 or tab_off[-1] >= 2 ** 27:
        raise ValueError(f"synth_points: {pt_off[-1]} points / {tab_off[-1]} segments do not fit the int32 offsets")
    tab_off, tip_off, pt_off = (x.astype(np.int32) for x in (tab_off, tip_off, pt_off))
    cat = lambda parts, shape, dt: np.concatenate(parts) if parts else np.zeros(shape, dt)
    rows = torch.from_numpy(cat([t.rows() for t in tables], (0, 16), np.float32)).to(dev)
    cdf = torch.from_numpy(cat([t.cdf for t in tables], (0,), np.uint32).view(np.int32)).to(dev)
    tips = torch.from_numpy(cat([t.tips for t in tables], (0, 3), np.float32)).to(dev)
    n = int(pt_off[-1])
    out = {"xyz": ((n, 3), torch.float32), "medial_vector": ((n, 3), torch.float32), "class_l": ((n,), torch.float32),
           "branch_ids": ((n,), torch.int32), "segment": ((n,), torch.int32)}
    res = {k: (outputs[k] if outputs is not None and k in outputs else torch.empty(shape, dtype=dt, device=dev))
           for k, (shape, dt) in out.items()}
    seeds64 = np.asarray([int(s) & _M64 for s in seeds], dtype=np.uint64)
    thr = np.asarray(fol_thr, dtype=np.uint32)
    ns, sg = np.asarray(noise, dtype=np.float32), np.asarray(foliage_sigma, dtype=np.float32)
    if not (len(seeds64) == len(thr) == len(ns) == len(sg) == B):
        raise ValueError("synth_points: one seed, threshold, noise and foliage_sigma per tree")
    host = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a.size else None
    p = lambda t: _lib.ptr(t) if t is not None and t.numel() else None
    _lib.check(L.st_synth_points_seg(p(rows), host(tab_off), p(cdf), p(tips), host(tip_off), host(pt_off), B, host(seeds64),
                                     host(thr), host(ns), host(sg), p(res["xyz"]), p(res["medial_vector"]), p(res["class_l"]),
                                     p(res["branch_ids"]), p(res["segment"]), _lib.stream(dev)))
    return res, pt_off, tab_off


def generate_trees(seeds, n_points, *, scale=1.0, noise=0.002, foliage_fraction=0.0, foliage_sigma=None, max_depth=7,
                   labels="segment", device=None):
    """Trees `seeds` (any integers: the low 32 bits seed `grow_tree`, all 64 key the point stream) sampled with `n_points` points
    each.  `n_points`, `foliage_fraction`, `noise` and `max_depth` may be one value or one per tree.  Returns one batched
    `Cloud` (`seg_off` set, `rgb` zeros, `medial_vector`, `class_l` [N,1], `branch_ids` [N,1] int32) and the ground-truth
    skeletons.  foliage_sigma=None: 0.08 * scale.
    labels: "segment" -- the medial vector of a branch point is that of the un-noised surface point it was drawn as (exact);
    "nearest" -- it is taken again from the noised point to the nearest tube of its own tree (st_points_to_nearest_tube), the
    reference's `skeleton_to_points` meaning."""
    if labels not in ("segment", "nearest"):
        raise ValueError(f"labels must be 'segment' or 'nearest', got {labels!r}")
    seeds = [int(s) for s in np.atleast_1d(np.asarray(seeds, dtype=object))]
    B = len(seeds)
    if B > MAX_TREES:
        raise ValueError(f"generate_trees: at most {MAX_TREES} trees per call (got {B})")
    dev = torch.device(device) if device is not None else torch.device("cuda:0")
    counts = [int(c) for c in _per_tree(n_points, B, "n_points")]
    depths = _per_tree(max_depth, B, "max_depth")
    sigma = 0.08 * scale if foliage_sigma is None else foliage_sigma
    grown = [grow_tree(s & 0xFFFFFFFF, scale, int(d)) for s, d in zip(seeds, depths)]
    tables = [segment_table(g) for g in grown]
    skeletons = [tree_skeleton(g, tree_id=i) for i, g in enumerate(grown)]
    res, pt_off, tab_off = synth_points(tables, counts, seeds, [foliage_threshold(f) for f in _per_tree(foliage_fraction, B,
                                        "foliage_fraction")], _per_tree(noise, B, "noise"), [sigma] * B, dev)
    mv = res["medial_vector"]
    if labels == "nearest":
        from ..util.queries import nearest_tube_device

        branch = res["class_l"] == 0
        for s, t in enumerate(tables):
            idx = (branch[pt_off[s]:pt_off[s + 1]]).nonzero().view(-1) + int(pt_off[s])
            if idx.numel():
                f = lambda x: torch.from_numpy(x).to(dev)
                vec, _, _ = nearest_tube_device(res["xyz"].index_select(0, idx), f(t.a), f(t.b), f(t.ra), f(t.rb))
                mv.index_copy_(0, idx, vec)
    cloud = Cloud(res["xyz"], torch.zeros_like(res["xyz"]), mv, None, res["branch_ids"].view(-1, 1), res["class_l"].view(-1, 1),
                  seg_off=torch.from_numpy(pt_off).to(dev))
    return cloud, skeletons


def leaf_centres(segs: TreeSegments, seed: int, leaves_per_tip: int, sigma: float) -> np.ndarray:
    """[T * leaves_per_tip, 3] float32: per tip (end point of a segment without children, in list order) `leaves_per_tip` centres,
    tip + sigma * N(0, 1) per axis, from numpy's `default_rng(seed mod 2^64)`."""
    tips = np.asarray(segs.b[segs.is_tip], dtype=np.float64).reshape(-1, 3)
    rng = np.random.default_rng(int(seed) & _M64)
    return (np.repeat(tips, int(leaves_per_tip), axis=0) + float(sigma) * rng.standard_normal((len(tips) * int(leaves_per_tip), 3))).astype(np.float32)


def scan_trees(seeds, scanners=3, *, step_deg=0.1, radius=6.0, height=1.5, scale=1.0, max_depth=7, leaves_per_tip=0, leaf_radius=0.02,
               foliage_sigma=None, range_noise=0.002, form="auto", device=None, beams=False):
    """Trees `seeds`, grown exactly as `generate_trees` grows them, each scanned by `scanners` positions on a ring of `radius`
    metres about its box, `height` above its lowest point, in beams `step_deg` apart (`scan.scanner_ring`; scanner k of tree `seed`
    draws its range noise with `seed + k`).  `leaves_per_tip` > 0 hangs that many spheres of `leaf_radius` about every tip, their
    centres drawn on the host (`leaf_centres`; foliage_sigma=None: 0.08 * scale); they are class 1, shadow the wood and carry no
    medial vector.  `max_depth` may be one value or one per tree.  Returns what `generate_trees` returns: one batched `Cloud` and
    the ground-truth skeletons; with `beams=True` also `scan_skeletons`' extras with every beam of the scan (`beam_dir`,
    `beam_range`, `beam_scanner`, `origins`), the input of `occupancy.beam_tally`."""
    from ..scan import scan_skeletons, scanner_ring, skeleton_box

    seeds = [int(s) for s in np.atleast_1d(np.asarray(seeds, dtype=object))]
    B = len(seeds)
    if B > MAX_TREES:
        raise ValueError(f"scan_trees: at most {MAX_TREES} trees per call (got {B})")
    dev = torch.device(device) if device is not None else torch.device("cuda:0")
    sigma = 0.08 * scale if foliage_sigma is None else foliage_sigma
    grown = [grow_tree(s & 0xFFFFFFFF, scale, int(d)) for s, d in zip(seeds, _per_tree(max_depth, B, "max_depth"))]
    skeletons = [tree_skeleton(g, tree_id=i) for i, g in enumerate(grown)]
    leaves = None
    if int(leaves_per_tip) > 0:
        centres = [leaf_centres(g, s, leaves_per_tip, sigma) for g, s in zip(grown, seeds)]
        leaves = [(c, np.full(len(c), leaf_radius, np.float32)) for c in centres]
    rings = [scanner_ring(int(scanners), radius, height, skeleton_box(sk, None if leaves is None else leaves[i]), step_deg, seed=seeds[i],
                          range_noise=range_noise) for i, sk in enumerate(skeletons)]
    cloud, extras = scan_skeletons(skeletons, rings, leaves, form, dev, beams=bool(beams))
    return (cloud, skeletons, extras) if beams else (cloud, skeletons)


# --------------------------------------------------------------------------------------------------------- dataset ---
def _mix64(x: int) -> int:
    """splitmix64's finaliser."""
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def item_seed(seed: int, mode: str, idx: int, epoch: int) -> int:
    """The tree seed of item `idx`: h = mix(seed); h = mix(h ^ m) with m = 0 / 1 / 2 for train / validation / test; h = mix(h ^
    idx); h = mix(h ^ epoch); mix is splitmix64's finaliser on 64 bits, the result is its low 63 bits."""
    h = _mix64(int(seed) & _M64)
    for v in (MODES.index(mode), int(idx), int(epoch)):
        h = _mix64(h ^ (v & _M64))
    return h & ((1 << 63) - 1)


class SyntheticTreeDataset(TreeDataset):
    """`TreeDataset`'s items -- `((inputs, targets), coords, loss_mask, name)` -- from trees generated on the device instead of
    files: item `idx` is the tree `item_seed(seed, mode, idx, epoch)`, through the same augmentation, whole-cloud voxelisation
    and gather.  `epoch` is 0 for validation and test (their trees are fixed) and what `set_epoch` last set in train (fresh
    trees every epoch; a resumed run asks for the same epoch's trees again).  `name` is `synthetic_<mode>_<seed>`.
    `scan`: None, or a dict of `scan_trees` keywords (`scanners`, `step_deg`, `radius`, ...): the item is then the tree as a ring of
    virtual scanners sees it (`scale` and `max_depth` are the dataset's own; `n_points`, `noise` and `foliage_fraction` do not
    apply)."""

    def __init__(self, voxel_size, mode: str, length: int, input_features, target_features, augmentation=None, seed: int = 0,
                 n_points: int = 100_000, scale: float = 1.0, noise: float = 0.002, foliage_fraction: float = 0.3,
                 max_depth: int = 7, device=None, scan=None):
        if mode not in MODES:
            raise ValueError(f"SyntheticTreeDataset: mode must be train / validation / test, got {mode!r}")
        self.voxel_size = voxel_size
        self.mode = mode
        self.length = int(length)
        self.augmentation = augmentation
        self.device = torch.device(device) if device is not None else torch.device("cuda:0")
        self.input_features = list(input_features)
        self.target_features = list(target_features)
        self.seed, self.epoch = int(seed), 0
        self.tree_args = dict(n_points=int(n_points), scale=scale, noise=noise, foliage_fraction=foliage_fraction, max_depth=max_depth)
        self.cache = None
        self.scan = None if scan is None else dict(scan)
        if self.scan is not None and {"scale", "max_depth", "device"} & set(self.scan):
            raise ValueError("SyntheticTreeDataset: scale, max_depth and device are the dataset's own arguments, not keys of scan")

    def set_epoch(self, epoch: int) -> None:
        self.epoch = int(epoch) if self.mode == "train" else 0

    def tree_seed(self, idx: int) -> int:
        return item_seed(self.seed, self.mode, idx, self.epoch)

    def cloud(self, idx: int) -> Cloud:
        if not 0 <= idx < self.length:
            raise IndexError(idx)
        if self.scan is not None:
            cld, _ = scan_trees([self.tree_seed(idx)], scale=self.tree_args["scale"], max_depth=self.tree_args["max_depth"],
                                device=self.device, **self.scan)
        else:
            cld, _ = generate_trees([self.tree_seed(idx)], device=self.device, **self.tree_args)
        cld.seg_off = None  # one tree: a plain cloud, as a file would give
        return cld

    def __getitem__(self, idx):
        return self.process_cloud(self.cloud(idx), f"synthetic_{self.mode}_{self.tree_seed(idx)}")

    def __len__(self) -> int:
        return self.length
