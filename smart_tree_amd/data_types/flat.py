"""The skeletons of a call as one flat host-side table: the one place that asks what kind of skeleton it was given.

A skeleton reaches `evaluate_skeleton`, `segment_cloud`, `refine_skeleton`, `measure_trees` and `render.skeleton_items` as a
`TreeSkeleton`, a `DisjointTreeSkeleton`, or the flat arrays `save_skeleton_npz` writes (a mapping with `branches` [B,5] = tree, id,
parent, offset, length; `xyz` [P,3]; `radii` [P]).  `FlatSkeletons` walks a list of them, one per cloud, once: the branches in the
order the input gives them (no regrouping), the tubes of a branch contiguous, so a tube's index is the same number for every
consumer and one row says who owns it.
"""
from __future__ import annotations

import numpy as np
import torch

from .branch import BranchSkeleton
from .cloud import Cloud
from .tree import DisjointTreeSkeleton, TreeSkeleton


def _walk(skeleton, caller):
    """([(tree, label)], [(tree, label, branch id, parent id, child id, vertices, radii were [n,1])], xyz [P,3], radii [P]) of one
    skeleton: its trees in the order of their first appearance (a tree object without branches included), its branches in input
    order and their vertices in that order, float64.  `tree` is the tree's index in a `DisjointTreeSkeleton`, 0 for a
    `TreeSkeleton`, the file's tree column for flat arrays; `label` is the tree's own `_id` (the file's column again)."""
    if isinstance(skeleton, (TreeSkeleton, DisjointTreeSkeleton)):
        members = [(0, skeleton)] if isinstance(skeleton, TreeSkeleton) else list(enumerate(skeleton.skeletons))
        found = [(t, int(s._id), int(k), b) for t, s in members for k, b in s.branches.items()]
        # one concatenation and one cast for the whole skeleton: a branch is a few vertices, a cloud has hundreds of branches
        cat = lambda parts, shape: torch.cat([torch.as_tensor(p).detach().cpu().reshape(shape) for p in parts]).double().numpy()
        return ([(t, int(s._id)) for t, s in members],
                [(t, lab, k, int(b.parent_id), b.child_id, len(b.xyz), torch.as_tensor(b.radii).ndim == 2) for t, lab, k, b in found],
                cat([b.xyz for _, _, _, b in found], (-1, 3)) if found else np.zeros((0, 3)),
                cat([b.radii for _, _, _, b in found], (-1,)) if found else np.zeros(0))
    try:
        rows, xyz, radii = skeleton["branches"], skeleton["xyz"], skeleton["radii"]
    except (KeyError, TypeError, IndexError):
        raise TypeError(f"{caller}: a TreeSkeleton, a DisjointTreeSkeleton or flat branches / xyz / radii arrays, got {type(skeleton).__name__}")
    rows = np.asarray(rows, np.int64).reshape(-1, 5)
    xyz, radii = np.asarray(xyz, np.float64).reshape(-1, 3), np.asarray(radii, np.float64).reshape(-1)
    first = np.concatenate([[0], np.cumsum(rows[:, 4])])
    vertex = np.repeat(rows[:, 3] - first[:-1], rows[:, 4]) + np.arange(first[-1])  # the file's offsets need not be in order
    return ([(t, t) for t in dict.fromkeys(rows[:, 0].tolist())], [(t, t, b, p, None, n, True) for t, b, p, _, n in rows.tolist()],
            xyz[vertex], radii[vertex])


class FlatSkeletons:
    """`rows` int64 [B,6] = cloud, tree, branch id, parent id, vertex offset, vertices, in `skeleton_owners` order; `xyz` [P,3] and
    `radii` [P] float64 (every float32 exactly: `float32()` is the input's own bits).  Per branch: `label` [B] (the tree's own id,
    to rebuild and to save with), `child` (list), `column` [B] (whether `radii` was [n,1]).  `trees`: per cloud its [(tree, label)].
    Derived: `tubes_of_row` [B]; `tube_first` [B + 1], the first tube of every row; `tube_start` [M], the first vertex of every tube;
    `tube_off` [clouds + 1]; `tree_rows` int64 [T,2] = (cloud, tree) in the order of their first branch; `tree_of_branch` [B]."""

    def __init__(self, skeletons, caller="FlatSkeletons"):
        rows, label, self.child, column, xyz, radii, self.trees, off = [], [], [], [], [np.zeros((0, 3))], [np.zeros(0)], [], 0
        for c, sk in enumerate(skeletons):
            trees, branches, sx, sr = _walk(sk, caller)
            self.trees.append(trees)
            xyz.append(sx)
            radii.append(sr)
            for tree, lab, bid, parent, child, n, col in branches:
                rows.append((c, tree, bid, parent, off, n))
                label.append(lab)
                self.child.append(child)
                column.append(col)
                off += n
        self.n_clouds = len(self.trees)
        self.rows = np.asarray(rows, np.int64).reshape(-1, 6)
        self.label, self.column = np.asarray(label, np.int64), np.asarray(column, bool)
        self.xyz, self.radii = np.concatenate(xyz), np.concatenate(radii)
        self.tubes_of_row = np.maximum(self.rows[:, 5] - 1, 0)
        self.tube_first = np.concatenate([[0], np.cumsum(self.tubes_of_row)]).astype(np.int64)
        self.tube_start = np.repeat(self.rows[:, 4] - self.tube_first[:-1], self.tubes_of_row) + np.arange(self.tube_first[-1])
        self.tube_off = self.tube_first[np.searchsorted(self.rows[:, 0], np.arange(self.n_clouds + 1))]
        seen = {}
        self.tree_of_branch = np.asarray([seen.setdefault((c, t), len(seen)) for c, t in self.rows[:, :2].tolist()], np.int64)
        self.tree_rows = np.asarray(list(seen), np.int64).reshape(-1, 2)

    def float32(self):
        """(xyz, radii) float32: what the kernels take."""
        return self.xyz.astype(np.float32), self.radii.astype(np.float32)

    def tubes(self, xyz=None, radii=None):
        """(a [M,3], b [M,3], r1 [M], r2 [M]) in `to_tubes()` order, of the table's own vertices or of `xyz`, `radii` in their place."""
        xyz, radii, s = self.xyz if xyz is None else xyz, self.radii if radii is None else radii, self.tube_start
        return xyz[s], xyz[s + 1], radii[s], radii[s + 1]

    def rebuild(self, xyz, radii) -> list:
        """One `DisjointTreeSkeleton` per cloud with `xyz`, `radii` as its vertices: the same trees (their own ids, in order of first
        appearance), branch ids, parents, children and vertex counts, and the radii in the shape they came in."""
        mine = {}
        for (c, tree, bid, parent, o, n), child, column in zip(self.rows.tolist(), self.child, self.column.tolist()):
            br = BranchSkeleton(bid, parent, torch.from_numpy(xyz[o:o + n].copy()), torch.from_numpy(radii[o:o + n].copy()).reshape(-1, 1), child)
            if not column:  # `smooth` leaves the radii of the branches it touched as [n]
                br.radii = br.radii.reshape(-1)
            mine.setdefault((c, tree), {})[bid] = br
        return [DisjointTreeSkeleton([TreeSkeleton(lab, mine.get((c, tree), {})) for tree, lab in trees]) for c, trees in enumerate(self.trees)]


def points_and_skeletons(cloud_or_xyz, skeleton, device, caller):
    """The arguments `segment_cloud`, `refine_skeleton` and `measure_trees` share: a `Cloud` or [n,3] points with one skeleton, or a
    collated `Cloud` with a list of them, one per cloud.  Returns (points float32 [n,3] on the device, `seg_off` or None, the list of
    skeletons, whether a list was given, the number of clouds)."""
    if isinstance(cloud_or_xyz, Cloud):
        xyz, seg_off = cloud_or_xyz.xyz, cloud_or_xyz.seg_off
    else:
        xyz, seg_off = torch.as_tensor(np.asarray(cloud_or_xyz) if not torch.is_tensor(cloud_or_xyz) else cloud_or_xyz), None
    dev = torch.device(device) if device is not None else xyz.device
    many = isinstance(skeleton, (list, tuple))
    skeletons = list(skeleton) if many else [skeleton]
    n_clouds = 1 if seg_off is None else int(seg_off.shape[0]) - 1
    if len(skeletons) != n_clouds:
        raise ValueError(f"{caller}: {len(skeletons)} skeleton(s) for {n_clouds} cloud(s); a collated Cloud takes a list, one per cloud")
    return xyz.to(dev).float().reshape(-1, 3).contiguous(), seg_off, skeletons, many, n_clouds
