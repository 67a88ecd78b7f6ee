"""Refine a skeleton on its points: every tube fitted to the points segmented onto it (csrc/fit.hip).

`python -m smart_tree_amd.refine cloud=<.npz|.ply> skeleton=<skeleton.npz> out=<dir|.npz> [iterations=2] [max_distance=]
[max_relative=0.5] [centre=false] [classes=[0]] [device=cuda:0]` writes the refined skeleton (`skeleton.npz`, the flat arrays of
`save_skeleton_npz`, and `skeleton_fit.npz` when `out` is a directory; the flat arrays alone when it is an `.npz`) and prints the
share of tubes fully fitted / radius only / not fitted, the points used and the mean relative radius change.  `classes` keeps the
points of these classes when the cloud carries `class_l` (foliage does not belong on a cylinder); `centre=true` runs `CentreCloud`
first, as for `segmentation`.  Overrides are parsed by config.py.

The skeleton's radii are the network's per-point prediction carried through the graph; `smooth` is their only correction.
`refine_skeleton` is the step cylinder-model tools for scanned trees take after their first guess: per iteration the points are
segmented onto the tubes (`st_segment_points_seg`), every tube gets one Gauss-Newton step of the geometric circle fit from ten
integer moments of its points (`st_fit_tubes`; include/smarttree_hip.h states the contract), the per-tube answers are read back once
and the vertices are updated on the host.  Integer moments: the same bits in every run, for a batch and for its clouds alone.

Known limits: a tube takes one radius, at its points' mean position (the taper inside a 1-5 cm tube is ignored); junctions and the
first tube of a repaired branch, which lies inside its parent, fit poorly and are only protected by `max_ratio` and the move limit;
there is no taper or monotonicity constraint along a branch.
"""
from __future__ import annotations

from dataclasses import dataclass
from pathlib import Path
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from .data_types.flat import FlatSkeletons, points_and_skeletons

FIT_COLUMNS = ("points", "radius", "offset_x", "offset_y", "offset_z", "rms", "spread", "status")
BRANCH_COLUMNS = ("cloud", "tree", "branch", "parent", "tubes", "fitted_tubes", "points", "mean_rms", "mean_radius_change")
MOMENTS = 10


def fit_tubes(pts, tube, a, b, r1, r2, max_relative=0.5, min_points=8, min_spread=0.01, moments=False) -> dict:
    """`st_fit_tubes` on device tensors: pts [n,3] with their tubes `tube` [n] int32 (what `segment_points` returned) against the
    tubes a, b [m,3], r1, r2 [m].  Returns "fit" float64 [m,8] (FIT_COLUMNS) and, when asked, "moments" int64 [m,10]."""
    L = _lib.lib()
    dev = pts.device
    f = lambda t, shape: t.to(dev).float().reshape(shape).contiguous()
    pts, a, b, r1, r2 = f(pts, (-1, 3)), f(a, (-1, 3)), f(b, (-1, 3)), f(r1, (-1,)), f(r2, (-1,))
    tube = tube.to(dev).to(torch.int32).reshape(-1).contiguous()
    n, m = pts.shape[0], a.shape[0]
    if tube.shape[0] != n or b.shape[0] != m or r1.shape[0] != m or r2.shape[0] != m:
        raise ValueError(f"fit_tubes: {n} points with {tube.shape[0]} tube ids; {m} tubes with {b.shape[0]} ends and {r1.shape[0]}, {r2.shape[0]} radii")
    out = {"fit": torch.empty((m, 8), dtype=torch.float64, device=dev)}
    if moments:
        out["moments"] = torch.empty((m, MOMENTS), dtype=torch.int64, device=dev)
    nbytes = L.st_fit_tubes_workspace_bytes(n, m)
    if nbytes < 0:
        raise _lib.StError(f"fit_tubes: {n} points and {m} tubes are outside what the call takes")
    ws = _lib.workspace(nbytes, dev)
    p = lambda t: _lib.ptr(t) if t is not None and t.numel() else None
    _lib.check(L.st_fit_tubes(p(pts), n, p(tube), p(a), p(b), p(r1), p(r2), m, float(max_relative), int(min_points), float(min_spread),
                              p(out.get("moments")), p(out["fit"]), _lib.ptr(ws), ws.numel(), _lib.stream(dev)))
    return out


# ------------------------------------------------------------------------------------------------ host side ---
class VertexLinks(NamedTuple):
    """Per vertex of a `FlatSkeletons`: the tubes it ends (`lo`) and begins (`hi`), -1 for none -- vertex i of a branch touches its
    tubes i - 1 and i -- and `pinned`: the first vertex of a branch with a parent, the connection point `repair` put on the
    parent's axis."""
    lo: np.ndarray
    hi: np.ndarray
    pinned: np.ndarray


def vertex_links(flat: FlatSkeletons) -> VertexLinks:
    P, tube = len(flat.xyz), np.arange(len(flat.tube_start))
    lo, hi, pinned = np.full(P, -1, np.int64), np.full(P, -1, np.int64), np.zeros(P, bool)
    hi[flat.tube_start], lo[flat.tube_start + 1] = tube, tube
    rows = flat.rows.tolist()
    known = {(c, tr, bid) for c, tr, bid, _, _, _ in rows}
    for c, tr, bid, parent, o, n in rows:
        if n and parent != bid and (c, tr, parent) in known:
            pinned[o] = True
    return VertexLinks(lo, hi, pinned)


def update_vertices(links: VertexLinks, xyz, radii, xyz0, radii0, fit, max_ratio=2.0, move_axis=True):
    """One vertex update from a per-tube table `fit` [m,8]: (new xyz, new radii) float32.  A vertex's radius becomes the N-weighted mean
    of R over its (at most two) tubes with status >= 1, kept within [prior / max_ratio, prior * max_ratio]; its position moves by the
    N-weighted mean offset over those with status 2 and stays within one prior radius of the prior position; the prior is the input
    skeleton (xyz0, radii0).  Without a fitted tube a vertex keeps both; a pinned vertex keeps its position."""
    pad = np.concatenate([np.asarray(fit, np.float64).reshape(-1, 8), np.zeros((1, 8))])  # the last row is what "no tube" (-1) indexes
    n_r, n_m = pad[:, 0] * (pad[:, 7] >= 1), pad[:, 0] * (pad[:, 7] == 2)
    lo, hi = links.lo, links.hi
    r0 = radii0.astype(np.float64)
    new_r, new_x = radii.astype(np.float64), xyz.astype(np.float64)
    w = n_r[lo] + n_r[hi]
    ok = (w > 0) & (r0 > 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean_r = (n_r[lo] * pad[lo, 1] + n_r[hi] * pad[hi, 1]) / w
        mean_r = np.minimum(np.maximum(mean_r, r0 / max_ratio), r0 * max_ratio)
    new_r = np.where(ok & np.isfinite(mean_r), mean_r, new_r)
    if move_axis:
        w = n_m[lo] + n_m[hi]
        with np.errstate(invalid="ignore", divide="ignore"):
            move = (n_m[lo, None] * pad[lo, 2:5] + n_m[hi, None] * pad[hi, 2:5]) / w[:, None]
            d = new_x + move - xyz0.astype(np.float64)  # from the prior position
            far = np.sqrt((d * d).sum(1))
            d = np.where((far > r0)[:, None], d * (r0 / far)[:, None], d)
        ok = (w > 0) & (r0 > 0) & ~links.pinned & np.isfinite(d).all(1)
        new_x = np.where(ok[:, None], xyz0.astype(np.float64) + d, new_x)
    return new_x.astype(np.float32), new_r.astype(np.float32)


@dataclass
class SkeletonFit:
    """`tubes`: float64 [m,8], the last iteration's row of every tube in `skeleton_tubes` order (FIT_COLUMNS: points used, fitted
    radius, offset of the axis, rms of the linear residual, spread of the points' directions, status 0 not fitted / 1 radius only /
    2 full fit).  `branches`: float64 [B,9], BRANCH_COLUMNS (mean_rms over the fitted tubes, mean_radius_change = the mean of
    (refined - input) / input over the branch's vertices; NaN where there is nothing to average).  `tube_off` [clouds + 1]."""
    tubes: np.ndarray
    branches: np.ndarray
    tube_off: np.ndarray
    iterations: int = 0

    def split(self) -> list:
        """The clouds of a batch, each as its own call gives it."""
        out = []
        for k in range(len(self.tube_off) - 1):
            rows = self.branches[self.branches[:, 0] == k].copy()
            rows[:, 0] = 0
            t0, t1 = int(self.tube_off[k]), int(self.tube_off[k + 1])
            out.append(SkeletonFit(self.tubes[t0:t1], rows, np.asarray([0, t1 - t0], np.int64), self.iterations))
        return out

    def save(self, path) -> None:
        path = Path(path)
        path.parent.mkdir(parents=True, exist_ok=True)
        np.savez(path, tubes=self.tubes, branches=self.branches, tube_off=self.tube_off, iterations=np.int64(self.iterations))

    @staticmethod
    def load(path) -> "SkeletonFit":
        with np.load(path) as z:
            return SkeletonFit(z["tubes"], z["branches"], z["tube_off"], int(z["iterations"]))


def _branch_table(flat: FlatSkeletons, fit, radii0, radii) -> np.ndarray:
    rows = flat.rows
    out = np.full((len(rows), 9), np.nan)
    if not len(rows):
        return out
    out[:, :4] = rows[:, :4]
    out[:, 4] = flat.tubes_of_row
    row_of_tube = np.repeat(np.arange(len(rows)), flat.tubes_of_row)
    fitted = fit[:, 7] >= 1
    count = lambda weights: np.bincount(row_of_tube, weights=weights, minlength=len(rows))
    out[:, 5] = count(fitted.astype(np.float64))
    out[:, 6] = count(np.where(fitted, fit[:, 0], 0.0))
    with np.errstate(invalid="ignore", divide="ignore"):
        out[:, 7] = count(np.where(fitted, fit[:, 5], 0.0)) / out[:, 5]
        change = (radii.astype(np.float64) - radii0) / radii0
    row_of_vertex = np.repeat(np.arange(len(rows)), rows[:, 5])
    good = np.isfinite(change)
    with np.errstate(invalid="ignore", divide="ignore"):
        out[:, 8] = np.bincount(row_of_vertex[good], weights=change[good], minlength=len(rows)) / np.bincount(row_of_vertex[good], minlength=len(rows))
    return out


def refine_skeleton(cloud_or_xyz, skeleton, iterations=2, max_distance=None, max_relative=0.5, min_points=8, min_spread=0.01,
                    max_ratio=2.0, move_axis=True, form="auto", device=None):
    """Fit the vertices of `skeleton` to the points it was made from.  Takes what `segment_cloud` takes: a `Cloud` or [n,3] points
    with a `TreeSkeleton`, a `DisjointTreeSkeleton` or the flat arrays of `save_skeleton_npz`; a collated `Cloud` with a list of
    skeletons, one per cloud (one segmentation call and one fit call per iteration for the whole batch).  Returns
    (`DisjointTreeSkeleton` or a list of them -- same ids, parents and vertex counts; the input is not modified --, `SkeletonFit`)."""
    from .segmentation import segment_points

    pts, seg_off, skeletons, many, _ = points_and_skeletons(cloud_or_xyz, skeleton, device, "refine_skeleton")
    dev = pts.device
    if int(iterations) < 0:
        raise ValueError(f"refine_skeleton: iterations must be >= 0, got {iterations}")
    if not max_ratio >= 1.0:
        raise ValueError(f"refine_skeleton: max_ratio must be >= 1, got {max_ratio}")
    flat = FlatSkeletons(skeletons, "refine_skeleton")
    links = vertex_links(flat)
    batched = seg_off is not None
    pt_off = seg_off if batched else None
    tube_off = torch.from_numpy(flat.tube_off.astype(np.int32)) if batched else None
    xyz0, radii0 = flat.float32()
    cur_xyz, cur_r = xyz0.copy(), radii0.copy()
    m = len(flat.tube_start)
    fit = np.zeros((m, 8))
    for _ in range(int(iterations)):
        a, b, r1, r2 = (torch.from_numpy(np.ascontiguousarray(t)).to(dev) for t in flat.tubes(cur_xyz, cur_r))
        seg = segment_points(pts, a, b, r1, r2, pt_off, tube_off, max_distance, form, tally=False, outputs=("tube",))
        res = fit_tubes(pts, seg["tube"], a, b, r1, r2, max_relative, min_points, min_spread)
        fit = res["fit"].cpu().numpy()  # the one read-back of an iteration
        cur_xyz, cur_r = update_vertices(links, cur_xyz, cur_r, xyz0, radii0, fit, max_ratio, move_axis)
    report = SkeletonFit(fit, _branch_table(flat, fit, flat.radii, cur_r), flat.tube_off, int(iterations))
    out = flat.rebuild(cur_xyz, cur_r)
    return (out if many else out[0]), report


def summary(fit: SkeletonFit) -> str:
    m = len(fit.tubes)
    share = lambda s: 100.0 * float((fit.tubes[:, 7] == s).sum()) / max(m, 1)
    change = fit.branches[:, 8] if len(fit.branches) else np.zeros(0)
    weight = fit.branches[:, 4] + 1 if len(fit.branches) else np.zeros(0)  # vertices of the branch
    good = np.isfinite(change)
    mean = float((change[good] * weight[good]).sum() / weight[good].sum()) if good.any() else float("nan")
    used = int(fit.tubes[fit.tubes[:, 7] >= 1, 0].sum())
    return (f"{m} tubes: {share(2):.1f} % full fit, {share(1):.1f} % radius only, {share(0):.1f} % not fitted\n"
            f"points used: {used}\nmean relative radius change: {100.0 * mean:+.2f} %")


# ---------------------------------------------------------------------------------------------------------------- cli ---
DEFAULTS = {"cloud": None, "skeleton": None, "out": None, "iterations": 2, "max_distance": None, "max_relative": 0.5, "centre": False,
            "classes": [0], "device": "cuda:0"}
USAGE = ("usage: python -m smart_tree_amd.refine cloud=<.npz|.ply> skeleton=<skeleton.npz> out=<dir|.npz> [iterations=2] "
         "[max_distance=] [max_relative=0.5] [centre=false] [classes=[0]] [device=]")


def main(argv=None):
    from .config import cloud_command
    from .evaluate import load_any_skeleton
    from .util.file import save_skeleton_npz

    cfg, dev, cloud = cloud_command(argv, DEFAULTS, USAGE)
    if cloud.class_l is not None and cfg["classes"] is not None:
        classes = cfg["classes"] if isinstance(cfg["classes"], (list, tuple)) else [cfg["classes"]]
        cloud = cloud.filter_by_class([int(c) for c in classes])
    refined, fit = refine_skeleton(cloud, load_any_skeleton(cfg["skeleton"]), iterations=int(cfg["iterations"]),
                                   max_distance=None if cfg["max_distance"] is None else float(cfg["max_distance"]),
                                   max_relative=float(cfg["max_relative"]), device=dev)
    out = Path(str(cfg["out"]))
    if out.suffix == ".npz":
        save_skeleton_npz(out, refined)
    else:
        save_skeleton_npz(out / "skeleton.npz", refined)
        fit.save(out / "skeleton_fit.npz")
    print(summary(fit))
    return refined, fit


if __name__ == "__main__":
    main()
