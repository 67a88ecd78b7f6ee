"""Score a skeleton against the ground-truth skeleton of its tree: precision, recall and F-score of the axis.

Both skeletons are sampled every `spacing` along their tubes (`st_sample_tubes_*`), every sample is matched to the nearest
axis of the other skeleton's tubes and the hits under each threshold are counted in the same launch (`st_skeleton_match`,
csrc/skeleton_eval.hip).  A sample is a hit when its distance is at most `threshold x` the GROUND-TRUTH radius there:

  recall[t]     ground-truth samples against the predicted tubes, tolerance t x the ground-truth sample's own radius
  precision[t]  predicted samples against the ground-truth tubes, tolerance t x the ground-truth radius at the projection
  f1[t]         2 P R / (P + R), 0 when P + R = 0;   auc = trapezoid of f1 over the thresholds / (t_max - t_min)

The reference has the pieces (`sample_tubes`, `TreeSkeleton.sample_skeleton`, `point_to_skeleton`) and no evaluation that
runs.  No N x M tensor exists at any point; an evaluation reads back the two sample counts and the two tallies.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from ..data_types.flat import FlatSkeletons
from ..data_types.tube import sample_tubes_device
from .prediction import PredictionTally, derive_metrics, prediction_tally, segment_offsets  # noqa: F401  (per-point predictions)

DEFAULT_THRESHOLDS = tuple(round(0.1 * k, 1) for k in range(1, 11))
MAX_THRESHOLDS = 32


def skeleton_tubes(skeleton):
    """(a [M,3], b [M,3], r1 [M], r2 [M]) float32 host tensors in `to_tubes()` order, for a `TreeSkeleton`, a
    `DisjointTreeSkeleton`, or the flat arrays `save_skeleton_npz` writes (a mapping with `branches` [B,5] = tree, id,
    parent, offset, length; `xyz` [P,3]; `radii` [P]): `FlatSkeletons.tubes` of the one skeleton."""
    flat = FlatSkeletons([skeleton], "skeleton_tubes")
    return tuple(torch.from_numpy(t) for t in flat.tubes(*flat.float32()))


def skeleton_owners(skeleton) -> np.ndarray:
    """int64 [B,4]: (tree, branch id, parent id, number of tubes) of every branch, in `skeleton_tubes` order -- the tubes of a
    branch are contiguous, so the rows say who owns each tube.  `tree` is the tree's index in a `DisjointTreeSkeleton`, 0 for a
    `TreeSkeleton`, the file's tree column for flat arrays; a branch of fewer than two points has no tube."""
    flat = FlatSkeletons([skeleton], "skeleton_owners")
    return np.column_stack([flat.rows[:, 1:4], flat.tubes_of_row])


def branch_key(tree, branch):
    """The id a branch is coloured by (`render.skeleton_items`, `CloudSegmentation.to_cloud`): 31 bits of tree * 65537 + branch."""
    return (tree * 65537 + branch) & 0x7FFFFFFF


def match(pts, rad, a, b, r1, r2, thresholds, ref_mode: int, per_sample: bool = True):
    """`st_skeleton_match` on device tensors: samples (pts [n,3], rad [n]) against tubes (a, b [m,3]; r1, r2 [m]).
    Returns {"hits": int64 [T], "sums": float64 [4]} (device, one buffer) and, with `per_sample`, "dist" [n], "idx" [n] int32,
    "tube_rad" [n].  Nothing is read back."""
    from .. import _lib

    L = _lib.lib()
    dev = pts.device
    f = lambda t: t.to(dev).float().contiguous()
    pts, rad = f(pts).reshape(-1, 3), f(rad).reshape(-1)
    a, b, r1, r2 = f(a).reshape(-1, 3), f(b).reshape(-1, 3), f(r1).reshape(-1), f(r2).reshape(-1)
    thr = f(torch.as_tensor(thresholds, dtype=torch.float32)).reshape(-1)
    n, m, T = pts.shape[0], a.shape[0], thr.shape[0]
    tally = torch.empty(T + 4, dtype=torch.int64, device=dev)
    out = {}
    if per_sample:
        out = {"dist": torch.empty(n, dtype=torch.float32, device=dev), "idx": torch.empty(n, dtype=torch.int32, device=dev),
               "tube_rad": torch.empty(n, dtype=torch.float32, device=dev)}
    nbytes = L.st_skeleton_match_workspace_bytes(n)
    ws = _lib.workspace(nbytes, dev)
    _lib.check(L.st_skeleton_match(_lib.ptr(pts), _lib.ptr(rad), n, _lib.ptr(a), _lib.ptr(b), _lib.ptr(r1), _lib.ptr(r2), m,
                                   _lib.ptr(thr), T, int(ref_mode), _lib.ptr(out.get("dist")), _lib.ptr(out.get("idx")),
                                   _lib.ptr(out.get("tube_rad")), _lib.ptr(tally), _lib.ptr(ws), nbytes, _lib.stream(dev)))
    out["hits"] = tally[:T]
    out["sums"] = tally[T:].view(torch.float64)
    out["tally"] = tally
    return out


def _auc(thresholds, f1):
    if len(thresholds) == 1:
        return float(f1[0])
    t, f = np.asarray(thresholds, np.float64), np.asarray(f1, np.float64)
    return float(np.sum((t[1:] - t[:-1]) * (f[1:] + f[:-1]) * 0.5) / (t.max() - t.min()))


def _lengths(a, b):
    return float((b.double() - a.double()).norm(dim=1).sum()) if a.shape[0] else 0.0


def evaluate_skeleton(pred, gt, spacing: float = 0.001, thresholds=None, device=None) -> dict:
    """Precision / recall / F-score of `pred` against `gt` (anything `skeleton_tubes` takes, or an (a, b, r1, r2) tuple).
    The lists `precision`, `recall`, `f1` are aligned with `thresholds`."""
    thresholds = [float(t) for t in (DEFAULT_THRESHOLDS if thresholds is None else thresholds)]
    if not 1 <= len(thresholds) <= MAX_THRESHOLDS:
        raise ValueError(f"evaluate_skeleton: 1 .. {MAX_THRESHOLDS} thresholds (got {len(thresholds)})")
    if any(t1 <= t0 for t0, t1 in zip(thresholds, thresholds[1:])):
        raise ValueError("evaluate_skeleton: thresholds must increase")
    dev = torch.device(device if device is not None else "cuda:0")
    tubes = lambda s: s if isinstance(s, tuple) and len(s) == 4 else skeleton_tubes(s)
    p_host, g_host = tubes(pred), tubes(gt)
    if g_host[0].shape[0] == 0:
        raise ValueError("evaluate_skeleton: the ground truth has no tubes")
    p_dev, g_dev = [t.to(dev) for t in p_host], [t.to(dev) for t in g_host]
    g_pts, g_rad = sample_tubes_device(*g_dev, spacing)[:2]
    n_gt = g_pts.shape[0]
    if n_gt == 0:
        raise ValueError("evaluate_skeleton: the ground truth has no samples (every tube has zero length)")
    T = len(thresholds)
    out = {"thresholds": thresholds, "spacing": float(spacing), "n_gt": n_gt, "n_pred": 0, "gt_length": _lengths(g_host[0], g_host[1]),
           "pred_length": _lengths(p_host[0], p_host[1]), "precision": [0.0] * T, "recall": [0.0] * T, "f1": [0.0] * T, "auc": 0.0,
           "mean_distance_pred_to_gt": math.nan, "mean_distance_gt_to_pred": math.nan, "radius_rel_error": math.nan}
    if p_host[0].shape[0] == 0:
        return out
    p_pts, p_rad = sample_tubes_device(*p_dev, spacing)[:2]
    n_pred = out["n_pred"] = p_pts.shape[0]
    rec = match(g_pts, g_rad, *p_dev, thresholds, ref_mode=0, per_sample=False)["tally"]
    pre = match(p_pts, p_rad, *g_dev, thresholds, ref_mode=1, per_sample=False)["tally"]
    rec, pre = rec.cpu(), pre.cpu()  # the two read-backs
    rec_hits, rec_sums = rec[:T].tolist(), rec[T:].view(torch.float64).tolist()
    pre_hits, pre_sums = pre[:T].tolist(), pre[T:].view(torch.float64).tolist()
    out["recall"] = [h / n_gt for h in rec_hits]
    out["precision"] = [h / n_pred if n_pred else 0.0 for h in pre_hits]
    out["f1"] = [2.0 * p * r / (p + r) if p + r > 0 else 0.0 for p, r in zip(out["precision"], out["recall"])]
    out["auc"] = _auc(thresholds, out["f1"])
    div = lambda s, c: s / c if c > 0 else math.nan
    out["mean_distance_gt_to_pred"] = div(rec_sums[0], rec_sums[3])
    out["mean_distance_pred_to_gt"] = div(pre_sums[0], pre_sums[3])
    out["radius_rel_error"] = div(pre_sums[2], pre_sums[3])
    return out
