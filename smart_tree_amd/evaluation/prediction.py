"""How good the network's per-point predictions are: confusion matrix, radius and direction error, and the distance between
the predicted and the labelled medial point, per tree of a batch, in one HIP pass (`st_prediction_metrics`,
csrc/prediction_metrics.hip; definitions in DESIGN.md "Evaluation: per-point predictions").

`prediction_tally(preds, targets, mask)` takes what `loss.compute_loss` takes and returns a `PredictionTally`: two device tensors
of per-segment records (int64 counts, float64 sums).  Tallies add (`+`, `.total()`, `.all_reduce(group)`) on the device;
`.metrics()` reads back once and derives the figures.  Counts come from integer atomics and the sums are added in a fixed order,
so a tally is a function of its rows: the same bits run to run, and a tree's record does not depend on its batch.
The reference has no such evaluation.
"""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass, replace

import numpy as np
import torch

DEFAULT_THRESHOLDS = (0.1, 0.25, 0.5, 1.0)
DEFAULT_RADIUS_EDGES = (0.005, 0.01, 0.02, 0.05, 0.1)
N_SCALARS, N_SUMS = 4, 5  # bad_class, vector_rows, bad_vector, rows; sum dr, dr/r, angle, err, err/r


def segment_offsets(indices) -> list:
    """Row offsets [n_seg + 1] of the trees of a collated batch from its `coords[:, 0]`: `batch_collate` writes the item index
    into that column and concatenates the items in order, so the ids must not decrease (an id without rows is an empty
    segment).  Reads the column back."""
    ids = torch.as_tensor(indices).detach().reshape(-1).cpu().long()
    if ids.numel() == 0:
        return [0]
    if int(ids[0]) < 0 or bool((ids[1:] < ids[:-1]).any()):
        raise ValueError("segment_offsets: the batch indices are not contiguous segments in item order (negative or decreasing ids)")
    return [0] + torch.cumsum(torch.bincount(ids), 0).tolist()


@dataclass(frozen=True)
class PredictionTally:
    ints: torch.Tensor  # [n_seg, C*C + 4 + T + NB] int64: confusion | bad_class vector_rows bad_vector rows | within | bin_count
    sums: torch.Tensor  # [n_seg, 5 + 2 NB] float64: dr, dr/r_gt, angle, err, err/r_gt | bin_dr_rel | bin_err_rel
    n_classes: int
    thresholds: tuple
    radius_edges: tuple
    vector_class: object
    target_radius_log: bool

    @property
    def n_seg(self) -> int:
        return self.ints.shape[0]

    def _params(self):
        return (self.n_classes, self.thresholds, self.radius_edges, self.vector_class, self.target_radius_log)

    def __add__(self, other: "PredictionTally") -> "PredictionTally":
        if not isinstance(other, PredictionTally):
            return NotImplemented
        if self._params() != other._params() or self.n_seg != other.n_seg:
            raise ValueError(f"PredictionTally: cannot add tallies with different parameters or segment counts "
                             f"({self._params()}, {self.n_seg} segments; {other._params()}, {other.n_seg} segments)")
        return replace(self, ints=self.ints + other.ints, sums=self.sums + other.sums)

    def segment(self, s: int) -> "PredictionTally":
        if not 0 <= s < self.n_seg:
            raise IndexError(f"PredictionTally: segment {s} of {self.n_seg}")
        return replace(self, ints=self.ints[s:s + 1], sums=self.sums[s:s + 1])

    def total(self) -> "PredictionTally":
        """One segment: the records added in index order."""
        ints, sums = self.ints[:1].clone(), self.sums[:1].clone()
        for s in range(1, self.n_seg):
            ints += self.ints[s:s + 1]
            sums += self.sums[s:s + 1]
        return replace(self, ints=ints, sums=sums)

    def all_reduce(self, group=None) -> "PredictionTally":
        """The ranks' tallies added in rank order (all_gather, then a sum whose order does not depend on arrival)."""
        import torch.distributed as dist

        world = dist.get_world_size(group)
        out = None
        for mine in (self.ints, self.sums):
            got = [torch.empty_like(mine) for _ in range(world)]
            dist.all_gather(got, mine.contiguous(), group=group)
            acc = got[0]
            for t in got[1:]:
                acc = acc + t
            out = (acc,) if out is None else out + (acc,)
        return replace(self, ints=out[0], sums=out[1])

    def metrics(self) -> dict:
        """The figures of the whole tally (its segments added), as plain floats and lists.  One read-back."""
        t = self.total() if self.n_seg != 1 else self
        host = torch.cat([t.ints.reshape(-1), t.sums.reshape(-1).view(torch.int64)]).cpu()
        n_int = t.ints.shape[1]
        return derive_metrics(host[:n_int].tolist(), host[n_int:].view(torch.float64).tolist(), self.n_classes, self.thresholds,
                              self.radius_edges)


def derive_metrics(ints, sums, n_classes: int, thresholds, radius_edges) -> dict:
    """`PredictionTally.metrics()` from one record given as two host lists."""
    C, T, NB = n_classes, len(thresholds), len(radius_edges) + 1
    if len(ints) != C * C + N_SCALARS + T + NB or len(sums) != N_SUMS + 2 * NB:
        raise ValueError(f"derive_metrics: record of {len(ints)} counts and {len(sums)} sums for {C} classes, {T} thresholds, {NB} bins")
    div = lambda a, b: a / b if b else math.nan
    conf = [[int(v) for v in ints[r * C:(r + 1) * C]] for r in range(C)]
    bad_class, vector_rows, bad_vector, rows = (int(v) for v in ints[C * C:C * C + N_SCALARS])
    within = ints[C * C + N_SCALARS:C * C + N_SCALARS + T]
    bin_count = [int(v) for v in ints[C * C + N_SCALARS + T:]]
    tp = [conf[c][c] for c in range(C)]
    n_target = [sum(conf[c]) for c in range(C)]
    n_pred = [sum(conf[r][c] for r in range(C)) for c in range(C)]
    union = [n_target[c] + n_pred[c] - tp[c] for c in range(C)]
    iou = [div(tp[c], union[c]) for c in range(C)]
    seen = [v for v, u in zip(iou, union) if u]
    return {
        "accuracy": div(sum(tp), sum(n_target)),
        "iou": iou,
        "precision": [div(tp[c], n_pred[c]) for c in range(C)],
        "recall": [div(tp[c], n_target[c]) for c in range(C)],
        "miou": div(sum(seen), len(seen)),
        "radius_mae": div(sums[0], vector_rows),
        "radius_rel_error": div(sums[1], vector_rows),
        "direction_angle_deg": math.degrees(div(sums[2], vector_rows)),
        "medial_error": div(sums[3], vector_rows),
        "medial_rel_error": div(sums[4], vector_rows),
        "within": [div(int(w), vector_rows) for w in within],
        "thresholds": [float(v) for v in thresholds],
        "by_radius": {"edges": [float(v) for v in radius_edges], "count": bin_count,
                      "radius_rel_error": [div(sums[N_SUMS + b], bin_count[b]) for b in range(NB)],
                      "medial_rel_error": [div(sums[N_SUMS + NB + b], bin_count[b]) for b in range(NB)]},
        "counts": {"rows": rows, "vector_rows": vector_rows, "bad_class": bad_class, "bad_vector": bad_vector},
        "confusion": conf,
    }


def prediction_tally(preds, targets, mask=None, *, seg_off=None, vector_class=None, target_radius_log=True,
                     thresholds=DEFAULT_THRESHOLDS, radius_edges=DEFAULT_RADIUS_EDGES) -> PredictionTally:
    """`st_prediction_metrics` on what `compute_loss` takes: preds {"radius" [n,1], "direction" [n,3], "class_l" [n,C]}, targets
    [n,5], mask [n] bool or None.  `seg_off`: host row offsets [n_seg + 1] of the trees (`segment_offsets`), None = one segment.
    Half-precision predictions are cast to float32, as the loss does.  Enqueue-only: nothing is read back."""
    from .. import _lib
    from ..model.loss import _prepare

    L = _lib.lib()
    radius, direction, class_l, targets, m, n = _prepare(preds["radius"], preds["direction"], preds["class_l"], targets, mask)
    dev = radius.device
    thresholds = tuple(float(v) for v in thresholds)
    radius_edges = tuple(float(v) for v in radius_edges)
    thr, edges = np.asarray(thresholds, dtype=np.float32), np.asarray(radius_edges, dtype=np.float32)
    C, T, NB = class_l.shape[1], len(thr), len(edges) + 1
    off = None if seg_off is None else np.ascontiguousarray(np.asarray(seg_off, dtype=np.int64).reshape(-1))
    n_seg = 1 if off is None else len(off) - 1
    n_int, n_sum = L.st_prediction_metrics_tally_ints(C, T, NB), L.st_prediction_metrics_tally_sums(NB)
    nbytes = L.st_prediction_metrics_workspace_bytes(n, n_seg, NB)
    # a size beyond the limits comes back as -1: the call below refuses it with the reason
    ints = torch.empty((max(n_seg, 1), max(n_int, 1)), dtype=torch.int64, device=dev)
    sums = torch.empty((max(n_seg, 1), max(n_sum, 1)), dtype=torch.float64, device=dev)
    ws = _lib.workspace(max(nbytes, 0), dev)
    host = lambda a: None if a is None or a.size == 0 else a.ctypes.data_as(ctypes.c_void_p)
    _lib.check(L.st_prediction_metrics(_lib.ptr(radius), _lib.ptr(direction), _lib.ptr(class_l), C, _lib.ptr(targets),
                                       targets.shape[1], _lib.ptr(m), n, host(off), n_seg,
                                       -1 if vector_class is None else int(vector_class), 1 if target_radius_log else 0,
                                       host(thr), T, host(edges), len(edges), _lib.ptr(ints), _lib.ptr(sums), _lib.ptr(ws),
                                       ws.numel(), _lib.stream(dev)))
    return PredictionTally(ints, sums, C, thresholds, radius_edges, None if vector_class is None else int(vector_class),
                           bool(target_radius_log))
