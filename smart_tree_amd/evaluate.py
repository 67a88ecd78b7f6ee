"""`python -m smart_tree_amd.evaluate pred=<file|dir> gt=<file|dir> [spacing=0.001] [thresholds=[0.1,...]]
[out=metrics.json] [device=cuda:0]`: score skeletons against the ground truth of their trees (smart_tree_amd/evaluation).

`gt` is any `.npz` with the reference's skeleton keys (`skeleton_xyz`, `skeleton_radii`, `branch_*`): a dataset tree or a
`save_skeleton` file.  `pred` is that layout or the flat `branches` / `xyz` / `radii` file the pipeline writes
(`save_skeleton_npz`).  Two directories are paired by file stem; a file without a partner is reported and skipped.  One line per
tree goes to stdout, the per-tree metrics and their mean to `out` as JSON.  Overrides are parsed by config.py, as for the
training run.
"""
from __future__ import annotations

import json
import sys
from pathlib import Path

import numpy as np

from .config import apply_overrides
from .evaluation import evaluate_skeleton

DEFAULTS = {"pred": None, "gt": None, "spacing": 0.001, "thresholds": None, "out": "metrics.json", "device": "cuda:0"}


def load_any_skeleton(path):
    """A `TreeSkeleton` (reference layout) or the flat arrays of `save_skeleton_npz`, by the keys the file holds."""
    from .util.file import load_skeleton

    with np.load(path) as z:
        keys = set(z.files)
        if "skeleton_xyz" in keys:
            return load_skeleton(path)
        if {"branches", "xyz", "radii"} <= keys:
            return {k: z[k] for k in ("branches", "xyz", "radii")}
    raise ValueError(f"{path}: neither the reference's skeleton keys (skeleton_xyz, ...) nor branches / xyz / radii")


def _files(path):
    path = Path(path)
    if path.is_dir():
        return {p.stem: p for p in sorted(path.glob("*.npz"))}
    if not path.is_file():
        raise FileNotFoundError(f"evaluate: {path} is neither a file nor a directory")
    return {path.stem: path}


def _mean(rows, key):
    vals = np.asarray([r[key] for r in rows], dtype=np.float64)
    keep = ~np.isnan(vals).reshape(len(rows), -1).any(1)  # a tree without a prediction has no mean distance
    if not keep.any():
        return float("nan")
    m = vals[keep].mean(0)
    return m.tolist() if m.ndim else float(m)


def main(argv=None) -> dict:
    cfg = apply_overrides(dict(DEFAULTS), argv if argv is not None else sys.argv[1:])
    unknown = sorted(set(cfg) - set(DEFAULTS))
    if unknown or cfg["pred"] is None or cfg["gt"] is None:
        raise SystemExit(f"usage: python -m smart_tree_amd.evaluate pred=<file|dir> gt=<file|dir> [spacing=] [thresholds=[...]] "
                         f"[out=metrics.json] [device=]" + (f"  (unknown: {', '.join(unknown)})" if unknown else ""))
    pred, gt = _files(cfg["pred"]), _files(cfg["gt"])
    if len(pred) == 1 and len(gt) == 1 and Path(cfg["pred"]).is_file() and Path(cfg["gt"]).is_file():
        pairs = {next(iter(gt)): (next(iter(pred.values())), next(iter(gt.values())))}  # two files: paired whatever their names
        skipped = []
    else:
        pairs = {s: (pred[s], gt[s]) for s in sorted(set(pred) & set(gt))}
        skipped = sorted(set(pred) ^ set(gt))
    for s in skipped:
        print(f"{s}: skipped, no {'ground truth' if s in pred else 'prediction'} with this stem")
    trees = {}
    for stem, (p, g) in pairs.items():
        r = evaluate_skeleton(load_any_skeleton(p), load_any_skeleton(g), spacing=float(cfg["spacing"]),
                              thresholds=cfg["thresholds"], device=cfg["device"])
        trees[stem] = r
        mid = len(r["thresholds"]) // 2
        print(f"{stem}: auc {r['auc']:.4f}  f1@{r['thresholds'][mid]:g} {r['f1'][mid]:.4f}  precision {r['precision'][mid]:.4f}  "
              f"recall {r['recall'][mid]:.4f}  pred->gt {r['mean_distance_pred_to_gt']:.5f}  gt->pred {r['mean_distance_gt_to_pred']:.5f}  "
              f"radius error {r['radius_rel_error']:.4f}  samples {r['n_pred']} / {r['n_gt']}")
    rows = list(trees.values())
    keys = ("precision", "recall", "f1", "auc", "mean_distance_pred_to_gt", "mean_distance_gt_to_pred", "radius_rel_error",
            "n_pred", "n_gt", "pred_length", "gt_length")
    result = {"trees": trees, "mean": {k: _mean(rows, k) for k in keys} if rows else {}, "skipped": skipped}
    if rows:
        result["mean"]["thresholds"] = rows[0]["thresholds"]
        print(f"mean of {len(rows)}: auc {result['mean']['auc']:.4f}")
    if cfg["out"]:
        out = Path(str(cfg["out"]))
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text(json.dumps(result, indent=1))
    return result


if __name__ == "__main__":
    main()
