"""`python -m smart_tree_amd.dataset.generate out=<dir> trees=N [points=100000] [scale=1.0] [noise=0.002]
[foliage_fraction=0.3] [max_depth=7] [seed=0] [split=[0.8,0.1,0.1]] [labels=segment] [device=cuda:0] [scan=false [scanners=3]
[step_deg=0.1] [radius=6] [height=1.5] [leaves_per_tip=0] [leaf_radius=0.02] [range_noise=0.002]]`: a folder of labelled
synthetic trees (dataset/synthetic.py) that `TreeDataset`, `train-smart-tree` and `smart_tree_amd.evaluate` read.

Tree i has the seed `seed + i` and is written as
* `tree_<seed>.npz`: xyz, rgb, medial_vector, class_l, branch_ids (`util.file.load_cloud`),
* `tree_<seed>_skeleton.npz`: its ground-truth skeleton (`util.file.save_skeleton`; `evaluate`'s `gt=`),
and `split.json` lists the cloud files as `{"train": [...], "validation": [...], "test": [...]}`: the first
round(split[0] * N) trees train, the next round(split[1] * N) validate, the rest test.  Trees are generated 64 to a launch.
`scan=true` writes the trees as a ring of virtual laser scanners sees them (`dataset.synthetic.scan_trees`; `points`, `noise`,
`foliage_fraction` and `labels` then do not apply).  Overrides are parsed by config.py, as for the training run.
"""
from __future__ import annotations

import json
import sys
from pathlib import Path

from ..config import apply_overrides
from .synthetic import MAX_TREES, generate_trees, scan_trees

DEFAULTS = {"out": None, "trees": None, "points": 100_000, "scale": 1.0, "noise": 0.002, "foliage_fraction": 0.3, "max_depth": 7,
            "seed": 0, "split": [0.8, 0.1, 0.1], "labels": "segment", "device": "cuda:0",
            "scan": False, "scanners": 3, "step_deg": 0.1, "radius": 6.0, "height": 1.5, "leaves_per_tip": 0, "leaf_radius": 0.02,
            "range_noise": 0.002}


def main(argv=None) -> dict:
    from ..util.file import save_cloud, save_skeleton

    cfg = apply_overrides(dict(DEFAULTS), argv if argv is not None else sys.argv[1:])
    unknown = sorted(set(cfg) - set(DEFAULTS))
    if unknown or cfg["out"] is None or cfg["trees"] is None:
        raise SystemExit("usage: python -m smart_tree_amd.dataset.generate out=<dir> trees=N [points=] [scale=] [noise=] "
                         "[foliage_fraction=] [max_depth=] [seed=] [split=[train,validation,test]] [labels=segment|nearest] [device=] "
                         "[scan=true [scanners=] [step_deg=] [radius=] [height=] [leaves_per_tip=] [leaf_radius=] [range_noise=]]"
                         + (f"  (unknown: {', '.join(unknown)})" if unknown else ""))
    split = [float(x) for x in cfg["split"]]
    if len(split) != 3 or min(split) < 0 or abs(sum(split) - 1.0) > 1e-6:
        raise SystemExit(f"generate: split must be three non-negative shares that add up to 1, got {cfg['split']}")
    out = Path(str(cfg["out"]))
    out.mkdir(parents=True, exist_ok=True)
    n = int(cfg["trees"])
    seeds = [int(cfg["seed"]) + i for i in range(n)]
    names = []
    scan = str(cfg["scan"]).lower() in ("true", "1", "yes", "on")
    for lo in range(0, n, MAX_TREES):
        batch = seeds[lo:lo + MAX_TREES]
        if scan:
            cloud, skeletons = scan_trees(batch, int(cfg["scanners"]), step_deg=float(cfg["step_deg"]), radius=float(cfg["radius"]),
                                          height=float(cfg["height"]), scale=float(cfg["scale"]), max_depth=int(cfg["max_depth"]),
                                          leaves_per_tip=int(cfg["leaves_per_tip"]), leaf_radius=float(cfg["leaf_radius"]),
                                          range_noise=float(cfg["range_noise"]), device=cfg["device"])
        else:
            cloud, skeletons = generate_trees(batch, int(cfg["points"]), scale=float(cfg["scale"]), noise=float(cfg["noise"]),
                                              foliage_fraction=float(cfg["foliage_fraction"]), max_depth=int(cfg["max_depth"]),
                                              labels=cfg["labels"], device=cfg["device"])
        for s, cld, skeleton in zip(batch, cloud.split(), skeletons):
            save_cloud(out / f"tree_{s}.npz", cld)
            save_skeleton(skeleton, out / f"tree_{s}_skeleton.npz")
            names.append(f"tree_{s}.npz")
    n_train, n_val = round(split[0] * n), round(split[1] * n)
    n_val = min(n_val, n - n_train)
    parts = {"train": names[:n_train], "validation": names[n_train:n_train + n_val], "test": names[n_train + n_val:]}
    (out / "split.json").write_text(json.dumps(parts, indent=1))
    print(f"{n} trees " + (f"scanned from {int(cfg['scanners'])} positions" if scan else f"of {int(cfg['points'])} points") + f" in {out}: {len(parts['train'])} train, {len(parts['validation'])} validation, "
          f"{len(parts['test'])} test")
    return {"out": out, "split": parts}


if __name__ == "__main__":
    main()
