"""`python -m smart_tree_amd.model.evaluate weights=<.pt> [config=training|training_synthetic] [directory= json_path=]
[split=test] [fp16=false] [out=prediction_metrics.json] [key=value ...]`: the per-point prediction metrics of trained weights on
one split of the training run's data (smart_tree_amd/evaluation/prediction.py).

The split's loader and the model are built from the training configuration the way `train.run` builds them (same overrides,
parsed by config.py); `weights` is either file the run writes, `<run_name>_model_weights.pt` or `last.pt`.  The split runs in
eval mode with one segment per tree: one line per tree goes to stdout, `{"trees": {name: metrics}, "total": metrics}` to `out`.
"""
from __future__ import annotations

import json
import sys
from pathlib import Path

import torch

from ..config import apply_overrides, instantiate, load_yaml
from ..evaluation.prediction import prediction_tally, segment_offsets
from . import train as T
from .sparse import sparse_from_batch

OWN = {"weights": None, "split": "test", "out": "prediction_metrics.json"}
SPLITS = ("train", "validation", "test")
USAGE = ("usage: python -m smart_tree_amd.model.evaluate weights=<.pt> [config=training|training_synthetic] [directory= json_path=] "
         "[split=test] [fp16=false] [out=prediction_metrics.json] [key=value ...]")


def _top(item: str) -> str:
    return item.lstrip("+").partition("=")[0].split(".")[0]


def load_weights(path) -> dict:
    """The model's state_dict from `<run_name>_model_weights.pt` (the state_dict itself) or `last.pt` (under "model")."""
    state = torch.load(path, map_location="cpu", weights_only=True)
    if isinstance(state, dict) and isinstance(state.get("model"), dict):
        state = state["model"]
    return state


def _line(name, m) -> str:
    at = m["thresholds"].index(0.5) if 0.5 in m["thresholds"] else len(m["thresholds"]) // 2
    within = f"  within {m['thresholds'][at]:g} r: {m['within'][at]:.4f}" if m["thresholds"] else ""
    return (f"{name}: miou {m['miou']:.4f}  radius error {m['radius_mae'] * 1000:.2f} mm ({m['radius_rel_error']:.4f} rel)  "
            f"medial error {m['medial_error'] * 1000:.2f} mm ({m['medial_rel_error']:.4f} rel){within}  "
            f"rows {m['counts']['rows']}")


@torch.no_grad()
def main(argv=None) -> dict:
    argv = list(sys.argv[1:] if argv is None else argv)
    own = apply_overrides(dict(OWN), [a for a in argv if _top(a) in OWN])
    rest = [a for a in argv if _top(a) not in OWN]
    named = [str(a.partition("=")[2]).strip() for a in rest if _top(a) == "config"]
    base = T.CONF.parent / f"{named[-1]}.yaml" if named else T.CONF
    known = set(load_yaml(base)) | {"config", "prediction_metrics"} if base.is_file() else None
    unknown = sorted({_top(a) for a in rest} - known) if known is not None else []
    if unknown or own["weights"] is None or own["split"] not in SPLITS or any("=" not in a for a in argv):
        raise SystemExit(USAGE + (f"  (unknown: {', '.join(unknown)})" if unknown else ""))
    cfg = T.load_training_config(rest)
    device = torch.device(cfg["device"])
    fp16 = bool(cfg["fp16"])
    pm = cfg.get("prediction_metrics")
    kw = T._metrics_keywords(dict(pm) if isinstance(pm, dict) else {}, instantiate(cfg["loss_fn"]))

    torch.manual_seed(42)
    torch.cuda.manual_seed_all(42)
    loader = instantiate(cfg[f"{own['split']}_data_loader"])
    model = instantiate(cfg["model"]).to(device)
    model.load_state_dict(load_weights(own["weights"]))
    model.eval()
    trees, total = {}, None
    for (feats, targets), coords, mask, names in loader:
        if fp16:  # as train._batches: the values rounded to half
            feats, targets = feats.half(), targets.half()
        offsets = segment_offsets(coords[:, 0])
        offsets += [offsets[-1]] * (len(names) + 1 - len(offsets))  # trailing trees without a voxel
        with torch.autocast(device.type, dtype=torch.float16, enabled=fp16):
            preds = model.forward(sparse_from_batch(feats.float(), coords, device=device))
        tally = prediction_tally(preds, targets.to(device).float(), mask.to(device), seg_off=offsets, **kw)
        for s, name in enumerate(names):
            key = str(name)
            while key in trees:
                key += "+"
            trees[key] = tally.segment(s).metrics()
            print(_line(key, trees[key]))
        total = tally.total() if total is None else total + tally.total()
    result = {"trees": trees, "total": total.metrics() if total is not None else None}
    if total is not None:
        print(_line(f"total of {len(trees)}", result["total"]))
    if own["out"]:
        out = Path(str(own["out"]))
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text(json.dumps(result, indent=1))
    return result


if __name__ == "__main__":
    main()
