"""Loss tracker at the reference's name (smart_tree/model/tracker.py), and the metrics file that takes wandb's place.

`Tracker.log(name, epoch, sink)` hands `{name: {radius, direction, class_l, total}}` to `sink.log(data, step=epoch)`; a
`MetricsSink` gathers everything logged for one step and `commit()` writes it as one JSON line `{"epoch": step, ...}`.
"""
from __future__ import annotations

import json
import logging
from pathlib import Path

import numpy as np

log = logging.getLogger(__name__)


class Tracker:
    def __init__(self):
        self.running_epoch_radius_loss = []
        self.running_epoch_direction_loss = []
        self.running_epoch_class_loss = []

    def update(self, loss_dict: dict):
        self.running_epoch_radius_loss.append(float(loss_dict["radius"]))
        self.running_epoch_direction_loss.append(float(loss_dict["direction"]))
        self.running_epoch_class_loss.append(float(loss_dict["class_l"]))

    @property
    def radius_loss(self):
        return float(np.mean(self.running_epoch_radius_loss))

    @property
    def direction_loss(self):
        return float(np.mean(self.running_epoch_direction_loss))

    @property
    def class_loss(self):
        return float(np.mean(self.running_epoch_class_loss))

    @property
    def total_loss(self):
        return self.radius_loss + self.direction_loss + self.class_loss

    def as_dict(self) -> dict:
        return {"radius": self.radius_loss, "direction": self.direction_loss, "class_l": self.class_loss, "total": self.total_loss}

    def log(self, name, epoch, sink=None):
        """tracker.py:33-42 without wandb: to `sink.log(data, step)` (e.g. a MetricsSink), or through `logging` without one."""
        if sink is None:
            log.info("%s epoch %d: %s", name, epoch, self.as_dict())
        else:
            sink.log({name: self.as_dict()}, step=epoch)


def total(means: dict) -> float:
    """Tracker.total_loss of per-term means (train.train_epoch / eval_epoch's dicts)."""
    return means["radius"] + means["direction"] + means["class_l"]


class MetricsSink:
    """`<run_dir>/metrics.jsonl`: one JSON line per step."""

    def __init__(self, path):
        self.path = Path(path)
        self.pending: dict = {}
        self.step = None

    def log(self, data: dict, step: int):
        if self.step is not None and step != self.step:
            self.commit()
        self.step = step
        self.pending.update(data)

    def commit(self):
        if self.step is None:
            return
        record = {"epoch": self.step, **self.pending}
        with open(self.path, "a") as f:
            f.write(json.dumps(record, allow_nan=True) + "\n")
        self.pending, self.step = {}, None

    def truncate(self, first_epoch: int):
        """Keep the lines of epochs before `first_epoch` (a resumed run rewrites what came after its checkpoint)."""
        if not self.path.exists():
            return
        keep = [ln for ln in self.path.read_text().splitlines() if ln.strip() and json.loads(ln)["epoch"] < first_epoch]
        self.path.write_text("".join(ln + "\n" for ln in keep))


def read_metrics(path) -> list:
    return [json.loads(ln) for ln in Path(path).read_text().splitlines() if ln.strip()]
