"""The small hydra stand-in behind `run-smart-tree` and `train-smart-tree`: YAML files whose nodes name a `_target_`,
command-line overrides, `${...}` interpolation and recursive instantiation.

* `instantiate(node, **extra)`: a dict with `_target_` is called with its other keys (instantiated first) plus `extra`; with
  `_partial_: True` it becomes `functools.partial(target, **kwargs)`, or the target itself when there is nothing to bind (the same
  callable, and `loss.compute_loss` recognises its fused loss functions by identity).  A dict without `_target_` is a dict of
  instantiated values, a list a list of them.
* `apply_overrides(cfg, ["a.b=value", "+key=value"])`: the value is parsed as YAML.
* `resolve(cfg)`: `${key}` / `${a.b}` after the overrides.  A string that is exactly one reference takes the referenced value or
  subtree (a fresh copy at every use, so that each place instantiates its own object, as hydra does); a reference inside a longer
  string is substituted as text.  `${now:FORMAT}` is the time of the call through `strftime`.  A missing key or a cycle raises
  `ConfigError` naming the key.
"""
from __future__ import annotations

import copy
import functools
import importlib
import re
import time
from pathlib import Path

import yaml

_REF = re.compile(r"\$\{([^}]*)\}")


class ConfigError(KeyError):
    def __str__(self):
        return str(self.args[0])


def instantiate(node, **extra):
    if isinstance(node, list):
        return [instantiate(v) for v in node]
    if not isinstance(node, dict):
        return node
    kwargs = {k: instantiate(v) for k, v in node.items() if k not in ("_target_", "_partial_")}
    if "_target_" not in node:
        return kwargs
    kwargs.update(extra)
    module, _, name = node["_target_"].rpartition(".")
    target = getattr(importlib.import_module(module), name)
    if node.get("_partial_", False):
        return functools.partial(target, **kwargs) if kwargs else target
    return target(**kwargs)


def load_yaml(path) -> dict:
    return yaml.safe_load(Path(path).read_text()) or {}


def apply_overrides(cfg: dict, overrides=()) -> dict:
    for item in overrides:
        key, _, value = item.lstrip("+").partition("=")
        node = cfg
        parts = key.split(".")
        for p in parts[:-1]:
            node = node.setdefault(p, {})
        node[parts[-1]] = yaml.safe_load(value)
    return cfg


def cloud_command(argv, defaults: dict, usage: str):
    """The opening of the `key=value` commands that work on a cloud and its skeleton (`segmentation`, `refine`, `inventory`):
    (cfg, device, cloud).  `defaults` with the overrides applied; a key it does not hold, or no `cloud`, `skeleton` or `out`, ends
    with `usage`; the cloud is loaded onto `cfg["device"]` and, with `centre=true`, centred by `CentreCloud`."""
    import sys

    import torch

    from .util.file import load_cloud

    cfg = apply_overrides(dict(defaults), argv if argv is not None else sys.argv[1:])
    unknown = sorted(set(cfg) - set(defaults))
    if unknown or cfg["cloud"] is None or cfg["skeleton"] is None or cfg["out"] is None:
        raise SystemExit(usage + (f"  (unknown: {', '.join(unknown)})" if unknown else ""))
    dev = torch.device(cfg["device"])
    cloud = load_cloud(cfg["cloud"]).to_device(dev)
    if str(cfg["centre"]).lower() in ("true", "1", "yes", "on"):
        from .dataset.augmentations import CentreCloud
        cloud = CentreCloud()(cloud)
    return cfg, dev, cloud


def resolve(cfg: dict) -> dict:
    now = time.localtime()
    done: dict = {}

    def lookup(key, stack):
        if key.startswith("now:"):
            return time.strftime(key[4:], now)
        if key in stack:
            raise ConfigError(f"interpolation cycle: {' -> '.join(stack + [key])}")
        if key not in done:
            node = cfg
            for p in key.split("."):
                if not isinstance(node, dict) or p not in node:
                    where = f" (referenced from '{stack[-1]}')" if stack else ""
                    raise ConfigError(f"interpolation key '{key}' not found{where}")
                node = node[p]
            done[key] = walk(node, stack + [key])
        return copy.deepcopy(done[key])

    def walk(node, stack):
        if isinstance(node, dict):
            return {k: walk(v, stack) for k, v in node.items()}
        if isinstance(node, list):
            return [walk(v, stack) for v in node]
        if isinstance(node, str):
            m = _REF.fullmatch(node)
            if m:
                return lookup(m.group(1).strip(), stack)
            return _REF.sub(lambda r: str(lookup(r.group(1).strip(), stack)), node)
        return node

    return walk(cfg, [])
