"""Training and evaluation epochs (reference smart_tree/model/train.py:24-84) for `trainable.TrainableSmartTree`.

Batches are `model.sparse.batch_collate` items: ((inputs, targets), coords, loss_mask, names).  Every step: forward, `loss_fn(preds,
targets, mask)` (e.g. `functools.partial(loss.compute_loss, radius_loss_fn=loss.L1Loss, ...)`), `sum(loss.values()).backward()`,
`optimizer.step()`, `optimizer.zero_grad()`.  No logger, progress bar or config framework.

Mixed precision (the reference's `fp16: True`, train.py:24-58 with helper.get_batch(..., fp_16=True)): `fp16=True` rounds features
and targets through half, runs forward and loss under `torch.autocast(device.type, dtype=torch.float16)` and steps through the
caller's `GradScaler` (`scaler.scale(total).backward()`, `scaler.step(optimizer)`, `scaler.update()`).  Pass the same scaler to every
epoch, as the reference threads one through its run: a fresh one per epoch would reset the scale.

The `train-smart-tree` run (train.py:166-262 with conf/training.yaml): `main(argv)` / `python -m smart_tree_amd.model.train
[key=value ...]` loads `conf/training.yaml` (smart_tree_amd/config.py), trains with the epochs above and writes `config.yaml`,
`metrics.jsonl`, `<run_name>_model_weights.pt` (each new best), `last.pt` (every epoch) and `captures/` into `run_dir`;
`resume=<run_dir>` continues from that run's `last.pt`.  `StopPolicy` holds the best / early-stop / scheduler decisions.
`prediction_metrics=true` (or a mapping of `evaluation.prediction_tally` keywords; no shipped configuration sets it) adds
`validation_metrics` and `test_metrics` to every line of `metrics.jsonl`: accuracy, IoU, radius and medial-point errors of the
predictions (`eval_epoch(metrics=...)`).  The best checkpoint is still chosen by the validation loss.

Data parallel (model/data_parallel.py, model/sync_bn.py): `train_epoch` / `eval_epoch(..., group=g)` take rank g's share of
every global batch, synchronise BatchNorm (the model must have gone through `sync_bn.convert_sync_batchnorm`), weight the loss
terms by the global row counts and all-reduce the gradients.  `python -m torch.distributed.run --nproc_per_node N -m
smart_tree_amd.model.train ...` (or `run(cfg)` under an initialised group of more than one rank) trains that way; rank 0 writes
the run's files, every rank its own trees' captures.  With one rank nothing changes.
"""
from __future__ import annotations

import logging
import math
import os
import random
import sys
import time
from dataclasses import dataclass
from pathlib import Path
from typing import List, NamedTuple

import numpy as np
import torch
import torch.distributed as dist
import yaml

from ..config import _REF, apply_overrides, instantiate, load_yaml, resolve
from ..data_types.cloud import Cloud
from . import data_parallel as dp
from .helper import get_batch, model_output_to_labelled_clds
from .sparse import sparse_from_batch
from .tracker import MetricsSink, total

log = logging.getLogger(__name__)
CONF = Path(__file__).resolve().parents[1] / "conf" / "training.yaml"
REQUIRED = ("directory", "json_path")


def _batches(data_loader, device, fp16=False, model=None):
    for item in data_loader:
        if item is None:  # data parallel: this rank owns no tree of the global batch
            feats, coords, targets, mask = dp.empty_batch(model, device)
        else:
            (feats, targets), coords, mask, _ = item
        if fp16:  # get_batch(fp_16=True): the values rounded to half (the convolutions cast to half under autocast, exactly)
            feats, targets = feats.half(), targets.half()
        yield sparse_from_batch(feats.float(), coords, device=device), targets.to(device).float(), mask.to(device)


def _mean(sums, count):
    return {k: v / max(count, 1) for k, v in sums.items()}


def _data_parallel(data_loader, model, loss_fn, group):
    """The rank's shard of `data_loader`, after checking that the model and the loss can be reduced across ranks."""
    dp.check_loss_fn(loss_fn)
    if any(isinstance(m, torch.nn.modules.batchnorm._BatchNorm) for m in model.modules()):
        raise ValueError("data-parallel training needs synchronised BatchNorm: call sync_bn.convert_sync_batchnorm(model, group) "
                         "before building the optimiser")
    return dp.shard_loader(data_loader, group)


def train_epoch(data_loader, model, optimizer, loss_fn, device=torch.device("cuda"), *, fp16=False, scaler=None, group=None) -> dict:
    """One pass over `data_loader` with an optimiser step per batch (train.py:24-58); returns the mean of each loss term.
    fp16=True: autocast to float16 and loss scaling through `scaler` (a torch.amp.GradScaler, required).
    group: data parallel over that process group (module docstring); the returned means are the global batches'."""
    device = torch.device(device)
    if fp16 and scaler is None:
        raise ValueError("train_epoch(fp16=True) needs the run's GradScaler (scaler=...), the same one for every epoch")
    if group is not None:
        data_loader = _data_parallel(data_loader, model, loss_fn, group)
    model.train()
    sums, count = {}, 0
    for sp_input, targets, mask in _batches(data_loader, device, fp16, model):
        logged = None
        if fp16:
            with torch.autocast(device.type, dtype=torch.float16):
                preds = model.forward(sp_input)
                if group is None:
                    loss = loss_fn(preds, targets, mask)
                else:
                    loss, logged = dp.global_loss(loss_fn, preds, targets, mask, group)
                total = sum(loss.values())
            assert total.dtype == torch.float32, total.dtype  # train.py:46
            scaler.scale(total).backward()
            if group is not None:
                dp.all_reduce_grads(model.parameters(), group)  # before the step: the same inf / NaN skip on every rank
            scaler.step(optimizer)
            scaler.update()
        else:
            preds = model.forward(sp_input)
            if group is None:
                loss = loss_fn(preds, targets, mask)
            else:
                loss, logged = dp.global_loss(loss_fn, preds, targets, mask, group)
            sum(loss.values()).backward()
            if group is not None:
                dp.all_reduce_grads(model.parameters(), group)
            optimizer.step()
        optimizer.zero_grad()
        for k, v in (logged or {k: float(v.detach()) for k, v in loss.items()}).items():
            sums[k] = sums.get(k, 0.0) + v
        count += 1
    return _mean(sums, count)


def _metrics_keywords(metrics, loss_fn) -> dict:
    """`prediction_tally`'s keywords for an epoch: `metrics` as given, with the loss's row selection (`vector_class`,
    `target_radius_log` of a `functools.partial` loss_fn) where `metrics` does not set it."""
    kw = {k: v for k, v in (getattr(loss_fn, "keywords", None) or {}).items() if k in ("vector_class", "target_radius_log")}
    kw.update(metrics)
    return kw


@torch.no_grad()
def eval_epoch(data_loader, model, loss_fn, device=torch.device("cuda"), *, fp16=False, group=None, metrics=None) -> dict:
    """train.py:61-84: the losses in eval mode (running BatchNorm statistics), no gradients; the model is left in train mode.
    fp16=True: under float16 autocast, as train_epoch.  group: each rank evaluates its share of every global batch and the
    per-batch values are the global count-weighted means.
    metrics: a dict of `evaluation.prediction_tally` keywords ({} = its defaults) tallies every batch's predictions in one more
    HIP pass, adds the tallies on the device (all-reduced once at the end under `group`) and returns their
    `PredictionTally.metrics()` under "metrics" (None for a loader without batches).  None (the default): nothing of this."""
    device = torch.device(device)
    if group is not None:
        data_loader = _data_parallel(data_loader, model, loss_fn, group)
    if metrics is not None:
        from ..evaluation.prediction import prediction_tally

        metrics = _metrics_keywords(metrics, loss_fn)
    tally = None
    model.eval()
    sums, count = {}, 0
    for sp_input, targets, mask in _batches(data_loader, device, fp16, model):
        with torch.autocast(device.type, dtype=torch.float16, enabled=fp16):
            preds = model.forward(sp_input)
            if group is None:
                values = {k: float(v) for k, v in loss_fn(preds, targets, mask).items()}
            else:
                values = dp.global_loss(loss_fn, preds, targets, mask, group)[1]
        for k, v in values.items():
            sums[k] = sums.get(k, 0.0) + v
        count += 1
        if metrics is not None:
            batch = prediction_tally(preds, targets, mask, **metrics)
            tally = batch if tally is None else tally + batch
    model.train()
    out = _mean(sums, count)
    if metrics is not None:
        if tally is not None and group is not None:
            tally = tally.all_reduce(group)
        out["metrics"] = tally.metrics() if tally is not None else None
    return out


@torch.no_grad()
def capture_clouds(loader, model, cmap, fp16=False, device=torch.device("cuda")) -> List[Cloud]:
    """train.py:110-138: the model's outputs on every tree of `loader` as labelled Clouds (helper.to_labelled_clds), in eval mode;
    the model is left in train mode."""
    device = torch.device(device)
    model.eval()
    clouds = []
    for sp_input, _, _, filenames in get_batch(loader, device, fp16):
        with torch.autocast(device.type, dtype=torch.float16, enabled=fp16):
            out = model.forward(sp_input)
        clouds.extend(model_output_to_labelled_clds(sp_input, out, cmap, filenames))
    model.train()
    return clouds


class Decision(NamedTuple):
    step_scheduler: bool
    save_best: bool
    stop: bool


@dataclass
class StopPolicy:
    """train.py:230-247 after each epoch's validation total: step the scheduler if `lr_decay`; a total below the best so far
    saves the weights and resets the no-improvement counter, otherwise the counter grows; stop when it equals
    `early_stop_epoch` and `early_stop` is set."""

    early_stop_epoch: int
    early_stop: bool = True
    lr_decay: bool = True
    best: float = math.inf
    epochs_no_improve: int = 0

    def update(self, val_total: float) -> Decision:
        save = val_total < self.best
        if save:
            self.best, self.epochs_no_improve = float(val_total), 0
        else:
            self.epochs_no_improve += 1
        stop = bool(self.early_stop) and self.epochs_no_improve == self.early_stop_epoch
        return Decision(bool(self.lr_decay), save, stop)


def _refers_to(node, key: str) -> bool:
    """Some value of the configuration interpolates `${key}`."""
    if isinstance(node, dict):
        return any(_refers_to(v, key) for v in node.values())
    if isinstance(node, list):
        return any(_refers_to(v, key) for v in node)
    return isinstance(node, str) and any(m.strip() == key for m in _REF.findall(node))


def load_training_config(overrides=()) -> dict:
    """conf/training.yaml (or `config=<name>`: conf/<name>.yaml; or, with `resume=<run_dir>`, that run's config.yaml) + overrides,
    `device: auto` decided, then the interpolations resolved.  `directory` and `json_path` are demanded when the configuration
    refers to them (conf/training.yaml does, conf/training_synthetic.yaml does not).  A resumed run writes into the run it
    continues."""
    overrides = list(overrides)
    base, named = CONF, None
    for item in overrides:
        key, _, value = item.lstrip("+").partition("=")
        if key == "resume" and yaml.safe_load(value):
            base = Path(str(yaml.safe_load(value))) / "config.yaml"
        elif key == "config" and yaml.safe_load(value):  # another bundled configuration: conf/<name>.yaml
            named = CONF.parent / f"{yaml.safe_load(value)}.yaml"
            if not named.is_file():
                raise ValueError(f"train-smart-tree: no bundled configuration '{yaml.safe_load(value)}' ({named})")
    if named is not None and base is CONF:  # a resumed run keeps the configuration it was started with
        base = named
    cfg = apply_overrides(load_yaml(base), overrides)
    missing = [k for k in REQUIRED if cfg.get(k) in (None, "???", "") and _refers_to(cfg, k)]
    if missing:
        raise ValueError(f"train-smart-tree: {' and '.join(missing)} not set: pass " + " ".join(f"{k}=..." for k in missing))
    if cfg.get("device", "auto") == "auto":  # under torchrun: this rank's GPU
        cfg["device"] = f"cuda:{int(os.environ.get('LOCAL_RANK', 0))}" if torch.cuda.is_available() else "cpu"
    cfg = resolve(cfg)
    if cfg.get("resume"):
        cfg["run_dir"] = str(cfg["resume"])
    return cfg


def rng_state() -> dict:
    """Every generator the run draws from (RandomCubicCrop and the DataLoader use torch's CPU one), as tensors and plain values
    so that the checkpoint loads with weights_only=True."""
    _, keys, pos, has_gauss, gauss = np.random.get_state()
    version, state, py_gauss = random.getstate()
    return {"torch": torch.get_rng_state(),
            "cuda": torch.cuda.get_rng_state_all() if torch.cuda.is_available() else [],
            "numpy": {"keys": torch.from_numpy(keys.astype(np.int64)), "pos": int(pos), "has_gauss": int(has_gauss),
                      "cached_gaussian": float(gauss)},
            "python": {"version": version, "state": torch.tensor(state, dtype=torch.int64), "gauss": py_gauss}}


def set_rng_state(s: dict) -> None:
    torch.set_rng_state(s["torch"])
    if s["cuda"] and torch.cuda.is_available():
        torch.cuda.set_rng_state_all(s["cuda"])
    n = s["numpy"]
    np.random.set_state(("MT19937", n["keys"].numpy().astype(np.uint32), n["pos"], n["has_gauss"], n["cached_gaussian"]))
    p = s["python"]
    random.setstate((p["version"], tuple(p["state"].tolist()), p["gauss"]))


def _save(obj, path: Path) -> None:
    tmp = path.with_name(path.name + ".tmp")
    torch.save(obj, tmp)
    os.replace(tmp, path)


def _capture(run_dir: Path, epoch: int, loaders: dict, model, cfg, device, group=None) -> None:
    from ..util.file import save_cloud

    for split, loader in loaders.items():
        if group is not None:  # each rank captures its own trees
            loader = [b for b in dp.shard_loader(loader, group) if b is not None]
        out = run_dir / "captures" / f"epoch_{epoch}" / split
        out.mkdir(parents=True, exist_ok=True)
        for cloud in capture_clouds(loader, model, cfg["cmap"], fp16=cfg["fp16"], device=device):
            save_cloud(out / f"{Path(cloud.filename).stem}.npz", cloud)
            if cfg.get("capture_images", False):  # the reference's render_cloud pictures, beside the .npz
                from ..render import Renderer
                from .render import write_cloud_images

                size = cfg.get("capture_image_size", [960, 540])
                write_cloud_images(Renderer(int(size[0]), int(size[1])), cloud.to_device(device), out / Path(cloud.filename).stem,
                                   cmap=cfg["cmap"])


def _gather_rng(group) -> list:
    """Every rank's rng_state(), on every rank (rank 0 writes them)."""
    states = [None] * dist.get_world_size(group)
    dist.all_gather_object(states, rng_state(), group=group)
    return states


def run(cfg: dict, group=None) -> dict:
    """train.py:166-262 on a resolved configuration (load_training_config).  Returns {"run_dir", "epochs", "best", "stopped"}.
    Data parallel over `group`, or over the default process group when one with more than one rank is initialised."""
    group = dp.default_group(group)
    rank, world = dp.rank_world(group)
    lead = rank == 0
    run_dir = Path(cfg["run_dir"])
    run_dir.mkdir(parents=True, exist_ok=True)
    device = torch.device(cfg["device"])
    fp16 = bool(cfg["fp16"])
    log.info("run directory: %s, device: %s%s", run_dir, device, f", rank {rank} of {world}" if group is not None else "")
    if group is not None:
        cfg = {**cfg, "world_size": world}
    if lead:
        (run_dir / "config.yaml").write_text(yaml.safe_dump(cfg, sort_keys=False))
    ep_kw = {"group": group} if group is not None else {}
    pm = cfg.get("prediction_metrics")  # absent / false: off; true: prediction_tally's defaults; a mapping: its keywords
    ev_kw = dict(ep_kw) if pm in (None, False) else {**ep_kw, "metrics": {} if pm is True else dict(pm)}

    torch.manual_seed(42)
    torch.cuda.manual_seed_all(42)
    train_loader = instantiate(cfg["train_data_loader"])
    val_loader = instantiate(cfg["validation_data_loader"])
    test_loader = instantiate(cfg["test_data_loader"])
    log.info("trees: %d train, %d validation, %d test", len(train_loader.dataset), len(val_loader.dataset),
             len(test_loader.dataset))
    model = instantiate(cfg["model"]).to(device).train()
    if group is not None:
        from .sync_bn import convert_sync_batchnorm

        convert_sync_batchnorm(model, group)
    optimizer = instantiate(cfg["optimizer"], params=model.parameters())
    scheduler = instantiate(cfg["scheduler"], optimizer=optimizer)
    loss_fn = instantiate(cfg["loss_fn"])
    scaler = torch.amp.GradScaler(device.type, enabled=fp16)
    policy = StopPolicy(cfg["early_stop_epoch"], cfg["early_stop"], cfg["lr_decay"])
    sink = MetricsSink(run_dir / "metrics.jsonl") if lead else None
    weights_path = run_dir / f"{cfg['run_name']}_model_weights.pt"

    start, stopped = 0, False
    if cfg.get("resume"):
        ck = torch.load(Path(cfg["resume"]) / "last.pt", map_location="cpu", weights_only=True)
        if ck.get("world_size", 1) != world:
            raise ValueError(f"resume: {cfg['resume']} was trained on {ck.get('world_size', 1)} rank(s) and this run has {world}: resume "
                             "with the same number of ranks (each rank restores its own random state)")
        model.load_state_dict(ck["model"])
        optimizer.load_state_dict(ck["optimizer"])
        scheduler.load_state_dict(ck["scheduler"])
        scaler.load_state_dict(ck["scaler"])
        policy.best, policy.epochs_no_improve = ck["best"], ck["epochs_no_improve"]
        start, stopped = ck["epoch"] + 1, ck["stopped"]
        set_rng_state(ck["rng_ranks"][rank] if group is not None else ck["rng"])
        if lead:
            sink.truncate(start)
        log.info("resumed after epoch %d (best %.6g)%s", ck["epoch"], policy.best, ", which had stopped early" if stopped else "")

    epoch = start - 1
    for epoch in range(start, cfg["num_epoch"] if not stopped else start):
        t0 = time.perf_counter()
        lr = optimizer.param_groups[0]["lr"]
        for loader in (train_loader, val_loader, test_loader):  # a dataset that generates its trees: this epoch's
            if hasattr(loader.dataset, "set_epoch"):
                loader.dataset.set_epoch(epoch)
        train = train_epoch(train_loader, model, optimizer, loss_fn, device, fp16=fp16, scaler=scaler, **ep_kw)
        val = eval_epoch(val_loader, model, loss_fn, device, fp16=fp16, **ev_kw)
        test = eval_epoch(test_loader, model, loss_fn, device, fp16=fp16, **ev_kw)
        val_metrics, test_metrics = val.pop("metrics", None), test.pop("metrics", None)
        if cfg["capture_output"] > 0 and (epoch + 1) % cfg["capture_output"] == 0:
            _capture(run_dir, epoch, {"test": test_loader, "validation": val_loader}, model, cfg, device, group)
        if group is not None:
            dp.check_replicas(model, group)
        decision = policy.update(total(val))
        if decision.step_scheduler:
            scheduler.step(total(val))
        if decision.save_best and lead:
            _save({k: v.detach().cpu() for k, v in model.state_dict().items()}, weights_path)
        stopped = decision.stop
        seconds = time.perf_counter() - t0
        if lead:
            sink.log({"lr": lr, "seconds": seconds, "best": policy.best}, step=epoch)
            for name, means in (("train", train), ("validation", val), ("test", test)):
                sink.log({name: {**means, "total": total(means)}}, step=epoch)
            if "metrics" in ev_kw:
                sink.log({"validation_metrics": val_metrics, "test_metrics": test_metrics}, step=epoch)
            sink.commit()
        log.info("epoch %d/%d: train %.4f, validation %.4f, test %.4f, lr %.3g, %.2f s%s", epoch + 1, cfg["num_epoch"], total(train),
                 total(val), total(test), lr, seconds, ", weights saved" if decision.save_best else "")
        state = {"model": model.state_dict(), "optimizer": optimizer.state_dict(), "scheduler": scheduler.state_dict(),
                 "scaler": scaler.state_dict(), "epoch": epoch, "best": policy.best,
                 "epochs_no_improve": policy.epochs_no_improve, "stopped": stopped, "rng": rng_state()}
        if group is not None:
            state.update(world_size=world, rng_ranks=_gather_rng(group))
            dist.barrier(group)  # every rank has read the previous last.pt before it is replaced
        if lead:
            _save(state, run_dir / "last.pt")
        if stopped:
            log.info("training ended: validation total not improving for %d epochs", policy.epochs_no_improve)
            break
    if group is not None:
        dist.barrier(group)  # rank 0's files are complete when any rank returns
    return {"run_dir": run_dir, "epochs": epoch + 1, "best": policy.best, "stopped": stopped}


def main(argv=None) -> dict:
    """The run; under torchrun (WORLD_SIZE > 1) the process group is initialised from its environment first."""
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(name)s: %(message)s")
    cfg = load_training_config(sys.argv[1:] if argv is None else argv)
    created = dp.init_from_env(cfg)
    try:
        return run(cfg)
    finally:
        if created:
            dist.destroy_process_group()


if __name__ == "__main__":
    main()
