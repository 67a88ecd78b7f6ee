"""Training and evaluation epochs (reference smart_tree/model/train.py:24-84) for `trainable.TrainableSmartTree`.

Batches are `model.sparse.batch_collate` items: ((inputs, targets), coords, loss_mask, names).  Every step: forward, `loss_fn(preds,
targets, mask)` (e.g. `functools.partial(loss.compute_loss, radius_loss_fn=loss.L1Loss, ...)`), `sum(loss.values()).backward()`,
`optimizer.step()`, `optimizer.zero_grad()`.  No logger, progress bar or config framework.

Mixed precision (the reference's `fp16: True`, train.py:24-58 with helper.get_batch(..., fp_16=True)): `fp16=True` rounds features
and targets through half, runs forward and loss under `torch.autocast(device.type, dtype=torch.float16)` and steps through the
caller's `GradScaler` (`scaler.scale(total).backward()`, `scaler.step(optimizer)`, `scaler.update()`).  Pass the same scaler to every
epoch, as the reference threads one through its run: a fresh one per epoch would reset the scale.
"""
from __future__ import annotations

import torch

from .sparse import sparse_from_batch


def _batches(data_loader, device, fp16=False):
    for (feats, targets), coords, mask, _ in data_loader:
        if fp16:  # get_batch(fp_16=True): the values rounded to half (the convolutions cast to half under autocast, exactly)
            feats, targets = feats.half(), targets.half()
        yield sparse_from_batch(feats.float(), coords, device=device), targets.to(device).float(), mask.to(device)


def _mean(sums, count):
    return {k: v / max(count, 1) for k, v in sums.items()}


def train_epoch(data_loader, model, optimizer, loss_fn, device=torch.device("cuda"), *, fp16=False, scaler=None) -> dict:
    """One pass over `data_loader` with an optimiser step per batch (train.py:24-58); returns the mean of each loss term.
    fp16=True: autocast to float16 and loss scaling through `scaler` (a torch.amp.GradScaler, required)."""
    device = torch.device(device)
    if fp16 and scaler is None:
        raise ValueError("train_epoch(fp16=True) needs the run's GradScaler (scaler=...), the same one for every epoch")
    model.train()
    sums, count = {}, 0
    for sp_input, targets, mask in _batches(data_loader, device, fp16):
        if fp16:
            with torch.autocast(device.type, dtype=torch.float16):
                preds = model.forward(sp_input)
                loss = loss_fn(preds, targets, mask)
                total = sum(loss.values())
            assert total.dtype == torch.float32, total.dtype  # train.py:46
            scaler.scale(total).backward()
            scaler.step(optimizer)
            scaler.update()
        else:
            preds = model.forward(sp_input)
            loss = loss_fn(preds, targets, mask)
            sum(loss.values()).backward()
            optimizer.step()
        optimizer.zero_grad()
        for k, v in loss.items():
            sums[k] = sums.get(k, 0.0) + float(v.detach())
        count += 1
    return _mean(sums, count)


@torch.no_grad()
def eval_epoch(data_loader, model, loss_fn, device=torch.device("cuda"), *, fp16=False) -> dict:
    """train.py:61-84: the losses in eval mode (running BatchNorm statistics), no gradients; the model is left in train mode.
    fp16=True: under float16 autocast, as train_epoch."""
    device = torch.device(device)
    model.eval()
    sums, count = {}, 0
    for sp_input, targets, mask in _batches(data_loader, device, fp16):
        with torch.autocast(device.type, dtype=torch.float16, enabled=fp16):
            loss = loss_fn(model.forward(sp_input), targets, mask)
        for k, v in loss.items():
            sums[k] = sums.get(k, 0.0) + float(v)
        count += 1
    model.train()
    return _mean(sums, count)
