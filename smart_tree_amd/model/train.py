"""Training and evaluation epochs (reference smart_tree/model/train.py:24-84) for `trainable.TrainableSmartTree`.

Batches are `model.sparse.batch_collate` items: ((inputs, targets), coords, loss_mask, names).  Every step: forward, `loss_fn(preds,
targets, mask)` (e.g. `functools.partial(loss.compute_loss, radius_loss_fn=loss.L1Loss, ...)`), `sum(loss.values()).backward()`,
`optimizer.step()`, `optimizer.zero_grad()`.  No logger, progress bar, AMP or config framework.
"""
from __future__ import annotations

import torch

from .sparse import sparse_from_batch


def _batches(data_loader, device):
    for (feats, targets), coords, mask, _ in data_loader:
        yield sparse_from_batch(feats.float(), coords, device=device), targets.to(device).float(), mask.to(device)


def _mean(sums, count):
    return {k: v / max(count, 1) for k, v in sums.items()}


def train_epoch(data_loader, model, optimizer, loss_fn, device=torch.device("cuda")) -> dict:
    """One pass over `data_loader` with an optimiser step per batch (train.py:24-58); returns the mean of each loss term."""
    device = torch.device(device)
    model.train()
    sums, count = {}, 0
    for sp_input, targets, mask in _batches(data_loader, device):
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
def eval_epoch(data_loader, model, loss_fn, device=torch.device("cuda")) -> dict:
    """train.py:61-84: the losses in eval mode (running BatchNorm statistics), no gradients; the model is left in train mode."""
    device = torch.device(device)
    model.eval()
    sums, count = {}, 0
    for sp_input, targets, mask in _batches(data_loader, device):
        for k, v in loss_fn(model.forward(sp_input), targets, mask).items():
            sums[k] = sums.get(k, 0.0) + float(v)
        count += 1
    model.train()
    return _mean(sums, count)
