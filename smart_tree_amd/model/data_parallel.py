"""Data-parallel training helpers (DESIGN.md "Training: data parallel").

The contract is global-batch semantics: a step on W ranks, each holding its share of a global batch of `batch_size` trees,
computes the same loss terms, gradients, parameter update and running statistics as one process given the whole batch (up to
float rounding).  Three reductions meet it:
  * BatchNorm statistics, forward and backward: model/sync_bn.py (`convert_sync_batchnorm`);
  * the loss means: each rank's fused loss terms (loss.compute_loss) weighted by its share of the global row counts, n_r / N,
    after one all-reduce of [n_v * radius, n_v * direction, n_c * focal, n_v, n_c] (float64) per step -- the upstream gradients
    carry the weights into st_loss_backward;
  * the gradients: one all_reduce(SUM) of a flat buffer of every gradient after backward, before the optimiser (or GradScaler)
    step, so every rank takes the same step and the same skip decision.

Sharding: `batch_size` stays the GLOBAL batch.  `ShardBatchSampler` gives rank r the positions r, r + W, ... of every global batch
of the loader's own batch sampler (`sharding.shard_indices` per batch), so the batches hold the trees the one-process run's do.  A
rank that owns no tree of a batch gets an empty batch (None from the collate function): it runs the network on zero rows, takes
part in every collective in the same order and contributes zero rows, zero loss weight and zero gradients.  The random crops are
drawn by the rank that loads the tree, so they differ from the one-process run's draws.
"""
from __future__ import annotations

import functools
import logging
import os

import torch
import torch.distributed as dist
from torch.utils.data import DataLoader, RandomSampler

from ..sharding import shard_indices
from . import loss as L

log = logging.getLogger(__name__)

TERMS = ("radius", "direction", "class_l")


def rank_world(group):
    """(rank, world size) in `group`; (0, 1) without one."""
    if group is None:
        return 0, 1
    return dist.get_rank(group), dist.get_world_size(group)


def default_group(group=None):
    """`group`, or the initialised default group when it has more than one rank, else None (the one-process run)."""
    if group is not None:
        return group
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        return dist.group.WORLD
    return None


def backend_for(cfg: dict, device: torch.device) -> str:
    b = str(cfg.get("dist_backend", "auto"))
    if b == "auto":
        return "nccl" if device.type == "cuda" else "gloo"
    return b


def init_from_env(cfg: dict) -> bool:
    """Initialise the default process group from torchrun's environment (WORLD_SIZE > 1) unless one exists.  Returns True when this
    call created it (the caller destroys it)."""
    if int(os.environ.get("WORLD_SIZE", "1")) <= 1 or dist.is_initialized():
        return False
    device = torch.device(cfg["device"])
    backend = backend_for(cfg, device)
    if device.type == "cuda":
        torch.cuda.set_device(device)
        dist.init_process_group(backend, device_id=device if backend == "nccl" else None)
    else:
        dist.init_process_group(backend)
    log.info("process group: rank %d of %d, backend %s, device %s", dist.get_rank(), dist.get_world_size(), backend, device)
    return True


class ShardBatchSampler:
    """Rank `rank`'s positions r, r + W, ... of every batch of `batch_sampler` (possibly none: an empty list)."""

    def __init__(self, batch_sampler, rank: int, world: int):
        self.batch_sampler, self.rank, self.world = batch_sampler, rank, world

    def __iter__(self):
        for batch in self.batch_sampler:
            batch = list(batch)
            yield [batch[i] for i in shard_indices(len(batch), self.rank, self.world)]

    def __len__(self):
        return len(self.batch_sampler)


class _SkipEmpty:
    def __init__(self, collate_fn):
        self.collate_fn = collate_fn

    def __call__(self, items):
        return self.collate_fn(items) if items else None


def shard_loader(loader: DataLoader, group) -> DataLoader:
    """`loader` with every global batch cut down to this rank's share (ShardBatchSampler); an empty share comes as None."""
    rank, world = rank_world(group)
    sampler = loader.batch_sampler
    if sampler is None:
        raise ValueError("data-parallel training needs a DataLoader with a batch size (batch_size=... is the global batch)")
    if isinstance(sampler.sampler, RandomSampler) and sampler.sampler.generator is None:
        raise ValueError("data-parallel training with shuffle=True needs a seeded generator=torch.Generator() on the DataLoader: "
                         "every rank must draw the same global batches")
    return DataLoader(loader.dataset, batch_sampler=ShardBatchSampler(sampler, rank, world), collate_fn=_SkipEmpty(loader.collate_fn),
                      num_workers=loader.num_workers, pin_memory=loader.pin_memory)


def check_loss_fn(loss_fn) -> dict:
    """The keyword arguments of a fused `compute_loss` partial; anything else is refused in data-parallel mode."""
    if not (isinstance(loss_fn, functools.partial) and loss_fn.func is L.compute_loss and not loss_fn.args):
        raise ValueError("data-parallel training takes loss_fn = functools.partial(loss.compute_loss, ...) with the fused loss "
                         f"functions only (got {loss_fn!r}): a foreign loss callable cannot be reduced across ranks")
    kw = dict(loss_fn.keywords)
    if kw.get("class_loss_fn") is L.dice_loss:
        raise ValueError("data-parallel training does not support dice_loss: it is a ratio of sums over the whole batch, not a mean "
                         "(use focal_loss)")
    if not (kw.get("radius_loss_fn") is L.L1Loss and kw.get("direction_loss_fn") is L.cosine_similarity_loss
            and kw.get("class_loss_fn") is L.focal_loss):
        raise ValueError("data-parallel training takes compute_loss with radius_loss_fn=L1Loss, direction_loss_fn="
                         "cosine_similarity_loss and class_loss_fn=focal_loss (the fused HIP loss)")
    return kw


def global_loss(loss_fn, preds, targets, mask, group):
    """(this rank's weighted terms for backward, the global means as floats): one all-reduce of the count-weighted sums."""
    raw = []
    terms = loss_fn(preds, targets, mask, raw_out=raw)
    (m_r, m_d, m_f, _, n_v, n_c), = raw
    dev = targets.device
    local = torch.tensor([n_v * m_r if n_v else 0.0, n_v * m_d if n_v else 0.0, n_c * m_f if n_c else 0.0, n_v, n_c],
                         dtype=torch.float64, device=dev)
    dist.all_reduce(local, op=dist.ReduceOp.SUM, group=group)
    s_r, s_d, s_f, N_v, N_c = local.tolist()
    w_v = n_v / N_v if N_v > 0 else 0.0
    w_c = n_c / N_c if N_c > 0 else 0.0
    weighted = {"radius": terms["radius"] * w_v, "direction": terms["direction"] * w_v, "class_l": terms["class_l"] * w_c}
    nan = float("nan")
    means = {"radius": s_r / N_v if N_v > 0 else nan, "direction": s_d / N_v if N_v > 0 else nan,
             "class_l": s_f / N_c if N_c > 0 else nan}
    # the one-process run logs float32 values: round the same way
    return weighted, {k: float(torch.tensor(v, dtype=torch.float32)) for k, v in means.items()}


def all_reduce_grads(params, group) -> None:
    """One all_reduce(SUM) of every gradient (a missing one counts as zeros), copied back into .grad."""
    params = [p for p in params if p.requires_grad]
    if not params:
        return
    flat = torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1) for p in params])
    dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=group)
    offset = 0
    for p in params:
        k = p.numel()
        g = flat[offset:offset + k].view_as(p)
        if p.grad is None:
            p.grad = g.clone()
        else:
            p.grad.copy_(g)
        offset += k


def check_replicas(model, group) -> float:
    """All ranks hold bit-identical parameters and buffers: a float64 checksum gathered from every rank must agree.  Returns it."""
    with torch.no_grad():
        vals = [t.detach().double().sum() for t in list(model.parameters()) + list(model.buffers()) if t.is_floating_point()]
        mine = torch.stack(vals).sum().reshape(1)
    everyone = [torch.empty_like(mine) for _ in range(dist.get_world_size(group))]
    dist.all_gather(everyone, mine, group=group)
    sums = [float(t) for t in everyone]
    log.debug("parameter checksum per rank: %s", sums)
    if any(s != sums[0] and not (s != s and sums[0] != sums[0]) for s in sums):
        raise RuntimeError(f"data-parallel replicas diverged: parameter checksums per rank {sums}")
    return sums[0]


def empty_batch(model, device, target_cols: int = 5):
    """A zero-row batch (features, coordinates, targets, mask) for a rank that owns no tree of a global batch."""
    cin = int(model.input_conv.sequence[0].weight.shape[-1])
    return (torch.zeros((0, cin)), torch.zeros((0, 4), dtype=torch.int32), torch.zeros((0, target_cols)),
            torch.zeros(0, dtype=torch.bool))
