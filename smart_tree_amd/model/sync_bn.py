"""Synchronised BatchNorm for data-parallel training (csrc/batchnorm.hip; DESIGN.md "Training: data parallel").

The reference trains with BatchNorm over the whole batch of `batch_size` trees.  With the batch split over W ranks, every BatchNorm
layer must still normalise with the statistics of the global batch, so one training step on W ranks computes what one process
given the whole batch computes (up to float rounding).  `SyncBatchNorm` does that with four HIP passes and two small all-reduces:

  train forward:   st_bn_stats -> all_reduce [sum | sumsq | n] (float64) -> global mean, biased variance, invstd; running mean and
                   running variance (torch's unbiased N / (N - 1) factor, momentum 0.1: every rank holds the same buffers)
                   -> st_bn_apply
  train backward:  st_bn_backward_stats -> all_reduce [sum dy | sum dy * xhat] -> st_bn_backward_apply
  eval:            st_bn_apply with the running statistics, no collective

dgamma and dbeta leave the Function as THIS rank's sums: the step's gradient all-reduce (model/data_parallel.py) adds them up;
returning the global sums would count them W times.

The module holds exactly nn.BatchNorm1d's state (weight, bias, running_mean, running_var, num_batches_tracked), so `state_dict()`
keys and shapes are the checkpoints'.  With no group the module is a plain single-process BatchNorm on the same kernels.  Float32
input, or float16 under autocast (float32 math and affine parameters, half in and out), as torch's BatchNorm does there.
"""
from __future__ import annotations

import torch
import torch.distributed as dist
from torch import nn

from .. import _lib
from .model import BN_EPS


def _all_reduce(t: torch.Tensor, group) -> None:
    if group is not None:
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)


def _check_input(x: torch.Tensor, C: int) -> torch.Tensor:
    if x.dim() != 2 or x.shape[1] != C:
        raise ValueError(f"SyncBatchNorm({C}) takes [n, {C}] rows (got {tuple(x.shape)})")
    if x.dtype not in (torch.float32, torch.float16):
        raise ValueError(f"SyncBatchNorm takes float32 or float16 rows (got {x.dtype})")
    return x.contiguous()


def batch_stats(x: torch.Tensor) -> torch.Tensor:
    """st_bn_stats: [sum x | sum x^2 | n] per channel of [n, C] rows, float64 [2C + 1] on x's device."""
    L = _lib.lib()
    n, C = x.shape
    out = torch.empty(2 * C + 1, dtype=torch.float64, device=x.device)
    ws = _lib.workspace(L.st_bn_workspace_bytes(n, C), x.device)
    _lib.check(L.st_bn_stats(_lib.ptr(x), int(x.dtype == torch.float16), n, C, _lib.ptr(out), _lib.ptr(ws), ws.numel(),
                             _lib.stream(x.device)))
    return out


def apply(x: torch.Tensor, mean: torch.Tensor, invstd: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """st_bn_apply: (x - mean) * invstd * weight + bias, in x's dtype; the four vectors float32 [C]."""
    L = _lib.lib()
    n, C = x.shape
    y = torch.empty_like(x)
    vecs = [v.detach().float().contiguous() for v in (mean, invstd, weight, bias)]
    _lib.check(L.st_bn_apply(_lib.ptr(x), int(x.dtype == torch.float16), n, C, *(_lib.ptr(v) for v in vecs), _lib.ptr(y),
                             _lib.stream(x.device)))
    return y


def backward_stats(x: torch.Tensor, dy: torch.Tensor, mean: torch.Tensor, invstd: torch.Tensor) -> torch.Tensor:
    """st_bn_backward_stats: [sum dy | sum dy * xhat] per channel, float64 [2C]."""
    L = _lib.lib()
    n, C = x.shape
    out = torch.empty(2 * C, dtype=torch.float64, device=x.device)
    ws = _lib.workspace(L.st_bn_workspace_bytes(n, C), x.device)
    _lib.check(L.st_bn_backward_stats(_lib.ptr(x), _lib.ptr(dy), int(x.dtype == torch.float16), n, C, _lib.ptr(mean), _lib.ptr(invstd),
                                      _lib.ptr(out), _lib.ptr(ws), ws.numel(), _lib.stream(x.device)))
    return out


def backward_apply(x: torch.Tensor, dy: torch.Tensor, mean: torch.Tensor, invstd: torch.Tensor, weight: torch.Tensor,
                   sums: torch.Tensor, count: torch.Tensor) -> torch.Tensor:
    """st_bn_backward_apply: dx = weight * invstd * (dy - sum_dy / N - xhat * sum_dy_xhat / N); sums float64 [2C], count float64 [1]."""
    L = _lib.lib()
    n, C = x.shape
    dx = torch.empty_like(x)
    w = weight.detach().float().contiguous()
    _lib.check(L.st_bn_backward_apply(_lib.ptr(x), _lib.ptr(dy), int(x.dtype == torch.float16), n, C, _lib.ptr(mean), _lib.ptr(invstd),
                                      _lib.ptr(w), _lib.ptr(sums), _lib.ptr(count), _lib.ptr(dx), _lib.stream(x.device)))
    return dx


class _SyncBNFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, num_batches_tracked, eps, momentum, group):
        C = weight.shape[0]
        x = _check_input(x, C)
        with torch.autocast(x.device.type, enabled=False):
            stats = batch_stats(x)
            _all_reduce(stats, group)
            count = stats[2 * C:].clone()  # global row count N, float64 [1], on the device
            mean64 = stats[:C] / count
            var64 = (stats[C:2 * C] / count - mean64 * mean64).clamp_min(0.0)  # biased
            mean = mean64.float().contiguous()
            invstd = (var64 + eps).rsqrt().float().contiguous()
            with torch.no_grad():
                unbiased = var64 * count / (count - 1.0).clamp_min(1.0)
                running_mean.mul_(1.0 - momentum).add_(mean64.to(running_mean.dtype), alpha=momentum)
                running_var.mul_(1.0 - momentum).add_(unbiased.to(running_var.dtype), alpha=momentum)
                num_batches_tracked.add_(1)
            y = apply(x, mean, invstd, weight, bias)
        ctx.save_for_backward(x, weight, mean, invstd, count)
        ctx.group = group
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, mean, invstd, count = ctx.saved_tensors
        C = weight.shape[0]
        dy = dy.contiguous().to(x.dtype)
        with torch.autocast(x.device.type, enabled=False):
            sums = backward_stats(x, dy, mean, invstd)
            dbeta = sums[:C].float()  # this rank's sums: the gradient all-reduce adds the ranks up
            dgamma = sums[C:].float()
            _all_reduce(sums, ctx.group)
            dx = backward_apply(x, dy, mean, invstd, weight, sums, count)
        need = ctx.needs_input_grad
        return (dx if need[0] else None, dgamma if need[1] else None, dbeta if need[2] else None,
                None, None, None, None, None, None)


class SyncBatchNorm(nn.Module):
    """nn.BatchNorm1d(num_features, eps, momentum) over [n, C] rows with the batch statistics of every rank in `group` (None: this
    process's rows only).  Same parameters, buffers and state_dict keys as nn.BatchNorm1d."""

    def __init__(self, num_features: int, eps: float = BN_EPS, momentum: float = 0.1, group=None):
        super().__init__()
        self.num_features = int(num_features)
        self.eps = float(eps)
        self.momentum = float(momentum)
        self.affine = True
        self.track_running_stats = True
        self.group = group
        self.weight = nn.Parameter(torch.ones(num_features))
        self.bias = nn.Parameter(torch.zeros(num_features))
        self.register_buffer("running_mean", torch.zeros(num_features))
        self.register_buffer("running_var", torch.ones(num_features))
        self.register_buffer("num_batches_tracked", torch.tensor(0, dtype=torch.long))

    def extra_repr(self) -> str:
        world = dist.get_world_size(self.group) if self.group is not None else 1
        return f"{self.num_features}, eps={self.eps}, momentum={self.momentum}, ranks={world}"

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self.training:
            return _SyncBNFn.apply(x, self.weight, self.bias, self.running_mean, self.running_var, self.num_batches_tracked,
                                   self.eps, self.momentum, self.group)
        x = _check_input(x, self.num_features)
        if torch.is_grad_enabled() and (x.requires_grad or self.weight.requires_grad):
            raise NotImplementedError("SyncBatchNorm in eval mode runs forward only (torch.no_grad()); train mode has the backward")
        with torch.autocast(x.device.type, enabled=False):
            invstd = (self.running_var.double() + self.eps).rsqrt().float()
            return apply(x, self.running_mean, invstd, self.weight, self.bias)

    @classmethod
    def from_batchnorm(cls, bn: nn.BatchNorm1d, group=None) -> "SyncBatchNorm":
        if not (bn.affine and bn.track_running_stats) or bn.momentum is None:
            raise ValueError("SyncBatchNorm replaces an affine BatchNorm1d with running statistics and a fixed momentum")
        out = cls(bn.num_features, bn.eps, bn.momentum, group)
        with torch.no_grad():
            out.weight = nn.Parameter(bn.weight.detach().clone(), requires_grad=bn.weight.requires_grad)
            out.bias = nn.Parameter(bn.bias.detach().clone(), requires_grad=bn.bias.requires_grad)
            for name in ("running_mean", "running_var", "num_batches_tracked"):
                setattr(out, name, getattr(bn, name).detach().clone())
        out.train(bn.training)
        return out


def convert_sync_batchnorm(model: nn.Module, group=None) -> nn.Module:
    """Swap every nn.BatchNorm1d of `model` (the `_bn`s of a TrainableSmartTree) for a SyncBatchNorm on `group`, in place, with its
    parameters and running statistics: each new module sits at the old one's name (nn.Sequential indices included).  Build the
    optimiser after this call: the parameters are new tensors.  Returns `model`."""
    for parent in list(model.modules()):
        for name, child in list(parent.named_children()):
            if isinstance(child, nn.BatchNorm1d):
                setattr(parent, name, SyncBatchNorm.from_batchnorm(child, group))
            elif isinstance(child, SyncBatchNorm):
                child.group = group
    return model
