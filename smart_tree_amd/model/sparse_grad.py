"""Autograd for the sparse convolution and the row permutation (training).

The reference trains through spconv's backward (smart_tree/model/train.py:24-58).  Here, in either storage type:
  * data gradient (dgrad): the forward kernel over the TRANSPOSED neighbour table with transposed weights -- gather form, no
    atomics, deterministic (`transposed_table` says which table that is);
  * weight gradient (wgrad): `conv_wgrad`, the one deterministic kernel family of csrc/sparse_conv_grad.hip, float32 sums and a
    float32 dW for both storage types;
  * `move_rows`: the gather's backward is the scatter and the other way round.
BatchNorm, ReLU, the residual add, the concat and F.normalize stay torch ops around these.

The two storage types:
  * float32: `sparse_ops.sparse_conv` and `st_sparse_conv_wgrad`;
  * half (mixed-precision training, the reference's `fp16: True`): under `torch.autocast(<device type>, dtype=torch.float16)`, or
    with float16 features, the convolution casts features and weight to half (as spconv's `custom_fwd(cast_inputs=torch.float16)`
    convs do), runs `sparse_ops.sparse_conv_half` (csrc/sparse_conv_half.hip) and returns half; `st_sparse_conv_wgrad_h` gives the
    float32 master weight its float32 dW -- never rounded to half (spconv would return a half dW that autograd then widens: an
    intended difference).  Autocast to any other dtype keeps the float32 path.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from .. import _lib
from . import sparse_ops as ops


def conv_wgrad(x0: torch.Tensor, x1: Optional[torch.Tensor], nbr: Optional[torch.Tensor], n_out: int, dy: torch.Tensor,
               K: int) -> torch.Tensor:
    """dW [K, Cin, Cout] = sum over live pairs (i = nbr[k][o], o) of cat(x0, x1)[i]^T dy[o]; nbr None = pointwise (K = 1).
    x0 / x1 / dy all float32 (st_sparse_conv_wgrad) or all float16 (st_sparse_conv_wgrad_h); dW float32, float32 sums, deterministic."""
    L = _lib.lib()
    if x0.dtype not in (torch.float32, torch.float16) or dy.dtype != x0.dtype or (x1 is not None and x1.dtype != x0.dtype):
        raise ValueError("conv_wgrad takes features and gradients that are all float32 or all float16")
    ws_bytes, run = ((L.st_sparse_conv_wgrad_workspace_bytes, L.st_sparse_conv_wgrad) if x0.dtype == torch.float32 else
                     (L.st_sparse_conv_wgrad_h_workspace_bytes, L.st_sparse_conv_wgrad_h))
    x0 = x0.contiguous()
    x1 = x1.contiguous() if x1 is not None else None
    dy = dy.contiguous()
    c0 = x0.shape[1]
    cin = c0 + (x1.shape[1] if x1 is not None else 0)
    cout = dy.shape[1]
    nbr_ptr, nbr_stride = ops._nbr_args(nbr)
    dw = torch.empty((K, cin, cout), dtype=torch.float32, device=x0.device)
    ws = _lib.workspace(ws_bytes(K, cin, cout, n_out), x0.device)
    _lib.check(run(_lib.ptr(x0), c0, _lib.ptr(x1), cin, nbr_ptr, K, n_out, nbr_stride, _lib.ptr(dy), cout, _lib.ptr(dw), _lib.ptr(ws),
                   ws.numel(), _lib.stream(x0.device)))
    return dw


def half_path(x0: torch.Tensor) -> bool:
    """The convolution runs in half storage: float16 features, or float16 autocast on the features' device type."""
    if x0.dtype == torch.float16:
        return True
    dt = x0.device.type
    return torch.is_autocast_enabled(dt) and torch.get_autocast_dtype(dt) == torch.float16


def transposed_table(kind: str, pyr, level: int) -> Tuple[Optional[torch.Tensor], bool]:
    """(table, flip) that runs a convolution's data gradient as a forward convolution: dx = conv(dy, W', table), where
    W'[k] = W[K-1-k]^T if flip else W[k]^T.
      "subm"  (k3 submanifold, table pyr.subm[level]):  nbr[k][o] = i  <=>  nbr[26-k][i] = o: the SAME table, offsets flipped.
      "down"  (k3 s2, table pyr.down[level]):           nbr_down[k][o] = i  <=>  nbr_up[k][i] = o: pyr.up[level].
      "up"    (inverse k3, table pyr.up[level]):        the other way: pyr.down[level].
      "point" (k1):                                      no table (dx = dy W^T row by row)."""
    if kind == "subm":
        return pyr.subm[level], True
    if kind == "down":
        return pyr.up[level], False
    if kind == "up":
        return pyr.down[level], False
    assert kind == "point", kind
    return None, False


class SparseConvFn(torch.autograd.Function):
    """y = sum_k cat(x0, x1)[nbr[k]] W[k] (w [K, Cin, Cout]), no epilogue; backward = dgrad through the forward kernel on
    (nbr_t, flip) from `transposed_table`, and wgrad."""

    @staticmethod
    def forward(ctx, x0, x1, w, nbr, n_out, nbr_t, flip):
        ctx.half = half_path(x0)
        ctx.dtypes = (x0.dtype, x1.dtype if x1 is not None else None, w.dtype)
        storage = torch.float16 if ctx.half else x0.dtype  # (.to(storage) returns the same tensor on the float32 path)
        x0 = x0.detach().to(storage).contiguous()
        x1 = x1.detach().to(storage).contiguous() if x1 is not None else None
        w = w.detach().to(storage).contiguous()
        y = (ops.sparse_conv_half if ctx.half else ops.sparse_conv)(x0, w, nbr, int(n_out), x1=x1)
        ctx.save_for_backward(x0, x1, w)
        ctx.nbr, ctx.nbr_t, ctx.flip, ctx.n_out = nbr, nbr_t, flip, int(n_out)
        return y

    @staticmethod
    def backward(ctx, dy):
        x0, x1, w = ctx.saved_tensors  # in the storage dtype
        dy = dy.to(w.dtype).contiguous()
        K = w.shape[0]
        dx0 = dx1 = dw = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            wt = (w.flip(0) if ctx.flip else w).transpose(1, 2).contiguous()  # [K, Cout, Cin]
            dx = (ops.sparse_conv_half if ctx.half else ops.sparse_conv)(dy, wt, ctx.nbr_t, x0.shape[0])
            if x1 is None:
                dx0 = dx
            else:
                c0 = x0.shape[1]
                dx0, dx1 = dx[:, :c0].contiguous(), dx[:, c0:].contiguous()
            dx0 = dx0.to(ctx.dtypes[0])
            dx1 = dx1.to(ctx.dtypes[1]) if dx1 is not None else None
        if ctx.needs_input_grad[2]:
            dw = conv_wgrad(x0, x1, ctx.nbr, ctx.n_out, dy, K).to(ctx.dtypes[2])  # float32 for a float32 weight
        return dx0, dx1, dw, None, None, None, None


def sparse_conv(x0: torch.Tensor, w: torch.Tensor, nbr: Optional[torch.Tensor], n_out: int, nbr_t: Optional[torch.Tensor],
                flip: bool, x1: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Differentiable `sparse_ops.sparse_conv` without epilogue (see SparseConvFn); half storage under float16 autocast or with
    float16 features (`half_path`)."""
    return SparseConvFn.apply(x0, x1, w, nbr, n_out, nbr_t, flip)


class MoveRowsFn(torch.autograd.Function):
    """`sparse_ops.move_rows`: x[order] (gather) or out[order] = x (scatter); each is the other's backward."""

    @staticmethod
    def forward(ctx, x, order, scatter):
        ctx.order, ctx.scatter = order, bool(scatter)
        return ops.move_rows(x, order, scatter=scatter)

    @staticmethod
    def backward(ctx, g):
        return ops.move_rows(g.contiguous(), ctx.order, not ctx.scatter), None, None


def move_rows(x: torch.Tensor, order: torch.Tensor, scatter: bool = False) -> torch.Tensor:
    return MoveRowsFn.apply(x, order, scatter)
