"""A trainable Smart_Tree: the reference's network (smart_tree/model/model.py:9-87, model_blocks.py) as a torch.nn.Module whose
sparse convolutions are HIP kernels with a backward pass (model/sparse_grad.py).

* Constructor: the reference's `Smart_Tree(input_channels, unet_planes, radius_fc_planes, direction_fc_planes, class_fc_planes)`,
  so a `training.yaml` `model._target_` swap works.  The heads are SparseFC (pointwise convolutions, as the shipped checkpoints
  hold them) and BatchNorm eps is 1e-4 (the checkpoints' attribute).
* Parameters are stored in spconv's layout [Cout, k, k, k, Cin] under the reference's key names: `state_dict()` has the
  checkpoints' keys and shapes and loads into `model.model.Smart_Tree` (the inference network) unchanged; `from_state_dict`
  goes the other way.
* BatchNorm, ReLU, the residual add, the concat and F.normalize are torch ops (train mode: batch statistics, running statistics
  updated with momentum 0.1; eval mode: running statistics).  The rulebooks and the row order are those `Smart_Tree.features`
  picks.
* Precision: float32, or mixed precision as the reference trains with `fp16: True` -- under `torch.autocast(<device type>,
  dtype=torch.float16)` (`train.train_epoch(..., fp16=True, scaler=...)`) or with float16 features the convolutions run in half
  storage with float32 sums (model/sparse_grad.py), except the direction head's output conv (see `forward`); parameters, their
  gradients and `state_dict()` stay float32.
"""
from __future__ import annotations

import math
from typing import Dict, Mapping

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from . import sparse_grad as sg
from . import sparse_ops as ops
from .model import BN_EPS


class SparseConvWeight(nn.Module):
    """One convolution's weight, spconv layout [Cout, k, k, k, Cin] (kernel offset k = (kz * 3 + ky) * 3 + kx)."""

    def __init__(self, cin: int, cout: int, k: int):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(cout, k, k, k, cin))
        bound = 1.0 / math.sqrt(cin * k ** 3)
        nn.init.uniform_(self.weight, -bound, bound)

    def forward(self, x0, nbr, n_out, nbr_t, flip, x1=None):
        cout, cin = self.weight.shape[0], self.weight.shape[-1]
        w = self.weight.reshape(cout, -1, cin).permute(1, 2, 0)  # [K, Cin, Cout]
        return sg.sparse_conv(x0, w, nbr, n_out, nbr_t, flip, x1=x1)


def _bn(c):
    bn = nn.BatchNorm1d(c, eps=BN_EPS, momentum=0.1)
    nn.init.ones_(bn.weight)  # Smart_Tree.set_bn_init
    nn.init.zeros_(bn.bias)
    return bn


class _Block(nn.Module):
    """SubMConvBlock / EncoderBlock / DecoderBlock: sequence = conv, BatchNorm, ReLU."""

    def __init__(self, cin, cout, k):
        super().__init__()
        self.sequence = nn.Sequential(SparseConvWeight(cin, cout, k), _bn(cout), nn.ReLU())

    def forward(self, x, nbr, n_out, nbr_t, flip):
        return F.relu(self.sequence[1](self.sequence[0](x, nbr, n_out, nbr_t, flip)))


class _ResBlock(nn.Module):
    """ResBlock (model_blocks.py:107-156): relu(bn(conv(relu(bn(conv(x))))) + identity(x)); identity = k1 conv if the widths differ."""

    def __init__(self, cin, cout):
        super().__init__()
        self.identity = nn.Sequential(nn.Identity() if cin == cout else SparseConvWeight(cin, cout, 1))
        self.sequence = nn.Sequential(SparseConvWeight(cin, cout, 3), _bn(cout), nn.ReLU(), SparseConvWeight(cout, cout, 3), _bn(cout))

    def forward(self, x, nbr, x1=None):
        n = x.shape[0]
        s = self.sequence
        h = F.relu(s[1](s[0](x, nbr, n, nbr, True, x1=x1)))
        h = s[4](s[3](h, nbr, n, nbr, True))
        ident = x if x1 is None else self.identity[0](x, None, n, None, False, x1=x1)
        return F.relu(h + ident)


class _UBlock(nn.Module):
    """UBlock (model_blocks.py:159-243)."""

    def __init__(self, planes):
        super().__init__()
        self.n_planes = list(planes)
        self.Head = _ResBlock(planes[0], planes[0])
        if len(planes) > 1:
            self.Encode = _Block(planes[0], planes[1], 3)
            self.U = _UBlock(planes[1:])
            self.Decode = _Block(planes[1], planes[0], 3)
            self.Tail = _ResBlock(2 * planes[0], planes[0])

    def forward(self, x, pyr, level):
        x = self.Head(x, pyr.subm[level])
        if len(self.n_planes) == 1:
            return x
        n_coarse = pyr.coords[level + 1].shape[0]
        z = self.Encode(x, pyr.down[level], n_coarse, *sg.transposed_table("down", pyr, level))
        z = self.U(z, pyr, level + 1)
        d = self.Decode(z, pyr.up[level], x.shape[0], *sg.transposed_table("up", pyr, level))
        return self.Tail(x, pyr.subm[level], x1=d)  # cat(skip, decoded) is the convolutions' concat input


class _SparseFC(nn.Module):
    """SparseFC (model_blocks.py:246-285): pointwise conv + BatchNorm + ReLU per hidden width, then a pointwise conv."""

    def __init__(self, planes, float_last=False):
        super().__init__()
        self.float_last = float_last
        mods = []
        for i in range(len(planes) - 2):
            mods += [SparseConvWeight(planes[i], planes[i + 1], 1), _bn(planes[i + 1]), nn.ReLU()]
        mods.append(SparseConvWeight(planes[-2], planes[-1], 1))
        self.sequence = nn.Sequential(*mods)

    def forward(self, x):
        n = x.shape[0]
        last = self.sequence[-1]
        for m in self.sequence:
            if m is last and self.float_last and sg.half_path(x):
                # float32 output conv in a mixed-precision step (see TrainableSmartTree.forward)
                with torch.autocast(x.device.type, enabled=False):
                    x = m(x.float(), None, n, None, False)
            elif isinstance(m, SparseConvWeight):
                x = m(x, None, n, None, False)
            elif isinstance(m, nn.ReLU):
                x = F.relu(x)
            else:
                x = m(x)
        return x


class TrainableSmartTree(nn.Module):
    def __init__(self, input_channels, unet_planes, radius_fc_planes, direction_fc_planes, class_fc_planes, bias=False, algo=None,
                 fp16: bool = False):
        super().__init__()
        if fp16:
            raise ValueError("TrainableSmartTree keeps float32 parameters and has no fp16 argument: for mixed-precision training "
                             "run it under torch.autocast(device_type, dtype=torch.float16), e.g. train_epoch(..., fp16=True, scaler=...)")
        if bias:
            raise ValueError("the network is built without bias (as the reference's default)")
        self.input_conv = _Block(input_channels, unet_planes[0], 1)
        self.UNet = _UBlock(unet_planes)
        self.radius_head = _SparseFC(radius_fc_planes)
        self.direction_head = _SparseFC(direction_fc_planes, float_last=True)
        self.class_head = _SparseFC(class_fc_planes)
        self.depth = len(unet_planes) - 1
        self.use_bricks = True
        self.spatial_order = True

    @classmethod
    def from_state_dict(cls, sd: Mapping[str, torch.Tensor]) -> "TrainableSmartTree":
        """The architecture read from a checkpoint's keys and shapes (as `model.model.Smart_Tree` does), the values loaded strictly."""
        sd = {k: torch.as_tensor(np.asarray(v)) if not torch.is_tensor(v) else v.detach().cpu() for k, v in sd.items()}
        depth = 0
        while f"UNet.{'U.' * (depth + 1)}Head.sequence.0.weight" in sd:
            depth += 1
        planes = [int(sd[f"UNet.{'U.' * l}Head.sequence.0.weight"].shape[0]) for l in range(depth + 1)]
        cin = int(sd["input_conv.sequence.0.weight"].shape[-1])

        def fc(name):
            idx = sorted(int(k.split(".")[2]) for k in sd if k.startswith(f"{name}.sequence.") and k.endswith(".weight")
                         and sd[k].ndim == 5)
            ws = [sd[f"{name}.sequence.{i}.weight"] for i in idx]
            return [int(ws[0].shape[-1])] + [int(w.shape[0]) for w in ws]

        net = cls(cin, planes, fc("radius_head"), fc("direction_head"), fc("class_head"))
        net.load_state_dict({k: v.float() if v.is_floating_point() else v for k, v in sd.items()}, strict=True)
        return net

    def _pyramid(self, sparse_input, feats):
        """Rulebooks and row order exactly as `Smart_Tree.features` picks them: (pyr, order or None, feats in that order)."""
        coords = sparse_input.indices.contiguous()
        blk_seg, n_seg = getattr(sparse_input, "blk_seg", None), getattr(sparse_input, "n_seg", 1)
        reorder = self.spatial_order and coords.shape[0] > 1
        hint = getattr(sparse_input, "brick_hint", None)
        bricks = ops.brick_pyramid(coords, self.depth, hint[0], hint[1], blk_seg, n_seg) if reorder and hint and self.use_bricks else None
        if bricks is not None:
            pyr, order = bricks
        else:
            order = ops.spatial_order(coords) if reorder else None
            if order is not None:
                coords = ops.move_rows(coords, order)
            pyr = ops.build_pyramid(coords, self.depth, blk_seg, n_seg)
        if order is not None:
            feats = sg.move_rows(feats, order)
        return pyr, order, feats

    def features(self, sparse_input) -> torch.Tensor:
        feats = sparse_input.features.contiguous()
        if feats.dtype not in (torch.float32, torch.float16):
            raise ValueError(f"TrainableSmartTree takes float32 or float16 features (got {feats.dtype})")
        pyr, order, x = self._pyramid(sparse_input, feats)
        x = self.input_conv(x, None, x.shape[0], None, False)
        x = self.UNet(x, pyr, 0)
        if order is not None:
            x = sg.move_rows(x, order, scatter=True)
        return x

    def forward(self, sparse_input) -> Dict[str, torch.Tensor]:
        x = self.features(sparse_input)
        # Mixed precision: the direction head's last (pointwise, 4 -> 3) conv runs in float32, so F.normalize sees float32.  A row whose
        # hidden ReLUs are all off has an exactly zero direction; normalize's gradient there is g / eps (eps = 1e-12), finite in
        # float32 and masked by the ReLUs below, but inf once rounded to half -- then 0 * inf = NaN in that conv's weight gradient and
        # GradScaler would skip every step while such rows exist (a random-init network has many).
        return {"radius": self.radius_head(x), "direction": F.normalize(self.direction_head(x)), "class_l": self.class_head(x)}
