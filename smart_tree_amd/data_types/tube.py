"""Tapered tube segment types (reference `smart_tree/data_types/tube.py:9-50`)."""
from __future__ import annotations

from dataclasses import dataclass
from typing import List

import torch


@dataclass
class Tube:
    a: torch.Tensor  # [3] start point
    b: torch.Tensor  # [3] end point
    r1: torch.Tensor  # [1] start radius
    r2: torch.Tensor  # [1] end radius


@dataclass
class CollatedTube:
    a: torch.Tensor  # [M,3]
    b: torch.Tensor  # [M,3]
    r1: torch.Tensor  # [1,M]
    r2: torch.Tensor  # [1,M]

    def to(self, device) -> "CollatedTube":
        return CollatedTube(self.a.to(device), self.b.to(device), self.r1.to(device), self.r2.to(device))


def collate_tubes(tubes: List[Tube]) -> CollatedTube:
    """Stack a list of tubes; r1/r2 become row vectors [1,M] (reference tube.py:43-50)."""
    stack = lambda name: torch.cat([getattr(t, name).reshape(-1) for t in tubes])
    return CollatedTube(stack("a").reshape(-1, 3), stack("b").reshape(-1, 3),
                        stack("r1").reshape(1, -1), stack("r2").reshape(1, -1))


def _tube_arrays(tubes):
    """(a [M,3], b [M,3], r1 [M], r2 [M]) float32 from a list of Tube, a CollatedTube or such a tuple."""
    if isinstance(tubes, (list,)) and (not tubes or isinstance(tubes[0], Tube)):
        if not tubes:
            z = torch.zeros((0, 3), dtype=torch.float32)
            return z, z.clone(), z[:, 0].clone(), z[:, 0].clone()
        tubes = collate_tubes(tubes)
    a, b, r1, r2 = (tubes.a, tubes.b, tubes.r1, tubes.r2) if isinstance(tubes, CollatedTube) else tubes
    f = lambda t: torch.as_tensor(t).to(torch.float32).contiguous()
    return f(a).reshape(-1, 3), f(b).reshape(-1, 3), f(r1).reshape(-1), f(r2).reshape(-1)


def sample_tubes_device(a, b, r1, r2, spacing: float):
    """`st_sample_tubes_*` (csrc/skeleton_eval.hip) on device tensors: (pts [N,3], radius [N], tube_of [N] int32,
    count [M] int32, off [M] int32).  One read-back (the total), then the fill is enqueued."""
    import ctypes

    from .. import _lib

    L = _lib.lib()
    dev = a.device
    f = lambda t: t.to(dev).float().contiguous()
    a, b, r1, r2 = f(a).reshape(-1, 3), f(b).reshape(-1, 3), f(r1).reshape(-1), f(r2).reshape(-1)
    m = a.shape[0]
    count = torch.empty(m, dtype=torch.int32, device=dev)
    off = torch.empty(m, dtype=torch.int32, device=dev)
    nbytes = L.st_sample_tubes_workspace_bytes(m)
    ws = _lib.workspace(nbytes, dev)
    total = ctypes.c_int64(0)
    s = _lib.stream(dev)
    _lib.check(L.st_sample_tubes_count(_lib.ptr(a), _lib.ptr(b), m, float(spacing), _lib.ptr(count), _lib.ptr(off),
                                       ctypes.byref(total), _lib.ptr(ws), nbytes, s))
    n = total.value
    pts = torch.empty((n, 3), dtype=torch.float32, device=dev)
    rad = torch.empty(n, dtype=torch.float32, device=dev)
    tube_of = torch.empty(n, dtype=torch.int32, device=dev)
    _lib.check(L.st_sample_tubes_fill(_lib.ptr(a), _lib.ptr(b), _lib.ptr(r1), _lib.ptr(r2), m, float(spacing), _lib.ptr(off), n,
                                      _lib.ptr(pts), _lib.ptr(rad), _lib.ptr(tube_of), s))
    return pts, rad, tube_of, count, off


def sample_tubes_host(a, b, r1, r2, spacing: float):
    """The same definition as a plain torch expression (host tensors): (pts, radius, tube_of, count, off)."""
    if not spacing > 0:
        raise ValueError(f"sample tubes: spacing must be > 0 (got {spacing})")
    a, b, r1, r2 = a.float().reshape(-1, 3), b.float().reshape(-1, 3), r1.float().reshape(-1), r2.float().reshape(-1)
    v = b - a
    length = ((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]).sqrt()
    live = torch.isfinite(length) & (length > 0)
    count = torch.where(live, torch.ceil(length.double() / float(spacing)), torch.zeros((), dtype=torch.float64)).to(torch.int64)
    if int(count.sum()) >= 2 ** 31:
        raise ValueError(f"sample tubes: {int(count.sum())} samples at spacing {spacing}, the limit is 2^31 - 1")
    off = torch.cumsum(count, 0) - count
    tube_of = torch.repeat_interleave(torch.arange(a.shape[0], device=a.device), count)
    k = torch.arange(tube_of.shape[0], device=a.device) - off[tube_of]
    f = k.float() / count[tube_of].float()
    pts = a[tube_of] + v[tube_of] * f[:, None]
    rad = r1[tube_of] + (r2 - r1)[tube_of] * f
    return pts, rad, tube_of.to(torch.int32), count.to(torch.int32), off.to(torch.int32)


def sample_tubes(tubes, spacing: float):
    """Reference `sample_tubes` (data_types/tube.py:53-74): points every `spacing` along each tube with interpolated radii,
    -> (pts [N,3], radius [N]).  Tube i gives n = ceil(len / spacing) samples a + v * (k / n), k < n, with radius
    r1 + (r2 - r1) * (k / n) -- the reference's rounded `arange` step gives n or n + 1 (DESIGN.md "Evaluation").  Device
    tensors go through the HIP kernel, host tensors through the torch expression of the same definition."""
    a, b, r1, r2 = _tube_arrays(tubes)
    pts, rad = (sample_tubes_device if a.is_cuda else sample_tubes_host)(a, b, r1, r2, spacing)[:2]
    return pts, rad
