"""Half-precision sparse-convolution training kernels: st_sparse_conv_h_fwd (forward, and the data gradient over the transposed table)
and st_move_rows_h (csrc/sparse_conv_half.hip), st_sparse_conv_wgrad_h (the half policy of csrc/sparse_conv_grad.hip), through
model/sparse_grad.py, on the CPU sanitizer build and on the GPU.

* Small-integer data: every product and partial sum is exact in float32, so the forward and the data gradient must equal the float64
  contraction rounded once to half, and the weight gradient the float64 one, bit for bit.
* Real values: |y - round_half(y64)| <= 1 half ulp of y64 + 32 * 2^-24 * sum |x||w|; dW within 32 * 2^-24 * sum |x||dy|.
* An inf in one row of dy reaches exactly the dx rows and dW offsets that row has a live pair with; two calls give the same bits."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import unet_oracle as uo
from smart_tree_amd.model import sparse_grad as sg
from smart_tree_amd.model import sparse_ops as ops
from test_conv_grad import _coords, _table

CSRC = Path(__file__).resolve().parents[1] / "smart_tree_amd" / "csrc"
SRC = {"HF_MFMA_CASE": CSRC / "sparse_conv_half.hip", "HF_VEC_CASE": CSRC / "sparse_conv_half.hip", "HW_FORM_CASE": CSRC / "sparse_conv_grad.hip"}
U = 32 * 2.0 ** -24  # accumulation bound per unit of sum |a| |b|


def _fwd_instance(cin, cout, c0):
    """The kernel instance st_sparse_conv_h_fwd launches (mirrors its dispatch; 16-byte / 8-byte aligned tensors)."""
    if cin >= 16 and cout >= 16:
        ct = 1 if cout <= 16 else 2 if cout <= 32 else 3 if cout <= 48 else 4
        return ("HF_MFMA_CASE", str(ct), cin % 8 == 0 and c0 % 8 == 0)
    return ("HF_VEC_CASE", "4" if cout <= 4 else "8", cin % 4 == 0 and c0 % 4 == 0)


def _wgrad_instance(cin, cout):
    pad = lambda c: (c + 15) // 16 * 16
    return ("HW_FORM_CASE", "true" if cin >= 16 and cout >= 16 and pad(cin) + pad(cout) <= 512 else "false")


# (kind, Cin, Cout, c0): the training config (3 -> 8, planes 8 / 16 / 32), the shipped widths (8 / 16 / 32 / 64), odd widths
# (6 / 10 / 18 / 34 / 5), the heads, every Tail concat split (cat(skip, decoded) into the k3 conv and the k1 identity); the data
# gradient runs each one's transposed shape.  Both sides of the matrix / vector switch (16 channels), of every column-tile count, the
# aligned and unaligned loads, and wgrad's tile groupings (1, 2, 3, 4, 16 and > 16 tiles, and past the matrix form's staging limit).
SHAPES = [("point", 3, 8, 3), ("point", 3, 6, 3), ("subm", 8, 8, 8), ("down", 8, 16, 8), ("up", 16, 8, 16), ("subm", 16, 16, 16),
          ("down", 16, 32, 16), ("up", 32, 16, 32), ("subm", 32, 32, 32), ("down", 32, 64, 32), ("up", 64, 32, 64),
          ("subm", 64, 64, 64),
          ("subm", 16, 8, 8), ("subm", 32, 16, 16), ("subm", 64, 32, 32), ("point", 16, 8, 8), ("point", 32, 16, 16), ("point", 64, 32, 32),
          ("subm", 6, 6, 6), ("down", 6, 10, 6), ("subm", 10, 10, 10), ("down", 10, 18, 10), ("up", 18, 10, 18), ("subm", 18, 18, 18),
          ("down", 18, 34, 18), ("up", 34, 18, 34), ("subm", 34, 34, 34), ("subm", 12, 6, 6), ("subm", 20, 10, 10), ("subm", 36, 18, 18),
          ("subm", 68, 34, 34), ("point", 12, 6, 6), ("point", 20, 10, 10), ("point", 36, 18, 18), ("point", 68, 34, 34),
          ("point", 8, 4, 8), ("point", 4, 1, 4), ("point", 4, 2, 4), ("point", 4, 3, 4), ("point", 8, 8, 8),
          ("point", 6, 5, 6), ("point", 5, 3, 5), ("point", 3, 1, 3), ("point", 3, 3, 3),
          ("subm", 15, 16, 15), ("subm", 16, 15, 16), ("subm", 17, 16, 17), ("subm", 16, 17, 16), ("subm", 16, 48, 16),
          ("point", 64, 80, 64), ("point", 16, 500, 16), ("subm", 24, 24, 12), ("subm", 16, 16, 5)]
IDS = [f"{k}-{a}x{b}-c0{c}" for k, a, b, c in SHAPES]


def _int_data(n_in, cin, cout, n_out, K, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-2, 3, (n_in, cin), generator=g).half()
    w = torch.randint(-2, 3, (K, cin, cout), generator=g).float()
    dy = torch.randint(-2, 3, (n_out, cout), generator=g).half()
    return x, w, dy


def _run(x, w, nbr, n_out, nbr_t, flip, dy, c0, device):
    """y, dx, dW through SparseConvFn's half path (float16 features, float32 master weight)."""
    x0 = x[:, :c0].contiguous().to(device).requires_grad_(True)
    x1 = x[:, c0:].contiguous().to(device).requires_grad_(True) if c0 < x.shape[1] else None
    wd = w.to(device).requires_grad_(True)
    y = sg.sparse_conv(x0, wd, nbr, n_out, nbr_t, flip, x1=x1)
    assert y.dtype == torch.float16
    y.backward(dy.to(device))
    dx = x0.grad if x1 is None else torch.cat([x0.grad, x1.grad], 1)
    assert dx.dtype == torch.float16 and wd.grad.dtype == torch.float32
    return y.detach().cpu(), dx.detach().cpu(), wd.grad.detach().cpu()


def _oracle64(x, w, nbr, n_out, dy):
    """float64 (y, dx, dW) and the bounds (sum |x||w|, sum |dy||w|, sum |x||dy|) through the oracle's convolution."""
    table = nbr.cpu().numpy().astype(np.int64) if nbr is not None else np.arange(x.shape[0], dtype=np.int64)[None]

    def run(xv, wv, dyv):
        xv = xv.detach().double().cpu().requires_grad_(True)
        ws = wv.detach().double().cpu().permute(2, 0, 1).contiguous().requires_grad_(True)
        y = uo.sparse_conv(xv, table, ws, n_out)
        y.backward(dyv.detach().double().cpu())
        return y.detach(), xv.grad, ws.grad.permute(1, 2, 0)

    y, dx, dw = run(x, w.half(), dy)
    by, bx, bw = run(x.abs(), w.half().abs(), dy.abs())
    return y, dx, dw, by, bx, bw


def _bits_equal(got, ref_half):
    return torch.equal(got.view(torch.int16), ref_half.view(torch.int16))


@pytest.mark.parametrize("kind,cin,cout,c0", SHAPES, ids=IDS)
def test_half_conv_grad_exact(backend, kind, cin, cout, c0):
    nbr, n_in, n_out, nbr_t, flip = _table(kind, backend)
    K = 1 if nbr is None else 27
    x, w, dy = _int_data(n_in, cin, cout, n_out, K, seed=cin * 100 + cout)
    y, dx, dw = _run(x, w, nbr, n_out, nbr_t, flip, dy, c0, backend)
    y64, dx64, dw64, *_ = _oracle64(x, w, nbr, n_out, dy)
    assert _bits_equal(y, y64.half()), "forward"
    assert _bits_equal(dx, dx64.half()), "data gradient"
    assert torch.equal(dw.double(), dw64), "weight gradient"
    y2, dx2, dw2 = _run(x, w, nbr, n_out, nbr_t, flip, dy, c0, backend)  # deterministic
    assert _bits_equal(y2, y) and _bits_equal(dx2, dx) and torch.equal(dw2, dw)


def test_every_dispatched_instance_has_a_case():
    """Each instance the dispatch macros of sparse_conv_half.hip (forward) and sparse_conv_grad.hip (weight gradient) name is reached by
    a case of SHAPES (forward or its transpose)."""
    named = set()
    for macro in ("HF_MFMA_CASE", "HF_VEC_CASE", "HW_FORM_CASE"):
        for arg in re.findall(rf"^\s*{macro}\((\w+)\)\s*$", SRC[macro].read_text(), re.M):
            named.add((macro, arg))
    assert len(named) == 8, named
    reached = set()
    for kind, cin, cout, c0 in SHAPES:
        for inst in (_fwd_instance(cin, cout, c0), _fwd_instance(cout, cin, cout)):
            reached.add(inst[:2])
        reached.add(_wgrad_instance(cin, cout))
    assert named <= reached, f"instances without a case: {sorted(named - reached)}"
    # both load forms of each forward form
    loads = {(_fwd_instance(a, b, c)[0], _fwd_instance(a, b, c)[2]) for _, a, b, c in SHAPES}
    assert loads == {("HF_MFMA_CASE", True), ("HF_MFMA_CASE", False), ("HF_VEC_CASE", True), ("HF_VEC_CASE", False)}


def _ulp_half(v):
    """One half-precision ulp at |v| (subnormal spacing 2^-24 below 2^-14)."""
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -14)))
    return torch.pow(2.0, e - 10)


@pytest.mark.parametrize("kind,cin,cout,c0", [SHAPES[i] for i in (0, 2, 3, 4, 5, 8, 11, 13, 23, 36, 48, 49)],
                         ids=[IDS[i] for i in (0, 2, 3, 4, 5, 8, 11, 13, 23, 36, 48, 49)])
def test_half_conv_grad_accuracy(backend, kind, cin, cout, c0):
    nbr, n_in, n_out, nbr_t, flip = _table(kind, backend)
    K = 1 if nbr is None else 27
    g = torch.Generator().manual_seed(7 + cin + 3 * cout)
    x = torch.randn(n_in, cin, generator=g).half()
    w = torch.randn(K, cin, cout, generator=g) / np.sqrt(K * cin)
    dy = torch.randn(n_out, cout, generator=g).half()
    y, dx, dw = _run(x, w, nbr, n_out, nbr_t, flip, dy, c0, backend)
    y64, dx64, dw64, by, bx, bw = _oracle64(x, w, nbr, n_out, dy)
    worst = {}
    for name, got, ref, bound in (("y", y, y64, by), ("dx", dx, dx64, bx)):
        err = (got.double() - ref.half().double()).abs()
        bar = _ulp_half(ref) + U * bound
        assert bool((err <= bar).all()), f"{name}: worst {float((err / bar).max()):.3g}"
        worst[name] = float((err / bar).max()) if err.numel() else 0.0
    err = (dw.double() - dw64).abs()
    bar = U * bw + 1e-300
    assert bool((err <= bar).all()), f"dW: worst {float((err / bar).max()):.3g}"
    worst["dW"] = float((err / bar).max())
    print(f"{kind} {cin}x{cout} [{backend.type}] worst err / bar: {worst}")


def _small_table(backend, K, n=40, seed=3):
    nbr_np = uo.subm_rulebook(_coords(seed=seed, n=n))
    if K == 8:
        nbr_np = nbr_np[[0, 2, 6, 8, 18, 20, 24, 26]]
    elif K == 1:
        nbr_np = nbr_np[[4]]
    return nbr_np


@pytest.mark.parametrize("K", [27, 8, 1])
def test_half_edge_cases(backend, K):
    """K in {27, 8, 1} tables, an offset without a live pair, an output row without an input, a capacity-strided table view (the brick
    pyramid's layout) giving the same bits as the contiguous table; n_out = 0."""
    nbr_np = _small_table(backend, K).copy()
    n = nbr_np.shape[1]
    if K > 1:
        nbr_np[1] = -1  # offset 1 without a live pair
    nbr_np[:, 7] = -1  # an output row without any input
    cap = n + 37
    wide = torch.full((K, cap), -7, dtype=torch.int32)
    wide[:, :n] = torch.from_numpy(nbr_np.astype(np.int32))
    view = wide.to(backend)[:, :n]
    assert view.stride(0) == cap
    nbr = torch.from_numpy(nbr_np.astype(np.int32)).to(backend)
    for cin, cout in ((8, 8), (16, 32)):
        x, w, dy = _int_data(n, cin, cout, n, K, seed=K + cin)
        y0 = ops.sparse_conv_half(x.to(backend), w.half().to(backend), nbr, n).cpu()
        yv = ops.sparse_conv_half(x.to(backend), w.half().to(backend), view, n).cpu()
        dw0 = sg.conv_wgrad(x.to(backend), None, nbr, n, dy.to(backend), K).cpu()
        dwv = sg.conv_wgrad(x.to(backend), None, view, n, dy.to(backend), K).cpu()
        y64, dx64, dw64, *_ = _oracle64(x, w, nbr, n, dy)
        assert _bits_equal(y0, y64.half()) and _bits_equal(yv, y0)
        assert torch.equal(dw0.double(), dw64) and torch.equal(dwv, dw0)
        assert not y0[7].any()
        if K > 1:
            assert not dw0[1].any()
    # n_out = 0: an empty output, zeros for dW
    empty = torch.zeros((K, 0), dtype=torch.int32, device=backend)
    x = torch.ones(5, 16, dtype=torch.float16, device=backend)
    assert ops.sparse_conv_half(x, torch.ones(K, 16, 16, dtype=torch.float16, device=backend), empty, 0).shape == (0, 16)
    dw = sg.conv_wgrad(x, None, empty, 0, torch.zeros((0, 16), dtype=torch.float16, device=backend), K)
    assert dw.shape == (K, 16, 16) and dw.dtype == torch.float32 and not dw.any()


def test_half_wgrad_chunked_rows(backend):
    """More rows than one chunk holds (several partial slabs added in chunk order), pointwise, both forms."""
    n = 256 * 256 + 300 if backend.type == "cuda" else 1500
    for cin, cout in ((3, 8), (32, 16)):
        g = torch.Generator().manual_seed(cin)
        x = torch.randint(-2, 3, (n, cin), generator=g).half()
        dy = torch.randint(-2, 3, (n, cout), generator=g).half()
        dw = sg.conv_wgrad(x.to(backend), None, None, n, dy.to(backend), 1).cpu()
        assert torch.equal(dw[0].double(), x.double().T @ dy.double())


@pytest.mark.parametrize("kind,cin,cout,c0", [("subm", 8, 8, 8), ("down", 8, 16, 8), ("up", 16, 8, 16), ("point", 3, 8, 3),
                                              ("subm", 12, 6, 6), ("point", 6, 5, 6)])
def test_half_vector_wgrad_equals_float32_kernel(backend, kind, cin, cout, c0):
    """The vector form on half inputs gives the bits of the float32 kernel on the same values: the conversions are exact, both run one
    body with the same batches (cin4 + cout4 <= 32: 256 pairs per batch in either type) and the same chunks (n_out <= 16384).  Shapes
    with cin >= 16 and cout >= 16 take the matrix form and are not expected to."""
    nbr, n_in, n_out, _, _ = _table(kind, backend)
    K = 1 if nbr is None else 27
    g = torch.Generator().manual_seed(31 + 7 * cin + cout)
    x = torch.randn(n_in, cin, generator=g).half().to(backend)
    dy = torch.randn(n_out, cout, generator=g).half().to(backend)
    x0, x1 = x[:, :c0].contiguous(), (x[:, c0:].contiguous() if c0 < cin else None)
    dw_h = sg.conv_wgrad(x0, x1, nbr, n_out, dy, K)
    dw_f = sg.conv_wgrad(x0.float(), x1.float() if x1 is not None else None, nbr, n_out, dy.float(), K)
    assert dw_h.dtype == torch.float32 and torch.equal(dw_h, dw_f)


@pytest.mark.parametrize("kind,cin,cout,c0", [("subm", 8, 8, 8), ("subm", 32, 16, 16), ("down", 16, 32, 16), ("up", 32, 16, 32),
                                              ("point", 8, 4, 8)])
def test_half_nonfinite_propagates(backend, kind, cin, cout, c0):
    """A single inf in one row of dy: every dx row that row reaches through a live pair and every dW[k] with such a pair turn
    non-finite; all other rows and offsets keep the bits of the run without it (loss scaling relies on this to skip the step)."""
    nbr, n_in, n_out, nbr_t, flip = _table(kind, backend)
    K = 1 if nbr is None else 27
    g = torch.Generator().manual_seed(11)
    x = (torch.randn(n_in, cin, generator=g) + 3.0).half()  # no zeros
    w = torch.randn(K, cin, cout, generator=g).sign() * (torch.rand(K, cin, cout, generator=g) + 0.5)  # no zeros
    dy = torch.randn(n_out, cout, generator=g).half()
    _, dx_ref, dw_ref = _run(x, w, nbr, n_out, nbr_t, flip, dy, c0, backend)
    table = nbr.cpu().numpy() if nbr is not None else np.arange(n_out)[None]
    r = int(np.argmax((table >= 0).sum(0)))  # the output row with the most live pairs
    for val in (float("inf"), float("-inf")):
        dyi = dy.clone()
        dyi[r, cout // 2] = val
        _, dx, dw = _run(x, w, nbr, n_out, nbr_t, flip, dyi, c0, backend)
        reached = set(int(i) for i in table[:, r] if i >= 0)
        bad_rows = set(np.nonzero(~torch.isfinite(dx).all(1).numpy())[0].tolist())
        assert bad_rows == reached
        for i in reached:
            assert not torch.isfinite(dx[i]).any(), "every entry of a reached row"
        keep = torch.ones(n_in, dtype=torch.bool)
        keep[list(reached)] = False
        assert _bits_equal(dx[keep], dx_ref[keep])
        offs = set(int(k) for k in np.nonzero(table[:, r] >= 0)[0])
        for k in range(K):
            if k in offs:
                assert not torch.isfinite(dw[k]).all()
            else:
                assert torch.equal(dw[k], dw_ref[k])


@pytest.mark.parametrize("c", [1, 3, 8, 17])
def test_move_rows_half(backend, c):
    n = 300
    g = torch.Generator().manual_seed(c)
    x = torch.randn(n, c, generator=g).half().to(backend)
    order = torch.randperm(n, generator=g).to(torch.int32).to(backend)
    gathered = sg.move_rows(x, order)
    assert gathered.dtype == torch.float16 and torch.equal(gathered.cpu(), x.cpu()[order.cpu().long()])
    back = sg.move_rows(gathered, order, scatter=True)
    assert torch.equal(back.cpu(), x.cpu())
    xr = x.clone().requires_grad_(True)
    sg.move_rows(xr, order).backward(gathered)
    assert torch.equal(xr.grad.cpu(), x.cpu())
