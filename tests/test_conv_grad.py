"""Sparse-convolution backward (smart_tree_amd/model/sparse_grad.py, csrc/sparse_conv_grad.hip): weight gradient (st_sparse_conv_wgrad)
and data gradient (the forward kernel over the transposed table) against float64 autograd through oracle.unet_oracle.sparse_conv, on
the CPU sanitizer build and on the GPU."""
import numpy as np
import pytest
import torch

from oracle import unet_oracle as uo
from smart_tree_amd import _lib
from smart_tree_amd.model import sparse_grad as sg
from smart_tree_amd.model.sparse_ops import RulebookPyramid

REL = 1e-5  # |g - g64| <= REL * sum over the contributing pairs of |a| |b|, entrywise


def _coords(seed=0, n=160, side=9):
    """Two blocks of random voxels plus isolated odd-coordinate voxels (each reaches all 8 of its coarse outputs)."""
    rng = np.random.RandomState(seed)
    pts = {(int(rng.randint(2)), *map(int, rng.randint(0, side, 3))) for _ in range(n)}
    pts |= {(0, 13, 13, 13), (1, 15, 1, 15)}
    return np.array(sorted(pts), np.int32)


_PYR = {}


def _pyramid(device):
    """One level of tables from the oracle's builders: subm, down (fine -> coarse) and up (coarse -> fine)."""
    if device.type not in _PYR:
        fine = _coords()
        coarse = uo.strided_out_coords(fine)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(device)
        pyr = RulebookPyramid(coords=[t(fine), t(coarse)], subm=[t(uo.subm_rulebook(fine))],
                              down=[t(uo.down_rulebook(coarse, fine))], up=[t(uo.up_rulebook(fine, coarse))])
        _PYR[device.type] = (pyr, len(fine), len(coarse))
    return _PYR[device.type]


def _table(kind, device):
    """(nbr, n_in, n_out, nbr_t, flip)"""
    pyr, nf, nc = _pyramid(device)
    if kind == "subm":
        return pyr.subm[0], nf, nf, *sg.transposed_table("subm", pyr, 0)
    if kind == "down":
        return pyr.down[0], nf, nc, *sg.transposed_table("down", pyr, 0)
    if kind == "up":
        return pyr.up[0], nc, nf, *sg.transposed_table("up", pyr, 0)
    return None, nf, nf, *sg.transposed_table("point", pyr, 0)


def _oracle(x, w, nbr, n_out, dy):
    """float64 autograd through the oracle's convolution: (dx, dW [K, Cin, Cout]) and the entrywise bounds sum |.| |dy|."""
    K, cin, cout = w.shape
    table = nbr.cpu().numpy().astype(np.int64) if nbr is not None else np.arange(x.shape[0], dtype=np.int64)[None]

    def run(xv, wv, dyv):
        xv = xv.detach().double().cpu().requires_grad_(True)
        ws = wv.detach().double().cpu().permute(2, 0, 1).contiguous().requires_grad_(True)  # spconv order [Cout, K, Cin]
        uo.sparse_conv(xv, table, ws, n_out).backward(dyv.detach().double().cpu())
        return xv.grad, ws.grad.permute(1, 2, 0)

    dx, dw = run(x, w, dy)
    bx, bw = run(x.abs(), w.abs(), dy.abs())
    return dx, dw, bx, bw


def _check(got, ref, bound, what):
    err = (got.double().cpu() - ref).abs()
    worst = float((err / (bound + 1e-300)).max()) if err.numel() else 0.0
    assert bool((err <= REL * bound + 1e-30).all()), f"{what}: worst |err| / bound = {worst:.3g} (bar {REL})"
    return worst


# (kind, Cin, Cout, c0): every convolution the shipped network, the [8, 16, 32] / 6-10-18-34 configurations and their heads use
# (the data gradient runs the transposed shape); c0 < Cin is the Tail's cat(skip, decoded)
SHAPES = [("point", 3, 8, 3), ("point", 3, 6, 3),
          ("subm", 8, 8, 8), ("subm", 16, 16, 16), ("subm", 32, 32, 32), ("subm", 64, 64, 64), ("subm", 6, 6, 6), ("subm", 10, 10, 10),
          ("down", 8, 16, 8), ("down", 16, 32, 16), ("down", 32, 64, 32), ("down", 6, 10, 6), ("down", 18, 34, 18),
          ("up", 16, 8, 16), ("up", 32, 16, 32), ("up", 64, 32, 64), ("up", 10, 6, 10), ("up", 34, 18, 34),
          ("subm", 16, 8, 8), ("subm", 32, 16, 16), ("subm", 64, 32, 32), ("subm", 12, 6, 6), ("subm", 20, 10, 10), ("subm", 36, 18, 18),
          ("point", 16, 8, 8), ("point", 64, 32, 32), ("point", 12, 6, 6), ("point", 20, 10, 10),
          ("point", 8, 8, 8), ("point", 8, 4, 8), ("point", 4, 1, 4), ("point", 4, 3, 4), ("point", 4, 2, 4),
          ("point", 6, 5, 6), ("point", 5, 3, 5), ("point", 3, 1, 3), ("point", 3, 3, 3)]


def _inputs(kind, cin, cout, c0, device, seed=0):
    nbr, n_in, n_out, nbr_t, flip = _table(kind, device)
    K = 1 if nbr is None else 27
    g = torch.Generator().manual_seed(seed + 1000 * cin + cout)
    x = torch.randn(n_in, cin, generator=g)
    w = torch.randn(K, cin, cout, generator=g) / np.sqrt(K * cin)
    dy = torch.randn(n_out, cout, generator=g)
    return nbr, n_in, n_out, nbr_t, flip, K, x, w, dy


def _hip_grads(x, w, nbr, n_out, nbr_t, flip, dy, c0, device):
    x0 = x[:, :c0].contiguous().to(device).requires_grad_(True)
    x1 = x[:, c0:].contiguous().to(device).requires_grad_(True) if c0 < x.shape[1] else None
    wd = w.to(device).requires_grad_(True)
    y = sg.sparse_conv(x0, wd, nbr, n_out, nbr_t, flip, x1=x1)
    y.backward(dy.to(device))
    dx = x0.grad if x1 is None else torch.cat([x0.grad, x1.grad], 1)
    return y.detach(), dx.detach(), wd.grad.detach()


@pytest.mark.parametrize("kind,cin,cout,c0", SHAPES, ids=[f"{k}-{a}x{b}-c0{c}" for k, a, b, c in SHAPES])
def test_conv_grad_matches_float64_autograd(backend, kind, cin, cout, c0):
    nbr, n_in, n_out, nbr_t, flip, K, x, w, dy = _inputs(kind, cin, cout, c0, backend)
    y, dx, dw = _hip_grads(x, w, nbr, n_out, nbr_t, flip, dy, c0, backend)
    rdx, rdw, bx, bw = _oracle(x, w, nbr, n_out, dy)
    _check(dw, rdw, bw, "dW")
    _check(dx, rdx, bx, "dx")
    if backend.type == "cuda":  # deterministic: a second call gives the same bits
        _, dx2, dw2 = _hip_grads(x, w, nbr, n_out, nbr_t, flip, dy, c0, backend)
        assert torch.equal(dw, dw2) and torch.equal(dx, dx2)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,cin,cout,c0", SHAPES[:20:3], ids=[f"{k}-{a}x{b}-c0{c}" for k, a, b, c in SHAPES[:20:3]])
def test_conv_grad_gpu_equals_sanitizer_build(emu_lib, monkeypatch, kind, cin, cout, c0):
    """The weight-gradient kernel and the forward kernels the data gradient runs on evaluate the same fmaf chains on both builds."""
    dev = torch.device("cuda:0")
    nbr, n_in, n_out, nbr_t, flip, K, x, w, dy = _inputs(kind, cin, cout, c0, dev)
    _, dx_g, dw_g = _hip_grads(x, w, nbr, n_out, nbr_t, flip, dy, c0, dev)
    monkeypatch.setattr(_lib, "_LIB", emu_lib)
    monkeypatch.setattr(_lib, "_ALLOW_HOST_POINTERS", True)
    cpu = torch.device("cpu")
    nbr, n_in, n_out, nbr_t, flip, K, x, w, dy = _inputs(kind, cin, cout, c0, cpu)
    _, dx_e, dw_e = _hip_grads(x, w, nbr, n_out, nbr_t, flip, dy, c0, cpu)
    assert torch.equal(dw_g.cpu(), dw_e), "wgrad: GPU and sanitizer build differ"
    assert torch.equal(dx_g.cpu(), dx_e), "dgrad: GPU and sanitizer build differ"


def test_wgrad_edge_cases(backend):
    """n_out = 0 writes zeros; an offset without a live pair gets an exact zero; a capacity-strided table view (the brick
    pyramid's layout) gives the same bits as the contiguous table."""
    g = torch.Generator().manual_seed(5)
    x = torch.randn(40, 16, generator=g).to(backend)
    w = torch.randn(27, 16, 8, generator=g).to(backend)
    dw = sg.conv_wgrad(x, None, torch.zeros((27, 0), dtype=torch.int32, device=backend), 0, torch.zeros((0, 8), device=backend), 27)
    assert dw.shape == (27, 16, 8) and not dw.any()
    nbr_np = uo.subm_rulebook(_coords(seed=3, n=40))
    n = nbr_np.shape[1]
    nbr_np[5] = -1  # offset 5 without a live pair
    nbr_np[:, 7] = -1  # an output row without any input
    cap = n + 37
    wide = torch.full((27, cap), -7, dtype=torch.int32)
    wide[:, :n] = torch.from_numpy(nbr_np.astype(np.int32))
    view = wide.to(backend)[:, :n]
    assert view.stride(0) == cap
    nbr = torch.from_numpy(nbr_np.astype(np.int32)).to(backend)
    x = torch.randn(n, 16, generator=g).to(backend)
    dy = torch.randn(n, 8, generator=g).to(backend)
    dw_c = sg.conv_wgrad(x, None, nbr, n, dy, 27)
    dw_v = sg.conv_wgrad(x, None, view, n, dy, 27)
    assert torch.equal(dw_c, dw_v)
    assert not dw_c[5].any()
    _, rdw, _, bw = _oracle(x, torch.zeros(27, 16, 8), nbr, n, dy)
    _check(dw_c, rdw, bw, "dW")
    # the data gradient over the strided view: the forward kernel honours the stride
    wd = w.clone().requires_grad_(True)
    xd = x.clone().requires_grad_(True)
    sg.sparse_conv(xd, wd, view, n, view, True).backward(dy)
    xc = x.clone().requires_grad_(True)
    sg.sparse_conv(xc, w.clone().requires_grad_(True), nbr, n, nbr, True).backward(dy)
    assert torch.equal(xd.grad, xc.grad) and torch.equal(wd.grad, dw_c)


def test_wgrad_chunked_rows(backend):
    """More rows than one chunk holds (several partial slabs added in chunk order) and a pointwise table."""
    g = torch.Generator().manual_seed(9)
    n = 256 * 64 + 300 if backend.type == "cuda" else 1500
    x = torch.randn(n, 4, generator=g).to(backend)
    dy = torch.randn(n, 3, generator=g).to(backend)
    dw = sg.conv_wgrad(x, None, None, n, dy, 1)
    ref = (x.double().T @ dy.double()).cpu()
    bound = (x.abs().double().T @ dy.abs().double()).cpu()
    _check(dw[0], ref, bound, "dW")


def test_wgrad_workspace_chunk_policy(backend):
    """The workspace queries are the outside view of the per-type row chunking (up to 64 chunks per offset for float32, 256 for half,
    256-row steps): K = 1, cin = 4, cout = 3 gives nchunks * 48 + 256 bytes."""
    L = _lib.lib()
    f32, f16 = L.st_sparse_conv_wgrad_workspace_bytes, L.st_sparse_conv_wgrad_h_workspace_bytes
    for n_out, want32, want16 in ((0, 304, 304), (256 * 64, 3328, 3328), (256 * 64 + 1, 33 * 48 + 256, 65 * 48 + 256)):
        assert (f32(1, 4, 3, n_out), f16(1, 4, 3, n_out)) == (want32, want16), n_out
    assert (33 * 48 + 256, 65 * 48 + 256) == (1840, 3376)
    for bad in ((0, 4, 3, 10), (1, 0, 3, 10), (1, 4, 0, 10), (1, 4, 3, -1)):
        assert f32(*bad) == -1 and f16(*bad) == -1, bad


def test_conv_wgrad_refuses_mixed_dtypes(backend):
    x, dy = torch.zeros(4, 8, device=backend), torch.zeros(4, 8, device=backend)
    for a, b, c in ((x.half(), None, dy), (x, None, dy.half()), (x, x.half(), dy), (x.double(), None, dy.double())):
        with pytest.raises(ValueError):
            sg.conv_wgrad(a, b, None, 4, c, 1)
