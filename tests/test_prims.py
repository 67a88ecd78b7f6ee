"""Device-wide scan / device-length fill / radix sort primitives against numpy.

References: sums on uint64 reduced mod 2**32, `np.argsort(kind="stable")`.  Every output sits inside a larger buffer filled with a
sentinel; whatever the call does not own must still hold it afterwards."""
import numpy as np
import pytest
import torch

from smart_tree_amd import _lib

T = 4096  # the scan's tile: 256 lanes x 16 items
SENT = 0xA5C3F00D
PAD = 8  # sentinel words in front of and behind every array (a multiple of 4: offset 0 stays 16-byte aligned)
ST_ERR_WORKSPACE = -2


def _dev(a: np.ndarray, backend) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).to(backend)


def _host(t: torch.Tensor) -> np.ndarray:
    return t.cpu().numpy().view(np.uint32)


class _Framed:
    """`n` words at element offset `off` inside a sentinel-filled buffer whose base is 16-byte aligned."""

    def __init__(self, backend, n, off, data=None, extra=0):
        self.n, self.lo = n + extra, PAD + off
        self.init = np.full(PAD + off + n + extra + PAD, SENT, np.uint32)
        if data is not None:
            self.init[self.lo:self.lo + n] = data
        self.buf = _dev(self.init, backend)
        assert self.buf.data_ptr() % 16 == 0
        self.view = self.buf[self.lo:self.lo + n + extra]

    def ptr(self, at=0):
        return _lib.ptr(self.buf[self.lo + at:])

    def check(self, expect: np.ndarray, what=""):
        """The first len(expect) words equal `expect`, every other word of the buffer is what it was."""
        want = self.init.copy()
        want[self.lo:self.lo + len(expect)] = expect
        np.testing.assert_array_equal(_host(self.buf), want, err_msg=what)


def _values(n, seed):
    return np.random.RandomState(seed).randint(0, 2 ** 32, n, dtype=np.int64).astype(np.uint32)


def _exclusive(a: np.ndarray):
    """(exclusive prefix sums, total) of a uint32 array, both mod 2**32."""
    c = np.cumsum(a.astype(np.uint64), dtype=np.uint64)  # < 2**32 * 2**23: no uint64 wrap at these sizes
    return ((c - a) & np.uint64(0xFFFFFFFF)).astype(np.uint32), int(c[-1] & np.uint64(0xFFFFFFFF)) if len(a) else 0


def _check_scan(backend, n):
    L = _lib.lib()
    a = np.random.RandomState(n).randint(0, 7, n).astype(np.int32)
    t = torch.from_numpy(a).to(backend)
    out = torch.zeros(max(n, 1), dtype=torch.int32, device=backend)
    total = torch.zeros(1, dtype=torch.int32, device=backend)
    ws = _lib.workspace(L.st_scan_workspace_bytes(n), backend)
    _lib.check(L.st_scan_u32(_lib.ptr(t), _lib.ptr(out), n, _lib.ptr(total), _lib.ptr(ws), ws.numel(), _lib.stream(backend)))
    ref = np.cumsum(a) - a
    np.testing.assert_array_equal(out.cpu().numpy()[:n], ref)
    assert int(total.cpu()[0]) == int(a.sum())


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 2047, 2048, 2049, 4095, 4096, 4097, 70001])
def test_exclusive_scan(backend, n):
    _check_scan(backend, n)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [4_300_003,    # > 1024 tiles: the recursive tile-offset scan
                               51_000_001])  # the cell table of a batched kNN grid
def test_exclusive_scan_large(n):
    assert torch.cuda.is_available()
    _check_scan(torch.device("cuda:0"), n)


# ------------------------------------------------------------------------------------------------ scan ---
def _run_scan(backend, a, in_off, out_off, inplace, total_mode, m=None, what=""):
    """One scan of `a` (m: the device length, None = the plain entry point) and every check on what it wrote."""
    L = _lib.lib()
    n = len(a)
    at_end = total_mode == "end"  # total = out + n: the graph stage's layout (counts, then their sum)
    src = _Framed(backend, n, in_off, a, extra=1 if (inplace and at_end) else 0)
    dst = src if inplace else _Framed(backend, n, out_off, extra=1 if at_end else 0)
    tot = _Framed(backend, 1, 0)
    total_ptr = {"none": None, "own": tot.ptr(), "end": dst.ptr(n)}[total_mode]
    ws = _lib.workspace(L.st_scan_workspace_bytes(n), backend)
    if m is None:
        rc = L.st_scan_u32(src.ptr(), dst.ptr(), n, total_ptr, _lib.ptr(ws), ws.numel(), _lib.stream(backend))
    else:
        n_dev = torch.tensor([m], dtype=torch.int64, device=backend)
        rc = L.st_scan_u32_dev(src.ptr(), dst.ptr(), n, total_ptr, _lib.ptr(ws), ws.numel(), _lib.ptr(n_dev), _lib.stream(backend))
    _lib.check(rc)
    live = n if m is None else min(n, m)
    ref, total = _exclusive(a[:live])
    want = np.concatenate([ref, a[live:] if inplace else np.full(n - live, SENT, np.uint32)])
    if at_end:
        want = np.concatenate([want, np.array([total], np.uint32)])
    dst.check(want, what)
    if not inplace:
        src.check(a, what + " (input)")
    tot.check(np.array([total if total_mode == "own" else SENT], np.uint32), what + " (total)")


SCAN_OFFSETS = [(0, 0), (1, 0), (0, 1), (3, 2), (4, 4)]  # (in, out): every mix of the 16-byte path and the scalar one


@pytest.mark.parametrize("offs", SCAN_OFFSETS, ids=lambda o: f"in{o[0]}out{o[1]}")
@pytest.mark.parametrize("n", [1, 15, 16, 17, T - 1, T, T + 1, 2 * T + 3])
def test_scan_wraps_at_every_alignment(backend, n, offs):
    """Full-range values (the sums wrap), each pointer with its own alignment, out of place and in place, with every way of asking
    for the total."""
    a = _values(n, 1000 + n)
    for inplace in (False, True):
        for total_mode in ("own", "none", "end"):
            _run_scan(backend, a, offs[0], offs[1], inplace, total_mode, what=f"inplace={inplace} total={total_mode}")


@pytest.mark.parametrize("n", [1, T + 1])
def test_scan_short_workspace_is_an_error(backend, n):
    L = _lib.lib()
    need = L.st_scan_workspace_bytes(n)
    ws = _lib.workspace(need, backend)
    src, dst, tot = _Framed(backend, n, 0, _values(n, 5)), _Framed(backend, n, 0), _Framed(backend, 1, 0)
    rc = L.st_scan_u32(src.ptr(), dst.ptr(), n, tot.ptr(), _lib.ptr(ws), need - 256, _lib.stream(backend))
    assert rc == ST_ERR_WORKSPACE and L.st_last_error()
    dst.check(np.zeros(0, np.uint32))
    tot.check(np.zeros(0, np.uint32))


SCAN_DEV_CASES = [(1, 0), (1, 1), (1, 5), (17, 16), (T, T - 1), (T, T), (T + 1, T), (T + 1, T + 1)] + \
    [(3 * T + 5, m) for m in (0, 1, T, 2 * T + 1, 3 * T + 4, 10 * T)]


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n,m", SCAN_DEV_CASES)
def test_scan_device_length(backend, n, m, off):
    """The launch is sized for n, the length in use lives on the device: the live prefix is scanned, nothing past it is written,
    the total is the live prefix's (0 for an empty one)."""
    a = _values(n, 2000 + n + m)
    for inplace in (False, True):
        for total_mode in ("own", "end"):
            _run_scan(backend, a, off, off, inplace, total_mode, m=m, what=f"inplace={inplace} total={total_mode}")


@pytest.mark.parametrize("n,m", [(1024 * T + 1, 1024 * T + 1), (1024 * T + 1, 1024 * T), (1025 * T + 3, 7 * T + 9), (1025 * T + 3, 0)])
def test_scan_device_length_recursive_level(backend, n, m):
    """More than 1024 tiles: the tile totals are scanned by a second level, which sees zeros for the tiles past the device length."""
    _run_scan(backend, _values(n, 7), 0, 0, True, "own", m=m)


# ------------------------------------------------------------------------------------------------ fill ---
def _run_fill(backend, n, m, off, value=0x9E3779B9):
    L = _lib.lib()
    dst = _Framed(backend, n, off)
    n_dev = torch.tensor([m], dtype=torch.int64, device=backend)
    _lib.check(L.st_fill_u32_len(dst.ptr(), n, _lib.ptr(n_dev), value, _lib.stream(backend)))
    dst.check(np.full(min(n, m), value, np.uint32))


@pytest.mark.parametrize("off", [0, 1, 3])
@pytest.mark.parametrize("n,m", [(1, 0), (1, 1), (3, 2), (4, 4), (5, 4), (1029, 1027), (1029, 5000), (70001, 69999), (70001, 0)])
def test_fill_device_length(backend, n, m, off):
    _run_fill(backend, n, m, off)


@pytest.mark.gpu
def test_fill_device_length_second_grid_stride_trip():
    """16384 workgroups x 256 lanes x 4 words is one trip of the grid-stride loop: five words more start the second."""
    n = 16384 * 256 * 4 + 5
    _run_fill(torch.device("cuda:0"), n, n - 2, 0)


# ------------------------------------------------------------------------------------------------ sort ---
SORT_KINDS = ["random", "equal", "two", "descending", "high"]


def _sort_keys(kind, n, bits, rng):
    """uint32 keys.  All kinds but "high" stay below 2**bits."""
    top = 2 ** bits
    if kind == "random":
        return rng.randint(0, top, n, dtype=np.int64).astype(np.uint32)
    if kind == "equal":  # 64 peers in every wavefront
        return np.full(n, rng.randint(0, top, dtype=np.int64), np.uint32)
    if kind == "two":
        pair = np.array([top - 1, rng.randint(0, top - 1, dtype=np.int64)], np.int64)
        return pair[rng.randint(0, 2, n)].astype(np.uint32)
    if kind == "descending":  # strictly where the field has room for n values (2**bits >= n), else non-increasing
        return ((np.arange(n - 1, -1, -1, dtype=np.int64) * top) // n).astype(np.uint32)
    # "high": random bits above the sorted field, four distinct values (two when bits == 1) inside it
    low = rng.choice(top, min(4, top), replace=False) if top <= 1 << 20 else rng.randint(0, top, 4, dtype=np.int64)
    k = np.asarray(low, np.int64)[rng.randint(0, len(low), n)]
    return (k | (rng.randint(0, 2 ** 32, n, dtype=np.int64) >> bits << bits)).astype(np.uint32)


def _run_sort(backend, k, v, bits, what=""):
    L = _lib.lib()
    n = len(k)
    keys, vals = _Framed(backend, n, 0, k), _Framed(backend, n, 0, v)
    ws = _lib.workspace(L.st_sort_workspace_bytes(n), backend)
    _lib.check(L.st_sort_pairs_u32(keys.ptr(), vals.ptr(), n, bits, _lib.ptr(ws), ws.numel(), _lib.stream(backend)))
    if n <= 1 or bits <= 0:
        order = np.arange(n)
    else:
        field = k & np.uint32(2 ** bits - 1)
        order = np.argsort(field.astype(np.uint8) if bits <= 8 else field, kind="stable")
    keys.check(k[order], what + " (keys)")  # whole keys: the bits above the field travel with their pair
    vals.check(v[order], what + " (values)")


@pytest.mark.parametrize("bits", [1, 7, 8, 9, 16, 17, 24, 25, 30, 32])  # 1 .. 4 passes: with and without the copy back
@pytest.mark.parametrize("n", [2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 5000])
def test_radix_sort_matrix(backend, n, bits):
    """Stable on the key bits [0, bits) and on nothing else; values are arbitrary words."""
    rng = np.random.RandomState(n * 64 + bits)
    for kind in SORT_KINDS:
        _run_sort(backend, _sort_keys(kind, n, bits, rng), _values(n, n + bits), bits, what=kind)


@pytest.mark.parametrize("n,bits", [(0, 8), (1, 8), (100, 0), (100, -3)])
def test_radix_sort_nothing_to_do(backend, n, bits):
    _run_sort(backend, _values(n, 3), _values(n, 4), bits)


def test_radix_sort_short_workspace_is_an_error(backend):
    L = _lib.lib()
    n = 1025
    need = L.st_sort_workspace_bytes(n)
    ws = _lib.workspace(need, backend)
    k, v = _values(n, 8), _values(n, 9)
    keys, vals = _Framed(backend, n, 0, k), _Framed(backend, n, 0, v)
    rc = L.st_sort_pairs_u32(keys.ptr(), vals.ptr(), n, 16, _lib.ptr(ws), need - 256, _lib.stream(backend))
    assert rc == ST_ERR_WORKSPACE and L.st_last_error()
    keys.check(k)
    vals.check(v)


@pytest.mark.gpu
def test_radix_sort_large_histogram_takes_the_recursive_scan():
    """16385 tiles x 256 digits = more than 1024 scan tiles of histogram.  16-bit keys sorted on their low 8 bits."""
    n = 16384 * 1024 + 1
    rng = np.random.RandomState(11)
    _run_sort(torch.device("cuda:0"), rng.randint(0, 2 ** 16, n, dtype=np.int64).astype(np.uint32), _values(n, 12), 8)


@pytest.mark.parametrize("n,bits", [(2, 8), (1000, 5), (1025, 13), (40001, 32)])
def test_radix_sort_is_stable(backend, n, bits):
    L = _lib.lib()
    rng = np.random.RandomState(n)
    k = rng.randint(0, 2 ** min(bits, 31), n).astype(np.int64)
    if bits == 32:
        k = rng.randint(0, 2 ** 32, n, dtype=np.int64)
    keys = torch.from_numpy(k.astype(np.uint32).view(np.int32)).to(backend)
    vals = torch.arange(n, dtype=torch.int32, device=backend)
    ws = _lib.workspace(L.st_sort_workspace_bytes(n), backend)
    _lib.check(L.st_sort_pairs_u32(_lib.ptr(keys), _lib.ptr(vals), n, bits, _lib.ptr(ws), ws.numel(), _lib.stream(backend)))
    order = np.argsort(k, kind="stable")
    np.testing.assert_array_equal(keys.cpu().numpy().view(np.uint32), k[order].astype(np.uint32))
    np.testing.assert_array_equal(vals.cpu().numpy(), order.astype(np.int32))
