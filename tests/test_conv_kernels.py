"""Every sparse-convolution kernel instance and tile variant of csrc/sparse_conv.hip against a float64 contraction.

Each case calls the C entry point named in its table row directly (not sparse_ops.sparse_conv, whose routing could send it to
another kernel).  Two regimes:
  exact  small-integer features and weights, power-of-two scale, shift in quarters, integer residual: every product and partial
         sum is exact in float32 (|sum| <= 27 * 64 * 16 < 2^24), in the split-bf16 pieces (mid = lo = 0) and in every matrix
         instruction, so every kernel, tile shape and summation order must return the float64 reference bit for bit (or its
         round-to-nearest-even half for half outputs).  A dropped, duplicated or mis-routed product fails outright.
  real   random normal features whose rows differ in scale by up to e^12: |got - ref| <= C * 2^-24 * A per element with
         A = |scale| * sum |x||w| + |shift| + |residual| (float64); half outputs may add half an ulp of half precision, and at least
         99 % of them must be the correctly rounded reference.
The reference is torch float64 on the CPU (index_select + matmul per offset)."""
from __future__ import annotations

import re
import zlib
from dataclasses import dataclass
from pathlib import Path

import numpy as np
import pytest
import torch

from smart_tree_amd import _lib
from smart_tree_amd.model import sparse_ops as ops

SRC = Path(__file__).resolve().parents[1] / "smart_tree_amd" / "csrc" / "sparse_conv.hip"

# Real-valued regime: worst |got - ref| / (2^-24 A) measured on the MI355X over every case below, ten seeds each (the test's own
# seed among them): 18.2 (float32 vector kernel, 64 -> 32), 16.7 (float32 matrix-core kernel), 14.2 (generic kernel), 12.0
# (split-bf16), 1.4 (half precision).  The CPU emulator adds the 32 products of a bf16 matrix instruction one rounding at a time
# and reaches 29 on split-bf16 (20 on the test's seeds).  One product of 27 * 64 is ~1/1728 of A: a missing product exceeds
# the bound ~300-fold.
C_REAL = 32.0
# Half outputs of the real-valued regime: share that is exactly round_half(float64 reference); measured on the MI355X: at least
# 99.76 % (float32 -> half converting kernel), 99.90 % (half matrix-core kernels).
HALF_EXACT_SHARE = 0.99
GUARD = 16  # rows after n_out that no kernel may write


@dataclass(frozen=True)
class Case:
    entry: str  # st_sparse_conv_{entry}_fwd ("fwd" = st_sparse_conv_fwd)
    family: str  # kernel family the arguments select
    cin: int
    cout: int
    variant: int = 0  # mfma: row tiles | LDS << 4; b3: row tiles; 0 = the library picks by size
    c0: int = 0  # concat split the instance test uses (0: a legal aligned split of the entry)

    @property
    def in_half(self):
        return self.family in ("f16x", "f16x_c16", "cast_h2f")

    @property
    def out_half(self):
        return self.family in ("f16x", "f16x_c16", "cast_f2h")

    def __str__(self):
        return f"{self.family}-{self.cin}x{self.cout}" + (f"-v{self.variant}" if self.variant else "") + (f"-c0_{self.c0}" if self.c0 else "")


VEC_SHAPES = [(3, 8), (8, 8), (8, 16), (16, 8), (16, 16), (16, 32), (32, 16), (32, 32), (32, 64), (64, 32), (64, 64)]
MFMA_SHAPES = [(16, 16), (16, 32), (32, 16), (32, 32), (32, 64), (64, 32), (64, 64)]
MFMA_VARIANTS = [1, 2, 4, 17, 18]
B3_SHAPES = [(32, 16), (32, 32), (32, 64), (64, 32), (64, 64)]
C16_SHAPES = [(16, 16), (16, 32)]
CAST_SHAPES = [(8, 16), (16, 8), (16, 32), (32, 16)]

CASES = (
    [Case("fwd", "vec", ci, co) for ci, co in VEC_SHAPES]
    # the generic kernel: shapes without an instance, and instantiated shapes with a split that is no multiple of 4
    + [Case("fwd", "any", 5, 7, c0=3), Case("fwd", "any", 24, 40, c0=10), Case("fwd", "any", 16, 16, c0=6), Case("fwd", "any", 3, 8, c0=2)]
    + [Case("mfma", "mfma", ci, co, v) for ci, co in MFMA_SHAPES for v in MFMA_VARIANTS]
    + [Case("b3", "b3", ci, co, rt) for ci, co in B3_SHAPES for rt in (1, 2)]
    + [Case("b3", "b3_c16", ci, co, rt) for ci, co in C16_SHAPES for rt in (1, 2)]
    + [Case("f16", "f16x", ci, co) for ci, co in B3_SHAPES]  # one row tile below 56 000 rows (two: test_production_thresholds)
    + [Case("f16", "f16x_c16", ci, co) for ci, co in C16_SHAPES]
    + [Case("f16", fam, ci, co) for ci, co in CAST_SHAPES for fam in ("cast_f2h", "cast_h2f")]
)

# One case per family and tile variant (the smallest shape): the edge tests run each of these.
FAMILIES = {
    "vec": Case("fwd", "vec", 16, 16), "vec_wide": Case("fwd", "vec", 32, 16), "vec_c3": Case("fwd", "vec", 3, 8),
    "any": Case("fwd", "any", 5, 7),
    **{f"mfma_v{v}": Case("mfma", "mfma", 16, 16, v) for v in MFMA_VARIANTS},
    "b3_rt1": Case("b3", "b3", 32, 16, 1), "b3_rt2": Case("b3", "b3", 32, 16, 2),
    "b3_c16_rt1": Case("b3", "b3_c16", 16, 16, 1), "b3_c16_rt2": Case("b3", "b3_c16", 16, 16, 2),
    "f16x": Case("f16", "f16x", 32, 16), "f16x_c16": Case("f16", "f16x_c16", 16, 16),
    "cast_f2h": Case("f16", "cast_f2h", 8, 16), "cast_h2f": Case("f16", "cast_h2f", 16, 8),
}
FAM = list(FAMILIES)


def legal_splits(case):
    if case.family in ("b3_c16", "f16x_c16", "cast_f2h", "cast_h2f"):
        return [case.cin]
    if case.entry == "fwd":
        return list(range(1, case.cin + 1))
    step = {"mfma": 16, "b3": 8, "f16": 16}[case.entry]
    return list(range(step, case.cin + 1, step))


def default_split(case):
    if case.c0:
        return case.c0
    cands = [s for s in legal_splits(case) if s < case.cin and (case.entry != "fwd" or s % 4 == 0)]
    return cands[(2 * len(cands)) // 3] if cands else case.cin


# ---------------------------------------------------------------------------------------------------------------- problems ---
def live_offsets(c):
    """The offsets an inverse k3-s2-p1 conv can pair for a row of coordinate parity class c (csrc/sparse_conv.hip conv_live_offsets)."""
    ax = [(0, 2) if (c >> b) & 1 else (1,) for b in (2, 1, 0)]  # z, y, x
    return [kz * 9 + ky * 3 + kx for kz in ax[0] for ky in ax[1] for kx in ax[2]]


@dataclass
class Problem:
    x: np.ndarray  # [n_in, cin] float32 (half-representable where the kernel reads half)
    w: np.ndarray  # [K, cin, cout] float32
    nbr: np.ndarray  # [K, cap] int32 (columns >= n_out: rows of another level) or None (pointwise)
    n_out: int
    c0: int
    scale: np.ndarray = None
    shift: np.ndarray = None
    res: np.ndarray = None
    relu: bool = False
    order: np.ndarray = None  # [n_out] int32 row_order entries
    stride: int = -1  # nbr_stride argument (-1: the table's column count)


def make_problem(case, seed, n_out=129, n_in=None, K=27, density=0.5, exact=True, epilogue="full", order="perm", cap_extra=5,
                 c0=None, pointwise=False, kind=None):
    rng = np.random.RandomState(seed)
    cin, cout = case.cin, case.cout
    n_in = (n_out if pointwise else max(n_out * 4 // 5, 1)) if n_in is None else n_in
    if exact:
        x = rng.randint(-4, 5, size=(n_in, cin)).astype(np.float32)
        w = rng.randint(-4, 5, size=(K, cin, cout)).astype(np.float32)
    else:
        rows = 3.0 if case.in_half else 6.0  # half inputs: keep the rows away from subnormal and overflowing halves
        x = (rng.randn(n_in, cin) * np.exp(rng.uniform(-rows, rows, size=(n_in, 1)))).astype(np.float32)
        w = (rng.randn(K, cin, cout) * 0.05).astype(np.float32)
        if case.in_half:
            x = x.astype(np.float16).astype(np.float32)
        if case.family in ("f16x", "f16x_c16"):
            w = w.astype(np.float16).astype(np.float32)
    nbr = None
    tags = None
    if not pointwise:
        cap = n_out + cap_extra
        nbr = rng.randint(0, n_in, size=(K, cap)).astype(np.int32)
        nbr[rng.rand(K, cap) >= density] = -1
        if order in ("tagged_grouped", "tagged_mixed"):
            assert K == 27
            tags = rng.randint(-1, 8, size=n_out)  # -1: untagged row (all 27 offsets may be live)
            for c in range(8):
                dead = np.setdiff1d(np.arange(27), live_offsets(c))
                nbr[np.ix_(dead, np.nonzero(tags == c)[0])] = -1
        live = lambda r: list(range(K)) if tags is None or tags[r] < 0 else live_offsets(tags[r])
        if density > 0:  # table entries at the first and the last input row
            nbr[live(0)[0], 0] = 0
            nbr[live(n_out - 1)[-1], n_out - 1] = n_in - 1
        if kind == "empty_offsets":  # whole offsets without an entry for any row: the wave-uniform skip
            nbr[[k for k in range(K) if k % 3 != 1]] = -1
        elif kind == "empty_rows":  # rows without any neighbour (epilogue only), among them whole wavefronts and blocks
            nbr[:, 16:min(16 + 300, n_out - 1)] = -1
            nbr[:, 5] = -1
    p = Problem(x, w, nbr, n_out, default_split(case) if c0 is None else c0)
    if epilogue in ("affine", "full"):
        if exact:
            p.scale = rng.choice([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], size=cout).astype(np.float32)
            p.shift = (rng.randint(-32, 33, size=cout) / 4.0).astype(np.float32)
        else:
            p.scale = (rng.uniform(0.5, 1.5, cout) * rng.choice([-1, 1], cout)).astype(np.float32)
            p.shift = rng.randn(cout).astype(np.float32)
    if epilogue == "full":
        p.relu = True
        if case.family not in ("cast_f2h", "cast_h2f"):  # the converting kernels take no residual
            p.res = rng.randint(-8, 9, size=(n_out, cout)).astype(np.float32) if exact else rng.randn(n_out, cout).astype(np.float32)
            if case.out_half:
                p.res = p.res.astype(np.float16).astype(np.float32)
    if order == "perm":
        p.order = rng.permutation(n_out).astype(np.int32)
    elif tags is not None:
        rows = np.argsort(tags, kind="stable") if order == "tagged_grouped" else rng.permutation(n_out)
        ent = rows.astype(np.int64) | np.where(tags[rows] >= 0, (8 + tags[rows]).astype(np.int64) << 28, 0)
        p.order = ent.astype(np.uint32).view(np.int32)
    return p


def reference(p, absolute=False):
    """float64: act(scale * sum_k W_k . x[nbr[k]] + shift + residual); absolute=True: the same over |.| without ReLU (the A of the
    real-valued bound)."""
    f = (lambda a: torch.from_numpy(np.abs(a) if absolute else a).double())
    x, w = f(p.x), f(p.w)
    if p.nbr is None:
        acc = x[: p.n_out] @ w[0]
    else:
        acc = torch.zeros((p.n_out, w.shape[2]), dtype=torch.float64)
        for k in range(w.shape[0]):
            idx = torch.from_numpy(p.nbr[k, : p.n_out]).long()
            hit = idx >= 0
            acc[hit] += x.index_select(0, idx[hit]) @ w[k]
    if p.scale is not None:
        acc = acc * f(p.scale) + f(p.shift)
    if p.res is not None:
        acc = acc + f(p.res)
    if p.relu and not absolute:
        acc = acc.clamp_min(0.0)
    return acc.numpy()


def run(case, p, dev, variant=None):
    """Call the case's C entry point on `dev`; returns the [n_out, cout] output as float64 (after checking the guard rows)."""
    L = _lib.lib()
    t = lambda a, dt=torch.float32: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)
    xdt = torch.float16 if case.in_half else torch.float32
    cin, cout, c0 = case.cin, case.cout, p.c0
    x0, x1 = t(p.x[:, :c0], xdt), (t(p.x[:, c0:], xdt) if c0 < cin else None)
    w = t(p.w)
    K = p.w.shape[0]
    if case.entry == "mfma":
        w = ops.mfma_weight(w)
    elif case.entry == "b3":
        w = ops.b3_weight(w)
    elif case.family in ("f16x", "f16x_c16"):
        w = ops.mfma_weight16_half(w)
    nbr = t(p.nbr, torch.int32)
    stride = (p.nbr.shape[1] if p.stride < 0 else p.stride) if p.nbr is not None else 0
    res = t(p.res, torch.float16 if case.out_half else torch.float32)
    scale, shift, order = t(p.scale), t(p.shift), t(p.order, torch.int32)
    ydt = torch.float16 if case.out_half else torch.float32
    y = torch.full((p.n_out + GUARD, cout), float("nan"), dtype=ydt, device=dev)
    P = _lib.ptr
    head = (P(x0), c0, P(x1), cin, P(nbr), K, p.n_out, P(w), cout, P(scale), P(shift), P(res), int(p.relu), P(y))
    s = _lib.stream(torch.device(dev))
    v = case.variant if variant is None else variant
    if case.entry == "fwd":
        rc = L.st_sparse_conv_fwd(*head, P(order), s, stride)
    elif case.entry == "mfma":
        rc = L.st_sparse_conv_mfma_fwd(*head, P(order), s, stride, v)
    elif case.entry == "b3":
        rc = L.st_sparse_conv_b3_fwd(*head, P(order), s, stride, v)
    else:
        rc = L.st_sparse_conv_f16_fwd(*head, int(case.in_half), int(case.out_half), P(order), s, stride)
    _lib.check(rc)
    y = y.cpu()
    assert torch.isnan(y[p.n_out:].float()).all(), "a kernel wrote past row n_out"
    return y[: p.n_out].double().numpy()


def expected_exact(case, p):
    ref = reference(p)
    with np.errstate(over="ignore"):  # beyond 65 504: +-inf, as the kernel's store rounds
        return ref.astype(np.float16).astype(np.float64) if case.out_half else ref


def check_exact(case, p, dev, variant=None):
    got = run(case, p, dev, variant)
    np.testing.assert_array_equal(got, expected_exact(case, p), err_msg=str(case))


def half_ulp(r):
    """Half an ulp of IEEE half precision at |r| (normal range; 2^-25 below it)."""
    _, e = np.frexp(np.abs(r))
    return np.where(np.abs(r) >= 2.0 ** -14, np.ldexp(1.0, e - 12), 2.0 ** -25)


def real_errors(case, p, got):
    """(worst error / (2^-24 A) beyond the half rounding, share of half outputs equal to the correctly rounded reference)."""
    ref, A = reference(p), reference(p, absolute=True)
    err = np.abs(got - ref)
    if case.out_half:
        err = np.maximum(err - half_ulp(ref), 0.0)
    share = float(np.mean(got == ref.astype(np.float16).astype(np.float64))) if case.out_half else 1.0
    return float((err / (2.0 ** -24 * A + 1e-300)).max()), share


# ------------------------------------------------------------------------------------------------------- regime 1: exact ---
@pytest.mark.parametrize("case", CASES, ids=str)
def test_every_instance_exact(backend, case):
    """Every instance and tile variant with concat, BatchNorm affine, residual, ReLU, a random row order and a capacity-strided
    table, bit for bit."""
    check_exact(case, make_problem(case, seed=zlib.crc32(str(case).encode()) % 1000), backend)


@pytest.mark.parametrize("n_out", [1, 15, 16, 17, 63, 65, 127, 129, 257, 601])
@pytest.mark.parametrize("fam", FAM)
def test_partial_tiles_waves_and_blocks(backend, fam, n_out):
    """Partial 16-row tiles, wavefronts and workgroups of every tile shape (row order none: the tail guard on the plain index)."""
    case = FAMILIES[fam]
    check_exact(case, make_problem(case, seed=n_out, n_out=n_out, density=0.3, order="none"), backend)


@pytest.mark.parametrize("n_in", ["fewer", "more"])
@pytest.mark.parametrize("fam", FAM)
def test_input_rows_fewer_and_more_than_output_rows(backend, fam, n_in):
    """Tables that point at input row 0 and row n_in - 1, with n_in below and above n_out."""
    case = FAMILIES[fam]
    check_exact(case, make_problem(case, seed=7, n_out=129, n_in=40 if n_in == "fewer" else 611), backend)


@pytest.mark.parametrize("kind", ["empty_offsets", "empty_rows", "dense"])
@pytest.mark.parametrize("fam", FAM)
def test_table_density(backend, fam, kind):
    """Offsets empty for every row (the wave-uniform skip), rows with no neighbour at all, a fully dense 27-offset table."""
    case = FAMILIES[fam]
    p = make_problem(case, seed=11, n_out=385, density=1.0 if kind == "dense" else 0.5, kind=None if kind == "dense" else kind,
                     order="none" if kind == "empty_rows" else "perm")
    check_exact(case, p, backend)


@pytest.mark.parametrize("K", [27, 8, 1, "pointwise"])
@pytest.mark.parametrize("fam", FAM)
def test_kernel_offset_counts(backend, fam, K):
    """K = 27, an even K (the 16-channel pair kernels without the zero pad), K = 1 with a table and pointwise (no table)."""
    case = FAMILIES[fam]
    pw = K == "pointwise"
    check_exact(case, make_problem(case, seed=13, n_out=129, K=1 if pw else K, pointwise=pw, density=0.6), backend)


ENTRY_SPLIT_CASES = {  # the widest input of every entry (and tile variant) that takes a concat
    "vec_16": Case("fwd", "vec", 16, 16), "vec_8": Case("fwd", "vec", 8, 16), "vec_3": Case("fwd", "vec", 3, 8),
    "vec_64": Case("fwd", "vec", 64, 32),
    "mfma_v1": Case("mfma", "mfma", 64, 32, 1), "mfma_v18": Case("mfma", "mfma", 64, 32, 18),
    "b3_rt1": Case("b3", "b3", 64, 32, 1), "b3_rt2": Case("b3", "b3", 64, 32, 2), "f16x": Case("f16", "f16x", 64, 32),
}


@pytest.mark.parametrize("name", list(ENTRY_SPLIT_CASES))
def test_every_legal_concat_split(backend, name):
    """Every split the entry accepts: st_sparse_conv_fwd any 0 < c0 <= cin (the unaligned ones on the generic kernel), the f32
    matrix-core kernel c0 % 16, split-bf16 c0 % 8, half precision c0 % 16."""
    case = ENTRY_SPLIT_CASES[name]
    splits = legal_splits(case)
    if case.entry == "fwd" and case.cin == 64:
        splits = [s for s in splits if s % 4 == 0] + [1, 6, 33, 63]
    for c0 in splits:
        check_exact(case, make_problem(case, seed=c0, n_out=65, c0=c0), backend)


@pytest.mark.parametrize("epilogue", ["none", "affine", "full"])
@pytest.mark.parametrize("fam", FAM)
def test_epilogues(backend, fam, epilogue):
    case = FAMILIES[fam]
    check_exact(case, make_problem(case, seed=17, n_out=129, epilogue=epilogue), backend)


@pytest.mark.parametrize("form", ["contiguous", "capacity_strided"])
@pytest.mark.parametrize("fam", FAM)
def test_table_stride(backend, fam, form):
    """nbr_stride = 0 on a [K, n_out] table, and a column slice [:, :n] of a [K, cap] table (cap > n) as the brick pyramid passes."""
    case = FAMILIES[fam]
    p = make_problem(case, seed=19, n_out=129, cap_extra=0 if form == "contiguous" else 93)
    if form == "contiguous":
        p.stride = 0
    check_exact(case, p, backend)


@pytest.mark.parametrize("order", ["none", "perm", "tagged_grouped", "tagged_mixed"])
@pytest.mark.parametrize("fam", FAM)
def test_row_orders(backend, fam, order):
    """No order, an untagged permutation, parity-tagged rows grouped by class, and tagged rows in random order (every wavefront
    mixes classes and untagged rows): the tables hold entries only at a tagged row's live offsets, so the result is the same."""
    case = FAMILIES[fam]
    check_exact(case, make_problem(case, seed=23, n_out=257, order=order), backend)


@pytest.mark.parametrize("fam", ["f16x", "f16x_c16", "cast_f2h"])
def test_half_outputs_overflow_to_inf(backend, fam):
    """Sums beyond 65 504 (exact in float32) round to +-inf on the half store, as torch's rounding does."""
    case = FAMILIES[fam]
    p = make_problem(case, seed=29, n_out=129, density=0.9, epilogue="none", order="perm")
    rng = np.random.RandomState(31)
    p.x = rng.randint(16, 33, size=p.x.shape).astype(np.float32)
    sign = rng.choice([-1, 1], size=p.w.shape)  # output columns 4j: all weights positive (sums beyond 65 504), 4j + 1: all
    sign[:, :, 0::4], sign[:, :, 1::4] = 1, -1  # negative, the others mixed (finite sums)
    p.w = (rng.randint(16, 33, size=p.w.shape) * sign).astype(np.float32)
    exp = expected_exact(case, p)
    assert np.isinf(exp).any() and np.isfinite(exp).any() and (exp > 0).any() and (exp < 0).any()
    np.testing.assert_array_equal(run(case, p, backend), exp)


@pytest.mark.parametrize("knob,value", [("MFMA_VARIANT", v) for v in MFMA_VARIANTS] + [("B3_VARIANT", v) for v in (1, 2)])
def test_bench_aid_variants_through_sparse_ops(backend, knob, value):
    """tools/bench_conv.py times the tile variants through sparse_ops' module knobs: each must compute the exact result."""
    rng = np.random.RandomState(value)
    n, n_in, K, cin, cout = 200, 170, 27, 32, 32
    x = torch.from_numpy(rng.randint(-4, 5, size=(n_in, cin)).astype(np.float32))
    w = torch.from_numpy(rng.randint(-4, 5, size=(K, cin, cout)).astype(np.float32))
    nbr = rng.randint(0, n_in, size=(K, n)).astype(np.int32)
    nbr[rng.rand(K, n) < 0.5] = -1
    ref = reference(Problem(x.numpy(), w.numpy(), nbr, n, cin))
    order = torch.from_numpy(rng.permutation(n).astype(np.int32)).to(backend)
    xd, wd, nd = x.to(backend), w.to(backend), torch.from_numpy(nbr).to(backend)
    kw = dict(wp=ops.mfma_weight(wd)) if knob == "MFMA_VARIANT" else dict(wq=ops.b3_weight(wd))
    setattr(ops, knob, value)
    try:
        got = ops.sparse_conv(xd, wd, nd, n, row_order=order, **kw)
    finally:
        setattr(ops, knob, 0)
    np.testing.assert_array_equal(got.cpu().double().numpy(), ref)


# ------------------------------------------------------------------------------------------------- regime 2: real values ---
@pytest.mark.parametrize("case", CASES, ids=str)
def test_every_instance_real_values(backend, case):
    """Random normal features (rows e^12 apart in scale), real weights and epilogue: within C_REAL * 2^-24 of the float64 contraction
    of absolute values, plus half an ulp for half outputs, and at least HALF_EXACT_SHARE of half outputs correctly rounded."""
    p = make_problem(case, seed=1 + zlib.crc32(str(case).encode()) % 1000, n_out=257, n_in=300, exact=False)
    worst, share = real_errors(case, p, run(case, p, backend))
    assert worst <= C_REAL, (str(case), worst)
    assert share >= HALF_EXACT_SHARE, (str(case), share)


@pytest.mark.parametrize("cin,cout", VEC_SHAPES)
def test_unaligned_split_gives_the_instance_bits(backend, cin, cout):
    """st_sparse_conv_fwd serves a split the instantiated kernel cannot (no multiple of 4, or a concat of a 3-channel input) on the
    generic kernel, which runs the same fmaf chain: real-valued results equal the instance's (no concat, or an aligned split)
    bit for bit."""
    case = Case("fwd", "vec", cin, cout)
    base = make_problem(case, seed=37, n_out=140, exact=False, c0=cin)
    want = run(case, base, backend)
    for c0 in sorted({1, 2, cin // 2 + 1, cin - 1} - {0, cin}):
        base.c0 = c0
        np.testing.assert_array_equal(run(case, base, backend), want, err_msg=f"c0={c0}")
    # and the generic kernel itself (a cout without an instance, the extra columns zero) on the instance's columns
    wide = Case("fwd", "any", cin, cout + 4)
    base.c0 = cin
    base.w = np.concatenate([base.w, np.zeros((base.w.shape[0], cin, 4), np.float32)], 2)
    base.scale, base.shift = np.concatenate([base.scale, np.ones(4, np.float32)]), np.concatenate([base.shift, np.zeros(4, np.float32)])
    base.res = np.concatenate([base.res, np.zeros((base.n_out, 4), np.float32)], 1)
    np.testing.assert_array_equal(run(wide, base, backend)[:, :cout], want)


# ---------------------------------------------------------------------------------------------- production tile switches ---
THRESHOLD_CASES = [  # (case, rows below / at the switch, with a row_order)
    (Case("mfma", "mfma", 16, 16), 150000, False),
    *[(Case(e, f, ci, co), n, ro) for e, f, ci, co in (("b3", "b3", 32, 16), ("b3", "b3_c16", 16, 16), ("f16", "f16x", 32, 16),
                                                      ("f16", "f16x_c16", 16, 16))
      for n, ro in ((56000, False), (300000, True))],
]
# two row tiles per wavefront on every half-precision shape (those have no variant argument: only the size selects them)
RT2_HALF_CASES = [Case("f16", "f16x", ci, co) for ci, co in B3_SHAPES] + [Case("f16", "f16x_c16", ci, co) for ci, co in C16_SHAPES]


@pytest.mark.gpu
@pytest.mark.parametrize("side", [-1, 0])
@pytest.mark.parametrize("case,switch,with_order", THRESHOLD_CASES, ids=lambda v: str(v) if isinstance(v, Case) else str(v))
def test_production_thresholds(case, switch, with_order, side, monkeypatch):
    """The size-picked tile shape on both sides of each switch (variant 0), bit for bit."""
    monkeypatch.setattr(_lib, "_LIB", None)
    dev = torch.device("cuda:0")
    p = make_problem(case, seed=41, n_out=switch + side, n_in=switch // 2, density=0.15, cap_extra=0,
                     order="tagged_mixed" if with_order else "none")
    check_exact(case, p, dev)


@pytest.mark.gpu
@pytest.mark.parametrize("case", RT2_HALF_CASES, ids=str)
def test_half_two_row_tiles_every_shape(case, monkeypatch):
    """Two row tiles per wavefront (from 56 000 rows) on every half-precision matrix-core shape, bit for bit."""
    monkeypatch.setattr(_lib, "_LIB", None)
    check_exact(case, make_problem(case, seed=43, n_out=56000 + 17, n_in=30000, density=0.15), torch.device("cuda:0"))


# ------------------------------------------------------------------------------------------------------------- routing ---
def test_sparse_ops_routes_the_shipped_layers(backend, monkeypatch):
    """sparse_ops.sparse_conv sends every layer of the shipped architecture to the entry point Smart_Tree expects: float32 mode ->
    split-bf16 for the >= 16-channel levels, the vector kernel at level 0; matrix-core f32 when split-bf16 is off (16 -> 16
    submanifold stays on the vector kernel); half mode -> f16 with the converting kernels between level 0 and 1."""
    from oracle import unet_oracle as uo
    from smart_tree_amd.model.model import Smart_Tree
    from smart_tree_amd.model.sparse import sparse_from_batch

    w = uo.load_weights(Path(__file__).resolve().parents[1] / "smart_tree_amd" / "model" / "weights" / "noble-elevator-58.npz")
    rng = np.random.RandomState(3)
    coords = np.unique(np.c_[np.zeros(700, int), rng.randint(0, 12, size=(700, 3))], axis=0).astype(np.int32)
    feats = rng.randn(coords.shape[0], 3).astype(np.float32)
    inner, calls = _lib.lib(), []

    class Recorder:
        def __getattr__(self, name):
            fn = getattr(inner, name)
            if not name.startswith("st_sparse_conv"):
                return fn

            def rec(*a):
                k1 = a[4] is None
                calls.append((name.replace("st_sparse_conv_", "").replace("_fwd", "") or "fwd", a[3], a[8], "k1" if k1 else "k27",
                              "cat" if a[1] < a[3] else "", "ord" if a[-4 if name in ("st_sparse_conv_mfma_fwd", "st_sparse_conv_b3_fwd") else -3] is not None else ""))
                return fn(*a)
            return rec

    monkeypatch.setattr(_lib, "_LIB", Recorder())
    F, M, B, H = "fwd", "mfma", "b3", "f16"
    f32 = {(F, 3, 8, "k1", "", ""), (F, 8, 8, "k27", "", ""), (F, 8, 16, "k27", "", ""), (F, 16, 8, "k27", "", "ord"),
           (F, 16, 8, "k27", "cat", ""), (F, 16, 8, "k1", "cat", "")}
    mode = {
        "b3": f32 | {(B, 16, 16, "k27", "", ""), (B, 16, 32, "k27", "", ""), (B, 32, 32, "k27", "", ""), (B, 32, 64, "k27", "", ""),
                     (B, 64, 64, "k27", "", ""), (B, 64, 32, "k27", "", "ord"), (B, 64, 32, "k27", "cat", ""), (B, 64, 32, "k1", "cat", ""),
                     (B, 32, 16, "k27", "", "ord"), (B, 32, 16, "k27", "cat", ""), (B, 32, 16, "k1", "cat", "")},
        "mfma": f32 | {(F, 16, 16, "k27", "", ""), (M, 16, 32, "k27", "", ""), (M, 32, 32, "k27", "", ""), (M, 32, 64, "k27", "", ""),
                       (M, 64, 64, "k27", "", ""), (M, 64, 32, "k27", "", "ord"), (M, 64, 32, "k27", "cat", ""), (M, 64, 32, "k1", "cat", ""),
                       (M, 32, 16, "k27", "", "ord"), (M, 32, 16, "k27", "cat", ""), (M, 32, 16, "k1", "cat", "")},
        "fp16": {(F, 3, 8, "k1", "", ""), (F, 8, 8, "k27", "", ""), (H, 8, 16, "k27", "", ""), (H, 16, 8, "k27", "", "ord"),
                 (F, 16, 8, "k27", "cat", ""), (F, 16, 8, "k1", "cat", ""), (H, 16, 16, "k27", "", ""), (H, 16, 32, "k27", "", ""),
                 (H, 32, 32, "k27", "", ""), (H, 32, 64, "k27", "", ""), (H, 64, 64, "k27", "", ""), (H, 64, 32, "k27", "", "ord"),
                 (H, 64, 32, "k27", "cat", ""), (H, 64, 32, "k1", "cat", ""), (H, 32, 16, "k27", "", "ord"), (H, 32, 16, "k27", "cat", ""),
                 (H, 32, 16, "k1", "cat", "")},
    }
    for name, want in mode.items():
        net = Smart_Tree(w, device=backend, fp16=name == "fp16")
        net.use_b3 = name == "b3"
        calls.clear()
        net.features(sparse_from_batch(torch.from_numpy(feats), torch.from_numpy(coords), backend))
        assert set(calls) == want, (name, sorted(set(calls) ^ want))


# ------------------------------------------------------------------------------------------------------------ coverage ---
def dispatched_instances(src: str):
    """(table, shape) of every kernel instance the dispatch tables of sparse_conv.hip name: their rows are <TABLE>_CASE(cin, cout[,
    cout tile]) (numeric macro arguments only: the #define lines take parameter names).  A sixteen-input-channel row of the
    split-bf16 / half tables is the pair kernel, counted per row-tile count: ("B3_C16" / "F16X_C16", (cout, row tiles))."""
    out = set()
    for m in re.finditer(r"\b([A-Z0-9]+)_CASE\((\d+),\s*(\d+)(?:,\s*(\d+))?\)", src):
        table, args = m.group(1), tuple(int(g) for g in m.groups()[1:] if g is not None)
        if table in ("B3", "F16X") and args[0] == 16:
            out |= {(table + "_C16", (args[1], rt)) for rt in (1, 2)}
        else:
            out.add((table, args))
    return out


def uncovered(src: str):
    cov = {(c.family, c.cin, c.cout, c.variant) for c in CASES}
    cov |= {(c.family, c.cin, c.cout, 2) for c, _, _ in THRESHOLD_CASES} | {(c.family, c.cin, c.cout, 2) for c in RT2_HALF_CASES}
    need = {
        "CONV": lambda a: [("vec", a[0], a[1], 0)],
        "MFMA": lambda a: [("mfma", a[0], a[1], v) for v in MFMA_VARIANTS],
        "B3": lambda a: [("b3", a[0], a[1], rt) for rt in (1, 2)],
        "B3_C16": lambda a: [("b3_c16", 16, a[0], a[1])],
        "F16X_C16": lambda a: [("f16x_c16", 16, a[0], 0 if a[1] == 1 else 2)],
        "F16X": lambda a: [("f16x", a[0], a[1], 0), ("f16x", a[0], a[1], 2)],
        "CAST": lambda a: [("cast_f2h", a[0], a[1], 0), ("cast_h2f", a[0], a[1], 0)],
    }
    return sorted((macro, args) for macro, args in dispatched_instances(src) if not set(need[macro](args)) <= cov)


def test_every_dispatched_instance_has_a_case():
    """Adding a kernel instance to the dispatch of sparse_conv.hip without a row in CASES (or the GPU threshold tables) fails here."""
    src = SRC.read_text()
    inst = dispatched_instances(src)
    assert len(inst) == 11 + 7 + 5 + 4 + 4 + 5 + 4, sorted(inst)  # the macros are still found
    assert uncovered(src) == []
    # the check notices a new instance
    extra = src.replace("    CONV_CASE(3, 8, 8)\n", "    CONV_CASE(3, 8, 8)\n    CONV_CASE(12, 24, 8)\n")
    assert extra != src and uncovered(extra) == [("CONV", (12, 24, 8))]
    extra = src.replace("    B3_CASE(16, 32)\n", "    B3_CASE(16, 32)\n    B3_CASE(16, 64)\n")  # a pair-kernel row: both row-tile counts
    assert extra != src and uncovered(extra) == [("B3_C16", (64, 1)), ("B3_C16", (64, 2))]


def test_half_weights_only_for_shapes_with_a_kernel():
    """The half-precision matrix-core weights exist for the shapes st_sparse_conv_f16_fwd has a kernel for; any other is refused."""
    for cin, cout in B3_SHAPES + C16_SHAPES:
        assert ops.mfma_weight16_half(torch.zeros(27, cin, cout)).dtype == torch.float16
    for cin, cout in [(16, 64), (48, 16)]:
        with pytest.raises(ValueError):
            ops.mfma_weight16_half(torch.zeros(27, cin, cout))
