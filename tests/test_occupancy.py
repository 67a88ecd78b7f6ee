"""Beam occupancy (csrc/occupancy.hip, smart_tree_amd/occupancy.py): beams walked through voxel grids.

Kernel level, on the CPU build and on the GPU: hand-checked scenes with exact expectations; every case in both forms (aggregated,
plain) bit for bit, a second call bit for bit, and against tests/occupancy_oracle.py's float32 restatement exactly -- the tallies
are integers, so there is no tolerance.  The random case also against the oracle's float64 brute force (a slab test of every beam
against every cell), two-sided, tau = 1e-4 cell, nothing left out.  Python level through the scanner; the physics of a Poisson
field of spheres on the GPU, with the oracle's own estimate checked on the CPU.
"""
import functools
import math
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from smart_tree_amd import _lib
from smart_tree_amd import occupancy as OC
from smart_tree_amd import scan as SC
from smart_tree_amd.dataset import synthetic as S

import occupancy_oracle as O

F = np.float32
INF = math.inf
TALLIES = ("enter", "hit", "behind", "path")
ROOT = Path(__file__).resolve().parents[1]


# --------------------------------------------------------------------------------------------------- helpers ---
def _grid(lo, cell, dim):
    return OC.VoxelGrid(lo, cell, dim)


def _call(dev, beams, grids, beam_off=None, form="aggregated", **kw):
    """One `beam_tally` call; per grid the four tallies and hit_cell as numpy, and the two counters."""
    origins, idx, dir, rng = beams
    t = lambda x, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(x, dt))).to(dev)
    res = OC.beam_tally(t(origins, F).reshape(-1, 3), t(idx, np.int32), t(dir, F).reshape(-1, 3), t(rng, F), list(grids), beam_off,
                        form=form, hit_cell=True, **kw)
    out = []
    for r in res:
        assert r.enter.device.type == dev.type and tuple(r.enter.shape) == r.grid.dim and r.path.dtype == torch.int64
        out.append({**{k: getattr(r, k).cpu().numpy() for k in TALLIES}, "hit_cell": r.hit_cell.cpu().numpy(), "n_bad": r.n_bad,
                    "n_outside": r.n_outside})
    return out


def _same(got, want, what):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        for name in TALLIES + ("hit_cell",):
            np.testing.assert_array_equal(g[name].astype(np.int64), w[name].astype(np.int64), err_msg=f"{what}: grid {k}: {name}")
        assert (g["n_bad"], g["n_outside"]) == (w["n_bad"], w["n_outside"]), f"{what}: grid {k}: counters"


def _check(dev, beams, grids, beam_off=None, **kw):
    """Aggregated and plain give the same bits, a second call the same again, "auto" the same, and all equal the float32 oracle."""
    got = _call(dev, beams, grids, beam_off, "aggregated", **kw)
    _same(_call(dev, beams, grids, beam_off, "plain", **kw), got, "plain against aggregated")
    _same(_call(dev, beams, grids, beam_off, "aggregated", **kw), got, "a second aggregated call")
    _same(_call(dev, beams, grids, beam_off, "auto", **kw), got, "auto")
    off = [0, len(beams[3])] if beam_off is None else list(beam_off)
    want, n_bad, n_outside = O.walk32_grids(*beams, [(g.lo, g.cell, g.dim) for g in grids], off, kw.get("max_range", INF), kw.get("behind", True))
    for w in want:
        w["n_bad"], w["n_outside"] = n_bad, n_outside
    _same(got, want, "against the float32 oracle")
    return got


def _beams(origins, idx, dir, rng):
    return (np.asarray(origins, F).reshape(-1, 3), np.asarray(idx, np.int32).reshape(-1), np.asarray(dir, F).reshape(-1, 3),
            np.asarray(rng, F).reshape(-1))


def _unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(F)


ROW = _grid((0, 0, 0), 1.0, (4, 1, 1))
START = (-0.5, 0.5, 0.5)


def _row(dev, rng, origin=START, direction=(1, 0, 0), **kw):
    d = _check(dev, _beams([origin], [0], [direction], [rng]), [ROW], **kw)[0]
    return {k: d[k].reshape(-1).tolist() for k in TALLIES} | {"hit_cell": int(d["hit_cell"][0]), "n_outside": d["n_outside"], "n_bad": d["n_bad"]}


# ------------------------------------------------------------------------------------- hand-checked scenes ---
@pytest.mark.parametrize("rng,kw,enter,hit,behind,path,hit_cell,n_outside", [
    (2.25, {}, [1, 1, 0, 0], [0, 1, 0, 0], [0, 0, 1, 1], [65536, 49152, 0, 0], 1, 0),
    (INF, {}, [1, 1, 1, 1], [0] * 4, [0] * 4, [65536] * 4, -1, 0),
    (0.25, {}, [0] * 4, [0] * 4, [1, 1, 1, 1], [0] * 4, -1, 0),
    (9.0, {}, [1, 1, 1, 1], [0] * 4, [0] * 4, [65536] * 4, -1, 0),
    (2.25, {"behind": False}, [1, 1, 0, 0], [0, 1, 0, 0], [0] * 4, [65536, 49152, 0, 0], 1, 0),
    (INF, {"max_range": 1.0}, [1, 0, 0, 0], [0] * 4, [0] * 4, [32768, 0, 0, 0], -1, 0),
], ids=["return", "miss", "before-the-grid", "beyond-the-grid", "behind-off", "max-range"])
def test_one_beam_along_a_row_of_four_cells(backend, rng, kw, enter, hit, behind, path, hit_cell, n_outside):
    d = _row(backend, rng, **kw)
    assert (d["enter"], d["hit"], d["behind"], d["path"]) == (enter, hit, behind, path)
    assert (d["hit_cell"], d["n_outside"], d["n_bad"]) == (hit_cell, n_outside, 0)


def test_a_beam_that_misses_the_box(backend):
    d = _row(backend, 2.25, origin=(-0.5, 5.0, 0.5))
    assert all(d[k] == [0] * 4 for k in TALLIES) and (d["hit_cell"], d["n_outside"], d["n_bad"]) == (-1, 1, 0)
    d = _row(backend, INF, origin=(-0.5, 0.5, 0.5), direction=(-1, 0, 0))  # it points away: the interval ends before it starts
    assert all(d[k] == [0] * 4 for k in TALLIES) and (d["hit_cell"], d["n_outside"]) == (-1, 1)


def test_origin_inside_a_beam_along_minus_x_and_zero_components(backend):
    # every beam of this file's row scenes has two direction components that are exactly 0 and lies in the interior of its cells
    d = _row(backend, INF, origin=(1.5, 0.5, 0.5))
    assert d["enter"] == [0, 1, 1, 1] and d["path"] == [0, 32768, 65536, 65536] and d["n_outside"] == 0
    d = _row(backend, 0.75, origin=(1.5, 0.5, 0.5))  # ends at x = 2.25, in cell 2
    assert (d["enter"], d["hit"], d["behind"], d["path"], d["hit_cell"]) == ([0, 1, 1, 0], [0, 0, 1, 0], [0, 0, 0, 1], [0, 32768, 16384, 0], 2)
    d = _row(backend, 2.25, origin=(4.5, 0.5, 0.5), direction=(-1, 0, 0))
    assert (d["enter"], d["hit"], d["behind"], d["path"], d["hit_cell"]) == ([0, 0, 1, 1], [0, 0, 1, 0], [1, 1, 0, 0], [0, 0, 49152, 65536], 2)
    d = _row(backend, INF, origin=(1.5, 0.5, 0.5), direction=(0, 0, 1))  # along z through one cell
    assert d["enter"] == [0, 1, 0, 0] and d["path"] == [0, 32768, 0, 0]
    # a return from beyond max_range is a beam stopped by max_range
    d = _row(backend, 2.25, max_range=1.0)
    assert (d["enter"], d["hit"], d["behind"], d["path"], d["hit_cell"]) == ([1, 0, 0, 0], [0] * 4, [0] * 4, [32768, 0, 0, 0], -1)


def test_the_diagonal_of_a_cube_of_27_cells_steps_x_before_y_before_z(backend):
    g = _grid((0, 0, 0), 1.0, (3, 3, 3))
    w = _unit([1, 1, 1])
    assert w[0] == w[1] == w[2]  # so the three exits of a corner are the same float: an exact tie
    d = _check(backend, _beams([(-1, -1, -1)], [0], [w], [INF]), [g])[0]
    # from the corner of cell (k, k, k): x steps first into (k+1, k, k), then y into (k+1, k+1, k), then z -- the two cells between
    # two diagonal ones are crossed with a chord of zero and still count as entered
    cells = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 1, 1), (2, 1, 1), (2, 2, 1), (2, 2, 2)]
    want = np.zeros((3, 3, 3), np.int64)
    for c in cells:
        want[c] = 1
    np.testing.assert_array_equal(d["enter"], want)
    assert d["hit"].sum() == 0 and d["behind"].sum() == 0 and d["n_outside"] == 0
    on = [int(d["path"][k, k, k]) for k in range(3)]
    assert all(abs(q - math.sqrt(3) * 65536) <= 2 for q in on), on  # sqrt(3) cells, to a unit of the chord's own rounding or two
    assert [int(d["path"][c]) for c in cells if len(set(c)) > 1] == [0, 0, 0, 0]
    back = _check(backend, _beams([(4, 4, 4)], [0], [-w], [INF]), [g])[0]  # from the far corner: (1,2,2), (1,1,2), (1,1,1), ...
    want = np.zeros((3, 3, 3), np.int64)
    for c in [(2, 2, 2), (1, 2, 2), (1, 1, 2), (1, 1, 1), (0, 1, 1), (0, 0, 1), (0, 0, 0)]:
        want[c] = 1
    np.testing.assert_array_equal(back["enter"], want)


def test_bad_beams_are_counted_and_touch_nothing(backend):
    origins = [START, (math.nan, 0.5, 0.5)]
    beams = _beams(origins, [1, 0, 0, 2, -1, 0, 0, 0], [(1, 0, 0), (0, 0, 0), (1, 0, 0), (1, 0, 0), (1, 0, 0), (1.1, 0, 0), (math.inf, 0, 0), (1, 0, 0)],
                   [1.0, 1.0, -1.0, 1.0, 1.0, 1.0, 1.0, math.nan])
    d = _check(backend, beams, [ROW])[0]
    assert d["n_bad"] == 8 and d["n_outside"] == 0 and (d["hit_cell"] == -1).all()
    assert all(d[k].sum() == 0 for k in TALLIES)
    one_good = _beams(origins, [1, 0], [(1, 0, 0), (1, 0, 0)], [1.0, 2.25])
    d = _check(backend, one_good, [ROW])[0]
    assert d["n_bad"] == 1 and d["enter"].reshape(-1).tolist() == [1, 1, 0, 0] and d["hit_cell"].tolist() == [-1, 1]


def test_refusals(backend):
    beams = _beams([START], [0], [(1, 0, 0)], [1.0])
    with pytest.raises(ValueError, match="VoxelGrid"):
        OC.VoxelGrid((0, 0, 0), 0.0, (1, 1, 1))
    with pytest.raises(ValueError, match="VoxelGrid"):
        OC.VoxelGrid((0, 0, 0), 1.0, (1, 1025, 1))
    with pytest.raises(ValueError, match="beam_off"):
        _call(backend, beams, [ROW, ROW])
    with pytest.raises(_lib.StError, match="beam_off"):
        _call(backend, beams, [ROW, ROW], [0, 2, 1])
    with pytest.raises(_lib.StError, match="max_range"):
        _call(backend, beams, [ROW], max_range=math.nan)
    with pytest.raises(_lib.StError, match="form"):
        _call(backend, beams, [ROW], form=3)
    with pytest.raises(ValueError, match="cells in one call"):
        _call(backend, beams, [_grid((0, 0, 0), 1.0, (1024, 1024, 1024))] * 2, [0, 1, 1])
    L = _lib.lib()
    assert L.st_beam_tally_workspace_bytes(-1, 1) == -1 and L.st_beam_tally_workspace_bytes(4, 65) == -1 and L.st_version() >= 119
    assert L.st_beam_tally_workspace_bytes(4, 64) > 0


# ------------------------------------------------------------------------ shapes at which the kernel can go wrong ---
def _fan(n, origin, seed, miss_every=3, reach=(0.2, 4.0)):
    """n beams from one origin, directions in a cone about +x, every `miss_every`-th without a return."""
    rng = np.random.default_rng(seed)
    w = _unit(np.array([1.0, 0.0, 0.0]) + 0.6 * rng.uniform(-1, 1, size=(n, 3)))
    r = rng.uniform(*reach, size=n).astype(F)
    r[::miss_every] = INF
    return _beams([origin], np.zeros(n, np.int32), w, r)


def test_200_beams_share_their_first_cell(backend):
    g = _grid((-0.5, -1.5, -1.25), 0.25, (12, 12, 10))
    beams = _fan(200, (-0.4, 0.05, 0.03), 1)  # the origin lies inside the grid: every beam starts in its cell
    d = _check(backend, beams, [g])[0]
    first = (0, 6, 5)
    assert d["enter"][first] == 200 and d["n_outside"] == 0 and d["n_bad"] == 0
    assert d["hit"].sum() == (d["hit_cell"] >= 0).sum() > 50 and d["behind"].sum() > 100
    _check(backend, beams, [g], behind=False, max_range=2.0)


def test_the_same_beams_over_two_grids(backend):
    a, b = _grid((-0.5, -1.5, -1.25), 0.25, (12, 12, 10)), _grid((-0.45, -2.0, -2.0), 0.4, (7, 10, 11))
    beams = _fan(200, (-0.4, 0.05, 0.03), 1)
    two = _check(backend, beams, [a, b], [0, 120, 200])
    alone = _check(backend, tuple(x[120:] if k else x for k, x in enumerate(beams)), [b])[0]  # a grid does not depend on its call
    for k in TALLIES:
        np.testing.assert_array_equal(two[1][k], alone[k])
    assert two[0]["enter"].sum() > 120 and two[1]["enter"].sum() > 80 and two[1]["hit_cell"].shape == (80,)
    three = _check(backend, beams, [a, b, a], [0, 120, 120, 200])  # an empty grid in the middle
    assert three[1]["enter"].sum() == 0 and three[2]["enter"].sum() > 80


def test_no_beam_one_beam_one_cell_and_a_row_of_1024(backend):
    g = _grid((0, 0, 0), 0.5, (3, 2, 2))
    none = _check(backend, _beams(np.zeros((0, 3)), [], np.zeros((0, 3)), []), [g])[0]
    assert none["enter"].shape == (3, 2, 2) and all(none[k].sum() == 0 for k in TALLIES) and none["hit_cell"].shape == (0,)
    one = _check(backend, _beams([(-1, 0.3, 0.6)], [0], [_unit([1, 0.1, 0.05])], [1.7]), [g])[0]
    assert one["hit"].sum() == 1 and one["hit_cell"][0] >= 0
    cell = _grid((0, 0, 0), 2.0, (1, 1, 1))
    d = _check(backend, _fan(70, (-1.0, 1.0, 1.0), 2, reach=(0.5, 3.5)), [cell])[0]
    assert d["enter"].shape == (1, 1, 1) and d["enter"][0, 0, 0] > 20 and d["hit"][0, 0, 0] > 5
    row = _grid((-5.12, -0.005, -0.005), 0.01, (1024, 1, 1))
    w = np.concatenate([[[1, 0, 0], [-1, 0, 0]], _unit(np.array([1.0, 0, 0]) + 1e-4 * np.random.default_rng(3).uniform(-1, 1, (66, 3)))])
    o = np.array([(-6.0, 0, 0), (6.0, 0, 0), (0.0033, 0.001, -0.002)])
    beams = _beams(o, [0, 1] + [0] * 33 + [2] * 33, w, [INF, 7.5] + [INF, 3.0, 9.0] * 22)
    d = _check(backend, beams, [row])[0]
    assert d["enter"][:, 0, 0].min() >= 1 and d["enter"][0, 0, 0] >= 2 and d["behind"].sum() > 0  # the two axis beams cross all 1024 cells


# ------------------------------------------------------------------------------------------- random parity ---
RANDOM_GRID = ((-2.0, -1.0, -1.5), 0.37, (13, 7, 9))
RANDOM_SEED = 5


@functools.lru_cache(maxsize=None)
def _random_case():
    """4096 beams: origins inside the grid and up to 3 m outside it, a third without a return, ranges from 0 to 8 m; the beams from
    outside mostly aim at a point of the grid, the others anywhere.  With the two oracle runs (computed once, never changed)."""
    lo, cell, dim = RANDOM_GRID
    rng = np.random.default_rng(RANDOM_SEED)
    lo64, hi64 = np.asarray(lo), np.asarray(lo) + cell * np.asarray(dim)
    n = 4096
    origins = rng.uniform(lo64 - 3.0, hi64 + 3.0, size=(n, 3))
    inside = rng.uniform(size=n) < 0.3
    origins[inside] = rng.uniform(lo64, hi64, size=(int(inside.sum()), 3))
    target = rng.uniform(lo64, hi64, size=(n, 3))
    aimed = ~inside & (rng.uniform(size=n) < 0.85)  # the other beams from outside point anywhere: most of them miss the grid
    w = np.where(aimed[:, None], target - origins, rng.normal(size=(n, 3)))
    r = rng.uniform(0.0, 8.0, size=n).astype(F)
    r[rng.uniform(size=n) < 1.0 / 3.0] = INF
    beams = _beams(origins, np.arange(n), _unit(w), r)
    o32 = O.walk32(*beams, lo, cell, dim)
    o64 = O.brute64(*beams, lo, cell, dim)
    for d in (o32, o64):
        for v in d.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return beams, o32, o64


def _against_float64(d, beams, o64, what):
    """The two-sided bounds of a result (the kernel's, or the float32 oracle's own) against the float64 brute force."""
    lo, cell, dim = RANDOM_GRID
    tau = o64["tau"]
    assert tau == 1e-4 * float(F(cell))
    enter, behind = d["enter"].astype(np.int64), d["behind"].astype(np.int64)
    for name, got, strict, loose in (("enter", enter, o64["enter_strict"], o64["enter_loose"]), ("behind", behind, o64["behind_strict"], o64["behind_loose"])):
        print(f"{what}: {name}: {got.sum()} in all, strict {strict.sum()}, loose {loose.sum()}; cells where loose > strict: {(loose > strict).sum()}")
        assert (strict <= got).all() and (got <= loose).all(), f"{what}: {name} outside [strict, loose] in {((strict > got) | (got > loose)).sum()} cell(s)"
    # every return lies within tau of its hit cell; a return without one lies outside the grid or within tau of its boundary
    rows, hc = o64["rows"], d["hit_cell"]
    assert (hc[np.setdiff1d(np.arange(len(hc)), rows)] == -1).all()
    hcg, ret, pt = hc[rows], o64["ret"], o64["point"]
    assert not (hcg[~ret] >= 0).any()
    has = ret & (hcg >= 0)
    blo, bhi = O.cell_box(hcg[has], o64["grid_lo"], float(F(cell)), dim)
    dist = O.box_distance(pt[has], blo, bhi)
    print(f"{what}: {has.sum()} returns with a hit cell, farthest from it {dist.max():.3g} m (tau {tau:.3g}); {(ret & (hcg < 0)).sum()} returns without")
    assert (dist <= tau).all()
    no = ret & (hcg < 0)
    deep = ((pt[no] >= o64["grid_lo"] + tau) & (pt[no] <= o64["grid_hi"] - tau)).all(1)
    assert not deep.any(), f"{what}: {deep.sum()} return(s) deep inside the grid without a hit cell"
    # path per cell and in all
    metres = d["path"].astype(np.float64) / 65536.0 * float(F(cell))
    err = np.abs(metres - o64["chord_sum"])
    bound = o64["enter_loose"] * (math.sqrt(3) * tau + float(F(cell)) / 131072.0)
    print(f"{what}: path per cell: worst error {err.max():.3g} m, worst error / bound {np.max(err / np.maximum(bound, 1e-300)):.3g}")
    assert (err <= bound).all()
    return float(metres.sum())


def test_the_oracle_alone_meets_its_float64_bounds():
    beams, o32, o64 = _random_case()
    assert o32["n_bad"] == 0 and 0 < o32["n_outside"] < 2000 and (o32["hit_cell"] >= 0).sum() > 500 and o32["behind"].sum() > 2000
    total32 = _against_float64(o32, beams, o64, "float32 oracle")
    assert abs(total32 - o64["free_total"]) <= o32["enter"].astype(np.int64).sum() * float(F(RANDOM_GRID[1])) / 131072.0


def test_random_beams_against_both_oracles(backend):
    beams, o32, o64 = _random_case()
    lo, cell, dim = RANDOM_GRID
    d = _check(backend, beams, [_grid(lo, cell, dim)])[0]  # (equal to o32, bit for bit, in there)
    total = _against_float64(d, beams, o64, "kernel")
    total32 = o32["path"].astype(np.float64).sum() / 65536.0 * float(F(cell))
    bound = d["enter"].astype(np.int64).sum() * float(F(cell)) / 131072.0 + 4.0 * abs(total32 - o64["free_total"])
    print(f"free length in the grid: kernel {total:.6f} m, float64 {o64['free_total']:.6f} m, bound {bound:.3g} m")
    assert abs(total - o64["free_total"]) <= bound


# ------------------------------------------------------------------------------------- through the scanner ---
def _tally_of(extras, grid, scanner=None, **kw):
    sel = slice(None) if scanner is None else extras["beam_scanner"] == scanner
    return OC.beam_tally(extras["origins"], extras["beam_scanner"][sel], extras["beam_dir"][sel], extras["beam_range"][sel], grid, **kw)


def test_through_the_scanner(backend):
    # the CPU build runs wave collectives as rendezvous of 64 fibers: there the plain form (the same bits, see _check) keeps this
    # test at seconds; on the GPU the default form runs
    form = dict(form="plain" if backend.type == "cpu" else "auto")
    kw = dict(step_deg=0.5, radius=6.0, height=1.5, max_depth=3, range_noise=0.0, device=backend)
    cloud, skeletons, extras = S.scan_trees([21], 2, beams=True, **kw)
    _, base = SC.scan_skeletons(skeletons, [SC.scanner_ring(2, 6.0, 1.5, SC.skeleton_box(skeletons[0]), 4.0, seed=21, range_noise=0.0)], device=backend)
    assert set(base) == {"ray", "scanner", "range", "segment", "dir", "tube_off", "ray_off"}  # beams=False: the keys of today
    assert set(extras) == set(base) | {"beam_dir", "beam_range", "beam_scanner", "origins"}
    R = int(extras["ray_off"][-1])
    assert extras["beam_dir"].shape == (R, 3) and extras["beam_range"].shape == (R,) and extras["origins"].shape == (2, 3)
    assert torch.equal(extras["beam_range"][extras["ray"].long()], extras["range"]) and torch.equal(extras["beam_dir"][extras["ray"].long()], extras["dir"])
    assert int(torch.isfinite(extras["beam_range"]).sum()) == len(cloud)
    grid = OC.VoxelGrid.around(cloud.xyz, 0.1)
    both = _tally_of(extras, grid, hit_cell=True, **form)
    assert both.n_bad == 0 and both.enter.shape == grid.dim
    returned = torch.isfinite(extras["beam_range"])
    hc = both.hit_cell.long()
    assert not (hc[~returned] >= 0).any()
    assert int(both.hit.sum()) == int((hc[returned] >= 0).sum()) > 0.99 * len(cloud)
    state = both.state()
    assert (state.reshape(-1)[hc[hc >= 0]] == 2).all()
    # hit / enter / behind and the four states fit together
    assert ((both.hit > 0) <= (both.enter > 0)).all() and set(state.unique().tolist()) <= {0, 1, 2, 3} and (state == 1).any()
    assert (OC.visibility_of_points(both, cloud.xyz) == 2).all()
    far = OC.visibility_of_points(both, torch.tensor([[1e3, 0.0, 0.0]], device=cloud.xyz.device))
    assert far.tolist() == [0]
    # one scanner alone: cells straight behind the trunk are occluded
    one_cloud, _, one = S.scan_trees([21], 1, beams=True, **kw)
    alone = _tally_of(one, grid, hit_cell=True, **form)
    trunk = (one_cloud.branch_ids.view(-1) == 0) & (one_cloud.xyz[:, 1] < 1.0)
    assert int(trunk.sum()) > 20
    hits, dirs = one_cloud.xyz[trunk], one["dir"][trunk]
    seen = torch.stack([OC.visibility_of_points(alone, hits + d * dirs) for d in (0.15, 0.2, 0.25, 0.3)])
    assert (seen == 3).any(), seen.unique().tolist()
    n_alone, n_both = int((alone.state() == 3).sum()), int((state == 3).sum())
    print(f"occluded cells: {n_alone} with one scanner, {n_both} with two, of {grid.n_cells}")
    assert 0 < n_both <= n_alone
    # beams_from_points: the returns alone, as a real scan with a scan position per point gives them
    sc = extras["scanner"].long()
    w, r = OC.beams_from_points(cloud.xyz, extras["origins"], sc)
    assert float((w - extras["dir"]).abs().max()) <= 1e-5 and float((r - extras["range"]).abs().max()) <= 1e-5
    only = OC.beam_tally(extras["origins"], sc, w, r, grid, **form)
    assert int(only.hit.sum()) >= 0.99 * len(cloud) and int(only.enter.sum()) < int(both.enter.sum())


# -------------------------------------------------------------------------------------------------- physics ---
N_SPHERES, SPHERE_R, CUBE = 2000, 0.02, 2.04
LAMBDA = N_SPHERES / CUBE ** 3 * math.pi * SPHERE_R ** 2  # 0.296 1/m
PHYSICS_GRID = ((-1.0, -1.0, -1.0), 0.25, (8, 8, 8))
PHYSICS_SEED = 12


def _sphere_field():
    return np.random.default_rng(PHYSICS_SEED).uniform(-CUBE / 2, CUBE / 2, size=(N_SPHERES, 3)).astype(F)


def _physics_scanner(step_deg):
    h = CUBE / 2
    return SC.Scanner.towards((-h, -h, -h), (h, h, h), (3.0, 0.0, 0.0), step_deg, up=2, range_noise=0.0)


def _contact_frequency(hit, path, cell):
    """Sum of hits over summed path length (1/m) over the cells that do not touch the grid's faces, and the hits."""
    inner = (slice(1, -1),) * 3
    hits = float(hit[inner].sum())
    return hits / (float(path[inner].sum()) / 65536.0 * cell), hits


def _assert_band(freq, hits, what):
    band = 5.0 / math.sqrt(hits) + 0.02
    print(f"{what}: {freq:.4f} 1/m from {hits:.0f} hits; lambda {LAMBDA:.4f}, relative error {abs(freq / LAMBDA - 1):.4f}, band {band:.4f}")
    assert abs(freq / LAMBDA - 1.0) <= band


def test_the_oracle_alone_finds_the_density_of_a_field_of_spheres():
    """Beams cast against the spheres in numpy (float64, the first root along every beam), tallied by the float32 oracle."""
    centres = _sphere_field().astype(np.float64)
    sc = _physics_scanner(0.5)
    az = sc.az[0] + np.arange(sc.az[2]) * sc.az[1]
    el = sc.el[0] + np.arange(sc.el[2]) * sc.el[1]
    A, E = np.meshgrid(az, el, indexing="ij")
    w = np.stack([np.cos(E) * np.cos(A), np.cos(E) * np.sin(A), np.sin(E)], axis=-1).reshape(-1, 3)
    o = np.asarray(sc.position)
    m = o - centres                                     # [L,3]
    r = np.empty(len(w))
    for k in range(0, len(w), 1024):                    # |o + s w - c|^2 = r^2: s^2 + 2 b s + (m.m - r^2) = 0, the nearer root
        b = w[k:k + 1024] @ m.T
        disc = b * b - ((m * m).sum(1) - SPHERE_R ** 2)[None]
        with np.errstate(invalid="ignore"):
            s = np.where(disc >= 0, -b - np.sqrt(disc), np.inf)
        s[s < sc.min_range] = np.inf
        r[k:k + 1024] = s.min(1)
    lo, cell, dim = PHYSICS_GRID
    d = O.walk32([o], np.zeros(len(r), np.int32), w.astype(F), r.astype(F), lo, cell, dim)
    _assert_band(*_contact_frequency(d["hit"].astype(np.float64), d["path"].astype(np.float64), cell), "oracle alone")


def test_the_density_of_a_field_of_spheres(backend):
    """On the GPU, and on the CPU build with all the beams (a second or two there, in the plain form)."""
    from smart_tree_amd.data_types.branch import BranchSkeleton
    from smart_tree_amd.data_types.tree import TreeSkeleton

    dev = backend
    twig = TreeSkeleton(0, {0: BranchSkeleton(0, -1, torch.tensor([[0.0, 0.0, 50.0], [0.0, 0.0, 50.001]]), torch.tensor([[1e-4], [1e-4]]))})
    centres = _sphere_field()
    _, extras = SC.scan_skeletons([twig], [[_physics_scanner(0.5)]], [(centres, np.full(N_SPHERES, SPHERE_R, F))], device=dev, beams=True)
    lo, cell, dim = PHYSICS_GRID
    tally = OC.beam_tally(extras["origins"], extras["beam_scanner"], extras["beam_dir"], extras["beam_range"], OC.VoxelGrid(lo, cell, dim), hit_cell=True,
                          form="plain" if dev.type == "cpu" else "auto")
    assert tally.n_bad == 0
    _assert_band(*_contact_frequency(tally.hit.double().cpu().numpy(), tally.path.double().cpu().numpy(), cell), "kernel")
    # plant area: attenuation / G x volume, summed; and shared among labels
    G = 0.5
    att = tally.attenuation()
    want = float((torch.nan_to_num(att, nan=0.0) / G * cell ** 3).sum())
    assert abs(tally.plant_area(G) - want) <= 1e-9 * want and want > 0
    labels = torch.zeros_like(tally.hit_cell)
    by_label = tally.plant_area_by_label(tally.hit_cell, labels, 3, G)
    area_of_hit_cells = float((tally.plant_area_cells(G) * (tally.hit > 0)).sum())
    assert abs(float(by_label[0]) - area_of_hit_cells) <= 1e-9 * want and by_label[1:].abs().sum() == 0
    assert abs(area_of_hit_cells - want) <= 1e-9 * want  # a cell without a hit has no area to share
    inner = (slice(1, -1),) * 3
    dens = float(tally.plant_area_density(G)[inner].nanmean())
    print(f"plant area {want:.3f} m2 in the grid; mean density of the inner cells {dens:.3f} m2/m3 (lambda / G = {LAMBDA / G:.3f})")


# -------------------------------------------------------------------------------------------------- surface ---
def test_the_derived_quantities_on_hand_made_tallies():
    g = OC.VoxelGrid((0, 0, 0), 0.5, (2, 2, 1))
    t = lambda rows: torch.tensor(rows, dtype=torch.int64).view(2, 2, 1)
    tally = OC.BeamTally(g, t([4, 2, 0, 0]), t([2, 0, 0, 0]), t([0, 1, 3, 0]), t([65536 * 2, 65536, 0, 0]), None, 0, 0)
    assert tally.state().view(-1).tolist() == [2, 1, 3, 0]
    att = tally.attenuation().view(-1)
    assert att[0].item() == 2.0 and att[1].item() == 0.0 and torch.isnan(att[2:]).all() and att.dtype == torch.float64
    assert torch.isnan(tally.attenuation(min_beams=3).view(-1)[1])
    assert tally.plant_area_density(0.5).view(-1)[0].item() == 4.0 and tally.plant_area(0.5) == 4.0 * 0.125
    hit_cell, labels = torch.tensor([0, 0, 0, -1, 1]), torch.tensor([1, 1, 0, 0, 2])
    np.testing.assert_allclose(tally.plant_area_by_label(hit_cell, labels, 3).tolist(), [0.5 / 3, 1.0 / 3, 0.0])
    assert OC.visibility_of_points(tally, torch.tensor([[0.1, 0.1, 0.1], [0.1, 0.6, 0.4], [0.6, 0.2, 0.2], [0.9, 0.9, 0.1], [2.0, 0, 0]])).tolist() == [2, 1, 3, 0, 0]
    around = OC.VoxelGrid.around(np.array([[0.0, 0, 0], [1.0, 0.55, 0.2], [np.nan, 0, 0]]), 0.5, margin=0.1)
    assert around.dim == (3, 2, 1) and np.allclose(around.lo, (-0.1, -0.1, -0.1))


def test_the_commands_round_trip(backend, tmp_path, capsys):
    from smart_tree_amd.synthetic import grow_tree
    from smart_tree_amd.util.file import save_skeleton_npz

    save_skeleton_npz(tmp_path / "sk.npz", S.tree_skeleton(grow_tree(30, 1.0, 2)))
    common = [f"skeleton={tmp_path / 'sk.npz'}", "scanners=2", "step_deg=0.6", "range_noise=0", f"device={backend}"]
    cloud = SC.main(common + [f"out={tmp_path / 'scan.npz'}", f"beams={tmp_path / 'b' / 'beams.npz'}"])
    without = SC.main(common + [f"out={tmp_path / 'scan2.npz'}"])
    assert torch.equal(cloud.xyz, without.xyz)
    with np.load(tmp_path / "b" / "beams.npz") as z:
        assert set(z.files) == {"origins", "origin_idx", "dir", "range"} and z["origins"].shape == (2, 3)
        assert int(np.isfinite(z["range"]).sum()) == len(cloud) and z["dir"].shape == (len(z["range"]), 3) and z["origin_idx"].max() == 1
    capsys.readouterr()
    tally = OC.main([f"beams={tmp_path / 'b' / 'beams.npz'}", f"out={tmp_path / 'occ'}", "cell=0.1", "max_range=inf", "behind=true", f"device={backend}"])
    text = capsys.readouterr().out
    with np.load(tmp_path / "occ" / "occupancy.npz") as z:
        assert set(z.files) == {"lo", "cell", "dim", "enter", "hit", "behind", "path", "state", "density"}
        dim = tuple(z["dim"].tolist())
        assert all(z[k].shape == dim for k in ("enter", "hit", "behind", "path", "state", "density")) and z["path"].dtype == np.uint64
        np.testing.assert_array_equal(z["enter"], tally.enter.cpu().numpy())
        counts = [int((z["state"] == k).sum()) for k in range(4)]
        assert int(z["hit"].sum()) >= 0.99 * len(cloud)
    printed = [int(re.search(rf"{name}: (\d+)", text).group(1)) for name in OC.STATES]
    assert printed == counts and sum(printed) == int(np.prod(dim)) and "plant area" in text
    OC.main([f"beams={tmp_path / 'b' / 'beams.npz'}", f"out={tmp_path / 'o2.npz'}", "cell=0.2", "margin=0.0", "max_range=5.5", "behind=false", f"device={backend}"])
    with np.load(tmp_path / "o2.npz") as z:
        assert z["behind"].sum() == 0 and z["enter"].sum() > 0
    with pytest.raises(SystemExit, match="usage"):
        OC.main(["beams=x.npz"])
    with pytest.raises(SystemExit, match="usage"):
        OC.main(["beams=x.npz", "out=y", "cells=3"])


def test_measure_trees_takes_a_leaf_area(backend, tmp_path):
    from smart_tree_amd import inventory as I

    cloud, (truth,) = S.generate_trees([3], 4000, foliage_fraction=0.0, noise=0.002, max_depth=2, device=backend)
    cloud.seg_off = None
    base = I.measure_trees(cloud, truth)
    none = I.measure_trees(cloud, truth, plant_area=None)
    base.save(tmp_path / "a")
    none.save(tmp_path / "b")
    for name in ("inventory.json", "trees.csv", "branches.csv"):
        assert (tmp_path / "a" / name).read_bytes() == (tmp_path / "b" / name).read_bytes()
    assert "leaf_area_m2" not in base.tree_columns
    with_area = I.measure_trees(cloud, truth, plant_area=torch.tensor([1.25], dtype=torch.float64))
    assert with_area.tree_columns == base.tree_columns + ("leaf_area_m2",) and with_area.column("leaf_area_m2").tolist() == [1.25]
    np.testing.assert_array_equal(with_area.trees[:, :-1], base.trees)
    with_area.save(tmp_path / "c")
    assert (tmp_path / "c" / "trees.csv").read_text().splitlines()[0].endswith(",leaf_area_m2")
    back = I.TreeInventory.load(tmp_path / "c")
    assert back.column("leaf_area_m2").tolist() == [1.25] and back.split()[0].tree_columns[-1] == "leaf_area_m2"
    with pytest.raises(ValueError, match="plant_area"):
        I.measure_trees(cloud, truth, plant_area=[1.0, 2.0])


def test_the_header_the_library_and_the_binding_agree(emu_lib):
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "smarttree_hip.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(st_[a-z0-9_]+)\s*\(", header))
    for name in ("st_beam_tally_seg", "st_beam_tally_workspace_bytes"):
        assert name in declared and name in _lib.SIGNATURES and hasattr(emu_lib, name)
    assert set(_lib.SIGNATURES) <= declared
    assert len(_lib.SIGNATURES["st_beam_tally_seg"][1]) == len(re.search(r"int st_beam_tally_seg\((.*?)\);", header, flags=re.S).group(1).split(","))
