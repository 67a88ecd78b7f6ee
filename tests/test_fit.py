"""Tube fits of a skeleton to its points (csrc/fit.hip, smart_tree_amd/refine.py).

The moments are compared bit for bit with tests/fit_oracle.py (a float32 numpy restatement of the frame, the pair and the
fixed-point terms), the solve with the oracle's float64 solve from the same integer moments.  The scenes reach every path of the
accumulation's LDS table: a handful of tubes per workgroup, every lane in the same slots, more tubes per workgroup than slots.
One oracle run per scene, shared and read-only.
"""
import functools

import numpy as np
import pytest
import torch

from smart_tree_amd import _lib
from smart_tree_amd import refine as R
from smart_tree_amd.data_types.branch import BranchSkeleton
from smart_tree_amd.data_types.cloud import Cloud
from smart_tree_amd.data_types.tree import DisjointTreeSkeleton, TreeSkeleton
from smart_tree_amd.data_types.flat import FlatSkeletons
from smart_tree_amd.evaluation import skeleton_tubes

import fit_oracle as fo
from segment_oracle import segment as oracle_segment

F = np.float32


def _t(x, dev, dtype=None):
    if x is None:
        return None
    return torch.from_numpy(np.array(x)).to(dev) if dtype is None else torch.as_tensor(np.array(x), dtype=dtype, device=dev)


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _run(dev, pts, tube, a, b, r1, r2, **kw):
    res = R.fit_tubes(_t(pts, dev), _t(tube, dev, torch.int32), _t(a, dev), _t(b, dev), _t(r1, dev), _t(r2, dev), moments=True, **kw)
    return res["moments"].cpu().numpy(), res["fit"].cpu().numpy()


# -------------------------------------------------------------------------------------------- scenes ---
def _chains(m, seed=0):
    """m tubes in chains like a skeleton's: a trunk (radius 0.4 m tapering to 0.1) and branches leaving it (<= 0.15 m down to 2 mm),
    segments of 1 to 5 cm."""
    rng = np.random.default_rng(seed)
    sizes = [m] if m <= 3 else [max(m // 5, 1)]
    while sum(sizes) < m:
        sizes.append(min(int(rng.integers(3, max(m // 12, 4) + 1)), m - sum(sizes)))
    a, b, r1, r2, trunk = [], [], [], [], None
    for c, k in enumerate(sizes):
        if c == 0:
            p, d, r_from = np.zeros(3), np.array([0.0, 1.0, 0.0]), 0.4
        else:
            p, d, r_from = trunk[rng.integers(len(trunk))], _unit(rng.normal(size=3)), float(rng.uniform(0.01, 0.15))
        pts = [p]
        for _ in range(k):
            d = _unit(d + 0.15 * rng.normal(size=3))
            pts.append(pts[-1] + d * rng.uniform(0.01, 0.05))
        pts = np.asarray(pts)
        rad = np.linspace(r_from, 0.1 if c == 0 else 0.002, k + 1)
        trunk = pts if c == 0 else trunk
        a.append(pts[:-1]); b.append(pts[1:]); r1.append(rad[:-1]); r2.append(rad[1:])
    return tuple(np.concatenate(x).astype(F) for x in (a, b, r1, r2))


def _surface_points(n, a, b, r1, r2, seed=0, which=None):
    """Points on and near the surfaces (within 10 % of the radius, a few up to twice the radius away), a little past the end caps
    too; returns (points, the tube each was drawn on)."""
    rng = np.random.default_rng(seed + 500)
    j = rng.integers(len(a), size=n) if which is None else which
    t = rng.uniform(-0.05, 1.05, size=(n, 1))
    q = a[j] + t * (b[j] - a[j])
    r = ((1 - t[:, 0]) * r1[j] + t[:, 0] * r2[j])[:, None]
    factor = np.where(rng.uniform(size=(n, 1)) < 0.9, rng.uniform(0.9, 1.1, size=(n, 1)), rng.uniform(0.0, 2.0, size=(n, 1)))
    ab = _unit((b[j] - a[j]).astype(np.float64))
    u = rng.normal(size=(n, 3))
    u = _unit(u - (u * ab).sum(1, keepdims=True) * ab)
    return (q + r * factor * u).astype(F), j.astype(np.int32)


@functools.lru_cache(maxsize=None)
def _scene(name):
    if name == "chains":  # the tubes by the segmentation, as the pipeline has them
        a, b, r1, r2 = _chains(37)
        pts, _ = _surface_points(4096, a, b, r1, r2)
        tube = oracle_segment(pts, a, b, r1, r2, check64=False)["tube"]
    elif name == "one_point":
        a, b, r1, r2 = _chains(1)
        pts, tube = _surface_points(1, a, b, r1, r2)
        pts = ((a[0] + b[0]) / 2 + np.array([r1[0], 0, 0], F)).reshape(1, 3).astype(F)
    elif name in ("one_tube", "three_tubes"):  # every lane of a workgroup in the same slots
        a, b, r1, r2 = _chains(1 if name == "one_tube" else 3, seed=4)
        pts, tube = _surface_points(20000, a, b, r1, r2)
    elif name == "many_tubes":  # ~1100 different tubes among the 2048 points of a workgroup: more than any table holds
        a, b, r1, r2 = _chains(1500, seed=2)
        pts, tube = _surface_points(6000, a, b, r1, r2)
    else:
        raise KeyError(name)
    out = (pts, tube.astype(np.int32), a, b, r1, r2)
    for x in out:
        x.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _scene_oracle(name, max_relative=0.5):
    mom, entered = fo.moments(*_scene(name), max_relative=max_relative)
    mom.setflags(write=False)
    return mom, entered


SCENES = ("chains", "one_point", "one_tube", "three_tubes", "many_tubes")


# ------------------------------------------------------------------------------------------ 1: moments ---
@pytest.mark.parametrize("name", SCENES)
def test_moments_equal_the_oracle(backend, name):
    scene = _scene(name)
    want, entered = _scene_oracle(name)
    mom, fit = _run(backend, *scene)
    np.testing.assert_array_equal(mom, want)
    assert mom[:, 0].sum() == entered.sum() and np.array_equal(fit[:, 0], mom[:, 0].astype(np.float64))
    if name != "one_point":  # the scene is not trivial: most points enter, some do not
        assert 0.5 * len(scene[0]) < entered.sum() < len(scene[0])
    if name == "many_tubes":
        assert (np.unique(scene[1][:2048]).size > 1000) and (mom[:, 0] > 0).sum() > 1000
    free, _ = _scene_oracle(name, -1.0)
    np.testing.assert_array_equal(_run(backend, *scene, max_relative=-1.0)[0], free)
    assert free[:, 0].sum() >= want[:, 0].sum()


def test_no_points_no_tubes(backend):
    pts, tube, a, b, r1, r2 = _scene("three_tubes")
    mom, fit = _run(backend, pts[:0], tube[:0], a, b, r1, r2)
    assert mom.shape == (3, 10) and fit.shape == (3, 8) and not mom.any() and not fit.any()
    mom, fit = _run(backend, pts, np.full(len(pts), -1, np.int32), a[:0], b[:0], r1[:0], r2[:0])
    assert mom.shape == (0, 10) and fit.shape == (0, 8)
    # n = 0 through the C call: outputs that held something are zeroed
    L = _lib.lib()
    m_dev = torch.full((3, 10), 77, dtype=torch.int64, device=backend)
    f_dev = torch.full((3, 8), 7.0, dtype=torch.float64, device=backend)
    ws = _lib.workspace(L.st_fit_tubes_workspace_bytes(0, 3), backend)
    ta, tb, t1, t2 = (_t(x, backend) for x in (a, b, r1, r2))
    _lib.check(L.st_fit_tubes(None, 0, None, _lib.ptr(ta), _lib.ptr(tb), _lib.ptr(t1), _lib.ptr(t2), 3, 0.5, 8, 0.01, _lib.ptr(m_dev),
                              _lib.ptr(f_dev), _lib.ptr(ws), ws.numel(), _lib.stream(backend)))
    assert not m_dev.cpu().numpy().any() and not f_dev.cpu().numpy().any()


# --------------------------------------------------------------------------------------- 2: who enters ---
def test_who_enters(backend):
    a = np.array([[0, 0, 0], [2, 2, 2]], F)
    b = np.array([[0, 0, 1], [2, 2, 2]], F)  # tube 1 has no length
    r = np.array([0.1, 0.1], F)
    pts = np.array([[0.1, 0, -1e-6],                          # 0: a hair before the first end cap
                    [0.1, 0, np.nextafter(F(1), F(2))],       # 1: a hair past the second
                    [0.1, 0, 0],                              # 2: q = 0 exactly
                    [0, 0.1, 1],                              # 3: q = 1 exactly
                    [0.1, 0, 0.5],                            # 4: no tube
                    [np.nan, 0, 0.5],                         # 5
                    [0.1, np.inf, 0.5],                       # 6
                    [2.1, 2, 2],                              # 7: on the zero-length tube
                    [0, 0, 0.5],                              # 8: on the axis
                    [0.125, 0, 0.5],                          # 9: |res| / r = 0.25
                    [1, 0, 0.5],                              # 10: far away
                    [0.1, 0, 0.5]], F)                        # 11: a tube index beyond the tubes
    tube = np.array([0, 0, 0, 0, -1, 0, 0, 1, 0, 0, 0, 5], np.int32)
    ratio = abs(float(F(0.125) - F(0.1))) / float(F(0.1))
    cases = {0.5: [2, 3, 9], ratio * (1 - 1e-4): [2, 3], ratio * (1 + 1e-4): [2, 3, 9], -1.0: [2, 3, 9, 10], 0.0: [2, 3]}
    for mr, inside in cases.items():
        want, entered = fo.moments(pts, tube, a, b, r, r, max_relative=mr)
        assert np.flatnonzero(entered).tolist() == inside, mr  # the oracle against the hand count
        mom, fit = _run(backend, pts, tube, a, b, r, r, max_relative=mr)
        np.testing.assert_array_equal(mom, want)
        assert mom[:, 0].tolist() == [len(inside), 0] and not mom[1].any()
    # the terms of one point by hand: tube 0 along z, k = 0, e1 = +y, e2 = -x; the point on +x has c = 0, s = -1, rho = 0.125
    mom, _ = _run(backend, pts[9:10], tube[9:10], a, b, r, r)
    one, rho = 1 << 24, 0.125 * (1 << 24)
    assert mom[0].tolist() == [1, 0, 0, one, 0, -one, 0, -rho, rho, rho / 8]


# --------------------------------------------------------------------------------------------- 3: solve ---
def _cylinder(n, arc_deg, radius=0.1, length=0.05, seed=0, centre_deg=0.0):
    """One tube a -> b (tilted, away from the origin) and n exact points of its surface over an arc around the direction
    `centre_deg` of the tube's own frame.  Returns (points, a, b, e1, e2) -- the frame as the contract forms it."""
    a = np.array([[0.3, -0.2, 1.0]], F)
    b = (a + _unit(np.array([1.0, 2.0, 3.0])) * length).astype(F)
    _, e1, e2 = fo.frames(a, b)
    rng = np.random.default_rng(seed)
    th = np.deg2rad(centre_deg) + np.deg2rad(arc_deg) * (rng.uniform(size=n) - 0.5)
    t = rng.uniform(0.02, 0.98, size=n)
    a64, ab = a[0].astype(np.float64), (b[0] - a[0]).astype(np.float64)
    p = a64 + t[:, None] * ab + radius * (np.cos(th)[:, None] * e1[0].astype(np.float64) + np.sin(th)[:, None] * e2[0].astype(np.float64))
    return p.astype(F), a, b, e1[0].astype(np.float64), e2[0].astype(np.float64)


def _assert_solve(mom, fit, a, b, **kw):
    want = fo.solve(mom, a, b, **kw)
    np.testing.assert_array_equal(fit[:, 0], want[:, 0])
    np.testing.assert_array_equal(fit[:, 7], want[:, 7])
    np.testing.assert_allclose(fit[:, 1:6], want[:, 1:6], rtol=0, atol=1e-9)
    np.testing.assert_allclose(fit[:, 6], want[:, 6], rtol=0, atol=1e-9)
    return want


@pytest.mark.parametrize("name", SCENES)
def test_solve_equals_the_float64_oracle(backend, name):
    scene = _scene(name)
    mom, fit = _run(backend, *scene)
    want = _assert_solve(mom, fit, scene[2], scene[3])
    if name == "chains":
        assert (want[:, 7] == 2).sum() > 20 and np.isin(want[:, 7], [0, 1, 2]).all()
    mom, fit = _run(backend, *scene, min_points=1, min_spread=0.2)
    _assert_solve(mom, fit, scene[2], scene[3], min_points=1, min_spread=0.2)


def test_solve_reaches_every_status(backend):
    """Three tubes in one call: a full ring (2), a 60 degree arc (1), five points (0)."""
    ring, a, b, _, _ = _cylinder(400, 360.0)
    arc = _cylinder(400, 60.0, seed=1)[0]
    few = _cylinder(5, 360.0, seed=2)[0]
    pts = np.concatenate([ring, arc, few])
    tube = np.repeat(np.arange(3, dtype=np.int32), [400, 400, 5])
    a3, b3 = np.tile(a, (3, 1)), np.tile(b, (3, 1))
    r = np.full(3, 0.1, F)
    mom, fit = _run(backend, pts, tube, a3, b3, r, r)
    np.testing.assert_array_equal(mom, fo.moments(pts, tube, a3, b3, r, r)[0])
    _assert_solve(mom, fit, a3, b3)
    assert fit[:, 7].tolist() == [2.0, 1.0, 0.0] and fit[:, 0].tolist() == [400.0, 400.0, 5.0]
    assert abs(fit[0, 1] - 0.1) < 1e-6 and np.abs(fit[0, 2:5]).max() < 1e-6 and fit[0, 5] < 1e-6 and abs(fit[0, 6] - 0.5) < 0.05
    assert not fit[2, 1:].any()


# ----------------------------------------------------------------------------------- 4: known cylinders ---
def _one_tube_skeleton(a, b, radius):
    xyz = torch.from_numpy(np.stack([a, b]).astype(F))
    return TreeSkeleton(0, {0: BranchSkeleton(0, -1, xyz, torch.full((2, 1), radius, dtype=torch.float32))})


@pytest.mark.parametrize("arc", [360.0, 180.0, 120.0, 100.0])
def test_known_cylinder_is_recovered(backend, arc):
    """Radius 0.1 m, length 0.05 m, 400 exact surface points; the predicted axis displaced by (0.03, -0.02) m in the tube's frame,
    the predicted radius 0.13 m.  The arc is centred on the frame's first direction."""
    pts, a, b, e1, e2 = _cylinder(400, arc)
    shift = (0.03 * e1 - 0.02 * e2)
    guess = _one_tube_skeleton(a[0].astype(np.float64) + shift, b[0].astype(np.float64) + shift, 0.13)
    refined, fit = R.refine_skeleton(_t(pts, backend), guess, iterations=3, max_relative=-1.0)
    assert fit.tubes[0, 7] == 2 and fit.tubes[0, 0] == 400
    br = refined.skeletons[0].branches[0]
    radius_error = np.abs(br.radii.numpy().reshape(-1).astype(np.float64) - 0.1).max() / 0.1
    d = br.xyz.numpy().astype(np.float64) - a[0].astype(np.float64)
    axis = _unit((b[0] - a[0]).astype(np.float64))
    axis_error = np.linalg.norm(d - (d @ axis)[:, None] * axis, axis=1).max() / 0.1
    print(f"arc {arc}: radius error {radius_error:.3g}, axis error {axis_error:.3g} (of the radius)")
    assert radius_error <= 1e-4 and axis_error <= 1e-4


def test_narrow_arc_and_few_points(backend):
    pts, a, b, e1, e2 = _cylinder(400, 60.0)
    shift = (0.03 * e1 - 0.02 * e2)
    ga, gb = (a + shift).astype(F), (b + shift).astype(F)
    r = np.full(1, 0.13, F)
    tube = np.zeros(400, np.int32)
    mom, fit = _run(backend, pts, tube, ga, gb, r, r, max_relative=-1.0)
    assert fit[0, 7] == 1 and fit[0, 0] == 400 and fit[0, 6] < 0.01
    assert fit[0, 1] == mom[0, 8] / 2.0 ** 24 / 400 and not fit[0, 2:5].any()
    mom, fit = _run(backend, pts[:7], tube[:7], ga, gb, r, r, max_relative=-1.0)
    assert fit[0, 7] == 0 and fit[0, 0] == 7 and mom[0, 0] == 7 and not fit[0, 1:].any()


# --------------------------------------------------------------------------------------- 5: update rules ---
def _two_branches():
    """A trunk of four vertices along y (tubes 0..2) and a child of three along x leaving vertex 2 (tubes 3, 4)."""
    trunk = BranchSkeleton(0, -1, torch.tensor([[0, 0, 0], [0, 1, 0], [0, 2, 0], [0, 3, 0]], dtype=torch.float32),
                           torch.tensor([[0.2], [0.2], [0.2], [0.1]]))
    child = BranchSkeleton(1, 0, torch.tensor([[0, 2, 0], [1, 2, 0], [2, 2, 0]], dtype=torch.float32), torch.tensor([[0.05], [0.05], [0.05]]))
    child.radii = child.radii.reshape(-1)  # as `smooth` leaves them
    return DisjointTreeSkeleton([TreeSkeleton(0, {0: trunk, 1: child})])


class _FitTable(FlatSkeletons):
    """The table as `refine_skeleton` works on it: float32 vertices and the links of every vertex to its tubes."""

    def __init__(self, skeletons):
        super().__init__(skeletons)
        self.xyz, self.radii = self.float32()
        self.links = R.vertex_links(self)
        self.lo, self.hi, self.pinned = self.links


def _rows(*rows):
    """fit rows (N, R, offset, status) -> [m,8]."""
    out = np.zeros((len(rows), 8))
    for k, (n, radius, off, status) in enumerate(rows):
        out[k, 0], out[k, 1], out[k, 2:5], out[k, 7] = n, radius, off, status
    return out


def test_update_rules():
    sk = _two_branches()
    flat = _FitTable([sk])
    assert flat.lo.tolist() == [-1, 0, 1, 2, -1, 3, 4] and flat.hi.tolist() == [0, 1, 2, -1, 3, 4, -1]
    assert flat.pinned.tolist() == [False, False, False, False, True, False, False] and flat.tube_off.tolist() == [0, 5]
    fit = _rows((30, 0.22, (0.01, 0, 0), 2),      # tube 0
                (10, 0.18, (0.05, 0, 0), 2),      # tube 1
                (50, 0.90, (0, 0, 0), 1),         # tube 2: radius only, far above the prior
                (20, 0.06, (0, 0, 0.5), 2),       # tube 3: an offset ten times the radius
                (5, 0.01, (0, 0.3, 0), 0))        # tube 4: not fitted
    xyz, radii = R.update_vertices(flat.links, flat.xyz, flat.radii, flat.xyz, flat.radii, fit)
    assert xyz.dtype == F and radii.dtype == F
    # vertex 0: tube 0 alone.  vertex 1: the weighted mean of tubes 0 and 1
    assert radii[0] == F(0.22) and np.allclose(xyz[0], [0.01, 0, 0])
    assert radii[1] == F((30 * 0.22 + 10 * 0.18) / 40) and np.allclose(xyz[1], [(30 * 0.01 + 10 * 0.05) / 40, 1, 0])
    # vertex 2: radii of tubes 1 and 2 -> (10 * 0.18 + 50 * 0.9) / 60 = 0.78, clamped to 2 x 0.2; only tube 1 moves it
    assert radii[2] == F(0.4) and np.allclose(xyz[2], [0.05, 2, 0])
    # vertex 3: tube 2 alone, 0.9 clamped to 2 x 0.1; radius only: it stays where it is
    assert radii[3] == F(0.2) and xyz[3].tolist() == [0, 3, 0]
    # vertex 4, the child's first: the radius follows tube 3, the position is the connection point
    assert radii[4] == F(0.06) and xyz[4].tolist() == [0, 2, 0]
    # vertex 5: tubes 3 (fitted) and 4 (not): tube 3 alone; the move of 0.5 is cut to the prior radius
    assert radii[5] == F(0.06) and np.allclose(xyz[5], [1, 2, 0.05])
    # vertex 6: no fitted tube
    assert radii[6] == F(0.05) and xyz[6].tolist() == [2, 2, 0]
    # downwards: the clamp at prior / max_ratio; another ratio; move_axis off
    low = R.update_vertices(flat.links, flat.xyz, flat.radii, flat.xyz, flat.radii, _rows((9, 0.01, (0, 0, 0), 1), *[(0, 0, (0, 0, 0), 0)] * 4))
    assert low[1][0] == F(0.1) and low[1][1] == F(0.1) and low[1][2] == F(0.2)
    wide = R.update_vertices(flat.links, flat.xyz, flat.radii, flat.xyz, flat.radii, fit, max_ratio=10.0)
    assert wide[1][3] == F(0.9) and wide[1][2] == F(0.78)
    still = R.update_vertices(flat.links, flat.xyz, flat.radii, flat.xyz, flat.radii, fit, move_axis=False)
    assert np.array_equal(still[0], flat.xyz) and np.array_equal(still[1], radii)
    # the limits hold against the PRIOR over several rounds: a second update from the moved state cannot leave the prior's reach
    again = R.update_vertices(flat.links, xyz, radii, flat.xyz, flat.radii, fit)
    assert np.linalg.norm(again[0] - flat.xyz, axis=1).max() <= flat.radii.max() + 1e-6 and np.allclose(again[0][5], [1, 2, 0.05])
    assert again[1][2] == F(0.4)


def test_refine_keeps_the_structure_and_the_input(backend):
    sk = _two_branches()
    a, b, r1, r2 = (t.numpy() for t in skeleton_tubes(sk))
    pts, _ = _surface_points(3000, a, b, r1 * F(1.1), r2 * F(1.1), seed=3)
    before = [(k, br.parent_id, br.xyz.clone(), br.radii.clone()) for k, br in sk.skeletons[0].branches.items()]
    refined, fit = R.refine_skeleton(_t(pts, backend), sk, iterations=2)
    for k, parent, xyz, radii in before:  # the input's tensors are untouched
        br = sk.skeletons[0].branches[k]
        assert torch.equal(br.xyz, xyz) and torch.equal(br.radii, radii) and br.radii.shape == radii.shape
    assert isinstance(refined, DisjointTreeSkeleton) and len(refined.skeletons) == 1 and refined.skeletons[0]._id == 0
    got = refined.skeletons[0].branches
    assert list(got.keys()) == [0, 1] and [got[k].parent_id for k in got] == [-1, 0] and [len(got[k]) for k in got] == [4, 3]
    assert got[0].radii.shape == (4, 1) and got[1].radii.shape == (3,) and got[0].xyz.dtype == torch.float32
    assert torch.equal(got[1].xyz[0], sk.skeletons[0].branches[1].xyz[0])  # the connection point
    assert not torch.equal(got[0].radii, sk.skeletons[0].branches[0].radii)  # and something was fitted: the points sit 10 % out
    assert fit.tubes.shape == (5, 8) and fit.branches.shape == (2, 9) and fit.branches[:, 4].tolist() == [3, 2]
    assert fit.branches[:, :4].tolist() == [[0, 0, 0, -1], [0, 0, 1, 0]] and fit.branches[0, 8] > 0.03
    # the kinds of skeleton a caller may hold give the same answer; no iterations: the input's copy
    flat = {"branches": np.array([[0, 0, -1, 0, 4], [0, 1, 0, 4, 3]]), "xyz": np.concatenate([b.xyz.numpy() for b in sk.skeletons[0].branches.values()]),
            "radii": np.concatenate([b.radii.numpy().reshape(-1) for b in sk.skeletons[0].branches.values()])}
    for other in (sk.skeletons[0], flat):
        again, _ = R.refine_skeleton(Cloud(xyz=_t(pts, backend)), other)
        assert _sig(again) == _sig(refined)
    same, none = R.refine_skeleton(_t(pts, backend), sk, iterations=0)
    assert _sig(same) == _sig(sk) and none.tubes.shape == (5, 8) and not none.tubes.any()
    with pytest.raises(ValueError):
        R.refine_skeleton(_t(pts, backend), [sk, sk])
    with pytest.raises(ValueError):
        R.refine_skeleton(_t(pts, backend), sk, max_ratio=0.5)


def _sig(sk):
    return [(t._id, b._id, b.parent_id, b.xyz.numpy().tobytes(), b.radii.numpy().reshape(-1).tobytes()) for t in sk.skeletons for b in t.branches.values()]


# ------------------------------------------------------------------------------------------ 6: same bits ---
def _subdivide(tree: TreeSkeleton, step=0.1) -> TreeSkeleton:
    """The same cones cut into tubes of at most `step`: the radius of a cone is linear along it, so the cut is exact."""
    out = {}
    for k, br in tree.branches.items():
        xyz, rad = br.xyz.numpy().astype(np.float64), br.radii.numpy().reshape(-1).astype(np.float64)
        px, pr = [xyz[:1]], [rad[:1]]
        for i in range(len(xyz) - 1):
            pieces = max(int(np.ceil(np.linalg.norm(xyz[i + 1] - xyz[i]) / step)), 1)
            t = np.arange(1, pieces + 1)[:, None] / pieces
            px.append(xyz[i] + t * (xyz[i + 1] - xyz[i]))
            pr.append(rad[i] + t[:, 0] * (rad[i + 1] - rad[i]))
        out[k] = BranchSkeleton(k, br.parent_id, torch.from_numpy(np.concatenate(px).astype(F)), torch.from_numpy(np.concatenate(pr).astype(F)).reshape(-1, 1))
    return TreeSkeleton(tree._id, out)


def _perturb(tree: TreeSkeleton) -> TreeSkeleton:
    """Every radius times a smooth factor within +-20 %; every vertex but a branch's first moved sideways by 0.2 of its radius."""
    out = {}
    for k, br in tree.branches.items():
        xyz, rad = br.xyz.numpy().astype(np.float64), br.radii.numpy().reshape(-1).astype(np.float64)
        s = np.concatenate([[0.0], np.cumsum(np.linalg.norm(np.diff(xyz, axis=0), axis=1))])
        factor = 1.0 + 0.2 * np.sin(2.0 * s + 0.7 * k)
        d = _unit(np.gradient(xyz, axis=0) + 1e-12)
        side = _unit(np.cross(d, np.where(np.abs(d[:, [1]]) < 0.9, [[0.0, 1.0, 0.0]], [[1.0, 0.0, 0.0]])))
        turn = np.cos(3.0 * s + k)[:, None] * side + np.sin(3.0 * s + k)[:, None] * np.cross(d, side)
        moved = xyz + 0.2 * rad[:, None] * turn
        moved[0] = xyz[0]
        out[k] = BranchSkeleton(k, br.parent_id, torch.from_numpy(moved.astype(F)), torch.from_numpy((rad * factor).astype(F)).reshape(-1, 1))
    return TreeSkeleton(tree._id, out)


TRUTH_SEEDS = (3, 11)




@functools.lru_cache(maxsize=None)
def _truth_case(seed, device, n=20000):
    """(points [n,3], the ground-truth skeleton in 10 cm tubes, its perturbed copy) of one generated tree."""
    from smart_tree_amd.dataset.synthetic import generate_trees

    cloud, (truth,) = generate_trees([seed], n, foliage_fraction=0.0, noise=0.002, max_depth=2, device=torch.device(device))
    truth = _subdivide(truth)
    xyz = cloud.xyz.cpu().numpy().copy()
    xyz.setflags(write=False)
    return xyz, truth, _perturb(truth)


def test_two_runs_are_bit_identical(backend):
    for name in ("chains", "many_tubes", "one_tube"):
        (m0, f0), (m1, f1) = _run(backend, *_scene(name)), _run(backend, *_scene(name))
        np.testing.assert_array_equal(m0, m1)
        np.testing.assert_array_equal(f0.view(np.uint64), f1.view(np.uint64))


def test_forms_upstream_give_the_same_skeleton(backend):
    xyz, _, guess = _truth_case(TRUTH_SEEDS[0], str(backend))
    pts = _t(xyz[:6000], backend)
    dense, fd = R.refine_skeleton(pts, guess, form="dense")
    grid, fg = R.refine_skeleton(pts, guess, form="grid")
    assert _sig(dense) == _sig(grid) and _sig(dense) != _sig(DisjointTreeSkeleton([guess]))
    np.testing.assert_array_equal(fd.tubes.view(np.uint64), fg.tubes.view(np.uint64))
    again, _ = R.refine_skeleton(pts, guess, form="dense")
    assert _sig(again) == _sig(dense)


def test_batch_equals_the_single_calls(backend):
    cases = [_truth_case(s, str(backend)) for s in TRUTH_SEEDS]
    clouds = [Cloud(xyz=_t(cases[0][0][:5000], backend)), Cloud(xyz=_t(cases[1][0][:700], backend)), Cloud(xyz=_t(cases[1][0][:3001], backend))]
    skeletons = [cases[0][2], DisjointTreeSkeleton([TreeSkeleton(0, {})]), DisjointTreeSkeleton([cases[1][2]])]
    singles = [R.refine_skeleton(c, s) for c, s in zip(clouds, skeletons)]
    batch, fit = R.refine_skeleton(Cloud.collate(clouds), skeletons)
    assert isinstance(batch, list) and len(batch) == 3 and len(fit.tube_off) == 4 and fit.tube_off[1] == fit.tube_off[2]
    for (one, one_fit), got, got_fit in zip(singles, batch, fit.split()):
        assert _sig(got) == _sig(one)
        np.testing.assert_array_equal(got_fit.tubes.view(np.uint64), one_fit.tubes.view(np.uint64))
        np.testing.assert_array_equal(got_fit.branches.view(np.uint64), one_fit.branches.view(np.uint64))
    assert len(batch[1].skeletons) == 1 and not batch[1].skeletons[0].branches and (fit.tubes[:, 7] == 2).sum() > 50
    assert sorted(set(fit.branches[:, 0])) == [0, 2]


def test_fit_report_round_trips(backend, tmp_path):
    xyz, _, guess = _truth_case(TRUTH_SEEDS[0], str(backend))
    _, fit = R.refine_skeleton(_t(xyz[:4000], backend), guess, iterations=1)
    fit.save(tmp_path / "deep" / "skeleton_fit.npz")
    back = R.SkeletonFit.load(tmp_path / "deep" / "skeleton_fit.npz")
    np.testing.assert_array_equal(back.tubes.view(np.uint64), fit.tubes.view(np.uint64))
    np.testing.assert_array_equal(back.branches.view(np.uint64), fit.branches.view(np.uint64))
    assert back.tube_off.tolist() == fit.tube_off.tolist() and back.iterations == 1
    # the branch table against its definition
    rows = np.repeat(np.arange(len(fit.branches)), fit.branches[:, 4].astype(int))
    fitted = fit.tubes[:, 7] >= 1
    assert fit.branches[:, 5].tolist() == np.bincount(rows[fitted], minlength=len(fit.branches)).tolist()
    assert fit.branches[:, 6].sum() == fit.tubes[fitted, 0].sum() > 1000
    text = R.summary(fit)
    assert "full fit" in text and "points used: %d" % int(fit.tubes[fitted, 0].sum()) in text and "mean relative radius change" in text


# ------------------------------------------------------------------------------- 7: against ground truth ---
def _oracle_refine(xyz, skeleton, iterations=2):
    """refine_skeleton with the two oracles in the kernels' places (the vertex update is host code either way)."""
    flat = _FitTable([skeleton])
    cur_xyz, cur_r, fit = flat.xyz.copy(), flat.radii.copy(), None
    for _ in range(iterations):
        a, b, r1, r2 = flat.tubes(cur_xyz, cur_r)
        tube = oracle_segment(xyz, a, b, r1, r2, check64=False)["tube"]
        fit = fo.fit(xyz, tube, a, b, r1, r2)[1]
        cur_xyz, cur_r = R.update_vertices(flat.links, cur_xyz, cur_r, flat.xyz, flat.radii, fit)
    return cur_xyz, cur_r, fit


def _errors(truth, xyz, radii, fit):
    """Over the vertices of true radius >= 0.02 m that touch a fully fitted tube: (median relative radius error, median distance
    from the true axis in true radii, the share of the >= 0.02 m vertices these are)."""
    flat = _FitTable([truth])
    status = np.concatenate([fit[:, 7], [0.0]])
    touched = (status[flat.lo] == 2) | (status[flat.hi] == 2)
    big = flat.radii >= 0.02
    sel = touched & big
    true_xyz, true_r = flat.xyz.astype(np.float64), flat.radii.astype(np.float64)
    d = np.zeros_like(true_xyz)
    for _, _, _, _, o, n in flat.rows.tolist():
        d[o:o + n] = _unit(np.gradient(true_xyz[o:o + n], axis=0))
    off = xyz.astype(np.float64) - true_xyz
    side = np.linalg.norm(off - (off * d).sum(1, keepdims=True) * d, axis=1)
    return (float(np.median(np.abs(radii[sel] - true_r[sel]) / true_r[sel])), float(np.median(side[sel] / true_r[sel])),
            float(sel.sum()) / float(big.sum()))


@pytest.mark.parametrize("seed", TRUTH_SEEDS)
def test_refinement_approaches_the_ground_truth(backend, seed):
    """Measured, the kernels and the oracle pipeline alike: seed 3 (147 tubes) radius error 0.1299 -> 0.0099, axis distance 0.2000 ->
    0.0116 radii, 92 % of the vertices; seed 11 (209 tubes) 0.1371 -> 0.0102, 0.2000 -> 0.0112, 90 %."""
    xyz, truth, guess = _truth_case(seed, str(backend))
    start = _FitTable([guess])
    o_xyz, o_r, o_fit = _oracle_refine(xyz, guess)
    refined, fit = R.refine_skeleton(_t(xyz, backend), guess, iterations=2)
    got = _FitTable([refined])
    before = _errors(truth, start.xyz, start.radii, fit.tubes)
    after = _errors(truth, got.xyz, got.radii, fit.tubes)
    o_before = _errors(truth, start.xyz, start.radii, o_fit)
    o_after = _errors(truth, o_xyz, o_r, o_fit)
    print(f"seed {seed}: {len(fit.tubes)} tubes, radius error {before[0]:.4f} -> {after[0]:.4f} (oracle {o_before[0]:.4f} -> {o_after[0]:.4f}), "
          f"axis distance {before[1]:.4f} -> {after[1]:.4f} radii (oracle {o_before[1]:.4f} -> {o_after[1]:.4f}), "
          f"share of vertices {after[2]:.3f} (oracle {o_after[2]:.3f})")
    assert o_after[2] >= 0.5 and after[2] >= 0.5
    assert after[0] < before[0] and after[1] < before[1] and o_after[0] < o_before[0] and o_after[1] < o_before[1]
    assert 0.5 * o_after[0] <= after[0] <= 2.0 * o_after[0] and 0.5 * o_after[1] <= after[1] <= 2.0 * o_after[1]


# ------------------------------------------------------------------------------------------ 8: refusals ---
def test_refusals(backend):
    L = _lib.lib()
    pts, tube, a, b, r1, r2 = _scene("three_tubes")
    n = 512
    tp, tt, ta, tb, t1, t2 = _t(pts[:n], backend), _t(tube[:n], backend), _t(a, backend), _t(b, backend), _t(r1, backend), _t(r2, backend)
    mom = torch.full((3, 10), -7, dtype=torch.int64, device=backend)
    fit = torch.full((3, 8), -7.0, dtype=torch.float64, device=backend)
    ws = _lib.workspace(L.st_fit_tubes_workspace_bytes(n, 3), backend)

    def call(n=n, m=3, mr=0.5, ms=0.01, ws_bytes=None, pts=tp):
        return L.st_fit_tubes(_lib.ptr(pts), n, _lib.ptr(tt), _lib.ptr(ta), _lib.ptr(tb), _lib.ptr(t1), _lib.ptr(t2), m, mr, 8, ms,
                              _lib.ptr(mom), _lib.ptr(fit), _lib.ptr(ws), ws.numel() if ws_bytes is None else ws_bytes, _lib.stream(backend))

    cases = {"points": dict(n=1 << 31), "negative points": dict(n=-1), "tubes": dict(m=1 << 31), "negative tubes": dict(m=-1),
             "nan max_relative": dict(mr=float("nan")), "nan min_spread": dict(ms=float("nan")), "no points array": dict(pts=None),
             "workspace": dict(ws_bytes=64)}
    for what, kw in cases.items():
        rc = call(**kw)
        assert rc == (-2 if what == "workspace" else -1), what
        text = L.st_last_error().decode()
        assert text.startswith("fit_tubes:") and len(text) > 20, what
    assert "workspace too small" in L.st_last_error().decode()
    assert (mom.cpu().numpy() == -7).all() and (fit.cpu().numpy() == -7).all()  # nothing was launched, nothing written
    assert L.st_fit_tubes_workspace_bytes(1 << 31, 3) == -1 and L.st_fit_tubes_workspace_bytes(5, -1) == -1
    assert L.st_fit_tubes_workspace_bytes(0, 0) >= 0
    assert call() == 0 and mom.cpu().numpy()[:, 0].sum() > 0 and L.st_version() >= 113
    with pytest.raises(_lib.StError, match="max_relative is NaN"):
        R.fit_tubes(tp, tt, ta, tb, t1, t2, max_relative=float("nan"))
    with pytest.raises(ValueError):
        R.fit_tubes(tp, tt[:5], ta, tb, t1, t2)


# ------------------------------------------------------------------------------------------ 9: Pipeline ---
def _pipeline(device, **kw):
    from pathlib import Path

    from smart_tree_amd.dataset.augmentations import AugmentationPipeline, CentreCloud
    from smart_tree_amd.model.model_inference import ModelInference
    from smart_tree_amd.pipeline import Pipeline
    from smart_tree_amd.skeleton.skeletonize import Skeletonizer

    weights = Path(__file__).resolve().parents[1] / "smart_tree_amd" / "model" / "weights" / "noble-elevator-58.npz"
    mi = ModelInference("unused_model.pt", weights, voxel_size=0.03, block_size=4, buffer_size=0.4, device=device)
    if device.type == "cpu":
        mi.model.use_mfma = False
    sk = Skeletonizer(K=16, min_connection_length=0.02, minimum_graph_vertices=32, device=device)
    sk.block_threads = 128 if device.type == "cpu" else 0
    return Pipeline(AugmentationPipeline([CentreCloud()]), mi, sk, device=device, prune_skeletons=True, min_skeleton_radius=0.01,
                    min_skeleton_length=0.02, repair_skeletons=True, smooth_skeletons=True, smooth_kernel_size=11, **kw)


def _pipeline_case(dev, tmp_path, capsys):
    from smart_tree_amd.synthetic import sample_tree_cloud
    from smart_tree_amd.util.file import save_cloud, save_skeleton_npz

    def cloud(seed, n):
        c = sample_tree_cloud(n, seed=seed, scale=0.5, max_depth=3)
        return Cloud(xyz=torch.from_numpy(c["xyz"]), rgb=torch.from_numpy(c["rgb"]))

    plain = _pipeline(dev)
    raw = plain.process_cloud(cloud=cloud(2, 6000))
    assert plain.last_fit is None and plain.last_raw_skeleton is None
    pipe = _pipeline(dev, refine_skeletons=True, save_outputs=True, save_path=tmp_path / "out")
    np.random.seed(5)
    refined = pipe.process_cloud(cloud=cloud(2, 6000))
    # the raw skeleton is the one the pipeline gives with the flag off; the refined one is refine_skeleton on the wood points
    assert _sig(pipe.last_raw_skeleton) == _sig(raw) and sum(len(t.branches) for t in raw.skeletons) >= 1
    wood = pipe.last_labelled_cloud.filter_by_class(pipe.branch_classes)
    want, want_fit = R.refine_skeleton(wood, pipe.last_raw_skeleton, iterations=2, max_relative=0.5, device=dev)
    assert _sig(refined) == _sig(want) and _sig(refined) != _sig(raw)
    np.testing.assert_array_equal(pipe.last_fit.tubes.view(np.uint64), want_fit.tubes.view(np.uint64))
    assert (pipe.last_fit.tubes[:, 7] >= 1).any()
    saved = R.SkeletonFit.load(tmp_path / "out" / "skeleton_fit.npz")
    np.testing.assert_array_equal(saved.tubes.view(np.uint64), want_fit.tubes.view(np.uint64))
    from smart_tree_amd.evaluate import load_any_skeleton
    flat = _FitTable([load_any_skeleton(tmp_path / "out" / "skeleton.npz")])  # what was saved is the refined skeleton
    got = _FitTable([refined])
    assert np.array_equal(flat.xyz, got.xyz) and np.array_equal(flat.radii, got.radii)
    # other settings reach the call
    pipe.refine_iterations, pipe.refine_max_relative, pipe.save_outputs = 1, 0.2, False
    other = pipe.process_cloud(cloud=cloud(2, 6000))
    assert _sig(other) == _sig(R.refine_skeleton(wood, raw, iterations=1, max_relative=0.2, device=dev)[0]) != _sig(refined)
    pipe.refine_iterations, pipe.refine_max_relative = 2, 0.5
    # a batch of two equals the single calls
    singles, fits = [refined], [pipe.last_fit]
    singles.append(pipe.process_cloud(cloud=cloud(7, 5000)))
    fits.append(pipe.last_fit)
    fits[0] = want_fit
    parts = pipe.process_clouds([cloud(2, 6000), cloud(7, 5000)])
    assert len(parts) == 2 and isinstance(pipe.last_raw_skeleton, list)
    for one, one_fit, part, part_fit in zip(singles, fits, parts, pipe.last_fit.split()):
        assert _sig(part) == _sig(one)
        np.testing.assert_array_equal(part_fit.tubes.view(np.uint64), one_fit.tubes.view(np.uint64))
    # the command line on a saved cloud and skeleton
    save_cloud(tmp_path / "wood.npz", wood)
    save_skeleton_npz(tmp_path / "raw.npz", raw)
    capsys.readouterr()
    cli, cli_fit = R.main([f"cloud={tmp_path / 'wood.npz'}", f"skeleton={tmp_path / 'raw.npz'}", f"out={tmp_path / 'cli'}", f"device={dev}"])
    assert _sig(cli) == _sig(refined)
    np.testing.assert_array_equal(cli_fit.tubes.view(np.uint64), want_fit.tubes.view(np.uint64))
    assert sorted(p.name for p in (tmp_path / "cli").iterdir()) == ["skeleton.npz", "skeleton_fit.npz"]
    back = _FitTable([load_any_skeleton(tmp_path / "cli" / "skeleton.npz")])
    assert np.array_equal(back.xyz, got.xyz) and np.array_equal(back.radii, got.radii)
    text = capsys.readouterr().out
    assert "full fit" in text and "points used:" in text and "mean relative radius change:" in text
    R.main([f"cloud={tmp_path / 'wood.npz'}", f"skeleton={tmp_path / 'raw.npz'}", f"out={tmp_path / 'one.npz'}", "iterations=1", "max_relative=0.2",
            "classes=[0]", f"device={dev}"])
    one = _FitTable([load_any_skeleton(tmp_path / "one.npz")])
    assert np.array_equal(one.xyz, _FitTable([other]).xyz)
    with pytest.raises(SystemExit):
        R.main(["cloud=x.npz"])


@pytest.mark.gpu
def test_pipeline_refines_its_skeleton(tmp_path, capsys, monkeypatch):
    assert torch.cuda.is_available(), "gpu-marked test needs a GPU"
    monkeypatch.setattr(_lib, "_LIB", None)
    _lib.lib()
    _pipeline_case(torch.device("cuda:0"), tmp_path, capsys)
