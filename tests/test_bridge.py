"""Bridging components across gaps (csrc/bridge.hip, skeleton.graph.bridge_components, Skeletonizer(connect_components=True)).

The definition is exact, and so is every comparison here.  Candidates are the vertex pairs in different kept components of one
cloud with d2 = (dx*dx + dy*dy) + dz*dz <= max_gap^2, everything float32; the bridges are the minimum spanning forest of the
component graph under the strict total order (bits of d2, lo, hi).  The reference below brute-forces every pair in numpy float32
and runs Kruskal with a union-find under that order.  Edge sets are compared for equality and the weights bit for bit.

Kernel-level inputs are hand-made graphs: sticks of vertices 0.01 apart, chained by explicit edges and pushed through
connected_components, so component membership is known by construction.  One run per case (the tie case runs twice: its second
run must give identical arrays)."""
import functools

import numpy as np
import pytest
import torch

from smart_tree_amd.data_types.cloud import Cloud
from smart_tree_amd.data_types.graph import Graph
from smart_tree_amd.skeleton import graph as G
from smart_tree_amd.skeleton.filter import outlier_removal
from smart_tree_amd.skeleton.skeletonize import DeviceSkeleton, Skeletonizer, run_components
from smart_tree_amd.synthetic import sample_tree_cloud

F = np.float32


# ----------------------------------------------------------------------------------- reference ---
def _d2(p, q):
    """(dx*dx + dy*dy) + dz*dz in float32, every operation rounded (numpy float32 arithmetic does not contract)."""
    dx, dy, dz = p[..., 0] - q[..., 0], p[..., 1] - q[..., 1], p[..., 2] - q[..., 2]
    assert dx.dtype == np.float32
    return (dx * dx + dy * dy) + dz * dz


def _candidates(P, comp, cloud, max_gap):
    """Every pair (lo < hi) of kept vertices in different components of one cloud with d2 <= max_gap^2: (bits of d2, lo, hi)."""
    r2 = F(max_gap) * F(max_gap)
    kept = np.flatnonzero(comp >= 0)
    out = []
    for a in range(0, len(kept), 256):
        u = kept[a:a + 256]
        d2 = _d2(P[u][:, None, :], P[kept][None, :, :])
        ok = (d2 <= r2) & (comp[u][:, None] != comp[kept][None, :]) & (cloud[u][:, None] == cloud[kept][None, :]) & (u[:, None] < kept[None, :])
        iu, iv = np.nonzero(ok)
        out.append(np.stack([d2[iu, iv].view(np.uint32).astype(np.int64), u[iu], kept[iv]], axis=1))
    return np.concatenate(out) if out else np.zeros((0, 3), np.int64)


def _kruskal(cand, comp):
    """Minimum spanning forest of the component graph under (d2 bits, lo, hi): rows of `cand`, in that order."""
    cand = cand[np.lexsort((cand[:, 2], cand[:, 1], cand[:, 0]))]
    parent = list(range(int(comp.max()) + 1 if len(comp) else 0))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    take = []
    for row in cand.tolist():
        a, b = find(int(comp[row[1]])), find(int(comp[row[2]]))
        if a != b:
            parent[a] = b
            take.append(row)
    groups = np.array([find(c) for c in range(len(parent))], np.int64)
    return np.array(take, np.int64).reshape(-1, 3), groups


def _reference(P, comp, cloud, max_gap):
    """(edges [B,2] sorted by (lo, hi), weights [B] float32, groups per component, all candidates)."""
    cand = _candidates(P, comp, cloud, max_gap)
    take, groups = _kruskal(cand, comp)
    take = take[np.lexsort((take[:, 2], take[:, 1]))] if len(take) else take
    w = np.sqrt(take[:, 0].astype(np.uint32).view(np.float32)) if len(take) else np.zeros(0, F)
    assert w.dtype == np.float32
    return take[:, 1:3], w, groups, cand


# ------------------------------------------------------------------------------------- inputs ---
def _stick(start, direction, count, step=0.01):
    d = np.asarray(direction, np.float64)
    d = d / np.linalg.norm(d)
    return (np.asarray(start, np.float64)[None, :] + (np.arange(count) * step)[:, None] * d[None, :]).astype(F)


def _scene(pieces):
    """pieces: list of [k,3] float32 arrays, one component each -> (P, edges chaining each piece, piece of every vertex)."""
    P = np.concatenate(pieces).astype(F) if pieces else np.zeros((0, 3), F)
    piece = np.concatenate([np.full(len(p), i) for i, p in enumerate(pieces)]).astype(np.int64) if pieces else np.zeros(0, np.int64)
    edges, base = [], 0
    for p in pieces:
        ids = base + np.arange(len(p))
        edges.append(np.stack([ids[:-1], ids[1:]], axis=1))
        base += len(p)
    edges = np.concatenate(edges).astype(np.int64) if edges else np.zeros((0, 2), np.int64)
    return P, edges, piece


def _t(a, dev):
    return torch.from_numpy(np.array(a, order="C")).to(dev)


def _run(dev, P, edges, piece, minv, max_gap, seg_off=None):
    """connected_components + bridge_components on the device; returns (edges sorted by (lo, hi), weights, comp of every vertex,
    cloud of every vertex, the raw device result)."""
    n = len(P)
    w = _d2(P[edges[:, 0]], P[edges[:, 1]]) if len(edges) else np.zeros(0, F)
    g = Graph(_t(P, dev), _t(edges.reshape(-1, 2), dev), _t(np.sqrt(w).astype(F), dev))
    if seg_off is not None:
        g.seg_off = _t(np.asarray(seg_off, np.int32), dev)
    cs = G.connected_components(g, minv)
    e, wt = G.bridge_components(cs, g.vertices, max_gap)
    if dev.type == "cuda":
        torch.cuda.synchronize()
    assert e.dtype == torch.int64 and wt.dtype == torch.float32 and e.ndim == 2 and e.shape[1] == 2 and wt.shape == (e.shape[0],)
    new_id = cs.new_id.cpu().numpy().astype(np.int64)
    comp_off = cs.comp_off.cpu().numpy().astype(np.int64)
    comp = np.where(new_id >= 0, np.searchsorted(comp_off, new_id, side="right") - 1, -1)
    # membership is what the construction says: one component per piece of at least minv vertices (a piece is one chain)
    sizes = np.bincount(piece, minlength=int(piece.max()) + 1 if n else 0)
    assert np.array_equal(comp >= 0, sizes[piece] >= max(minv, 1)) if n else True
    for c in np.unique(comp[comp >= 0]):
        assert len(np.unique(piece[comp == c])) == 1
    cloud = np.zeros(n, np.int64) if seg_off is None else np.searchsorted(np.asarray(seg_off)[1:], np.arange(n), side="right")
    ge, gw = e.cpu().numpy(), wt.cpu().numpy()
    assert np.all(ge[:, 0] < ge[:, 1])
    o = np.lexsort((ge[:, 1], ge[:, 0]))
    return ge[o], gw[o], comp, cloud, (e, wt)


def _check(dev, P, edges, piece, minv, max_gap, seg_off=None):
    ge, gw, comp, cloud, raw = _run(dev, P, edges, piece, minv, max_gap, seg_off)
    re_, rw, groups, cand = _reference(P, comp, cloud, max_gap)
    np.testing.assert_array_equal(ge, re_)
    np.testing.assert_array_equal(gw.view(np.uint32), rw.view(np.uint32))
    return ge, gw, comp, groups, cand, raw


# -------------------------------------------------------------------------------- kernel level ---
def test_threshold_and_chaining(backend):
    """Six collinear sticks with end-to-end gaps 0.03, 0.05, 0.05, 0.2, 0.5 and max_gap 0.1: the first four join in a chain, the
    last two stay alone.  Beside them three mutually close sticks: two bridges, not three."""
    lens, gaps = [64, 300, 100, 129, 257, 65], [0.03, 0.05, 0.05, 0.2, 0.5]
    pieces, x = [], 0.0
    for k, ln in enumerate(lens):
        pieces.append(_stick([x, 0, 0], [1, 0, 0], ln))
        x += (ln - 1) * 0.01 + (gaps[k] if k < len(gaps) else 0.0)
    trio = [_stick([0, 5, 0], [1, 0, 0], 70), _stick([0, 5.04, 0], [1, 0, 0], 90), _stick([0, 5, 0.04], [1, 0, 0], 80)]
    P, edges, piece = _scene(pieces + trio)
    ge, gw, comp, groups, cand, _ = _check(backend, P, edges, piece, 10, 0.1)
    # the groups are the components of the thresholded component graph (an edge wherever any pair is within max_gap)
    near = {(min(a, b), max(a, b)) for a, b in zip(comp[cand[:, 1]].tolist(), comp[cand[:, 2]].tolist())}
    pc = {int(comp[np.flatnonzero(piece == i)[0]]): i for i in range(9)}  # component -> piece
    assert {tuple(sorted((pc[a], pc[b]))) for a, b in near} == {(0, 1), (1, 2), (2, 3), (6, 7), (6, 8), (7, 8)}
    by_piece = lambda g: sorted(sorted(pc[c] for c in range(9) if g[c] == r) for r in set(g.tolist()))
    assert by_piece(groups) == [[0, 1, 2, 3], [4], [5], [6, 7, 8]]
    got_groups = _kruskal(np.concatenate([np.zeros((len(ge), 1), np.int64), ge], axis=1), comp)[1]
    assert by_piece(got_groups) == by_piece(groups)
    assert len(ge) == 5 and sum(1 for u, v in ge.tolist() if piece[u] >= 6) == 2
    # the chain's bridges are the end-to-end gaps themselves
    chain = sorted(float(w) for (u, v), w in zip(ge.tolist(), gw) if piece[u] < 6)
    np.testing.assert_allclose(chain, [0.03, 0.05, 0.05], rtol=1e-4)


def test_ties_on_a_lattice(backend):
    """Coordinates are multiples of 1/64 (every d2 exact): most candidates share their d2 with many others, and the order's
    (lo, hi) part decides.  A second run returns identical arrays."""
    pieces = []
    for j in range(6):
        for k in range(3):
            for x0 in (0, 9):
                pieces.append((np.stack([x0 + np.arange(7), np.full(7, 3 * j), np.full(7, 3 * k)], axis=1) / 64.0).astype(F))
    rng = np.random.RandomState(3)
    pieces = [pieces[i] for i in rng.permutation(len(pieces))]  # component numbers do not follow the geometry
    P, edges, piece = _scene(pieces)
    ge, gw, comp, groups, cand, raw = _check(backend, P, edges, piece, 0, 4.0 / 64.0)
    d2s, counts = np.unique(cand[:, 0], return_counts=True)
    assert len(ge) == 35 and len(set(groups.tolist())) == 1 and len(cand) > 20 * len(d2s) and counts.max() > 100
    assert len(np.unique(gw)) <= 3  # 3/64 and 2/64 apart: the forest itself is made of tied edges
    again = _run(backend, P, edges, piece, 0, 4.0 / 64.0)[4]
    assert torch.equal(raw[0], again[0]) and torch.equal(raw[1].view(torch.int32), again[1].view(torch.int32))


def test_the_bound_is_inclusive(backend):
    """max_gap = 0.125, max_gap^2 = 2^-6 exactly.  One pair of sticks has its nearest vertices at d2 == 2^-6 and is bridged; another
    has them at the next float32 above and is not."""
    up = F(3.0 * 2.0 ** -16)  # dy: dy*dy = 2.25 * 2^-30, and 2^-6 + that rounds to 2^-6 + one ulp
    P, edges, piece = _scene([_stick([0, 0, 0], [-1, 0, 0], 64), _stick([0.125, 0, 0], [1, 0, 0], 70),
                              _stick([0, 0, 10], [-1, 0, 0], 66), _stick([0.125, up, 10], [1, 0, 0], 68)])
    r2 = F(0.125) * F(0.125)
    assert _d2(P[0], P[64]) == r2 and _d2(P[134], P[200]) == np.nextafter(r2, F(1)) and P[200, 1] == up
    ge, gw, comp, groups, cand, _ = _check(backend, P, edges, piece, 10, 0.125)
    assert ge.tolist() == [[0, 64]] and gw.tolist() == [0.125] and len(cand) == 1


@pytest.mark.parametrize("minv,bridges", [(10, 0), (0, 2)])
def test_dropped_components_are_no_stepping_stones(backend, minv, bridges):
    """A 5-vertex clump midway between two sticks that are 0.15 apart, max_gap 0.1.  With minimum_vertices 10 the clump is
    dropped: no bridge, none of its vertices in an edge.  (Kept -- minimum_vertices 0 -- it joins both sticks.)"""
    clump = _stick([0.075, 0, 0], [0, 1, 0], 5, step=0.001)
    P, edges, piece = _scene([_stick([0, 0, 0], [-1, 0, 0], 100), clump, _stick([0.15, 0, 0], [1, 0, 0], 120)])
    ge, gw, comp, groups, cand, _ = _check(backend, P, edges, piece, minv, 0.1)
    assert len(ge) == bridges
    if minv == 10:
        assert np.all(comp[piece == 1] == -1) and len(cand) == 0
    else:
        assert all((piece[u] == 1) != (piece[v] == 1) for u, v in ge.tolist())


@functools.lru_cache(maxsize=None)
def _random_sticks(seed, count, box):
    rng = np.random.RandomState(seed)
    pieces = []
    for _ in range(count):
        d = rng.normal(size=3)
        pieces.append(_stick(rng.uniform(0, box, 3), d, int(rng.randint(64, 190))))
    return _scene(pieces)


def test_across_workgroups(backend):
    """~5000 vertices in 40 randomly placed sticks (about twenty workgroups of queries): the minima of one component come from
    many workgroups, and the forest needs several Boruvka rounds."""
    P, edges, piece = _random_sticks(11, 40, 2.4)
    assert 4500 < len(P) < 5600
    ge, gw, comp, groups, cand, _ = _check(backend, P, edges, piece, 10, 0.25)
    stats = dict(G.last_bridge_stats)
    assert stats["bridges"] == len(ge) >= 25 and len(set(groups.tolist())) == 40 - len(ge)
    assert stats["rounds"] >= 4  # three rounds that hook and the one that finds nothing
    assert 0 < stats["boundary"] < len(P)  # later rounds run over a subset


def test_batch_of_clouds(backend):
    """Two clouds in the same space with a cloud that keeps no component between them: no bridge crosses clouds, and every cloud
    gets what it gets alone (ids shifted by the cloud's first vertex)."""
    a = _random_sticks(21, 12, 1.2)
    b = _random_sticks(22, 14, 1.2)
    tiny = _scene([_stick([0.5, 0.5, 0.5], [0, 0, 1], 5)])
    P = np.concatenate([a[0], tiny[0], b[0]])
    off = np.cumsum([0, len(a[0]), len(tiny[0]), len(b[0])])
    edges = np.concatenate([a[1], tiny[1] + off[1], b[1] + off[2]])
    piece = np.concatenate([a[2], tiny[2] + 100, b[2] + 200])
    ge, gw, comp, groups, cand, _ = _check(backend, P, edges, piece, 10, 0.2, seg_off=off)
    cloud = np.searchsorted(off[1:], ge, side="right")
    assert np.all(cloud[:, 0] == cloud[:, 1]) and set(cloud[:, 0].tolist()) == {0, 2}
    assert np.all(comp[off[1]:off[2]] == -1)
    # without the clouds' ranges the two trees WOULD be joined: the separation is the batch's doing, not the geometry's
    assert len(_candidates(P, comp, np.zeros(len(P), np.int64), 0.2)) > len(cand)
    for (pp, ee, pc), base, which in ((a, off[0], 0), (b, off[2], 2)):
        se, sw = _run(backend, pp, ee, pc, 10, 0.2)[:2]
        sel = cloud[:, 0] == which
        np.testing.assert_array_equal(ge[sel] - base, se)
        np.testing.assert_array_equal(gw[sel].view(np.uint32), sw.view(np.uint32))
        assert len(se) >= 5


def test_degenerate_inputs(backend):
    def empty(P, edges, piece, minv, max_gap):
        ge, gw = _run(backend, P, edges, piece, minv, max_gap)[:2]
        assert ge.shape == (0, 2) and gw.shape == (0,) and ge.dtype == np.int64 and gw.dtype == np.float32

    empty(*_scene([]), 0, 0.1)  # n = 0
    empty(*_scene([_stick([0, 0, 0], [1, 0, 0], 80)]), 10, 0.1)  # one component
    two = _scene([_stick([0, 0, 0], [-1, 0, 0], 80), _stick([0.02, 0, 0], [1, 0, 0], 80)])
    empty(*two, 10, 0.0)  # max_gap = 0 (and below)
    empty(*two, 10, -1.0)
    empty(*two, 100, 0.1)  # nothing kept
    empty(*_scene([np.full((40, 3), 0.25, F)]), 10, 0.1)  # all vertices identical: one component of zero extent
    # identical vertices in SEVERAL components are candidates like any others (d2 = 0 <= max_gap^2): the definition holds there too
    ge, gw = _check(backend, *_scene([np.full((40, 3), 0.25, F)] * 3), 10, 0.1)[:2]
    assert len(ge) == 2 and np.all(gw == 0.0) and ge.tolist() == [[0, 40], [0, 80]]
    assert len(_check(backend, *two, 10, 0.1)[0]) == 1  # (the pair above does join once max_gap allows it)
    with pytest.raises(ValueError):
        Skeletonizer(K=16, min_connection_length=0.02, minimum_graph_vertices=32, device=backend, connect_components=True)
    with pytest.raises(ValueError):
        Skeletonizer(K=16, min_connection_length=0.02, minimum_graph_vertices=32, device=backend, connect_components=True, max_gap=-0.1)


# ---------------------------------------------------------------------------------- end to end ---
SLABS = ((0.55, 0.70), (1.78, 1.90))  # heights (y of the axis point) cut out: across the trunk, and across the boughs above it
MAX_GAP = 0.25


@functools.lru_cache(maxsize=None)
def _cut_tree(seed=5, n=3300):
    """A seeded synthetic tree with exact medial vectors (no surface noise: xyz + medial_vector is the axis point) and two slabs
    removed across its branches."""
    c = sample_tree_cloud(n, seed=seed, scale=0.5, max_depth=2, noise=0.0)
    y = (c["xyz"] + c["medial_vector"])[:, 1]
    keep = np.ones(len(y), bool)
    for lo, hi in SLABS:
        keep &= ~((y >= lo) & (y <= hi))
    assert (~keep).sum() > 0.05 * n
    xyz, mv = np.ascontiguousarray(c["xyz"][keep]), np.ascontiguousarray(c["medial_vector"][keep])
    xyz.setflags(write=False)
    mv.setflags(write=False)
    return xyz, mv


def _skeletonizer(dev, **kw):
    sk = Skeletonizer(K=16, min_connection_length=0.02, minimum_graph_vertices=32, device=dev, **kw)
    sk.block_threads = 128 if dev.type == "cpu" else 0
    return sk


def _cloud(dev, xyz, mv):
    return Cloud(xyz=_t(xyz, dev), medial_vector=_t(mv, dev))


def _signature(sk):
    return [(tree._id, b._id, b.parent_id, b.xyz.numpy().tobytes(), b.radii.numpy().tobytes())
            for tree in sk.skeletons for b in tree.branches.values()]


_OFF = {}


def _feature_off(dev):
    """(trees, signature) of the cut tree without the feature: computed once per backend, shared, never written."""
    if dev.type not in _OFF:
        sk = _skeletonizer(dev).forward(_cloud(dev, *_cut_tree()))
        _OFF[dev.type] = (len(sk.skeletons), _signature(sk))
    return _OFF[dev.type]


def _expected_with_reference_bridges(dev, xyz, mv, max_gap):
    """Today's stage on a plain Graph whose edge list is the kNN edges plus the REFERENCE's bridges (the edge-list path of
    connected_components, tests/test_graph_stage.py).  The first stages are Skeletonizer.forward's own."""
    sk = _skeletonizer(dev)
    cloud = _cloud(dev, xyz, mv)
    medial, radius = G.medial_points(cloud.xyz, cloud.medial_vector)
    keep = outlier_removal(medial, radius.unsqueeze(1), nb_points=8).nonzero().view(-1)
    cloud = cloud.filter(keep, assume_sorted=True)
    medial, radius = medial.index_select(0, keep), radius.index_select(0, keep)
    graph = G.nn_graph(medial, radius.clamp(min=sk.min_connection_length), K=sk.K)
    cs = graph.connected_cugraph_components(minimum_vertices=sk.minimum_graph_vertices)
    new_id, comp_off = cs.new_id.cpu().numpy().astype(np.int64), cs.comp_off.cpu().numpy().astype(np.int64)
    comp = np.where(new_id >= 0, np.searchsorted(comp_off, new_id, side="right") - 1, -1)
    P = medial.cpu().numpy()
    be, bw, groups, _ = _reference(P, comp, np.zeros(len(P), np.int64), max_gap)
    joined = Graph(medial, torch.cat((graph.edges, _t(be, dev))), torch.cat((graph.edge_weights, _t(bw, dev))))
    cs2 = G.connected_components(joined, sk.minimum_graph_vertices)
    res = run_components(cs2, medial, radius, cloud.xyz[:, 1].contiguous(), block_threads=sk.block_threads)
    return DeviceSkeleton.from_components(cs2, res, medial, radius), cs.n_components, len(be), len(set(groups.tolist()))


def test_skeletonizer_joins_a_cut_tree(backend):
    xyz, mv = _cut_tree()
    assert 3000 <= len(xyz) <= 5000
    k_off, _ = _feature_off(backend)
    on = _skeletonizer(backend, connect_components=True, max_gap=MAX_GAP).forward(_cloud(backend, xyz, mv))
    assert G.last_bridge_stats["bridges"] == k_off - 1 >= 2  # k > 1 skeletons without the feature ...
    assert len(on.skeletons) == 1  # ... exactly one with it, max_gap above the slabs' width
    assert max(hi - lo for lo, hi in SLABS) < MAX_GAP
    branches = on.skeletons[0].branches
    parents = [b.parent_id for b in branches.values()]
    assert len(parents) >= 5 and sum(p == -1 for p in parents) == 1  # every branch but the root has a parent ...
    assert all(p in branches for p in parents if p != -1)  # ... and it is a branch of the tree
    want, k_graph, n_ref, n_groups = _expected_with_reference_bridges(backend, xyz, mv, MAX_GAP)
    assert k_graph == k_off and n_ref == k_off - 1 and n_groups == 1
    assert _signature(on) == _signature(want)  # branch for branch, bit for bit


def test_max_gap_below_every_gap_changes_nothing(backend):
    xyz, mv = _cut_tree()
    k_off, sig_off = _feature_off(backend)
    G.last_bridge_stats.clear()
    on = _skeletonizer(backend, connect_components=True, max_gap=0.015).forward(_cloud(backend, xyz, mv))
    assert G.last_bridge_stats == {"rounds": 1, "boundary": 0, "bridges": 0}  # the search ran and found nobody
    assert k_off >= 3 and _signature(on) == sig_off


class _ExactInference:
    """Stands in for the network in a Pipeline: every point gets its exact medial vector back and class 0 (Pipeline passes xyz
    and rgb on; a cloud is recognised by its size, the batch by the sum)."""

    def __init__(self, clouds):
        self.by_size = {len(x): mv for x, mv in clouds}
        assert len(self.by_size) == len(clouds)
        self.by_size[sum(len(x) for x, _ in clouds)] = np.concatenate([mv for _, mv in clouds])

    def forward(self, cloud):
        n, dev = len(cloud), cloud.xyz.device
        return Cloud(xyz=cloud.xyz, rgb=cloud.rgb, medial_vector=_t(self.by_size[n], dev), class_l=torch.zeros((n, 1), device=dev),
                     seg_off=cloud.seg_off)


def test_process_clouds_equals_process_cloud(backend):
    """Pipeline.process_clouds on three cut trees (prune, repair and smooth on, as in conf/pipeline.yaml) equals process_cloud on
    each of them."""
    from smart_tree_amd.dataset.augmentations import AugmentationPipeline, CentreCloud
    from smart_tree_amd.pipeline import Pipeline

    trees = [_cut_tree(seed=2, n=1700), _cut_tree(seed=7, n=1500), _cut_tree(seed=3, n=1500)]
    pipe = Pipeline(AugmentationPipeline([CentreCloud()]), _ExactInference(trees),
                    _skeletonizer(backend, connect_components=True, max_gap=MAX_GAP), repair_skeletons=True, smooth_skeletons=True,
                    smooth_kernel_size=11, prune_skeletons=True, min_skeleton_radius=0.01, min_skeleton_length=0.02, device=backend)
    cloud = lambda xyz: Cloud(xyz=_t(xyz, backend), rgb=torch.zeros((len(xyz), 3), device=backend))
    serial, bridged = [], 0
    for xyz, _ in trees:
        serial.append(pipe.process_cloud(cloud=cloud(xyz)))
        bridged += G.last_bridge_stats["bridges"]
        assert G.last_bridge_stats["bridges"] >= 2 and len(serial[-1].skeletons) == 1
    parts = pipe.process_clouds([cloud(xyz) for xyz, _ in trees])
    assert G.last_bridge_stats["bridges"] == bridged and len(parts) == 3
    for one, got in zip(serial, parts):
        assert len(_signature(one)) >= 2 and _signature(got) == _signature(one)
