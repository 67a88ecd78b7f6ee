"""The neighbour searches serve a RUN of consecutive queries per wavefront (csrc/knn.hip, KNN_QW): ragged runs, runs that straddle
clouds, unequal neighbours inside a run, subsets and non-finite queries -- every row exactly the oracle's, whatever the run length."""
import functools

import numpy as np
import pytest
import torch

from oracle import skeleton_oracle as so
from smart_tree_amd.skeleton import graph as G
from smart_tree_amd.skeleton.filter import outlier_removal

N1S = [1, 2, 3, 5, 7, 9, 15, 17, 31, 33, 63, 65, 255, 257]


@functools.lru_cache(maxsize=None)
def _cloud():
    rng = np.random.RandomState(3)
    dst = rng.uniform(0, 1, (1500, 3)).astype(np.float32)
    dst[100:140] = dst[50]  # exact duplicates: index tie-break
    src = np.concatenate([dst[:200], rng.uniform(-0.1, 1.1, (57, 3)).astype(np.float32)])
    return src, dst


@functools.lru_cache(maxsize=None)
def _ref_other(K):
    src, dst = _cloud()
    return so.knn(src, dst, K, 0.12)


def _bounded(idx, d, bound, strict):
    """graph.py:38-40 / filter.py:9-10: neighbours beyond the query's own bound dropped (a prefix of the sorted row stays)."""
    idx, d = idx.copy(), d.copy()
    with np.errstate(invalid="ignore"):
        far = ~((d < bound[:, None]) if strict else (d <= bound[:, None]))
    idx[far], d[far] = -1, np.nan
    return idx, d


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _check(got, want):
    np.testing.assert_array_equal(got[0].cpu().numpy(), want[0])
    np.testing.assert_array_equal(got[1].cpu().numpy(), want[1])  # NaN == NaN under assert_array_equal


@pytest.mark.parametrize("K", [1, 8, 16, 64])
def test_ragged_runs_other_source(backend, K):
    """src != dst: the run is consecutive src rows; every n1 around the run lengths 2, 4, 8 and the 4 wavefronts of a workgroup."""
    src, dst = _cloud()
    ref_idx, ref_d = _ref_other(K)
    d = _t(dst, backend)
    for n1 in N1S:
        got = G.knn(_t(src[:n1], backend), d, K=K, r=0.12)
        _check(got, (ref_idx[:n1], ref_d[:n1]))


@pytest.mark.parametrize("K", [1, 8, 16, 64])
def test_ragged_runs_cell_order(backend, K):
    """src IS dst: the run is consecutive records of the cell-sorted list; with per-query bounds, and the counting query beside it."""
    _, dst = _cloud()
    rng = np.random.RandomState(5)
    for n1 in N1S:
        pts = dst[:n1]
        bound = rng.uniform(0.1, 0.5, n1).astype(np.float32)
        p = _t(pts, backend)
        want = _bounded(*so.knn(pts, pts, K, 0.4), bound, False)
        _check(G.knn(p, p, K=K, r=0.4, bound=_t(bound, backend), bound_mode=G.BOUND_LE), want)
        if K == 8:  # count = search: the mask of k_knn<8, true> is the 8th slot of the K = 8 search
            idx, _, _ = G.knn(p, p, K=8, r=-1.0, bound=_t(bound, backend), bound_mode=G.BOUND_LT, cell=-G.SEARCH_CELL_DIV)
            keep = outlier_removal(p, _t(bound, backend).unsqueeze(1), nb_points=8).cpu().numpy()
            np.testing.assert_array_equal(keep, idx[:, 7].cpu().numpy() != -1)
            np.testing.assert_array_equal(keep, so.outlier_removal(pts, bound, 8))


@pytest.mark.parametrize("K", [8, 16])
def test_run_straddles_clouds(backend, K):
    """A batch of clouds of 5, 1, 0, 11 and 300 points: runs hold queries of several clouds and an empty cloud between them; the
    radius is each cloud's own max(bound) (r < 0), a factor 10 apart from cloud to cloud."""
    sizes = [5, 1, 0, 11, 300]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    rng = np.random.RandomState(9)
    pts = rng.uniform(0, 0.3, (off[-1], 3)).astype(np.float32)
    bound = np.empty(off[-1], np.float32)
    for c, top in enumerate([0.5, 0.05, 1.0, 0.4, 0.04]):
        a, b = off[c], off[c + 1]
        bound[a:b] = rng.uniform(0.3, 1.0, b - a).astype(np.float32) * np.float32(top)
        if b > a:
            bound[a] = np.float32(top)
    p, bd, seg = _t(pts, backend), _t(bound, backend), _t(off, backend)
    idx, d, _ = G.knn(p, p, K=K, r=-1.0, bound=bd, bound_mode=G.BOUND_LE, cell=-G.GRAPH_CELL_DIV, src_seg_off=seg, dest_seg_off=seg)
    idx, d = idx.cpu().numpy(), d.cpu().numpy()
    keep = outlier_removal(p, bd.unsqueeze(1), nb_points=8, seg_off=seg).cpu().numpy()
    for c in range(len(sizes)):
        a, b = off[c], off[c + 1]
        if a == b:
            continue
        want = _bounded(*so.knn(pts[a:b], pts[a:b], K, float(bound[a:b].max())), bound[a:b], False)
        one = G.knn(_t(pts[a:b], backend), _t(pts[a:b], backend), K=K, r=-1.0, bound=_t(bound[a:b], backend), bound_mode=G.BOUND_LE,
                    cell=-G.GRAPH_CELL_DIV)
        _check(one, want)
        np.testing.assert_array_equal(np.where(idx[a:b] >= 0, idx[a:b] - a, -1), want[0])
        np.testing.assert_array_equal(d[a:b], want[1])
        np.testing.assert_array_equal(keep[a:b], so.outlier_removal(pts[a:b], bound[a:b], 8))


def test_unequal_neighbours_in_one_run(backend):
    """Bounds alternate between 0.02 and 0.5 from query to query: a query with one row chunk and a handful of candidates next to one
    with several chunks, more than 4096 candidates in a chunk (4200 copies of one point among 6000: no start marks) and far more
    than KNN_CAP hits -- while its neighbours in the run find fewer than K.  Cuts in one query must not leak into the next."""
    rng = np.random.RandomState(13)
    dst = rng.uniform(0, 1, (6000, 3)).astype(np.float32)
    dst[1000:5200] = dst[1000]
    lonely = rng.uniform(2.0, 3.0, (12, 3)).astype(np.float32)  # nobody within 0.02
    dst[:12] = lonely
    src = np.empty((24, 3), np.float32)
    src[0::2] = dst[1000] + rng.uniform(-0.01, 0.01, (12, 3)).astype(np.float32)
    src[1::2] = lonely
    bound = np.tile(np.array([0.5, 0.02], np.float32), 12)
    for K in (8, 16):
        want = _bounded(*so.knn(src, dst, K, 0.5), bound, False)
        assert (want[0][0::2, -1] >= 0).all() and (want[0][1::2, 1] == -1).all() and (want[0][1::2, 0] >= 0).all()
        got = G.knn(_t(src, backend), _t(dst, backend), K=K, r=0.5, bound=_t(bound, backend), bound_mode=G.BOUND_LE, cell=0.25)
        _check(got, want)


def test_unequal_neighbours_cell_order_count_equals_search(backend):
    """The same alternation with src IS dst: the counting query and the K = 8 / K = 16 searches over one cloud with a dense clump
    (more hits than KNN_CAP) whose neighbours in cell order are sparse."""
    rng = np.random.RandomState(17)
    pts = rng.uniform(0, 1, (1400, 3)).astype(np.float32)
    pts[300:700] = pts[300] + rng.uniform(-0.003, 0.003, (400, 3)).astype(np.float32)
    bound = np.tile(np.array([0.02, 0.5], np.float32), 700)
    p, bd = _t(pts, backend), _t(bound, backend)
    for K in (8, 16):
        want = _bounded(*so.knn(pts, pts, K, 0.5), bound, True)
        got = G.knn(p, p, K=K, r=-1.0, bound=bd, bound_mode=G.BOUND_LT, cell=-G.SEARCH_CELL_DIV)
        _check(got, want)
    keep = outlier_removal(p, bd.unsqueeze(1), nb_points=8).cpu().numpy()
    idx8 = G.knn(p, p, K=8, r=-1.0, bound=bd, bound_mode=G.BOUND_LT, cell=-G.SEARCH_CELL_DIV)[0].cpu().numpy()
    np.testing.assert_array_equal(keep, idx8[:, 7] != -1)
    np.testing.assert_array_equal(keep, so.outlier_removal(pts, bound, 8))
    assert 0 < keep.sum() < len(keep)


@pytest.mark.parametrize("nvalid", [1001, 0, 3000], ids=["1001-of-3000", "none", "all"])
def test_subset_is_filtering_first(backend, nvalid):
    """st_radius_count_seg with `valid`: the number of valid points is no multiple of any run length, so the last run is ragged
    against the table's total, not against n."""
    rng = np.random.RandomState(19)
    n = 3000
    pts = rng.rand(n, 3).astype(np.float32)
    rad = rng.uniform(0.02, 0.2, n).astype(np.float32)
    valid = np.zeros(n, bool)
    valid[rng.permutation(n)[:nvalid]] = True
    got = outlier_removal(_t(pts, backend), _t(rad, backend).unsqueeze(1), nb_points=8, valid=_t(valid, backend)).cpu().numpy()
    want = np.zeros(n, bool)
    sel = np.nonzero(valid)[0]
    if nvalid:
        sub = outlier_removal(_t(pts[sel], backend), _t(rad[sel], backend).unsqueeze(1), nb_points=8).cpu().numpy()
        np.testing.assert_array_equal(sub, so.outlier_removal(pts[sel], rad[sel], 8))
        idx8 = G.knn(_t(pts[sel], backend), _t(pts[sel], backend), K=8, r=-1.0, bound=_t(rad[sel], backend), bound_mode=G.BOUND_LT,
                     cell=-G.SEARCH_CELL_DIV)[0].cpu().numpy()
        np.testing.assert_array_equal(sub, idx8[:, 7] != -1)
        want[sel] = sub
        assert 0 < sub.sum() < nvalid
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("same", [False, True], ids=["other-source", "cell-order"])
def test_non_finite_inside_a_run(backend, same):
    """A NaN coordinate, an infinite coordinate, a NaN bound and an infinite bound at positions 1 and 2 of a run: their own rows are
    empty (the infinite bound: everything inside r) and their neighbours' rows are what the oracle says."""
    rng = np.random.RandomState(23)
    dst = rng.uniform(0, 0.5, (600, 3)).astype(np.float32)
    src = dst if same else dst[:40].copy()
    bound = rng.uniform(0.05, 0.2, len(src)).astype(np.float32)
    src[1, 1] = np.nan
    src[2, 0] = np.inf
    bound[9] = np.nan  # (rows 1, 2 and 9, 10: positions 1 and 2 of a run of 2, 4 or 8)
    bound[10] = np.inf
    s = _t(src, backend)
    d = s if same else _t(dst, backend)
    ok = np.delete(np.arange(len(src)), [1, 2])  # the oracle's grid takes finite points only: it searches the cloud without them
    for K in (8, 16):
        if same:
            ci, cd = _bounded(*so.knn(src[ok], src[ok], K, 0.15), bound[ok], False)
            want = np.full((len(src), K), -1, np.int64), np.full((len(src), K), np.nan, np.float32)
            want[0][ok], want[1][ok] = np.where(ci >= 0, ok[np.maximum(ci, 0)], -1), cd
        else:
            want = _bounded(*so.knn(src, dst, K, 0.15), bound, False)
        assert (want[0][[1, 2, 9]] == -1).all() and (want[0][10] >= 0).sum() > 1 and (want[0][[0, 3, 8, 11]][:, 0] >= 0).all()
        _check(G.knn(s, d, K=K, r=0.15, bound=_t(bound, backend), bound_mode=G.BOUND_LE), want)
    if same:
        with np.errstate(invalid="ignore"):
            dd = src[:, None, :] - src[None, :, :]
            d2 = (dd[..., 0] * dd[..., 0] + dd[..., 1] * dd[..., 1]) + dd[..., 2] * dd[..., 2]
            brute = (np.sqrt(d2) < bound[:, None]).sum(1) >= 8
        keep = outlier_removal(s, _t(bound, backend).unsqueeze(1), nb_points=8).cpu().numpy()
        idx8 = G.knn(s, s, K=8, r=-1.0, bound=_t(bound, backend), bound_mode=G.BOUND_LT, cell=-G.SEARCH_CELL_DIV)[0].cpu().numpy()
        np.testing.assert_array_equal(keep, idx8[:, 7] != -1)
        np.testing.assert_array_equal(keep, brute)
        assert not keep[1] and not keep[2] and not keep[9] and keep[10]
