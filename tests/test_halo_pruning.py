"""Halo pruning: in blocks mode the decoder computes only the rows the inner voxels depend on (csrc/st_rule.h "Which decoder
rows ...", csrc/brick.hip st_brick_pyramid_need, ModelInference(prune_halo=True)).

What is checked:
  * the row lists against an EXACT closure walked backwards through the pyramid's own tables (every list prefix is a superset),
    against the rule itself restated in numpy (the lists are exactly what the rule says), and their form (no duplicates, rows of
    the level, brick order inside a margin class, counts = the host counts, the filtered parity order a sub-sequence of the full one);
  * the lists leave rows out at the shape tested (a condition on the inputs, so the equalities below are not vacuous);
  * the kept rows come out bit for bit as without pruning, the others are zero, and no row that a list launch left out is read
    (convolution outputs poisoned with NaN);
  * the modes that must not prune give today's outputs on every row.
Shapes: 5 cm voxels, 1 m blocks with a 0.4 m halo -- a halo of eight level-0 voxels, so that pruning acts at levels 0 and 1."""
import functools
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import voxel_oracle as vo
from smart_tree_amd.data_types.cloud import Cloud
from smart_tree_amd.dataset.augmentations import AugmentationPipeline, CentreCloud
from smart_tree_amd.model import sparse_ops as ops
from smart_tree_amd.model.model_inference import ModelInference
from smart_tree_amd.model.sparse import sparse_from_batch
from smart_tree_amd.pipeline import Pipeline
from smart_tree_amd.skeleton.skeletonize import Skeletonizer
from smart_tree_amd.synthetic import sample_tree_cloud

ROOT = Path(__file__).resolve().parents[1]
WEIGHTS = ROOT / "smart_tree_amd" / "model" / "weights" / "noble-elevator-58.npz"
VOXEL, BLOCK, BUFFER = 0.05, 1.0, 0.4
DEPTH = 3
BASE = (0, 1, 2)  # a[l] of csrc/st_rule.h for the levels that have lists
N_POINTS, SEED, SCALE = 4000, 2, 0.35  # the tree of the network tests: at least three blocks (asserted)


@functools.lru_cache(maxsize=None)
def _tree(n=N_POINTS, seed=SEED, scale=SCALE):
    c = sample_tree_cloud(n, seed=seed, scale=scale, max_depth=4)
    return vo.centre_cloud(c["xyz"]), c["rgb"]


@functools.lru_cache(maxsize=None)
def _voxels(n=N_POINTS, seed=SEED, scale=SCALE, buffer=BUFFER):
    xyz, rgb = _tree(n, seed, scale)
    return vo.voxelize_cloud(xyz, rgb, VOXEL, BLOCK, buffer)


def _bound(buffer=BUFFER):
    return int(round((BLOCK + 2 * buffer) / VOXEL)) + 2


# ---- the lists ------------------------------------------------------------------------------------------------------------------
def _rule_classes(coords, level, lo, hi):
    """margin class (0, 1, 2; 3 = not needed) of every row of a level: the rule of csrc/st_rule.h in numpy"""
    b = coords[:, 0]
    blo, bhi = lo[b] >> level, (hi[b] + (1 << level) - 1) >> level
    c = coords[:, 1:]
    margin = np.maximum(np.maximum(blo - c, c - bhi), 0).max(1)
    cls = np.clip(margin - BASE[level], 0, 3)
    cls[(lo[b] > hi[b]).any(1)] = 3
    return cls


def _closure(pyr, inner_rows):
    """Exact: per level the rows Tail.sequence.3 / identity, Tail.sequence.0 and Decode must compute for the inner rows."""
    reach = lambda table, rows: np.unique(table[:, rows][table[:, rows] >= 0])
    out, s3 = [], np.asarray(inner_rows)
    for level in range(DEPTH):
        subm, up = pyr.subm[level].cpu().numpy(), pyr.up[level].cpu().numpy()
        s0 = reach(subm, s3)  # sequence.3 is submanifold (a row reads itself: s0 holds s3)
        dec = np.union1d(reach(subm, s0), s3)  # sequence.0 and the identity read cat(skip, decoded)
        out.append((s3, s0, dec))
        s3 = reach(up, dec)  # the inverse convolution reads the Tail of the level below
    return out


def _check_lists(coords, mask, backend, blk_seg=None, n_seg=1, bound=None):
    nb = int(coords[:, 0].max()) + 1
    bound = bound or int(coords[:, 1:].max()) + 1
    got = ops.brick_pyramid(torch.from_numpy(coords).to(backend), DEPTH, nb, bound, blk_seg, n_seg, torch.from_numpy(mask).to(backend))
    assert got is not None
    pyr, order0 = got
    order0 = order0.cpu().numpy()
    assert len(pyr.need) == DEPTH
    inner = mask[order0].astype(bool)  # brick order
    c0 = pyr.coords[0].cpu().numpy()
    lo, hi = np.full((nb, 3), 2 ** 30), np.full((nb, 3), -1)
    np.minimum.at(lo, c0[inner, 0], c0[inner, 1:])
    np.maximum.at(hi, c0[inner, 0], c0[inner, 1:])
    exact = _closure(pyr, np.nonzero(inner)[0])
    shares = []
    for level in range(DEPTH):
        need, n = pyr.need[level], pyr.coords[level].shape[0]
        order, up_need = need.order.cpu().numpy(), need.up_order.cpu().numpy()
        cls = _rule_classes(pyr.coords[level].cpu().numpy(), level, lo, hi)
        # the lists are what the rule says: class 0, then 1, then 2, brick order inside a class; counts = the host counts
        want = np.concatenate([np.nonzero(cls == t)[0] for t in range(3)])
        np.testing.assert_array_equal(order, want)
        assert need.counts == tuple(int((cls <= t).sum()) for t in range(3)) and len(order) == need.counts[2]
        assert len(np.unique(order)) == len(order) and (len(order) == 0 or (order.min() >= 0 and order.max() < n))
        # every prefix holds the exact set of its convolution
        for t, rows in enumerate(exact[level]):
            assert np.isin(rows, order[: need.counts[t]]).all(), (level, t)
        # the filtered parity order: the sub-sequence of the full one whose rows have a class, tags and grouping kept
        full = pyr.up_order[level].cpu().numpy()
        np.testing.assert_array_equal(up_need, full[cls[full & 0x0FFFFFFF] < 3])
        rows = up_need & 0x0FFFFFFF
        cu = pyr.coords[level].cpu().numpy()[rows]
        par = ((cu[:, 1] & 1) << 2) | ((cu[:, 2] & 1) << 1) | (cu[:, 3] & 1)
        assert (np.diff(par) >= 0).all() and np.array_equal((up_need >> 28) & 0xF, 8 + par)
        assert np.isin(exact[level][2], rows).all()
        shares.append(tuple(c / max(n, 1) for c in need.counts))
    return shares, pyr


def _no_inner_block(v):
    """coords, mask with the inner rows of the last block cleared: a block whose rows are all halo"""
    coords, mask = v["coords"].astype(np.int32), v["mask"].astype(np.uint8).copy()
    assert coords[:, 0].max() >= 2, "the test cloud must have at least three blocks"
    mask[coords[:, 0] == coords[:, 0].max()] = 0
    return coords, mask


def test_lists_hold_the_exact_closure_and_leave_rows_out(backend):
    """One cloud, >= 3 blocks, one of them without an inner row.  Not vacuous: the level-0 list of Tail.sequence.3 leaves out at
    least 20 % of the rows and every level-1 list leaves some out (a condition on the chosen inputs, checked on the oracle's
    voxelisation -- the lists are functions of coordinates and mask alone)."""
    coords, mask = _no_inner_block(_voxels())
    perm = np.random.RandomState(0).permutation(len(coords))  # any input order
    shares, pyr = _check_lists(coords[perm], mask[perm], backend, bound=_bound())
    assert shares[0][0] <= 0.8, shares
    assert all(s < 1.0 for s in shares[1]), shares
    c0 = pyr.coords[0].cpu().numpy()
    last = c0[:, 0] == c0[:, 0].max()
    assert last.any() and not np.isin(np.nonzero(last)[0], pyr.need[0].order.cpu().numpy()).any()  # no box: nothing needed


def test_lists_of_a_two_cloud_batch(backend):
    a, b = _voxels(), _voxels(3000, 5, 0.3)
    cb = b["coords"].astype(np.int32).copy()
    na = int(a["coords"][:, 0].max()) + 1
    cb[:, 0] += na
    coords = np.concatenate([a["coords"].astype(np.int32), cb])
    mask = np.concatenate([a["mask"], b["mask"]]).astype(np.uint8)
    seg = np.concatenate([np.zeros(na, np.int32), np.ones(int(cb[:, 0].max()) + 1 - na, np.int32)])
    shares, _ = _check_lists(coords, mask, backend, torch.from_numpy(seg).to(backend), 2, bound=_bound())
    assert shares[0][0] < 1.0


def test_without_a_halo_every_list_is_the_whole_level(backend):
    v = _voxels(buffer=0.0)
    assert v["mask"].all()
    shares, _ = _check_lists(v["coords"].astype(np.int32), v["mask"].astype(np.uint8), backend, bound=_bound(0.0))
    assert all(s == (1.0, 1.0, 1.0) for s in shares), shares


def test_lists_at_coordinates_0_and_bound_minus_1(backend):
    """Hand-made: two blocks filled at random up to both faces of the grid, inner boxes that touch coordinate 0 (block 0) and
    bound - 1 (block 1), so margins are taken across the whole grid and the boxes halve at both ends."""
    rng = np.random.RandomState(3)
    bound = 27  # odd: level boxes with an odd upper end
    cells = np.stack(np.meshgrid(*[np.arange(bound)] * 3, indexing="ij"), -1).reshape(-1, 3)
    parts, masks = [], []
    for b, (blo, bhi) in enumerate(((0, 9), (19, bound - 1))):
        c = cells[rng.rand(len(cells)) < 0.15]
        c = np.unique(np.concatenate([c, [[0, 0, 0], [bound - 1] * 3]]), axis=0)
        parts.append(np.concatenate([np.full((len(c), 1), b), c], 1))
        masks.append(((c >= blo) & (c <= bhi)).all(1))
    coords, mask = np.concatenate(parts).astype(np.int32), np.concatenate(masks).astype(np.uint8)
    assert mask[0] == 1 and mask[-1] == 1  # (0, 0, 0) of block 0 and (bound - 1,) * 3 of block 1 are inner rows
    shares, _ = _check_lists(coords, mask, backend, bound=bound)
    assert shares[0][0] < 0.5 and shares[1][0] < 1.0


# ---- the network ----------------------------------------------------------------------------------------------------------------
def _inference(backend, fp16=False, **kw):
    mi = ModelInference("unused", WEIGHTS, voxel_size=VOXEL, block_size=BLOCK, buffer_size=BUFFER, device=backend, fp16=fp16, **kw)
    if backend.type == "cpu":  # (the matrix-core kernels cost a fiber rendezvous per instruction on the CPU build; the vector
        mi.model.use_mfma = fp16  # kernels take the same lists -- half storage has matrix-core kernels only)
    return mi


def _cloud(backend, trees):
    t = lambda a: torch.from_numpy(a).to(backend)
    clouds = [Cloud(xyz=t(xyz), rgb=t(rgb)) for xyz, rgb in trees]
    return clouds[0] if len(clouds) == 1 else Cloud.collate(clouds)


def _same_on_the_mask(pruned, full):
    m = pruned._mask  # (MaskedCloud: the labelled cloud of every voxel and the pending inner-block mask)
    assert torch.equal(m, full._mask) and 0 < int(m.sum()) < m.numel()
    a, b = pruned._base, full._base
    assert torch.equal(a.medial_vector[m], b.medial_vector[m]) and torch.equal(a.class_l[m], b.class_l[m])
    assert torch.isfinite(a.medial_vector[m]).all()
    assert not a.medial_vector[~m].any() and not a.class_l[~m].any()  # rows off the mask: zero
    assert b.medial_vector[~m].any()  # (... which they are not without pruning: the comparison above is not of zeros)


def _pruned_against_full(backend, trees, fp16=False):
    cloud = _cloud(backend, trees)
    out = {prune: _inference(backend, fp16=fp16, prune_halo=prune).forward(cloud) for prune in (True, False)}
    _same_on_the_mask(out[True], out[False])


@pytest.mark.parametrize("case", ["one", "three"])
def test_pruned_rows_on_the_mask_have_the_same_bits(backend, case):
    """ModelInference with and without pruning: torch.equal medial vectors and classes on the mask rows, zeros off them.  One cloud
    and a batch of three."""
    _pruned_against_full(backend, [_tree()] if case == "one" else [_tree(), _tree(1500, 5, 0.25), _tree(1500, 7, 0.25)])


@pytest.mark.gpu
def test_pruned_rows_have_the_same_bits_in_half_storage():
    """The half-precision storage mode (on the GPU only: its matrix-core kernels run a fiber rendezvous per instruction on the
    CPU build, and the list launches of the float32 matrix-core kernels are the same code)."""
    _pruned_against_full(torch.device("cuda:0"), [_tree()], fp16=True)


def _sparse_input(backend, v, hint=True):
    nb = int(v["coords"][:, 0].max()) + 1
    return sparse_from_batch(torch.from_numpy(v["feats"][:, :3].copy()).to(backend), torch.from_numpy(v["coords"].astype(np.int32)).to(backend),
                             device=backend, brick_hint=(nb, _bound()) if hint else None)


def test_forward_with_a_mask_and_no_read_of_a_row_left_out(backend, monkeypatch):
    """Smart_Tree.forward with the mask (one block without an inner row) against without: equal radius, direction and class_l on
    the mask rows.  Then the same pruned pass with every convolution output starting as NaN: a read of a row that a list launch
    left out would reach a mask row -- they are unchanged and finite."""
    v = _voxels()
    _, mask = _no_inner_block(v)
    net = _inference(backend).model
    sp = _sparse_input(backend, v)
    m = torch.from_numpy(mask).to(backend)
    full, pruned = net.forward(sp), net.forward(sp, m)
    monkeypatch.setattr(ops, "POISON_OUTPUTS", True)
    poisoned = net.forward(sp, m)
    keep = m.bool()
    for k in ("radius", "direction", "class_l"):
        assert torch.equal(pruned[k][keep], full[k][keep]), k
        assert torch.equal(poisoned[k][keep], full[k][keep]) and torch.isfinite(poisoned[k][keep]).all(), k
        assert not pruned[k][~keep].any() and full[k][~keep].any(), k  # rows off the mask: zero, the last block's among them


def test_modes_that_do_not_prune(backend):
    """return_masked=False, a trace, blocking="whole" and the hash-table pyramid compute every row: equal to the unpruned outputs."""
    cloud = _cloud(backend, [_tree(2000, SEED, 0.3)])  # (six passes: a smaller tree; what is compared is every row, not the lists)
    ref = _inference(backend, prune_halo=False).forward(cloud, return_masked=False)
    mi = _inference(backend)
    assert mi.prune_halo
    got = mi.forward(cloud, return_masked=False)
    assert torch.equal(got.medial_vector, ref.medial_vector) and torch.equal(got.class_l, ref.class_l)
    mi.model.use_bricks = False  # hash-table builders
    got = mi.forward(cloud)._base
    assert torch.equal(got.medial_vector, ref.medial_vector) and torch.equal(got.class_l, ref.class_l)
    mi.model.use_bricks, mi.model.trace = True, {}
    got = mi.forward(cloud)._base
    assert torch.equal(got.medial_vector, ref.medial_vector) and torch.equal(got.class_l, ref.class_l) and "tail0" in mi.model.trace
    whole = [_inference(backend, blocking="whole", prune_halo=p).forward(cloud)._base for p in (True, False)]
    assert torch.equal(whole[0].medial_vector, whole[1].medial_vector) and whole[0].medial_vector.any(1).all()


@pytest.mark.gpu
def test_pipeline_skeletons_do_not_depend_on_pruning():
    """Pipeline.process_cloud with pruning on and off: identical skeletons (ids, parents, coordinates, radii)."""
    dev = torch.device("cuda:0")
    c = sample_tree_cloud(50000, seed=11, scale=0.8, max_depth=4)
    cloud = Cloud(xyz=torch.from_numpy(c["xyz"]).to(dev), rgb=torch.from_numpy(c["rgb"]).to(dev))
    skeletons = []
    for prune in (True, False):
        mi = ModelInference("unused", WEIGHTS, voxel_size=0.02, block_size=4, buffer_size=0.4, device=dev, prune_halo=prune)
        sk = Skeletonizer(K=16, min_connection_length=0.02, minimum_graph_vertices=32, device=dev)
        pipe = Pipeline(AugmentationPipeline([CentreCloud()]), mi, sk, repair_skeletons=True, smooth_skeletons=True, smooth_kernel_size=11,
                        prune_skeletons=True, min_skeleton_radius=0.01, min_skeleton_length=0.02, device=dev)
        skeletons.append(pipe.process_cloud(cloud=cloud).skeletons)
    a, b = skeletons
    assert len(a) == len(b) > 0
    for x, y in zip(a, b):
        assert sorted(x.branches) == sorted(y.branches) and len(x.branches) > 0
        for k in x.branches:
            assert x.branches[k].parent_id == y.branches[k].parent_id
            assert torch.equal(x.branches[k].xyz, y.branches[k].xyz) and torch.equal(x.branches[k].radii, y.branches[k].radii)
