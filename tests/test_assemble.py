"""st_assemble_branches (k_asm_trees / k_asm_branches / k_asm_geometry, csrc/postprocess.hip) on synthetic component tables,
against a numpy restatement of the layout it documents (skeleton/path.py:128-133 for every tree at once): exact equality of
tree_off, parent, start, length, xyz, rad and both counts; nothing written outside what the call owns."""
import ctypes

import numpy as np
import pytest
import torch

from smart_tree_amd import _lib

ST_ERR_INVALID, ST_ERR_WORKSPACE = -1, -2
I_GUARD, F_GUARD = -777, -7777.0  # what every output holds before the call


def _components(rng, C):
    """C components of 0-3 branches of 2-4 vertices; none at the front, in the middle and at the end.  Component c owns the slot
    range [comp_off[c], comp_off[c] + m_c) of the branch table, of path_verts and of vert_order alike (m_c vertices)."""
    n_br = rng.integers(1, 4, C)
    if C >= 3:
        n_br[[0, C // 2, C - 1]] = 0
        n_br[rng.random(C) < 0.1] = 0
    elif C == 2:
        n_br[:] = (0, 2)
    lens = [rng.integers(2, 5, n) for n in n_br]
    m_c = np.array([max(1, int(l.sum())) + int(rng.integers(0, 3)) for l in lens])
    comp_off = np.concatenate([[0], np.cumsum(m_c)])
    m = int(comp_off[-1])
    bpar, boff, blen, pverts = (np.zeros(m, np.int32) for _ in range(4))
    for c in range(C):
        base, n = comp_off[c], n_br[c]
        blen[base: base + n] = lens[c]
        boff[base: base + n] = np.cumsum(lens[c]) - lens[c]
        bpar[base: base + n] = [int(rng.integers(-1, i)) if i else -1 for i in range(n)]
        pverts[base: base + int(lens[c].sum())] = rng.integers(0, m_c[c], int(lens[c].sum()))
    vorder = np.concatenate([comp_off[c] + rng.permutation(m_c[c]) for c in range(C)])
    vorder = rng.permutation(m + 50)[vorder]  # ids into a cloud larger than the kept vertices, component ranges scattered in it
    return dict(C=C, m=m, comp_off=comp_off[:-1].astype(np.int32), n_br=n_br.astype(np.int32), bpar=bpar, boff=boff, blen=blen,
                pverts=pverts, vorder=vorder.astype(np.int32), medial=rng.normal(0, 1, (m + 50, 3)).astype(np.float32),
                radius=rng.uniform(0.01, 0.1, m + 50).astype(np.float32))


def _reference(t):
    tree_off = np.concatenate([[0], np.cumsum(t["n_br"])]).astype(np.int32)
    parent, start, length, ids = [], [], [], []
    slot = 0
    for c in range(t["C"]):
        base = int(t["comp_off"][c])
        for i in range(t["n_br"][c]):
            s = base + i
            v = t["vorder"][base + t["pverts"][base + t["boff"][s] + np.arange(t["blen"][s])]]
            ids += [v[:1], v]  # slot start[b] repeats the first vertex and radius
            parent.append(t["bpar"][s])
            start.append(slot)
            length.append(t["blen"][s])
            slot += t["blen"][s] + 1
    ids = np.concatenate(ids) if ids else np.zeros(0, np.int64)
    i32 = lambda a: np.asarray(a, np.int32)
    return dict(tree_off=tree_off, parent=i32(parent), start=i32(start), length=i32(length), xyz=t["medial"][ids], rad=t["radius"][ids],
                B=len(parent), P=slot)


def _call(t, dev, cap_b, cap_p, wait=True, guard=64, ws_short=0, n_comp=None):
    """Outputs are `guard` elements longer than the capacities the call is told, and pre-filled."""
    L = _lib.lib()
    dv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    ins = [dv(t[k]) for k in ("comp_off", "n_br", "bpar", "boff", "blen", "pverts", "vorder", "medial", "radius")]
    ints = lambda n: torch.full((n,), I_GUARD, dtype=torch.int32, device=dev)
    out = dict(tree_off=ints(t["C"] + 1 + guard), parent=ints(cap_b + guard), start=ints(cap_b + guard), length=ints(cap_b + guard),
               xyz=torch.full((cap_p + guard, 3), F_GUARD, dtype=torch.float32, device=dev),
               rad=torch.full((cap_p + guard,), F_GUARD, dtype=torch.float32, device=dev))
    need = L.st_assemble_workspace_bytes(cap_b)
    ws = _lib.workspace(need, dev)
    counts = (ctypes.c_int64 * 2)(-5, -5) if wait else None
    rc = (L.st_assemble_branches if wait else L.st_assemble_branches_nowait)(
        t["C"] if n_comp is None else n_comp, *(_lib.ptr(x) for x in ins), *(_lib.ptr(out[k]) for k in ("tree_off", "parent", "start", "length", "xyz", "rad")),
        cap_b, cap_p, counts, _lib.ptr(ws), need - ws_short, _lib.stream(dev))
    err = L.st_last_error().decode()
    return rc, err, (None if counts is None else (counts[0], counts[1])), {k: v.cpu().numpy() for k, v in out.items()}


def _check(out, ref, C, cap_b, cap_p, B=None, P=None):
    """The first B branches / P slots equal the reference (default: all of them), everything behind them is untouched -- except
    start, which is a scan over the whole capacity: the unused entries hold the slot total."""
    B, P = ref["B"] if B is None else B, ref["P"] if P is None else P
    np.testing.assert_array_equal(out["tree_off"][: C + 1], ref["tree_off"])
    for k in ("parent", "length"):
        np.testing.assert_array_equal(out[k][:B], ref[k][:B])
        assert (out[k][B:] == I_GUARD).all()
    np.testing.assert_array_equal(out["start"][:B], ref["start"][:B])
    slots = int(ref["start"][B - 1] + ref["length"][B - 1] + 1) if B else 0
    assert (out["start"][B:cap_b] == slots).all() and (out["start"][cap_b:] == I_GUARD).all()
    assert (out["tree_off"][C + 1:] == I_GUARD).all()
    np.testing.assert_array_equal(out["xyz"][:P], ref["xyz"][:P])
    np.testing.assert_array_equal(out["rad"][:P], ref["rad"][:P])
    assert (out["xyz"][P:] == F_GUARD).all() and (out["rad"][P:] == F_GUARD).all()


@pytest.mark.parametrize("capacity", ["exact", "product", "large"])
@pytest.mark.parametrize("C", [1, 2, 1023, 1024, 1025, 2500])  # k_asm_trees scans 1024 components per pass and carries the total
def test_assemble_matches_the_layout(backend, C, capacity):
    t = _components(np.random.default_rng(C), C)
    ref = _reference(t)
    assert ref["B"] == t["n_br"].sum() and ref["P"] == ref["B"] + sum(ref["length"]) and ref["P"] < 40000
    cap_b, cap_p = {"exact": (ref["B"], ref["P"]), "product": (t["m"], 2 * t["m"]), "large": (4 * t["m"] + 1000, 8 * t["m"] + 1000)}[capacity]
    for wait in (True, False):  # with the count read-back / the enqueue-only form: the same arrays
        rc, err, counts, out = _call(t, backend, cap_b, cap_p, wait=wait)
        assert rc == 0, err
        assert counts in (None, (ref["B"], ref["P"]))
        _check(out, ref, C, cap_b, cap_p)


def test_assemble_without_components(backend):
    t = _components(np.random.default_rng(5), 5)
    rc, err, counts, out = _call(t, backend, 16, 64, n_comp=0)
    assert rc == 0 and counts == (0, 0)
    assert all((v == (F_GUARD if v.dtype == np.float32 else I_GUARD)).all() for v in out.values())  # nothing was launched


def test_assemble_workspace_too_small(backend):
    t = _components(np.random.default_rng(5), 5)
    rc, err, counts, out = _call(t, backend, t["m"], 2 * t["m"], ws_short=1)
    assert rc == ST_ERR_WORKSPACE and "workspace" in err
    assert all((v == (F_GUARD if v.dtype == np.float32 else I_GUARD)).all() for v in out.values())


@pytest.mark.parametrize("short", ["branches and slots", "slots"])
@pytest.mark.parametrize("C", [2, 1025])
def test_assemble_capacity_exceeded(backend, C, short):
    """One branch / one slot too few: the blocking form refuses and names both counts; either form lays out what fits (the first
    cap_b branches, of their geometry the first cap_p slots) and touches nothing behind the capacities."""
    t = _components(np.random.default_rng(C), C)
    ref = _reference(t)
    cap_b, cap_p = (ref["B"] - 1, ref["P"] - 1) if short == "branches and slots" else (ref["B"], ref["P"] - 1)
    fits_b = min(ref["B"], cap_b)
    fits_p = min(int(ref["start"][fits_b - 1] + ref["length"][fits_b - 1] + 1), cap_p)
    rc, err, counts, out = _call(t, backend, cap_b, cap_p)
    assert rc == ST_ERR_INVALID and counts == (ref["B"], ref["P"])
    assert "capacity" in err and str(ref["B"]) in err and str(ref["P"]) in err
    _check(out, ref, C, cap_b, cap_p, B=fits_b, P=fits_p)
    rc, err, counts, out = _call(t, backend, cap_b, cap_p, wait=False)
    assert rc == 0
    _check(out, ref, C, cap_b, cap_p, B=fits_b, P=fits_p)
