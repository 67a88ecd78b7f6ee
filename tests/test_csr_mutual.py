"""st_component_csr_knn on hand-built neighbour tables: the mutual-pair test (one packed int32 row of the other endpoint per
edge) against the rule written out in numpy and against the library's own edge-list build (st_component_csr's rows through the
small-workspace fall-back, de-duplicated per pair).  The C oracle (oracle/skeleton_oracle.c) has no adjacency of its own: its
graph checks go through tests/test_skeleton.py, which stay as they are."""
import numpy as np
import pytest
import torch

from smart_tree_amd import _lib


def _table(kind, n, K, rng):
    """idx [n,K] int64 (no vertex twice in a row), first_of [n] or None, new_id [n], m."""
    idx = np.full((n, K), -1, dtype=np.int64)
    first_of, keep = None, np.ones(n, dtype=bool)
    ring = lambda i, s: (i + s) % n
    if kind == "all_mutual":  # i lists i +- 1 .. i +- K/2 on a ring: every pair from both sides
        for i in range(n):
            nb = [ring(i, s) for h in range(1, K // 2 + 1) for s in (h, -h)][:K]
            nb = list(dict.fromkeys(j for j in nb if j != i))
            idx[i, :len(nb)] = nb
        if K == 1:  # pairs (2t, 2t + 1)
            idx[:, 0] = [i ^ 1 if (i ^ 1) < n else -1 for i in range(n)]
    elif kind == "none_mutual":  # forward only: i lists i + 1 .. i + K (no wrap)
        for i in range(n):
            nb = [j for j in range(i + 1, min(i + 1 + K, n))]
            idx[i, :len(nb)] = nb
    elif kind == "padding":  # random rows, each cut short by -1 entries
        for i in range(n):
            cand = [j for j in rng.permutation(n)[:K] if j != i]
            cand = cand[:rng.randint(0, len(cand) + 1)]
            idx[i, :len(cand)] = cand
    elif kind == "self":  # the row starts with the vertex itself (as a search over its own set returns it)
        for i in range(n):
            cand = [i] + [j for j in rng.permutation(n)[:K] if j != i]
            idx[i, :min(K, len(cand))] = cand[:K]
    elif kind == "first_of":  # two clouds; entries at or below the cloud's first vertex are not edges
        cut = n // 2
        first_of = np.where(np.arange(n) < cut, 0, cut).astype(np.int32)
        for i in range(n):
            lo, hi = (0, max(cut, 1)) if i < cut else (cut, n)
            cand = [j for j in (lo + rng.permutation(hi - lo))[:K] if j != i]
            if cand and rng.rand() < 0.5:
                cand[0] = lo  # the first vertex itself
            cand = list(dict.fromkeys(cand))
            idx[i, :len(cand)] = cand
    elif kind == "dropped":  # a third of the vertices is not kept
        keep = rng.rand(n) < 0.66
        for i in range(n):
            cand = [j for j in rng.permutation(n)[:K] if j != i]
            idx[i, :len(cand)] = cand
    elif kind == "last_slot":  # i lists i + 1 first; i + 1 lists i in its LAST slot, behind K - 1 others
        for i in range(n):
            others = [j for j in rng.permutation(n) if j not in (i, i - 1, i + 1)][:K]
            row = ([i + 1] if i + 1 < n else []) + others
            row = row[:K]
            if i > 0 and len(row) == K:
                row[K - 1] = i - 1
            elif i > 0:
                row.append(i - 1)
            row = list(dict.fromkeys(row))
            idx[i, :len(row)] = row
    new_id = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)
    return idx, first_of, new_id, int(keep.sum())


def _weights(idx):
    """dist [n,K]: a symmetric function of the pair, so both copies of a mutual pair carry the same float."""
    i = np.arange(idx.shape[0])[:, None].astype(np.int64)
    a, b = np.minimum(i, idx), np.maximum(i, idx)
    return (0.5 + ((a * 131 + b * 17) % 1009) / 1009.0).astype(np.float32)


def _rule(idx, dist, first_of, new_id, m):
    n, K = idx.shape
    rows = [[] for _ in range(m)]
    for i in range(n):
        x, first = new_id[i], (0 if first_of is None else int(first_of[i]))
        if x < 0:
            continue
        for k in range(K):
            j = int(idx[i, k])
            if j > first and j != i and new_id[j] >= 0:
                rows[x].append((int(new_id[j]), float(dist[i, k])))
                if not (i > first and i in idx[j]):
                    rows[new_id[j]].append((int(x), float(dist[i, k])))
    return rows


def _run(backend, idx, dist, first_of, new_id, m, small_ws):
    L = _lib.lib()
    n, K = idx.shape
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(backend)
    row_off = torch.zeros(m + 1, dtype=torch.int32, device=backend)
    col = torch.zeros(max(2 * n * K, 1), dtype=torch.int32, device=backend)
    wgt = torch.zeros(max(2 * n * K, 1), dtype=torch.float32, device=backend)
    nbytes = L.st_component_csr_workspace_bytes(m) if small_ws else L.st_component_csr_knn_workspace_bytes(m, n, K)
    ws = _lib.workspace(nbytes, backend)
    di, dd, df, dn = t(idx), t(dist), t(first_of), t(new_id)
    _lib.check(L.st_component_csr_knn(_lib.ptr(di), _lib.ptr(dd), n, K, _lib.ptr(df), _lib.ptr(dn), m, _lib.ptr(row_off),
                                      _lib.ptr(col), _lib.ptr(wgt), _lib.ptr(ws), ws.numel(), _lib.stream(backend)))
    if backend.type == "cuda":
        torch.cuda.synchronize()
    ro, c, w = row_off.cpu().numpy().astype(np.int64), col.cpu().tolist(), wgt.cpu().tolist()
    return ro, [list(zip(c[ro[v]: ro[v + 1]], w[ro[v]: ro[v + 1]])) for v in range(m)]


KINDS = ["all_mutual", "none_mutual", "padding", "self", "first_of", "dropped", "last_slot"]


@pytest.mark.parametrize("K", [1, 2, 16, 64])
@pytest.mark.parametrize("n", [1, 17, 300])
def test_rows_from_tables_keep_every_pair_once(backend, n, K):
    rng = np.random.RandomState(1000 * K + n)
    for kind in KINDS:
        idx, first_of, new_id, m = _table(kind, n, K, rng)
        if m == 0:
            continue
        dist = _weights(idx)
        want = _rule(idx, dist, first_of, new_id, m)
        ro, rows = _run(backend, idx, dist, first_of, new_id, m, small_ws=False)
        want_off = np.concatenate([[0], np.cumsum([len(r) for r in want])])
        np.testing.assert_array_equal(ro, want_off, err_msg=kind)
        _, both = _run(backend, idx, dist, first_of, new_id, m, small_ws=True)  # the edge-list build: mutual pairs twice
        for v in range(m):
            assert sorted(rows[v]) == sorted(want[v]), (kind, v)
            assert sorted(rows[v]) == sorted(set(both[v])), (kind, v)
            fwd = [(int(new_id[j]), float(dist[np.flatnonzero(new_id == v)[0], k]))
                   for k, j in enumerate(idx[np.flatnonzero(new_id == v)[0]])
                   if j > (0 if first_of is None else first_of[np.flatnonzero(new_id == v)[0]])
                   and j != np.flatnonzero(new_id == v)[0] and new_id[j] >= 0]
            assert rows[v][:len(fwd)] == fwd, (kind, v)  # forward entries first, in table order
    # the cases do what their names say
    idx, first_of, new_id, m = _table("all_mutual", 17, 16, rng) if n == 17 and K == 16 else (None, None, None, 0)
    if m:
        assert all(i in idx[j] for i in range(17) for j in idx[i] if j >= 0)
