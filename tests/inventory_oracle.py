"""The tree tally and the skeleton metrics of smart_tree_amd/inventory.py, restated in numpy and plain Python (tests only).

The tally follows include/smarttree_hip.h: float32 for the cell arithmetic in the header's operation order, the box through the
order-preserving integer map of the float bits, Python sets for the distinct cells.  The skeleton metrics are float64, tube by tube.
"""
import math

import numpy as np

F = np.float32
MAX_INDEX = 16383


def f2ord(x):
    u = np.asarray(x, F).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def ord2f(u):
    u = np.asarray(u, np.uint32)
    return np.where(u & np.uint32(0x80000000), u & np.uint32(0x7fffffff), ~u).astype(np.uint32).view(F)


def takes_part(pts, tree, n_trees, cls=None, n_classes=1):
    ok = np.isfinite(pts).all(1) & (tree >= 0) & (tree < n_trees)
    if cls is not None:
        ok &= cls < n_classes
    return ok


def tally(pts, tree, n_trees, cls=None, n_classes=1, up=1, cell=0.1, layers=256):
    """{"box" float32 [T,6], "counts" int64 [T,C], "area_cells" int64 [T], "profile" int64 [T,layers]}."""
    pts, tree = np.asarray(pts, F).reshape(-1, 3), np.asarray(tree, np.int64).reshape(-1)
    T, C = int(n_trees), (1 if cls is None else int(n_classes))
    ok = takes_part(pts, tree, T, cls, C)
    lo = np.full((T, 3), f2ord(F(np.inf)), np.uint32)
    hi = np.full((T, 3), f2ord(F(-np.inf)), np.uint32)
    counts = np.zeros((T, C), np.int64)
    o = f2ord(pts)
    for k in range(3):
        np.minimum.at(lo[:, k], tree[ok], o[ok, k])
        np.maximum.at(hi[:, k], tree[ok], o[ok, k])
    np.add.at(counts, (tree[ok], np.zeros(int(ok.sum()), np.int64) if cls is None else np.asarray(cls, np.int64)[ok]), 1)
    box = np.concatenate([ord2f(lo), ord2f(hi)], axis=1)
    area, profile = np.zeros(T, np.int64), np.zeros((T, int(layers)), np.int64)
    if ok.any():
        t = tree[ok]
        with np.errstate(over="ignore"):
            d = (pts[ok] - box[t, :3]).astype(F)            # one float32 subtraction
            q = np.floor((d / F(cell)).astype(F))             # one float32 division, floorf
        idx = np.clip(q, 0, MAX_INDEX).astype(np.int64)
        h0, h1 = (1 if up == 0 else 0), (1 if up == 2 else 2)
        plan, volume = set(), set()
        for tr, i in zip(t.tolist(), idx.tolist()):
            plan.add((tr, i[h0], i[h1]))
            volume.add((tr, i[h0], i[h1], i[up]))
        for tr, _, _ in plan:
            area[tr] += 1
        for tr, _, _, iu in volume:
            profile[tr, min(iu, int(layers) - 1)] += 1
    return {"box": box, "counts": counts, "area_cells": area, "profile": profile}


# ------------------------------------------------------------------------------------------------ skeleton metrics ---
def _dist2_to_segment(p, a, b):
    ab = [b[k] - a[k] for k in range(3)]
    den = sum(x * x for x in ab)
    t = 0.0 if den <= 0 else min(max(sum((p[k] - a[k]) * ab[k] for k in range(3)) / den, 0.0), 1.0)
    return sum((a[k] + t * ab[k] - p[k]) ** 2 for k in range(3))


def branches(tree_branches):
    """`tree_branches`: [(branch id, parent id, xyz [n,3], radii [n])] of ONE tree.  Returns ({id: dict of the branch's metrics},
    [orphan ids])."""
    by_id = {b: (p, np.asarray(x, np.float64).reshape(-1, 3), np.asarray(r, np.float64).reshape(-1)) for b, p, x, r in tree_branches}
    out, orphans = {}, []

    def order(b, seen=()):
        p = by_id[b][0]
        if p == b or p not in by_id or p in seen:
            return 0
        return order(p, seen + (b,)) + 1

    for b, (p, x, r) in by_id.items():
        m = {"parent": p, "order": order(b), "tubes": max(len(x) - 1, 0), "length": 0.0, "volume": 0.0, "area": 0.0}
        weighted = 0.0
        for i in range(len(x) - 1):
            h = math.sqrt(sum((x[i + 1][k] - x[i][k]) ** 2 for k in range(3)))
            r1, r2 = r[i], r[i + 1]
            m["length"] += h
            m["volume"] += math.pi * h * (r1 * r1 + r1 * r2 + r2 * r2) / 3.0
            m["area"] += math.pi * (r1 + r2) * math.sqrt(h * h + (r1 - r2) ** 2)
            weighted += h * (r1 + r2) / 2.0
        m["mean_radius"] = weighted / m["length"] if m["length"] > 0 else float("nan")
        m["base_radius"] = r[0] if len(r) else float("nan")
        m["tip_radius"] = r[-1] if len(r) else float("nan")
        m["angle"] = float("nan")
        has_parent = p != b and p in by_id
        if not has_parent and p != -1 and p != b:
            orphans.append(b)
        if has_parent and len(x) >= 2 and len(by_id[p][1]) >= 2:
            px = by_id[p][1]
            d2 = [_dist2_to_segment(x[0], px[i], px[i + 1]) for i in range(len(px) - 1)]
            near = d2.index(min(d2))
            u, w = x[1] - x[0], px[near + 1] - px[near]
            den = math.sqrt(float(u @ u)) * math.sqrt(float(w @ w))
            if den > 0:
                m["angle"] = math.degrees(math.acos(min(max(float(u @ w) / den, -1.0), 1.0)))
        out[b] = m
    return out, orphans


def radius_at(x, r, level, up=1):
    for i in range(len(x) - 1):
        ua, ub = x[i][up], x[i + 1][up]
        if min(ua, ub) <= level <= max(ua, ub):
            t = (level - ua) / (ub - ua) if ub != ua else 0.0
            return r[i] + t * (r[i + 1] - r[i])
    return float("nan")


def tree(tree_branches, box, counts, area_cells, profile, cell, breast_height=1.3, up=1):
    """The named values of one tree's row from its branches and its rows of the tally."""
    per, orphans = branches(tree_branches)
    n_pts = int(np.sum(counts))
    ends = [x[up] for _, _, xyz, _ in tree_branches for x in np.asarray(xyz, np.float64).reshape(-1, 3)]
    base = float(box[up]) if n_pts else (min(ends) if ends else float("nan"))
    h0, h1 = (1 if up == 0 else 0), (1 if up == 2 else 2)
    out = {"points": n_pts, "base": base,
           "height": float(box[3 + up]) - float(box[up]) if n_pts else float("nan"),
           "crown_width": max(float(box[3 + h0]) - float(box[h0]), float(box[3 + h1]) - float(box[h1])) if n_pts else float("nan"),
           "crown_area": int(area_cells) * cell * cell, "crown_volume": int(np.sum(profile)) * cell * cell * cell,
           "widest_layer_height": (int(np.argmax(profile)) + 0.5) * cell if np.any(profile) else float("nan"),
           "branches": len(per), "max_order": max(m["order"] for m in per.values()),
           "length": sum(m["length"] for m in per.values()), "wood_volume": sum(m["volume"] for m in per.values()),
           "wood_area": sum(m["area"] for m in per.values())}
    for k in range(4):
        out[f"volume_order_{k}"] = sum(m["volume"] for m in per.values() if (m["order"] == k if k < 3 else m["order"] >= 3))
    root = next(b for b, _, _, _ in tree_branches if per[b]["order"] == 0)
    _, _, x, r = next(t for t in tree_branches if t[0] == root)
    out["trunk_length"] = per[root]["length"]
    out["dbh"] = 2.0 * radius_at(np.asarray(x, np.float64).reshape(-1, 3), np.asarray(r, np.float64).reshape(-1), base + breast_height, up)
    return out, per, orphans
