"""numpy restatement of st_prediction_metrics (csrc/prediction_metrics.hip): `evaluate(..., dtype=np.float64)` is the oracle,
`dtype=np.float32` mirrors the kernel's float32 order of operations (numpy evaluates float32 expressions one rounding per
operation, no contraction).  Both take the float32 inputs the kernel takes.  The sums are float64 sums of the per-row terms in
either case.  "Finite" means representable in float32 for both, so that an `expf` overflow is a bad row in the oracle too.

`assert_margins` is the condition under which an ulp of difference in the device's expf / acosf cannot flip a count: no row's
medial error within 1e-4 relative of a threshold, no target radius within 1e-4 relative of a bin edge, no two logits of a row
closer than 1e-4 unless bit-equal.
"""
import numpy as np

N_SCALARS, N_SUMS = 4, 5
FLT_MAX = float(np.finfo(np.float32).max)


def _rows(radius, direction, class_l, targets, target_radius_log, dtype):
    """Per-row quantities for every row (selection is applied by the caller)."""
    f = dtype
    radius, direction, class_l, targets = (np.asarray(a, dtype=np.float32) for a in (radius, direction, class_l, targets))
    n, C = class_l.shape
    with np.errstate(all="ignore"):
        tcf = targets[:, 4]
        tc_ok = (tcf > -1.0) & (tcf < C)
        tc = np.where(tc_ok, np.trunc(np.where(tc_ok, tcf, 0.0)), -1).astype(np.int64)
        isn = np.isnan(class_l)
        pc = np.where(isn.any(1), isn.argmax(1), np.argmax(np.where(isn, -np.inf, class_l), 1)) if n else np.zeros(0, np.int64)
        r_gt = targets[:, 0].astype(f)
        r_in = radius.reshape(-1).astype(f)
        r_pred = np.exp(r_in) if target_radius_log else r_in
        dr = np.abs(r_pred - r_gt)
        p, q = direction.astype(f), targets[:, 1:4].astype(f)
        eps = f(np.float32(1e-8))
        n_p = np.fmax(np.sqrt(p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1] + p[:, 2] * p[:, 2]), eps)
        n_q = np.fmax(np.sqrt(q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2]), eps)
        u, h = p / n_p[:, None], q / n_q[:, None]
        cs = u[:, 0] * h[:, 0] + u[:, 1] * h[:, 1] + u[:, 2] * h[:, 2]
        cs = np.where(cs < f(-1), f(-1), np.where(cs > f(1), f(1), cs))  # a NaN stays
        ang = np.arccos(cs)
        e = r_pred[:, None] * u - r_gt[:, None] * h
        err = np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])
        dr_rel, err_rel = dr / r_gt, err / r_gt
        finite = np.ones(n, dtype=bool)
        for x in (dr, dr_rel, ang, err, err_rel):
            finite &= np.abs(x) <= FLT_MAX  # False for NaN
    assert all(x.dtype == f for x in (dr, dr_rel, ang, err, err_rel))
    return dict(tc_ok=tc_ok, tc=tc, pc=pc.astype(np.int64), r_gt=r_gt, dr=dr, dr_rel=dr_rel, ang=ang, err=err, err_rel=err_rel,
                finite=finite)


def evaluate(radius, direction, class_l, targets, mask=None, seg_off=None, vector_class=None, target_radius_log=True,
             thresholds=(), radius_edges=(), dtype=np.float64):
    """{"ints": int64 [n_seg, C*C + 4 + T + NB], "sums": float64 [n_seg, 5 + 2 NB]} in the kernel's record layout."""
    class_l = np.asarray(class_l, dtype=np.float32)
    n, C = class_l.shape
    R = _rows(radius, direction, class_l, targets, target_radius_log, dtype)
    thr = np.asarray(thresholds, dtype=np.float32).astype(dtype)
    edges = np.asarray(radius_edges, dtype=np.float32).astype(dtype)
    T, NB = len(thr), len(edges) + 1
    seg_off = [0, n] if seg_off is None else list(seg_off)
    sel = np.ones(n, dtype=bool) if mask is None else np.asarray(mask).astype(bool)
    ints = np.zeros((len(seg_off) - 1, C * C + N_SCALARS + T + NB), dtype=np.int64)
    sums = np.zeros((len(seg_off) - 1, N_SUMS + 2 * NB), dtype=np.float64)
    for s in range(len(seg_off) - 1):
        inside = np.zeros(n, dtype=bool)
        inside[seg_off[s]:seg_off[s + 1]] = True
        S = sel & inside
        cls = S & R["tc_ok"]
        vec = cls & (R["tc"] == vector_class if vector_class is not None and vector_class >= 0 else True)
        ok = vec & R["finite"]
        ints[s, :C * C] = np.bincount(R["tc"][cls] * C + R["pc"][cls], minlength=C * C)
        ints[s, C * C:C * C + N_SCALARS] = [(S & ~R["tc_ok"]).sum(), ok.sum(), (vec & ~R["finite"]).sum(), S.sum()]
        r_gt, err = R["r_gt"][ok], R["err"][ok]
        for j in range(T):
            ints[s, C * C + N_SCALARS + j] = (err <= thr[j] * r_gt).sum()
        which = (r_gt[:, None] >= edges[None, :]).sum(1)
        ints[s, C * C + N_SCALARS + T:] = np.bincount(which, minlength=NB)
        for k, key in enumerate(("dr", "dr_rel", "ang", "err", "err_rel")):
            sums[s, k] = R[key][ok].astype(np.float64).sum()
        for b in range(NB):
            sums[s, N_SUMS + b] = R["dr_rel"][ok][which == b].astype(np.float64).sum()
            sums[s, N_SUMS + NB + b] = R["err_rel"][ok][which == b].astype(np.float64).sum()
    return {"ints": ints, "sums": sums}


def margin_violations(radius, direction, class_l, targets, target_radius_log, thresholds, radius_edges, rel=1e-4):
    """Rows (bool [n]) that break a condition of the module docstring, judged in float64 on the rows whose terms are finite."""
    R = _rows(radius, direction, class_l, targets, target_radius_log, np.float64)
    class_l = np.asarray(class_l, dtype=np.float32)
    bad = np.zeros(class_l.shape[0], dtype=bool)
    with np.errstate(all="ignore"):
        for t in np.asarray(thresholds, dtype=np.float32).astype(np.float64):
            lim = t * R["r_gt"]
            bad |= R["finite"] & (np.abs(R["err"] - lim) <= rel * np.abs(lim))
        for e in np.asarray(radius_edges, dtype=np.float32).astype(np.float64):
            bad |= R["finite"] & (np.abs(R["r_gt"] - e) <= rel * abs(e))
        for a in range(class_l.shape[1]):
            for b in range(a + 1, class_l.shape[1]):
                za, zb = class_l[:, a], class_l[:, b]
                bad |= (np.abs(za.astype(np.float64) - zb.astype(np.float64)) < rel) & (za.view(np.uint32) != zb.view(np.uint32))
    return bad


def assert_margins(*args, **kw):
    bad = margin_violations(*args, **kw)
    assert not bad.any(), f"{int(bad.sum())} rows sit on a decision boundary (first: {np.flatnonzero(bad)[:5]})"
