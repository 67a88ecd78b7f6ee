"""Loss backward (st_loss_backward, smart_tree_amd/model/loss.py `_LossFn`) against float64 autograd of the reference's expressions
(smart_tree/model/loss.py:7-97, restated as in oracle/loss_oracle.py), on the CPU sanitizer build and on the GPU."""
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from smart_tree_amd.model import loss as L

GOLDEN = Path(__file__).parent / "golden"
CASES = {"plain": dict(mask=False, vector_class=None, target_radius_log=True),
         "masked": dict(mask=True, vector_class=None, target_radius_log=True),
         "masked_vector0": dict(mask=True, vector_class=0, target_radius_log=True),
         "vector1_rawradius": dict(mask=False, vector_class=1, target_radius_log=False)}
WEIGHTS = (0.7, 1.3, 0.4)  # upstream gradients of the radius, direction and class terms
TOL = 1e-5  # |g - g64| <= TOL * max |g64| of the tensor (+ 1e-4 relative)


def _inputs(device):
    g = np.load(GOLDEN / "loss_vectors.npz")
    t = lambda k: torch.from_numpy(np.ascontiguousarray(g[k])).float().to(device)
    return t("radius"), t("direction"), t("class_l"), t("targets"), torch.from_numpy(g["mask"]).to(device)


def _reference(radius, direction, class_l, targets, mask, vector_class, target_radius_log, cls):
    """float64 autograd of the reference's compute_loss with L1 / cosine (norms clamped at 1e-8) / focal or dice."""
    r, d, c = (x.detach().double().cpu().requires_grad_(True) for x in (radius, direction, class_l))
    t = targets.double().cpu()
    t_class, t_dir, t_rad = t[:, 4].long(), t[:, 1:4], t[:, 0]
    rs, ds, cs = r.view(-1), d, c
    if mask is not None:
        m = mask.cpu()
        rs, ds, cs, t_class, t_dir, t_rad = rs[m], ds[m], cs[m], t_class[m], t_dir[m], t_rad[m]
    tc_all = t_class
    if vector_class is not None:
        vm = t_class == vector_class
        rs, ds, t_dir, t_rad = rs[vm], ds[vm], t_dir[vm], t_rad[vm]
    if target_radius_log:
        t_rad = torch.log(t_rad)
    l1 = (rs - t_rad).abs().mean()
    cos = ((ds / ds.norm(dim=1, keepdim=True).clamp_min(1e-8)) * (t_dir / t_dir.norm(dim=1, keepdim=True).clamp_min(1e-8))).sum(1)
    lcos = (1 - cos).mean()
    if cls == "focal":
        logpt = F.log_softmax(cs, dim=1).gather(1, tc_all.view(-1, 1)).view(-1)
        lcls = (-1 * (1 - logpt.exp()) ** 2 * logpt).mean()
    else:
        p = F.softmax(cs, dim=1)
        oh = F.one_hot(tc_all, cs.shape[1]).double()
        lcls = 1 - (2.0 * (p * oh).sum() + 1) / (p.sum() + oh.sum() + 1)
    (WEIGHTS[0] * l1 + WEIGHTS[1] * lcos + WEIGHTS[2] * lcls).backward()
    return (l1, lcos, lcls), (r.grad, d.grad, c.grad)


def _close(got, ref, what):
    got, ref = got.detach().double().cpu(), ref.double()
    scale = float(ref.abs().max()) if ref.numel() else 0.0
    err = (got - ref).abs()
    bad = err > TOL * scale + 1e-4 * ref.abs()
    assert not bool(bad.any()), f"{what}: worst {float(err.max()):.3g} at scale {scale:.3g}"


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("cls", ["focal", "dice"])
def test_loss_backward_matches_float64_autograd(backend, case, cls):
    radius, direction, class_l, targets, mask = _inputs(backend)
    kw = CASES[case]
    m = mask if kw["mask"] else None
    preds = {k: v.clone().requires_grad_(True) for k, v in (("radius", radius), ("direction", direction), ("class_l", class_l))}
    res = L.compute_loss(preds, targets, m, L.L1Loss, L.cosine_similarity_loss, L.focal_loss if cls == "focal" else L.dice_loss,
                         target_radius_log=kw["target_radius_log"], vector_class=kw["vector_class"])
    assert all(v.requires_grad for v in res.values())
    (WEIGHTS[0] * res["radius"] + WEIGHTS[1] * res["direction"] + WEIGHTS[2] * res["class_l"]).backward()
    vals, grads = _reference(radius, direction, class_l, targets, m, kw["vector_class"], kw["target_radius_log"], cls)
    np.testing.assert_allclose([float(res[k].detach()) for k in ("radius", "direction", "class_l")], [float(v.detach()) for v in vals], rtol=1e-5)
    for name, ref in zip(("radius", "direction", "class_l"), grads):
        _close(preds[name].grad, ref, f"{case}/{cls}: d {name}")


@pytest.mark.parametrize("fn", ["L1Loss", "cosine_similarity_loss", "focal_loss", "dice_loss"])
def test_single_loss_functions_backward(backend, fn):
    """The functions on their own (as the reference's compute_loss would call them with other partners)."""
    radius, direction, class_l, targets, _ = _inputs(backend)
    if fn == "L1Loss":
        x, t = radius.view(-1).clone().requires_grad_(True), torch.log(targets[:, 0])
        ref = lambda a: (a - t.double().cpu()).abs().mean()
    elif fn == "cosine_similarity_loss":
        x, t = direction.clone().requires_grad_(True), targets[:, 1:4]
        tq = t.double().cpu()
        ref = lambda a: (1 - ((a / a.norm(dim=1, keepdim=True).clamp_min(1e-8)) * (tq / tq.norm(dim=1, keepdim=True).clamp_min(1e-8))).sum(1)).mean()
    else:
        x, t = class_l.clone().requires_grad_(True), targets[:, 4].long()
        tl = t.cpu()
        if fn == "focal_loss":
            ref = lambda a: (-(1 - F.log_softmax(a, 1).gather(1, tl.view(-1, 1)).exp()) ** 2 * F.log_softmax(a, 1).gather(1, tl.view(-1, 1))).mean()
        else:
            ref = lambda a: 1 - (2.0 * (F.softmax(a, 1) * F.one_hot(tl, 2)).sum() + 1) / (F.softmax(a, 1).sum() + tl.numel() + 1)
    out = getattr(L, fn)(x, t)
    (2.5 * out).backward()
    x64 = x.detach().double().cpu().requires_grad_(True)
    v64 = ref(x64)
    (2.5 * v64).backward()
    assert abs(float(out.detach()) - float(v64.detach())) <= 1e-5 * max(abs(float(v64.detach())), 1e-3)
    _close(x.grad, x64.grad, fn)


def test_values_without_grad_are_unchanged(backend):
    """Predictions that require grad give the same loss values, bit for bit, as the forward-only path; without grad (or under
    no_grad) the results carry no graph, as before."""
    radius, direction, class_l, targets, mask = _inputs(backend)
    for cls in (L.focal_loss, L.dice_loss):
        kw = dict(radius_loss_fn=L.L1Loss, direction_loss_fn=L.cosine_similarity_loss, class_loss_fn=cls, vector_class=0)
        plain = L.compute_loss({"radius": radius, "direction": direction, "class_l": class_l}, targets, mask, **kw)
        preds = {"radius": radius.clone().requires_grad_(True), "direction": direction.clone().requires_grad_(True),
                 "class_l": class_l.clone().requires_grad_(True)}
        graph = L.compute_loss(preds, targets, mask, **kw)
        with torch.no_grad():
            nograd = L.compute_loss(preds, targets, mask, **kw)
        for k in plain:
            assert plain[k].dtype == torch.float32 and plain[k].dim() == 0 and not plain[k].requires_grad
            assert not nograd[k].requires_grad and graph[k].requires_grad
            assert torch.equal(plain[k], graph[k].detach()) and torch.equal(plain[k], nograd[k])


def test_loss_backward_gradient_is_deterministic(backend):
    radius, direction, class_l, targets, mask = _inputs(backend)
    out = []
    for _ in range(2):
        preds = {k: v.clone().requires_grad_(True) for k, v in (("radius", radius), ("direction", direction), ("class_l", class_l))}
        res = L.compute_loss(preds, targets, mask, L.L1Loss, L.cosine_similarity_loss, L.focal_loss, vector_class=0)
        sum(res.values()).backward()
        out.append([preds[k].grad for k in ("radius", "direction", "class_l")])
    for a, b in zip(*out):
        assert torch.equal(a, b)
