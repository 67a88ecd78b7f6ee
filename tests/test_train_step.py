"""One training step of TrainableSmartTree (smart_tree_amd/model/trainable.py) against tests/golden/train_step.npz, a float64 step of
the reference's own Smart_Tree + compute_loss + backward (tools/make_goldens.py --only train_step): outputs, losses and running
statistics directly; gradients entrywise against a float64 oracle step that is held to the fixture's digest of the reference's
gradients.  Also the state-dict round trip into the inference network, and (GPU) a short Adam run through train_epoch that must lower
the loss."""
import functools
import json
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import unet_oracle as uo
from smart_tree_amd.model import loss as L
from smart_tree_amd.model import train as T
from smart_tree_amd.model.model import Smart_Tree
from smart_tree_amd.model.sparse import batch_collate, sparse_from_batch
from smart_tree_amd.model.trainable import TrainableSmartTree

GOLDEN = Path(__file__).parent / "golden"
WEIGHTS = Path(__file__).resolve().parents[1] / "smart_tree_amd" / "model" / "weights"
OUT_REL = 1e-4  # outputs, relative to the tensor's largest entry
LOSS_TOL = 1e-5  # loss terms, relative
STAT_TOL = 1e-5  # running statistics, relative to the tensor's largest entry
GRAD_REL = 1e-3  # each gradient tensor: |g - g64| <= GRAD_REL * max|g64| ...
GRAD_FLOOR = 1e-6  # ... or this fraction of the case's largest gradient (tensors whose float64 gradient is ~0)
LOSS_FN = functools.partial(L.compute_loss, radius_loss_fn=L.L1Loss, direction_loss_fn=L.cosine_similarity_loss,
                            class_loss_fn=L.focal_loss, target_radius_log=True, vector_class=0)


DIGEST_SAMPLES = 64
DIGEST_TOL = 1e-9  # float64 oracle step against the reference's float64 step: digest entries, relative to the case's largest gradient


def grad_digest(g) -> np.ndarray:
    """float64 [sum, sum |g|, sqrt(sum g^2), max |g|, up to DIGEST_SAMPLES evenly strided entries] of a gradient tensor: what
    tests/golden/train_step.npz keeps of the reference's gradients (tools/make_goldens.py --only train_step)."""
    v = np.asarray(g, np.float64).reshape(-1)
    idx = np.linspace(0, v.size - 1, min(v.size, DIGEST_SAMPLES)).round().astype(np.int64)
    return np.concatenate([[v.sum(), np.abs(v).sum(), np.sqrt((v * v).sum()), np.abs(v).max()], v[idx]])


def _oracle_conv(x0, w, nbr, n_out, nbr_t, flip, x1=None):
    """sparse_grad.sparse_conv in float64 through the oracle's gather-matmul (torch autograd does the backward)."""
    x = x0 if x1 is None else torch.cat([x0, x1], 1)
    table = nbr.cpu().numpy().astype(np.int64) if nbr is not None else np.arange(x.shape[0], dtype=np.int64)[None]
    return uo.sparse_conv(x, table, w.permute(2, 0, 1), n_out)  # [K, Cin, Cout] -> the oracle's [Cout, K, Cin]


def _oracle_pyramid(coords, depth):
    from smart_tree_amd.model.sparse_ops import RulebookPyramid

    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32))
    pyr = RulebookPyramid()
    for level in range(depth + 1):
        pyr.coords.append(t(coords))
        pyr.subm.append(t(uo.subm_rulebook(coords)))
        if level == depth:
            break
        coarse = uo.strided_out_coords(coords)
        pyr.down.append(t(uo.down_rulebook(coarse, coords)))
        pyr.up.append(t(uo.up_rulebook(coords, coarse)))
        coords = coarse
    return pyr


def _oracle_loss(preds, targets, mask):
    """The reference's compute_loss (L1 / cosine / focal, vector_class 0, log target radius) in float64 torch."""
    t = targets[mask]
    tc = t[:, 4].long()
    vm = tc == 0
    r, d, c = preds["radius"][mask].view(-1)[vm], preds["direction"][mask][vm], preds["class_l"][mask]
    t_rad, t_dir = torch.log(t[vm, 0]), t[vm, 1:4]
    cos = ((d / d.norm(dim=1, keepdim=True).clamp_min(1e-8)) * (t_dir / t_dir.norm(dim=1, keepdim=True).clamp_min(1e-8))).sum(1)
    logpt = torch.nn.functional.log_softmax(c, dim=1).gather(1, tc.view(-1, 1)).view(-1)
    return {"radius": (r - t_rad).abs().mean(), "direction": (1 - cos).mean(), "class_l": (-1 * (1 - logpt.exp()) ** 2 * logpt).mean()}


def _oracle_step(g, case, monkeypatch):
    """The same training step in float64 on the CPU: TrainableSmartTree's modules with every convolution replaced by the oracle's
    and the oracle's rulebooks.  Returns {parameter key: float64 gradient}."""
    from smart_tree_amd.model import sparse_grad as sg

    net = TrainableSmartTree.from_state_dict(_case_weights(g, case)).double().train()
    monkeypatch.setattr(sg, "sparse_conv", _oracle_conv)
    pyr = _oracle_pyramid(g["coords"], net.depth)
    x = torch.from_numpy(g["xyz"]).double()
    x = net.input_conv(x, None, x.shape[0], None, False)
    x = net.UNet(x, pyr, 0)
    preds = {"radius": net.radius_head(x), "direction": torch.nn.functional.normalize(net.direction_head(x)), "class_l": net.class_head(x)}
    sum(_oracle_loss(preds, torch.from_numpy(g["targets"]), torch.from_numpy(g["mask"])).values()).backward()
    monkeypatch.undo()
    return {k: p.grad.numpy() for k, p in net.named_parameters()}


def _case_weights(g, case):
    if f"{case}/checkpoint" in g:
        return uo.load_weights(WEIGHTS / f"{g[f'{case}/checkpoint']}.npz")
    from test_unet_wiring import random_case_weights, weights_digest

    w = random_case_weights(case)
    assert weights_digest(w) == str(g[f"{case}/weights_sha256"]), f"{case}: not the weights the fixture was made with"
    return w


def _step(g, case, device):
    net = TrainableSmartTree.from_state_dict(_case_weights(g, case)).to(device).train()
    x = sparse_from_batch(torch.from_numpy(g["xyz"]), torch.from_numpy(g["coords"]), device)
    preds = net(x)
    loss = LOSS_FN(preds, torch.from_numpy(g["targets"]).float().to(device), torch.from_numpy(g["mask"]).to(device))
    sum(loss.values()).backward()
    return net, preds, loss


def _rel(a, b):
    b = np.asarray(b, np.float64)
    return float(np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-300))


@pytest.mark.parametrize("case", ["noble", "depth2", "other"])
def test_oracle_step_matches_reference_digest(case, monkeypatch):
    """The float64 oracle step reproduces the digest of the reference's own gradients (so that it can stand in for them entrywise)."""
    g = np.load(GOLDEN / "train_step.npz")
    grads = _oracle_step(g, case, monkeypatch)
    assert list(grads) == list(g[f"{case}/param_keys"])
    top = max(float(np.abs(v).max()) for v in grads.values())
    worst = 0.0
    for k, v in grads.items():
        err = float(np.abs(grad_digest(v) - g[f"{case}/grad_digest/{k}"]).max()) / top
        worst = max(worst, err)
        assert err <= DIGEST_TOL, f"{case}: d {k}: digest differs by {err:.3g} of the largest gradient"
    print(f"{case}: oracle digest worst {worst:.3g} of the largest gradient")


@pytest.mark.parametrize("case", ["noble", "depth2", "other"])
def test_train_step_matches_reference(backend, case, monkeypatch):
    g = np.load(GOLDEN / "train_step.npz")
    net, preds, loss = _step(g, case, backend)
    report = {}
    for k in ("radius", "direction", "class_l"):
        report[k] = _rel(preds[k].detach().cpu().numpy(), g[f"{case}/{k}"])
        assert report[k] <= OUT_REL, f"{case}/{k}: {report[k]:.3g}"
    got = np.array([float(loss[k].detach()) for k in ("radius", "direction", "class_l")])
    np.testing.assert_allclose(got, g[f"{case}/losses"], rtol=LOSS_TOL)
    params = dict(net.named_parameters())
    assert list(params) == list(g[f"{case}/param_keys"])
    ref_grads = _oracle_step(g, case, monkeypatch)  # pinned to the reference by test_oracle_step_matches_reference_digest
    top = max(float(np.abs(v).max()) for v in ref_grads.values())
    worst, worst_key = 0.0, None
    for k, p in params.items():
        ref = ref_grads[k]
        assert p.grad is not None, k
        err = np.abs(p.grad.cpu().numpy().astype(np.float64) - ref).max()
        bar = max(GRAD_REL * np.abs(ref).max(), GRAD_FLOOR * top)
        ratio = err / bar * GRAD_REL
        if ratio > worst:
            worst, worst_key = ratio, k
        assert err <= bar, f"{case}: d {k}: |err| {err:.3g} > bar {bar:.3g} (max |g64| {np.abs(ref).max():.3g})"
    sd = net.state_dict()
    for k in g.files:
        if k.startswith(f"{case}/running/"):
            key = k[len(f"{case}/running/"):]
            r = _rel(sd[key].cpu().numpy(), g[k])
            assert r <= STAT_TOL, f"{case}: {key} {r:.3g}"
    assert int(sd["input_conv.sequence.1.num_batches_tracked"]) == 1 + int(_case_weights(g, case).get(
        "input_conv.sequence.1.num_batches_tracked", 0))
    print(f"{case} [{backend.type}]: outputs {report}, worst gradient {worst:.3g} of max|g64| ({worst_key})")


def test_state_dict_keys_and_round_trip(backend):
    """Keys and shapes equal the checkpoints'; the state dict loads into the inference network unchanged, whose forward equals
    TrainableSmartTree.eval()'s at the float32 bar."""
    w = np.load(GOLDEN / "unet_wiring.npz")
    for case, planes, fc, nc in (("noble", [8, 16, 32, 64], [8, 8, 4], 2), ("other", [6, 10, 18, 34], [6, 5, 3], 3)):
        net = TrainableSmartTree(3, planes, fc + [1], fc + [3], fc + [nc])
        sd = net.state_dict()
        assert list(sd) == list(w[f"{case}/ref_keys"])
        assert [",".join(str(s) for s in v.shape) for v in sd.values()] == list(w[f"{case}/ref_shapes"])
    g = np.load(GOLDEN / "train_step.npz")
    torch.manual_seed(3)
    net = TrainableSmartTree(3, [8, 16, 32], [8, 8, 4, 1], [8, 8, 4, 3], [8, 8, 4, 2]).to(backend)
    x = sparse_from_batch(torch.from_numpy(g["xyz"]), torch.from_numpy(g["coords"]), backend)
    with torch.no_grad():
        net.train()(x)  # one batch of statistics, so that the running statistics are not the identity
    net.eval()
    with torch.no_grad():
        mine = net(x)
    inf = Smart_Tree({k: v.detach().cpu() for k, v in net.state_dict().items()}, device=backend)
    inf.use_mfma = backend.type != "cpu"
    ref = inf.forward(x)
    for k in mine:
        assert _rel(mine[k].cpu().numpy(), ref[k].cpu().numpy()) <= OUT_REL, k
    back = TrainableSmartTree.from_state_dict(net.state_dict())
    assert all(torch.equal(a.cpu(), b.cpu()) for a, b in zip(back.state_dict().values(), net.state_dict().values()))


def test_fp16_and_float64_are_refused():
    with pytest.raises(ValueError):
        TrainableSmartTree(3, [8, 16], [8, 4, 1], [8, 4, 3], [8, 4, 2], fp16=True)


STEPS = 30
LR = 1e-2


def _loader(tmp_path, device):
    from smart_tree_amd.dataset.dataset import TreeDataset
    from smart_tree_amd.synthetic import sample_tree_cloud

    names = []
    for k, s in enumerate((1, 2)):
        c = sample_tree_cloud(6000, seed=s, scale=0.6, max_depth=3, foliage_fraction=0.3)
        np.savez(tmp_path / f"tree_{k}.npz", xyz=c["xyz"], rgb=c["rgb"], medial_vector=c["medial_vector"], class_l=c["class_l"])
        names.append(f"tree_{k}.npz")
    (tmp_path / "split.json").write_text(json.dumps({"train": names, "validation": names, "test": names}))
    ds = TreeDataset(0.05, tmp_path / "split.json", tmp_path, "train", ["xyz"], ["radius", "direction", "class_l"], device=device)
    return torch.utils.data.DataLoader(ds, batch_size=2, collate_fn=batch_collate)


def _run(loader, device):
    torch.manual_seed(0)
    net = TrainableSmartTree(3, [8, 16, 32], [8, 8, 4, 1], [8, 8, 4, 3], [8, 8, 4, 2]).to(device)
    opt = torch.optim.Adam(net.parameters(), lr=LR)
    hist = [T.train_epoch(loader, net, opt, LOSS_FN, device) for _ in range(STEPS)]
    return net, hist, T.eval_epoch(loader, net, LOSS_FN, device)


@pytest.mark.gpu
def test_training_run_lowers_the_loss(tmp_path):
    """train_epoch over a DataLoader of two synthetic trees (TreeDataset + batch_collate), Adam from a fixed seed.  Reports whether
    two runs are bit-identical."""
    dev = torch.device("cuda:0")
    loader = _loader(tmp_path, dev)
    net, hist, ev = _run(loader, dev)
    total = [sum(h.values()) for h in hist]
    print("training losses:", [round(t, 4) for t in total], "eval:", ev)
    assert all(np.isfinite(total)) and net.training
    assert total[-1] <= 0.6 * total[0], f"loss {total[0]:.4f} -> {total[-1]:.4f}"  # measured: 4.327 -> 2.242 (0.52)
    net2, hist2, _ = _run(loader, dev)
    same = all(torch.equal(a, b) for a, b in zip(net.state_dict().values(), net2.state_dict().values()))
    print("two runs bit-identical:", same)
