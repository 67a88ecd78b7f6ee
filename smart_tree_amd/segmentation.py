"""Segment a cloud by its skeleton: the tube, tree and branch every point belongs to (csrc/segment.hip).

`python -m smart_tree_amd.segmentation cloud=<.npz|.ply> skeleton=<skeleton.npz> out=<dir|.npz> [max_distance=0.1] [centre=false]
[png=<file>] [form=auto] [device=cuda:0]` writes `segmentation.npz` (and `seg_cld.ply`, the points coloured by branch, when `out` is
a directory) and prints the points per tree and the unassigned share.  `centre=true` runs `CentreCloud` first: that puts a raw
cloud into the frame of the skeleton the pipeline saved for it.  Overrides are parsed by config.py, as for `evaluate` / `render`.

The reference has `skeleton_to_points` (util/queries.py:139-166): distance, radius and vector to the nearest tube, by a dense
sweep, and no ids.  `segment_cloud` answers per point which tube wins -- the minimum of |distance to the axis - radius|, ties to
the lowest tube, exactly as include/smarttree_hip.h states it -- and turns the tube into (tree, branch) through the table of
branches the renderer colours tubes with (`data_types.flat.FlatSkeletons`).  A batch of clouds goes through one call, each cloud against
its own trees.  Per-branch statistics come from integer per-tube tallies: identical from run to run.
"""
from __future__ import annotations

from dataclasses import dataclass
from pathlib import Path
from typing import Optional

import numpy as np
import torch

from . import _lib
from .data_types.cloud import Cloud
from .data_types.flat import FlatSkeletons, points_and_skeletons
from .evaluation import branch_key

FORMS = {"auto": 0, "dense": 1, "grid": 2}
UNASSIGNED_KEY = 0x7FFFFFFF  # `to_cloud`'s branch id of a point without a tube (no (tree, branch) below 2^15 trees maps to it)
BRANCH_COLUMNS = ("cloud", "tree", "branch", "parent", "tubes", "points", "mean_abs_residual", "mean_residual")
FIX = float(1 << 24)  # the tallies count residuals in 2^-24 m


def segment_points(pts, a, b, r1, r2, pt_off=None, tube_off=None, max_distance=None, form="auto", tally=True,
                   outputs=("tube", "residual", "vec", "rad")) -> dict:
    """`st_segment_points_seg` on device tensors: pts [n,3] against tubes a, b [m,3], r1, r2 [m]; pt_off / tube_off [B+1] int32 for a
    batch.  Returns the requested per-point tensors, "tally" int64 [m,3] and "ws" (its first four int64: the grid's statistics)."""
    L = _lib.lib()
    dev = pts.device
    f = lambda t, shape: t.to(dev).float().reshape(shape).contiguous()
    pts, a, b, r1, r2 = f(pts, (-1, 3)), f(a, (-1, 3)), f(b, (-1, 3)), f(r1, (-1,)), f(r2, (-1,))
    n, m = pts.shape[0], a.shape[0]
    nseg = 1
    if pt_off is not None or tube_off is not None:
        if pt_off is None or tube_off is None or pt_off.shape[0] != tube_off.shape[0]:
            raise ValueError("segment_points: a batch needs the offsets of its points and of its tubes, one entry per cloud plus one")
        pt_off, tube_off = (t.to(dev).to(torch.int32).contiguous() for t in (pt_off, tube_off))
        nseg = pt_off.shape[0] - 1
    out = {"tube": torch.empty(n, dtype=torch.int32, device=dev) if "tube" in outputs else None,
           "residual": torch.empty(n, dtype=torch.float32, device=dev) if "residual" in outputs else None,
           "vec": torch.empty((n, 3), dtype=torch.float32, device=dev) if "vec" in outputs else None,
           "rad": torch.empty(n, dtype=torch.float32, device=dev) if "rad" in outputs else None,
           "tally": torch.empty((m, 3), dtype=torch.int64, device=dev) if tally else None}
    nbytes = L.st_segment_workspace_bytes(n, m, nseg)
    if nbytes < 0:
        raise _lib.StError(f"segment_points: {n} points, {m} tubes and {nseg} cloud(s) are outside what the call takes")
    ws = _lib.workspace(nbytes, dev)
    p = lambda t: _lib.ptr(t) if t is not None and t.numel() else None
    _lib.check(L.st_segment_points_seg(p(pts), n, p(pt_off), p(a), p(b), p(r1), p(r2), m, p(tube_off), nseg,
                                       -1.0 if max_distance is None else float(max_distance), FORMS[form] if isinstance(form, str) else int(form),
                                       p(out["tube"]), p(out["residual"]), p(out["vec"]), p(out["rad"]), p(out["tally"]),
                                       _lib.ptr(ws), ws.numel(), _lib.stream(dev)))
    out["ws"] = ws
    return {k: v for k, v in out.items() if v is not None}


@dataclass
class CloudSegmentation:
    """Per point (device tensors, aligned with the cloud): `tube` int32 (position among the tubes of the call, `skeleton_tubes`
    order), `tree_id` (the tree's index inside its cloud), `branch_id` (the branch's id in its tree), `residual` (distance to the axis
    minus the radius there, negative inside), `radius`, `vector` (projection - point).  Unassigned: -1 in the three ids, +inf, NaN, 0.
    `branches`: float64 [B,8] on the host, one row per branch, columns BRANCH_COLUMNS (the means in metres, NaN without points)."""
    tube: torch.Tensor
    tree_id: torch.Tensor
    branch_id: torch.Tensor
    residual: torch.Tensor
    radius: torch.Tensor
    vector: torch.Tensor
    branches: np.ndarray
    seg_off: Optional[torch.Tensor] = None   # [B+1] int32: the clouds of a batch in the point arrays
    tube_off: Optional[np.ndarray] = None    # [B+1]: the clouds' tubes

    def __len__(self) -> int:
        return int(self.tube.shape[0])

    @property
    def n_assigned(self) -> int:
        return int(self.branches[:, 5].sum())

    def tree_mask(self, t: int, cloud: int = 0) -> torch.Tensor:
        """Points of tree `t` (of cloud `cloud` of a batch)."""
        mask = self.tree_id == int(t)
        if self.seg_off is not None:
            off = self.seg_off.tolist()
            inside = torch.zeros_like(mask)
            inside[off[cloud]:off[cloud + 1]] = True
            mask = mask & inside
        return mask

    def split(self) -> list:
        """The clouds of a batch, each as its own one-cloud call gives it: tube indices count from the cloud's first tube."""
        if self.seg_off is None:
            return [self]
        off, toff = self.seg_off.tolist(), [int(x) for x in self.tube_off]
        parts = []
        for k, (p0, p1) in enumerate(zip(off[:-1], off[1:])):
            tube = self.tube[p0:p1]
            rows = self.branches[self.branches[:, 0] == k].copy()
            rows[:, 0] = 0
            parts.append(CloudSegmentation(torch.where(tube >= 0, tube - toff[k], tube), self.tree_id[p0:p1], self.branch_id[p0:p1],
                                           self.residual[p0:p1], self.radius[p0:p1], self.vector[p0:p1], rows))
        return parts

    def keys(self) -> torch.Tensor:
        """int32 [n]: the colour key of every point's branch (`render.skeleton_items` gives its tubes the same), UNASSIGNED_KEY
        without one."""
        key = branch_key(self.tree_id.to(torch.int64), self.branch_id.to(torch.int64))
        return torch.where(self.tube >= 0, key, torch.full_like(key, UNASSIGNED_KEY)).to(torch.int32)

    def to_cloud(self, cloud: Cloud) -> Cloud:
        """`cloud` with `branch_ids` set to the keys: `cloud_items(colour="branch")` then colours points like their tubes."""
        if len(cloud) != len(self):
            raise ValueError(f"to_cloud: a segmentation of {len(self)} points for a cloud of {len(cloud)}")
        return Cloud(xyz=cloud.xyz, rgb=cloud.rgb, medial_vector=cloud.medial_vector, branch_direction=cloud.branch_direction,
                     branch_ids=self.keys().to(cloud.xyz.device).reshape(-1, 1), class_l=cloud.class_l, filename=cloud.filename,
                     seg_off=cloud.seg_off)

    def save(self, path) -> None:
        path = Path(path)
        path.parent.mkdir(parents=True, exist_ok=True)
        h = lambda t: t.detach().cpu().numpy()
        extra = {} if self.seg_off is None else {"seg_off": h(self.seg_off), "tube_off": np.asarray(self.tube_off, np.int64)}
        np.savez(path, tube=h(self.tube), tree_id=h(self.tree_id), branch_id=h(self.branch_id), residual=h(self.residual),
                 radius=h(self.radius), vector=h(self.vector), branches=self.branches, **extra)

    @staticmethod
    def load(path, device="cpu") -> "CloudSegmentation":
        with np.load(path) as z:
            t = lambda k: torch.from_numpy(z[k]).to(device)
            return CloudSegmentation(t("tube"), t("tree_id"), t("branch_id"), t("residual"), t("radius"), t("vector"), z["branches"],
                                     t("seg_off") if "seg_off" in z.files else None, z["tube_off"] if "tube_off" in z.files else None)


def segment_cloud(cloud_or_xyz, skeleton, max_distance=None, form="auto", tally=True, device=None) -> CloudSegmentation:
    """Every point of a `Cloud` (or an [n,3] tensor / array) to the tube, tree and branch of `skeleton`: a `TreeSkeleton`, a
    `DisjointTreeSkeleton`, the flat arrays of `save_skeleton_npz`, or a list of these, one per cloud of a collated `Cloud` (what
    `Pipeline.process_clouds` returns).  `max_distance` (metres from the tube's surface): points further than that stay
    unassigned.  `tally=False` skips the per-branch statistics (their columns are NaN)."""
    xyz, seg_off, skeletons, _, _ = points_and_skeletons(cloud_or_xyz, skeleton, device, "segment_cloud")
    dev = xyz.device
    flat = FlatSkeletons(skeletons, "segment_cloud")
    a, b, r1, r2 = (torch.from_numpy(t) for t in flat.tubes(*flat.float32()))
    tube_off = flat.tube_off
    owner = np.column_stack([flat.rows[:, :4], flat.tubes_of_row])  # cloud, tree, id, parent, tubes
    batched = seg_off is not None
    res = segment_points(xyz, a, b, r1, r2, seg_off if batched else None,
                         torch.from_numpy(tube_off.astype(np.int32)) if batched else None, max_distance, form, tally)
    tube = res["tube"]
    # tube -> (tree, branch): one table row per tube and a last row of -1 that tube = -1 indexes
    row_of_tube = np.repeat(np.arange(len(owner)), owner[:, 4])
    table = np.full((len(row_of_tube) + 1, 2), -1, np.int32)
    table[:-1] = owner[row_of_tube, 1:3]
    ids = torch.from_numpy(table).to(dev).index_select(0, torch.where(tube >= 0, tube, torch.full_like(tube, len(row_of_tube))).long())
    branches = np.full((len(owner), 8), np.nan)
    branches[:, :5] = owner
    if tally:
        per_tube = res["tally"].cpu().numpy()  # the one read-back
        sums = np.zeros((len(owner), 3), np.int64)
        np.add.at(sums, row_of_tube, per_tube)
        branches[:, 5] = sums[:, 0]
        with np.errstate(invalid="ignore", divide="ignore"):
            branches[:, 6] = np.where(sums[:, 0] > 0, sums[:, 1] / FIX / sums[:, 0], np.nan)
            branches[:, 7] = np.where(sums[:, 0] > 0, sums[:, 2] / FIX / sums[:, 0], np.nan)
    return CloudSegmentation(tube, ids[:, 0].contiguous(), ids[:, 1].contiguous(), res["residual"], res["rad"], res["vec"], branches,
                             seg_off.to(dev) if batched else None, tube_off if batched else None)


def key_colours(keys: np.ndarray) -> np.ndarray:
    """float32 [n,3] in [0,1]: the renderer's colour of an id (csrc/render.hip: bytes of the 64-bit mix of id + 1, halved and lifted)."""
    h = (np.asarray(keys).astype(np.int64) + 1).astype(np.uint64)
    with np.errstate(over="ignore"):
        h ^= h >> np.uint64(33)
        h *= np.uint64(0xff51afd7ed558ccd)
        h ^= h >> np.uint64(33)
        h *= np.uint64(0xc4ceb9fe1a85ec53)
        h ^= h >> np.uint64(33)
    byte = lambda s: (64 + ((h >> np.uint64(s)) & np.uint64(127))).astype(np.float32) / np.float32(255)
    return np.stack([byte(8), byte(24), byte(40)], axis=1)


def save_segmentation(directory, cloud: Cloud, seg: CloudSegmentation) -> None:
    """`segmentation.npz` and `seg_cld.ply` (the points coloured by branch; unassigned points grey)."""
    from .util.file import write_ply_points

    directory = Path(directory)
    seg.save(directory / "segmentation.npz")
    keys = seg.keys().cpu().numpy()
    rgb = key_colours(keys)
    rgb[keys == UNASSIGNED_KEY] = 0.5
    write_ply_points(directory / "seg_cld.ply", cloud.xyz.detach().cpu().numpy(), rgb)


def write_view(path, cloud: Cloud, skeleton, seg: CloudSegmentation, device, width: int = 1920, height: int = 1080) -> None:
    """`segmentation.png`: the points coloured by their branch over the tubes in the same colours."""
    from .render import Renderer, cloud_items, fit, skeleton_items, write_png

    items = cloud_items(seg.to_cloud(cloud), colour="branch") + skeleton_items(skeleton, device=device)
    r = Renderer(width, height)
    write_png(path, r.render(items, [fit(items, (-1, 0, 0), width, height)], outputs=("rgb",))["rgb"][0])


def summary(seg: CloudSegmentation) -> str:
    """One line per tree with its points, and the unassigned share."""
    n = len(seg)
    lines = []
    rows = seg.branches
    for cloud, tree in sorted({(int(r[0]), int(r[1])) for r in rows}):
        sel = (rows[:, 0] == cloud) & (rows[:, 1] == tree)
        pts = np.nansum(rows[sel, 5])
        lines.append(f"cloud {cloud} tree {tree}: {int(pts)} points on {int(sel.sum())} branches")
    unassigned = int((seg.tube < 0).sum())
    lines.append(f"unassigned: {unassigned} of {n} points ({100.0 * unassigned / max(n, 1):.2f} %)")
    return "\n".join(lines)


# ---------------------------------------------------------------------------------------------------------------- cli ---
DEFAULTS = {"cloud": None, "skeleton": None, "out": None, "max_distance": None, "centre": False, "png": None, "width": 1920,
            "height": 1080, "form": "auto", "device": "cuda:0"}
USAGE = ("usage: python -m smart_tree_amd.segmentation cloud=<.npz|.ply> skeleton=<skeleton.npz> out=<dir|.npz> "
         "[max_distance=0.1] [centre=false] [png=<file>] [width=1920] [height=1080] [form=auto|dense|grid] [device=]")


def main(argv=None) -> CloudSegmentation:
    from .config import cloud_command
    from .evaluate import load_any_skeleton

    cfg, dev, cloud = cloud_command(argv, DEFAULTS, USAGE)
    if str(cfg["form"]) not in FORMS:
        raise SystemExit(f"segmentation: form must be one of {', '.join(FORMS)}")
    skeleton = load_any_skeleton(cfg["skeleton"])
    seg = segment_cloud(cloud, skeleton, max_distance=None if cfg["max_distance"] is None else float(cfg["max_distance"]),
                        form=str(cfg["form"]), device=dev)
    out = Path(str(cfg["out"]))
    if out.suffix == ".npz":
        seg.save(out)
    else:
        save_segmentation(out, cloud, seg)
    if cfg["png"] is not None:
        write_view(Path(str(cfg["png"])), cloud, skeleton, seg, dev, int(cfg["width"]), int(cfg["height"]))
    print(summary(seg))
    return seg


if __name__ == "__main__":
    main()
