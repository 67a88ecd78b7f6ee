"""Pipeline: point cloud -> skeleton (reference smart_tree/pipeline.py:13-106).

Constructor keywords, defaults and `process_cloud(path=None, cloud=None)` / `post_process(skeleton)`
match the reference.  Additive change: `process_cloud` returns the `DisjointTreeSkeleton` (the
reference only views / saves it).  An interactive window needs open3d and is out of scope: with a view flag
set and `view_path` given, the views are rendered offscreen (smart_tree_amd/render.py) and written there as
`model_output.png` / `skeleton.png`; without `view_path` a view flag raises.  `save_outputs` writes
dependency-free files (util/file.py).  Additive: `segment_cloud=True` assigns every point of the preprocessed cloud to
a tree and a branch of the post-processed skeleton (segmentation.py) and keeps the result in `last_segmentation`;
`save_outputs` then also writes `segmentation.npz` / `seg_cld.ply`, `view_skeletons` also `segmentation.png`.
Additive: `refine_skeletons=True` fits the post-processed skeleton's radii and axes to the points the network called wood
(refine.py); the refined skeleton is what is returned, segmented, drawn and saved, `last_raw_skeleton` / `last_fit` keep the
skeleton as it was and the per-tube report, and `save_outputs` also writes `skeleton_fit.npz`.
Additive: `measure_trees=True` measures every tree of the final skeleton on the preprocessed cloud (inventory.py: height, DBH,
crown extent, wood volume per tree and per branch), segmenting first when `segment_cloud` was not asked for; the result is kept in
`last_inventory` and `save_outputs` also writes `inventory.json`, `trees.csv` and `branches.csv`.
Additive: `remove_ground=True` models the terrain under the preprocessed cloud (terrain.py) and takes the ground points out before the
network sees the cloud, so that everything downstream works on the cloud without ground; the model is kept in `last_ground`,
`measure_trees` takes the trees' bases from it, and `save_outputs` also writes `ground.npz` and `dtm.asc`.
"""
from __future__ import annotations

from pathlib import Path

import numpy as np
import torch

from . import profiling
from .data_types.cloud import Cloud
from .data_types.tree import DisjointTreeSkeleton
from .util.mesh import skeleton_mesh, write_ply_mesh
from .util.file import load_cloud, save_skeleton, save_skeleton_npz, write_ply_points, write_ply_skeleton


class Pipeline:
    def __init__(self, preprocessing, model_inference, skeletonizer, repair_skeletons=False, smooth_skeletons=False,
                 smooth_kernel_size=0, prune_skeletons=False, min_skeleton_radius=0.0, min_skeleton_length=1000,
                 view_model_output=False, view_skeletons=False, save_outputs=False, save_path="/", branch_classes=[0],
                 cmap=[[1, 0, 0], [0, 1, 0]], device=torch.device("cuda:0"), view_path=None, segment_cloud=False,
                 segment_max_distance=None, refine_skeletons=False, refine_iterations=2, refine_max_relative=0.5,
                 measure_trees=False, inventory_cell=0.1, inventory_layers=256, remove_ground=False, ground_cell=0.5,
                 ground_max_window=8.0, ground_slope=0.3, ground_tolerance=0.2):
        self.preprocessing = preprocessing
        self.model_inference = model_inference
        self.skeletonizer = skeletonizer
        self.repair_skeletons = repair_skeletons
        self.smooth_skeletons = smooth_skeletons
        self.smooth_kernel_size = smooth_kernel_size
        self.prune_skeletons = prune_skeletons
        self.min_skeleton_radius = min_skeleton_radius
        self.min_skeleton_length = min_skeleton_length
        self.view_model_output = view_model_output
        self.view_skeletons = view_skeletons
        self.save_outputs = save_outputs
        self.save_path = save_path
        self.branch_classes = branch_classes
        self.cmap = np.asarray(cmap)
        self.device = torch.device(device)
        self.view_path = view_path
        self.last_labelled_cloud = None
        self.segment_cloud = segment_cloud
        self.segment_max_distance = segment_max_distance
        self.last_segmentation = None
        self._segmented = None  # (cloud, its segmentation) the next write_views call draws
        self.refine_skeletons = refine_skeletons
        self.refine_iterations = refine_iterations
        self.refine_max_relative = refine_max_relative
        self.last_raw_skeleton = None
        self.last_fit = None
        self.measure_trees = measure_trees
        self.inventory_cell = inventory_cell
        self.inventory_layers = inventory_layers
        self.last_inventory = None
        self.remove_ground = remove_ground
        self.ground_cell = ground_cell
        self.ground_max_window = ground_max_window
        self.ground_slope = ground_slope
        self.ground_tolerance = ground_tolerance
        self.last_ground = None

    def process_cloud(self, path: Path = None, cloud: Cloud = None) -> DisjointTreeSkeleton:
        cloud = load_cloud(path) if path is not None else cloud
        cloud = cloud.to_device(self.device)
        with profiling.stage("preprocess"):
            cloud = self.preprocessing(cloud)
        if self.remove_ground:
            cloud = self._without_ground(cloud)
        lc = self.model_inference.forward(cloud).to_device(self.device)
        self.last_labelled_cloud = lc
        with profiling.stage("class_filter"):
            branch_cloud = lc.filter_by_class(self.branch_classes)
        skeleton = self.skeletonizer.forward(branch_cloud)
        with profiling.stage("post_process"):
            self.post_process(skeleton)
            skeleton.skeletons  # materialise: device post-processing kernel, one D->H copy, BranchSkeleton objects
        if self.refine_skeletons:
            skeleton = self._refine(branch_cloud, skeleton)
        if self.segment_cloud:
            self._segment(cloud, skeleton)
            self._segmented = (cloud, self.last_segmentation)
        if self.measure_trees:
            self._measure(cloud, skeleton)
        if self.view_model_output or self.view_skeletons:
            if self.view_path is None:
                raise NotImplementedError("viewing needs open3d, which is out of scope of smart_tree_amd")
            self.write_views(Path(self.view_path), lc, skeleton)
        if self.save_outputs:  # reference pipeline.py:85-93 (skeleton.ply / cloud.ply; meshes need open3d)
            sp = Path(self.save_path)
            save_skeleton_npz(sp / "skeleton.npz", skeleton)
            for tree in skeleton.skeletons:  # the reference's own per-tree layout (util/file.py:73-94), readable by its load_skeleton
                if tree.branches:
                    save_skeleton(tree, sp / f"skeleton_{tree._id}.npz")
            write_ply_skeleton(sp / "skeleton.ply", skeleton)
            verts, tris = skeleton_mesh(skeleton)  # reference pipeline.py:90: mesh.ply = the skeleton's tube mesh
            write_ply_mesh(sp / "mesh.ply", verts, tris)
            write_ply_points(sp / "cloud.ply", lc.xyz.cpu().numpy(), lc.rgb.cpu().numpy() if lc.rgb is not None else None)
            if self.segment_cloud:  # the reference's fourth file name (pipeline.py:93 `seg_cld.ply`), here the points by branch
                from .segmentation import save_segmentation
                save_segmentation(sp, cloud, self.last_segmentation)
            if self.refine_skeletons:
                self.last_fit.save(sp / "skeleton_fit.npz")
            if self.measure_trees:
                self.last_inventory.save(sp)
            if self.remove_ground:
                self.last_ground.save(sp)
        return skeleton

    def _without_ground(self, cloud: Cloud) -> Cloud:
        """The cloud `preprocessing` returned (one, or a batch: one call) without the points its ground model calls ground."""
        from .terrain import ground_model

        with profiling.stage("remove_ground"):
            self.last_ground = ground_model(cloud, cell=self.ground_cell, max_window=self.ground_max_window, slope=self.ground_slope,
                                            ground_tolerance=self.ground_tolerance, device=self.device)
            return cloud.filter(~self.last_ground.is_ground)

    def _refine(self, branch_cloud: Cloud, skeleton):
        """The skeleton (or the skeletons of a batch) fitted to the points it was made from: the points of `branch_classes`."""
        from .refine import refine_skeleton

        with profiling.stage("refine_skeleton"):
            self.last_raw_skeleton = skeleton
            refined, self.last_fit = refine_skeleton(branch_cloud, skeleton, iterations=self.refine_iterations,
                                                     max_relative=self.refine_max_relative, device=self.device)
        return refined

    def _segment(self, cloud: Cloud, skeleton) -> None:
        """Every point the caller gave, in the skeleton's frame (the cloud `preprocessing` returned), to its tree and branch."""
        from .segmentation import segment_cloud

        with profiling.stage("segment_cloud"):
            self.last_segmentation = segment_cloud(cloud, skeleton, max_distance=self.segment_max_distance, device=self.device)

    def _measure(self, cloud: Cloud, skeleton) -> None:
        """Every tree of the skeleton (or of the skeletons of a batch) measured on the cloud `preprocessing` returned: one call."""
        from .inventory import measure_trees
        from .segmentation import segment_cloud

        with profiling.stage("measure_trees"):
            seg = self.last_segmentation if self.segment_cloud else segment_cloud(cloud, skeleton, max_distance=self.segment_max_distance,
                                                                                  device=self.device)
            self.last_inventory = measure_trees(cloud, skeleton, segmentation=seg, cell=self.inventory_cell, layers=self.inventory_layers,
                                                device=self.device, ground=self.last_ground if self.remove_ground else None)

    def process_clouds(self, clouds) -> list:
        """B independent clouds through ONE set of kernel launches (additive; the reference's unit of work is a batch
        as well: model/sparse.py:40-61 writes the batch index into coords[:,0], model_inference.py:62-78 runs a batch per
        forward -- here the batch index is carried through every stage: blocks / voxels, network, kNN graph, components,
        SSSP, branch selection, post-processing).  Returns one DisjointTreeSkeleton per cloud, each identical to
        `process_cloud` of that cloud alone (tests/test_batch.py)."""
        clouds = [c.to_device(self.device) for c in clouds]
        if not clouds:
            return []
        batch = Cloud.collate([Cloud(c.xyz, c.rgb if c.rgb is not None else torch.zeros_like(c.xyz)) for c in clouds])
        with profiling.stage("preprocess"):
            batch = self.preprocessing(batch)
        if batch.n_seg != len(clouds):  # an augmentation that rebuilt the Cloud without its batch offsets would merge the inputs
            raise RuntimeError(f"process_clouds: preprocessing returned {batch.n_seg} cloud(s) for a batch of {len(clouds)}")
        if self.remove_ground:  # one ground model for the whole batch; `last_ground.split()` gives the clouds' parts
            batch = self._without_ground(batch)
        lc = self.model_inference.forward(batch).to_device(self.device)
        self.last_labelled_cloud = lc
        with profiling.stage("class_filter"):
            branch_cloud = lc.filter_by_class(self.branch_classes)
        skeleton = self.skeletonizer.forward(branch_cloud)
        with profiling.stage("post_process"):
            self.post_process(skeleton)
            parts = skeleton.split()  # device post-processing of all clouds, ONE device-to-host copy, per-cloud views
        if len(parts) != len(clouds):
            raise RuntimeError(f"process_clouds: {len(parts)} skeleton(s) for a batch of {len(clouds)} clouds")
        if self.refine_skeletons:  # one segmentation and one fit per iteration for the whole batch
            parts = self._refine(branch_cloud, parts)
        if self.segment_cloud:  # each cloud against its own trees, one call
            self._segment(batch, parts)
        if self.measure_trees:  # the whole batch in one call; `last_inventory.split()` gives the clouds' parts
            self._measure(batch, parts)
        if self.view_model_output or self.view_skeletons:
            if self.view_path is None:
                raise NotImplementedError("viewing needs open3d, which is out of scope of smart_tree_amd")
            drawn = list(zip(batch.split(), self.last_segmentation.split())) if self.segment_cloud else [None] * len(parts)
            for k, (cloud_k, part) in enumerate(zip(lc.split(), parts)):
                self._segmented = drawn[k]
                self.write_views(Path(self.view_path), cloud_k, part, prefix=f"cloud_{k}_")
        return parts

    def write_views(self, path: Path, labelled_cloud: Cloud, skeleton, prefix: str = "", width: int = 1920, height: int = 1080) -> None:
        """What the reference shows in a window, as pictures: `model_output.png` (the segmentation; view_model_output) and
        `skeleton.png` (the tubes coloured by branch over the cloud in its own colours; view_skeletons)."""
        from .render import Renderer, cloud_items, fit, skeleton_items, write_png

        r = Renderer(width, height)
        look = lambda items: r.render(items, [fit(items, (-1, 0, 0), width, height)], outputs=("rgb",))["rgb"][0]
        if self.view_model_output:
            write_png(path / f"{prefix}model_output.png", look(cloud_items(labelled_cloud, "class", cmap=self.cmap)))
        if self.view_skeletons:
            items = cloud_items(labelled_cloud, "rgb") + skeleton_items(skeleton, device=self.device)
            write_png(path / f"{prefix}skeleton.png", look(items))
            if self._segmented is not None:  # segment_cloud: the points by branch over the tubes in the same colours
                cloud, seg = self._segmented
                items = cloud_items(seg.to_cloud(cloud), "branch") + skeleton_items(skeleton, device=self.device)
                write_png(path / f"{prefix}segmentation.png", look(items))
        self._segmented = None

    def post_process(self, skeleton: DisjointTreeSkeleton) -> None:
        if self.prune_skeletons:
            skeleton.prune(min_length=self.min_skeleton_length, min_radius=self.min_skeleton_radius)
        if self.repair_skeletons:
            skeleton.repair()
        if self.smooth_skeletons:
            skeleton.smooth(self.smooth_kernel_size)
