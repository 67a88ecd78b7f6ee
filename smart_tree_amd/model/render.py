"""The reference's `model/render.py:7-35`: three pictures of a labelled cloud -- the cloud in its colours, the class segmentation
and the medial vectors -- through `smart_tree_amd.render.Renderer` (its `log_images` went to wandb and is out of scope)."""
from __future__ import annotations

from ..render import cloud_items, medial_vector_items


def render_cloud(renderer, labelled_cloud, camera_position=[1, 0, 0], camera_up=[0, 1, 0], cmap=None) -> list:
    """[cloud image, segmentation image, medial-vector image], each uint8 [H,W,3] on the host: the reference's return order.  The
    lines of the third picture start at the cloud's points, so all three share one aim."""
    seg = cloud_items(labelled_cloud, "class", **({} if cmap is None else {"cmap": cmap}))
    segmented_img = renderer.capture(seg, camera_position, camera_up)
    cld_img = renderer.capture(cloud_items(labelled_cloud, "rgb"), camera_position, camera_up)
    projected_img = renderer.capture(medial_vector_items(labelled_cloud), camera_position, camera_up)
    return [cld_img, segmented_img, projected_img]


def write_cloud_images(renderer, labelled_cloud, stem, camera_position=[1, 0, 0], camera_up=[0, 1, 0], cmap=None) -> list:
    """`render_cloud` to `<stem>_cloud.png`, `<stem>_segmentation.png`, `<stem>_medial.png`; returns the paths."""
    from pathlib import Path

    from ..render import write_png

    stem = Path(stem)
    paths = [stem.with_name(f"{stem.name}_{kind}.png") for kind in ("cloud", "segmentation", "medial")]
    for path, img in zip(paths, render_cloud(renderer, labelled_cloud, camera_position, camera_up, cmap)):
        write_png(path, img)
    return paths
