"""Batch and output helpers at the reference's names (smart_tree/model/helper.py), for ported scripts and the training run's
captures.

`to_labelled_clds` slices each tree's rows out of the collated batch's contiguous segments (batch_collate writes the sample
index into coords[:, 0] in item order) instead of one mask per cloud.  The reference fills every captured cloud's `rgb` with
random values (helper.py:76); here `rgb` stays empty.
"""
from __future__ import annotations

from pathlib import Path
from typing import List

import torch

from ..data_types.cloud import Cloud
from .sparse import sparse_from_batch


def get_batch(dataloader, device, fp_16=False):
    """helper.py:12-32: yields (sparse input, targets, mask, filenames) per batch_collate batch; fp_16 rounds features and
    targets through half (as train.train_epoch's fp16 path)."""
    for (feats, targets), coords, mask, filenames in dataloader:
        if fp_16:
            feats, targets = feats.half(), targets.half()
        yield sparse_from_batch(feats.float(), coords, device=device), targets.to(device).float(), mask.to(device), filenames


def split_outputs(features, mask):
    """helper.py:47-52: radius (exp of the log radius), direction and class id of the rows `mask` selects (a mask or a slice)."""
    radii = torch.exp(features["radius"][mask].float())
    direction = features["direction"][mask].float()
    class_l = torch.argmax(features["class_l"], dim=1)[mask]
    return radii, direction, class_l


def to_labelled_clds(cloud_ids, coords, rgb, model_output, cmap, filenames) -> List[Cloud]:
    """helper.py:55-88: one Cloud per tree of the batch (on the CPU), xyz = the input features' first three columns,
    medial_vector = exp(radius) * direction, class_l = argmax.  `rgb` and `cmap` are accepted for the reference's signature."""
    n = len(filenames)
    counts = torch.bincount(cloud_ids.long(), minlength=n).tolist() if cloud_ids.numel() else [0] * n
    if len(counts) != n or any(c == 0 for c in counts):
        raise ValueError(f"to_labelled_clds: {len(filenames)} file names for rows of clouds {counts}")
    radii, direction, class_l = split_outputs(model_output, slice(None))
    clouds, start = [], 0
    for i, c in enumerate(counts):
        rows = slice(start, start + c)
        start += c
        clouds.append(Cloud(xyz=coords[rows].float(), medial_vector=radii[rows] * direction[rows],
                            class_l=class_l[rows].reshape(-1, 1), filename=Path(filenames[i])).to_device(torch.device("cpu")))
    return clouds


def model_output_to_labelled_clds(sparse_input, model_output, cmap, filenames) -> List[Cloud]:
    """helper.py:35-44."""
    return to_labelled_clds(sparse_input.indices[:, 0], sparse_input.features[:, :3], sparse_input.features[:, 3:6], model_output,
                            cmap, filenames)
