"""``model_to_frame_batch`` and ``frame_to_model_batch`` (reference: lightning_pose/data/bboxes.py:194-288, frame_to_norm :45-71,
norm_to_frame :74-105, norm_to_model :129-147)."""

from __future__ import annotations

import torch

from .. import ops


def batch_num_views(batch_dict: dict) -> int:
    """Number of camera views encoded in a batch (reference bboxes.py:254-271)."""
    if "num_views" in batch_dict and (int(batch_dict["num_views"].max()) > 1 or batch_dict.get("is_multiview", False)):
        unique = torch.unique(batch_dict["num_views"])
        if unique.numel() != 1:
            raise ValueError(f"each batch element must contain the same number of views; found elements with {unique} views")
        return int(unique)
    if batch_dict.get("is_multiview", False):
        return batch_dict["bbox"].shape[1] // 4
    return 1


def model_dims(batch_dict: dict) -> tuple[int, int]:
    img = batch_dict["images"] if "images" in batch_dict else batch_dict["frames"]
    return img.shape[-2], img.shape[-1]


def model_to_frame_batch(batch_dict: dict, model_keypoints: torch.Tensor, in_place: bool = True) -> torch.Tensor:
    """(B, 2K) keypoints in network-input px -> original-frame px using ``batch_dict['bbox']`` rows [x, y, h, w].

    Unlike the reference this never writes through its argument (the reference's default ``in_place=True`` rewrites
    the decode output through a reshape view - SURVEY.md section 8b "aliasing"); the returned values are identical.
    """
    mh, mw = model_dims(batch_dict)
    views = batch_num_views(batch_dict)
    k = model_keypoints.shape[1] // 2
    bbox = batch_dict["bbox"]
    if bbox.shape[0] != model_keypoints.shape[0]:  # context batch: no predictions for the first / last two frames (norm_to_frame :99-104)
        bbox = bbox[2:-2]
    fm = ops.DecodeFrameMap(None, False, bbox, views, mh, mw, k)
    return ops.frame_map_apply(model_keypoints, fm)


def frame_to_model_batch(batch_dict: dict, frame_keypoints: torch.Tensor) -> torch.Tensor:
    """(batch, num_views, num_keypoints, 2) keypoints in original-frame px -> network-input px: per view, ``(kp - bbox[x, y]) / bbox[w, h] *
    model[w, h]`` with ``batch_dict['bbox'][:, 4 v : 4 v + 4]`` = [x, y, h, w] (reference :194-219).  A few elementwise torch operations on
    whatever device the keypoints live on (differentiable); the training step does not come through here - its reprojection applies this map
    inside the fused geometry kernel (``ops.camera_chain``)."""
    batch, views, _, _ = frame_keypoints.shape
    mh, mw = model_dims(batch_dict)
    bbox = batch_dict["bbox"].to(device=frame_keypoints.device, dtype=frame_keypoints.dtype).reshape(batch, views, 4)
    offset = bbox[:, :, None, 0:2]                                  # x, y
    size = torch.stack([bbox[:, :, 3], bbox[:, :, 2]], dim=-1)[:, :, None, :]   # w, h
    scale = torch.tensor([float(mw), float(mh)], device=frame_keypoints.device, dtype=frame_keypoints.dtype)
    return (frame_keypoints - offset) / size * scale
