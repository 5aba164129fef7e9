"""Output contracts of ``get_loss_inputs_*`` (reference: lightning_pose/models/datatypes.py:40-74).
``models.factory._validate_loss_model_compatibility`` reads these annotations."""

from __future__ import annotations

from typing import TypedDict

import torch


class HeatmapTrackerLabeledOutputsDict(TypedDict):
    heatmaps_targ: torch.Tensor
    heatmaps_pred: torch.Tensor
    keypoints_targ: torch.Tensor
    keypoints_pred: torch.Tensor
    confidences: torch.Tensor


class HeatmapTrackerMultiviewTransformerLabeledOutputsDict(HeatmapTrackerLabeledOutputsDict):
    """``HeatmapTrackerMultiviewTransformer.get_loss_inputs_labeled``: the 3-D projection keys are filled only from camera
    calibration data and ``None`` otherwise (reference :66-74)."""
    keypoints_targ_3d: torch.Tensor | None
    keypoints_pred_3d: torch.Tensor | None
    keypoints_pred_2d_reprojected: torch.Tensor | None


class HeatmapTrackerUnlabeledOutputsDict(TypedDict):
    heatmaps_pred: torch.Tensor
    keypoints_pred: torch.Tensor
    keypoints_pred_augmented: torch.Tensor
    confidences: torch.Tensor
