"""Batch-dict contracts consumed by the training step (reference: lightning_pose/data/datatypes.py:163-250) and the result containers of
prediction and evaluation (reference :33-109)."""

from __future__ import annotations

from dataclasses import dataclass
from typing import Any, TypedDict

import numpy as np
import pandas as pd
import torch


@dataclass
class ComputeMetricsSingleResult:
    """one table per metric that was computed (rows = the prediction table's index, one column per keypoint, plus ``set`` for a labeled set)"""

    pixel_error_df: pd.DataFrame | None = None
    temporal_norm_df: pd.DataFrame | None = None
    pca_sv_df: pd.DataFrame | None = None
    pca_mv_df: pd.DataFrame | None = None


@dataclass
class PredictionResult:
    predictions: pd.DataFrame
    metrics: ComputeMetricsSingleResult | None = None

    def to_dict(self) -> dict[str, Any]:
        """Predictions and metrics as a flat dict of named arrays, all (n_frames, n_keypoints) in the same row order: ``keypoint_names``,
        ``index``, ``x``, ``y``, ``confidence``, and ``pixel_error`` / ``temporal_norm`` / ``pca_singleview_error`` /
        ``pca_multiview_error`` (None where the metric was not computed)."""
        def _metric(df: pd.DataFrame | None) -> np.ndarray | None:
            if df is None:
                return None
            return df[[c for c in df.columns if c != "set"]].to_numpy()

        m = self.metrics
        return {
            "keypoint_names": list(self.predictions.columns.get_level_values(1).unique()),
            "index": list(self.predictions.index),
            "x": self.predictions.xs("x", level=2, axis=1).to_numpy(),
            "y": self.predictions.xs("y", level=2, axis=1).to_numpy(),
            "confidence": self.predictions.xs("likelihood", level=2, axis=1).to_numpy(),
            "pixel_error": _metric(m.pixel_error_df) if m else None,
            "temporal_norm": _metric(m.temporal_norm_df) if m else None,
            "pca_singleview_error": _metric(m.pca_sv_df) if m else None,
            "pca_multiview_error": _metric(m.pca_mv_df) if m else None,
        }


@dataclass
class MultiviewPredictionResult:
    predictions: dict[str, pd.DataFrame]
    metrics: dict[str, ComputeMetricsSingleResult] | None = None

    def to_dict(self) -> dict[str, dict[str, Any]]:
        """``PredictionResult.to_dict()`` per view, keyed by view name"""
        return {view: PredictionResult(predictions=df, metrics=self.metrics.get(view) if self.metrics else None).to_dict()
                for view, df in self.predictions.items()}


class HeatmapLabeledBatchDict(TypedDict):
    images: torch.Tensor      # (B, 3, H, W) or (B, V, 3, H, W)
    keypoints: torch.Tensor   # (B, 2K)
    heatmaps: torch.Tensor    # (B, K, h, w)
    bbox: torch.Tensor        # (B, 4) or (B, 4V)   rows [x, y, h, w]
    idxs: torch.Tensor


class MultiviewHeatmapLabeledBatchDict(TypedDict, total=False):
    images: torch.Tensor      # (B, V, 3, H, W)
    keypoints: torch.Tensor   # (B, 2 V K) model px
    heatmaps: torch.Tensor    # (B, V K, h, w)
    bbox: torch.Tensor        # (B, 4V)   [x, y, h, w] per view
    idxs: torch.Tensor
    num_views: torch.Tensor   # (B,)
    concat_order: list
    view_names: list
    # present when camera calibration is available ((B, 1) placeholders otherwise, as in the reference)
    keypoints_3d: torch.Tensor       # (B, K, 3)
    intrinsic_matrix: torch.Tensor   # (B, V, 3, 3)
    extrinsic_matrix: torch.Tensor   # (B, V, 3, 4)
    distortions: torch.Tensor        # (B, V, 4 | 5 | 8 | 12) OpenCV order


class UnlabeledBatchDict(TypedDict):
    frames: torch.Tensor      # (S, 3, H, W)
    transforms: torch.Tensor  # (2, 3) | (S, 2, 3) | (1,) sentinel
    bbox: torch.Tensor        # (S, 4)
    is_multiview: bool


class MultiviewUnlabeledBatchDict(TypedDict):
    frames: torch.Tensor      # (S, V, 3, H, W)
    transforms: torch.Tensor  # (V, 2, 3) | (V, 1, 1)
    bbox: torch.Tensor        # (S, 4V)
    is_multiview: bool


class SemiSupervisedHeatmapBatchDict(TypedDict):
    labeled: HeatmapLabeledBatchDict
    unlabeled: UnlabeledBatchDict
