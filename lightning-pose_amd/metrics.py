"""Evaluation of a prediction table: pixel error, temporal norm and the PCA reprojection errors (reference: lightning_pose/metrics.py).

Same five names, signatures and return conventions as the reference - the array functions return float64 numpy arrays of shape
(samples, n_keypoints), ``compute_metrics_single`` reads a prediction CSV (+ the label CSV), writes ``<stem>_pixel_error.csv`` /
``_temporal_norm.csv`` / ``_pca_singleview_error.csv`` / ``_pca_multiview_error.csv`` next to it and returns the tables - but the arithmetic
is ONE launch of ``lp_kp_metrics`` (csrc/metrics.hip) over the table on the device; the reference goes CSV -> pandas -> numpy / CPU torch.
The array functions take numpy arrays or torch tensors, on the host or on the device; host data is moved to the current ROCm device (there
is no CPU path: without a device ``ops`` raises ``LpHipUnavailable``).  Values are computed in fp32, as the reference's torch paths are.

The prediction calls of ``utils.predictions`` (``compute_metrics=True``) use ``metric_tables`` / ``metrics_result`` directly on the stacked
device predictions, so nothing is read back before the tables are made.

CSV conventions (reference metrics.py:1-22): three header rows (scorer / bodyparts / coords); label coords are ``x``, ``y`` and optionally
``visible``; prediction coords are ``x``, ``y``, ``likelihood``; a trailing column whose first level is ``set`` marks a labeled set (pixel
error) as opposed to a video (temporal norm).
"""

from __future__ import annotations

import os
from pathlib import Path
from typing import Any

import numpy as np
import pandas as pd
import torch

from . import ops
from .data.datatypes import ComputeMetricsSingleResult
from .utils.pca import KeypointPCA

__all__ = ["pixel_error", "temporal_norm", "pca_singleview_reprojection_error", "pca_multiview_reprojection_error", "compute_metrics_single"]

# metric table (ops.keypoint_metrics) -> (field of ComputeMetricsSingleResult, file suffix)
_OUTPUTS = {"pixel_error": ("pixel_error_df", "_pixel_error.csv"), "temporal_norm": ("temporal_norm_df", "_temporal_norm.csv"),
            "pca_singleview_error": ("pca_sv_df", "_pca_singleview_error.csv"), "pca_multiview_error": ("pca_mv_df", "_pca_multiview_error.csv")}


def _get(cfg: Any, key: str, default: Any = None) -> Any:
    """cfg may be an omegaconf DictConfig, a plain dict, or any attribute container."""
    if cfg is None:
        return default
    if hasattr(cfg, "get"):
        return cfg.get(key, default)
    return getattr(cfg, key, default)


def _on_device(x, device: torch.device | None = None) -> torch.Tensor:
    """numpy / host tensor / device tensor -> fp32 tensor on the device the kernel runs on (a device tensor stays where it is)"""
    t = x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))
    t = t.detach().to(torch.float32)
    if device is not None:
        return t.to(device)
    if not t.is_cuda and torch.cuda.is_available():
        return t.to(torch.device("cuda", torch.cuda.current_device()))
    return t   # (a host without a device: ops.require_device refuses it)


def _as_txk2(t: torch.Tensor) -> torch.Tensor:
    return t.reshape(t.shape[0], -1, 2)


def _host64(t: torch.Tensor) -> np.ndarray:
    return t.cpu().numpy().astype(np.float64)


def pixel_error(keypoints_true, keypoints_pred) -> np.ndarray:
    """(samples, n_keypoints, 2) x 2 -> (samples, n_keypoints): Euclidean distance, NaN where a coordinate of either is NaN"""
    pred = _on_device(keypoints_pred)
    true = _on_device(keypoints_true, pred.device)
    if true.shape != pred.shape:
        raise ValueError(f"operands could not be broadcast together with shapes {tuple(true.shape)} {tuple(pred.shape)}")
    return _host64(ops.keypoint_metrics(_as_txk2(pred), _as_txk2(true), temporal=False)["pixel_error"])


def temporal_norm(keypoints_pred) -> np.ndarray:
    """(samples, n_keypoints * 2) or (samples, n_keypoints, 2) -> (samples, n_keypoints): norm of the difference between successive rows;
    the first row is NaN"""
    return _host64(ops.keypoint_metrics(_as_txk2(_on_device(keypoints_pred)))["temporal_norm"])


def _pca_error(keypoints_pred, pca: KeypointPCA, loss_type: str) -> np.ndarray:
    if pca.loss_type != loss_type:
        raise ValueError(f"expected a {loss_type} KeypointPCA, got {pca.loss_type}")
    pred = _as_txk2(_on_device(keypoints_pred))
    spec = ops.PcaMetricSpec.from_pca(pca, int(pred.shape[1]), pred.device)
    sv = loss_type == "pca_singleview"
    out = ops.keypoint_metrics(pred, pca_singleview=spec if sv else None, pca_multiview=None if sv else spec, temporal=False)
    return _host64(out[loss_type + "_error"])


def pca_singleview_reprojection_error(keypoints_pred, pca: KeypointPCA) -> np.ndarray:
    """(samples, n_keypoints, 2) + a fitted pca_singleview ``KeypointPCA`` -> (samples, n_keypoints): distance of every selected keypoint to
    its reprojection from the kept subspace; keypoints outside ``columns_for_singleview_pca`` are NaN"""
    return _pca_error(keypoints_pred, pca, "pca_singleview")


def pca_multiview_reprojection_error(keypoints_pred, pca: KeypointPCA) -> np.ndarray:
    """(samples, n_keypoints, 2) + a fitted pca_multiview ``KeypointPCA`` -> (samples, n_keypoints): per view, the distance of every matched
    keypoint to its reprojection; keypoints outside ``mirrored_column_matches`` are NaN"""
    assert pca.mirrored_column_matches is not None
    return _pca_error(keypoints_pred, pca, "pca_multiview")


# ---- helpers the reference takes from utils/io.py ---------------------------------------------------------------------------------------
def get_keypoint_names(cfg: Any = None, csv_file: str | None = None, header_rows: list | None = [0, 1, 2]) -> list[str]:
    """keypoint names from a DLC-style CSV (the columns whose coord is ``x``, in file order), else ``bp_<n>`` from ``cfg.data.num_targets``
    (reference utils/io.py:149-187)"""
    if csv_file is not None and os.path.exists(csv_file):
        if header_rows is None:
            header_rows = list(_get(_get(cfg, "data"), "header_rows", None) or [0, 1, 2])
        columns = pd.read_csv(csv_file, header=header_rows, nrows=5).columns
        if header_rows in ([1, 2], [0, 1]):
            return [c[0] for c in columns if c[1] == "x"]
        return [c[1] for c in columns if c[2] == "x"]
    assert cfg is not None, "cfg must be provided when csv_file is not given"
    return [f"bp_{n}" for n in range(int(_get(_get(cfg, "data"), "num_targets")) // 2)]


def fix_empty_first_row(df: pd.DataFrame) -> pd.DataFrame:
    """``pd.read_csv`` takes an all-NaN first data row for the index name (pandas issue 21995): put it back as a NaN row
    (reference utils/io.py:529-554)"""
    if df.index.name is None:
        return df
    first = pd.DataFrame({c: np.nan for c in df.columns}, index=pd.Index([df.index.name]), columns=df.columns, dtype="float64")
    fixed = pd.concat([first, df])
    assert fixed.index.name is None
    return fixed


# ---- which metrics, and the PCA fits ----------------------------------------------------------------------------------------------------
def _pca_wanted(cfg: Any, data_module: Any) -> tuple[bool, bool]:
    """(pca_singleview, pca_multiview) under the reference's conditions (metrics.py:226-239)"""
    from .data.datasets import MultiviewHeatmapDataset

    if data_module is None or isinstance(data_module.dataset, MultiviewHeatmapDataset):
        return False, False
    data = _get(cfg, "data")
    sv, mv = _get(data, "columns_for_singleview_pca", None), _get(data, "mirrored_column_matches", None)
    return sv is not None and len(sv) != 0, mv is not None and len(mv) != 0


def _fit_pcas(cfg: Any, data_module: Any) -> dict[str, KeypointPCA]:
    """the fitted ``KeypointPCA`` per PCA metric that applies; a single-view fit that fails with "cannot fit PCA" is left out silently, as the
    reference does (metrics.py:301-303).  Both take their settings from ``cfg.losses.pca_singleview`` (sic, reference :310-313)."""
    want_sv, want_mv = _pca_wanted(cfg, data_module)
    if not (want_sv or want_mv):
        return {}
    settings = _get(_get(cfg, "losses"), "pca_singleview")
    common = dict(data_module=data_module, components_to_keep=_get(settings, "components_to_keep"),
                  empirical_epsilon_percentile=_get(settings, "empirical_epsilon_percentile", 1.0))
    fitted = {}
    if want_sv:
        try:
            pca = KeypointPCA(loss_type="pca_singleview", columns_for_singleview_pca=_get(_get(cfg, "data"), "columns_for_singleview_pca"),
                              centering_method=_get(settings, "centering_method", None), **common)
            pca()
            fitted["pca_singleview"] = pca
        except ValueError as e:
            if "cannot fit PCA" not in str(e):
                raise
    if want_mv:
        pca = KeypointPCA(loss_type="pca_multiview", mirrored_column_matches=_get(_get(cfg, "data"), "mirrored_column_matches"), **common)
        pca()
        fitted["pca_multiview"] = pca
    return fitted


def metric_tables(keypoints_pred: torch.Tensor, keypoints_true: torch.Tensor | None, cfg: Any, data_module: Any = None, *,
                  is_video: bool) -> dict[str, torch.Tensor]:
    """The reference's choice of metrics (video -> temporal norm, labeled set -> pixel error, PCA under ``_pca_wanted``) for one table of
    DEVICE predictions (T, K, 2) or (T, 2K), in one launch: name -> (T, K) fp32 device tensor."""
    if not is_video:
        assert keypoints_true is not None, '"pixel_error" metric requires labels'
    pred = _as_txk2(keypoints_pred)
    specs = {name: ops.PcaMetricSpec.from_pca(pca, int(pred.shape[1]), pred.device) for name, pca in _fit_pcas(cfg, data_module).items()}
    return ops.keypoint_metrics(pred, None if is_video else _as_txk2(keypoints_true), specs.get("pca_singleview"), specs.get("pca_multiview"),
                                temporal=is_video)


def metrics_result(tables: dict[str, torch.Tensor], index, keypoint_names: list[str], set_column=None,
                   preds_file: str | Path | None = None) -> ComputeMetricsSingleResult:
    """device tables -> one float64 DataFrame per metric (rows ``index``, columns ``keypoint_names`` + ``set`` when given), written next to
    ``preds_file`` under the reference's names when a file name is given"""
    result = ComputeMetricsSingleResult()
    for name, (field, suffix) in _OUTPUTS.items():
        if name not in tables:
            continue
        df = pd.DataFrame(_host64(tables[name]), index=pd.Index(index), columns=pd.Index(keypoint_names))
        if set_column is not None:
            df["set"] = set_column
        if preds_file is not None:
            path = Path(preds_file)
            df.to_csv(path.with_name(path.stem + suffix))
        setattr(result, field, df)
    return result


def compute_metrics_single(cfg: Any, labels_file: str | Path | None, preds_file: str | Path, data_module: Any = None) -> ComputeMetricsSingleResult:
    """Compute the metrics of one single-view prediction CSV and write them next to it (reference metrics.py:187-327).

    ``labels_file``: the label CSV, required for a labeled set (pixel error); ``data_module``: required for the PCA metrics."""
    pred_df = pd.read_csv(preds_file, header=[0, 1, 2], index_col=0)
    keypoint_names = get_keypoint_names(cfg, csv_file=str(preds_file), header_rows=[0, 1, 2])
    xyl = pred_df.columns.get_level_values("coords").isin(["x", "y", "likelihood"])
    keypoints_pred = pred_df.loc[:, xyl].to_numpy().reshape(pred_df.shape[0], -1, 3)[:, :, :2]
    index = pred_df.index
    is_video = pred_df.keys()[-1][0] != "set"
    set_column = None if is_video else pred_df.iloc[:, -1].to_numpy()
    keypoints_true = None
    if not is_video:
        assert labels_file is not None, '"pixel_error" metric requires labels_file'
        labels_df = fix_empty_first_row(pd.read_csv(labels_file, header=[0, 1, 2], index_col=0))
        assert labels_df.index.equals(index)
        labels_df = labels_df.loc[:, labels_df.columns.get_level_values("coords").isin(["x", "y"])]
        keypoints_true = labels_df.to_numpy().reshape(labels_df.shape[0], -1, 2)
    pred = _on_device(np.ascontiguousarray(keypoints_pred))
    tables = metric_tables(pred, None if keypoints_true is None else _on_device(keypoints_true, pred.device), cfg, data_module, is_video=is_video)
    return metrics_result(tables, index, keypoint_names, set_column, preds_file)
