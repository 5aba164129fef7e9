"""Inference path: ``predict_step`` batches -> DLC-style prediction tables.

Mirror of ``lightning_pose/utils/predictions.py`` for the part that sits directly after the hot path:
``PredictionHandler`` (:41-330), ``make_dlc_pandas_index`` (:551-570) and the prediction loop that
``predict_dataset`` / ``predict_video`` (:332-548) delegate to ``pl.Trainer.predict``.  Same names, argument meaning,
column layout and error behaviour; the arithmetic (trunk, head, fused decode incl. the bounding-box map) is the HIP
path behind ``HeatmapTracker.predict_step`` - nothing here computes keypoints on the host.

``predict_video_cropzoom`` is the reference's two-stage workflow (``litpose predict`` -> ``create_bbox`` -> ``smooth_bbox`` -> ``crop`` ->
``predict`` with ``bbox_file``; utils/cropzoom.py) in one call that never leaves the device between the two models.

With ``compute_metrics=True`` the three prediction calls also evaluate the table (reference: ``compute_metrics_single`` after every predict
call of its API): the stacked predictions go through ``lp_kp_metrics`` while still on the device, the metric files are written next to the
prediction file, and the call returns ``PredictionResult`` / ``MultiviewPredictionResult`` (data/datatypes.py).

Not mirrored (outside the hot path): video readers (DALI / pynvvc / OpenCV), labeled-video rendering.
``frame_count`` therefore takes the number of frames from the caller (``frame_count=...``) or from a reader-provided
``count_frames`` callable instead of opening the video with OpenCV.
"""

from __future__ import annotations

import os
from typing import Any, Callable, Iterable

import numpy as np
import pandas as pd
import torch


def _get(cfg: Any, key: str, default: Any = None) -> Any:
    """cfg may be an omegaconf DictConfig, a plain dict, or any attribute container."""
    if hasattr(cfg, "get"):
        return cfg.get(key, default)
    return getattr(cfg, key, default)


def make_dlc_pandas_index(cfg: Any, keypoint_names: list[str]) -> pd.MultiIndex:
    """Three-level (scorer, bodyparts, coords) column index; scorer = ``<model_type>_tracker`` (reference :551-570)."""
    model_type = _get(_get(cfg, "model"), "model_type")
    return pd.MultiIndex.from_product([[f"{model_type}_tracker"], list(keypoint_names), ["x", "y", "likelihood"]],
                                      names=["scorer", "bodyparts", "coords"])


class PredictionHandler:
    """Convert batches of model outputs into a prediction dataframe (reference :41-330)."""

    def __init__(self, cfg: Any, data_module: Any = None, video_file: str | None = None, *, frame_count: int | None = None,
                 count_frames: Callable[[str], int] | None = None) -> None:
        if data_module is None and video_file is None:
            raise ValueError("must pass either data_module or video_file")
        if _get(_get(cfg, "data"), "keypoint_names", None) is None:
            raise ValueError("must include `keypoint_names` field in cfg.data")
        self.cfg = cfg
        self.data_module = data_module
        self.video_file = video_file
        self._frame_count = frame_count
        self._count_frames = count_frames

    @property
    def frame_count(self) -> int:
        """Number of frames in the video or in the labeled dataset (reference :67-74)."""
        if self.video_file is not None:
            if self._frame_count is not None:
                return int(self._frame_count)
            if self._count_frames is not None:
                return int(self._count_frames(self.video_file))
            raise RuntimeError("video prediction needs frame_count=<n> or count_frames=<callable>: this package does not "
                               "open video files (the reference uses OpenCV, data/utils.py count_frames)")
        return len(self.data_module.dataset)

    @property
    def keypoint_names(self) -> list[str]:
        return list(_get(_get(self.cfg, "data"), "keypoint_names"))

    @property
    def do_context(self) -> bool:
        if self.data_module:
            return bool(self.data_module.dataset.do_context)
        return _get(_get(self.cfg, "model"), "model_type") == "heatmap_mhcrnn"

    def unpack_preds(self, preds: list[tuple[torch.Tensor, torch.Tensor]]) -> tuple[torch.Tensor, torch.Tensor]:
        """Stack per-batch (keypoints, confidences); for video loaders drop the padded rows of the last sequence and undo
        the two-frame shift of context models (reference :97-144)."""
        stacked_preds = torch.vstack([pred[0] for pred in preds])
        stacked_confs = torch.vstack([pred[1] for pred in preds])
        if self.video_file is not None:
            num_rows_to_discard = stacked_preds.shape[0] - self.frame_count
            if num_rows_to_discard > 0:
                stacked_preds = stacked_preds[:-num_rows_to_discard]
                stacked_confs = stacked_confs[:-num_rows_to_discard]
            if self.do_context:
                stacked_preds = self.fix_context_preds_confs(stacked_preds)
                zero_pad = _get(_get(self.cfg, "model"), "model_type") != "heatmap_mhcrnn"
                stacked_confs = self.fix_context_preds_confs(stacked_confs, zero_pad_confidence=zero_pad)
        return stacked_preds, stacked_confs

    def fix_context_preds_confs(self, stacked_preds: torch.Tensor, zero_pad_confidence: bool = False) -> torch.Tensor:
        """Row 0 of a context loader belongs to frame 2: shift by two, replicate the edges (reference :146-177)."""
        head = torch.tile(stacked_preds[0], (2, 1))
        combined = torch.vstack([head, stacked_preds[0:-2]])
        if combined.shape[0] == self.frame_count:
            combined[-2:, :] = combined[-3, :]
        else:
            n_pad = self.frame_count - combined.shape[0]
            combined = torch.vstack([combined, torch.tile(combined[0], (n_pad, 1))])
        if zero_pad_confidence:
            combined[:2, :] = 0.0
            combined[-2:, :] = 0.0
        return combined

    @staticmethod
    def make_pred_arr_undo_resize(keypoints_np: np.ndarray, confidence_np: np.ndarray) -> np.ndarray:
        """(n, 2K) + (n, K) -> (n, 3K) with columns (x, y, likelihood) per keypoint (reference :179-206)."""
        assert keypoints_np.shape[0] == confidence_np.shape[0]
        assert keypoints_np.shape[1] == confidence_np.shape[1] * 2
        num_joints = confidence_np.shape[-1]
        predictions = np.zeros((keypoints_np.shape[0], num_joints * 3))
        predictions[:, 0::3] = keypoints_np[:, 0::2]
        predictions[:, 1::3] = keypoints_np[:, 1::2]
        predictions[:, 2::3] = confidence_np
        return predictions

    def make_dlc_pandas_index(self, keypoint_names: list | None = None) -> pd.MultiIndex:
        return make_dlc_pandas_index(cfg=self.cfg, keypoint_names=keypoint_names or self.keypoint_names)

    def add_split_indices_to_df(self, df: pd.DataFrame) -> pd.DataFrame:
        """Column ("set", "", "") = train / validation / test / unused per labeled frame (reference :222-239)."""
        df["set"] = np.array(["unused"] * df.shape[0])
        splits = {"train": self.data_module.train_dataset.indices, "validation": self.data_module.val_dataset.indices,
                  "test": self.data_module.test_dataset.indices}
        for key, val in splits.items():
            df.loc[val, ("set", "", "")] = np.repeat(key, len(val))
        return df

    def __call__(self, preds: list[tuple[torch.Tensor, torch.Tensor]], is_multiview_video: bool = False):
        """Prediction table of one video / labeled dataset; a dict of tables keyed by view name for multiview models
        (reference :264-330)."""
        stacked_preds, stacked_confs = self.unpack_preds(preds=preds)
        view_names = _get(_get(self.cfg, "data"), "view_names", None)
        if view_names and len(view_names) > 1 and (self.video_file is None or is_multiview_video):
            num_keypoints = len(self.keypoint_names)
            view_to_df = {}
            for view_idx, view_name in enumerate(view_names):
                beg, end = view_idx * num_keypoints, (view_idx + 1) * num_keypoints
                pred_arr = self.make_pred_arr_undo_resize(stacked_preds[:, beg * 2:end * 2].cpu().numpy(),
                                                          stacked_confs[:, beg:end].cpu().numpy())
                df = pd.DataFrame(pred_arr, columns=self.make_dlc_pandas_index(self.keypoint_names))
                view_to_df[view_name] = df
                if self.video_file is None:
                    df = self.add_split_indices_to_df(df)
                    df.index = self.data_module.dataset.dataset[view_name].image_names
            return view_to_df
        pred_arr = self.make_pred_arr_undo_resize(stacked_preds.cpu().numpy(), stacked_confs.cpu().numpy())
        df = pd.DataFrame(pred_arr, columns=self.make_dlc_pandas_index())
        if self.video_file is None:
            df = self.add_split_indices_to_df(df)
            df.index = self.data_module.dataset.image_names
        return df


def predict_batches(model: Any, batches: Iterable[dict], return_heatmaps: bool = False) -> list[tuple[torch.Tensor, ...]]:
    """What ``pl.Trainer(...).predict(model, dataloaders=..., return_predictions=True)`` does for this module: eval mode
    (BatchNorm running statistics), no autograd tape, ``predict_step`` per batch.  Outputs stay on the device."""
    was_training = model.training
    model.eval()
    out = []
    try:
        with torch.no_grad():
            for batch_idx, batch in enumerate(batches):
                out.append(model.predict_step(batch, batch_idx, return_heatmaps=return_heatmaps))
    finally:
        model.train(was_training)
    return out


def _labels_on_device(labels_file: Any, index: pd.Index, dataset: Any, device: torch.device) -> torch.Tensor:
    """(N, K, 2) fp32 labels of a labeled table on ``device``: the label file read as ``compute_metrics_single`` reads it (x / y columns
    only, an all-NaN first row restored, the index checked against the predictions'), or - no file given - the dataset's own parsed
    labels.  Either way float64 file values narrowed to fp32 once, the cast ``compute_metrics_single`` applies."""
    if labels_file is None:
        assert list(dataset.image_names) == list(index)
        return dataset.keypoints.to(device)
    from ..metrics import fix_empty_first_row

    labels_df = fix_empty_first_row(pd.read_csv(labels_file, header=[0, 1, 2], index_col=0))
    assert labels_df.index.equals(index)
    labels_df = labels_df.loc[:, labels_df.columns.get_level_values("coords").isin(["x", "y"])]
    return torch.as_tensor(labels_df.to_numpy().reshape(labels_df.shape[0], -1, 2)).to(torch.float32).to(device)


def _table_metrics(keypoints: torch.Tensor, labels: torch.Tensor | None, df: pd.DataFrame, cfg: Any, data_module: Any, preds_file: Any):
    """``ComputeMetricsSingleResult`` of one single-view table from its DEVICE keypoints (T, 2K): what ``compute_metrics_single`` computes
    from the written file, without the round trip through it.  Files are written only next to a prediction file."""
    from .. import metrics

    is_video = df.keys()[-1][0] != "set"
    tables = metrics.metric_tables(keypoints, labels, cfg, data_module, is_video=is_video)
    return metrics.metrics_result(tables, df.index, [c[1] for c in df.columns if c[2] == "x"], None if is_video else df.iloc[:, -1].to_numpy(),
                                  preds_file)


def _per_view(stacked: torch.Tensor, num_keypoints: int, view_idx: int) -> torch.Tensor:
    return stacked[:, view_idx * num_keypoints * 2:(view_idx + 1) * num_keypoints * 2]


def predict_dataset(model: Any, data_module: Any, preds_file: str | list[str], cfg: Any = None, *, compute_metrics: bool = False,
                    labels_file: str | list[str] | None = None):
    """Predict every labeled frame and save the table(s) (reference :332-393).  ``model`` is the tracker itself or an object
    with ``.model`` / ``.config.cfg`` like the reference's API wrapper.

    ``compute_metrics=True``: pixel error (and the PCA metrics the cfg / data module call for) from the device predictions, written next to
    every prediction file; returns ``PredictionResult`` (``MultiviewPredictionResult``: each view evaluated as a single-view table, no PCA).
    ``labels_file`` (one per view for a multi-view dataset): the label CSV(s) to compare with; default: the dataset's own labels."""
    module = getattr(model, "model", model)
    cfg_eff = cfg if cfg is not None else model.config.cfg
    preds = predict_batches(module, data_module.full_labeled_dataloader())
    handler = PredictionHandler(cfg=cfg_eff, data_module=data_module, video_file=None)
    df = handler(preds=[(p[0], p[1]) for p in preds])
    if isinstance(df, dict):
        if isinstance(preds_file, str):
            files = [preds_file.replace(".csv", f"_{view_name}.csv") for view_name in df]
        else:
            assert list(df.keys()) == list(_get(_get(cfg_eff, "data"), "view_names"))
            if len(preds_file) != len(df):
                raise ValueError("preds_file must have one entry per view")
            files = list(preds_file)
        for d, f in zip(df.values(), files):
            d.to_csv(f)
    else:
        assert isinstance(preds_file, str), "preds_file must be a str for single-view predictions"
        df.to_csv(preds_file)
    if not compute_metrics:
        return df
    from ..data.datatypes import MultiviewPredictionResult, PredictionResult

    stacked = handler.unpack_preds(preds=[(p[0], p[1]) for p in preds])[0]
    if isinstance(df, dict):
        if labels_file is not None and (isinstance(labels_file, str) or len(labels_file) != len(df)):
            raise ValueError("labels_file must have one entry per view")
        k = len(handler.keypoint_names)
        results = {}
        for i, (view_name, d) in enumerate(df.items()):
            labels = _labels_on_device(None if labels_file is None else labels_file[i], d.index, data_module.dataset.dataset[view_name], stacked.device)
            results[view_name] = _table_metrics(_per_view(stacked, k, i), labels, d, cfg_eff, data_module, files[i])
        return MultiviewPredictionResult(predictions=df, metrics=results)
    labels = _labels_on_device(labels_file, df.index, data_module.dataset, stacked.device)
    return PredictionResult(predictions=df, metrics=_table_metrics(stacked, labels, df, cfg_eff, data_module, preds_file))


def predict_video(video_file: str | list[str], model: Any, predict_loader: Iterable[dict], output_pred_file: str | list[str] | None = None,
                  *, cfg: Any = None, frame_count: int | None = None, count_frames: Callable[[str], int] | None = None,
                  compute_metrics: bool = False, data_module: Any = None):
    """Predict one video (or one video per view) from a loader of ``{"frames", "bbox", ...}`` batches and save the table(s)
    (reference :416-548).  The loader is the caller's: building it from a file is the video producer's job (8f N1).

    ``compute_metrics=True``: the temporal norm (and, with ``data_module``, the PCA metrics its cfg calls for) of the device predictions
    after the padded rows are dropped, written next to every prediction file; returns ``PredictionResult``, or
    ``MultiviewPredictionResult`` keyed by view name (each view a single-view table)."""
    is_multiview = not isinstance(video_file, str)
    module = getattr(model, "model", model)
    cfg_eff = cfg if cfg is not None else model.config.cfg
    if is_multiview:
        if output_pred_file is not None and not isinstance(output_pred_file, list):
            raise ValueError("for multiview prediction, 'output_pred_file' should be a list corresponding to view_names")
        view_names = list(_get(_get(cfg_eff, "data"), "view_names"))
        if len(view_names) != len(video_file):
            raise ValueError("expected video_file to correspond 1-1 with cfg.data.view_names")
        for f, view_name in zip(video_file, view_names):
            assert view_name in os.path.splitext(os.path.basename(f))[0], \
                "expected video_file to correspond 1-1 with cfg.data.view_name"
    handler = PredictionHandler(cfg=cfg_eff, video_file=video_file[0] if is_multiview else video_file, frame_count=frame_count,
                                count_frames=count_frames)
    preds = predict_batches(module, predict_loader)
    df = handler(preds=[(p[0], p[1]) for p in preds], is_multiview_video=is_multiview)
    if isinstance(df, dict):
        df = [df[v] for v in _get(_get(cfg_eff, "data"), "view_names")]
    if output_pred_file is not None:
        if is_multiview:
            if len(output_pred_file) != len(df):
                raise ValueError("output_pred_file must have one entry per view")
            for d, f in zip(df, output_pred_file):
                os.makedirs(os.path.dirname(f) or ".", exist_ok=True)
                d.to_csv(f)
        else:
            df.to_csv(output_pred_file)
    if not compute_metrics:
        return df
    from ..data.datatypes import MultiviewPredictionResult, PredictionResult

    stacked = handler.unpack_preds(preds=[(p[0], p[1]) for p in preds])[0]
    if is_multiview:
        k = len(handler.keypoint_names)
        results = {v: _table_metrics(_per_view(stacked, k, i), None, d, cfg_eff, data_module, None if output_pred_file is None else output_pred_file[i])
                   for i, (v, d) in enumerate(zip(view_names, df))}
        return MultiviewPredictionResult(predictions=dict(zip(view_names, df)), metrics=results)
    return PredictionResult(predictions=df, metrics=_table_metrics(stacked, None, df, cfg_eff, data_module, output_pred_file))


def _resize_dims(cfg: Any) -> tuple[int, int]:
    dims = _get(_get(cfg, "data"), "image_resize_dims", None)
    if dims is None:
        raise ValueError("must include `image_resize_dims` (height, width) field in cfg.data")
    return int(_get(dims, "height")), int(_get(dims, "width"))


def predict_video_cropzoom(video_file: str, detector: Any, pose_model: Any, videos: Any, detector_cfg: Any, *, cfg_detector: Any = None,
                           cfg_pose: Any = None, sequence_length: int = 16, smooth_window: int | None = None,
                           output_pred_file: str | None = None, output_bbox_file: str | None = None,
                           output_detector_pred_file: str | None = None, resident_bytes: int = 4 << 30, border: str = "clamp",
                           compute_metrics: bool = False, data_module: Any = None):
    """Two-stage prediction of one decoded video (``videos``: a uint8 array / tensor (N, H, W, 3)): the detector on whole frames -> one box
    per frame from its keypoints (``detector_cfg``: ``anchor_keypoints`` and ``crop_ratio`` or ``crop_height`` / ``crop_width``, as
    ``utils.cropzoom.generate_bbox``) -> optionally their rolling median over ``smooth_window`` frames -> the pose model on every frame's own
    crop -> the pose model's table in ORIGINAL-frame coordinates (``predict_step`` maps through the per-frame ``bbox``).

    Keypoints and boxes stay on the device from the detector's decode to the crop kernel; nothing is read back before the tables are made.
    A video of at most ``resident_bytes`` keeps its device windows from the first pass for the second, so it crosses PCIe once.
    Optional files, in the reference's formats: the detector's table, the (smoothed) box table ``x, y, h, w`` indexed by frame, the pose table.
    Returns the pose table.  Single-view trackers only.

    ``compute_metrics=True``: the pose table's temporal norm (and, with ``data_module``, the PCA metrics ``cfg_pose`` calls for) from the
    device keypoints after the map back through the boxes, written next to ``output_pred_file``; returns ``PredictionResult``."""
    from .. import ops
    from ..data.producers import CropZoomFramePipeline, FrameWindowSource, VideoFramePipeline
    from .cropzoom import anchor_indices, check_bbox_mode

    if not isinstance(video_file, str):
        raise NotImplementedError("crop-zoom prediction is single-view: pass one video file name")
    det, pose = getattr(detector, "model", detector), getattr(pose_model, "model", pose_model)
    cfg_det = cfg_detector if cfg_detector is not None else detector.config.cfg
    cfg_pos = cfg_pose if cfg_pose is not None else pose_model.config.cfg
    crop_ratio, crop_height, crop_width = (_get(detector_cfg, k) for k in ("crop_ratio", "crop_height", "crop_width"))
    check_bbox_mode(crop_ratio, crop_height, crop_width)
    det_names = list(_get(_get(cfg_det, "data"), "keypoint_names"))
    anchors = anchor_indices(det_names, list(_get(detector_cfg, "anchor_keypoints", None) or []))
    if smooth_window is not None and not 1 <= int(smooth_window) <= ops.BBOX_SMOOTH_MAX_WINDOW:
        raise ValueError(f"smooth_window must lie in [1, {ops.BBOX_SMOOTH_MAX_WINDOW}], got {smooth_window}")

    device = next(det.parameters()).device
    source = FrameWindowSource(videos, sequence_length=sequence_length, device=device)
    if len(source.videos) != 1:
        raise NotImplementedError("crop-zoom prediction takes one video")
    n_frames, video = source.frame_count, source.videos[0]
    frame_bytes = int(np.prod(video.shape[1:]))
    resident = len(source) * source.sequence_length * frame_bytes <= int(resident_bytes)
    kept: list[torch.Tensor] = []

    def first_pass():
        pipe = VideoFramePipeline(_resize_dims(cfg_det), border=border)
        for window in source:
            if resident:
                kept.append(window)
            yield pipe(window)

    handler = PredictionHandler(cfg=cfg_det, video_file=video_file, frame_count=n_frames)
    det_preds = predict_batches(det, first_pass())
    keypoints = torch.vstack([p[0] for p in det_preds])[:n_frames]     # the padded tail goes BEFORE the boxes are smoothed
    boxes = ops.bbox_from_keypoints(keypoints, anchors, crop_ratio, crop_height, crop_width)
    if smooth_window is not None:
        boxes = ops.bbox_smooth(boxes, int(smooth_window))
    pad = len(source) * source.sequence_length - n_frames
    padded = boxes if pad == 0 else torch.cat([boxes, torch.zeros(pad, 4, dtype=boxes.dtype, device=boxes.device)])   # zero frames: no box

    def second_pass():
        pipe = CropZoomFramePipeline(_resize_dims(cfg_pos), border=border)
        for i, window in enumerate(kept if resident else source):
            yield pipe(window, padded[i * source.sequence_length:(i + 1) * source.sequence_length])

    pose_preds = predict_batches(pose, second_pass())
    kept.clear()
    pose_handler = PredictionHandler(cfg=cfg_pos, video_file=video_file, frame_count=n_frames)
    df = pose_handler(preds=[(p[0], p[1]) for p in pose_preds])
    for path, table in ((output_detector_pred_file, lambda: handler(preds=[(p[0], p[1]) for p in det_preds])),
                        (output_bbox_file, lambda: pd.DataFrame(boxes.cpu().numpy().astype(np.int64), columns=pd.Index(["x", "y", "h", "w"]))),
                        (output_pred_file, lambda: df)):
        if path is not None:
            os.makedirs(os.path.dirname(str(path)) or ".", exist_ok=True)
            table().to_csv(path)
    if compute_metrics:
        from ..data.datatypes import PredictionResult

        stacked = pose_handler.unpack_preds(preds=[(p[0], p[1]) for p in pose_preds])[0]
        return PredictionResult(predictions=df, metrics=_table_metrics(stacked, None, df, cfg_pos, data_module, output_pred_file))
    return df
