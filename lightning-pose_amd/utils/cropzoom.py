"""File-level tools of the two-stage "crop-zoom" workflow (mirror of ``lightning_pose/utils/cropzoom.py``): boxes from a detector's prediction
table, their rolling-median smoothing, the labels of cropped frames, the cropped labeled frames themselves.  Same names, signatures, file
formats and error texts as the reference, so box files interchange with it.

These tools work at CSV scale on the host (numpy / pandas); their arithmetic is that of the device kernels (``ops.bbox_from_keypoints``,
``ops.bbox_smooth``; csrc/cropzoom.hip), which ``utils.predictions.predict_video_cropzoom`` runs instead of going through files:
double precision, sums over the keypoints in column order, pandas' centred rolling median rounded half to even.

Differences from the reference, all stated:
  * a frame whose anchor keypoints are not all finite, or whose box comes out with size 0, gets the box [0, 0, 0, 0] (the reference casts NaN to
    an integer or writes an empty crop and fails later);
  * ``crop_labeled_frames`` crops the frames the box table indexes; the reference additionally looks for their context frames
    (n - 2 .. n + 2) on disk and crops those with the centre frame's box - context models are not built here, so that lookup is left out;
  * ``crop_video`` is not built: there is no video encoder here, and ``predict_video_cropzoom`` crops on the device, from the decoded frames,
    without a cropped video ever existing.
"""

from __future__ import annotations

import json
import logging
from pathlib import Path
from typing import Any, Sequence

import numpy as np
import pandas as pd

logger = logging.getLogger(__name__)

__all__ = ["generate_bbox", "smooth_bbox", "crop_labeled_frames", "generate_cropped_csv_file"]


def _get(cfg: Any, key: str, default: Any = None) -> Any:
    if hasattr(cfg, "get"):
        return cfg.get(key, default)
    return getattr(cfg, key, default)


def _fix_empty_first_row(df: pd.DataFrame) -> pd.DataFrame:
    """``pd.read_csv`` with a multi-row header takes an all-NaN first data row for the index name: put that row back
    (the reference's utils/io.py ``fix_empty_first_row``)."""
    if df.index.name is None:
        return df
    first = pd.DataFrame(np.nan, index=pd.Index([df.index.name]), columns=df.columns, dtype="float64")
    out = pd.concat([first, df])
    out.index.name = None
    return out


def check_bbox_mode(crop_ratio, crop_height, crop_width) -> bool:
    """-> fixed-size mode?  Raises the reference's two errors (utils/cropzoom.py:100-104)."""
    fixed = crop_height is not None and crop_width is not None
    if fixed and crop_ratio is not None:
        raise ValueError("provide either crop_ratio or (crop_height, crop_width), not both.")
    if not fixed and crop_ratio is None:
        raise ValueError("one of crop_ratio or (crop_height, crop_width) must be provided.")
    return fixed


def anchor_indices(keypoint_names: Sequence[str], anchor_keypoints: Sequence[str]) -> list[int]:
    """Indices of the anchor keypoints in table order (the reference selects them with a column mask, so their order in
    ``anchor_keypoints`` does not matter); [] = every keypoint.  Unknown names: the reference's assertion."""
    if len(anchor_keypoints) == 0:
        return []
    invalid_keypoints = set(anchor_keypoints) - set(keypoint_names)
    assert not invalid_keypoints, f"Anchor keypoints not found in DataFrame: {invalid_keypoints}"
    wanted = set(anchor_keypoints)
    return [i for i, name in enumerate(keypoint_names) if name in wanted]


def bbox_from_keypoints(keypoints: np.ndarray, anchors: Sequence[int] = (), crop_ratio: float | None = None, crop_height: int | None = None,
                        crop_width: int | None = None) -> np.ndarray:
    """(N, K, 2) keypoints -> (N, 4) int64 [x, y, h, w]: lp_bbox_from_keypoints' arithmetic on the host (include/lp_hip.h), i.e. the
    reference's ``_compute_bbox_df`` with the sums taken in keypoint order and [0, 0, 0, 0] for a degenerate frame."""
    fixed = check_bbox_mode(crop_ratio, crop_height, crop_width)
    kp = np.asarray(keypoints, np.float64)
    sel = kp[:, list(anchors)] if len(anchors) else kp
    n, cnt = sel.shape[0], sel.shape[1]
    total = np.zeros((n, 2))
    for a in range(cnt):
        total = total + sel[:, a]
    finite = np.isfinite(sel).all(axis=(1, 2))
    safe = np.where(finite[:, None, None], sel, 0.0)
    if fixed:
        h = np.full(n, int(crop_height) + int(crop_height) % 2, np.int64)
        w = np.full(n, int(crop_width) + int(crop_width) % 2, np.int64)
    else:
        span = np.maximum(safe[:, :, 0].max(1) - safe[:, :, 0].min(1), safe[:, :, 1].max(1) - safe[:, :, 1].min(1))
        size = np.ceil(span * float(crop_ratio))
        size = np.where((size >= 1.0) & (size < 2.0 ** 30), size, 0.0).astype(np.int64)
        h = w = size + size % 2
    with np.errstate(invalid="ignore"):
        corner = np.trunc(np.where(finite[:, None], total, 0.0) / cnt - np.column_stack([h // 2, w // 2]))   # (sic) x moves by h // 2
    ok = finite & (h > 0) & (w > 0) & (np.abs(corner) < 2.0 ** 31).all(axis=1)
    box = np.column_stack([corner.astype(np.int64), h, w])
    return np.where(ok[:, None], box, 0)


def smooth_boxes(bbox: np.ndarray | pd.DataFrame, window: int) -> pd.DataFrame:
    """the reference's smoothing (utils/cropzoom.py:391-392) = lp_bbox_smooth's arithmetic: centred rolling median, rounded half to even"""
    df = bbox if isinstance(bbox, pd.DataFrame) else pd.DataFrame(np.asarray(bbox), columns=["x", "y", "h", "w"])
    return df.rolling(window=window, center=True, min_periods=1).median().round(0).astype(int)


def _compute_bbox_df(pred_df: pd.DataFrame, anchor_keypoints: list[str], crop_ratio: float | None = None, crop_height: int | None = None,
                     crop_width: int | None = None) -> pd.DataFrame:
    check_bbox_mode(crop_ratio, crop_height, crop_width)
    coords = pred_df.columns.get_level_values("coords")
    names = list(dict.fromkeys(pred_df.columns.get_level_values("bodyparts")[coords.isin(["x", "y"])]))
    anchors = anchor_indices(names, list(anchor_keypoints))
    keypoints = pred_df.loc[:, coords.isin(["x", "y"])].to_numpy().reshape(pred_df.shape[0], -1, 2)
    boxes = bbox_from_keypoints(keypoints, anchors, crop_ratio, crop_height, crop_width)
    return pd.DataFrame(boxes, index=pd.Index(pred_df.index), columns=pd.Index(["x", "y", "h", "w"]))


def generate_bbox(input_preds_file: Path, detector_cfg: Any, output_bbox_file: Path) -> None:
    """Boxes from a prediction table (``predict_video``'s CSV) -> a box CSV with columns x, y, h, w and the table's index.
    ``detector_cfg`` holds ``anchor_keypoints`` and either ``crop_ratio`` or ``crop_height`` / ``crop_width``."""
    # (round_trip: pandas' default parser is not correctly rounded; with it the table holds exactly the doubles that were written, so the boxes
    # equal the device path's, which never goes through text)
    pred_df = _fix_empty_first_row(pd.read_csv(input_preds_file, header=[0, 1, 2], index_col=0, float_precision="round_trip"))
    bbox_df = _compute_bbox_df(pred_df, list(_get(detector_cfg, "anchor_keypoints", None) or []), crop_ratio=_get(detector_cfg, "crop_ratio"),
                               crop_height=_get(detector_cfg, "crop_height"), crop_width=_get(detector_cfg, "crop_width"))
    output_bbox_file = Path(output_bbox_file)
    output_bbox_file.parent.mkdir(parents=True, exist_ok=True)
    bbox_df.to_csv(output_bbox_file)


def smooth_bbox(input_bbox_dir: Path, output_dir: Path, method: str = "median", window: int = 5) -> None:
    """Smooth every ``*_bbox.csv`` of ``input_bbox_dir`` into ``output_dir`` and record the parameters in ``metadata.json``."""
    supported_methods = ("median",)
    if method not in supported_methods:
        raise ValueError(f"unsupported method {method!r}; choose one of {supported_methods}.")
    input_bbox_dir, output_dir = Path(input_bbox_dir), Path(output_dir)
    bbox_files = sorted(input_bbox_dir.glob("*_bbox.csv"))
    if not bbox_files:
        raise ValueError(f"no *_bbox.csv files found in {input_bbox_dir}.")
    output_dir.mkdir(parents=True, exist_ok=True)
    for bbox_file in bbox_files:
        smooth_boxes(pd.read_csv(bbox_file, index_col=0), window).to_csv(output_dir / bbox_file.name)
        logger.info(f"smoothed {bbox_file.name} -> {output_dir / bbox_file.name}")
    metadata = {"method": method, "window": window, "source": str(input_bbox_dir.resolve())}
    (output_dir / "metadata.json").write_text(json.dumps(metadata, indent=2))


def generate_cropped_csv_file(input_csv_file: str | Path, input_bbox_file: str | Path, output_csv_file: str | Path, mode: str = "subtract") -> None:
    """Shift every x / y column of a label (or prediction) table by its row's box corner: "subtract" = frame -> crop coordinates,
    "add" = back.  Rows are matched by index."""
    if mode not in ("add", "subtract"):
        raise ValueError(f"{mode} is not a valid mode")
    csv_data = _fix_empty_first_row(pd.read_csv(input_csv_file, header=[0, 1, 2], index_col=0, float_precision="round_trip"))
    bbox_data = pd.read_csv(input_bbox_file, index_col=0)
    for col in csv_data.columns:
        if col[-1] in ("x", "y"):
            csv_data[col] = csv_data[col] - bbox_data[col[-1]] if mode == "subtract" else csv_data[col] + bbox_data[col[-1]]
    output_csv_file = Path(output_csv_file)
    output_csv_file.parent.mkdir(parents=True, exist_ok=True)
    csv_data.to_csv(output_csv_file)


def crop_labeled_frames(input_data_dir: Path, input_csv_file: Path, input_bbox_file: Path, output_data_dir: Path, output_csv_file: Path) -> None:
    """Crop the labeled frames a box table indexes (PIL ``crop``: zero padding outside the frame) into ``output_data_dir`` under the same
    relative paths, and write the labels in crop coordinates."""
    from PIL import Image

    input_data_dir, output_data_dir = Path(input_data_dir), Path(output_data_dir)
    bbox_df = pd.read_csv(input_bbox_file, index_col=0)
    output_data_dir.mkdir(parents=True, exist_ok=True)
    for img_path, row in bbox_df.iterrows():
        box = (int(row.x), int(row.y), int(row.x + row.w), int(row.y + row.h))
        target = output_data_dir / str(img_path)
        target.parent.mkdir(parents=True, exist_ok=True)
        with Image.open(input_data_dir / str(img_path)) as img:
            img.crop(box).save(target)
    generate_cropped_csv_file(input_csv_file=input_csv_file, input_bbox_file=input_bbox_file, output_csv_file=output_csv_file)
