"""The file-level crop-zoom tools (lightning_pose_amd/utils/cropzoom.py) on a dataset written to a temporary directory, against the outputs of
the reference's own tools on the same inputs (tests/golden/cropzoom.npz, written by tests/golden/make_golden_cropzoom.py)."""

import json
import os

import numpy as np
import pandas as pd
import pytest
from PIL import Image

from lightning_pose_amd.utils import cropzoom as cz

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cropzoom.npz"))
BBOX_CASES = sorted({k.split("/")[1] for k in GOLDEN.files if k.startswith("bbox/")})


class _Cfg(dict):
    __getattr__ = dict.get


def _pred_csv(path, kp):
    n, k, _ = kp.shape
    cols = pd.MultiIndex.from_product([["heatmap_tracker"], [f"kp{i}" for i in range(k)], ["x", "y", "likelihood"]],
                                      names=["scorer", "bodyparts", "coords"])
    pd.DataFrame(np.concatenate([kp, np.full((n, k, 1), 0.9)], axis=2).reshape(n, 3 * k), columns=cols).to_csv(path)


def _detector_cfg(case):
    ratio, ch, cw = [None if np.isnan(v) else v for v in GOLDEN[f"bbox/{case}/params"]]
    cfg = _Cfg(anchor_keypoints=[f"kp{i}" for i in GOLDEN[f"bbox/{case}/anchors"]])
    if ratio is not None:
        cfg["crop_ratio"] = float(ratio)
    if ch is not None:
        cfg["crop_height"], cfg["crop_width"] = int(ch), int(cw)
    return cfg


@pytest.mark.parametrize("case", BBOX_CASES)
def test_generate_bbox_matches_reference(tmp_path, case):
    _pred_csv(tmp_path / "preds.csv", GOLDEN[f"bbox/{case}/keypoints"])
    out = tmp_path / "boxes" / "video_bbox.csv"          # the directory is created
    cz.generate_bbox(tmp_path / "preds.csv", _detector_cfg(case), out)
    got = pd.read_csv(out, index_col=0)
    assert list(got.columns) == ["x", "y", "h", "w"] and all(np.issubdtype(t, np.integer) for t in got.dtypes)
    assert list(got.index) == list(range(len(got)))
    np.testing.assert_array_equal(got.to_numpy(), GOLDEN[f"bbox/{case}/bbox"])


def test_generate_bbox_anchor_order_does_not_matter_and_errors(tmp_path):
    kp = GOLDEN["bbox/ratio_subset/keypoints"]
    _pred_csv(tmp_path / "preds.csv", kp)
    cz.generate_bbox(tmp_path / "preds.csv", _Cfg(anchor_keypoints=["kp3", "kp0", "kp2"], crop_ratio=1.5), tmp_path / "a_bbox.csv")
    np.testing.assert_array_equal(pd.read_csv(tmp_path / "a_bbox.csv", index_col=0).to_numpy(), GOLDEN["bbox/ratio_subset/bbox"])
    with pytest.raises(ValueError, match=r"provide either crop_ratio or \(crop_height, crop_width\), not both\."):
        cz.generate_bbox(tmp_path / "preds.csv", _Cfg(anchor_keypoints=[], crop_ratio=1.5, crop_height=8, crop_width=8), tmp_path / "b.csv")
    with pytest.raises(ValueError, match=r"one of crop_ratio or \(crop_height, crop_width\) must be provided\."):
        cz.generate_bbox(tmp_path / "preds.csv", _Cfg(anchor_keypoints=[], crop_height=8), tmp_path / "b.csv")
    with pytest.raises(AssertionError, match=r"Anchor keypoints not found in DataFrame: \{'tail'\}"):
        cz.generate_bbox(tmp_path / "preds.csv", _Cfg(anchor_keypoints=["kp0", "tail"], crop_ratio=1.5), tmp_path / "b.csv")


def test_generate_bbox_degenerate_rows_are_zero(tmp_path):
    """the stated deviation, on the host as in the kernel: a NaN anchor -> [0, 0, 0, 0]; an all-NaN first row survives the CSV round trip"""
    kp = GOLDEN["bbox/ratio_subset/keypoints"].copy()
    kp[0] = np.nan
    kp[5, 2, 1] = np.nan
    kp[7, 1, 0] = np.nan          # not an anchor
    _pred_csv(tmp_path / "preds.csv", kp)
    df = pd.read_csv(tmp_path / "preds.csv", header=[0, 1, 2], index_col=0)
    df.loc[0, df.columns.get_level_values("coords") == "likelihood"] = np.nan
    df.to_csv(tmp_path / "preds.csv")
    cz.generate_bbox(tmp_path / "preds.csv", _Cfg(anchor_keypoints=["kp0", "kp2", "kp3"], crop_ratio=1.5), tmp_path / "v_bbox.csv")
    got = pd.read_csv(tmp_path / "v_bbox.csv", index_col=0).to_numpy()
    want = GOLDEN["bbox/ratio_subset/bbox"].copy()
    want[[0, 5]] = 0
    assert got.shape == want.shape
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("window", [1, 2, 3, 4, 5, 6])
def test_smooth_bbox_matches_reference(tmp_path, window):
    src, dst = tmp_path / "raw", tmp_path / "smooth" / "deep"
    src.mkdir()
    for tag in ("n10", "n3", "n1"):
        pd.DataFrame(GOLDEN[f"smooth/{tag}/bbox"], columns=["x", "y", "h", "w"]).to_csv(src / f"{tag}_bbox.csv")
    pd.DataFrame(GOLDEN["smooth/n3/bbox"], columns=["x", "y", "h", "w"]).to_csv(src / "not_a_box_table.csv")
    cz.smooth_bbox(src, dst, window=window)
    assert sorted(p.name for p in dst.iterdir()) == ["metadata.json", "n10_bbox.csv", "n1_bbox.csv", "n3_bbox.csv"]
    for tag in ("n10", "n3", "n1"):
        got = pd.read_csv(dst / f"{tag}_bbox.csv", index_col=0)
        assert list(got.columns) == ["x", "y", "h", "w"]
        np.testing.assert_array_equal(got.to_numpy(), GOLDEN[f"smooth/{tag}/window{window}"])
    assert json.loads((dst / "metadata.json").read_text()) == {"method": "median", "window": window, "source": str(src.resolve())}


def test_smooth_bbox_errors(tmp_path):
    (tmp_path / "empty").mkdir()
    with pytest.raises(ValueError, match=r"unsupported method 'mean'; choose one of \('median',\)\."):
        cz.smooth_bbox(tmp_path / "empty", tmp_path / "out", method="mean")
    with pytest.raises(ValueError, match=r"no \*_bbox\.csv files found in "):
        cz.smooth_bbox(tmp_path / "empty", tmp_path / "out")
    assert not (tmp_path / "out").exists()


def _labels_csv(path, names, kp):
    n, k, _ = kp.shape
    cols = pd.MultiIndex.from_product([["scorer"], [f"kp{i}" for i in range(k)], ["x", "y"]], names=["scorer", "bodyparts", "coords"])
    pd.DataFrame(kp.reshape(n, 2 * k), columns=cols, index=names).to_csv(path)


def _labels(tmp_path):
    names, kp, bbox = [str(s) for s in GOLDEN["labels/names"]], GOLDEN["labels/keypoints"], GOLDEN["labels/bbox"]
    _labels_csv(tmp_path / "CollectedData.csv", names, kp)
    pd.DataFrame(bbox, columns=["x", "y", "h", "w"], index=names).to_csv(tmp_path / "labels_bbox.csv")
    return names, kp, bbox


def test_generate_cropped_csv_file_matches_reference_and_round_trips(tmp_path):
    names, kp, _ = _labels(tmp_path)
    cz.generate_cropped_csv_file(tmp_path / "CollectedData.csv", tmp_path / "labels_bbox.csv", tmp_path / "out" / "cropped.csv")
    cropped = pd.read_csv(tmp_path / "out" / "cropped.csv", header=[0, 1, 2], index_col=0)
    assert list(cropped.index) == names and list(cropped.columns.names) == ["scorer", "bodyparts", "coords"]
    np.testing.assert_array_equal(cropped.to_numpy().reshape(kp.shape), GOLDEN["labels/subtract"])
    cz.generate_cropped_csv_file(tmp_path / "out" / "cropped.csv", tmp_path / "labels_bbox.csv", tmp_path / "restored.csv", mode="add")
    restored = pd.read_csv(tmp_path / "restored.csv", header=[0, 1, 2], index_col=0).to_numpy().reshape(kp.shape)
    np.testing.assert_array_equal(restored, GOLDEN["labels/add"])
    np.testing.assert_array_equal(restored, kp)           # subtract, then add: the labels (NaN where they were NaN)
    with pytest.raises(ValueError, match="multiply is not a valid mode"):
        cz.generate_cropped_csv_file(tmp_path / "CollectedData.csv", tmp_path / "labels_bbox.csv", tmp_path / "x.csv", mode="multiply")


def test_crop_labeled_frames_pixels_equal_pil_crop(tmp_path):
    names, kp, bbox = _labels(tmp_path)
    rng = np.random.default_rng(3)
    images = {}
    for name in names:
        (tmp_path / "data" / name).parent.mkdir(parents=True, exist_ok=True)
        images[name] = rng.integers(0, 256, size=(90, 130, 3), dtype=np.uint8)
        Image.fromarray(images[name]).save(tmp_path / "data" / name)
    assert (bbox[:, 1] < 0).any() and (bbox[:, 0] + bbox[:, 3] > 130).any() and (bbox[:, 1] + bbox[:, 2] > 90).any()   # boxes overhang the top, right and bottom edges
    cz.crop_labeled_frames(tmp_path / "data", tmp_path / "CollectedData.csv", tmp_path / "labels_bbox.csv", tmp_path / "cropped",
                           tmp_path / "cropped" / "CollectedData.csv")
    for name, (x, y, h, w) in zip(names, bbox.tolist()):
        got = np.asarray(Image.open(tmp_path / "cropped" / name))
        want = np.asarray(Image.fromarray(images[name]).crop((x, y, x + w, y + h)))
        assert got.shape == (h, w, 3)
        np.testing.assert_array_equal(got, want)
        pad = np.zeros((h, w, 3), np.uint8)            # PIL pads with zeros: the rule lp_frames_crop_resize restates
        y0, y1, x0, x1 = max(y, 0), min(y + h, 90), max(x, 0), min(x + w, 130)
        if y1 > y0 and x1 > x0:         # (two boxes start below the frame: their crops are all padding)
            pad[y0 - y:y1 - y, x0 - x:x1 - x] = images[name][y0:y1, x0:x1]
        np.testing.assert_array_equal(got, pad)
    cropped = pd.read_csv(tmp_path / "cropped" / "CollectedData.csv", header=[0, 1, 2], index_col=0)
    np.testing.assert_array_equal(cropped.to_numpy().reshape(kp.shape), GOLDEN["labels/subtract"])
