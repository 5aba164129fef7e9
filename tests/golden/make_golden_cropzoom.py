"""Generate tests/golden/cropzoom.npz: inputs and outputs of the reference's OWN crop-zoom file tools (its utils/cropzoom.py, loaded by path:
``_compute_bbox_df``, ``smooth_bbox``, ``generate_cropped_csv_file``).  Build container only (needs the reference tree):

    python tests/golden/make_golden_cropzoom.py [path/to/reference]

The module's imports that are not installed here (cv2, moviepy, omegaconf, tqdm) and its ``lightning_pose.utils.io`` are stubbed in
``sys.modules``: none of the three recorded functions calls into them, except ``io.fix_empty_first_row``, which is the identity on tables
whose first row holds a value (every table written here).  The file holds arrays and name lists only.

Keypoints lie on a 1/8-px grid below 4096, so every sum over the keypoints is exact in double precision and the recorded boxes do not depend
on the order of summation (numpy's ``mean`` and a kernel's loop agree)."""

from __future__ import annotations

import importlib.util
import os
import sys
import tempfile
import types
from pathlib import Path

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle.ref_loader import REFERENCE_ROOT  # noqa: E402  (where the build container keeps the reference tree)

SCORER = "heatmap_tracker"

# name -> (N, K, anchor indices, crop_ratio, crop_height, crop_width); "rows" cases are spelled out in bbox_inputs()
BBOX_CASES = {
    "ratio_subset": (12, 5, [0, 2, 3], 1.5, None, None),
    "ratio_all": (12, 5, [], 1.25, None, None),
    "fixed_odd": (12, 5, [1, 4], None, 101, 64),     # 101 x 64 -> 102 x 64; x moves by h // 2 = 51, y by w // 2 = 32
    "negative_corner": (4, 2, [], None, 20, 20),      # centroids 3.5, 0.5, 9.875, 10: corners -6.5 -> -6, -9.5 -> -9, -0.125 -> 0, 0
    "odd_size": (3, 2, [], 1.0, None, None),          # spans 7, 6.125, 8: sizes 7 -> 8, ceil 7 -> 8, 8
    "single_frame": (1, 4, [0, 3], 2.0, None, None),
}
SMOOTH_SHAPES = {"n10": 10, "n3": 3, "n1": 1}
SMOOTH_WINDOWS = (1, 2, 3, 4, 5, 6)


def keypoint_names(k: int) -> list[str]:
    return [f"kp{i}" for i in range(k)]


def bbox_inputs(name: str) -> np.ndarray:
    """(N, K, 2) float64 keypoints of a case"""
    n, k = BBOX_CASES[name][:2]
    if name == "negative_corner":
        c = np.array([[3.5, 0.5], [0.5, 3.5], [9.875, 10.0], [10.0, 9.875]])
        return np.stack([c - 1.0, c + 1.0], axis=1)
    if name == "odd_size":
        return np.array([[[100.0, 50.0], [107.0, 52.0]], [[30.0, 10.0], [31.0, 16.125]], [[8.0, 200.0], [16.0, 204.0]]])
    rng = np.random.default_rng(sum(map(ord, name)))
    centre = rng.integers(200 * 8, 3800 * 8, size=(n, 1, 2))
    return (centre + rng.integers(-150 * 8, 150 * 8, size=(n, k, 2))).clip(0, 4096 * 8 - 1) / 8.0


def smooth_inputs(n: int) -> np.ndarray:
    """(N, 4) int64 boxes: x, y random walks; h takes both parities next to each other, so the even-count medians at the edges end in .5
    with an even and with an odd floor; w is the same pattern negated"""
    rng = np.random.default_rng(100 + n)
    xy = np.cumsum(rng.integers(-9, 10, size=(n, 2)), axis=0) + np.array([40, -3])
    h = np.array([0, 1, 3, 4, 2, 7, 5, 5, 10, 13])[:n] if n > 1 else np.array([6])
    return np.column_stack([xy, h, -h]).astype(np.int64)


def pred_table(kp: np.ndarray) -> pd.DataFrame:
    n, k, _ = kp.shape
    cols = pd.MultiIndex.from_product([[SCORER], keypoint_names(k), ["x", "y", "likelihood"]], names=["scorer", "bodyparts", "coords"])
    arr = np.concatenate([kp, np.full((n, k, 1), 0.9)], axis=2).reshape(n, 3 * k)
    return pd.DataFrame(arr, columns=cols)


def labels_fixture() -> tuple[list[str], np.ndarray, np.ndarray]:
    """image names, (N, K, 2) labels with two NaN keypoints, (N, 4) boxes"""
    names = [f"labeled-data/vid{i // 3}/img{i:04d}.png" for i in range(6)]
    rng = np.random.default_rng(7)
    kp = rng.integers(0, 300 * 8, size=(6, 3, 2)) / 8.0
    kp[1, 2] = np.nan
    kp[4, 0] = np.nan
    bbox = np.column_stack([rng.integers(-20, 120, size=6), rng.integers(-20, 120, size=6), np.full(6, 64), np.full(6, 48)])
    return names, kp, bbox.astype(np.int64)


def labels_table(names: list[str], kp: np.ndarray) -> pd.DataFrame:
    n, k, _ = kp.shape
    cols = pd.MultiIndex.from_product([["scorer"], keypoint_names(k), ["x", "y"]], names=["scorer", "bodyparts", "coords"])
    return pd.DataFrame(kp.reshape(n, 2 * k), columns=cols, index=names)


def load_reference_cropzoom(ref_root: str):
    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    def fix_empty_first_row(df):
        assert df.index.name is None, "a table of this fixture starts with a row of values"
        return df

    stub("cv2")
    stub("tqdm", tqdm=lambda it, **kw: it)
    stub("moviepy", VideoFileClip=object)
    stub("omegaconf", DictConfig=dict)
    io = stub("lightning_pose.utils.io", fix_empty_first_row=fix_empty_first_row)
    stub("lightning_pose.utils", io=io)
    stub("lightning_pose")
    spec = importlib.util.spec_from_file_location("_reference_cropzoom", os.path.join(ref_root, "lightning_pose", "utils", "cropzoom.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main() -> None:
    ref = load_reference_cropzoom(sys.argv[1] if len(sys.argv) > 1 else REFERENCE_ROOT)
    out: dict[str, np.ndarray] = {}
    for name, (n, k, anchors, ratio, ch, cw) in BBOX_CASES.items():
        kp = bbox_inputs(name)
        assert kp.shape == (n, k, 2) and np.all(kp * 8 == np.round(kp * 8)) and kp.max() < 4096
        names = keypoint_names(k)
        df = ref._compute_bbox_df(pred_table(kp), [names[a] for a in anchors], crop_ratio=ratio, crop_height=ch, crop_width=cw)
        assert list(df.columns) == ["x", "y", "h", "w"]
        out[f"bbox/{name}/keypoints"] = kp
        out[f"bbox/{name}/anchors"] = np.asarray(anchors, np.int64)
        out[f"bbox/{name}/params"] = np.array([np.nan if v is None else float(v) for v in (ratio, ch, cw)])
        out[f"bbox/{name}/bbox"] = df.to_numpy().astype(np.int64)
    with tempfile.TemporaryDirectory() as tmp:
        tmp = Path(tmp)
        for tag, n in SMOOTH_SHAPES.items():
            raw = smooth_inputs(n)
            src = tmp / f"raw_{tag}"
            src.mkdir()
            pd.DataFrame(raw, columns=["x", "y", "h", "w"]).to_csv(src / "video_bbox.csv")
            out[f"smooth/{tag}/bbox"] = raw
            for window in SMOOTH_WINDOWS:
                dst = tmp / f"smooth_{tag}_{window}"
                ref.smooth_bbox(src, dst, method="median", window=window)
                got = pd.read_csv(dst / "video_bbox.csv", index_col=0)
                assert list(got.columns) == ["x", "y", "h", "w"]
                out[f"smooth/{tag}/window{window}"] = got.to_numpy().astype(np.int64)
        names, kp, bbox = labels_fixture()
        labels_table(names, kp).to_csv(tmp / "labels.csv")
        pd.DataFrame(bbox, columns=["x", "y", "h", "w"], index=names).to_csv(tmp / "labels_bbox.csv")
        ref.generate_cropped_csv_file(tmp / "labels.csv", tmp / "labels_bbox.csv", tmp / "cropped.csv", mode="subtract")
        ref.generate_cropped_csv_file(tmp / "cropped.csv", tmp / "labels_bbox.csv", tmp / "restored.csv", mode="add")
        cropped = pd.read_csv(tmp / "cropped.csv", header=[0, 1, 2], index_col=0)
        restored = pd.read_csv(tmp / "restored.csv", header=[0, 1, 2], index_col=0)
        out["labels/names"] = np.array(names)
        out["labels/keypoints"] = kp
        out["labels/bbox"] = bbox
        out["labels/subtract"] = cropped.to_numpy().reshape(kp.shape)
        out["labels/add"] = restored.to_numpy().reshape(kp.shape)
        assert list(cropped.index) == names
    path = os.path.join(HERE, "cropzoom.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
