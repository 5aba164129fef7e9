"""Metrics inside the prediction calls (utils/predictions.py, ``compute_metrics=True``): the tables made from the device-resident predictions
must equal, bit for bit, what ``compute_metrics_single`` computes from the files just written - values, columns, index and the written
metric files - and the default must leave return values and files exactly as a call without the keyword."""

import os

import numpy as np
import pandas as pd
import pytest
import torch

from tests.test_cropzoom_predict import _CentroidTracker, _video

NAMES = ["a", "b", "c"]
FIELDS = ("pixel_error_df", "temporal_norm_df", "pca_sv_df", "pca_mv_df")


class _Cfg(dict):
    __getattr__ = dict.get


def _cfg(h=32, w=40, pca=False, views=None):
    data = _Cfg(keypoint_names=NAMES, image_resize_dims=_Cfg(height=h, width=w))
    if pca:
        data.update(columns_for_singleview_pca=[0, 2], mirrored_column_matches=[[0], [1]])
    if views:
        data.update(view_names=views)
    return _Cfg(data=data, model=_Cfg(model_type="heatmap"), losses=_Cfg(pca_singleview=_Cfg(components_to_keep=0.9)))


class _EchoTracker(torch.nn.Module):
    """predictions travel in the batch: what a tracker returns is its business, the metrics only see the stacked rows"""

    def __init__(self, device):
        super().__init__()
        self.anchor = torch.nn.Parameter(torch.zeros(1, device=device))

    def predict_step(self, batch, batch_idx, return_heatmaps=False):
        kp = batch["keypoints_pred"]
        return kp, torch.full((kp.shape[0], kp.shape[1] // 2), 0.75, device=kp.device)


class _Labeled:
    def __init__(self, image_names, keypoints):
        self.image_names, self.keypoints, self.do_context = image_names, keypoints, False

    def __len__(self):
        return len(self.image_names)


class _Split:
    def __init__(self, indices):
        self.indices = indices


class _DataModule:
    """the slice of BaseDataModule that prediction and evaluation touch"""

    def __init__(self, dataset, preds, dev, batch=7, train=None):
        n = len(dataset)
        self.dataset, self._preds, self._dev, self._batch = dataset, preds, dev, batch
        self.train_dataset, self.val_dataset, self.test_dataset = _Split(list(range(0, n - 6))), _Split([n - 6, n - 5, n - 4]), _Split([n - 3, n - 2])
        self._train = train

    def full_labeled_dataloader(self):
        for lo in range(0, len(self._preds), self._batch):
            yield {"keypoints_pred": self._preds[lo:lo + self._batch].to(self._dev)}

    def pca_keypoints(self):
        return self._train


def _poses(seed, n, k=3):
    g = np.random.default_rng(seed)
    base, mixing = g.uniform(100.0, 900.0, 2 * k), g.normal(scale=30.0, size=(2, 2 * k))
    return (base + g.normal(size=(n, 2)) @ mixing + g.normal(scale=2.0, size=(n, 2 * k))).astype(np.float32)


def _same_tables(got, want, fields):
    for f in FIELDS:
        a, b = getattr(got, f), getattr(want, f)
        assert (a is not None) == (f in fields) and (b is not None) == (f in fields), f
        if a is None:
            continue
        assert list(a.columns) == list(b.columns) and list(a.index) == list(b.index), f
        names = [c for c in a.columns if c != "set"]
        av, bv = a[names].to_numpy(), b[names].to_numpy()
        assert av.dtype == bv.dtype == np.float64 and np.array_equal(np.ascontiguousarray(av).view(np.int64), np.ascontiguousarray(bv).view(np.int64)), f
        if "set" in a.columns:
            assert list(a["set"]) == list(b["set"])


def _files(folder):
    return {n: (folder / n).read_bytes() for n in sorted(os.listdir(folder))}


def _from_files(cfg, labels_file, preds_file, data_module, folder):
    """compute_metrics_single on the written prediction file: its tables, and the bytes of the metric files it (re)writes"""
    from lightning_pose_amd.metrics import compute_metrics_single

    before = _files(folder)
    result = compute_metrics_single(cfg, labels_file, preds_file, data_module=data_module)
    assert _files(folder) == before, "the files written from the device tables differ from compute_metrics_single's"
    return result


# ---- video ------------------------------------------------------------------------------------------------------------------------------
def _loader(dev, n=23, seq=8):
    from lightning_pose_amd.data.producers import FrameWindowSource, VideoFramePipeline

    pipe = VideoFramePipeline((32, 40), imgaug="default")
    return [pipe(w) for w in FrameWindowSource(_video(n), seq, device=dev)]


def test_predict_video_default_is_unchanged(stack_backend, tmp_path):
    from lightning_pose_amd.utils.predictions import predict_video

    dev = stack_backend
    tracker, loader = _CentroidTracker(dev), _loader(dev)
    (tmp_path / "a").mkdir(), (tmp_path / "b").mkdir()
    plain = predict_video("clip.mp4", tracker, loader, str(tmp_path / "a" / "clip.csv"), cfg=_cfg(), frame_count=23)
    off = predict_video("clip.mp4", tracker, loader, str(tmp_path / "b" / "clip.csv"), cfg=_cfg(), frame_count=23, compute_metrics=False)
    assert isinstance(off, pd.DataFrame) and off.equals(plain) and list(off.columns) == list(plain.columns)
    assert _files(tmp_path / "a") == _files(tmp_path / "b") and list(_files(tmp_path / "a")) == ["clip.csv"]


@pytest.mark.parametrize("with_pca", [False, True])
def test_predict_video_metrics_equal_the_file_path(stack_backend, tmp_path, with_pca):
    from lightning_pose_amd.data.datatypes import PredictionResult
    from lightning_pose_amd.utils.predictions import predict_video

    dev = stack_backend
    tracker, loader, cfg = _CentroidTracker(dev), _loader(dev), _cfg(pca=with_pca)
    dm = _DataModule(_Labeled([], None), None, dev, train=torch.from_numpy(_poses(1, 12))) if with_pca else None
    plain = predict_video("clip.mp4", tracker, loader, cfg=cfg, frame_count=23)
    out = tmp_path / "clip.csv"
    res = predict_video("clip.mp4", tracker, loader, str(out), cfg=cfg, frame_count=23, compute_metrics=True, data_module=dm)
    assert isinstance(res, PredictionResult) and res.predictions.equals(plain) and res.predictions.shape == (23, 9)      # the padded row is gone
    fields = ("temporal_norm_df", "pca_sv_df", "pca_mv_df") if with_pca else ("temporal_norm_df",)
    suffixes = {"temporal_norm_df": "temporal_norm", "pca_sv_df": "pca_singleview_error", "pca_mv_df": "pca_multiview_error"}
    assert sorted(os.listdir(tmp_path)) == sorted(["clip.csv"] + [f"clip_{suffixes[f]}.csv" for f in fields])
    _same_tables(res.metrics, _from_files(cfg, None, out, dm, tmp_path), fields)
    t = res.metrics.temporal_norm_df.to_numpy()
    assert t.shape == (23, 3) and np.isnan(t[0]).all() and (t[1:] > 0).all()
    d = res.to_dict()
    assert d["keypoint_names"] == NAMES and d["x"].shape == (23, 3) and np.array_equal(d["temporal_norm"], t, equal_nan=True) and d["pixel_error"] is None
    if with_pca:
        sv, mv = res.metrics.pca_sv_df.to_numpy(), res.metrics.pca_mv_df.to_numpy()
        assert np.isnan(sv[:, 1]).all() and not np.isnan(sv[:, [0, 2]]).any() and np.isnan(mv[:, 2]).all() and not np.isnan(mv[:, :2]).any()
    # without a prediction file nothing is written, the tables are the same
    before = _files(tmp_path)
    nofile = predict_video("clip.mp4", tracker, loader, cfg=cfg, frame_count=23, compute_metrics=True, data_module=dm)
    assert _files(tmp_path) == before
    _same_tables(nofile.metrics, res.metrics, fields)


def test_predict_video_multiview_metrics_per_view(stack_backend, tmp_path):
    from lightning_pose_amd.data.datatypes import MultiviewPredictionResult
    from lightning_pose_amd.utils.predictions import predict_video

    dev = stack_backend
    views, cfg = ["top", "side"], _cfg(views=["top", "side"])
    preds = torch.from_numpy(_poses(3, 24, k=6))                      # 3 windows of 8 for 21 frames: 3 padded rows
    loader = [{"keypoints_pred": preds[lo:lo + 8].to(dev)} for lo in range(0, 24, 8)]
    videos, outs = [f"s_{v}.mp4" for v in views], [str(tmp_path / f"s_{v}.csv") for v in views]
    plain = predict_video(videos, _EchoTracker(dev), loader, cfg=cfg, frame_count=21)
    res = predict_video(videos, _EchoTracker(dev), loader, outs, cfg=cfg, frame_count=21, compute_metrics=True)
    assert isinstance(plain, list) and isinstance(res, MultiviewPredictionResult) and list(res.predictions) == views == list(res.metrics)
    for i, v in enumerate(views):
        assert res.predictions[v].equals(plain[i]) and res.predictions[v].shape == (21, 9)
        np.testing.assert_array_equal(res.predictions[v].to_numpy()[:, 0::3], preds[:21, 6 * i:6 * i + 6:2].numpy().astype(np.float64))
        _same_tables(res.metrics[v], _from_files(cfg, None, outs[i], None, tmp_path), ("temporal_norm_df",))
    assert sorted(os.listdir(tmp_path)) == sorted([f"s_{v}{s}.csv" for v in views for s in ("", "_temporal_norm")])
    assert sorted(res.to_dict()) == sorted(views) and res.to_dict()["side"]["temporal_norm"].shape == (21, 3)


# ---- labeled sets -----------------------------------------------------------------------------------------------------------------------
def _write_labels(path, names, xy, visible):
    coords = ["x", "y", "visible"] if visible else ["x", "y"]
    cols = pd.MultiIndex.from_product([["me"], NAMES, coords], names=["scorer", "bodyparts", "coords"])
    table = np.concatenate([xy, np.where(np.isnan(xy[..., :1]), 0.0, 2.0)], axis=2) if visible else xy
    pd.DataFrame(table.reshape(len(xy), -1), index=names, columns=cols).to_csv(path)


@pytest.mark.parametrize("labels_from", ["file", "dataset"])
def test_predict_dataset_metrics_equal_the_file_path(stack_backend, tmp_path, labels_from):
    from lightning_pose_amd.data.datasets import parse_label_csv
    from lightning_pose_amd.data.datatypes import PredictionResult
    from lightning_pose_amd.utils.predictions import predict_dataset

    dev, n = stack_backend, 19
    names = [f"labeled-data/img{i:02d}.png" for i in range(n)]
    truth = _poses(5, n).astype(np.float64).reshape(n, 3, 2) / 3.0       # (values that fp32 does not hold: the cast matters)
    truth[4, 1] = np.nan
    _write_labels(tmp_path / "CollectedData.csv", names, truth, visible=True)
    preds = torch.from_numpy(truth.reshape(n, 6)).float().nan_to_num(200.0) + torch.from_numpy(_poses(6, n)) * 0.01
    parsed = parse_label_csv(str(tmp_path / "CollectedData.csv"))
    dm = _DataModule(_Labeled(parsed.image_names, parsed.keypoints), preds, dev, train=torch.from_numpy(_poses(7, 12)))
    cfg, out = _cfg(pca=True), tmp_path / "out" / "predictions.csv"
    out.parent.mkdir()
    plain = predict_dataset(_EchoTracker(dev), dm, str(tmp_path / "plain.csv"), cfg=cfg)
    res = predict_dataset(_EchoTracker(dev), dm, str(out), cfg=cfg, compute_metrics=True,
                          labels_file=str(tmp_path / "CollectedData.csv") if labels_from == "file" else None)
    assert isinstance(plain, pd.DataFrame) and isinstance(res, PredictionResult) and res.predictions.equals(plain)
    assert (tmp_path / "plain.csv").read_bytes() == out.read_bytes()
    fields = ("pixel_error_df", "pca_sv_df", "pca_mv_df")
    assert sorted(os.listdir(out.parent)) == ["predictions.csv", "predictions_pca_multiview_error.csv", "predictions_pca_singleview_error.csv",
                                              "predictions_pixel_error.csv"]
    _same_tables(res.metrics, _from_files(cfg, tmp_path / "CollectedData.csv", out, dm, out.parent), fields)
    err = res.metrics.pixel_error_df
    assert list(err.columns) == NAMES + ["set"] and list(err.index) == names
    assert list(err["set"]) == ["train"] * 13 + ["validation"] * 3 + ["test"] * 2 + ["unused"]
    assert np.isnan(err.loc[names[4], "b"]) and np.isnan(err[NAMES].to_numpy()).sum() == 1 and (err[NAMES].to_numpy()[np.isfinite(err[NAMES].to_numpy())] < 40).all()


def test_predict_dataset_multiview_metrics_per_view(stack_backend, tmp_path):
    from lightning_pose_amd.data.datasets import parse_label_csv
    from lightning_pose_amd.data.datatypes import MultiviewPredictionResult
    from lightning_pose_amd.utils.predictions import predict_dataset

    dev, n, views = stack_backend, 11, ["top", "side"]
    per_view = {}
    for i, v in enumerate(views):
        truth = _poses(20 + i, n).astype(np.float64).reshape(n, 3, 2) / 7.0
        truth[2 + i, i] = np.nan
        _write_labels(tmp_path / f"{v}.csv", [f"labeled-data/s_{v}/img{j:02d}.png" for j in range(n)], truth, visible=False)
        parsed = parse_label_csv(str(tmp_path / f"{v}.csv"))
        per_view[v] = _Labeled(parsed.image_names, parsed.keypoints)
    holder = _Labeled(per_view["top"].image_names, None)
    holder.dataset = per_view
    preds = torch.from_numpy(_poses(9, n, k=6))
    dm = _DataModule(holder, preds, dev, batch=4)
    cfg = _cfg(views=views)
    res = predict_dataset(_EchoTracker(dev), dm, str(tmp_path / "predictions.csv"), cfg=cfg, compute_metrics=True)
    assert isinstance(res, MultiviewPredictionResult) and list(res.metrics) == views
    for v in views:
        _same_tables(res.metrics[v], _from_files(cfg, tmp_path / f"{v}.csv", tmp_path / f"predictions_{v}.csv", None, tmp_path), ("pixel_error_df",))
        assert np.isnan(res.metrics[v].pixel_error_df[NAMES].to_numpy()).sum() == 1
    assert {f"predictions_{v}_pixel_error.csv" for v in views} <= set(os.listdir(tmp_path))
    files = [str(tmp_path / f"{v}.csv") for v in views]
    again = predict_dataset(_EchoTracker(dev), dm, str(tmp_path / "predictions.csv"), cfg=cfg, compute_metrics=True, labels_file=files)
    for v in views:
        _same_tables(again.metrics[v], res.metrics[v], ("pixel_error_df",))
    with pytest.raises(ValueError, match="one entry per view"):
        predict_dataset(_EchoTracker(dev), dm, str(tmp_path / "predictions.csv"), cfg=cfg, compute_metrics=True, labels_file=files[0])


# ---- crop-zoom --------------------------------------------------------------------------------------------------------------------------
def test_predict_video_cropzoom_metrics_equal_the_file_path(stack_backend, tmp_path):
    from lightning_pose_amd.data.datatypes import PredictionResult
    from lightning_pose_amd.utils.predictions import predict_video_cropzoom

    dev = stack_backend
    video, detector, pose = _video(), _CentroidTracker(dev), _CentroidTracker(dev)
    cfg_det, cfg_pose = _cfg(48, 64), _cfg(32, 40, pca=True)
    dm = _DataModule(_Labeled([], None), None, dev, train=torch.from_numpy(_poses(1, 12)))
    kw = dict(cfg_detector=cfg_det, cfg_pose=cfg_pose, sequence_length=8, smooth_window=4)
    detector_cfg = _Cfg(anchor_keypoints=["c", "a"], crop_ratio=3.0)
    (tmp_path / "a").mkdir(), (tmp_path / "b").mkdir()
    plain = predict_video_cropzoom("clip.mp4", detector, pose, video, detector_cfg, output_pred_file=str(tmp_path / "a" / "clip.csv"), **kw)
    res = predict_video_cropzoom("clip.mp4", detector, pose, video, detector_cfg, output_pred_file=str(tmp_path / "b" / "clip.csv"),
                                 compute_metrics=True, data_module=dm, **kw)
    assert isinstance(plain, pd.DataFrame) and isinstance(res, PredictionResult) and res.predictions.equals(plain)
    assert (tmp_path / "a" / "clip.csv").read_bytes() == (tmp_path / "b" / "clip.csv").read_bytes() and os.listdir(tmp_path / "a") == ["clip.csv"]
    fields = ("temporal_norm_df", "pca_sv_df", "pca_mv_df")
    _same_tables(res.metrics, _from_files(cfg_pose, None, tmp_path / "b" / "clip.csv", dm, tmp_path / "b"), fields)
    assert len(os.listdir(tmp_path / "b")) == 4 and res.metrics.temporal_norm_df.shape == (23, 3)


@pytest.mark.gpu
def test_predict_video_metrics_with_a_heatmap_tracker(tmp_path):
    """a real tracker (ResNet-50 ``HeatmapTracker``, random weights) on 32 frames of 128 x 128: the device tables against the file path"""
    from lightning_pose_amd.data.producers import FrameWindowSource, VideoFramePipeline
    from lightning_pose_amd.models import HeatmapTracker
    from lightning_pose_amd.utils.predictions import predict_video

    dev = torch.device("cuda:0")
    tracker = HeatmapTracker(num_keypoints=3, backbone="resnet50", pretrained=False, torch_seed=1, device=dev)
    pipe, cfg = VideoFramePipeline((128, 128), imgaug="default"), _cfg(128, 128, pca=True)
    loader = [pipe(w) for w in FrameWindowSource(_video(32, 128, 128, seed=2), 16, device=dev)]
    dm = _DataModule(_Labeled([], None), None, dev, train=torch.from_numpy(_poses(1, 12)))
    out = tmp_path / "clip.csv"
    res = predict_video("clip.mp4", tracker, loader, str(out), cfg=cfg, frame_count=32, compute_metrics=True, data_module=dm)
    assert res.predictions.shape == (32, 9) and np.isfinite(res.predictions.to_numpy()).all()
    _same_tables(res.metrics, _from_files(cfg, None, out, dm, tmp_path), ("temporal_norm_df", "pca_sv_df", "pca_mv_df"))
    assert np.isfinite(res.metrics.temporal_norm_df.to_numpy()[1:]).all()
