"""``lightning_pose_amd.metrics`` (the reference's five metric functions through lp_kp_metrics), ``BaseDataModule.pca_keypoints`` and the PCA
fits that stand on it (``PCALoss``, ``get_loss_factories``, the PCA metrics of ``compute_metrics_single``) - on a dataset written to disk."""

import os

import numpy as np
import pandas as pd
import pytest
import torch

from tests.test_metrics_kernel import case_inputs, restated

N, K, H, W = 30, 6, 128, 128
NAMES = ["nose", "ear", "paw", "hip", "knee", "tail"]
SIZES = [(40, 56), (48, 64)]                      # stored (height, width): two sizes, so the size of every file matters
SV_COLUMNS, MV_MATCHES = [0, 1, 2, 4], [[0, 1, 2], [3, 4, 5]]


class _Cfg(dict):
    __getattr__ = dict.get


def _cfg(sv=SV_COLUMNS, mv=MV_MATCHES, names=NAMES, **data):
    return _Cfg(data=_Cfg(keypoint_names=names, columns_for_singleview_pca=sv, mirrored_column_matches=mv, **data), model=_Cfg(model_type="heatmap"),
                losses=_Cfg(pca_singleview=_Cfg(components_to_keep=0.99), pca_multiview=_Cfg(components_to_keep=3)))


def _labels(seed, n=N, k=K):
    """stored-px labels off a 2-dimensional pose model, some unlabeled"""
    g = np.random.default_rng(seed)
    base, mixing = g.uniform(8.0, 34.0, 2 * k), g.normal(scale=2.0, size=(2, 2 * k))
    xy = (base + g.normal(size=(n, 2)) @ mixing + g.normal(scale=0.3, size=(n, 2 * k))).reshape(n, k, 2)
    xy[3, 1] = np.nan
    xy[7, k - 2] = np.nan
    return np.round(xy, 3)


def _write_view(root, folder, csv_name, xy, visible=False, first_row_nan=False):
    from PIL import Image

    g = np.random.default_rng(1)
    os.makedirs(os.path.join(root, "labeled-data", folder), exist_ok=True)
    names = [f"labeled-data/{folder}/img{i:03d}.png" for i in range(len(xy))]
    for i, n in enumerate(names):
        Image.fromarray(g.integers(0, 256, (*SIZES[i % 2], 3), dtype=np.uint8)).save(os.path.join(root, n))
    xy = xy.copy()
    if first_row_nan:
        xy[0] = np.nan
    coords = ["x", "y", "visible"] if visible else ["x", "y"]
    cols = pd.MultiIndex.from_product([["me"], NAMES[:xy.shape[1]], coords], names=["scorer", "bodyparts", "coords"])
    table = np.concatenate([xy, np.where(np.isnan(xy[..., :1]), 0.0, 2.0)], axis=2) if visible else xy
    pd.DataFrame(table.reshape(len(xy), -1), index=names, columns=cols).to_csv(os.path.join(root, csv_name))
    return names


@pytest.fixture(scope="module")
def disk(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("metrics_data"))
    xy = _labels(0)
    names = _write_view(root, "sess_top", "CollectedData.csv", xy, visible=True)
    _write_view(root, "sess_top", "FirstRowNaN.csv", xy, first_row_nan=True)
    views = {v: _labels(10 + i, k=3) for i, v in enumerate(["top", "side"])}
    for v, lab in views.items():
        _write_view(root, f"mv_{v}", f"{v}.csv", lab)
    return dict(root=root, xy=xy, names=names, views=views)


def _data_module(disk, dev, csv="CollectedData.csv", **kw):
    from lightning_pose_amd.data.datamodules import BaseDataModule
    from lightning_pose_amd.data.datasets import HeatmapDataset

    return BaseDataModule(HeatmapDataset(disk["root"], csv, H, W, device=dev), train_probability=0.8, val_probability=0.1, torch_seed=3, **kw)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _unaugmented_batches(ds, idx):
    """``batch(..., augment=False)["keypoints"]`` of these examples, row for row (a batch must hold images of one size: two batches)"""
    out = torch.empty(len(idx), ds.num_targets)
    for parity in (0, 1):
        rows = [r for r, i in enumerate(idx) if i % 2 == parity]
        out[rows] = ds.batch([idx[r] for r in rows], augment=False)["keypoints"].cpu()
    return out


# ---- the array functions --------------------------------------------------------------------------------------------------------------
def test_five_functions_from_numpy_host_and_device_inputs(stack_backend):
    from lightning_pose_amd import metrics as M
    from lightning_pose_amd.utils.pca import KeypointPCA

    dev = stack_backend
    pred, labels, sv, mv = case_inputs(41, 6, SV_COLUMNS, 2, 3, 3, seed=5)
    pred[7, 2, 0] = np.nan
    labels[3, 1] = np.nan
    rng = np.random.default_rng(2)
    flat = pred.reshape(41, 12)
    train = torch.from_numpy((flat[np.isfinite(flat).all(axis=1)] + rng.normal(size=(40, 12))).astype(np.float32))      # 40 complete poses
    pca_sv = KeypointPCA("pca_singleview", components_to_keep=0.9, columns_for_singleview_pca=SV_COLUMNS, data_arr=train)
    pca_mv = KeypointPCA("pca_multiview", components_to_keep=3, mirrored_column_matches=MV_MATCHES, data_arr=train)
    pca_sv(), pca_mv()
    spec = lambda p: dict(index=p.index_table(6), mean=p.parameters["mean"].numpy(), kept=p.parameters["kept_eigenvectors"].numpy())   # noqa: E731
    want, low = (restated(pred, labels, spec(pca_sv), spec(pca_mv), t) for t in (np.float64, np.float32))
    forms = {"numpy": lambda a: a, "float64": lambda a: a.astype(np.float64), "host": lambda a: torch.from_numpy(a), "device": lambda a: torch.from_numpy(a).to(dev)}
    got = {}
    for name, conv in forms.items():
        p, lab = conv(pred), conv(labels)
        got[name] = {"pixel_error": M.pixel_error(lab, p), "temporal_norm": M.temporal_norm(p),
                     "temporal_norm_flat": M.temporal_norm(p.reshape(41, 12)),
                     "pca_singleview": M.pca_singleview_reprojection_error(p, pca_sv), "pca_multiview": M.pca_multiview_reprojection_error(p, pca_mv)}
    for name, tables in got.items():
        for key, a in tables.items():
            assert isinstance(a, np.ndarray) and a.dtype == np.float64 and a.shape == (41, 6), (name, key)
            assert np.array_equal(_bits(a), _bits(got["numpy"][key])), (name, key)
            w, l32 = want[key.replace("_flat", "")], low[key.replace("_flat", "")]
            fin = ~np.isnan(w)
            assert np.array_equal(np.isnan(a), ~fin)
            assert np.abs(a - w)[fin].max() <= 4.0 * np.abs(l32.astype(np.float64) - w)[fin].max(), (name, key)
    assert np.isnan(got["numpy"]["pca_singleview"][7]).all() and np.isnan(got["numpy"]["pca_singleview"][:, [3, 5]]).all()
    with pytest.raises(AssertionError):
        M.pca_multiview_reprojection_error(pred, pca_sv)
    with pytest.raises(ValueError, match="expected a pca_singleview"):
        M.pca_singleview_reprojection_error(pred, pca_mv)
    with pytest.raises(ValueError, match="shapes"):
        M.pixel_error(labels[:5], pred)


def test_result_containers():
    from lightning_pose_amd.data.datatypes import ComputeMetricsSingleResult, MultiviewPredictionResult, PredictionResult
    from lightning_pose_amd.utils.predictions import make_dlc_pandas_index

    df = pd.DataFrame(np.arange(12.0).reshape(2, 6), columns=make_dlc_pandas_index(_cfg(), ["a", "b"]))
    err = pd.DataFrame([[1.0, 2.0], [3.0, np.nan]], columns=["a", "b"])
    err["set"] = ["train", "test"]
    empty = PredictionResult(predictions=df).to_dict()
    assert empty["keypoint_names"] == ["a", "b"] and empty["index"] == [0, 1] and empty["pixel_error"] is None and empty["temporal_norm"] is None
    np.testing.assert_array_equal(empty["x"], [[0.0, 3.0], [6.0, 9.0]])
    np.testing.assert_array_equal(empty["confidence"], [[2.0, 5.0], [8.0, 11.0]])
    full = PredictionResult(predictions=df, metrics=ComputeMetricsSingleResult(pixel_error_df=err)).to_dict()
    np.testing.assert_array_equal(full["pixel_error"], [[1.0, 2.0], [3.0, np.nan]])
    assert full["pca_singleview_error"] is None and full["pca_multiview_error"] is None
    both = MultiviewPredictionResult(predictions={"top": df, "side": df}, metrics={"top": ComputeMetricsSingleResult(temporal_norm_df=err[["a", "b"]])}).to_dict()
    assert sorted(both) == ["side", "top"] and both["side"]["temporal_norm"] is None and both["top"]["temporal_norm"].shape == (2, 2)


# ---- compute_metrics_single on files ----------------------------------------------------------------------------------------------------
def _write_preds(path, xy, index=None, set_column=None, names=NAMES):
    from lightning_pose_amd.utils.predictions import make_dlc_pandas_index

    t, k, _ = xy.shape
    arr = np.concatenate([xy.astype(np.float32).astype(np.float64), np.full((t, k, 1), 0.5)], axis=2).reshape(t, 3 * k)
    df = pd.DataFrame(arr, columns=make_dlc_pandas_index(_cfg(), names))
    if set_column is not None:
        df["set"] = set_column
    if index is not None:
        df.index = index
    df.to_csv(path)
    return arr.reshape(t, k, 3)[:, :, :2].astype(np.float32)


def _check_table(df, want, index, set_column=None, names=NAMES):
    assert list(df.columns) == names + ([] if set_column is None else ["set"]) and list(df.index) == list(index)
    values = df[names].to_numpy()
    assert values.dtype == np.float64 and np.array_equal(_bits(values), _bits(want))
    if set_column is not None:
        assert list(df["set"]) == list(set_column)


def test_compute_metrics_single_video_table(stack_backend, disk, tmp_path):
    from lightning_pose_amd import metrics as M

    dm = _data_module(disk, stack_backend)
    g = np.random.default_rng(4)
    xy = _write_preds(tmp_path / "clip.csv", g.uniform(0, 60, (20, K, 2)))
    res = M.compute_metrics_single(_cfg(), None, tmp_path / "clip.csv", data_module=None)
    assert res.pixel_error_df is None and res.pca_sv_df is None and res.pca_mv_df is None
    _check_table(res.temporal_norm_df, M.temporal_norm(xy), range(20))
    assert sorted(os.listdir(tmp_path)) == ["clip.csv", "clip_temporal_norm.csv"]
    # with a data module and the cfg entries: the PCA tables, fitted on pca_keypoints()
    res = M.compute_metrics_single(_cfg(), None, str(tmp_path / "clip.csv"), data_module=dm)
    assert sorted(os.listdir(tmp_path)) == ["clip.csv", "clip_pca_multiview_error.csv", "clip_pca_singleview_error.csv", "clip_temporal_norm.csv"]
    fitted = M._fit_pcas(_cfg(), dm)
    _check_table(res.pca_sv_df, M.pca_singleview_reprojection_error(xy, fitted["pca_singleview"]), range(20))
    _check_table(res.pca_mv_df, M.pca_multiview_reprojection_error(xy, fitted["pca_multiview"]), range(20))
    assert np.isnan(res.pca_sv_df[["hip", "tail"]].to_numpy()).all() and not np.isnan(res.pca_sv_df[["nose", "ear", "paw", "knee"]].to_numpy()).any()
    back = pd.read_csv(tmp_path / "clip_pca_singleview_error.csv", index_col=0)
    np.testing.assert_allclose(back.to_numpy(), res.pca_sv_df.to_numpy(), rtol=1e-12)
    # an empty selection switches a PCA metric off (reference metrics.py:226-239)
    res = M.compute_metrics_single(_cfg(sv=[], mv=None), None, tmp_path / "clip.csv", data_module=dm)
    assert res.pca_sv_df is None and res.pca_mv_df is None and res.temporal_norm_df is not None


@pytest.mark.parametrize("labels_csv", ["CollectedData.csv", "FirstRowNaN.csv"])      # a ``visible`` column / an all-NaN first row
def test_compute_metrics_single_labeled_table(stack_backend, disk, tmp_path, labels_csv):
    from lightning_pose_amd import metrics as M

    g = np.random.default_rng(6)
    sets = np.array(["train", "validation", "test"])[g.integers(0, 3, N)]
    xy = _write_preds(tmp_path / "predictions.csv", disk["xy"] + g.normal(scale=3.0, size=disk["xy"].shape), index=disk["names"], set_column=sets)
    labels = disk["xy"].copy()
    if labels_csv == "FirstRowNaN.csv":
        labels[0] = np.nan
    labels_file = os.path.join(disk["root"], labels_csv)
    assert (pd.read_csv(labels_file, header=[0, 1, 2], index_col=0).index.name is not None) == (labels_csv == "FirstRowNaN.csv")
    res = M.compute_metrics_single(_cfg(), labels_file, tmp_path / "predictions.csv")
    assert res.temporal_norm_df is None and res.pca_sv_df is None
    _check_table(res.pixel_error_df, M.pixel_error(labels.astype(np.float32), xy), disk["names"], sets)
    assert np.array_equal(np.isnan(res.pixel_error_df[NAMES].to_numpy()), np.isnan(labels[..., 0]) | np.isnan(xy[..., 0]))
    assert sorted(os.listdir(tmp_path)) == ["predictions.csv", "predictions_pixel_error.csv"]
    assert list(pd.read_csv(tmp_path / "predictions_pixel_error.csv", index_col=0).columns) == NAMES + ["set"]
    with pytest.raises(AssertionError):
        M.compute_metrics_single(_cfg(), None, tmp_path / "predictions.csv")
    _write_preds(tmp_path / "shifted.csv", xy.astype(np.float64), index=disk["names"][1:] + disk["names"][:1], set_column=sets)
    with pytest.raises(AssertionError):
        M.compute_metrics_single(_cfg(), labels_file, tmp_path / "shifted.csv")                  # the index-equality check


def test_compute_metrics_single_swallows_a_pca_that_cannot_be_fitted(stack_backend, disk, tmp_path):
    from lightning_pose_amd import metrics as M
    from lightning_pose_amd.utils.pca import KeypointPCA

    dm = _data_module(disk, stack_backend, train_frames=5)          # 5 samples < 12 observation dimensions
    assert len(dm.train_dataset.indices) == 5
    with pytest.raises(ValueError, match="cannot fit PCA"):
        KeypointPCA("pca_singleview", data_module=dm, columns_for_singleview_pca=list(range(K)))()
    _write_preds(tmp_path / "clip.csv", np.random.default_rng(8).uniform(0, 60, (9, K, 2)))
    res = M.compute_metrics_single(_cfg(sv=list(range(K)), mv=None), None, tmp_path / "clip.csv", data_module=dm)
    assert res.pca_sv_df is None and res.temporal_norm_df is not None and sorted(os.listdir(tmp_path)) == ["clip.csv", "clip_temporal_norm.csv"]


# ---- pca_keypoints and what is fitted from it ----------------------------------------------------------------------------------------
def test_pca_keypoints_decodes_no_image(stack_backend, disk, monkeypatch):
    from lightning_pose_amd.data.datasets import HeatmapDataset

    dev = stack_backend
    dm = _data_module(disk, dev)
    calls = []
    real = HeatmapDataset.load_images
    monkeypatch.setattr(HeatmapDataset, "load_images", lambda self, idx: calls.append(len(idx)) or real(self, idx))
    got = dm.pca_keypoints()
    assert calls == [], "pca_keypoints loaded images"
    train = list(dm.train_dataset.indices)
    assert 20 <= len(train) < N and tuple(got.shape) == (len(train), 2 * K) and got.dtype == torch.float32 and got.device.type == dev.type
    want = _unaugmented_batches(dm.dataset, train)
    assert len(calls) == 2 and sum(calls) == len(train)
    assert torch.equal(got.cpu().view(torch.int32), want.view(torch.int32))
    # model px: stored px scaled by the size of each example's own file; NaN where unlabeled
    sizes = np.array([SIZES[i % 2] for i in train], dtype=np.float64)
    scaled = disk["xy"][train] * np.stack([W / sizes[:, 1], H / sizes[:, 0]], axis=1)[:, None, :]
    np.testing.assert_allclose(got.cpu().numpy().reshape(len(train), K, 2), scaled, rtol=1e-6, equal_nan=True)
    assert np.isnan(got.cpu().numpy()).sum() == 2 * sum(i in train for i in (3, 7))


def test_pca_keypoints_of_a_multiview_dataset(stack_backend, disk, monkeypatch):
    from lightning_pose_amd.data.datamodules import BaseDataModule
    from lightning_pose_amd.data.datasets import HeatmapDataset, MultiviewHeatmapDataset

    ds = MultiviewHeatmapDataset(disk["root"], ["top.csv", "side.csv"], ["top", "side"], H, W, device=stack_backend)
    dm = BaseDataModule(ds, train_probability=0.5, val_probability=0.25, torch_seed=1)
    calls = []
    real = HeatmapDataset.load_images
    monkeypatch.setattr(HeatmapDataset, "load_images", lambda self, idx: calls.append(len(idx)) or real(self, idx))
    got = dm.pca_keypoints()
    assert calls == [] and tuple(got.shape) == (15, 2 * 2 * 3)
    want = _unaugmented_batches(ds, list(dm.train_dataset.indices))
    assert len(calls) == 4 and sum(calls) == 30 and torch.equal(got.cpu().view(torch.int32), want.view(torch.int32))


def test_pca_loss_and_loss_factories_fit_from_a_data_module(stack_backend, disk):
    from lightning_pose_amd.losses import PCALoss, get_loss_factories
    from lightning_pose_amd.utils.pca import KeypointPCA

    dev = stack_backend
    dm = _data_module(disk, dev)
    by_hand = KeypointPCA("pca_singleview", components_to_keep=0.99, columns_for_singleview_pca=SV_COLUMNS, data_arr=dm.pca_keypoints())
    by_hand()
    loss = PCALoss("pca_singleview", components_to_keep=0.99, columns_for_singleview_pca=SV_COLUMNS, data_module=dm, device=dev)
    for name in ("mean", "kept_eigenvectors", "epsilon"):
        assert torch.equal(loss.pca.parameters[name].cpu(), by_hand.parameters[name].cpu()), name
    kp = dm.pca_keypoints()[:4].nan_to_num(50.0)
    value, _ = loss(kp.to(dev), stage="train")
    assert torch.isfinite(value.cpu()).item()
    cfg = {"model": {"model_type": "heatmap", "losses_to_use": ["pca_singleview", "pca_multiview"]},
           "data": {"columns_for_singleview_pca": SV_COLUMNS, "mirrored_column_matches": MV_MATCHES},
           "losses": {"pca_singleview": {"log_weight": 5.0, "components_to_keep": 0.99, "device": dev},
                      "pca_multiview": {"log_weight": 5.0, "components_to_keep": 3, "device": dev}}}
    factories = get_loss_factories(cfg, dm)
    unsup = factories["unsupervised"].loss_instance_dict
    assert sorted(unsup) == ["pca_multiview", "pca_singleview"]
    assert torch.equal(unsup["pca_singleview"].pca.parameters["kept_eigenvectors"].cpu(), by_hand.parameters["kept_eigenvectors"].cpu())
    assert tuple(unsup["pca_multiview"].pca.parameters["kept_eigenvectors"].shape) == (3, 4)
