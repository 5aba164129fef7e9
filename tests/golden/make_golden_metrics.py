"""Generate tests/golden/metrics.npz: inputs, fitted PCA parameters and outputs of the reference's OWN metric functions (its metrics.py:
``pixel_error``, ``temporal_norm``, ``pca_singleview_reprojection_error``, ``pca_multiview_reprojection_error``) with its own
``KeypointPCA`` fit (utils/pca.py, driven by ``oracle.ref_loader.fit_keypoint_pca``).  Build container only (needs the reference tree):

    python tests/golden/make_golden_metrics.py

The file holds arrays only, a few KB.  Coordinates are frame scale (0 - 1300 px) with residuals of a few px off a low-dimensional pose model:
the scale at which the reference's add-the-mean-back reprojection loses digits.  One prediction coordinate and two labels are NaN, so the
recorded outputs also pin the reference's NaN propagation (a whole frame in the single-view table, one matched keypoint's views in the
multi-view table)."""

from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import ref_loader  # noqa: E402

T, K, N_TRAIN, LATENT = 37, 8, 80, 3
SV_COLUMNS = [0, 1, 2, 4, 6]
MV_MATCHES = [[0, 1, 2], [4, 5, 6]]      # two views, three matched keypoints; keypoints 3 and 7 belong to no sample
NAN_PRED = (11, 1, 0)                    # frame 11, keypoint 1 (selected single-view, matched keypoint 1 of view 0), x


def poses(rng, n, base, mixing):
    """n poses of K keypoints: a base pose + a LATENT-dimensional linear pose model + 2 px of noise, float32"""
    z = rng.normal(size=(n, LATENT))
    return (base + z @ mixing + rng.normal(scale=2.0, size=(n, 2 * K))).astype(np.float32)


def main() -> None:
    rng = np.random.default_rng(20240607)
    base = rng.uniform(100.0, 1200.0, size=2 * K)
    mixing = rng.normal(scale=40.0, size=(LATENT, 2 * K))
    train = poses(rng, N_TRAIN, base, mixing)
    pred = poses(rng, T, base, mixing).reshape(T, K, 2)
    labels = (pred + rng.normal(scale=30.0, size=pred.shape)).astype(np.float32)
    pred[NAN_PRED] = np.nan
    labels[3, 2, 1] = np.nan
    labels[20, 5, :] = np.nan

    M = ref_loader.load("metrics")
    sv = ref_loader.fit_keypoint_pca("pca_singleview", torch.from_numpy(train), components_to_keep=0.99, columns_for_singleview_pca=SV_COLUMNS)
    mv = ref_loader.fit_keypoint_pca("pca_multiview", torch.from_numpy(train), components_to_keep=3, mirrored_column_matches=MV_MATCHES)
    out = {
        "pred": pred, "labels": labels, "train": train,
        "sv_columns": np.asarray(SV_COLUMNS, np.int32), "mv_matches": np.asarray(MV_MATCHES, np.int32),
        "sv_mean": sv.parameters["mean"].numpy(), "sv_kept": sv.parameters["kept_eigenvectors"].numpy(),
        "mv_mean": mv.parameters["mean"].numpy(), "mv_kept": mv.parameters["kept_eigenvectors"].numpy(),
        "ref_pixel_error": np.asarray(M.pixel_error(labels, pred), np.float64),
        "ref_temporal_norm": np.asarray(M.temporal_norm(pred), np.float64),
        "ref_pca_singleview": np.asarray(M.pca_singleview_reprojection_error(pred, sv), np.float64),
        "ref_pca_multiview": np.asarray(M.pca_multiview_reprojection_error(pred, mv), np.float64),
    }
    path = os.path.join(HERE, "metrics.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes; kept components: singleview {out['sv_kept'].shape}, multiview {out['mv_kept'].shape}")
    for name in ("ref_pixel_error", "ref_temporal_norm", "ref_pca_singleview", "ref_pca_multiview"):
        print(f"  {name}: shape {out[name].shape}, NaN {int(np.isnan(out[name]).sum())}, max {np.nanmax(out[name]):.3f}")


if __name__ == "__main__":
    main()
