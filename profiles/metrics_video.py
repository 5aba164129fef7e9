"""Prediction metrics on the device at the size of an hour of 100 Hz video: T = 360 000 rows, K = 17 keypoints, both PCA specs.  One JSON line
appended to ``--out`` (default profiles/metrics_video.txt).

1. ``lp_kp_metrics`` alone, device events around alternating windows of launches after a warm-up: the video set (temporal norm + single-view
   PCA over 13 keypoints, 8 components + multi-view PCA, 2 views x 8 matched keypoints, 3 components) and all four tables (+ pixel error
   against labels).  Algorithmic bytes from the shapes: predictions (and labels) read once, every requested table written once.  Next to
   it, in the same process and timed the same way, a plain device-to-device copy that moves the same number of bytes (half read, half
   written).
2. ``predict_video`` on a stub tracker whose predictions are already on the device (the time of the tracker itself is not the question), with
   and without ``compute_metrics``, no files: a host clock around calls that end with the tables on the host.

No parent-commit number exists for this path and the reference's own function does not run on the device: no speed-up is claimed.
Needs the device; reads nothing outside the tree.

    python profiles/metrics_video.py
"""

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import _lp_bootstrap  # noqa: E402,F401
from lightning_pose_amd import ops  # noqa: E402

SV_COLUMNS = list(range(13))
MV_MATCHES = [list(range(0, 8)), list(range(8, 16))]


class Cfg(dict):
    __getattr__ = dict.get


def windows(fns: dict, n_windows: int, reps: int) -> dict:
    """alternating windows of ``reps`` calls, device events around each window -> ms per call, per window"""
    out = {k: [] for k in fns}
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for _ in range(n_windows):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            b.synchronize()
            out[name].append(round(a.elapsed_time(b) / reps, 4))
    return out


def inputs(t: int, k: int, dev):
    """frame-scale poses off a 3-dimensional pose model + 2 px of noise, and PCA specs fitted on 2000 of them (numpy SVD)"""
    rng = np.random.default_rng(0)
    base, mixing = rng.uniform(100.0, 1200.0, 2 * k), rng.normal(scale=40.0, size=(3, 2 * k))
    draw = lambda n: (base + rng.normal(size=(n, 3)) @ mixing + rng.normal(scale=2.0, size=(n, 2 * k))).astype(np.float32)   # noqa: E731
    train, pred = draw(2000).reshape(-1, k, 2), draw(t)
    labels = pred + rng.normal(scale=5.0, size=pred.shape).astype(np.float32)

    def spec(index, ncomp):
        index = np.asarray(index, dtype=np.int32)
        samples = np.concatenate([train[:, row].reshape(len(train), -1) for row in index]).astype(np.float64)
        mean = samples.mean(axis=0)
        vt = np.linalg.svd(samples - mean, full_matrices=False)[2]
        return ops.PcaMetricSpec(index, torch.from_numpy(mean.astype(np.float32)), torch.from_numpy(vt[:ncomp].astype(np.float32)), dev)

    return torch.from_numpy(pred).to(dev), torch.from_numpy(labels).to(dev), spec([SV_COLUMNS], 8), spec(np.asarray(MV_MATCHES).T, 3)


def kernel(dev, t, k, n_windows, reps) -> dict:
    pred, labels, sv, mv = inputs(t, k, dev)
    sets = {"video (temporal + both PCA)": (None, 3), "all four tables": (labels, 4)}
    rec = {"what": "lp_kp_metrics, one launch per call, against a device copy of the same bytes; alternating windows", "T": t, "K": k,
           "singleview": {"points": sv.points, "ncomp": sv.ncomp}, "multiview": {"rows": mv.rows, "points": mv.points, "ncomp": mv.ncomp}, "sets": {}}
    for name, (lab, n_tables) in sets.items():
        nbytes = t * k * 2 * 4 * (1 if lab is None else 2) + n_tables * t * k * 4
        c_src, c_dst = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev), torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
        ts = windows({"lp_kp_metrics": lambda: ops.keypoint_metrics(pred, lab, sv, mv), "copy": lambda: c_dst.copy_(c_src)}, n_windows, reps)
        med = {n: statistics.median(v) for n, v in ts.items()}
        gbs = {n: round(nbytes / (v * 1e-3) / 1e9, 1) for n, v in med.items()}
        rec["sets"][name] = {"algorithmic_mb": round(nbytes / 1e6, 2), "ms_per_launch_windows": ts, "ms_per_launch_median": med,
                             "algorithmic_gbs": gbs, "rate_over_copy_rate": round(gbs["lp_kp_metrics"] / gbs["copy"], 3)}
        del c_src, c_dst
    a, b = ops.keypoint_metrics(pred, labels, sv, mv), ops.keypoint_metrics(pred, labels, sv, mv)
    rec["two_runs_bit_identical"] = all(bool(torch.equal(a[n].view(torch.int32), b[n].view(torch.int32))) for n in a)
    return rec


class StubTracker(torch.nn.Module):
    def __init__(self, dev):
        super().__init__()
        self.anchor = torch.nn.Parameter(torch.zeros(1, device=dev))

    def predict_step(self, batch, batch_idx, return_heatmaps=False):
        return batch["keypoints_pred"], batch["confidences"]


class StubDataModule:
    """what the PCA fits ask of a data module: a single-view ``dataset`` and ``pca_keypoints()``"""

    def __init__(self, train):
        self.dataset, self._train = object(), train

    def pca_keypoints(self):
        return self._train


def end_to_end(dev, t, k, seq) -> dict:
    from lightning_pose_amd.utils.predictions import predict_video

    pred = inputs(t, k, dev)[0]
    conf = torch.full((t, k), 0.9, device=dev)
    loader = [{"keypoints_pred": pred[lo:lo + seq], "confidences": conf[lo:lo + seq]} for lo in range(0, t, seq)]
    cfg = Cfg(data=Cfg(keypoint_names=[f"p{i}" for i in range(k)], columns_for_singleview_pca=SV_COLUMNS, mirrored_column_matches=MV_MATCHES),
              model=Cfg(model_type="heatmap"), losses=Cfg(pca_singleview=Cfg(components_to_keep=8)))
    dm = StubDataModule(pred[:2000].cpu())
    tracker = StubTracker(dev)

    def clock(fn, n=3):
        fn()
        ts = []
        for _ in range(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(round(time.perf_counter() - t0, 4))
        return ts

    plain = clock(lambda: predict_video("clip.mp4", tracker, loader, cfg=cfg, frame_count=t))
    temporal = clock(lambda: predict_video("clip.mp4", tracker, loader, cfg=cfg, frame_count=t, compute_metrics=True))
    with_pca = clock(lambda: predict_video("clip.mp4", tracker, loader, cfg=cfg, frame_count=t, compute_metrics=True, data_module=dm))
    return {"what": "predict_video on a stub tracker (device-resident predictions), no files: host clock, tables on the host at the end; the PCA "
                    "variant includes both fits (host, float64) on 2000 training poses", "T": t, "K": k, "sequence_length": seq,
            "seconds_plain": plain, "seconds_compute_metrics_temporal": temporal, "seconds_compute_metrics_temporal_and_pca": with_pca}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=360000)
    ap.add_argument("--keypoints", type=int, default=17)
    ap.add_argument("--windows", type=int, default=6)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sequence-length", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metrics_video.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("profiles/metrics_video.py measures on the device; none here - nothing recorded", file=sys.stderr)
        return 1
    dev = torch.device("cuda:0")
    rec = {"kernel": kernel(dev, a.rows, a.keypoints, a.windows, a.reps), "predict_video": end_to_end(dev, a.rows, a.keypoints, a.sequence_length)}
    line = json.dumps(rec)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
