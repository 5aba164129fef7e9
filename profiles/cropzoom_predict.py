"""Crop-zoom prediction on the device: three measurements, one JSON line appended to ``--out`` (default profiles/cropzoom_predict.txt).

1. ``lp_frames_crop_resize`` against ``lp_frames_resize`` on the SAME work: full-frame boxes, 128 frames of 1024 x 1280 -> 256 x 256, normalised
   planes.  The two kernels alternate inside one process - A B A B ... windows of ``--reps`` launches after a warm-up of both - each window
   timed with device events.  The outputs are compared bit for bit first.  Expectation: the new kernel takes at most 1.03 x the other's time
   (the README records a +-2.5 % box-to-box spread); the record says whether it did.
2. ``lp_frames_crop_resize`` on realistic boxes: about 400 x 400, jittering from frame to frame, some over the frame's edge.  Algorithmic bytes
   = the in-frame part of every box (3 bytes per pixel) + the planes written, from the shapes; next to it a plain device-to-device copy that
   moves the same number of bytes (half read, half written), timed the same way in the same process.
3. The whole two-stage prediction: ``predict_video_cropzoom`` with two ResNet-50 ``HeatmapTracker``s (random weights, 256 x 256 inputs) on a
   decoded video in host memory (1024 frames: 4 GB, which ``resident_bytes`` keeps on the device between the passes), frames per second by a
   host clock around the call (it ends with the tables on the host), next to the sum of two plain ``predict_video`` passes over the same
   video (what two models cost without the crop: whole frames both times).

Needs the device; reads nothing outside the tree.

    python profiles/cropzoom_predict.py
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

MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


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


def kernel_pair(dev, frames, hs, ws, size, n_windows, reps) -> dict:
    g = torch.Generator().manual_seed(0)
    src = torch.randint(0, 256, (frames, hs, ws, 3), generator=g, dtype=torch.uint8).to(dev)
    full = torch.tensor([[0, 0, hs, ws]], dtype=torch.int32).repeat(frames, 1).to(dev)
    a = ops.frames_resize(src, size, size, "clamp", MEAN, STD)
    b = ops.frames_crop_resize(src, full, size, size, MEAN, STD, "clamp")
    same = bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))
    del a, b
    t = windows({"frames_resize": lambda: ops.frames_resize(src, size, size, "clamp", MEAN, STD),
                 "frames_crop_resize": lambda: ops.frames_crop_resize(src, full, size, size, MEAN, STD, "clamp")}, n_windows, reps)
    med = {k: statistics.median(v) for k, v in t.items()}
    ratio = med["frames_crop_resize"] / med["frames_resize"]
    rec = {"what": "full-frame boxes: lp_frames_crop_resize against lp_frames_resize, alternating windows", "frames": frames, "source": [hs, ws],
           "size": size, "bit_identical": same, "ms_per_launch_windows": t, "ms_per_launch_median": med, "ratio_crop_over_resize": round(ratio, 4),
           "within_1.03": bool(ratio <= 1.03)}

    # realistic boxes: ~400 x 400, a drifting centre with jitter
    rng = np.random.default_rng(1)
    cx = np.clip(ws / 2 + np.cumsum(rng.normal(0, 25, frames)), 100, ws - 100)
    cy = np.clip(hs / 2 + np.cumsum(rng.normal(0, 25, frames)), 100, hs - 100)
    side = 2 * rng.integers(180, 221, frames)
    boxes = np.column_stack([np.trunc(cx - side / 2), np.trunc(cy - side / 2), side, side]).astype(np.int32)
    x0, x1 = np.maximum(boxes[:, 0], 0), np.minimum(boxes[:, 0] + boxes[:, 3], ws)
    y0, y1 = np.maximum(boxes[:, 1], 0), np.minimum(boxes[:, 1] + boxes[:, 2], hs)
    roi_bytes = int((np.maximum(x1 - x0, 0) * np.maximum(y1 - y0, 0)).sum()) * 3
    out_bytes = frames * 3 * size * size * 4
    dbox = torch.from_numpy(boxes).to(dev)
    half = (roi_bytes + out_bytes) // 2
    c_src, c_dst = torch.empty(half, dtype=torch.uint8, device=dev), torch.empty(half, dtype=torch.uint8, device=dev)
    t2 = windows({"frames_crop_resize": lambda: ops.frames_crop_resize(src, dbox, size, size, MEAN, STD, "clamp"),
                  "copy": lambda: c_dst.copy_(c_src)}, n_windows, reps)
    med2 = {k: statistics.median(v) for k, v in t2.items()}
    gbs = {k: round((roi_bytes + out_bytes) / (v * 1e-3) / 1e9, 1) for k, v in med2.items()}
    rec["realistic_boxes"] = {"box_side_range": [int(side.min()), int(side.max())], "roi_mb": round(roi_bytes / 1e6, 2), "planes_mb": round(out_bytes / 1e6, 2),
                              "ms_per_launch_windows": t2, "ms_per_launch_median": med2, "algorithmic_gbs": gbs,
                              "rate_over_copy_rate": round(gbs["frames_crop_resize"] / gbs["copy"], 3)}
    return rec


def two_stage(dev, frames, hs, ws, size, seq) -> dict:
    from lightning_pose_amd.data.producers import FrameWindowSource, VideoFramePipeline
    from lightning_pose_amd.models import HeatmapTracker
    from lightning_pose_amd.utils.predictions import predict_video, predict_video_cropzoom

    rng = np.random.default_rng(2)
    block = rng.integers(0, 256, size=(min(frames, 64), hs, ws, 3), dtype=np.uint8)
    video = np.concatenate([block] * ((frames + len(block) - 1) // len(block)))[:frames]     # (a repeated block: the content does not matter to the time)
    names_d, names_p = [f"d{i}" for i in range(4)], [f"p{i}" for i in range(17)]
    cfg = lambda names: Cfg(data=Cfg(keypoint_names=names, image_resize_dims=Cfg(height=size, width=size)), model=Cfg(model_type="heatmap"))  # noqa: E731
    det = HeatmapTracker(num_keypoints=4, backbone="resnet50", pretrained=False, torch_seed=1, device=dev)
    pose = HeatmapTracker(num_keypoints=17, backbone="resnet50", pretrained=False, torch_seed=2, device=dev)
    detector_cfg = Cfg(anchor_keypoints=[], crop_height=400, crop_width=400)     # (random weights: a ratio box would be arbitrary)

    def cropzoom():
        return predict_video_cropzoom("clip.mp4", det, pose, video, detector_cfg, cfg_detector=cfg(names_d), cfg_pose=cfg(names_p),
                                      sequence_length=seq, smooth_window=5)

    def plain(model, names):
        pipe = VideoFramePipeline([size, size], imgaug="default")
        return predict_video("clip.mp4", model, (pipe(w) for w in FrameWindowSource(video, seq, device=dev)), cfg=cfg(names), frame_count=frames)

    def clock(fn, n=3):
        fn()  # warm-up: code objects, workspaces
        ts = []
        for _ in range(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(round(time.perf_counter() - t0, 4))
        return ts

    t_cz, t_d, t_p = clock(cropzoom), clock(lambda: plain(det, names_d)), clock(lambda: plain(pose, names_p))
    m_cz, m_two = statistics.median(t_cz), statistics.median(t_d) + statistics.median(t_p)
    return {"what": "predict_video_cropzoom (ResNet-50 detector + pose, fixed 400 x 400 boxes, window 5) against two plain predict_video passes",
            "frames": frames, "source": [hs, ws], "size": size, "sequence_length": seq, "seconds_cropzoom": t_cz, "seconds_plain_detector": t_d,
            "seconds_plain_pose": t_p, "frames_per_s_cropzoom": round(frames / m_cz, 1), "frames_per_s_two_plain_passes": round(frames / m_two, 1),
            "cropzoom_over_two_plain": round(m_cz / m_two, 3)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--source", type=int, nargs=2, default=[1024, 1280])
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--windows", type=int, default=6)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--video-frames", type=int, default=1024, help="length of the video of the third measurement")
    ap.add_argument("--sequence-length", type=int, default=32)
    ap.add_argument("--skip-two-stage", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cropzoom_predict.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("profiles/cropzoom_predict.py measures on the device; none here - nothing recorded", file=sys.stderr)
        return 1
    dev = torch.device("cuda:0")
    rec = {"kernel": kernel_pair(dev, a.frames, a.source[0], a.source[1], a.size, a.windows, a.reps)}
    torch.cuda.empty_cache()
    if not a.skip_two_stage:
        rec["two_stage"] = two_stage(dev, a.video_frames, a.source[0], a.source[1], a.size, a.sequence_length)
    line = json.dumps(rec)
    print(line)
    with open(a.out, "a") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
