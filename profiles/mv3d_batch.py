"""The multi-view labeled batch with its 3-D augmentation at 8 samples x 4 views of 1024 x 1280 -> 256 x 256, 17 keypoints:

1. ``ops.mv3d_plan``, ``ops.mv3d_fill`` and ``ops.mv3d_finish`` - device time per launch (events around ``--launches`` launches after a warm-up),
   each against its bytes: the plan's inputs and outputs (it is latency, not traffic), the uint8 source read once for the fill, the touched
   source rows plus the fp32 output written once for the finish;
2. the whole ``MultiviewLabeledBatchProducer`` call on device-resident uint8 images (plan + 4 x (fill + finish) + targets), device time and host
   wall time per batch;
3. the supervised multi-view transformer step that batch feeds (ViT-S/16, both calibrated 3-D losses), for scale.

One JSON line each, appended to ``--out`` (default profiles/mv3d_batch.txt).  There is no parent-commit number (the path is new) and the
reference's own path cannot run in this environment (cv2, kornia and aniposelib are absent): nothing here is a speed-up claim.  Reads nothing
outside the tree.

    python profiles/mv3d_batch.py
    python profiles/mv3d_batch.py --skip-step
"""

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import _lp_bootstrap  # noqa: E402,F401
from lightning_pose_amd import ops  # noqa: E402
from lightning_pose_amd.data.producers import MultiviewLabeledBatchProducer  # noqa: E402
from tests import cameras_fp64 as O  # noqa: E402

B, V, K, HS, WS, HW = 8, 4, 17, 1024, 1280, 256
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def timed(fn, warmup, launches):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    wall = time.perf_counter()
    t0.record()
    for _ in range(launches):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / launches * 1e3, (time.perf_counter() - wall) / launches * 1e6


def inputs(dev):
    rig = O.make_rig(B, V, K, 5, seed=7)
    bbox = torch.tensor([0.0, 0.0, float(HS), float(WS)]).repeat(B, V)                   # the whole frames: stored px = frame px
    kp = rig["points_2d"].float()
    images = [torch.randint(0, 256, (B, HS, WS, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(v)).to(dev) for v in range(V)]
    cal = {n: rig[n].float().to(dev) for n in ("intrinsics", "extrinsics", "distortions")}
    return images, kp.to(dev), bbox.to(dev), cal


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mv3d_batch.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    images, kp, bbox, cal = inputs(dev)
    src_hw = torch.tensor([float(HS), float(WS)], device=dev).repeat(B, V, 1)
    draws = torch.from_numpy(np.random.default_rng(0).uniform([0.8, -1, -1, -1], [1.2, 1, 1, 1], size=(B, 4)).astype(np.float32)).to(dev)
    shape = {"samples": B, "views": V, "keypoints": K, "source": [HS, WS], "model": [HW, HW]}
    recs = []

    plan = lambda: ops.mv3d_plan(kp, src_hw, bbox, cal["intrinsics"], cal["extrinsics"], cal["distortions"], draws, HW, HW)  # noqa: E731
    us, _ = timed(plan, 20, a.launches)
    kp3d, kp2d, affine, status = plan()
    moved = 4 * (kp.numel() + src_hw.numel() + bbox.numel() + B * V * (9 + 12 + 12) + draws.numel() + kp3d.numel() + kp2d.numel() + affine.numel() + B)
    recs.append({"what": "ops.mv3d_plan", **shape, "launches": a.launches, "us_per_launch": round(us, 2), "moved_kb": round(moved / 1e3, 1),
                 "status": status.tolist()})

    us, _ = timed(lambda: ops.mv3d_fill(images[0], MEAN, STD), 20, a.launches)
    src_bytes = images[0].numel()
    recs.append({"what": "ops.mv3d_fill (one view)", **shape, "launches": a.launches, "us_per_launch": round(us, 2),
                 "source_mb": round(src_bytes / 1e6, 2), "source_read_once_gbs": round(src_bytes / us / 1e3, 1)})

    fill = ops.mv3d_fill(images[0], MEAN, STD)
    out = torch.empty(B, V, 3, HW, HW, device=dev)
    us, _ = timed(lambda: ops.mv3d_finish(images[0], affine, fill, MEAN, STD, 0, out), 20, a.launches)
    # an output row's 2 resize taps read 2 warped rows, each up to 2 source rows (4 under a rotation's slant, not counted): the touched rows
    touched = min(HS, 4 * HW) * WS * 3 * B
    written = B * 3 * HW * HW * 4
    recs.append({"what": "ops.mv3d_finish (one view)", **shape, "launches": a.launches, "us_per_launch": round(us, 2),
                 "touched_source_rows_mb": round(touched / 1e6, 2), "output_mb": round(written / 1e6, 2),
                 "touched_plus_written_gbs": round((touched + written) / us / 1e3, 1)})

    producer = MultiviewLabeledBatchProducer(HW, HW)
    names = [f"cam{v}" for v in range(V)]
    whole = lambda: producer(images, kp, names, bbox=bbox, **cal)  # noqa: E731
    us, wall = timed(whole, a.warmup, max(a.launches // 10, 5))
    recs.append({"what": "MultiviewLabeledBatchProducer, the whole batch (device-resident uint8 images)", **shape,
                 "device_us_per_batch": round(us, 1), "host_wall_us_per_batch": round(wall, 1)})

    if not a.skip_step:
        from lightning_pose_amd.losses import LossFactory
        from lightning_pose_amd.models import get_model_class

        factory = LossFactory({"heatmap_mse": {"log_weight": 0.0}, "supervised_pairwise_projections": {"log_weight": 0.5},
                               "supervised_reprojection_heatmap_mse": {"log_weight": 0.5, "original_image_height": HW, "original_image_width": HW,
                                                                       "downsampled_image_height": HW // 4, "downsampled_image_width": HW // 4}}, None)
        model = get_model_class("heatmap_multiview_transformer", False)(num_keypoints=K, num_views=V, loss_factory=factory, backbone="vits_dino",
                                                                        pretrained=False, torch_seed=0, device=dev)
        model.train()
        opt = model.configure_optimizers()["optimizer"]
        batch = whole()

        def one():
            opt.zero_grad()
            loss = model.training_step(batch, 0)["loss"]
            loss.backward()
            opt.step()

        us, _ = timed(one, a.warmup, a.steps)
        recs.append({"what": "supervised multi-view step on that batch (ViT-S/16, both 3-D losses)", **shape, "steps": a.steps,
                     "ms_per_step": round(us / 1e3, 3)})

    lines = [json.dumps(r) for r in recs]
    print("\n".join(lines))
    with open(a.out, "a") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
