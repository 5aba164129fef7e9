"""Geometry of the calibrated 3-D losses at B = 8 samples, V = 4 views, K = 17 keypoints: forward + backward, device events around the timed
block, warm-up first (measured values are appended to ``--out``, default profiles/cam3d_step.txt; one JSON line each).

  (a) ``fused``     ops.camera_chain (triangulate every pair, mean, reproject, distort, frame -> model px) + ops.pairwise_projections_loss,
                    and their backward: 2 launches forward, 1 backward (+ the scalar glue of autograd)
  (b) ``torch``     the same quantity by torch ops on the device in the reference's formulation (data/cameras.py:22-171): a Python loop over
                    camera pairs and samples, a host read of the valid mask and one small torch.linalg.svd per iteration, autograd backward
  (c) ``step``      the multi-view transformer training step of profiles/mvt_step.py (ViT-S/16, 4 x 256 px, 8 + 8 samples, bf16-mixed) with and
                    without the two calibrated losses

    python profiles/cam3d_step.py [--only geometry|step] [--iters 50] [--warmup 10]
"""

import argparse
import itertools
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
import _lp_bootstrap  # noqa: E402,F401
from lightning_pose_amd import ops  # noqa: E402
from lightning_pose_amd.losses import LossFactory  # noqa: E402
from lightning_pose_amd.models import get_model_class  # noqa: E402
from tests import cameras_fp64 as O  # noqa: E402  (the synthetic calibrated rig and the torch formulas)

B, V, K, HW = 8, 4, 17, 256


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters * 1e3   # us


def torch_reference_formulation(points, intr, extr, dist, bbox, targ):
    """project_camera_pairs_to_3d as the reference writes it (loops, torch.where on the host, one SVD per pair and sample), then the mean,
    the projection, the frame -> model map and the pairwise loss; returns the scalar that is differentiated"""
    x, y = O.undistort(points, intr, dist)
    und = torch.stack([x, y], -1)
    p3d = []
    for j1, j2 in itertools.combinations(range(V), 2):
        p1, p2 = und[:, j1], und[:, j2]
        valid = ~(torch.isnan(p1).any(-1) | torch.isnan(p2).any(-1))
        tri = torch.full((B, K, 3), float("nan"), device=points.device, dtype=points.dtype)
        for b in range(B):
            idx = torch.where(valid[b])[0]
            if len(idx) > 0:
                a1, a2, P1, P2 = p1[b][valid[b]], p2[b][valid[b]], extr[b, j1], extr[b, j2]
                A = torch.stack([a1[:, 0:1] * P1[2] - P1[0], a1[:, 1:2] * P1[2] - P1[1], a2[:, 0:1] * P2[2] - P2[0], a2[:, 1:2] * P2[2] - P2[1]], 1)
                h = torch.linalg.svd(A)[2][:, -1]
                tri[b, valid[b]] = h[:, :3] / h[:, 3:4]
        p3d.append(tri)
    p3d = torch.stack(p3d, 1)
    p2d = O.project(p3d.mean(1), intr, extr, dist, bbox, HW, HW)
    return O.pairwise_loss(targ, p3d) + p2d.sum() * 1e-3


def geometry(dev, warmup, iters):
    r = {k: v.float().to(dev) for k, v in O.make_rig(B, V, K, 5, seed=1).items()}
    pts = r["points_2d"].clone().requires_grad_(True)
    cam = (r["intrinsics"], r["extrinsics"], r["distortions"])

    def fused():
        pts.grad = None
        p3d, p2d = ops.camera_chain(pts, *cam, r["bbox"], HW, HW)
        (ops.pairwise_projections_loss(r["points_3d"], p3d) + p2d.sum() * 1e-3).backward()

    def reference():
        pts.grad = None
        torch_reference_formulation(pts, *cam, r["bbox"], r["points_3d"]).backward()

    fused()
    g_fused = pts.grad.clone()
    reference()
    g_ref = pts.grad.clone()
    rel = float((g_fused - g_ref).abs().max() / g_ref.abs().max())
    a, b = timed(fused, warmup, iters), timed(reference, max(2, warmup // 5), max(5, iters // 5))
    return [{"what": "geometry fwd+bwd", "B": B, "V": V, "K": K, "fused_us": round(a, 1), "torch_reference_formulation_us": round(b, 1),
             "torch_over_fused": round(b / a, 2), "grad_rel_diff": rel, "warmup": warmup, "iters": iters}]


def step(dev, warmup, iters):
    import mvt_step

    out = []
    rig = O.make_rig(mvt_step.BL, V, K, 5, seed=2)
    for with_3d in (False, True):
        p = {"heatmap_mse": {"log_weight": 0.0}}
        if with_3d:
            p["supervised_pairwise_projections"] = {"log_weight": 0.5}
            p["supervised_reprojection_heatmap_mse"] = {"log_weight": 0.5, "original_image_height": HW, "original_image_width": HW,
                                                        "downsampled_image_height": HW // 4, "downsampled_image_width": HW // 4}
        unsup = LossFactory({"temporal": {"log_weight": 5.0, "epsilon": 5.0, "prob_threshold": 0.05}}, None)
        model = get_model_class("heatmap_multiview_transformer", True)(num_views=V, num_keypoints=K, loss_factory=LossFactory(p, None),
                                                                       loss_factory_unsupervised=unsup, backbone="vits_dino", pretrained=False,
                                                                       torch_seed=0, device=dev)
        batch = mvt_step.batches(dev)
        batch["labeled"].update(keypoints_3d=rig["points_3d"].float().to(dev), intrinsic_matrix=rig["intrinsics"].float().to(dev),
                                extrinsic_matrix=rig["extrinsics"].float().to(dev), distortions=rig["distortions"].float().to(dev),
                                bbox=rig["bbox"].float().to(dev))
        model.train()
        opt = model.configure_optimizers()["optimizer"]
        for g in opt.param_groups:
            g["lr"] = 1e-4
        n = [0]

        def one():
            opt.zero_grad()
            loss = model.training_step(batch, n[0])["loss"]
            loss.backward()
            opt.step()
            n[0] += 1
            return loss

        us = timed(one, warmup, iters)
        out.append({"what": "mvt step", "calibrated_losses": with_3d, "ms_per_step": round(us / 1e3, 3), "warmup": warmup, "iters": iters,
                    "loss_finite": bool(torch.isfinite(one()).item())})
    out.append({"what": "mvt step", "with_over_without": round(out[1]["ms_per_step"] / out[0]["ms_per_step"], 4)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["geometry", "step"])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cam3d_step.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    recs = []
    if a.only in (None, "geometry"):
        recs += geometry(dev, a.warmup, a.iters)
    if a.only in (None, "step"):
        recs += step(dev, max(3, a.warmup // 2), max(10, a.iters // 3))
    lines = [json.dumps(r) for r in recs]
    print("\n".join(lines))
    with open(a.out, "a") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
