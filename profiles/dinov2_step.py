"""The cost of DINOv2's LayerScale in a training step: "vits_dinov2" against "vits_dino" at the shape of config C4 (ViT-S/16, 192 frames of
384 x 384 per step, K = 17, bf16-mixed), supervised heatmap_mse step with the backbone unfrozen (forward, backward, FusedAdam) so that every
kernel the two differ in runs.  The two models alternate inside ONE process - A B A B ... windows of ``--steps`` steps after a warm-up of both -
and each window is timed with device events; the record carries every window, the medians and their ratio.

What differs: the four LayerNorm walks per layer become lp_layernorm_ls_* (DESIGN.md 4.3e); the backward ones read one more bf16 (M, D) tensor
each (the unscaled branch output) - 2 reads per layer, and the tape holds those two tensors per layer.  The position table is 37 x 37 instead
of 14 x 14 (interpolated to 24 x 24 either way).  ``est_added_read_gb`` / ``est_added_ms`` are that traffic from the shapes, at the
--ln-gbs rate (what the LayerNorm walks reach, profiles/r06_final_vit_kernel_stats.txt), next to the measured difference.

One JSON line appended to ``--out`` (default profiles/dinov2_step.txt).  Needs the device; reads nothing outside the tree.

    python profiles/dinov2_step.py
"""

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import _lp_bootstrap  # noqa: E402,F401
from lightning_pose_amd import ops  # noqa: E402
from lightning_pose_amd.losses import LossFactory  # noqa: E402
from lightning_pose_amd.models import get_model_class  # noqa: E402

K = 17


def make(backbone, dev, frames, px):
    g = torch.Generator().manual_seed(0)
    kp = torch.rand(frames, K, 2, generator=g) * (px - 16) + 8
    batch = {"images": torch.randn(frames, 3, px, px, generator=g).to(dev), "keypoints": kp.reshape(frames, -1).to(dev),
             "heatmaps": ops.generate_heatmaps(kp.to(dev), px, px, (px // 4, px // 4)),
             "bbox": torch.tensor([[0.0, 0.0, float(px), float(px)]]).repeat(frames, 1).to(dev), "idxs": torch.arange(frames)}
    model = get_model_class("heatmap", False)(num_keypoints=K, loss_factory=LossFactory({"heatmap_mse": {"log_weight": 0.0}}, None),
                                              backbone=backbone, pretrained=False, torch_seed=0, device=dev)
    model.train()
    opt = model.configure_optimizers()["optimizer"]
    for group in opt.param_groups:   # the backbone trains: its gradients, LayerScale's among them, are computed and applied
        group["lr"] = 1e-4

    def one(i):
        opt.zero_grad()
        loss = model.training_step(batch, i)["loss"]
        loss.backward()
        opt.step()
        return loss

    return one


def window(one, steps, i0):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for i in range(steps):
        loss = one(i0 + i)
    t1.record()
    torch.cuda.synchronize()
    assert torch.isfinite(loss).item()
    return t0.elapsed_time(t1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=192)
    ap.add_argument("--px", type=int, default=384)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--windows", type=int, default=4)
    ap.add_argument("--ln-gbs", type=float, default=4000.0, help="bytes/s the LayerNorm walks reach, for the estimate")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dinov2_step.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("profiles/dinov2_step.py measures on the device: none found")
    dev = torch.device("cuda:0")
    names = ("vits_dino", "vits_dinov2")
    steps = {n: make(n, dev, a.frames, a.px) for n in names}
    for n in names:
        for i in range(a.warmup):
            steps[n](i)
    torch.cuda.synchronize()
    ms = {n: [] for n in names}
    for w in range(a.windows):
        for n in names:
            ms[n].append(round(window(steps[n], a.steps, a.warmup + w * a.steps), 3))
    med = {n: statistics.median(ms[n]) for n in names}
    depth, D = 12, 384
    M = a.frames * ((a.px // 16) ** 2 + 1)
    added = 2 * depth * M * D * 2          # two more bf16 (M, D) reads per layer in the backward pass
    rec = {"what": "training step, vits_dinov2 against vits_dino, alternating windows in one process", "frames": a.frames, "px": a.px, "K": K,
           "precision": "bf16-mixed", "warmup": a.warmup, "steps_per_window": a.steps, "ms_per_step_windows": ms,
           "ms_per_step_median": {n: round(med[n], 3) for n in names}, "ratio_dinov2_over_dino": round(med[names[1]] / med[names[0]], 4),
           "measured_added_ms": round(med[names[1]] - med[names[0]], 3), "est_added_read_gb": round(added / 1e9, 3),
           "est_added_ms": round(added / (a.ln_gbs * 1e9) * 1e3, 3), "est_rate_gbs": a.ln_gbs}
    line = json.dumps(rec)
    print(line)
    with open(a.out, "a") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
