"""Semi-supervised training step of the multi-view transformer tracker (ViT-S/16, V = 4 views of 256 px, K = 17, 8 labeled + 8 unlabeled
samples, bf16-mixed) against the single-view ``vits_dino`` tracker on the SAME (B, V, ...) batches through its 5-D branch - the same number
of view-images, no cross-view attention.  5 warm-up + 20 timed steps each, device events around the timed block; one JSON line per model
and a ratio, appended to ``--out`` (default profiles/mvt_step.txt).  Reads nothing outside the tree.

    python profiles/mvt_step.py                 # both models, timed
    python profiles/mvt_step.py --only mvt --steps 3 --warmup 2     # e.g. under rocprofv3 --kernel-trace --stats
"""

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import _lp_bootstrap  # noqa: E402,F401
from lightning_pose_amd import ops  # noqa: E402
from lightning_pose_amd.losses import LossFactory  # noqa: E402
from lightning_pose_amd.models import get_model_class  # noqa: E402

K, V, HW, BL, S = 17, 4, 256, 8, 8


def batches(dev):
    g = torch.Generator().manual_seed(0)
    kp = torch.rand(BL, V * K, 2, generator=g) * (HW - 16) + 8
    box = torch.tensor([[0.0, 0.0, float(HW), float(HW)] * V])
    labeled = {"images": torch.randn(BL, V, 3, HW, HW, generator=g).to(dev), "keypoints": kp.reshape(BL, -1).to(dev),
               "heatmaps": ops.generate_heatmaps(kp.to(dev), HW, HW, (HW // 4, HW // 4)), "bbox": box.repeat(BL, 1).to(dev),
               "num_views": torch.full((BL,), V), "idxs": torch.arange(BL)}
    tf = torch.tensor([[1.0, 0.05, 1.0], [-0.05, 1.0, 2.0]]).repeat(V, 1, 1)
    unlabeled = {"frames": torch.randn(S, V, 3, HW, HW, generator=g).to(dev), "transforms": tf.to(dev), "bbox": box.repeat(S, 1).to(dev),
                 "is_multiview": True}
    return {"labeled": labeled, "unlabeled": unlabeled}


def build(which, dev):
    sup = LossFactory({"heatmap_mse": {"log_weight": 0.0}}, None)
    unsup = LossFactory({"temporal": {"log_weight": 5.0, "epsilon": 5.0, "prob_threshold": 0.05}}, None)
    kw = dict(num_keypoints=K, loss_factory=sup, loss_factory_unsupervised=unsup, backbone="vits_dino", pretrained=False, torch_seed=0,
              device=dev)
    if which == "mvt":
        return get_model_class("heatmap_multiview_transformer", True)(num_views=V, **kw)
    return get_model_class("heatmap", True)(**kw)


def run(which, dev, warmup, steps):
    model, batch = build(which, dev), batches(dev)
    model.train()
    opt = model.configure_optimizers()["optimizer"]
    for g in opt.param_groups:
        g["lr"] = 1e-4          # the unfrozen backbone: every gradient and every optimiser range is live

    def step(i):
        opt.zero_grad()
        loss = model.training_step(batch, i)["loss"]
        loss.backward()
        opt.step()
        return loss

    for i in range(warmup):
        step(i)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for i in range(steps):
        loss = step(warmup + i)
    t1.record()
    torch.cuda.synchronize()
    ms = t0.elapsed_time(t1) / steps
    assert torch.isfinite(loss).item()
    return {"model": which, "views": V, "px": HW, "keypoints": K, "labeled": BL, "unlabeled": S, "warmup": warmup, "steps": steps,
            "ms_per_step": round(ms, 3), "view_images_per_s": round((BL + S) * V / ms * 1e3, 1), "loss": round(float(loss), 6)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["mvt", "single"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mvt_step.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    recs = [run(w, dev, a.warmup, a.steps) for w in ([a.only] if a.only else ["mvt", "single"])]
    lines = [json.dumps(r) for r in recs]
    if len(recs) == 2:
        lines.append(json.dumps({"mvt_over_single_view_images_per_s": round(recs[0]["view_images_per_s"] / recs[1]["view_images_per_s"], 4)}))
    print("\n".join(lines))
    with open(a.out, "a") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
