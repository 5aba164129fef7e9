"""Patch masking at the multi-view step's shapes (ViT-S/16, 8 samples x 4 views x 256 px: 32 images of 256 patches, 128 of them masked):

1. ``ops.patch_mask`` - device time per launch (events around ``--launches`` launches after a warm-up) against the bytes it moves;
2. the reference's verbatim ``PatchMasker`` (oracle/ref_loader.py) on the same device tensor - HOST wall time per call, ending in a device
   synchronise: its per-patch loop waits for the device 4096 times a call, which is what a training loop would feel;
3. the supervised multi-view step (the callback masks a batch with a top-level "images" entry) with and without ``PatchMasking``.

One JSON line each, appended to ``--out`` (default profiles/patch_mask_step.txt).  Exits non-zero unless (1) is below (2) - the only
pass condition; everything else is recorded.  Reads nothing outside the tree.

    python profiles/patch_mask_step.py
    python profiles/patch_mask_step.py --skip-reference --skip-step     # e.g. under rocprofv3 --kernel-trace --stats
"""

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import _lp_bootstrap  # noqa: E402,F401
from lightning_pose_amd import ops  # noqa: E402
from lightning_pose_amd.callbacks import PatchMasking  # noqa: E402
from lightning_pose_amd.losses import LossFactory  # noqa: E402
from lightning_pose_amd.models import get_model_class  # noqa: E402

K, V, HW, BL, COUNT = 17, 4, 256, 8, 128
ALWAYS_HALF = {"init_step": 0, "final_step": 1, "init_ratio": 0.5, "final_ratio": 0.5}


def kernel(images, warmup, launches):
    for i in range(warmup):
        ops.patch_mask(images, (0, i), COUNT)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for i in range(launches):
        ops.patch_mask(images, (0, warmup + i), COUNT)
    t1.record()
    torch.cuda.synchronize()
    us = t0.elapsed_time(t1) / launches * 1e3
    n = (HW // 16) ** 2
    batch = images.numel() * 4
    moved = batch + batch * (n - COUNT) // n          # every pixel written, the kept ones read
    return {"what": "ops.patch_mask", "images": list(images.shape), "count": COUNT, "launches": launches, "us_per_launch": round(us, 2),
            "batch_mb": round(batch / 1e6, 2), "nominal_read_plus_write_gbs": round(2 * batch / us / 1e3, 1),
            "moved_mb": round(moved / 1e6, 2), "moved_gbs": round(moved / us / 1e3, 1)}


def reference(images, calls):
    import transformers  # noqa: F401  (before the loader's stand-ins)
    from oracle import ref_loader

    masker = ref_loader.load("callbacks").PatchMasker(patch_mask_config=dict(ALWAYS_HALF), patch_seed=0)
    masked, mask = masker.apply_patch_masking(images, training_step=1)    # warm-up
    assert int((mask == 0).sum()) == BL * V * COUNT
    torch.cuda.synchronize()
    t = time.perf_counter()
    for i in range(calls):
        masker.apply_patch_masking(images, training_step=2 + i)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t) / calls * 1e3
    return {"what": "reference PatchMasker (verbatim), host wall time", "calls": calls, "ms_per_call": round(ms, 2)}


def step(images, with_callback, warmup, steps):
    dev = images.device
    g = torch.Generator().manual_seed(0)
    kp = torch.rand(BL, V * K, 2, generator=g) * (HW - 16) + 8
    labeled = {"images": images, "keypoints": kp.reshape(BL, -1).to(dev), "heatmaps": ops.generate_heatmaps(kp.to(dev), HW, HW, (HW // 4, HW // 4)),
               "bbox": torch.tensor([[0.0, 0.0, float(HW), float(HW)] * V]).repeat(BL, 1).to(dev), "num_views": torch.full((BL,), V),
               "idxs": torch.arange(BL)}
    model = get_model_class("heatmap_multiview_transformer", False)(
        num_keypoints=K, num_views=V, loss_factory=LossFactory({"heatmap_mse": {"log_weight": 0.0}}, None), backbone="vits_dino", pretrained=False,
        torch_seed=0, device=dev)
    model.train()
    opt = model.configure_optimizers()["optimizer"]
    for group in opt.param_groups:
        group["lr"] = 1e-4
    callback = PatchMasking(dict(ALWAYS_HALF), patch_seed=0)

    class Steps:   # what the callback reads of a trainer
        global_step = 0

    def one(i):
        batch = dict(labeled)
        if with_callback:
            Steps.global_step = i
            callback.on_train_batch_start(Steps, model, batch, i)
        opt.zero_grad()
        loss = model.training_step(batch, i)["loss"]
        loss.backward()
        opt.step()
        return loss

    for i in range(warmup):
        one(i)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for i in range(steps):
        loss = one(warmup + i)
    t1.record()
    torch.cuda.synchronize()
    assert torch.isfinite(loss).item()
    return {"what": "supervised multi-view step", "patch_masking": with_callback, "views": V, "px": HW, "samples": BL, "warmup": warmup, "steps": steps,
            "ms_per_step": round(t0.elapsed_time(t1) / steps, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=2000)
    ap.add_argument("--reference-calls", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--skip-reference", action="store_true")
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "patch_mask_step.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    images = torch.randn(BL, V, 3, HW, HW, generator=torch.Generator().manual_seed(0)).to(dev)
    recs = [kernel(images, 20, a.launches)]
    if not a.skip_reference:
        recs.append(reference(images, a.reference_calls))
    if not a.skip_step:
        recs += [step(images, False, a.warmup, a.steps), step(images, True, a.warmup, a.steps), step(images, False, a.warmup, a.steps),
                 step(images, True, a.warmup, a.steps)]
    lines = [json.dumps(r) for r in recs]
    print("\n".join(lines))
    with open(a.out, "a") as fh:
        fh.write("\n".join(lines) + "\n")
    if not a.skip_reference:
        assert recs[0]["us_per_launch"] < recs[1]["ms_per_call"] * 1e3, "the launch is not faster than the reference's PatchMasker"


if __name__ == "__main__":
    main()
