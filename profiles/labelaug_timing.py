"""Device time to produce one labeled batch (64 images, 406 x 396 -> 384 x 384): (a) the un-augmented LabeledBatchProducer call, (b) the "dlc"
preset with its own probabilities, (c) "dlc" with every operator forced on.  Events around each of REPS calls after WARMUP calls, one
process; prints median / min / max in ms and the host time of one draw, and writes the JSON.  Launches per batch and the per-kernel split come from a
kernel trace of `--profile` (see profile()).

    timeout 600 python profiles/labelaug_timing.py [out.json]
"""

import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import _lp_bootstrap  # noqa: E402,F401
from lightning_pose_amd import _lib  # noqa: E402
from lightning_pose_amd.data import augmentations as A  # noqa: E402
from lightning_pose_amd.data.producers import LabeledBatchProducer  # noqa: E402

WARMUP, REPS, B, HS, WS, SIZE, K = 10, 50, 64, 406, 396, 384, 17


def timed(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms))}


def profile(which: str, b: int, n: int = 10) -> None:
    """exactly n batches of one case with a kept draw and nothing else, for a kernel trace:
        rocprofv3 --kernel-trace --stats -d out -o name -- python profiles/labelaug_timing.py --profile b 64
    calls / n in the stats = launches per batch (torch's fills included), total time / n = the per-kernel split"""
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    imgs = torch.from_numpy(rng.integers(0, 256, (b, HS, WS, 3), dtype=np.uint8)).to(dev)
    kp = torch.rand(b, 2 * K, device=dev) * 300
    prod = LabeledBatchProducer(SIZE, SIZE)
    spec = A.expand_imgaug_str_to_dict("dlc")
    if which == "c":
        spec = {k: {**v, "p": 1.0} for k, v in spec.items()}
    kept = A.imgaug_transform(spec, seed=0).draw(b, HS, WS) if which != "a" else None
    for _ in range(n):
        prod(imgs, kp, augment=kept)
    torch.cuda.synchronize()


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--profile":
        return profile(sys.argv[2], int(sys.argv[3]))
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    imgs = torch.from_numpy(rng.integers(0, 256, (B, HS, WS, 3), dtype=np.uint8)).to(dev)
    kp = torch.rand(B, 2 * K, device=dev) * 300
    prod = LabeledBatchProducer(SIZE, SIZE)
    spec = A.expand_imgaug_str_to_dict("dlc")
    dlc = A.imgaug_transform(spec, seed=0)
    forced = A.imgaug_transform({k: {**v, "p": 1.0} for k, v in spec.items()}, seed=0)
    out = {"shape": {"batch": B, "source": [HS, WS], "model": SIZE, "warmup": WARMUP, "reps": REPS},
           "a_plain": timed(lambda: prod(imgs, kp)),
           "b_dlc": timed(lambda: prod(imgs, kp, augment=dlc.draw(B, HS, WS))),          # host draw + table upload included: what a step pays
           "c_dlc_all_on": timed(lambda: prod(imgs, kp, augment=forced.draw(B, HS, WS)))}
    kept = dlc.draw(B, HS, WS)
    out["b_dlc_replayed_draw"] = timed(lambda: prod(imgs, kp, augment=kept))               # the same without the host draw
    t0 = time.perf_counter()
    for _ in range(REPS):
        dlc.draw(B, HS, WS)
    out["host_draw_ms"] = (time.perf_counter() - t0) / REPS * 1e3
    print(json.dumps(out, indent=1))
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
