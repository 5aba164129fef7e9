"""Where every executor puts its parameters in the flat buffers: the cases of tests/test_engine_layout.py and the description the test
holds against engine_layout.json.  Constructing an engine launches no kernel, so this runs anywhere the kernel library loads (the
emulated build included).  Rewrite the JSON - only when a layout change is intended - with
    python tests/golden/engine_layout.py"""

import json
import os

SMALL_VIT = dict(hidden=128, depth=2, heads=2, mlp=256, patch=16, pretrain_grid=3)


def build_cases(dev) -> dict:
    from lightning_pose_amd.engine import Engine, HeadEngine
    from lightning_pose_amd.vit_engine import ViTEngine

    return {
        "resnet": Engine(17, 2, dev),
        "vit": ViTEngine(5, 2, dev, **SMALL_VIT),
        "vit_views2": ViTEngine(5, 2, dev, **SMALL_VIT, num_views=2),
        "vit_dinov2": ViTEngine(5, 2, dev, **SMALL_VIT, arch="dinov2"),
        "head": HeadEngine(512, 32, 5, 2, device=dev),
        "head_options": HeadEngine(512, 32, 5, 2, deconv_out_channels=32, final_softmax=False, device=dev),
    }


def describe(eng) -> dict:
    plan = eng.plan
    bufs = {eng.P.untyped_storage().data_ptr(): "P", eng.R.untyped_storage().data_ptr(): "R"}
    sd = {k: [bufs.get(v.untyped_storage().data_ptr(), "own"), v.storage_offset(), list(v.shape), list(v.stride())]
          for k, v in eng.state_dict().items()}
    layers = list(plan.convs) + (plan.linears() if hasattr(plan, "linears") else [])
    return {"n_total": plan.n_total, "n_wd": plan.n_wd, "n_running": plan.n_running,
            "group_ranges": {k: list(v) for k, v in plan.group_ranges().items()},
            "state_dict": sd, "wd_off": {l.name: l.wd_off for l in layers}}


if __name__ == "__main__":
    import sys

    import torch

    HERE = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    import _lp_bootstrap  # noqa: F401
    from lightning_pose_amd import _lib, ops
    from tests.hipemu import emu

    _lib._lib = emu.emu_lib()
    ops.require_device_type = lambda d: None
    out = {name: describe(eng) for name, eng in build_cases(torch.device("cpu")).items()}
    with open(os.path.join(HERE, "engine_layout.json"), "w") as f:
        json.dump(out, f, indent=0)   # (key order kept: it is the order of state_dict())
        f.write("\n")
