"""Bit identity of the executors across a host-side refactor: every engine class, through its public constructor and methods only, on
seeded parameters and inputs; one line per result with the SHA-256 of its bytes.  Run it on two trees (same kernel library: LP_HIP_LIB)
and diff the outputs.  On the device it uses cuda:0; without one, the CPU with the emulated kernel library (as tests/conftest.py's
``stack_backend`` does).      python profiles/engine_identity.py > out.txt

A result that the device accumulates with fp32 atomics in arrival order (LayerNorm / bias gradients inside ``G``) can differ between two
runs of the SAME tree: compare two runs of one tree first, and read a line that differs there as no evidence either way.  The emulated
build has the same property with several worker threads; with HIPEMU_THREADS=1 it has one arrival order and every line repeats."""

import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import _lp_bootstrap  # noqa: E402,F401
from lightning_pose_amd import _lib, ops  # noqa: E402

SMALL = dict(hidden=128, depth=2, heads=2, mlp=256, patch=16, pretrain_grid=3)   # (the widths of tests/test_engine_layout.py)


def device() -> torch.device:
    if torch.cuda.is_available():
        return torch.device("cuda:0")
    from tests.hipemu import emu

    _lib._lib = emu.emu_lib()
    ops.require_device = lambda *a: None
    ops.require_device_type = lambda d: None
    ops._stream = lambda: None
    return torch.device("cpu")


def sha(t: torch.Tensor) -> str:
    t = t.detach().to("cpu").contiguous()
    return hashlib.sha256(t.view(torch.uint8).numpy().tobytes()).hexdigest()[:32] + f" {tuple(t.shape)}"


def seed_parameters(eng, seed: int) -> None:
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, v in eng.state_dict().items():
        r = torch.randn(v.shape, generator=g)
        if k.endswith("num_batches_tracked"):
            sd[k] = torch.tensor(3)
        elif k.endswith("running_var"):
            sd[k] = r.abs() + 0.5
        elif k.endswith("running_mean"):
            sd[k] = 0.1 * r
        elif k.endswith("lambda1") or (v.dim() == 1 and k.endswith("weight")):   # LayerScale, BatchNorm / LayerNorm scales
            sd[k] = 1.0 + 0.1 * r
        else:
            sd[k] = 0.05 * r
    eng.load_state_dict(sd)


def images(dev, seed: int, *shape) -> torch.Tensor:
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(dev)


def weight_gradients(eng) -> torch.Tensor:
    """G under every matrix-shaped state_dict entry but the token / position / view embeddings: the weight gradients, which no kernel
    accumulates in arrival order - the part of G that repeats bit for bit where the whole of it does not"""
    p0 = eng.P.untyped_storage().data_ptr()
    skip = ("cls_token", "mask_token", "position_embeddings", "view_embeddings")
    return torch.cat([eng.G.as_strided(v.shape, v.stride(), v.storage_offset()).reshape(-1) for k, v in eng.state_dict().items()
                      if v.dim() >= 2 and v.untyped_storage().data_ptr() == p0 and not k.endswith(skip)])


def report(name: str, eng, heat, tape=None, dfeat=None) -> None:
    print(f"{name} heat {sha(heat)}")
    print(f"{name} G {sha(eng.G)}")
    print(f"{name} G.weights {sha(weight_gradients(eng))}")
    print(f"{name} R {sha(eng.R)}")
    if dfeat is not None:
        print(f"{name} dfeat {sha(dfeat)}")
    print(f"{name} nbt {int(eng.nbt)}")
    print(f"{name} tape {' '.join(sorted(tape.t)) if tape is not None else '-'}")
    sys.stdout.flush()


def train_case(name: str, eng, x, training: bool = True) -> None:
    heat, tape = eng.forward(x, training=training)
    eng.zero_grad()
    g_heat = torch.randn(heat.shape, generator=torch.Generator().manual_seed(11)).to(heat.device) * heat
    dfeat = eng.backward(tape, g_heat)
    report(name, eng, heat, tape, dfeat)


def infer_case(name: str, eng, x) -> None:
    eng.zero_grad()
    report(name, eng, eng.forward_infer(x))


def main() -> None:
    dev = device()
    from lightning_pose_amd.engine import Engine, HeadEngine
    from lightning_pose_amd.engine_fp32 import Fp32Engine
    from lightning_pose_amd.vit_engine import ViTEngine
    from lightning_pose_amd.vit_engine_fp32 import Fp32ViTEngine

    eng = Engine(17, 2, dev)
    seed_parameters(eng, 1)
    train_case("resnet.single", eng, images(dev, 2, 4, 3, 64, 64))
    train_case("resnet.joint", eng, (images(dev, 3, 8, 3, 128, 128), images(dev, 4, 8, 3, 128, 128)))
    infer_case("resnet.infer", eng, images(dev, 2, 4, 3, 64, 64))
    train_case("resnet.eval", eng, images(dev, 5, 4, 3, 64, 64), training=False)

    for name, kw, batch in (("vit.single", {}, 2), ("vit.views2", dict(num_views=2), 4), ("vit.dinov2", dict(arch="dinov2"), 2)):
        eng = ViTEngine(5, 2, dev, **SMALL, **kw)
        seed_parameters(eng, 6)
        train_case(name, eng, images(dev, 7, batch, 3, 64, 64))
        if not kw:
            train_case("vit.joint", eng, (images(dev, 7, 2, 3, 64, 64), images(dev, 8, 3, 3, 64, 64)))
            infer_case("vit.infer", eng, images(dev, 7, 2, 3, 64, 64))

    for name, kw in (("head.default", {}), ("head.options", dict(deconv_out_channels=32, final_softmax=False))):
        eng = HeadEngine(512, 32, 5, 2, device=dev, **kw)
        seed_parameters(eng, 9)
        train_case(name, eng, images(dev, 10, 2, 512, 4, 4))

    eng = Fp32Engine(17, 2, dev)
    seed_parameters(eng, 1)
    train_case("fp32.resnet", eng, images(dev, 2, 2, 3, 64, 64))
    train_case("fp32.resnet.joint", eng, (images(dev, 2, 2, 3, 64, 64), images(dev, 3, 2, 3, 64, 64)))
    eng = Fp32ViTEngine(5, 2, dev, **SMALL)
    seed_parameters(eng, 6)
    train_case("fp32.vit", eng, images(dev, 7, 2, 3, 64, 64))
    eng = Fp32ViTEngine(5, 2, dev, **SMALL, arch="dinov2")
    seed_parameters(eng, 6)
    train_case("fp32.vit.dinov2", eng, images(dev, 7, 2, 3, 64, 64))


if __name__ == "__main__":
    main()
