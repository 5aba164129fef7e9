"""The DINOv2 backbones ("vits_dinov2" / "vitb_dinov2") through the public surface: registry, both tracker classes from ``get_model``, a short
FusedAdam run, parameter groups, ``pretrained=True`` with and without a ``Dinov2Model`` checkpoint (14 x 14 projection resampled to 16 x 16 as the
reference does), the Lightning-style ``.ckpt`` round trip, and the multi-view refusal.  A 2-layer / 2-head model of width 128 stands in for
DINOv2-small (tests/test_dinov2_engine.py holds the engine to the HF model)."""

import importlib.util
import os

import numpy as np
import pytest
import torch

transformers = pytest.importorskip("transformers")

PRE = "backbone.vision_encoder."
TINY = (128, 2, 2, 256, 16, 3)      # hidden, depth, heads, mlp, patch, pretraining grid
PROJ = PRE + "embeddings.patch_embeddings.projection.weight"


@pytest.fixture
def tiny_dinov2(monkeypatch):
    from lightning_pose_amd.models.backbones import factory as bf
    monkeypatch.setitem(bf.DINOV2_CONFIGS, "vits_dinov2", TINY)
    monkeypatch.setitem(bf._IMPLEMENTED, "vits_dinov2", TINY[0])


def _hf_model(patch, seed=0):
    from transformers import Dinov2Config, Dinov2Model
    torch.manual_seed(seed)
    cfg = Dinov2Config(hidden_size=TINY[0], num_hidden_layers=TINY[1], num_attention_heads=TINY[2], mlp_ratio=2, image_size=patch * TINY[5],
                       patch_size=patch)
    m = Dinov2Model(cfg)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith("lambda1") or n.endswith(".bias"):
                p.normal_(std=0.5)
    return m


def _tracker(dev, semi=False, **kw):
    from lightning_pose_amd.losses import LossFactory
    from lightning_pose_amd.models import get_model_class
    args = dict(num_keypoints=3, loss_factory=LossFactory({"heatmap_mse": {"log_weight": 0.0}}, None), backbone="vits_dinov2", pretrained=False,
                torch_seed=0, device=dev, optimizer="AdamW", optimizer_params={"learning_rate": 1e-3})
    if semi:
        args["loss_factory_unsupervised"] = LossFactory({"temporal": {"log_weight": 5.0, "epsilon": 5.0}}, None)
    args.update(kw)
    return get_model_class("heatmap", semi)(**args)


def test_registry_values_and_strides():
    from lightning_pose_amd.models.backbones import BACKBONE_STRIDES, backbone_features
    from lightning_pose_amd.models.backbones.factory import DINOV2_CONFIGS, VIT_CONFIGS
    from lightning_pose_amd.models.heatmap_tracker_multiview import ALLOWED_TRANSFORMER_BACKBONES_MULTIVIEW

    assert backbone_features("vits_dinov2") == 384 and backbone_features("vitb_dinov2") == 768
    assert BACKBONE_STRIDES["vits_dinov2"] == 16 and BACKBONE_STRIDES["vitb_dinov2"] == 16
    assert DINOV2_CONFIGS == {"vits_dinov2": (384, 12, 6, 1536, 16, 37), "vitb_dinov2": (768, 12, 12, 3072, 16, 37)}
    assert not set(DINOV2_CONFIGS) & set(VIT_CONFIGS)
    assert ALLOWED_TRANSFORMER_BACKBONES_MULTIVIEW == ("vits_dino", "vitb_dino")     # multi-view DINOv2 is not part of this package
    for other in ("vits_dinov3", "vitb_dinov3", "vitb_imagenet", "vitb_sam"):        # ... and neither are these, in any tracker
        with pytest.raises(ValueError, match="is not a valid backbone"):
            backbone_features(other)


def test_get_model_builds_both_tracker_classes(stack_backend, tiny_dinov2, monkeypatch):
    from lightning_pose_amd.losses import LossFactory
    from lightning_pose_amd.models import HeatmapTracker, SemiSupervisedHeatmapTracker, heatmap_tracker
    from lightning_pose_amd.models.factory import get_model
    from lightning_pose_amd.vit_engine import ViTEngine
    from lightning_pose_amd.vit_engine_fp32 import Fp32ViTEngine

    dev = stack_backend
    monkeypatch.setattr(heatmap_tracker, "_default_device", lambda: dev)
    cfg = {"model": {"model_type": "heatmap", "backbone": "vits_dinov2", "backbone_pretrained": False, "losses_to_use": []},
           "data": {"image_resize_dims": {"height": 64, "width": 64}, "num_keypoints": 3, "downsample_factor": 2},
           "training": {"rng_seed_model_pt": 0, "optimizer": "Adam", "optimizer_params": {"learning_rate": 1e-3}}}
    sup = LossFactory({"heatmap_mse": {"log_weight": 0.0}}, None)
    unsup = LossFactory({"temporal": {"log_weight": 5.0, "epsilon": 5.0}}, None)
    m = get_model(cfg, None, {"supervised": sup, "unsupervised": None})
    assert type(m) is HeatmapTracker and type(m.net) is ViTEngine and m.net.arch == "dinov2" and m.net.ln_eps == 1e-6
    assert m.num_fc_input_features == 128 and m.net.grid0 == 3 and m.net.plan.patch == 16
    cfg["model"]["losses_to_use"] = ["temporal"]
    m2 = get_model(cfg, None, {"supervised": sup, "unsupervised": unsup})
    assert type(m2) is SemiSupervisedHeatmapTracker and m2.net.arch == "dinov2"
    m3 = _tracker(dev, precision="fp32")
    assert type(m3.net) is Fp32ViTEngine and m3.net.arch == "dinov2"
    # the state_dict carries Dinov2Model's names under the reference's prefix; seeding is reproducible and honours torch_seed
    hf_keys = {PRE + k for k in _hf_model(16).state_dict()}
    sd = m.state_dict()
    assert {k for k in sd if k.startswith(PRE)} == hf_keys and set(sd) - hf_keys == {"head.upsampling_layers.1.weight", "head.upsampling_layers.1.bias"}
    again, other = _tracker(dev, optimizer="Adam").state_dict(), _tracker(dev, torch_seed=1).state_dict()
    assert all(torch.equal(sd[k].cpu(), again[k].cpu()) for k in sd)
    assert not torch.equal(sd[PROJ].cpu(), other[PROJ].cpu())
    assert torch.equal(sd[PRE + "encoder.layer.0.layer_scale1.lambda1"].cpu(), torch.ones(128)) and not sd[PRE + "embeddings.mask_token"].any()
    m.eval()
    with torch.no_grad():
        heat = m(torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(0)).to(dev))
    assert heat.shape == (2, 3, 16, 16)


@pytest.mark.parametrize("precision", ["bf16-mixed", "fp32"])
def test_training_lowers_the_loss_and_moves_lambda1(stack_backend, tiny_dinov2, precision):
    from lightning_pose_amd import ops
    from lightning_pose_amd.optim import FusedAdam
    from lightning_pose_amd.trainer import Trainer

    dev = stack_backend
    model = _tracker(dev, precision=precision)
    # parameter groups: everything under backbone.* - lambda1 and mask_token included - is the backbone group (frozen until unfrozen)
    groups = model.get_parameters()
    assert [g["name"] for g in groups] == ["backbone", "head"] and groups[0]["lr"] == 0
    named = dict(model.named_parameters())
    bb = {id(p) for p in groups[0]["params"]}
    for n in (PRE + "encoder.layer.0.layer_scale1.lambda1", PRE + "encoder.layer.1.layer_scale2.lambda1", PRE + "embeddings.mask_token",
              PRE + "encoder.layer.0.attention.attention.key.bias"):
        assert id(named[n]) in bb, n
    assert len(bb) + len(groups[1]["params"]) == len(named)
    lo, hi = model.net.plan.group_ranges()["backbone"]
    for n, p in named.items():   # ... and one contiguous range of the flat buffer the fused optimiser steps
        off = (p.data_ptr() - model.net.P.data_ptr()) // 4
        assert (lo <= off and off + p.numel() <= hi) == n.startswith("backbone."), n

    gen = torch.Generator().manual_seed(0)
    kp = torch.rand(2, 3, 2, generator=gen) * 60 + 2
    batch = {"images": torch.randn(2, 3, 64, 64, generator=gen).to(dev), "keypoints": kp.reshape(2, -1).to(dev),
             "heatmaps": ops.generate_heatmaps(kp.to(dev), 64, 64, (16, 16)), "bbox": torch.tensor([[0.0, 0.0, 64.0, 64.0]] * 2).to(dev)}
    tr = Trainer(data_parallel=False)
    tr.setup(model)
    opt = model.optimizers()
    assert isinstance(opt, FusedAdam)
    model.train()
    lam = named[PRE + "encoder.layer.0.layer_scale1.lambda1"]
    tr.training_batch(model, batch, 0)
    assert torch.equal(lam.detach().cpu(), torch.ones(128))        # frozen backbone: lr 0
    for g in opt.param_groups:                                     # unfreeze the backbone (what UnfreezeBackbone does at its epoch)
        g["lr"] = 1e-3
    losses = [float(tr.training_batch(model, batch, i)) for i in range(1, 6)]
    assert all(l == l for l in losses) and losses[-1] < losses[0], losses
    for n in ("encoder.layer.0.layer_scale1.lambda1", "encoder.layer.1.layer_scale2.lambda1"):
        moved = (named[PRE + n].detach().cpu() - 1).abs()
        assert moved.max() > 1e-4 and torch.isfinite(moved).all(), n
    assert not named[PRE + "embeddings.mask_token"].detach().any()   # zero gradient, zero weight: it stays where it was


def test_pretrained_needs_a_checkpoint(stack_backend, tiny_dinov2):
    with pytest.raises(RuntimeError, match="pretrained=True needs the DINOv2 weights"):
        _tracker(stack_backend, pretrained=True)


def _reference_resize(weight14):
    """the reference's own ``_resize_patch_embedding_weights`` on a config-built model, where its tree is present"""
    from oracle import ref_loader
    path = os.path.join(ref_loader.REFERENCE_ROOT, "lightning_pose", "models", "backbones", "vit_dino.py")
    if not os.path.isfile(path):
        return None
    spec = importlib.util.spec_from_file_location("_ref_vit_dino", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    enc = mod.VisionEncoderDino.__new__(mod.VisionEncoderDino)
    torch.nn.Module.__init__(enc)
    enc.vision_encoder = _hf_model(14)
    with torch.no_grad():
        enc.vision_encoder.embeddings.patch_embeddings.projection.weight.copy_(weight14)
    enc.patch_size = 16
    enc._resize_patch_embedding_weights()
    return enc.vision_encoder.embeddings.patch_embeddings.projection.weight.detach()


@pytest.mark.parametrize("fmt", ["pt", "safetensors", "ckpt"])
def test_dinov2_checkpoint_with_a_14px_projection_is_resampled(stack_backend, tiny_dinov2, tmp_path, fmt, golden):
    from lightning_pose_amd.models.backbones.dinov2 import resize_patch_projection

    dev = stack_backend
    hf = _hf_model(14, seed=3)
    hf_sd = {k: v.detach().clone() for k, v in hf.state_dict().items()}
    assert hf_sd["embeddings.patch_embeddings.projection.weight"].shape == (128, 3, 14, 14)
    path = str(tmp_path / ("dinov2." + ("safetensors" if fmt == "safetensors" else "pt")))
    if fmt == "safetensors":
        import safetensors.torch
        safetensors.torch.save_file({k: v.contiguous() for k, v in hf_sd.items()}, path)
    elif fmt == "ckpt":     # a torch.save'd dict with the tensors under "state_dict", names already prefixed
        torch.save({"state_dict": {PRE + k: v for k, v in hf_sd.items()}}, path)
    else:
        torch.save(hf_sd, path)
    model = _tracker(dev, pretrained=True, backbone_checkpoint=path)
    sd = {k: v.cpu() for k, v in model.state_dict().items()}
    for k, v in hf_sd.items():
        if k != "embeddings.patch_embeddings.projection.weight":
            assert torch.equal(sd[PRE + k], v.reshape(sd[PRE + k].shape)), k       # bias included: copied as it is
    want = _reference_resize(hf_sd["embeddings.patch_embeddings.projection.weight"])
    if want is not None:
        assert torch.equal(sd[PROJ], want)
    assert sd[PROJ].shape == (128, 3, 16, 16)
    # ... and, wherever this runs, the helper against the array recorded from the reference's function
    g = golden("dinov2_patch_resize")
    got = resize_patch_projection(g.t("weight14"))
    torch.testing.assert_close(got, g.t("weight16"), atol=1e-6, rtol=1e-6)
    assert torch.equal(model.net.Wb[model.net.plan.patch_lin.w_off:][:128 * 768].cpu().view(128, 3, 16, 16), sd[PROJ].to(torch.bfloat16))


def test_dinov2_checkpoint_with_a_16px_projection_loads_unchanged(stack_backend, tiny_dinov2, tmp_path):
    dev = stack_backend
    hf_sd = {k: v.detach().clone() for k, v in _hf_model(16, seed=4).state_dict().items()}
    torch.save(hf_sd, str(tmp_path / "dinov2_p16.pt"))
    model = _tracker(dev, pretrained=True, backbone_checkpoint=str(tmp_path / "dinov2_p16.pt"))
    sd = model.state_dict()
    for k, v in hf_sd.items():
        assert torch.equal(sd[PRE + k].cpu(), v.reshape(sd[PRE + k].shape)), k
    bad = dict(hf_sd)
    bad["encoder.layer.0.mlp.fc1.weight"] = torch.zeros(64, 128)      # a tensor of another model: an error, not a silent skip
    torch.save(bad, str(tmp_path / "bad.pt"))
    with pytest.raises(ValueError, match="mlp.fc1.weight has shape"):
        _tracker(dev, pretrained=True, backbone_checkpoint=str(tmp_path / "bad.pt"))


def test_lightning_style_ckpt_round_trip(stack_backend, tiny_dinov2, tmp_path):
    from lightning_pose_amd import checkpoint as ck
    from lightning_pose_amd.models import SemiSupervisedHeatmapTracker

    dev = stack_backend
    model = _tracker(dev, semi=True, torch_seed=1, image_size=64)
    with torch.no_grad():
        model.state_dict()[PRE + "encoder.layer.1.layer_scale1.lambda1"].uniform_(-1.5, 1.5)
    model.net.refresh_weight_copies()
    assert model.hparams["backbone"] == "vits_dinov2"
    path = ck.save_checkpoint(model, str(tmp_path / "dinov2.ckpt"), optimizer=model.configure_optimizers()["optimizer"])
    raw = torch.load(path, map_location="cpu", weights_only=False)
    assert PRE + "encoder.layer.1.layer_scale2.lambda1" in raw["state_dict"] and PRE + "embeddings.mask_token" in raw["state_dict"]
    again = ck.load_model_from_checkpoint(path, strict=True, loss_factory=model.loss_factory, loss_factory_unsupervised=model.loss_factory_unsup,
                                          device=dev)
    assert type(again) is SemiSupervisedHeatmapTracker and again.net.arch == "dinov2"
    a, b = model.state_dict(), again.state_dict()
    assert set(a) == set(b) and all(torch.equal(a[k].cpu(), b[k].cpu()) for k in a)
    assert torch.equal(model.net.Wb.cpu(), again.net.Wb.cpu())
    # the backbone half loads strictly into the HF model itself
    hf = _hf_model(16)
    hf.load_state_dict({k[len(PRE):]: v.cpu() for k, v in a.items() if k.startswith(PRE)}, strict=True)


def test_multi_view_with_dinov2_raises(stack_backend, tiny_dinov2):
    from lightning_pose_amd.models import HeatmapTrackerMultiviewTransformer
    from lightning_pose_amd.vit_engine import ViTEngine

    dev = stack_backend
    with pytest.raises(NotImplementedError, match="multi-view"):
        ViTEngine(3, 2, dev, hidden=128, depth=2, heads=2, mlp=256, patch=16, pretrain_grid=3, num_views=2, arch="dinov2")
    for exc in (NotImplementedError, ValueError):
        with pytest.raises(exc, match="is not supported for multiview transformer models"):
            HeatmapTrackerMultiviewTransformer(num_keypoints=3, num_views=2, backbone="vits_dinov2", pretrained=False, device=dev)
