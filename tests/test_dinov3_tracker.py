"""The DINOv3 backbones ("vits_dinov3" / "vitb_dinov3") through the public surface: registry, both tracker classes in both precisions,
``pretrained=True`` with and without a ``DINOv3ViTModel`` checkpoint (a gated-MLP checkpoint, a wrong shape and a ``k_proj.bias`` are refused
by name), a short FusedAdam run, the Lightning-style ``.ckpt`` round trip, ``train()`` / ``eval()`` reaching the rotary coordinates' draws, and
the multi-view refusal.  A 2-layer / 2-head model of width 128 stands in for DINOv3 ViT-S (tests/test_dinov3_engine.py holds the engine to the
HF model)."""

import pytest
import torch

transformers = pytest.importorskip("transformers")

PRE = "backbone.vision_encoder."
TINY = (128, 2, 2, 256, 16, 4)      # hidden, depth, heads, mlp, patch, register tokens
HEAD_KEYS = {"head.upsampling_layers.1.weight", "head.upsampling_layers.1.bias"}


@pytest.fixture
def tiny_dinov3(monkeypatch):
    from lightning_pose_amd.models.backbones import factory as bf
    monkeypatch.setitem(bf.DINOV3_CONFIGS, "vits_dinov3", TINY)


def _hf_model(seed=0, **kw):
    from transformers import DINOv3ViTConfig, DINOv3ViTModel
    torch.manual_seed(seed)
    cfg = DINOv3ViTConfig(hidden_size=TINY[0], num_hidden_layers=TINY[1], num_attention_heads=TINY[2], intermediate_size=TINY[3],
                          patch_size=16, num_register_tokens=TINY[5], image_size=48, **kw)
    m = DINOv3ViTModel(cfg)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith("lambda1") or n.endswith(".bias"):
                p.normal_(std=0.5)
    return m


def _tracker(dev, semi=False, **kw):
    from lightning_pose_amd.losses import LossFactory
    from lightning_pose_amd.models import get_model_class
    args = dict(num_keypoints=3, loss_factory=LossFactory({"heatmap_mse": {"log_weight": 0.0}}, None), backbone="vits_dinov3", pretrained=False,
                torch_seed=0, device=dev, optimizer="AdamW", optimizer_params={"learning_rate": 1e-3})
    if semi:
        args["loss_factory_unsupervised"] = LossFactory({"temporal": {"log_weight": 5.0, "epsilon": 5.0}}, None)
    args.update(kw)
    return get_model_class("heatmap", semi)(**args)


def _batch(dev, n=2, seed=0):
    from lightning_pose_amd import ops
    gen = torch.Generator().manual_seed(seed)
    kp = torch.rand(n, 3, 2, generator=gen) * 60 + 2
    return {"images": torch.randn(n, 3, 64, 64, generator=gen).to(dev), "keypoints": kp.reshape(n, -1).to(dev),
            "heatmaps": ops.generate_heatmaps(kp.to(dev), 64, 64, (16, 16)), "bbox": torch.tensor([[0.0, 0.0, 64.0, 64.0]] * n).to(dev)}


def test_registry_values_and_strides():
    from lightning_pose_amd.models.backbones import BACKBONE_STRIDES, backbone_features, tracker_backbone_features
    from lightning_pose_amd.models.backbones.factory import DINOV2_CONFIGS, DINOV3_CONFIGS, VIT_CONFIGS
    from lightning_pose_amd.models.heatmap_tracker_multiview import ALLOWED_TRANSFORMER_BACKBONES_MULTIVIEW

    # the widths come from DINOV3_CONFIGS through the single-view trackers' lookup; backbone_features() keeps its list (and, for every other
    # name, the two lookups agree)
    assert tracker_backbone_features("vits_dinov3") == 384 and tracker_backbone_features("vitb_dinov3") == 768
    for name in ("resnet50", "vits_dino", "vitb_dinov2"):
        assert tracker_backbone_features(name) == backbone_features(name)
    assert BACKBONE_STRIDES["vits_dinov3"] == 16 and BACKBONE_STRIDES["vitb_dinov3"] == 16
    assert DINOV3_CONFIGS == {"vits_dinov3": (384, 12, 6, 1536, 16, 4), "vitb_dinov3": (768, 12, 12, 3072, 16, 4)}
    assert not set(DINOV3_CONFIGS) & (set(VIT_CONFIGS) | set(DINOV2_CONFIGS))
    assert ALLOWED_TRANSFORMER_BACKBONES_MULTIVIEW == ("vits_dino", "vitb_dino")     # multi-view DINOv3 is not part of this package
    for other in ("vith_dinov3", "convnext_dinov3", "vitb_imagenet"):                # ... and the larger / ConvNeXt DINOv3 models are in no tracker
        with pytest.raises(ValueError, match="is not a valid backbone; allowed backbones: .*vits_dinov3"):
            tracker_backbone_features(other)


def test_get_model_builds_both_tracker_classes_in_both_precisions(stack_backend, tiny_dinov3, monkeypatch):
    from lightning_pose_amd.losses import LossFactory
    from lightning_pose_amd.models import HeatmapTracker, SemiSupervisedHeatmapTracker, heatmap_tracker
    from lightning_pose_amd.models.factory import get_model
    from lightning_pose_amd.vit_engine import ViTEngine
    from lightning_pose_amd.vit_engine_fp32 import Fp32ViTEngine

    dev = stack_backend
    monkeypatch.setattr(heatmap_tracker, "_default_device", lambda: dev)
    cfg = {"model": {"model_type": "heatmap", "backbone": "vits_dinov3", "backbone_pretrained": False, "losses_to_use": []},
           "data": {"image_resize_dims": {"height": 64, "width": 64}, "num_keypoints": 3, "downsample_factor": 2},
           "training": {"rng_seed_model_pt": 0, "optimizer": "Adam", "optimizer_params": {"learning_rate": 1e-3}}}
    sup = LossFactory({"heatmap_mse": {"log_weight": 0.0}}, None)
    unsup = LossFactory({"temporal": {"log_weight": 5.0, "epsilon": 5.0}}, None)
    m = get_model(cfg, None, {"supervised": sup, "unsupervised": None})
    assert type(m) is HeatmapTracker and type(m.net) is ViTEngine and m.net.arch == "dinov3" and m.net.ln_eps == 1e-5
    assert m.num_fc_input_features == 128 and m.net.plan.registers == 4 and m.net.plan.patch == 16 and m.net.plan.n_pos == 0
    assert m.net.rope_aug == dict(shift=None, jitter=None, rescale=2.0)              # the released configs' knobs
    cfg["model"]["losses_to_use"] = ["temporal"]
    m2 = get_model(cfg, None, {"supervised": sup, "unsupervised": unsup})
    assert type(m2) is SemiSupervisedHeatmapTracker and m2.net.arch == "dinov3"
    for semi in (False, True):
        m3 = _tracker(dev, semi=semi, precision="fp32")
        assert type(m3.net) is Fp32ViTEngine and m3.net.arch == "dinov3"
    # the state_dict carries DINOv3ViTModel's names under the reference's prefix; seeding is reproducible and honours torch_seed
    hf_keys = {PRE + k for k in _hf_model().state_dict()}
    sd = m.state_dict()
    assert {k for k in sd if k.startswith(PRE)} == hf_keys and set(sd) - hf_keys == HEAD_KEYS
    assert {n for n, _ in m.named_parameters()} == set(sd)                           # every entry is a parameter: no key bias anywhere
    proj = PRE + "embeddings.patch_embeddings.weight"
    again, other = _tracker(dev, optimizer="Adam").state_dict(), _tracker(dev, torch_seed=1).state_dict()
    assert all(torch.equal(sd[k].cpu(), again[k].cpu()) for k in sd)
    assert not torch.equal(sd[proj].cpu(), other[proj].cpu())
    assert torch.equal(sd[PRE + "model.layer.0.layer_scale1.lambda1"].cpu(), torch.ones(128)) and not sd[PRE + "embeddings.mask_token"].any()
    m.eval()
    with torch.no_grad():
        heat = m(torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(0)).to(dev))
    assert heat.shape == (2, 3, 16, 16)


def test_pretrained_needs_a_checkpoint(stack_backend, tiny_dinov3):
    with pytest.raises(RuntimeError, match="pretrained=True needs the DINOv3 weights.*facebook/dinov3-vits16-pretrain-lvd1689m"):
        _tracker(stack_backend, pretrained=True)
    from lightning_pose_amd.models.backbones.dinov3 import HF_NAMES
    assert HF_NAMES["vitb_dinov3"] == "facebook/dinov3-vitb16-pretrain-lvd1689m"


@pytest.mark.parametrize("fmt", ["pt", "safetensors", "ckpt"])
def test_dinov3_checkpoint_loads(stack_backend, tiny_dinov3, tmp_path, fmt):
    dev = stack_backend
    hf_sd = {k: v.detach().clone() for k, v in _hf_model(seed=3).state_dict().items()}
    path = str(tmp_path / ("dinov3." + ("safetensors" if fmt == "safetensors" else "pt")))
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
        assert torch.equal(sd[PRE + k], v), k
    w = model.net.plan.patch_lin
    assert torch.equal(model.net.Wb[w.w_off:][:128 * 768].cpu().view(128, 3, 16, 16), sd[PRE + "embeddings.patch_embeddings.weight"].to(torch.bfloat16))


def test_dinov3_checkpoint_refusals_name_the_key(stack_backend, tiny_dinov3, tmp_path):
    dev = stack_backend
    hf_sd = {k: v.detach().clone() for k, v in _hf_model(seed=4).state_dict().items()}

    def refused(sd, match, name):
        torch.save(sd, str(tmp_path / name))
        with pytest.raises(ValueError, match=match):
            _tracker(dev, pretrained=True, backbone_checkpoint=str(tmp_path / name))

    refused({**hf_sd, "model.layer.0.mlp.up_proj.weight": torch.zeros(64, 128)}, r"model\.layer\.0\.mlp\.up_proj\.weight has shape", "shape.pt")
    gated = {k: v.detach().clone() for k, v in _hf_model(seed=4, use_gated_mlp=True).state_dict().items()}
    assert "model.layer.0.mlp.gate_proj.weight" in gated
    refused(gated, r"mlp\.gate_proj\..* gated-MLP", "gated.pt")
    biased = {k: v.detach().clone() for k, v in _hf_model(seed=4, key_bias=True).state_dict().items()}
    assert "model.layer.1.attention.k_proj.bias" in biased
    refused(biased, r"model\.layer\.0\.attention\.k_proj\.bias.*no key bias", "keybias.pt")
    from lightning_pose_amd.models.backbones.dinov3 import dinov3_seeded_state_dict, load_dinov3_checkpoint
    init = dinov3_seeded_state_dict(*TINY)
    assert set(init) == {PRE + k for k in hf_sd}
    torch.save({**hf_sd, "pooler.dense.weight": torch.zeros(4, 4)}, str(tmp_path / "extra.pt"))     # keys of other modules are ignored
    load_dinov3_checkpoint(str(tmp_path / "extra.pt"), init)
    assert all(torch.equal(init[PRE + k], v) for k, v in hf_sd.items())


@pytest.mark.parametrize("precision", ["bf16-mixed", "fp32"])
def test_training_lowers_the_loss(stack_backend, tiny_dinov3, precision):
    from lightning_pose_amd.optim import FusedAdam
    from lightning_pose_amd.trainer import Trainer

    dev = stack_backend
    model = _tracker(dev, precision=precision)
    groups = model.get_parameters()
    assert [g["name"] for g in groups] == ["backbone", "head"] and groups[0]["lr"] == 0
    named = dict(model.named_parameters())
    bb = {id(p) for p in groups[0]["params"]}
    for n in (PRE + "model.layer.0.layer_scale1.lambda1", PRE + "embeddings.register_tokens", PRE + "embeddings.mask_token",
              PRE + "embeddings.cls_token", PRE + "model.layer.1.attention.q_proj.bias"):
        assert id(named[n]) in bb, n
    assert len(bb) + len(groups[1]["params"]) == len(named)
    lo, hi = model.net.plan.group_ranges()["backbone"]
    for n, p in named.items():   # one contiguous range of the flat buffer the fused optimiser steps
        off = (p.data_ptr() - model.net.P.data_ptr()) // 4
        assert (lo <= off and off + p.numel() <= hi) == n.startswith("backbone."), n
    batch = _batch(dev)
    tr = Trainer(data_parallel=False)
    tr.setup(model)
    opt = model.optimizers()
    assert isinstance(opt, FusedAdam)
    model.train()
    reg0 = named[PRE + "embeddings.register_tokens"].detach().cpu().clone()
    tr.training_batch(model, batch, 0)
    assert torch.equal(named[PRE + "embeddings.register_tokens"].detach().cpu(), reg0)        # frozen backbone: lr 0
    for g in opt.param_groups:                                     # unfreeze the backbone (what UnfreezeBackbone does at its epoch)
        g["lr"] = 1e-3
    losses = [float(tr.training_batch(model, batch, i)) for i in range(1, 7)]
    assert all(l == l for l in losses) and losses[-1] < losses[0], losses
    for n in ("embeddings.register_tokens", "embeddings.cls_token", "model.layer.1.layer_scale2.lambda1"):
        moved = (named[PRE + n].detach().cpu() - (reg0 if n.endswith("register_tokens") else 0)).abs()
        assert torch.isfinite(moved).all(), n
    assert (named[PRE + "embeddings.register_tokens"].detach().cpu() - reg0).abs().max() > 1e-4
    assert not named[PRE + "embeddings.mask_token"].detach().any()   # zero gradient, zero weight: it stays where it was


def test_lightning_style_ckpt_round_trip(stack_backend, tiny_dinov3, tmp_path):
    from lightning_pose_amd import checkpoint as ck
    from lightning_pose_amd.models import SemiSupervisedHeatmapTracker

    dev = stack_backend
    model = _tracker(dev, semi=True, torch_seed=1, image_size=64)
    with torch.no_grad():
        model.state_dict()[PRE + "model.layer.1.layer_scale1.lambda1"].uniform_(-1.5, 1.5)
        model.state_dict()[PRE + "embeddings.register_tokens"].normal_(std=0.5)
    model.net.refresh_weight_copies()
    assert model.hparams["backbone"] == "vits_dinov3"
    path = ck.save_checkpoint(model, str(tmp_path / "dinov3.ckpt"), optimizer=model.configure_optimizers()["optimizer"])
    raw = torch.load(path, map_location="cpu", weights_only=False)
    assert PRE + "embeddings.register_tokens" in raw["state_dict"] and PRE + "model.layer.1.mlp.down_proj.weight" in raw["state_dict"]
    assert not any(k.endswith("k_proj.bias") for k in raw["state_dict"])
    again = ck.load_model_from_checkpoint(path, strict=True, loss_factory=model.loss_factory, loss_factory_unsupervised=model.loss_factory_unsup,
                                          device=dev)
    assert type(again) is SemiSupervisedHeatmapTracker and again.net.arch == "dinov3" and again.net.plan.registers == 4
    a, b = model.state_dict(), again.state_dict()
    assert set(a) == set(b) and all(torch.equal(a[k].cpu(), b[k].cpu()) for k in a)
    assert torch.equal(model.net.Wb.cpu(), again.net.Wb.cpu())
    # the backbone half loads strictly into the HF model itself
    _hf_model().load_state_dict({k[len(PRE):]: v.cpu() for k, v in a.items() if k.startswith(PRE)}, strict=True)


def test_eval_predictions_are_deterministic_and_train_forwards_draw(stack_backend, tiny_dinov3):
    """predict_step under eval() uses the plain coordinates; under train() every forward draws a new rescale"""
    dev = stack_backend
    model = _tracker(dev)
    batch = _batch(dev, seed=5)
    model.eval()
    with torch.no_grad():
        kp1, conf1, heat1 = model.predict_step(batch, 0, return_heatmaps=True)
        kp2, conf2, heat2 = model.predict_step(batch, 0, return_heatmaps=True)
    assert torch.equal(heat1, heat2) and torch.equal(kp1, kp2) and torch.equal(conf1, conf2)
    assert torch.equal(heat1, model.net.forward(batch["images"], training=False)[0])
    model.train()
    assert model.training
    a, b = model(batch["images"]), model(batch["images"])           # (grad enabled: Engine.forward(training=True))
    assert not torch.equal(a, b) and not torch.equal(a.detach(), heat1)
    with torch.no_grad():
        c, d = model(batch["images"]), model(batch["images"])
    assert not torch.equal(c, d)
    model.eval()
    with torch.no_grad():
        assert torch.equal(model(batch["images"]), heat1)


def test_multi_view_with_dinov3_raises(stack_backend, tiny_dinov3):
    from lightning_pose_amd.models import HeatmapTrackerMultiviewTransformer
    from lightning_pose_amd.models.heatmap_tracker_multiview import BackboneNotImplementedError
    from lightning_pose_amd.vit_engine import ViTEngine

    dev = stack_backend
    with pytest.raises(NotImplementedError, match="multi-view"):
        ViTEngine(3, 2, dev, hidden=128, depth=2, heads=2, mlp=256, patch=16, num_views=2, arch="dinov3")
    for name in ("vits_dinov3", "vitb_dinov3"):
        with pytest.raises(BackboneNotImplementedError, match="is not supported for multiview transformer models"):
            HeatmapTrackerMultiviewTransformer(num_keypoints=3, num_views=2, backbone=name, pretrained=False, device=dev)
