"""The SAM backbone ("vitb_sam") through the public surface: registry, both tracker classes in both precisions, ``pretrained=True`` with and
without a ``SamModel`` / ``SamVisionEncoder`` checkpoint (prefixes, foreign keys, the position table's resize, a wrong shape refused by name),
a short FusedAdam run, the Lightning-style ``.ckpt`` round trip, the refusals that remain, and one semi-supervised step against the
reference's own tracker (tests/golden/step_sam.npz, made by tests/golden/make_golden_sam.py) at tests/test_step_parity.py's bars.  A 3-layer /
2-head model of width 128 stands in for SAM ViT-B (tests/test_sam_engine.py holds the engine to the HF module)."""

import pytest
import torch
import torch.nn.functional as F

from oracle import restated as O
from tests.golden.step_inputs import PCA_LOG_WEIGHT, TEMPORAL, TORCH_SEED, make_step_inputs, seeded_backbone_weights
from tests.golden.step_inputs_sam import SAM_VIT

transformers = pytest.importorskip("transformers")

PRE = "backbone.vision_encoder."
TINY = (128, 3, 2, 256, 16, 3, (1,), 8, 32)   # hidden, depth, heads, mlp, patch, window, global layers, pretraining grid, neck channels
SIDE = 80                                     # a 5 x 5 grid under window 3: four windows, three of them ragged
HEAD_KEYS = {"head.upsampling_layers.1.weight", "head.upsampling_layers.1.bias"}


@pytest.fixture
def tiny_sam(monkeypatch):
    from lightning_pose_amd.models.backbones import factory as bf
    monkeypatch.setitem(bf.SAM_CONFIGS, "vitb_sam", TINY)


def _vision_config(cfg=TINY):
    hidden, depth, heads, mlp, patch, window, global_layers, grid0, neck = cfg
    return transformers.SamVisionConfig(hidden_size=hidden, num_hidden_layers=depth, num_attention_heads=heads, mlp_dim=mlp, patch_size=patch,
                                        image_size=patch * grid0, window_size=window, global_attn_indexes=list(global_layers),
                                        output_channels=neck, initializer_range=0.02)


def _hf_encoder(seed=0, grid=None):
    from transformers.models.sam.modeling_sam import SamVisionEncoder
    torch.manual_seed(seed)
    m = SamVisionEncoder(_vision_config())
    with torch.no_grad():
        for n, p in m.named_parameters():
            if p.dim() == 1 or "rel_pos" in n or n == "pos_embed":
                p.normal_(std=0.3)
    if grid is not None:
        m.pos_embed = torch.nn.Parameter(torch.zeros(1, grid, grid, TINY[0]))
    return m


def _tracker(dev, semi=False, **kw):
    from lightning_pose_amd.losses import LossFactory
    from lightning_pose_amd.models import get_model_class
    args = dict(num_keypoints=3, loss_factory=LossFactory({"heatmap_mse": {"log_weight": 0.0}}, None), backbone="vitb_sam", pretrained=False,
                torch_seed=0, device=dev, optimizer="AdamW", optimizer_params={"learning_rate": 1e-3}, image_size=SIDE)
    if semi:
        args["loss_factory_unsupervised"] = LossFactory({"temporal": {"log_weight": 5.0, "epsilon": 5.0}}, None)
    args.update(kw)
    return get_model_class("heatmap", semi)(**args)


def _batch(dev, n=2, seed=0):
    from lightning_pose_amd import ops
    gen = torch.Generator().manual_seed(seed)
    kp = torch.rand(n, 3, 2, generator=gen) * (SIDE - 4) + 2
    return {"images": torch.randn(n, 3, SIDE, SIDE, generator=gen).to(dev), "keypoints": kp.reshape(n, -1).to(dev),
            "heatmaps": ops.generate_heatmaps(kp.to(dev), SIDE, SIDE, (SIDE // 4, SIDE // 4)),
            "bbox": torch.tensor([[0.0, 0.0, float(SIDE), float(SIDE)]] * n).to(dev)}


def test_registry_values_and_the_refusals_that_remain():
    from lightning_pose_amd.models.backbones import BACKBONE_STRIDES, backbone_features, tracker_backbone_features
    from lightning_pose_amd.models.backbones import sam
    from lightning_pose_amd.models.backbones.factory import DINOV2_CONFIGS, DINOV3_CONFIGS, SAM_CONFIGS, VIT_CONFIGS
    from lightning_pose_amd.models.heatmap_tracker_multiview import ALLOWED_TRANSFORMER_BACKBONES_MULTIVIEW

    assert tracker_backbone_features("vitb_sam") == 768 and BACKBONE_STRIDES["vitb_sam"] == 16
    assert SAM_CONFIGS is sam.SAM_CONFIGS == {"vitb_sam": (768, 12, 12, 3072, 16, 14, (2, 5, 8, 11), 64, 256)}
    assert not set(SAM_CONFIGS) & (set(VIT_CONFIGS) | set(DINOV2_CONFIGS) | set(DINOV3_CONFIGS))
    for name in ("resnet50", "vits_dino", "vitb_dinov2"):
        assert tracker_backbone_features(name) == backbone_features(name)
    with pytest.raises(ValueError, match="is not a valid backbone"):        # backbone_features() keeps its list (tests/test_dinov2_tracker.py)
        backbone_features("vitb_sam")
    assert ALLOWED_TRANSFORMER_BACKBONES_MULTIVIEW == ("vits_dino", "vitb_dino")     # multi-view SAM is not part of this package
    for other in ("vitb_sam2", "vits_sam2", "vitb_imagenet"):                         # ... and Hiera / MAE are in no tracker
        with pytest.raises(ValueError, match="is not a valid backbone; allowed backbones: .*vitb_sam"):
            tracker_backbone_features(other)


def test_multi_view_with_sam_raises(stack_backend, tiny_sam):
    from lightning_pose_amd.models import HeatmapTrackerMultiviewTransformer
    with pytest.raises(ValueError, match="is not supported for multiview transformer models"):
        HeatmapTrackerMultiviewTransformer(num_keypoints=3, num_views=2, backbone="vitb_sam", pretrained=False, device=stack_backend)


def test_get_model_builds_both_tracker_classes_in_both_precisions(stack_backend, tiny_sam, monkeypatch):
    from lightning_pose_amd.losses import LossFactory
    from lightning_pose_amd.models import HeatmapTracker, SemiSupervisedHeatmapTracker, heatmap_tracker
    from lightning_pose_amd.models.factory import get_model
    from lightning_pose_amd.vit_engine import ViTEngine
    from lightning_pose_amd.vit_engine_fp32 import Fp32ViTEngine

    dev = stack_backend
    monkeypatch.setattr(heatmap_tracker, "_default_device", lambda: dev)
    cfg = {"model": {"model_type": "heatmap", "backbone": "vitb_sam", "backbone_pretrained": False, "losses_to_use": []},
           "data": {"image_resize_dims": {"height": SIDE, "width": SIDE}, "num_keypoints": 3, "downsample_factor": 2},
           "training": {"rng_seed_model_pt": 0, "optimizer": "Adam", "optimizer_params": {"learning_rate": 1e-3}}}
    sup = LossFactory({"heatmap_mse": {"log_weight": 0.0}}, None)
    unsup = LossFactory({"temporal": {"log_weight": 5.0, "epsilon": 5.0}}, None)
    m = get_model(cfg, None, {"supervised": sup, "unsupervised": None})
    assert type(m) is HeatmapTracker and type(m.net) is ViTEngine and m.net.arch == "sam" and m.net.ln_eps == 1e-6
    assert m.num_fc_input_features == 128 and m.net.plan.patch == 16 and m.net.plan.n_pos == 25 and m.net.sam_grid == 5
    assert [L["window"] for L in m.net.plan.layers] == [3, 0, 3]
    cfg["model"]["losses_to_use"] = ["temporal"]
    m2 = get_model(cfg, None, {"supervised": sup, "unsupervised": unsup})
    assert type(m2) is SemiSupervisedHeatmapTracker and m2.net.arch == "sam"
    for semi in (False, True):
        m3 = _tracker(dev, semi=semi, precision="fp32")
        assert type(m3.net) is Fp32ViTEngine and m3.net.arch == "sam"
    # the state_dict carries SamVisionEncoder's names under the reference's prefix; rel_pos_* / neck.* are buffers, everything else trains
    hf_keys = {PRE + k for k in _hf_encoder().state_dict()}
    sd = m.state_dict()
    assert {k for k in sd if k.startswith(PRE)} == hf_keys and set(sd) - hf_keys == HEAD_KEYS
    carried = {k for k in sd if "rel_pos" in k or ".neck." in k}
    assert {n for n, _ in m.named_parameters()} == set(sd) - carried and {n for n, _ in m.named_buffers()} == carried
    assert sd[PRE + "pos_embed"].shape == (1, 5, 5, 128)
    proj = PRE + "patch_embed.projection.weight"
    again, other = _tracker(dev, optimizer="Adam").state_dict(), _tracker(dev, torch_seed=1).state_dict()
    assert all(torch.equal(sd[k].cpu(), again[k].cpu()) for k in sd)
    assert not torch.equal(sd[proj].cpu(), other[proj].cpu()) and float(sd[proj].std()) > 1e-3     # (not SamVisionConfig's 1e-10)
    m.eval()
    with torch.no_grad():
        heat = m(torch.randn(2, 3, SIDE, SIDE, generator=torch.Generator().manual_seed(0)).to(dev))
    assert heat.shape == (2, 3, SIDE // 4, SIDE // 4)
    with pytest.raises(ValueError, match="built for 80 x 80 images"):       # the position table holds exactly the fine-tuning grid
        with torch.no_grad():
            m(torch.zeros(1, 3, 64, 64).to(dev))


def test_pretrained_needs_a_checkpoint(stack_backend, tiny_sam):
    with pytest.raises(RuntimeError, match="pretrained=True needs the SAM weights.*facebook/sam-vit-base"):
        _tracker(stack_backend, pretrained=True)
    with pytest.raises(FileNotFoundError):
        _tracker(stack_backend, pretrained=True, backbone_checkpoint="/nonexistent/sam.pt")


def _sam_model_state():
    """a synthetic whole-``SamModel`` state dict: ``vision_encoder.*`` next to ``prompt_encoder.*`` / ``mask_decoder.*``"""
    torch.manual_seed(3)
    full = transformers.SamModel(transformers.SamConfig(vision_config=_vision_config()))
    sd = {k: v.detach().clone() for k, v in full.state_dict().items()}
    gen = torch.Generator().manual_seed(4)
    for k in sd:
        if k.startswith("vision_encoder.") and (sd[k].dim() == 1 or "rel_pos" in k or k.endswith("pos_embed")):
            sd[k] = 0.3 * torch.randn(sd[k].shape, generator=gen)
    assert any(k.startswith("prompt_encoder.") for k in sd) and any(k.startswith("mask_decoder.") for k in sd)
    assert sd["vision_encoder.pos_embed"].shape == (1, 8, 8, 128)
    return sd


@pytest.mark.parametrize("fmt", ["sam_model.pt", "sam_model.safetensors", "encoder.pt", "ckpt"])
def test_sam_checkpoint_loads(stack_backend, tiny_sam, tmp_path, fmt):
    dev = stack_backend
    full = _sam_model_state()
    enc = {k[len("vision_encoder."):]: v for k, v in full.items() if k.startswith("vision_encoder.")}
    path = str(tmp_path / ("sam." + ("safetensors" if fmt.endswith("safetensors") else "pt")))
    if fmt == "sam_model.safetensors":
        import safetensors.torch
        safetensors.torch.save_file({k: v.contiguous() for k, v in full.items()}, path)
    elif fmt == "sam_model.pt":
        torch.save(full, path)
    elif fmt == "encoder.pt":      # a bare SamVisionEncoder state dict: no prefix
        torch.save(enc, path)
    else:                          # a torch.save'd dict with the tensors under "state_dict", names already prefixed
        torch.save({"state_dict": {PRE + k: v for k, v in enc.items()}}, path)
    model = _tracker(dev, pretrained=True, backbone_checkpoint=path)
    sd = {k: v.cpu() for k, v in model.state_dict().items()}
    for k, v in enc.items():
        if k != "pos_embed":
            assert torch.equal(sd[PRE + k], v), k
    assert not any(k.startswith(("prompt_encoder", "mask_decoder", "shared_image_embedding")) or "prompt_encoder" in k for k in sd)
    # the 8 x 8 pretraining table resized to the 5 x 5 fine-tuning grid: the reference's one interpolate call
    want = F.interpolate(enc["pos_embed"].permute(0, 3, 1, 2), size=(5, 5), mode="bicubic", antialias=True).permute(0, 2, 3, 1)
    assert sd[PRE + "pos_embed"].shape == (1, 5, 5, 128)
    assert float((sd[PRE + "pos_embed"] - want).abs().max()) <= 1e-6
    assert float((want - enc["pos_embed"][:, :5, :5]).abs().max()) > 1e-2      # (a crop would not do)
    w = model.net.plan.patch_lin
    assert torch.equal(model.net.Wb[w.w_off:][:128 * 768].cpu().view(128, 3, 16, 16), sd[PRE + "patch_embed.projection.weight"].to(torch.bfloat16))


def test_sam_checkpoint_refusals_name_the_key(stack_backend, tiny_sam, tmp_path):
    dev = stack_backend
    full = _sam_model_state()

    def refused(sd, match, name):
        torch.save(sd, str(tmp_path / name))
        with pytest.raises(ValueError, match=match):
            _tracker(dev, pretrained=True, backbone_checkpoint=str(tmp_path / name))

    refused({**full, "vision_encoder.layers.0.mlp.lin1.weight": torch.zeros(64, 128)}, r"vision_encoder\.layers\.0\.mlp\.lin1\.weight has shape", "w.pt")
    refused({**full, "vision_encoder.pos_embed": torch.zeros(1, 8, 6, 128)}, r"vision_encoder\.pos_embed has shape \(1, 8, 6, 128\)", "pos.pt")
    refused({**full, "vision_encoder.pos_embed": torch.zeros(1, 8, 8, 64)}, r"vision_encoder\.pos_embed has shape", "posc.pt")
    refused({**full, "vision_encoder.layers.1.attn.rel_pos_h": torch.zeros(127, 64)}, r"layers\.1\.attn\.rel_pos_h has shape \(127, 64\)", "rel.pt")
    from lightning_pose_amd.models.backbones.sam import load_sam_checkpoint, sam_seeded_state_dict
    init = sam_seeded_state_dict(*TINY, 5)
    assert set(init) == {PRE + k for k in _hf_encoder().state_dict()} and init[PRE + "pos_embed"].shape == (1, 5, 5, 128)
    torch.save({**full, "pooler.dense.weight": torch.zeros(4, 4)}, str(tmp_path / "extra.pt"))     # keys of other modules are ignored
    load_sam_checkpoint(str(tmp_path / "extra.pt"), init)
    assert all(torch.equal(init["backbone." + k], v) for k, v in full.items() if k.startswith("vision_encoder.") and not k.endswith("pos_embed"))
    assert set(init) == {PRE + k for k in _hf_encoder().state_dict()}


@pytest.mark.parametrize("precision", ["bf16-mixed", "fp32"])
def test_training_lowers_the_loss(stack_backend, tiny_sam, precision):
    from lightning_pose_amd.optim import FusedAdam
    from lightning_pose_amd.trainer import Trainer

    dev = stack_backend
    model = _tracker(dev, precision=precision)
    groups = model.get_parameters()
    assert [g["name"] for g in groups] == ["backbone", "head"] and groups[0]["lr"] == 0
    named = dict(model.named_parameters())
    bb = {id(p) for p in groups[0]["params"]}
    for n in (PRE + "pos_embed", PRE + "layers.0.attn.qkv.bias", PRE + "layers.2.mlp.lin2.weight", PRE + "patch_embed.projection.bias"):
        assert id(named[n]) in bb, n
    assert len(bb) + len(groups[1]["params"]) == len(named)
    assert not any("rel_pos" in n or ".neck." in n for n in named)
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
    pos0 = named[PRE + "pos_embed"].detach().cpu().clone()
    tr.training_batch(model, batch, 0)
    assert torch.equal(named[PRE + "pos_embed"].detach().cpu(), pos0)        # frozen backbone: lr 0
    for g in opt.param_groups:                                     # unfreeze the backbone (what UnfreezeBackbone does at its epoch)
        g["lr"] = 1e-3
    losses = [float(tr.training_batch(model, batch, i)) for i in range(1, 7)]
    assert all(l == l for l in losses) and losses[-1] < losses[0], losses
    assert (named[PRE + "pos_embed"].detach().cpu() - pos0).abs().max() > 1e-4
    assert (named[PRE + "layers.0.attn.qkv.bias"].detach().cpu()).abs().max() > 1e-4          # (zero at the start)


def test_lightning_style_ckpt_round_trip(stack_backend, tiny_sam, tmp_path):
    from lightning_pose_amd import checkpoint as ck
    from lightning_pose_amd.models import SemiSupervisedHeatmapTracker

    dev = stack_backend
    model = _tracker(dev, semi=True, torch_seed=1)
    with torch.no_grad():
        for k, v in model.state_dict().items():
            if "rel_pos" in k or ".neck." in k or k.endswith("pos_embed"):
                v.normal_(std=0.5)
    model.net.refresh_weight_copies()
    assert model.hparams["backbone"] == "vitb_sam" and model.hparams["image_size"] == SIDE
    path = ck.save_checkpoint(model, str(tmp_path / "sam.ckpt"), optimizer=model.configure_optimizers()["optimizer"])
    raw = torch.load(path, map_location="cpu", weights_only=False)
    for k in ("pos_embed", "layers.0.attn.rel_pos_h", "layers.1.attn.rel_pos_w", "neck.conv2.weight", "layers.2.mlp.lin2.weight"):
        assert PRE + k in raw["state_dict"], k
    again = ck.load_model_from_checkpoint(path, strict=True, loss_factory=model.loss_factory, loss_factory_unsupervised=model.loss_factory_unsup,
                                          device=dev)
    assert type(again) is SemiSupervisedHeatmapTracker and again.net.arch == "sam" and again.net.sam_grid == 5
    a, b = model.state_dict(), again.state_dict()
    assert set(a) == set(b) and all(torch.equal(a[k].cpu(), b[k].cpu()) for k in a)
    assert torch.equal(model.net.Wb.cpu(), again.net.Wb.cpu())
    # the backbone half loads strictly into the HF module itself (at the fine-tuning grid, as the reference's wrapper leaves it)
    _hf_encoder(grid=5).load_state_dict({k[len(PRE):]: v.cpu() for k, v in a.items() if k.startswith(PRE)}, strict=True)


# ---- golden step parity against the verbatim reference classes (tests/golden/step_sam.npz, made by tests/golden/make_golden_sam.py) ---------
def _to(d, dev):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in d.items()}


def _step_model(dev, precision):
    from lightning_pose_amd.losses import LossFactory
    from lightning_pose_amd.models import SemiSupervisedHeatmapTracker

    inp = make_step_inputs("sam", O.generate_heatmaps)
    cfg = inp["cfg"]
    sup = LossFactory({"heatmap_mse": {"log_weight": 0.0}}, None)
    pca = {"loss_name": "pca_singleview", "log_weight": PCA_LOG_WEIGHT, "components_to_keep": 0.99, "data_arr": inp["pca_fit"], "device": str(dev),
           "columns_for_singleview_pca": inp["cols"]}
    unsup = LossFactory({"temporal": dict(TEMPORAL), "pca_singleview": pca}, None)
    model = SemiSupervisedHeatmapTracker(num_keypoints=cfg["K"], loss_factory=sup, loss_factory_unsupervised=unsup, backbone="vitb_sam",
                                         pretrained=False, torch_seed=TORCH_SEED, device=dev, precision=precision, image_size=cfg["HW"])
    model.total_unsupervised_importance = torch.tensor(1.0)
    batch = {"labeled": _to(inp["batch"]["labeled"], dev), "unlabeled": _to(inp["batch"]["unlabeled"], dev)}
    return model, batch, inp


def _run_sam(name, dev, precision, g):
    """tests/test_step_parity.py::_run for this model: the same seeded inputs, backbone draw and trained head, at the step's image size"""
    assert name == "sam"
    model, batch, inp = _step_model(dev, precision)
    sd = model.state_dict()
    assert set(sd) == {str(n) for n in g["state_dict_names"]}
    for k in [k for k in g if k.startswith("head/")]:
        sd["head." + k[len("head/"):]] = g.t(k).to(dev)
    new = seeded_backbone_weights({k: v.cpu() for k, v in sd.items()})
    assert sorted(new) == [str(n) for n in g["backbone_names"]], "backbone tensor names differ from the reference's SamVisionEncoder"
    sd.update({k: v.to(dev) for k, v in new.items()})
    model.load_state_dict(sd)
    # what the reference never gives a gradient (rel_pos_*, neck.*) is exactly what is carried here as buffers
    assert {str(n) for n in g["no_grad_names"]} == {n for n, _ in model.named_buffers()}
    seen = {}
    for meth in ("get_loss_inputs_labeled", "get_loss_inputs_unlabeled"):
        orig = getattr(model, meth)

        def wrapped(batch_dict, _orig=orig, _m=meth):
            d = _orig(batch_dict)
            seen[_m] = {k: (v.detach().float().cpu() if torch.is_tensor(v) else v) for k, v in d.items()}
            return d
        setattr(model, meth, wrapped)
    model.train()
    opt = model.configure_optimizers()["optimizer"]
    opt.zero_grad()
    out = model.training_step(batch, 0)
    out["loss"].backward()
    return model, out, seen, inp


@pytest.mark.parametrize("precision", ["fp32", "bf16-mixed"])
def test_golden_step_parity_against_the_verbatim_classes(stack_backend, golden, monkeypatch, precision):
    """one semi-supervised step (heatmap_mse + temporal + pca_singleview, 96-px frames, window 4 on a 6 x 6 grid, 4 + 6 frames) against the
    reference's own class: every logged scalar, the total loss, keypoints, confidences, heat-maps and gradients through
    tests/test_step_parity.py's checker at its TOL, unchanged"""
    from lightning_pose_amd.models.backbones import factory as bf
    from tests import test_step_parity as sp

    monkeypatch.setitem(bf.SAM_CONFIGS, "vitb_sam", SAM_VIT)
    monkeypatch.setattr(sp, "_run", _run_sam)
    sp._check("sam", stack_backend, precision, golden("step_sam"))


def test_live_forward_against_the_reference_class(monkeypatch):
    """CPU only (the emulated fp32 executor), where the reference tree is present: the reference's own tracker, built as
    tests/golden/make_golden_sam.py builds it, and the product from the same state dict give the same heat-maps"""
    from oracle import ref_loader
    if not ref_loader.available() or not __import__("os").path.exists(__import__("os").path.join(
            ref_loader.REFERENCE_ROOT, "lightning_pose", "models", "backbones", "vit_sam.py")):
        pytest.skip("the reference tree (with models/backbones/vit_sam.py) is not present")
    from lightning_pose_amd import _lib, ops
    from lightning_pose_amd.models.backbones import factory as bf
    from tests.golden.make_golden_sam import build_reference_tracker
    from tests.hipemu import emu

    monkeypatch.setattr(_lib, "_lib", emu.emu_lib())
    monkeypatch.setattr(ops, "require_device", lambda *a: None)
    monkeypatch.setattr(ops, "require_device_type", lambda d: None)
    monkeypatch.setattr(ops, "_stream", lambda: None)
    ops._device_tables.cache_clear()
    monkeypatch.setitem(bf.SAM_CONFIGS, "vitb_sam", SAM_VIT)
    saved = transformers.SamModel.from_pretrained
    try:
        ref, _, sd_names, _ = build_reference_tracker(make_step_inputs("sam", O.generate_heatmaps))
    finally:
        transformers.SamModel.from_pretrained = saved
    model, batch, _ = _step_model(torch.device("cpu"), "fp32")
    assert set(model.state_dict()) == set(sd_names)
    model.load_state_dict({k: v.detach().clone() for k, v in ref.state_dict().items()}, strict=True)
    ref.eval()
    model.eval()
    with torch.no_grad():
        want = ref(batch["labeled"]["images"])
        got = model(batch["labeled"]["images"])
    torch.testing.assert_close(got, want, atol=1e-6, rtol=1e-4)
    ops._device_tables.cache_clear()
