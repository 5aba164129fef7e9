"""HeatmapTrackerMultiviewTransformer / SemiSupervisedHeatmapTrackerMultiviewTransformer (model_type "heatmap_multiview_transformer")
through the registry surface: classes, constructor errors, state_dict, parameter groups, output dicts, and a short training run under
Trainer + FusedAdam with its three parameter groups.  A 2-layer / 2-head ViT of width 128 stands in for ViT-S (tests/test_emu_vit_engine.py)."""

import pytest
import torch

from oracle import restated as O
from tests.golden.step_inputs import PCA_LOG_WEIGHT, TEMPORAL, make_step_inputs
from tests.golden.step_inputs_mvt import MVT_VIT

LABELED_KEYS = {"heatmaps_targ", "heatmaps_pred", "keypoints_targ", "keypoints_pred", "confidences", "keypoints_targ_3d", "keypoints_pred_3d",
                "keypoints_pred_2d_reprojected"}
UNLABELED_KEYS = {"heatmaps_pred", "keypoints_pred", "keypoints_pred_augmented", "confidences"}


@pytest.fixture
def small_vit(monkeypatch):
    from lightning_pose_amd.models.backbones import factory as bf
    monkeypatch.setitem(bf.VIT_CONFIGS, "vits_dino", MVT_VIT)
    monkeypatch.setitem(bf._IMPLEMENTED, "vits_dino", MVT_VIT[0])


def _to(d, dev):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in d.items()}


def _model(dev, semi=True, precision="bf16-mixed", **kw):
    from lightning_pose_amd.losses import LossFactory
    from lightning_pose_amd.models import get_model_class

    inp = make_step_inputs("mvt", O.generate_heatmaps)
    cfg = inp["cfg"]
    sup = LossFactory({"heatmap_mse": {"log_weight": 0.0}}, None)
    args = dict(num_keypoints=cfg["K"], num_views=cfg["V"], loss_factory=sup, backbone="vits_dino", pretrained=False, torch_seed=0, device=dev,
                precision=precision, optimizer_params={"learning_rate": 1e-3})
    if semi:
        pca = {"loss_name": "pca_multiview", "log_weight": PCA_LOG_WEIGHT, "components_to_keep": 3, "data_arr": inp["pca_fit"], "device": str(dev),
               "mirrored_column_matches": inp["mcm"]}
        args["loss_factory_unsupervised"] = LossFactory({"temporal": dict(TEMPORAL), "pca_multiview": pca}, None)
    args.update(kw)
    model = get_model_class("heatmap_multiview_transformer", semi)(**args)
    batch = {"labeled": _to(inp["batch"]["labeled"], dev), "unlabeled": _to(inp["batch"]["unlabeled"], dev)}
    return model, batch, cfg


def test_registry_returns_the_two_classes():
    from lightning_pose_amd import models
    from lightning_pose_amd.models import get_model_class
    from lightning_pose_amd.models.base import SemiSupervisedTrackerMixin
    from lightning_pose_amd.models.heatmap_tracker_multiview import HeatmapTrackerMultiviewTransformer as A
    from lightning_pose_amd.models.heatmap_tracker_multiview import SemiSupervisedHeatmapTrackerMultiviewTransformer as B

    assert get_model_class("heatmap_multiview_transformer", False) is A is models.HeatmapTrackerMultiviewTransformer
    assert get_model_class("heatmap_multiview_transformer", True) is B is models.SemiSupervisedHeatmapTrackerMultiviewTransformer
    assert issubclass(B, A) and issubclass(B, SemiSupervisedTrackerMixin) and A in models.ALLOWED_MODELS and B in models.ALLOWED_MODELS
    with pytest.raises(NotImplementedError):
        get_model_class("heatmap_mhcrnn", False)


def test_constructor_errors_match_the_reference(stack_backend, small_vit):
    from lightning_pose_amd.losses import LossFactory
    dev = stack_backend
    with pytest.raises(ValueError, match="HeatmapTrackerMultiviewTransformer does not currently support context frames"):
        _model(dev, do_context=False)
    with pytest.raises(ValueError, match=r'backbone "resnet50" is not supported for multiview transformer models; allowed backbones: \['
                                         r"'vits_dino', 'vitb_dino'\]"):
        _model(dev, backbone="resnet50")
    for out_of_scope in ("vits_dinov2", "vitb_dinov3", "vitb_imagenet"):     # the reference's list, not this package's: both exception types
        with pytest.raises(NotImplementedError, match="is not supported for multiview transformer models"):
            _model(dev, backbone=out_of_scope)
        with pytest.raises(ValueError, match="allowed backbones"):
            _model(dev, backbone=out_of_scope)
    with pytest.raises(NotImplementedError, match="heatmap_mlp is not a valid multiview transformer head"):
        _model(dev, head="heatmap_mlp")
    with pytest.raises(TypeError):                                           # num_views is required
        from lightning_pose_amd.models import HeatmapTrackerMultiviewTransformer
        HeatmapTrackerMultiviewTransformer(num_keypoints=3, backbone="vits_dino", pretrained=False, device=dev)
    calibrated = LossFactory({"heatmap_mse": {"log_weight": 0.0}}, None)
    calibrated.loss_instance_dict["supervised_pairwise_projections"] = object()
    with pytest.raises(NotImplementedError, match="supervised_pairwise_projections"):
        _model(dev, loss_factory=calibrated)


def test_state_dict_parameter_groups_and_output_dicts(stack_backend, small_vit):
    from lightning_pose_amd.models.factory import _produced_keys, _validate_loss_model_compatibility

    dev = stack_backend
    model, batch, cfg = _model(dev)
    K, V, D = cfg["K"], cfg["V"], MVT_VIT[0]
    assert model.num_views == V and model.rmse_loss is not None and model.head is not None
    sd = model.state_dict()
    assert list(sd)[0] == "view_embeddings" and sd["view_embeddings"].shape == (V, D) and isinstance(model.view_embeddings, torch.nn.Parameter)
    assert float(model.view_embeddings.detach().std()) == pytest.approx(0.02, rel=0.2)
    assert sd["backbone.vision_encoder.embeddings.cls_token"].shape == (1, 1, D)
    assert sd["backbone.vision_encoder.embeddings.position_embeddings"].shape == (1, 1 + MVT_VIT[5] ** 2, D)
    assert sd["head.upsampling_layers.1.weight"].shape == (D // 4, K, 3, 3)
    assert all(k == "view_embeddings" or k.startswith(("backbone.vision_encoder.", "head.upsampling_layers.")) for k in sd)
    assert set(sd) == set(model.net.state_dict())
    groups = model.get_parameters()
    assert [g["name"] for g in groups] == ["backbone", "head", "view_embeddings"]
    assert groups[0]["lr"] == 0.0 and "lr" not in groups[1] and "lr" not in groups[2]
    assert len(groups[2]["params"]) == 1 and groups[2]["params"][0] is model.view_embeddings
    n_named = len(list(model.named_parameters()))
    assert sum(len(list(g["params"])) for g in groups) == n_named
    assert model.hparams["num_views"] == V and model.hparams["head"] == "heatmap_cnn" and model.hparams["image_size"] == 256
    # the output dicts and their annotations
    model.eval()
    with torch.no_grad():
        lab = model.get_loss_inputs_labeled(batch["labeled"])
        unl = model.get_loss_inputs_unlabeled(batch["unlabeled"])
    assert set(lab) == LABELED_KEYS == _produced_keys(type(model).get_loss_inputs_labeled)
    assert set(unl) == UNLABELED_KEYS == _produced_keys(type(model).get_loss_inputs_unlabeled)
    assert lab["keypoints_targ_3d"] is None and lab["keypoints_pred_3d"] is None and lab["keypoints_pred_2d_reprojected"] is None
    Bl, S, h = cfg["Bl"], cfg["S"], cfg["HW"] // 4
    assert lab["heatmaps_pred"].shape == (Bl, V * K, h, h) and lab["keypoints_pred"].shape == (Bl, 2 * V * K) and lab["confidences"].shape == (Bl, V * K)
    assert unl["heatmaps_pred"].shape == (S, V * K, h, h) and unl["keypoints_pred_augmented"].shape == (S, 2 * V * K)
    _validate_loss_model_compatibility(type(model), {"supervised": model.loss_factory, "unsupervised": model.loss_factory_unsup})
    # predict_step: both batch forms
    for b in (batch["labeled"], batch["unlabeled"]):
        with torch.no_grad():
            kp, conf, hm = model.predict_step(b, 0, return_heatmaps=True)
        n = (b["images"] if "images" in b else b["frames"]).shape[0]
        assert kp.shape == (n, 2 * V * K) and conf.shape == (n, V * K) and hm.shape == (n, V * K, h, h)
    with torch.no_grad(), pytest.raises(ValueError, match="num_views"):
        model.forward(batch["labeled"]["images"][:, :2])


@pytest.mark.parametrize("precision", ["bf16-mixed", "fp32"])
def test_trains_through_the_reference_surface(stack_backend, small_vit, precision):
    """Trainer + FusedAdam on a fixed semi-supervised batch: the loss goes down, view_embeddings and the head move, the backbone stays
    bit-identical while its lr is 0 and moves once param_groups[0]["lr"] is set; zero_grad leaves usable gradients"""
    from lightning_pose_amd.trainer import Trainer

    dev = stack_backend
    model, batch, cfg = _model(dev, precision=precision)
    tr = Trainer(data_parallel=False)
    tr.setup(model)
    model.train()
    opt = model.optimizers()
    assert [g["name"] for g in opt.param_groups] == ["backbone", "head", "view_embeddings"]
    assert opt.param_groups[0]["lr"] == 0.0 and opt.param_groups[2]["lr"] == 1e-3
    pl = model.net.plan
    assert opt._ranges == {"backbone": (pl.n_view, pl.n_backbone), "head": (pl.n_backbone, pl.n_total), "view_embeddings": (0, pl.n_view)}
    before = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    losses = [float(tr.training_batch(model, batch, i)) for i in range(4)]
    assert all(l == l for l in losses) and losses[-1] < losses[0], losses
    after = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    assert not torch.equal(after["view_embeddings"], before["view_embeddings"])
    assert not torch.equal(after["head.upsampling_layers.1.weight"], before["head.upsampling_layers.1.weight"])
    for k in before:
        if k.startswith("backbone."):
            assert torch.equal(after[k], before[k]), k                      # lr 0: not a bit moves
    opt.param_groups[0]["lr"] = 1e-3                                         # what UnfreezeBackbone does
    tr.training_batch(model, batch, 4)
    moved = {k for k, v in model.state_dict().items() if k.startswith("backbone.") and not torch.equal(v.detach().cpu(), before[k])}
    assert "backbone.vision_encoder.layers.0.attention.q_proj.weight" in moved and "backbone.vision_encoder.embeddings.position_embeddings" in moved
    cls = "backbone.vision_encoder.embeddings.cls_token"
    assert cls not in moved                                                  # zero gradient, Adam: zero update
    opt.zero_grad()
    assert float(model.net.G.abs().sum()) == 0 and model.view_embeddings.grad is not None and not model.view_embeddings.grad.any()
    model.training_step(batch, 5)["loss"].backward()
    assert float(model.view_embeddings.grad.abs().sum()) > 0
    assert model.view_embeddings.grad.data_ptr() == model.net.G.data_ptr()   # the views of the flat buffer, still bound


def test_checkpoint_round_trip(stack_backend, small_vit, tmp_path):
    from lightning_pose_amd import checkpoint

    dev = stack_backend
    model, batch, cfg = _model(dev)
    path = checkpoint.save_checkpoint(model, str(tmp_path / "mvt.ckpt"))
    ck = checkpoint.read_checkpoint(path)
    assert "view_embeddings" in ck["state_dict"] and ck["hyper_parameters"]["num_views"] == cfg["V"]
    again = checkpoint.load_model_from_checkpoint(path, strict=True, device=dev, loss_factory=model.loss_factory,
                                                  loss_factory_unsupervised=model.loss_factory_unsup)
    assert type(again) is type(model)
    for k, v in model.state_dict().items():
        assert torch.equal(again.state_dict()[k].cpu(), v.cpu()), k


# ---- against the VERBATIM reference classes, live (build container only: needs the reference tree; never on the device) -------------------
def _reference_has_multiview() -> bool:
    import os
    from oracle import ref_loader
    # (the reference tree itself, not the copy of a few modules that ships to the device)
    return ref_loader.REFERENCE_ROOT != ref_loader._SHIPPED and os.path.exists(os.path.join(ref_loader._PKG, "models", "heatmap_tracker_multiview.py"))


@pytest.fixture
def emu_stack(monkeypatch):
    """the 'emu' branch of conftest's stack_backend: the product host stack on the CPU-emulated kernels"""
    from lightning_pose_amd import _lib, ops
    from tests.hipemu import emu

    monkeypatch.setattr(_lib, "_lib", emu.emu_lib())
    monkeypatch.setattr(ops, "require_device", lambda *a: None)
    monkeypatch.setattr(ops, "require_device_type", lambda d: None)
    monkeypatch.setattr(ops, "_stream", lambda: None)
    ops._device_tables.cache_clear()
    yield torch.device("cpu")
    ops._device_tables.cache_clear()


def _verbatim_class(monkeypatch):
    import sys
    import types

    import transformers
    from oracle import ref_loader as R

    R.install_stubs()
    cameras = types.ModuleType("lightning_pose.data.cameras")    # stand-in for the two imported names (calibration is out of scope)

    def _no_calibration(*a, **k):
        raise NotImplementedError("no camera calibration in this test")
    cameras.project_3d_to_2d = cameras.project_camera_pairs_to_3d = _no_calibration
    monkeypatch.setitem(sys.modules, "lightning_pose.data.cameras", cameras)
    hidden, depth, heads, mlp, patch, grid = MVT_VIT

    def _from_config(model_name, add_pooling_layer=False, **kw):   # no network: the architecture from its config (make_golden.py:531-539)
        c = transformers.ViTConfig(hidden_size=hidden, num_hidden_layers=depth, num_attention_heads=heads, intermediate_size=mlp,
                                   patch_size=patch, image_size=patch * grid, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
        return transformers.ViTModel(c, add_pooling_layer=add_pooling_layer)
    monkeypatch.setattr(transformers.ViTModel, "from_pretrained", staticmethod(_from_config))
    return R.load("models.heatmap_tracker_multiview").HeatmapTrackerMultiviewTransformer


@pytest.mark.reference
@pytest.mark.skipif(not _reference_has_multiview(), reason="needs the reference tree (build container only)")
def test_strict_round_trip_and_step_against_the_verbatim_class(emu_stack, small_vit, monkeypatch, tmp_path):
    """state_dict / .ckpt strict in both directions with the reference's own HeatmapTrackerMultiviewTransformer, the same parameter groups,
    and - on the same weights - its heat-maps and every parameter gradient from the fp32 executor at test_emu_vit_engine.py's fp32 bars"""
    pytest.importorskip("transformers")
    from lightning_pose_amd import checkpoint

    dev = emu_stack
    Ref = _verbatim_class(monkeypatch)
    mine, batch, cfg = _model(dev, semi=False, precision="fp32")
    ref = Ref(num_keypoints=cfg["K"], num_views=cfg["V"], backbone="vits_dino", pretrained=False, torch_seed=3, image_size=cfg["HW"])
    rsd, msd = ref.state_dict(), mine.state_dict()
    assert set(rsd) == set(msd) and all(rsd[k].shape == msd[k].shape for k in rsd)
    assert [g["name"] for g in ref.get_parameters()] == [g["name"] for g in mine.get_parameters()]
    assert [len(list(g["params"])) for g in ref.get_parameters()] == [len(list(g["params"])) for g in mine.get_parameters()]
    mine.load_state_dict(rsd, strict=True)                                   # reference -> product
    path = checkpoint.save_checkpoint(mine, str(tmp_path / "mvt.ckpt"))      # product -> .ckpt -> reference
    with torch.no_grad():
        for p in ref.parameters():
            p.zero_()
    ref.load_state_dict(torch.load(path, map_location="cpu")["state_dict"], strict=True)
    for k, v in rsd.items():
        assert torch.equal(ref.state_dict()[k], v) and torch.equal(mine.state_dict()[k].cpu(), v), k
    # one forward / backward on the same weights
    with torch.no_grad():
        ref.view_embeddings.mul_(25.0)                                       # (0.02 -> 0.5: the views must matter)
    mine.load_state_dict(ref.state_dict(), strict=True)
    images = batch["labeled"]["images"]
    ref.train()
    mine.train()
    want = ref(images.cpu())
    g = torch.randn(want.shape, generator=torch.Generator().manual_seed(5))
    (want * g).sum().backward()
    mine.net.zero_grad()
    heat = mine(images)
    (heat * g.to(dev)).sum().backward()
    torch.testing.assert_close(heat.detach().cpu(), want.detach(), atol=1e-6, rtol=1e-4)
    mgrads = {n: p.grad.detach().cpu() for n, p in mine.named_parameters()}
    for n, p in ref.named_parameters():
        gr = p.grad if p.grad is not None else torch.zeros_like(p)
        if gr.norm() < 1e-5:
            assert mgrads[n].norm() < 1e-5, n
            continue
        rel = ((mgrads[n].reshape(gr.shape) - gr).norm() / gr.norm()).item()
        assert rel < 1e-4, (n, rel)


# ---- golden step parity against the verbatim reference classes (tests/golden/step_mvt.npz, made by tests/golden/make_golden_mvt.py) -------
def _run_mvt(name, dev, precision, g):
    """tests/test_step_parity.py::_run for this model: the same seeded inputs, backbone draw, view embeddings and trained head"""
    from tests.golden.make_golden_mvt import view_embeddings
    from tests.golden.step_inputs import TORCH_SEED, seeded_backbone_weights

    assert name == "mvt"
    model, batch, cfg = _model(dev, precision=precision, torch_seed=TORCH_SEED)
    model.total_unsupervised_importance = torch.tensor(1.0)
    sd = model.state_dict()
    assert set(sd) == {str(n) for n in g["state_dict_names"]}
    for k in [k for k in g if k.startswith("head/")]:
        sd["head." + k[len("head/"):]] = g.t(k).to(dev)
    new = seeded_backbone_weights({k: v.cpu() for k, v in sd.items()})
    assert sorted(new) == [str(n) for n in g["backbone_names"]], "backbone tensor names differ from the reference's ViTModel"
    sd.update({k: v.to(dev) for k, v in new.items()})
    sd["view_embeddings"] = view_embeddings(cfg["V"], MVT_VIT[0]).to(dev)
    model.load_state_dict(sd)
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
    return model, out, seen, make_step_inputs("mvt", O.generate_heatmaps)


@pytest.mark.parametrize("precision", ["fp32", "bf16-mixed"])
def test_golden_step_parity_against_the_verbatim_classes(stack_backend, small_vit, golden, monkeypatch, precision):
    """one semi-supervised step (heatmap_mse + temporal + pca_multiview, 3 views, 2 + 3 samples) against the reference's own class: every
    logged scalar, the total loss, keypoints, confidences, heat-maps and gradients through tests/test_step_parity.py's checker - the fp32
    executor at its TOL["fp32"], bf16-mixed at TOL_S64_BF16, the bars of the emulator-sized fixture"""
    from tests import test_step_parity as sp

    monkeypatch.setattr(sp, "_run", _run_mvt)
    monkeypatch.setitem(sp.TOL, "bf16-mixed", sp.TOL_S64_BF16)
    sp._check("mvt", stack_backend, precision, golden("step_mvt"))
