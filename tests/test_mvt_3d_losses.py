"""The calibrated 3-D supervised losses of the multi-view transformer tracker: PairwiseProjectionsLoss / ReprojectionHeatmapLoss against the
VERBATIM reference classes, the tracker's three 3-D output keys on a calibrated batch, a training step with both losses, and the loss
factories with and without ``data.camera_params_file``."""

import pytest
import torch
import transformers  # noqa: F401  (first import probes for torchvision: before oracle.ref_loader puts its stand-in module in its place)

from oracle import restated as OR
from tests import cameras_fp64 as O
from tests.conftest import needs_reference
from tests.golden.step_inputs_mvt import MVT_VIT

K, V, HW, BL = 2, 3, 64, 2


@pytest.fixture
def small_vit(monkeypatch):
    from lightning_pose_amd.models.backbones import factory as bf
    monkeypatch.setitem(bf.VIT_CONFIGS, "vits_dino", MVT_VIT)
    monkeypatch.setitem(bf._IMPLEMENTED, "vits_dino", MVT_VIT[0])


def test_the_camera_module_and_the_loss_classes_exist():
    """(fails on the tree before this feature: no data/cameras.py, neither loss registered)"""
    from lightning_pose_amd.data import cameras
    from lightning_pose_amd.data.bboxes import frame_to_model_batch  # noqa: F401
    from lightning_pose_amd.data.datatypes import MultiviewHeatmapLabeledBatchDict
    from lightning_pose_amd.losses.factory import get_loss_classes
    from lightning_pose_amd.losses.losses import PairwiseProjectionsLoss, ReprojectionHeatmapLoss

    assert callable(cameras.project_camera_pairs_to_3d) and callable(cameras.project_3d_to_2d)
    assert {"keypoints_3d", "intrinsic_matrix", "extrinsic_matrix", "distortions"} <= set(MultiviewHeatmapLabeledBatchDict.__annotations__)
    classes = get_loss_classes()
    assert classes["supervised_pairwise_projections"] is PairwiseProjectionsLoss
    assert classes["supervised_reprojection_heatmap_mse"] is ReprojectionHeatmapLoss


def test_losses_raise_the_reference_errors_without_calibration():
    from lightning_pose_amd.losses.losses import PairwiseProjectionsLoss, ReprojectionHeatmapLoss

    with pytest.raises(ValueError, match="3D keypoints not available for train stage. Camera params file is required but not found;"
                                         "Turn off supervised_pairwise_projections loss to avoid this error."):
        PairwiseProjectionsLoss()(keypoints_targ_3d=None, keypoints_pred_3d=None, stage="train")
    with pytest.raises(ValueError, match="Reprojected keypoints not available for val stage. Camera params file is required but not found;"
                                         "Turn off supervised_reprojection_heatmap loss to avoid this error."):
        ReprojectionHeatmapLoss(64, 64, 16, 16)(heatmaps_targ=torch.zeros(1, 1, 16, 16), keypoints_pred_2d_reprojected=None, stage="val")


def test_14_distortion_parameters_need_a_zero_tilt(stack_backend):
    from lightning_pose_amd.data.cameras import project_3d_to_2d

    f = {k: v.float().to(stack_backend) for k, v in O.fly_fixture().items()}
    d14 = torch.nn.functional.pad(f["distortions"], (0, 9))
    same = project_3d_to_2d(f["points_3d"], f["intrinsics"], f["extrinsics"], d14)
    assert torch.equal(same, project_3d_to_2d(f["points_3d"], f["intrinsics"], f["extrinsics"], f["distortions"]))
    d14[0, 1, 13] = 0.01
    with pytest.raises(NotImplementedError, match="tilted"):
        project_3d_to_2d(f["points_3d"], f["intrinsics"], f["extrinsics"], d14)
    with pytest.raises(ValueError, match="4, 5, 8, 12 or 14"):
        project_3d_to_2d(f["points_3d"], f["intrinsics"], f["extrinsics"], d14[..., :6])


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


@needs_reference
@pytest.mark.reference
@pytest.mark.parametrize("case", ["plain", "nan_pred", "nan_targ", "nothing_valid"])
def test_pairwise_loss_against_the_reference_class(stack_backend, case):
    from lightning_pose_amd.losses.losses import PairwiseProjectionsLoss
    from oracle import ref_loader

    R = ref_loader.load("losses.losses")
    g = torch.Generator().manual_seed(3)
    targ, pred = torch.randn(3, 5, 3, generator=g), torch.randn(3, 6, 5, 3, generator=g)
    pred[1, 2, 3] = targ[1, 3]                     # a distance of exactly 0: gradient 0
    if case == "nan_pred":
        pred[0, 1, 2, 0] = float("nan")
        pred[2, :, 4] = float("nan")
    elif case == "nan_targ":
        targ[1, 0, 1] = float("nan")
    elif case == "nothing_valid":
        targ[:] = float("nan")
    want_p = pred.clone().requires_grad_(True)
    want, want_logs = R.PairwiseProjectionsLoss(log_weight=1.0)(keypoints_targ_3d=targ, keypoints_pred_3d=want_p, stage="train")
    want.backward()
    got_p = pred.to(stack_backend).requires_grad_(True)
    mine = PairwiseProjectionsLoss(log_weight=1.0)
    got, logs = mine(keypoints_targ_3d=targ.to(stack_backend), keypoints_pred_3d=got_p, stage="train")
    got.backward()
    assert [l["name"] for l in logs] == [l["name"] for l in want_logs] and float(mine.weight) == pytest.approx(float(want_logs[1]["value"]))
    assert not torch.isnan(got_p.grad).any()
    if case == "nothing_valid":
        assert float(got.detach()) == 0.0 == float(want.detach()) and not got_p.grad.any()
        return
    assert abs(float(got.detach()) - float(want.detach())) <= 1e-5 * abs(float(want.detach()))
    ref_grad = torch.nan_to_num(want_p.grad, nan=0.0)     # (the reference's masked entries carry 0, or NaN through norm'(0): both "no gradient")
    assert _rel(got_p.grad.cpu(), ref_grad) <= 1e-5


@needs_reference
@pytest.mark.reference
@pytest.mark.parametrize("case", ["plain", "nan_keypoint", "zero_target", "all_zero_targets"])
def test_reprojection_loss_against_the_reference_class(stack_backend, case):
    from lightning_pose_amd.losses.losses import ReprojectionHeatmapLoss
    from oracle import ref_loader

    R = ref_loader.load("losses.losses")
    g = torch.Generator().manual_seed(4)
    kp_t = torch.rand(2, 6, 2, generator=g) * 56 + 4
    kp = (kp_t + 3 * torch.randn(2, 6, 2, generator=g)).clamp(2, 62)
    targ = OR.generate_heatmaps(kp_t, 64, 64, (16, 16))
    if case == "nan_keypoint":
        kp[0, 2] = float("nan")
    elif case == "zero_target":
        targ[1, 3] = 0.0
    elif case == "all_zero_targets":
        targ[:] = 0.0
    args = dict(original_image_height=64, original_image_width=64, downsampled_image_height=16, downsampled_image_width=16, log_weight=0.5)
    want_k = kp.clone().requires_grad_(True)
    want, want_logs = R.ReprojectionHeatmapLoss(**args)(heatmaps_targ=targ, keypoints_pred_2d_reprojected=want_k, stage="train")
    want.backward()
    got_k = kp.to(stack_backend).requires_grad_(True)
    got, logs = ReprojectionHeatmapLoss(**args)(heatmaps_targ=targ.to(stack_backend), keypoints_pred_2d_reprojected=got_k, stage="train")
    got.backward()
    assert [l["name"] for l in logs] == [l["name"] for l in want_logs]
    got_v, want_v = float(got.detach()), float(want.detach())
    print(f"{case}: loss {got_v:.8g} reference {want_v:.8g}")
    assert not torch.isnan(got_k.grad).any()
    assert abs(got_v - want_v) <= 1e-5 * max(abs(want_v), 1e-30)
    fin = torch.isfinite(want_k.grad)             # (a NaN keypoint: the reference's autograd leaves NaN there; this package passes no gradient)
    assert not got_k.grad.cpu()[~fin].any()
    if case == "all_zero_targets":
        assert got_v == 0.0 and not got_k.grad.any()
    else:
        assert _rel(got_k.grad.cpu()[fin], want_k.grad[fin]) <= 1e-5


# ---- the tracker -----------------------------------------------------------------------------------------------------------------
def _calibrated_batch(dev, calibrated=True):
    g = torch.Generator().manual_seed(11)
    rig = O.make_rig(BL, V, K, 5, seed=21)
    kp = torch.rand(BL, V * K, 2, generator=g) * (HW - 16) + 8
    batch = {"images": torch.randn(BL, V, 3, HW, HW, generator=g), "keypoints": kp.reshape(BL, -1),
             "heatmaps": OR.generate_heatmaps(kp, HW, HW, (HW // 4, HW // 4)), "bbox": rig["bbox"].float(),
             "num_views": torch.full((BL,), V), "idxs": torch.arange(BL)}
    if calibrated:
        batch.update(keypoints_3d=rig["points_3d"].float(), intrinsic_matrix=rig["intrinsics"].float(),
                     extrinsic_matrix=rig["extrinsics"].float(), distortions=rig["distortions"].float())
    else:   # what the reference's dataset hands over without a calibration file: (B, 1) placeholders
        batch.update(keypoints_3d=torch.zeros(BL, 1), intrinsic_matrix=torch.zeros(BL, 1), extrinsic_matrix=torch.zeros(BL, 1),
                     distortions=torch.zeros(BL, 1))
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in batch.items()}


def _factory(with_3d):
    from lightning_pose_amd.losses import LossFactory

    p = {"heatmap_mse": {"log_weight": 0.0}}
    if with_3d:
        p["supervised_pairwise_projections"] = {"log_weight": 0.5}
        p["supervised_reprojection_heatmap_mse"] = {"log_weight": 0.5, "original_image_height": HW, "original_image_width": HW,
                                                    "downsampled_image_height": HW // 4, "downsampled_image_width": HW // 4}
    return LossFactory(p, None)


def _model(dev, factory, precision="bf16-mixed"):
    from lightning_pose_amd.models import get_model_class

    return get_model_class("heatmap_multiview_transformer", False)(
        num_keypoints=K, num_views=V, loss_factory=factory, backbone="vits_dino", pretrained=False, torch_seed=0, device=dev,
        precision=precision, optimizer_params={"learning_rate": 1e-3})


def test_constructor_accepts_this_packages_loss_instances(stack_backend, small_vit):
    """(fails on the tree before this feature: the constructor raised NotImplementedError for these names)"""
    from lightning_pose_amd.losses.losses import PairwiseProjectionsLoss

    model = _model(stack_backend, _factory(True))
    assert type(model.loss_factory.loss_instance_dict["supervised_pairwise_projections"]) is PairwiseProjectionsLoss

    class Other(PairwiseProjectionsLoss):      # a subclass is not this package's class: its inputs are not known to be the kernels'
        pass

    f = _factory(True)
    f.loss_instance_dict["supervised_pairwise_projections"] = Other()
    with pytest.raises(NotImplementedError, match="supervised_pairwise_projections"):
        _model(stack_backend, f)


@pytest.mark.parametrize("precision", ["bf16-mixed", "fp32"])
def test_tracker_on_a_calibrated_batch(stack_backend, small_vit, precision):
    dev = stack_backend
    batch = _calibrated_batch(dev)
    P = V * (V - 1) // 2
    grads = {}
    for with_3d in (True, False):
        model = _model(dev, _factory(with_3d), precision)
        model.train()
        opt = model.configure_optimizers()["optimizer"]
        opt.zero_grad()
        if with_3d:
            with torch.no_grad():
                out = model.get_loss_inputs_labeled(batch)
            assert out["keypoints_targ_3d"].shape == (BL, K, 3) and out["keypoints_pred_3d"].shape == (BL, P, K, 3)
            assert out["keypoints_pred_2d_reprojected"].shape == (BL, V * K, 2)
            assert torch.isfinite(out["keypoints_pred_3d"]).all() and torch.isfinite(out["keypoints_pred_2d_reprojected"]).all()
            # ... and they are the oracle's values for the predicted keypoints
            pts = out["keypoints_pred"].reshape(BL, V, K, 2).double().cpu()
            rig = [batch[k].double().cpu() for k in ("intrinsic_matrix", "extrinsic_matrix", "distortions")]
            w3, w2 = O.chain(pts, *rig, batch["bbox"].double().cpu(), HW, HW)
            assert _rel(out["keypoints_pred_3d"].double().cpu(), w3) < 1e-4
            assert _rel(out["keypoints_pred_2d_reprojected"].double().cpu(), w2.reshape(BL, V * K, 2)) < 1e-4
        loss = model.training_step(batch, 0)["loss"]
        loss.backward()
        assert torch.isfinite(loss).item()
        names = set(model.logged)
        assert ("train_supervised_pairwise_projections_loss" in names) == with_3d
        assert ("train_supervised_reprojection_heatmap_mse_loss" in names) == with_3d
        grads[with_3d] = {n: p.grad.detach().float().cpu().clone() for n, p in model.named_parameters()}
    for n, g in grads[True].items():
        assert torch.isfinite(g).all(), n
        # a parameter that takes a gradient at all takes another one with the two losses ([CLS] never does: no token attends from it)
        if grads[False][n].any():
            assert not torch.equal(g, grads[False][n]), n
    assert sum(bool(g.any()) for g in grads[False].values()) >= len(grads[False]) - 1


def test_reprojection_key_only_when_its_loss_is_configured(stack_backend, small_vit):
    from lightning_pose_amd.losses import LossFactory

    dev = stack_backend
    f = LossFactory({"heatmap_mse": {"log_weight": 0.0}, "supervised_pairwise_projections": {"log_weight": 0.0}}, None)
    model = _model(dev, f)
    with torch.no_grad():
        out = model.get_loss_inputs_labeled(_calibrated_batch(dev))
    assert out["keypoints_pred_3d"] is not None and out["keypoints_targ_3d"] is not None and out["keypoints_pred_2d_reprojected"] is None
    with torch.no_grad():
        out = model.get_loss_inputs_labeled(_calibrated_batch(dev, calibrated=False))
    assert out["keypoints_pred_3d"] is None and out["keypoints_targ_3d"] is None and out["keypoints_pred_2d_reprojected"] is None
    with pytest.raises(ValueError, match="3D keypoints not available for train stage"):
        model.train()
        model.training_step(_calibrated_batch(dev, calibrated=False), 0)


def test_loss_factories_follow_the_camera_params_file():
    from lightning_pose_amd.losses.factory import get_loss_factories
    from lightning_pose_amd.losses.losses import PairwiseProjectionsLoss, ReprojectionHeatmapLoss

    def cfg(model_type="heatmap_multiview_transformer", camera="calibration.toml", losses=None):
        return {"model": {"model_type": model_type, "heatmap_loss_type": "mse", "losses_to_use": []},
                "data": {"camera_params_file": camera, "image_resize_dims": {"height": 128, "width": 256}, "downsample_factor": 2},
                "losses": losses if losses is not None else {"supervised_pairwise_projections": {"log_weight": 0.5},
                                                             "supervised_reprojection_heatmap_mse": {"log_weight": 1.5}}}

    sup = get_loss_factories(cfg(), None)["supervised"].loss_instance_dict
    assert list(sup) == ["heatmap_mse", "supervised_pairwise_projections", "supervised_reprojection_heatmap_mse"]
    assert type(sup["supervised_pairwise_projections"]) is PairwiseProjectionsLoss and float(sup["supervised_pairwise_projections"].log_weight) == 0.5
    r = sup["supervised_reprojection_heatmap_mse"]
    assert type(r) is ReprojectionHeatmapLoss and float(r.log_weight) == 1.5
    assert (r.original_image_height, r.original_image_width, r.downsampled_image_height, r.downsampled_image_width) == (128, 256, 32, 64)
    for other in (cfg(camera=None), cfg(camera=""), cfg(model_type="heatmap"), cfg(losses={})):
        assert list(get_loss_factories(other, None)["supervised"].loss_instance_dict) == ["heatmap_mse"]
    only = get_loss_factories(cfg(losses={"supervised_pairwise_projections": {"log_weight": 0.0}, "supervised_reprojection_heatmap_mse": {}}), None)
    assert list(only["supervised"].loss_instance_dict) == ["heatmap_mse", "supervised_pairwise_projections"]


def test_the_3d_losses_are_annealed_like_every_non_heatmap_loss(stack_backend):
    f = _factory(True)
    dev = stack_backend
    g = torch.Generator().manual_seed(1)
    kp = torch.rand(1, 2, 2, generator=g) * 40 + 12
    hm = OR.generate_heatmaps(kp, HW, HW, (16, 16)).to(dev)
    kw = dict(heatmaps_targ=hm, heatmaps_pred=hm * 0.5, keypoints_targ_3d=torch.zeros(1, 2, 3, device=dev),
              keypoints_pred_3d=torch.ones(1, 1, 2, 3, device=dev), keypoints_pred_2d_reprojected=(kp + 2.0).to(dev))
    full, logs = f(stage="train", anneal_weight=1.0, **kw)
    none, _ = f(stage="train", anneal_weight=0.0, **kw)
    w = {l["name"]: float(l["value"]) for l in logs}
    assert float(none) == pytest.approx(w["train_heatmap_mse_loss_weighted"], rel=1e-6)
    assert float(full) == pytest.approx(sum(v for k, v in w.items() if k.endswith("_loss_weighted")), rel=1e-6)
    assert w["train_supervised_pairwise_projections_loss"] == pytest.approx(3 ** 0.5, rel=1e-6)
