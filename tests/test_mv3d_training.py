"""A batch of MultiviewHeatmapDataset (3-D augmented, built on the device) through one training step of the multi-view transformer tracker with
both calibrated 3-D losses: the producer's keys, shapes and devices are the ones the tracker reads."""

import pytest
import torch
import transformers  # noqa: F401  (first import probes for torchvision: before oracle.ref_loader puts its stand-in module in its place)

from tests.golden.step_inputs_mvt import MVT_VIT
from tests.test_mv3d_dataset import H, IDX, K, PARAMS, V, W, make_dataset, write_dataset


@pytest.fixture
def small_vit(monkeypatch):
    from lightning_pose_amd.models.backbones import factory as bf
    monkeypatch.setitem(bf.VIT_CONFIGS, "vits_dino", MVT_VIT)
    monkeypatch.setitem(bf._IMPLEMENTED, "vits_dino", MVT_VIT[0])


def _model(dev):
    """the small configuration of tests/test_mvt_3d_losses.py, at this dataset's image size"""
    from lightning_pose_amd.losses import LossFactory
    from lightning_pose_amd.models import get_model_class

    factory = LossFactory({"heatmap_mse": {"log_weight": 0.0}, "supervised_pairwise_projections": {"log_weight": 0.5},
                           "supervised_reprojection_heatmap_mse": {"log_weight": 0.5, "original_image_height": H, "original_image_width": W,
                                                                   "downsampled_image_height": H // 4, "downsampled_image_width": W // 4}}, None)
    return get_model_class("heatmap_multiview_transformer", False)(
        num_keypoints=K, num_views=V, loss_factory=factory, backbone="vits_dino", pretrained=False, torch_seed=0, device=dev,
        precision="bf16-mixed", optimizer_params={"learning_rate": 1e-3})


def test_one_training_step_on_the_datasets_batch(tmp_path, stack_backend, small_vit):
    write_dataset(str(tmp_path))
    ds = make_dataset(tmp_path, stack_backend)
    batch = ds.batch(IDX[:2], params=PARAMS[:2])
    assert ds.producer.last_plan["status"].tolist() == [0, 0]
    model = _model(stack_backend)
    model.train()
    model.configure_optimizers()["optimizer"].zero_grad()
    loss = model.training_step(batch, 0)["loss"]
    loss.backward()
    assert torch.isfinite(loss).item()
    logged = {k: float(v) for k, v in model.logged.items() if k.endswith("_loss")}
    print(logged)
    for name in ("train_heatmap_mse_loss", "train_supervised_pairwise_projections_loss", "train_supervised_reprojection_heatmap_mse_loss"):
        assert name in logged and logged[name] == logged[name] and abs(logged[name]) < float("inf"), name
    assert logged["train_supervised_pairwise_projections_loss"] > 0.0
    grads = {n: p.grad for n, p in model.named_parameters()}
    assert all(g is None or bool(torch.isfinite(g).all()) for g in grads.values())
    moving = sum(1 for g in grads.values() if g is not None and bool(g.any()))
    assert moving >= len(grads) - 1                      # ([CLS] takes none: no token attends from it)
