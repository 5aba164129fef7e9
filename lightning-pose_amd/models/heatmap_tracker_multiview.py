"""HeatmapTrackerMultiviewTransformer / SemiSupervisedHeatmapTrackerMultiviewTransformer (reference:
lightning_pose/models/heatmap_tracker_multiview.py:36-484) on the MI355X engine - ``model_type: heatmap_multiview_transformer``.

``images (B, V, 3, H, W)`` are flattened to ``(B * V, 3, H, W)`` (row ``b * V + v`` is view ``v``); the ViT's patch tokens - without
``[CLS]`` - get the learned ``view_embeddings[v]`` added and are attended over as ONE sequence of ``V * Np`` tokens per sample
(``forward_vit``, :143-223); the heat-map head runs per view and the maps come back as ``(B, V * K, h, w)``.  Constructor arguments,
attributes (``num_views``, ``view_embeddings``, ``head``, ``rmse_loss``), ``state_dict`` keys, parameter groups and the keys of the
``get_loss_inputs_*`` dicts are the reference's; underneath, the whole network is the multi-view mode of
:class:`lightning_pose_amd.vit_engine.ViTEngine` (``lp_vit_mv_tokens_fwd`` / ``_bwd`` for the token assembly, every other kernel shared with
the single-view ViT tracker), and decode / affine-undo / bounding-box maps are the fused decode of :class:`HeatmapTracker`.

Calibrated rigs: when the labeled batch carries ``keypoints_3d`` (last dimension 3) with ``intrinsic_matrix``, ``extrinsic_matrix`` and
``distortions``, ``get_loss_inputs_labeled`` triangulates the predicted keypoints from every camera pair (``keypoints_pred_3d``) and - when
``supervised_reprojection_heatmap_mse`` is configured - reprojects the mean of the pairs into every view in model px
(``keypoints_pred_2d_reprojected``): one launch forward and one backward (``ops.camera_chain``, ``csrc/cameras.hip``) in place of the
reference's Python loop over pairs and samples.  The batch dict is where this starts: the calibration-file loader (``CameraGroup``) is not part
of this package.

The ``PatchMasking`` curriculum the reference trains this model with is ``lightning_pose_amd.callbacks.PatchMasking``
(``callbacks.get_patch_masking_callback(cfg)`` builds it under the reference's condition).

Outside this path (each raises where a configuration asks for it):
* the DINOv2 / DINOv3 / MAE ("vitb_imagenet") backbones of the reference's multi-view list: ``vits_dino`` and ``vitb_dino`` are implemented.
"""

from __future__ import annotations

from typing import Any, Literal

import torch

from .. import ops
from ..data.bboxes import model_dims
from ..losses.losses import PairwiseProjectionsLoss, ReprojectionHeatmapLoss
from .backbones.factory import VIT_CONFIGS
from .base import SemiSupervisedTrackerMixin
from .datatypes import HeatmapTrackerMultiviewTransformerLabeledOutputsDict, HeatmapTrackerUnlabeledOutputsDict
from .heatmap_tracker import HeatmapTracker

# the reference's ALLOWED_TRANSFORMER_BACKBONES_MULTIVIEW (models/backbones/factory.py:82-90) ...
_REFERENCE_MULTIVIEW_BACKBONES = ("vits_dino", "vits_dinov2", "vits_dinov3", "vitb_dino", "vitb_dinov2", "vitb_dinov3", "vitb_imagenet")
# ... of which this package implements
ALLOWED_TRANSFORMER_BACKBONES_MULTIVIEW = tuple(b for b in _REFERENCE_MULTIVIEW_BACKBONES if b in VIT_CONFIGS)
_CALIBRATED_LOSSES = {"supervised_pairwise_projections": PairwiseProjectionsLoss, "supervised_reprojection_heatmap_mse": ReprojectionHeatmapLoss}


class BackboneNotImplementedError(NotImplementedError, ValueError):
    """a backbone the reference's multi-view transformer accepts and this package does not implement: the reference's ValueError for
    a backbone outside the allowed list, and a NotImplementedError for callers that tell the two apart"""


class HeatmapTrackerMultiviewTransformer(HeatmapTracker):
    """Transformer network that handles multi-view datasets."""

    def __init__(self, num_keypoints: int, num_views: int, loss_factory: Any = None, backbone: str = "vits_dino", pretrained: bool = True,
                 head: Literal["heatmap_cnn"] = "heatmap_cnn", downsample_factor: Literal[1, 2, 3] = 2, torch_seed: int = 123,
                 optimizer: str = "Adam", optimizer_params: Any = None, lr_scheduler: str = "multisteplr", lr_scheduler_params: Any = None,
                 image_size: int = 256, **kwargs: Any) -> None:
        if "do_context" in kwargs.keys():  # backwards compatibility (reference :77-81)
            raise ValueError("HeatmapTrackerMultiviewTransformer does not currently support context frames")
        allowed = list(ALLOWED_TRANSFORMER_BACKBONES_MULTIVIEW)
        if backbone not in allowed:
            message = f'backbone "{backbone}" is not supported for multiview transformer models; allowed backbones: {allowed}'
            if backbone in _REFERENCE_MULTIVIEW_BACKBONES:
                raise BackboneNotImplementedError(message + " (the DINOv2 / DINOv3 / MAE backbones are not implemented on the MI355X path)")
            raise ValueError(message)
        if head != "heatmap_cnn":
            raise NotImplementedError(f"{head} is not a valid multiview transformer head")
        if int(num_views) < 1:
            raise ValueError(f"num_views must be a positive number of camera views, got {num_views}")
        # the calibrated 3-D losses are this package's own classes (their inputs come from the fused geometry kernel); anything else under
        # those names - the reference's torch implementation, a stand-in - is refused rather than fed
        registered = getattr(loss_factory, "loss_instance_dict", {})
        asked = [n for n, cls in _CALIBRATED_LOSSES.items() if n in registered and type(registered[n]) is not cls]
        if asked:
            raise NotImplementedError(f"the calibrated 3-D supervised losses {asked} (camera projection) are outside the MI355X path unless they "
                                      "are lightning_pose_amd.losses.losses.PairwiseProjectionsLoss / ReprojectionHeatmapLoss")
        self.num_views = int(num_views)   # (read by _vit_engine_extras while HeatmapTracker.__init__ builds the engine)
        super().__init__(num_keypoints=num_keypoints, loss_factory=loss_factory, backbone=backbone, downsample_factor=downsample_factor,
                         pretrained=pretrained, torch_seed=torch_seed, optimizer=optimizer, optimizer_params=optimizer_params,
                         lr_scheduler=lr_scheduler, lr_scheduler_params=lr_scheduler_params, **kwargs)
        # (Lightning keeps the arguments of every __init__ of the hierarchy that calls this; these add num_views, head and image_size)
        self.save_hyperparameters(ignore=["loss_factory", "loss_factory_unsupervised"])

    def _vit_engine_extras(self, hidden: int) -> tuple[dict, dict]:
        # learnable view embeddings, 0.02 N(0, 1) from a generator of their own seeded with torch_seed (reference :111-119)
        generator = torch.Generator().manual_seed(self.torch_seed)
        return {"num_views": self.num_views}, {"view_embeddings": torch.randn(self.num_views, hidden, generator=generator) * 0.02}

    def _check_views(self, images: torch.Tensor) -> None:
        if images.dim() != 5 or images.shape[1] != self.num_views:
            raise ValueError(f"images must be (batch, num_views = {self.num_views}, channels, height, width), got {tuple(images.shape)}")

    def joint_forward(self, images_a: torch.Tensor, images_b: torch.Tensor) -> bool:
        """labeled + unlabeled samples in ONE pass: samples never attend to each other, so the joint pass computes what two calls do"""
        self._check_views(images_a)
        self._check_views(images_b)
        return super().joint_forward(images_a, images_b)

    def forward(self, images: torch.Tensor) -> torch.Tensor:
        """(B, V, 3, H, W) -> (B, V * K, h, w) (reference :225-248)."""
        parked = getattr(self, "_joint", None)
        if not (parked and id(images) in parked):
            self._check_views(images)
        return super().forward(images)

    def get_loss_inputs_labeled(self, batch_dict: dict) -> HeatmapTrackerMultiviewTransformerLabeledOutputsDict:
        """Predicted heat-maps and keypoints (frame px) and, for a calibrated batch, the 3-D keys (reference :250-314: ``None`` whenever the
        batch carries no calibration; the reprojection only when its loss is configured)."""
        out = super().get_loss_inputs_labeled(batch_dict)
        targ_3d = pred_3d = reprojected = None
        if "keypoints_3d" in batch_dict and batch_dict["keypoints_3d"].shape[-1] == 3:
            pred = out["keypoints_pred"]
            views = batch_dict["images"].shape[1]
            k = pred.shape[1] // 2 // views
            points = pred.reshape(-1, views, k, 2)
            rig = (batch_dict["intrinsic_matrix"].float(), batch_dict["extrinsic_matrix"].float(), batch_dict["distortions"].float())
            targ_3d = batch_dict["keypoints_3d"]
            if "supervised_reprojection_heatmap_mse" in getattr(self.loss_factory, "loss_instance_dict", {}):
                mh, mw = model_dims(batch_dict)
                pred_3d, reprojected = ops.camera_chain(points, *rig, batch_dict["bbox"], mh, mw)
                reprojected = reprojected.reshape(-1, views * k, 2)
            else:
                pred_3d = ops.camera_pairs_to_3d(points, *rig)
        return {**out, "keypoints_targ_3d": targ_3d, "keypoints_pred_3d": pred_3d, "keypoints_pred_2d_reprojected": reprojected}

    def get_parameters(self) -> list[dict]:
        """Order matters: UnfreezeBackbone requires group 0 = backbone, group 1 = head; view_embeddings follow (reference :352-367)."""
        return [
            {"params": list(self.backbone.parameters()), "name": "backbone", "lr": 0.0},
            {"params": list(self.head.parameters()), "name": "head"},
            {"params": [self.view_embeddings], "name": "view_embeddings"},
        ]


class SemiSupervisedHeatmapTrackerMultiviewTransformer(SemiSupervisedTrackerMixin, HeatmapTrackerMultiviewTransformer):
    """Semi-supervised HeatmapTrackerMultiviewTransformer that supports unsupervised losses."""

    def __init__(self, num_keypoints: int, num_views: int, loss_factory: Any = None, loss_factory_unsupervised: Any = None,
                 backbone: str = "vits_dino", pretrained: bool = True, head: Literal["heatmap_cnn"] = "heatmap_cnn",
                 downsample_factor: Literal[1, 2, 3] = 2, torch_seed: int = 123, optimizer: str = "Adam", optimizer_params: Any = None,
                 lr_scheduler: str = "multisteplr", lr_scheduler_params: Any = None, image_size: int = 256, **kwargs: Any) -> None:
        super().__init__(num_keypoints=num_keypoints, num_views=num_views, loss_factory=loss_factory, backbone=backbone,
                         pretrained=pretrained, head=head, downsample_factor=downsample_factor, torch_seed=torch_seed, optimizer=optimizer,
                         optimizer_params=optimizer_params, lr_scheduler=lr_scheduler, lr_scheduler_params=lr_scheduler_params,
                         image_size=image_size, **kwargs)
        self.loss_factory_unsup = loss_factory_unsupervised
        self.total_unsupervised_importance = torch.tensor(1.0)

    def get_loss_inputs_unlabeled(self, batch_dict: dict) -> HeatmapTrackerUnlabeledOutputsDict:
        pred_heatmaps = self.forward(batch_dict["frames"])
        transforms = batch_dict["transforms"]
        if transforms.dim() == 4:   # [num_views, 1, 2, 3] or [1, num_views, 2, 3] -> [num_views, 2, 3] (reference :452-459)
            if transforms.shape[1] == 1:
                transforms = transforms.squeeze(1)
            elif transforms.shape[0] == 1:
                transforms = transforms.squeeze(0)
        pred_keypoints_augmented, pred_keypoints, confidence = self._decode(
            pred_heatmaps, batch_dict, transforms, bool(batch_dict["is_multiview"]))
        return {
            "heatmaps_pred": pred_heatmaps,                          # if augmented, augmented heatmaps
            "keypoints_pred": pred_keypoints,                        # if augmented, original keypoints (frame px)
            "keypoints_pred_augmented": pred_keypoints_augmented,    # match pred_heatmaps (model px)
            "confidences": confidence,
        }
