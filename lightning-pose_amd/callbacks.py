"""AnnealWeight / UnfreezeBackbone / PatchMasking (reference: lightning_pose/callbacks.py:32-459): the callbacks that mutate
hot-path state.  Same constructor arguments and hook names, so they work under ``pl.Trainer`` and under
``lightning_pose_amd.trainer.Trainer``."""

from __future__ import annotations

import copy
import logging
import math
from typing import Any, Literal

import torch

from . import ops

logger = logging.getLogger(__name__)

try:  # pragma: no cover
    from lightning.pytorch.callbacks import Callback  # type: ignore
except Exception:  # noqa: BLE001
    class Callback:  # type: ignore[no-redef]
        pass


class AnnealWeight(Callback):
    """Linearly raise ``pl_module.<attr_name>`` from init_val to final_val, one increment per epoch after the freeze."""

    def __init__(self, attr_name: str, init_val: float = 0.0, increase_factor: float = 0.01, final_val: float = 1.0,
                 freeze_until_epoch: int = 0) -> None:
        super().__init__()
        self.attr_name, self.init_val, self.increase_factor = attr_name, init_val, increase_factor
        self.final_val, self.freeze_until_epoch = final_val, freeze_until_epoch

    def on_train_start(self, trainer: Any, pl_module: Any) -> None:
        setattr(pl_module, self.attr_name, torch.tensor(self.init_val))

    def on_train_epoch_start(self, trainer: Any, pl_module: Any) -> None:
        if pl_module.current_epoch > self.freeze_until_epoch:
            eff_epoch = pl_module.current_epoch - self.freeze_until_epoch
            setattr(pl_module, self.attr_name, torch.tensor(min(self.init_val + eff_epoch * self.increase_factor, self.final_val)))


class UnfreezeBackbone(Callback):
    """Backbone lr: 0 until the unfreeze epoch/step, then initial_ratio * head_lr, then x warm_up_ratio per epoch/step until
    it reaches the head lr.  Needs optimizer.param_groups == [backbone, head] (reference :79-196)."""

    def __init__(self, unfreeze_epoch: int | None = None, unfreeze_step: int | None = None, initial_ratio: float = 0.1,
                 warm_up_ratio: float = 1.5) -> None:
        assert (unfreeze_epoch is None) != (unfreeze_step is None), "Exactly one must be provided."
        self.unfreeze_epoch, self.unfreeze_step = unfreeze_epoch, unfreeze_step
        self.initial_ratio, self.warm_up_ratio = initial_ratio, warm_up_ratio
        self._warmed_up = False
        self._initial_lr = 0.0

    def on_train_batch_start(self, trainer: Any, pl_module: Any, batch: Any, batch_idx: int) -> None:
        if self._warmed_up:
            return
        optimizer = pl_module.optimizers()
        assert optimizer.param_groups[0]["name"] == "backbone"
        head_lr = optimizer.param_groups[1]["lr"]
        optimizer.param_groups[0]["lr"] = self._get_backbone_lr(pl_module.global_step, pl_module.current_epoch, head_lr)

    def _get_backbone_lr(self, current_step: int | None, current_epoch: int, upsampling_lr: float) -> float:
        assert not self._warmed_up
        thaw, now = (self.unfreeze_step, current_step) if self.unfreeze_step is not None else (self.unfreeze_epoch, current_epoch)
        if now < thaw:
            return 0.0
        if now == thaw:
            self._initial_lr = self.initial_ratio * upsampling_lr
            return self._initial_lr
        next_lr = min(self._initial_lr * self.warm_up_ratio ** (now - thaw), upsampling_lr)
        if next_lr == upsampling_lr:
            self._warmed_up = True
        return next_lr


class PatchMasker:
    """The masking curriculum of the multi-view transformer (reference :279-459): no masking before ``init_step``, then the fraction of
    16 x 16 patches zeroed in every view grows linearly from ``init_ratio`` to ``final_ratio`` at ``final_step`` and stays there.

    ``selection`` chooses WHICH patches go:

    * ``"device"`` (default): ``ops.patch_mask`` - choice and zeroing in one kernel launch, nothing read back.  Patch ``p`` of view ``v`` of
      sample ``b`` is masked when the rank of its Philox word (key = seed | step << 32, counter = (p, b * V + v)) is below the count, so
      every (step, sample, view) has a stream of its own.
    * ``"reference"``: the reference's draw - a ``torch.Generator`` on the images' device seeded ``patch_seed + step + 1000 b + 100 v`` and
      ``randperm(N)[:m]`` - bit for bit, for users who need its patch choice.  It keeps the reference's seed collisions (step 100 of
      (b, v) = (0, 0) draws what step 0 of (0, 1) drew; so do (0, 10) and (1, 0)), and costs one generator and one permutation per view on
      the host's side of the stream; the mask is assembled with tensor operations and the zeroing is the same kernel launch.
    """

    PATCH_SIZE = 16   # the reference's constant (ViT-S/16, ViT-B/16)

    def __init__(self, patch_mask_config: dict | None = None, patch_seed: int = 0,
                 selection: Literal["device", "reference"] = "device") -> None:
        if selection not in ("device", "reference"):
            raise ValueError(f"selection must be 'device' or 'reference', got {selection!r}")
        self.patch_seed = patch_seed
        self.selection = selection
        if patch_mask_config is None:
            patch_mask_config = {}
        self.patch_init_step = patch_mask_config.get("init_step", 700)
        self.patch_final_step = patch_mask_config.get("final_step", 5000)
        self.patch_init_ratio = patch_mask_config.get("init_ratio", 0.1)
        self.patch_final_ratio = patch_mask_config.get("final_ratio", 0.5)
        self.use_patch_masking = self.patch_final_ratio > 0.0   # enabled by a positive final ratio
        if self.use_patch_masking and patch_seed is None:
            logger.warning("patch_seed is None but patch masking is enabled; results may not be reproducible")

    def _schedule(self, step: int) -> tuple[float, float]:
        """(mask ratio, progress through the ramp in [0, 1]) at an enabled curriculum's ``step >= init_step``"""
        progress = min((step - self.patch_init_step) / (self.patch_final_step - self.patch_init_step), 1.0)
        return self.patch_init_ratio + progress * (self.patch_final_ratio - self.patch_init_ratio), progress

    def _reference_mask(self, images: torch.Tensor, step: int, n: int, count: int) -> torch.Tensor:
        b, v = images.shape[:2]
        chosen = []
        for bi in range(b):
            for vi in range(v):
                generator = torch.Generator(device=images.device)
                generator.manual_seed(self.patch_seed + step + bi * 1000 + vi * 100)
                chosen.append(torch.randperm(n, device=images.device, generator=generator)[:count])
        mask = torch.ones(b * v, n, device=images.device)
        mask.scatter_(1, torch.stack(chosen), 0.0)
        return mask.view(b, v, n)

    def apply_patch_masking(self, images: torch.Tensor, training_step: int = 0, is_training: bool = True) -> tuple[torch.Tensor, torch.Tensor]:
        """``images`` (B, V, C, H, W) -> (masked images, (B, V, N) mask of 1 = kept / 0 = masked).  Outside training, or while the schedule
        masks nothing, the images come back as they are (the same tensor) with a mask of ones."""
        batch_size, num_views, _, height, width = images.shape
        total_patches = (height // self.PATCH_SIZE) * (width // self.PATCH_SIZE)
        ratio = self._schedule(training_step)[0] if is_training and training_step >= self.patch_init_step else 0.0
        patches_to_mask = int(ratio * total_patches)
        if patches_to_mask <= 0:
            return images, torch.ones(batch_size, num_views, total_patches, device=images.device)
        if self.selection == "reference":
            given = self._reference_mask(images, training_step, total_patches, patches_to_mask)
            return ops.patch_mask(images, 0, patches_to_mask, self.PATCH_SIZE, mask=given)
        return ops.patch_mask(images, (self.patch_seed or 0, training_step), patches_to_mask, self.PATCH_SIZE)

    def apply_masking(self, images: torch.Tensor, training_step: int = 0, is_training: bool = True) -> tuple[torch.Tensor, torch.Tensor]:
        """``apply_patch_masking`` when enabled; otherwise the images and the reference's (B, V) dummy mask of ones"""
        if self.use_patch_masking:
            return self.apply_patch_masking(images, training_step, is_training)
        return images, torch.ones(images.shape[0], images.shape[1], device=images.device)

    def get_training_schedule_info(self, current_step: int) -> dict[str, Any]:
        ratio, progress, to_start, to_max = 0.0, 0.0, 0, 0
        if self.use_patch_masking:
            if current_step < self.patch_init_step:
                to_start, to_max = self.patch_init_step - current_step, self.patch_final_step - current_step
            else:
                ratio, progress = self._schedule(current_step)
                to_max = max(0, self.patch_final_step - current_step)
        return {"step": current_step, "mask_ratio": ratio, "curriculum_progress": f"{progress * 100:.1f}%",
                "steps_to_patch_masking": to_start, "steps_to_max_masking": to_max}

    def should_start_patch_masking(self, current_step: int) -> bool:
        return self.use_patch_masking and current_step == self.patch_init_step


class PatchMasking(Callback):
    """Apply the :class:`PatchMasker` curriculum to every training batch (reference :199-276).

    The batch rules are the reference's, literally: a dict is masked through its ``"images"`` entry, else its ``"frames"`` entry, else left
    alone (and ``pl_module`` is not touched); anything else is taken for the image tensor itself.  A semi-supervised batch
    ``{"labeled": ..., "unlabeled": ...}`` has neither key at its top level, so - as in the reference - it is NOT masked.  The dict entry is
    replaced by a new tensor, the original is never written; the mask is left on ``pl_module.current_patch_mask`` (nothing reads it)."""

    def __init__(self, patch_mask_config: dict | None = None, patch_seed: int = 0,
                 selection: Literal["device", "reference"] = "device") -> None:
        super().__init__()
        self.curriculum_masking = PatchMasker(patch_mask_config=patch_mask_config, patch_seed=patch_seed, selection=selection)

    def on_train_batch_start(self, trainer: Any, pl_module: Any, batch: Any, batch_idx: int) -> None:
        if not self.curriculum_masking.use_patch_masking:
            return
        key = None
        if isinstance(batch, dict):
            key = "images" if "images" in batch else "frames" if "frames" in batch else None
            if key is None:
                return
        images = batch if key is None else batch[key]
        masked, patch_mask = self.curriculum_masking.apply_patch_masking(images, training_step=trainer.global_step, is_training=True)
        if key is not None:
            batch[key] = masked
        pl_module.current_patch_mask = patch_mask

    def on_train_epoch_end(self, trainer: Any, pl_module: Any) -> None:
        if not self.curriculum_masking.use_patch_masking:
            return
        info = self.curriculum_masking.get_training_schedule_info(trainer.global_step)
        pl_module.log("patch_mask_ratio", info["mask_ratio"], on_step=False, on_epoch=True, prog_bar=True)


def _cfg_get(cfg: Any, key: str, default: Any = None) -> Any:
    try:
        return cfg[key]
    except (KeyError, TypeError, AttributeError):
        return getattr(cfg, key, default)


def get_patch_masking_callback(cfg: Any, steps_per_epoch: int | None = None) -> PatchMasking | None:
    """The ``PatchMasking`` callback a config asks for, under the reference's condition (``get_callbacks``, :718-726): the model is
    ``heatmap_multiview_transformer`` and ``training.patch_mask.final_ratio > 0``; ``None`` otherwise.  Its seed is
    ``training.rng_seed_model_pt``.  A schedule given in epochs (``init_epoch`` / ``final_epoch``) becomes steps as the reference's
    train.py:334-340 does, ``ceil(epoch * steps_per_epoch)``, on a copy: the caller's config is not changed."""
    training = _cfg_get(cfg, "training", {})
    if str(_cfg_get(_cfg_get(cfg, "model", {}), "model_type", "")) != "heatmap_multiview_transformer":
        return None
    schedule = _cfg_get(training, "patch_mask", None) or {}
    if not _cfg_get(schedule, "final_ratio", 0.0) > 0.0:
        return None
    schedule = {k: copy.deepcopy(schedule[k]) for k in schedule}
    if "init_epoch" in schedule:
        if steps_per_epoch is None:
            raise ValueError("training.patch_mask gives its schedule in epochs (init_epoch / final_epoch): steps_per_epoch is needed")
        schedule["init_step"] = math.ceil(schedule["init_epoch"] * steps_per_epoch)
        schedule["final_step"] = math.ceil(schedule["final_epoch"] * steps_per_epoch)
    return PatchMasking(patch_mask_config=schedule, patch_seed=_cfg_get(training, "rng_seed_model_pt", 0))
