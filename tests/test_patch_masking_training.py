"""PatchMasking under Trainer.fit with the multi-view transformer tracker (the 2-layer ViT of tests/test_mvt_tracker.py, 3 views of 64 x 64 px:
16 patches per view): what training_step sees, what the module and the log keep, where the epoch-end hook runs."""

import torch

from tests.test_mvt_tracker import _model, small_vit  # noqa: F401  (the fixture that swaps ViT-S for the small configuration)

SCHEDULE = {"init_step": 1, "final_step": 2, "init_ratio": 0.25, "final_ratio": 0.5}


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _zeroed_patches(images: torch.Tensor) -> torch.Tensor:
    """(B, V) number of 16 x 16 patches that are zero in all channels"""
    b, v, c, h, w = images.shape
    blocks = images.detach().cpu().view(b, v, c, h // 16, 16, w // 16, 16)
    return (blocks == 0).all(dim=6).all(dim=4).all(dim=2).sum(dim=(2, 3))


class _Recorder:
    """placed after PatchMasking: sees the batch as training_step will"""

    def __init__(self):
        self.images, self.masks, self.epoch_ends = [], [], []

    def on_train_batch_start(self, trainer, pl_module, batch, batch_idx):
        self.images.append(batch["images"])
        self.masks.append(getattr(pl_module, "current_patch_mask", None))

    def on_train_epoch_end(self, trainer, pl_module):
        self.epoch_ends.append({"validations": len(trainer.validation_history), "scheduler_steps": trainer.scheduler.last_epoch,
                                "global_step": trainer.global_step})


def test_three_steps_of_the_curriculum_under_fit(stack_backend, small_vit):  # noqa: F811
    from lightning_pose_amd.callbacks import PatchMasking
    from lightning_pose_amd.trainer import Trainer

    dev = stack_backend
    model, batch, cfg = _model(dev, semi=False)
    labeled = batch["labeled"]
    source = labeled["images"]
    before = _bits(source).clone()
    n = (cfg["HW"] // 16) ** 2
    seen = []
    step = model.training_step
    model.training_step = lambda b, i: (seen.append(b["images"]), step(b, i))[1]
    recorder = _Recorder()
    trainer = Trainer(max_epochs=1, callbacks=[PatchMasking(dict(SCHEDULE), patch_seed=3), recorder], data_parallel=False, log_every_n_steps=1)
    assert trainer.global_step == 0
    trainer.fit(model, lambda epoch: (dict(labeled) for _ in range(3)), val_batches=lambda epoch: [dict(labeled)])
    assert trainer.global_step == model.global_step == 3
    # what training_step saw: 0, int(.25 N), int(.5 N) zeroed patches in every view of every sample
    assert len(seen) == 3 and all(a is b for a, b in zip(seen, recorder.images))
    for images, want in zip(seen, (0, int(0.25 * n), int(0.5 * n))):
        assert (_zeroed_patches(images) == want).all(), (_zeroed_patches(images), want)
    assert seen[0] is source and seen[1] is not source
    # the module's mask is the one of the batch: its zeros are the zero blocks, everything else is the source's bits
    for images, mask in zip(seen[1:], recorder.masks[1:]):
        assert mask.shape == (cfg["Bl"], cfg["V"], n) and mask.device == source.device
        side = cfg["HW"] // 16
        pixels = mask.cpu().view(cfg["Bl"], cfg["V"], 1, side, 1, side, 1).expand(-1, -1, 3, -1, 16, -1, 16).reshape(source.shape).bool()
        assert torch.equal(_bits(images), torch.where(pixels, before, torch.zeros_like(before)))
    assert model.current_patch_mask is recorder.masks[2]
    assert torch.equal(_bits(source), before)                                  # the source batch is unchanged
    losses = [rec["train_supervised_loss"] for rec in trainer.logged_history]
    assert len(losses) == 3 and all(torch.isfinite(torch.tensor(l)) for l in losses), losses
    # the epoch-end hook: once, after the epoch's validation and before the scheduler's step; it logged the ratio at step 3
    assert recorder.epoch_ends == [{"validations": 1, "scheduler_steps": 0, "global_step": 3}]
    assert trainer.scheduler.last_epoch == 1
    assert float(model.logged["patch_mask_ratio"]) == 0.5


def test_a_step_on_the_callbacks_batch_is_a_step_on_a_batch_masked_by_hand(stack_backend, small_vit):  # noqa: F811
    from lightning_pose_amd.callbacks import PatchMasking
    from lightning_pose_amd.trainer import Trainer

    dev = stack_backend
    model, batch, cfg = _model(dev, semi=False)
    labeled = batch["labeled"]
    trainer = Trainer(callbacks=[PatchMasking(dict(SCHEDULE), patch_seed=3)], data_parallel=False)
    trainer.setup(model)
    model.train()
    model.global_step = 2                                                      # half of the patches
    by_callback = dict(labeled)
    trainer._hook("on_train_batch_start", model, by_callback, 0)
    mask = model.current_patch_mask.cpu()
    assert ((mask == 0).sum(-1) == 8).all()
    by_hand = labeled["images"].clone()
    side = cfg["HW"] // 16
    for b, v, p in zip(*torch.nonzero(mask == 0, as_tuple=True)):
        y, x = int(p) // side * 16, int(p) % side * 16
        by_hand[b, v, :, y:y + 16, x:x + 16] = 0
    assert torch.equal(_bits(by_callback["images"]), _bits(by_hand))
    losses = []
    for images in (by_callback["images"], by_hand, labeled["images"]):
        model.optimizers().zero_grad()
        loss = model.training_step({**labeled, "images": images}, 0)["loss"]
        loss.backward()
        losses.append(loss.detach().cpu())
    assert torch.equal(losses[0], losses[1]) and torch.isfinite(losses[0])
    assert not torch.equal(losses[0], losses[2])                               # and masking matters to the model
