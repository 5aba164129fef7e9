"""callbacks.PatchMasker / PatchMasking / get_patch_masking_callback: the reference's masking curriculum for the multi-view transformer
(lightning_pose/callbacks.py:199-459) with the patch choice and the zeroing in one kernel launch (ops.patch_mask).  The schedule, the
batch rules and the logging are checked against the behaviour the reference's own test classes pin, the images against the definition
(masked patches are zero blocks, everything else is the input's bits), and ``selection="reference"`` and the ``Trainer`` boundary against
the reference's verbatim classes."""

import copy
from unittest.mock import MagicMock

import pytest
import torch

from tests.conftest import needs_reference

CONFIG = {"init_step": 100, "final_step": 500, "init_ratio": 0.1, "final_ratio": 0.5}
STEPS = (50, 100, 300, 500, 700)
ZEROED = (0, 1, 4, 8, 8)       # int(ratio * 16) at STEPS: ratio 0, 0.1, 0.3, 0.5, 0.5


def _enabled(**kw):
    from lightning_pose_amd.callbacks import PatchMasking
    return PatchMasking(patch_mask_config=dict(CONFIG), patch_seed=42, **kw)


def _disabled():
    from lightning_pose_amd.callbacks import PatchMasking
    return PatchMasking(patch_mask_config={**CONFIG, "final_ratio": 0.0}, patch_seed=42)


def _images(dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(2, 2, 3, 64, 64, generator=g) + 3.0).to(dev)    # (no zeros of its own: a zero pixel is a masked pixel)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ---- attributes, defaults, schedule (no device) ---------------------------------------------------------------------------------------
def test_attributes_and_defaults():
    from lightning_pose_amd.callbacks import PatchMasker

    m = PatchMasker(patch_mask_config=dict(CONFIG), patch_seed=42)
    assert (m.patch_seed, m.patch_init_step, m.patch_final_step, m.patch_init_ratio, m.patch_final_ratio) == (42, 100, 500, 0.1, 0.5)
    assert m.use_patch_masking is True and m.selection == "device"
    for d in (PatchMasker(), PatchMasker(patch_mask_config={}, patch_seed=0)):
        assert (d.patch_seed, d.patch_init_step, d.patch_final_step, d.patch_init_ratio, d.patch_final_ratio) == (0, 700, 5000, 0.1, 0.5)
        assert d.use_patch_masking is True
    assert PatchMasker({"final_ratio": 0.0}).use_patch_masking is False
    assert _enabled().curriculum_masking.use_patch_masking is True and _enabled().curriculum_masking.patch_seed == 42
    with pytest.raises(ValueError, match="selection"):
        PatchMasker(selection="host")


def test_schedule_at_the_reference_test_steps():
    m = _enabled().curriculum_masking
    info = {s: m.get_training_schedule_info(s) for s in STEPS}
    assert set(info[50]) == {"step", "mask_ratio", "curriculum_progress", "steps_to_patch_masking", "steps_to_max_masking"}
    assert info[50] == {"step": 50, "mask_ratio": 0.0, "curriculum_progress": "0.0%", "steps_to_patch_masking": 50, "steps_to_max_masking": 450}
    assert info[100]["mask_ratio"] == 0.1 and info[100]["curriculum_progress"] == "0.0%" and info[100]["steps_to_max_masking"] == 400
    assert abs(info[300]["mask_ratio"] - 0.3) < 1e-6 and info[300]["curriculum_progress"] == "50.0%"
    assert info[500]["mask_ratio"] == 0.5 and info[500]["curriculum_progress"] == "100.0%" and info[500]["steps_to_max_masking"] == 0
    assert info[700]["mask_ratio"] == 0.5 and info[700]["curriculum_progress"] == "100.0%" and info[700]["steps_to_patch_masking"] == 0
    assert [m.should_start_patch_masking(s) for s in (99, 100, 101)] == [False, True, False]


def test_disabled_schedule_masking_and_hooks():
    cb = _disabled()
    m = cb.curriculum_masking
    assert m.use_patch_masking is False and not m.should_start_patch_masking(100)
    assert m.get_training_schedule_info(300) == {"step": 300, "mask_ratio": 0.0, "curriculum_progress": "0.0%", "steps_to_patch_masking": 0,
                                                 "steps_to_max_masking": 0}
    images = torch.ones(2, 2, 3, 64, 64)
    same, dummy = m.apply_masking(images, training_step=300)
    assert same is images and dummy.shape == (2, 2) and bool((dummy == 1).all())
    trainer, module = MagicMock(), MagicMock(spec=["log"])
    trainer.global_step = 300
    batch = {"images": images}
    cb.on_train_batch_start(trainer, module, batch, batch_idx=0)
    assert batch["images"] is images and not hasattr(module, "current_patch_mask")
    cb.on_train_epoch_end(trainer, module)
    module.log.assert_not_called()


def test_epoch_end_logs_the_ratio_once():
    trainer, module = MagicMock(), MagicMock()
    trainer.global_step = 300
    _enabled().on_train_epoch_end(trainer, module)
    module.log.assert_called_once()
    args, kwargs = module.log.call_args
    assert args[0] == "patch_mask_ratio" and abs(args[1] - 0.3) < 1e-6
    assert kwargs == {"on_step": False, "on_epoch": True, "prog_bar": True}


# ---- the masked images --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("selection", ["device", "reference"])
def test_masked_patches_are_zero_blocks_and_the_rest_is_the_input(stack_backend, selection):
    dev = stack_backend
    m = _enabled(selection=selection).curriculum_masking
    images = _images(dev)
    before = _bits(images).clone()
    for step, zeroed in zip(STEPS, ZEROED):
        masked, mask = m.apply_patch_masking(images, training_step=step, is_training=True)
        assert mask.dtype == torch.float32 and mask.shape == (2, 2, 16) and mask.device == images.device
        assert masked.shape == images.shape and masked.dtype == torch.float32 and masked.device == images.device
        assert ((mask == 0).sum(-1) == zeroed).all() and ((mask == 0) | (mask == 1)).all()
        # the mask, blown up to pixels, says exactly which bits are zero and which are the input's
        pixels = mask.cpu().view(2, 2, 1, 4, 1, 4, 1).expand(2, 2, 3, 4, 16, 4, 16).reshape(2, 2, 3, 64, 64).bool()
        assert torch.equal(_bits(masked), torch.where(pixels, before, torch.zeros_like(before)))
        assert torch.equal(_bits(images), before)                         # the original is untouched
        if zeroed == 0:
            assert masked is images
    off, ones = m.apply_patch_masking(images, training_step=500, is_training=False)
    assert off is images and ones.shape == (2, 2, 16) and bool((ones == 1).all()) and ones.device == images.device
    again = m.apply_patch_masking(images, training_step=300)[1]          # the same step: the same choice; another step: another
    assert torch.equal(again, m.apply_patch_masking(images, training_step=300)[1])
    assert not torch.equal(again, m.apply_patch_masking(images, training_step=301)[1])


def test_batch_rules_images_frames_no_key_and_bare_tensor(stack_backend):
    dev = stack_backend
    cb = _enabled()
    trainer = MagicMock()
    trainer.global_step = 200                                                 # ratio 0.2: 3 of 16 patches
    for key in ("images", "frames"):
        module = MagicMock(spec=[])
        images = _images(dev)
        before = _bits(images).clone()
        batch = {key: images, "labels": torch.ones(2)}
        cb.on_train_batch_start(trainer, module, batch, batch_idx=0)
        assert batch[key] is not images and not torch.equal(batch[key], images) and torch.equal(_bits(images), before)
        assert module.current_patch_mask.shape == (2, 2, 16) and ((module.current_patch_mask == 0).sum(-1) == 3).all()
        assert int((batch[key] == 0).sum()) == 2 * 2 * 3 * 3 * 256
    both = {"images": _images(dev), "frames": _images(dev, 1)}               # "images" wins, "frames" is left alone
    frames = both["frames"]
    cb.on_train_batch_start(trainer, MagicMock(spec=[]), both, batch_idx=0)
    assert both["frames"] is frames and int((both["images"] == 0).sum()) > 0
    module = MagicMock(spec=[])
    cb.on_train_batch_start(trainer, module, {"labels": torch.ones(2)}, batch_idx=0)
    assert not hasattr(module, "current_patch_mask")
    # a semi-supervised batch has neither key at its top level: not masked (the reference's behaviour, mirrored)
    nested = {"labeled": {"images": _images(dev)}, "unlabeled": {"frames": _images(dev, 1)}}
    kept = nested["labeled"]["images"], nested["unlabeled"]["frames"]
    cb.on_train_batch_start(trainer, module, nested, batch_idx=0)
    assert nested["labeled"]["images"] is kept[0] and nested["unlabeled"]["frames"] is kept[1] and not hasattr(module, "current_patch_mask")
    # a bare tensor: the mask is stored, the caller's tensor is not written
    bare = _images(dev)
    before = _bits(bare).clone()
    cb.on_train_batch_start(trainer, module, bare, batch_idx=0)
    assert torch.equal(_bits(bare), before) and ((module.current_patch_mask == 0).sum(-1) == 3).all()


def test_ops_patch_mask_argument_checks(stack_backend):
    from lightning_pose_amd import ops

    dev = stack_backend
    images = _images(dev)
    a, ma = ops.patch_mask(images, (42, 300), 4)
    b, mb = ops.patch_mask(images, ops.patch_mask_key(42, 300), 4)            # (seed, step) and the packed key: the same call
    assert torch.equal(_bits(a), _bits(b)) and torch.equal(ma, mb)
    view = images.transpose(3, 4)                                             # not contiguous: made so
    c, mc = ops.patch_mask(view, (42, 300), 4)
    d, md = ops.patch_mask(view.contiguous(), (42, 300), 4)
    assert torch.equal(_bits(c), _bits(d)) and torch.equal(mc, md)
    given = torch.ones(2, 2, 16, device=dev)
    given[1, 0, 5] = 0
    e, me = ops.patch_mask(images, 0, 0, mask=given)
    assert torch.equal(me, given) and int((e == 0).sum()) == 3 * 256 and bool((e[1, 0, :, 16:32, 16:32] == 0).all())
    with pytest.raises(AssertionError):
        ops.patch_mask(images.clone().requires_grad_(), (0, 0), 1)
    with pytest.raises(ValueError):
        ops.patch_mask(images[0], (0, 0), 1)
    with pytest.raises(ValueError):
        ops.patch_mask(images, (0, 0), 17)                                    # more than N patches: the library's argument error
    with pytest.raises(ValueError):
        ops.patch_mask(images, (0, 0), 1, mask=torch.ones(2, 2, 15, device=dev))
    with pytest.raises(NotImplementedError, match="528 x 512"):
        ops.patch_mask(torch.zeros(1, 1, 1, 528, 512, device=dev), (0, 0), 1)


# ---- get_patch_masking_callback ------------------------------------------------------------------------------------------------------------
def _cfg(model_type="heatmap_multiview_transformer", **patch_mask):
    return {"model": {"model_type": model_type}, "training": {"rng_seed_model_pt": 7, "patch_mask": patch_mask}}


def test_get_patch_masking_callback():
    from lightning_pose_amd.callbacks import PatchMasking, get_patch_masking_callback

    cfg = _cfg(init_epoch=40, final_epoch=300, init_ratio=0.1, final_ratio=0.5)
    untouched = copy.deepcopy(cfg)
    cb = get_patch_masking_callback(cfg, steps_per_epoch=7)
    m = cb.curriculum_masking
    assert isinstance(cb, PatchMasking) and (m.patch_init_step, m.patch_final_step, m.patch_seed) == (280, 2100, 7)
    assert (m.patch_init_ratio, m.patch_final_ratio) == (0.1, 0.5)
    assert cfg == untouched                                                   # the caller's config is not changed
    assert get_patch_masking_callback(_cfg(init_epoch=0.5, final_epoch=1.5, final_ratio=0.5), 7).curriculum_masking.patch_init_step == 4
    with pytest.raises(ValueError, match="steps_per_epoch"):
        get_patch_masking_callback(cfg)
    steps = get_patch_masking_callback(_cfg(init_step=10, final_step=20, final_ratio=0.25))
    assert (steps.curriculum_masking.patch_init_step, steps.curriculum_masking.patch_final_step) == (10, 20)
    assert get_patch_masking_callback(_cfg(final_ratio=0.5)).curriculum_masking.patch_init_step == 700      # the reference's default config
    assert get_patch_masking_callback(_cfg(final_ratio=0.0)) is None
    assert get_patch_masking_callback(_cfg(model_type="heatmap", final_ratio=0.5)) is None
    assert get_patch_masking_callback({"model": {"model_type": "heatmap_multiview_transformer"}, "training": {"rng_seed_model_pt": 0}}) is None


# ---- against the reference's verbatim classes ----------------------------------------------------------------------------------------------
def _reference_callbacks():
    """the reference's own lightning_pose/callbacks.py, executed verbatim"""
    import transformers  # noqa: F401  (first: it probes for torchvision when imported, and the loader registers a bare stand-in under that name)
    from oracle import ref_loader as R

    return R.load("callbacks")


@needs_reference
@pytest.mark.reference
def test_reference_selection_is_the_verbatim_patch_masker_bit_for_bit(stack_backend):
    dev = stack_backend
    ref = _reference_callbacks().PatchMasker(patch_mask_config=dict(CONFIG), patch_seed=42)
    mine = _enabled(selection="reference").curriculum_masking
    images = _images(dev)
    for step in (100, 300, 500):
        want, want_mask = ref.apply_patch_masking(images, training_step=step, is_training=True)
        got, got_mask = mine.apply_patch_masking(images, training_step=step, is_training=True)
        assert torch.equal(_bits(got), _bits(want)) and torch.equal(got_mask, want_mask)
        assert got_mask.dtype == want_mask.dtype and got_mask.device == want_mask.device and got_mask.shape == want_mask.shape
    for step in (0, 50, 99, 100, 101, 250, 300, 499, 500, 700):
        assert mine.get_training_schedule_info(step) == ref.get_training_schedule_info(step)
    off = _reference_callbacks().PatchMasker(patch_mask_config={**CONFIG, "final_ratio": 0.0}, patch_seed=42)
    assert _disabled().curriculum_masking.get_training_schedule_info(300) == off.get_training_schedule_info(300)
    assert off.apply_masking(images)[1].shape == _disabled().curriculum_masking.apply_masking(images)[1].shape


class _Module:
    """the LightningModule surface Trainer.fit uses, around one weight"""
    device = torch.device("cpu")
    training = True

    def __init__(self):
        self.global_step, self.current_epoch, self.logged = 0, 0, {}
        self.w = torch.zeros(1, requires_grad=True)
        self.seen = []

    def train(self, mode=True):
        self.training = mode

    def optimizers(self):
        return self

    def zero_grad(self):
        pass

    def step(self):
        pass

    def get_scheduler(self, opt):
        return self

    def log(self, name, value, **kwargs):
        self.logged[name] = torch.tensor(float(value))

    def training_step(self, batch, batch_idx):
        self.seen.append(batch["images"])
        return {"loss": (self.w * 0).sum()}


@needs_reference
@pytest.mark.reference
def test_the_verbatim_patch_masking_callback_runs_under_the_product_trainer():
    """the boundary from the reference's side: its callback reads ``trainer.global_step`` and is called at ``on_train_epoch_end``"""
    from lightning_pose_amd.trainer import Trainer

    cb = _reference_callbacks().PatchMasking(patch_mask_config={"init_step": 1, "final_step": 2, "init_ratio": 0.25, "final_ratio": 0.5}, patch_seed=3)
    model = _Module()
    trainer = Trainer(max_epochs=1, callbacks=[cb], data_parallel=False)
    assert trainer.global_step == 0
    images = torch.ones(2, 2, 3, 64, 64)
    trainer.fit(model, [{"images": images}, {"images": images}])
    assert trainer.global_step == model.global_step == 2
    assert [int((x == 0).sum()) for x in model.seen] == [0, 4 * 4 * 3 * 256]   # step 0: nothing; step 1: int(0.25 * 16) patches per view
    assert model.current_patch_mask.shape == (2, 2, 16) and bool((images == 1).all())
    assert float(model.logged["patch_mask_ratio"]) == 0.5                       # logged at the end of the epoch, at step 2
