"""Host-side pieces of the DINOv2 backbones ("vits_dinov2" / "vitb_dinov2"; reference lightning_pose/models/backbones/vit_dino.py,
factory.py:194-201): the seeded initial weights, and the loader of a ``Dinov2Model`` checkpoint.

The reference loads ``facebook/dinov2-{small,base}`` (patch 14, a 37 x 37 position table from 518-px pretraining) and resamples the patch
projection to 16 x 16 once, at construction; everything downstream runs at patch 16.  Here the weights arrive through
``backbone_checkpoint`` (nothing is downloaded), and the same resampling is applied to a projection that is not 16 x 16 yet."""

from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

PREFIX = "backbone.vision_encoder."
PROJECTION = "embeddings.patch_embeddings.projection.weight"


def resize_patch_projection(weight: torch.Tensor, patch: int = 16) -> torch.Tensor:
    """(D, C, p, p) patch-projection weights -> (D, C, patch, patch): every (output, input) channel pair is one p x p image, resized
    bicubically with ``align_corners=True, antialias=True`` (the reference's ``_resize_patch_embedding_weights``).  A projection that
    already has the target size is returned as it is."""
    d, c, ph, pw = weight.shape
    if (ph, pw) == (patch, patch):
        return weight
    planes = weight.detach().to(torch.float32).reshape(d * c, 1, ph, pw)
    return F.interpolate(planes, size=(patch, patch), mode="bicubic", align_corners=True, antialias=True).reshape(d, c, patch, patch)


def dinov2_seeded_state_dict(hidden: int, depth: int, heads: int, mlp: int, patch: int, grid: int) -> dict[str, torch.Tensor]:
    """Random DINOv2 weights under the reference's ``backbone.vision_encoder.*`` names (those of ``transformers.Dinov2Model``): what
    ``Dinov2Model(config)`` gives under the current seed when transformers is installed, its initialisation restated otherwise (truncated
    normal 0.02 for weights, the [CLS] token and the position table; zero biases and ``mask_token``; LayerNorm 1 / 0; ``lambda1`` = 1)."""
    try:
        from transformers import Dinov2Config, Dinov2Model
        cfg = Dinov2Config(hidden_size=hidden, num_hidden_layers=depth, num_attention_heads=heads, mlp_ratio=mlp // hidden,
                           image_size=patch * grid, patch_size=patch)
        return {PREFIX + k: v.detach() for k, v in Dinov2Model(cfg).state_dict().items()}
    except ImportError:
        tn = lambda *shape: nn.init.trunc_normal_(torch.empty(*shape), std=0.02)  # noqa: E731
        sd = {"embeddings.cls_token": tn(1, 1, hidden), "embeddings.mask_token": torch.zeros(1, hidden),
              "embeddings.position_embeddings": tn(1, 1 + grid * grid, hidden), PROJECTION: tn(hidden, 3, patch, patch),
              "embeddings.patch_embeddings.projection.bias": torch.zeros(hidden)}
        for i in range(depth):
            p = f"encoder.layer.{i}"
            for nm, (n, k) in (("attention.attention.query", (hidden, hidden)), ("attention.attention.key", (hidden, hidden)),
                               ("attention.attention.value", (hidden, hidden)), ("attention.output.dense", (hidden, hidden)),
                               ("mlp.fc1", (mlp, hidden)), ("mlp.fc2", (hidden, mlp))):
                sd[f"{p}.{nm}.weight"], sd[f"{p}.{nm}.bias"] = tn(n, k), torch.zeros(n)
            for nm in ("norm1", "norm2"):
                sd[f"{p}.{nm}.weight"], sd[f"{p}.{nm}.bias"] = torch.ones(hidden), torch.zeros(hidden)
            sd[f"{p}.layer_scale1.lambda1"], sd[f"{p}.layer_scale2.lambda1"] = torch.ones(hidden), torch.ones(hidden)
        sd["layernorm.weight"], sd["layernorm.bias"] = torch.ones(hidden), torch.zeros(hidden)
        return {PREFIX + k: v for k, v in sd.items()}


def load_dinov2_checkpoint(path: str, init: dict[str, torch.Tensor], patch: int = 16) -> None:
    """Overwrite the entries of ``init`` (``backbone.vision_encoder.*`` names) with the tensors of a ``Dinov2Model`` state dict: a
    ``.safetensors`` file or a ``torch.save``d dict (bare, or under "state_dict"), keys with or without the ``backbone.vision_encoder.``
    prefix.  The patch projection is resampled to ``patch``; any other tensor whose shape does not fit is an error, not a silent skip."""
    if str(path).endswith(".safetensors"):
        import safetensors.torch
        hf = safetensors.torch.load_file(path, device="cpu")
    else:
        hf = torch.load(path, map_location="cpu")
        hf = hf.get("state_dict", hf)
    for k, v in hf.items():
        key = k if k.startswith(PREFIX) else PREFIX + k
        if key not in init:
            continue   # (e.g. the head of a whole-model checkpoint, a pooler)
        if key == PREFIX + PROJECTION:
            v = resize_patch_projection(v, patch)
        if tuple(init[key].shape) != tuple(v.shape):
            raise ValueError(f"backbone_checkpoint: {k} has shape {tuple(v.shape)}, this backbone needs {tuple(init[key].shape)}")
        init[key] = v
