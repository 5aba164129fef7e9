"""Host-side pieces of the SAM backbone ("vitb_sam"; reference lightning_pose/models/backbones/vit_sam.py, factory.py:219-222): its
configuration, the seeded initial weights, and the loader of a ``SamModel`` / ``SamVisionEncoder`` checkpoint.

The reference loads ``facebook/sam-vit-base`` and keeps the vision encoder: relative positions switched off, the neck skipped, and
``pos_embed`` (1, 64, 64, C) resized ONCE, at construction, to the fine-tuning grid - it is the trained parameter at that size.  Here the
weights arrive through ``backbone_checkpoint`` (nothing is downloaded) and go through the same one ``interpolate`` call."""

from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

PREFIX = "backbone.vision_encoder."
HF_NAMES = {"vitb_sam": "facebook/sam-vit-base"}

# (hidden, depth, heads, mlp, patch, window, global layers, pretraining grid, neck channels) of facebook/sam-vit-base's vision config.
# Single-view only; a table of its own (VIT_CONFIGS is also the multi-view transformer tracker's list of backbones).
SAM_CONFIGS = {"vitb_sam": (768, 12, 12, 3072, 16, 14, (2, 5, 8, 11), 64, 256)}


def resize_pos_embed(pos: torch.Tensor, grid: int) -> torch.Tensor:
    """``VisionEncoderSam._resize_pos_embed``: (1, g0, g0, C) -> (1, grid, grid, C) with its one bicubic, anti-aliased ``interpolate`` call;
    a table already at ``grid`` is returned as it is"""
    if pos.shape[1] == grid and pos.shape[2] == grid:
        return pos
    out = F.interpolate(pos.permute(0, 3, 1, 2), size=(grid, grid), mode="bicubic", antialias=True)
    return out.permute(0, 2, 3, 1).contiguous()


def sam_seeded_state_dict(hidden: int, depth: int, heads: int, mlp: int, patch: int, window: int, global_layers: tuple[int, ...],
                          pretrain_grid: int, neck_channels: int, grid: int) -> dict[str, torch.Tensor]:
    """Random SAM weights under the reference's ``backbone.vision_encoder.*`` names (those of ``transformers``' ``SamVisionEncoder``), with
    ``pos_embed`` at the fine-tuning ``grid``: what ``SamVisionEncoder(config)`` gives under the current seed when transformers carries it,
    its initialisation restated otherwise.  ``SamVisionConfig.initializer_range`` defaults to 1e-10 - SAM is only ever loaded pretrained -
    which no model can train from, so the weights are drawn with the 0.02 of the other ViTs here; ``pos_embed``, ``rel_pos_*`` and the
    biases are zero and the LayerNorms 1 / 0, as HF leaves them."""
    try:
        from transformers import SamVisionConfig
        from transformers.models.sam.modeling_sam import SamVisionEncoder
        cfg = SamVisionConfig(hidden_size=hidden, num_hidden_layers=depth, num_attention_heads=heads, mlp_dim=mlp, patch_size=patch,
                              image_size=patch * pretrain_grid, window_size=window, global_attn_indexes=list(global_layers),
                              output_channels=neck_channels, initializer_range=0.02)
        sd = {k: v.detach() for k, v in SamVisionEncoder(cfg).state_dict().items()}
    except ImportError:
        hd = hidden // heads
        tn = lambda *shape: nn.init.trunc_normal_(torch.empty(*shape), std=0.02)  # noqa: E731
        sd = {"pos_embed": torch.zeros(1, pretrain_grid, pretrain_grid, hidden), "patch_embed.projection.weight": tn(hidden, 3, patch, patch),
              "patch_embed.projection.bias": torch.zeros(hidden)}
        for i in range(depth):
            p = f"layers.{i}"
            n_rel = 2 * (pretrain_grid if i in global_layers else window) - 1
            sd[f"{p}.attn.rel_pos_h"], sd[f"{p}.attn.rel_pos_w"] = torch.zeros(n_rel, hd), torch.zeros(n_rel, hd)
            for nm, (n, k) in (("attn.qkv", (3 * hidden, hidden)), ("attn.proj", (hidden, hidden)), ("mlp.lin1", (mlp, hidden)),
                               ("mlp.lin2", (hidden, mlp))):
                sd[f"{p}.{nm}.weight"], sd[f"{p}.{nm}.bias"] = tn(n, k), torch.zeros(n)
            for nm in ("layer_norm1", "layer_norm2"):
                sd[f"{p}.{nm}.weight"], sd[f"{p}.{nm}.bias"] = torch.ones(hidden), torch.zeros(hidden)
        sd["neck.conv1.weight"], sd["neck.conv2.weight"] = tn(neck_channels, hidden, 1, 1), tn(neck_channels, neck_channels, 3, 3)
        for nm in ("neck.layer_norm1", "neck.layer_norm2"):
            sd[f"{nm}.weight"], sd[f"{nm}.bias"] = torch.ones(neck_channels), torch.zeros(neck_channels)
    sd["pos_embed"] = resize_pos_embed(sd["pos_embed"], grid)
    return {PREFIX + k: v for k, v in sd.items()}


def load_sam_checkpoint(path: str, init: dict[str, torch.Tensor]) -> None:
    """Overwrite the entries of ``init`` (``backbone.vision_encoder.*`` names, ``pos_embed`` at the fine-tuning grid) with the tensors of a
    ``SamModel`` or ``SamVisionEncoder`` state dict: a ``.safetensors`` file or a ``torch.save``d dict (bare, or under "state_dict"), keys
    as ``vision_encoder.*`` (SamModel), bare (SamVisionEncoder) or already under ``backbone.vision_encoder.``.  ``pos_embed`` arrives at
    its pretraining grid and is resized with the reference's one ``interpolate`` call.  A tensor whose shape does not fit is an error that
    names the key, not a silent skip; keys of other modules (``prompt_encoder.*``, ``mask_decoder.*``, a head) are ignored."""
    if str(path).endswith(".safetensors"):
        import safetensors.torch
        hf = safetensors.torch.load_file(path, device="cpu")
    else:
        hf = torch.load(path, map_location="cpu")
        hf = hf.get("state_dict", hf)
    pos_key = PREFIX + "pos_embed"
    for k, v in hf.items():
        key = k if k.startswith(PREFIX) else ("backbone." + k if k.startswith("vision_encoder.") else PREFIX + k)
        if key not in init:
            continue   # (the prompt encoder and mask decoder of a whole SamModel, a head)
        want = tuple(init[key].shape)
        if key == pos_key:
            if v.dim() != 4 or v.shape[0] != 1 or v.shape[1] != v.shape[2] or v.shape[3] != want[3]:
                raise ValueError(f"backbone_checkpoint: {k} has shape {tuple(v.shape)}, this backbone needs (1, g, g, {want[3]}) - a square "
                                 f"position table, resized here to {want[1]} x {want[2]}")
            v = resize_pos_embed(v.to(torch.float32), want[1])
        if tuple(v.shape) != want:
            raise ValueError(f"backbone_checkpoint: {k} has shape {tuple(v.shape)}, this backbone needs {want}")
        init[key] = v
