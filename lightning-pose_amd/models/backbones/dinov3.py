"""Host-side pieces of the DINOv3 backbones ("vits_dinov3" / "vitb_dinov3"; reference lightning_pose/models/backbones/vit_dino.py,
factory.py:69-89): the seeded initial weights, and the loader of a ``DINOv3ViTModel`` checkpoint.

The reference loads ``facebook/dinov3-vit{s,b}16-pretrain-lvd1689m`` (native 16-px patches: nothing is resampled, and there is no position
table - the positions are rotary).  Here the weights arrive through ``backbone_checkpoint`` (nothing is downloaded).  The engine runs the
plain-MLP models without a key bias only, so a gated-MLP checkpoint (ViT-H+ and up) or one with a ``k_proj.bias`` is refused by name."""

from __future__ import annotations

import torch
import torch.nn as nn

PREFIX = "backbone.vision_encoder."
HF_NAMES = {"vits_dinov3": "facebook/dinov3-vits16-pretrain-lvd1689m", "vitb_dinov3": "facebook/dinov3-vitb16-pretrain-lvd1689m"}


def dinov3_seeded_state_dict(hidden: int, depth: int, heads: int, mlp: int, patch: int, registers: int) -> dict[str, torch.Tensor]:
    """Random DINOv3 weights under the reference's ``backbone.vision_encoder.*`` names (those of ``transformers.DINOv3ViTModel``): what
    ``DINOv3ViTModel(config)`` gives under the current seed when transformers carries it, its initialisation restated otherwise (truncated
    normal 0.02 for weights, the [CLS] and register tokens; zero biases and ``mask_token``; LayerNorm 1 / 0; ``lambda1`` = 1)."""
    try:
        from transformers import DINOv3ViTConfig, DINOv3ViTModel
        cfg = DINOv3ViTConfig(hidden_size=hidden, num_hidden_layers=depth, num_attention_heads=heads, intermediate_size=mlp, patch_size=patch,
                              num_register_tokens=registers, image_size=14 * patch)
        sd = {PREFIX + k: v.detach() for k, v in DINOv3ViTModel(cfg).state_dict().items()}
        for k in list(sd):   # (a config default that would add a key bias: the engine has none)
            if k.endswith("k_proj.bias"):
                del sd[k]
        return sd
    except ImportError:
        tn = lambda *shape: nn.init.trunc_normal_(torch.empty(*shape), std=0.02)  # noqa: E731
        sd = {"embeddings.cls_token": tn(1, 1, hidden), "embeddings.mask_token": torch.zeros(1, 1, hidden),
              "embeddings.register_tokens": tn(1, registers, hidden), "embeddings.patch_embeddings.weight": tn(hidden, 3, patch, patch),
              "embeddings.patch_embeddings.bias": torch.zeros(hidden)}
        for i in range(depth):
            p = f"model.layer.{i}"
            for nm, (n, k) in (("attention.q_proj", (hidden, hidden)), ("attention.k_proj", (hidden, hidden)),
                               ("attention.v_proj", (hidden, hidden)), ("attention.o_proj", (hidden, hidden)),
                               ("mlp.up_proj", (mlp, hidden)), ("mlp.down_proj", (hidden, mlp))):
                sd[f"{p}.{nm}.weight"] = tn(n, k)
                if nm != "attention.k_proj":
                    sd[f"{p}.{nm}.bias"] = torch.zeros(n)
            for nm in ("norm1", "norm2"):
                sd[f"{p}.{nm}.weight"], sd[f"{p}.{nm}.bias"] = torch.ones(hidden), torch.zeros(hidden)
            sd[f"{p}.layer_scale1.lambda1"], sd[f"{p}.layer_scale2.lambda1"] = torch.ones(hidden), torch.ones(hidden)
        sd["norm.weight"], sd["norm.bias"] = torch.ones(hidden), torch.zeros(hidden)
        return {PREFIX + k: v for k, v in sd.items()}


def load_dinov3_checkpoint(path: str, init: dict[str, torch.Tensor]) -> None:
    """Overwrite the entries of ``init`` (``backbone.vision_encoder.*`` names) with the tensors of a ``DINOv3ViTModel`` state dict: a
    ``.safetensors`` file or a ``torch.save``d dict (bare, or under "state_dict"), keys with or without the ``backbone.vision_encoder.``
    prefix.  A gated-MLP checkpoint (``mlp.gate_proj.*``), a ``k_proj.bias`` or a tensor whose shape does not fit is an error that names the
    key, not a silent skip; keys of other modules (a head, a pooler) are ignored."""
    if str(path).endswith(".safetensors"):
        import safetensors.torch
        hf = safetensors.torch.load_file(path, device="cpu")
    else:
        hf = torch.load(path, map_location="cpu")
        hf = hf.get("state_dict", hf)
    for k, v in hf.items():
        key = k if k.startswith(PREFIX) else PREFIX + k
        if ".mlp.gate_proj." in key:
            raise ValueError(f"backbone_checkpoint: {k} belongs to a gated-MLP DINOv3 model (use_gated_mlp=True, ViT-H+ and larger); "
                             "only the plain-MLP models (vits16, vitb16) are implemented")
        if key.endswith("attention.k_proj.bias"):
            raise ValueError(f"backbone_checkpoint: {k}: this backbone has no key bias (DINOv3ViTConfig.key_bias=False)")
        if key not in init:
            continue   # (e.g. the head of a whole-model checkpoint)
        if tuple(init[key].shape) != tuple(v.shape):
            raise ValueError(f"backbone_checkpoint: {k} has shape {tuple(v.shape)}, this backbone needs {tuple(init[key].shape)}")
        init[key] = v
