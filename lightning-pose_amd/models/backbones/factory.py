"""Backbone registry for the MI355X path (reference: lightning_pose/models/backbones/factory.py:98-168,170-236,238-348)."""

from __future__ import annotations

# SAM ("vitb_sam": windowed attention, no [CLS], position table at the fine-tuning grid) has its own table, next to its loader
from .sam import SAM_CONFIGS  # noqa: F401

# The reference's ResNet-50 variants differ only in where their pretrained weights come from (torchvision ImageNet for "resnet50",
# mmpose checkpoints for the animal / human ones - reference :253-283; its shipped default is "resnet50_animal_ap10k",
# config_default.yaml:121): one architecture here, the weights arrive through ``backbone_checkpoint``.
RESNET50_VARIANTS = ("resnet50", "resnet50_animal_apose", "resnet50_animal_ap10k", "resnet50_human_jhmdb", "resnet50_human_res_rle",
                     "resnet50_human_top_res", "resnet50_human_hand")

BACKBONE_STRIDES: dict[str, int] = {**{n: 32 for n in RESNET50_VARIANTS}, "vits_dino": 16, "vitb_dino": 16, "vits_dinov2": 16, "vitb_dinov2": 16,
                                    "vits_dinov3": 16, "vitb_dinov3": 16, "vitb_sam": 16}

# name -> number of output features
_IMPLEMENTED = {**{n: 2048 for n in RESNET50_VARIANTS}, "vits_dino": 384, "vitb_dino": 768, "vits_dinov2": 384, "vitb_dinov2": 768}

# ViT variants: (hidden, depth, heads, mlp, patch, pretraining grid) of facebook/dino-vit{s,b}16
VIT_CONFIGS = {"vits_dino": (384, 12, 6, 1536, 16, 14), "vitb_dino": (768, 12, 12, 3072, 16, 14)}

# DINOv2 variants, same fields: facebook/dinov2-{small,base} with the patch projection resampled from 14 to 16 px (reference
# models/backbones/vit_dino.py; the 37 x 37 position table is that of the 518-px pretraining).  A table of their own: VIT_CONFIGS is also the
# list of backbones the multi-view transformer tracker accepts, and DINOv2 is single-view only.
DINOV2_CONFIGS = {"vits_dinov2": (384, 12, 6, 1536, 16, 37), "vitb_dinov2": (768, 12, 12, 3072, 16, 37)}

# DINOv3 variants: (hidden, depth, heads, mlp, patch, register tokens) of facebook/dinov3-vit{s,b}16-pretrain-lvd1689m - native 16-px patches,
# rotary positions instead of a table (so no pretraining grid), plain GELU MLP.  Single-view only, as DINOv2.
DINOV3_CONFIGS = {"vits_dinov3": (384, 12, 6, 1536, 16, 4), "vitb_dinov3": (768, 12, 12, 3072, 16, 4)}


def backbone_features(backbone_arch: str) -> int:
    """Output features of the backbones every tracker family knows.  The DINOv3 variants and SAM are NOT in this list: it keeps refusing their
    names, as tests/test_dinov2_tracker.py holds it to; the single-view heatmap trackers, which do run them, ask ``tracker_backbone_features``."""
    if backbone_arch not in _IMPLEMENTED:
        raise ValueError(f'"{backbone_arch}" is not a valid backbone; allowed backbones: {sorted(_IMPLEMENTED)}')
    return _IMPLEMENTED[backbone_arch]


def tracker_backbone_features(backbone_arch: str) -> int:
    """Output features of a backbone of the single-view heatmap trackers: ``backbone_features``' list, the DINOv3 variants and SAM"""
    if backbone_arch in DINOV3_CONFIGS:
        return DINOV3_CONFIGS[backbone_arch][0]
    if backbone_arch in SAM_CONFIGS:
        return SAM_CONFIGS[backbone_arch][0]
    if backbone_arch not in _IMPLEMENTED:
        raise ValueError(f'"{backbone_arch}" is not a valid backbone; allowed backbones: {sorted([*_IMPLEMENTED, *DINOV3_CONFIGS, *SAM_CONFIGS])}')
    return _IMPLEMENTED[backbone_arch]
