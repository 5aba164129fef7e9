"""ViT-S/16 ("vits_dino") backbone + heat-map head on the MI355X kernels: the drop-in for
``VisionEncoder`` -> HuggingFace ``ViTModel`` (reference models/backbones/vit.py:16-49, factory.py:188-190).

Same contract as :class:`lightning_pose_amd.engine.Engine` (flat fp32 parameter / gradient buffers, bf16 operand copies,
``forward`` -> (heat-maps, tape), hand-written ``backward``), parameters exposed under the reference's ``state_dict`` names
(``backbone.vision_encoder.embeddings.*``, ``...layers.{i}.attention.{q,k,v,o}_proj.*``, ``...layers.{i}.mlp.fc{1,2}.*``,
``...layernorm*``, ``head.upsampling_layers.*`` - the names of the installed transformers 5.x ``ViTModel``; the 4.x names
``encoder.layer.{i}.attention.attention.query`` ... are accepted by ``load_state_dict``).

Every Linear layer runs on the MFMA GEMM (``lp_gemm_nt``: forward and data-gradient; ``lp_conv_wgrad_bias``: weight + bias gradient).
Attention is ``lp_attn_fwd`` - one fused kernel per layer working straight on the (image, head) slices of the fused QKV tensor: the
scores never leave the chip, the probabilities are written once in bf16 (row pitch padded to a multiple of 64) for the backward
pass - and, backward, ``lp_attn_rowdot`` + ``lp_attn_dscores`` (soft-max backward in the store pass of dO V^T), ``lp_gemm_tn`` (dV, dK:
both operands contracted over their rows, no transposed copies) and one more ``lp_gemm_nt`` (dQ).  The glue (LayerNorm, GELU, token
assembly, the small head-slice transpose) is csrc/vit.hip.  The residual stream, LayerNorm statistics and all reductions are fp32;
GEMM operands bf16.
"""

from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib, ops
from ._lib import check
from .engine import ConvP, EngineCore, Tape, build_head, image_parts, place_head
from .ops import _p

LN_EPS = 1e-12  # ViTConfig.layer_norm_eps
DINOV2_LN_EPS = 1e-6  # Dinov2Config.layer_norm_eps
DINOV3_LN_EPS = 1e-5  # DINOv3ViTConfig.layer_norm_eps
SAM_LN_EPS = 1e-6     # SamVisionConfig.layer_norm_eps


def bicubic_matrix(n_in: int, n_out: int) -> np.ndarray:
    """(n_out, n_in) weights of torch's 1-D bicubic resize, align_corners=False (A = -0.75, border taps clamped)."""
    A = -0.75
    w = np.zeros((n_out, n_in), np.float64)
    scale = n_in / n_out

    def k1(t):
        return ((A + 2) * t - (A + 3)) * t * t + 1

    def k2(t):
        return ((A * t - 5 * A) * t + 8 * A) * t - 4 * A

    for i in range(n_out):
        src = (i + 0.5) * scale - 0.5
        i0 = math.floor(src)
        t = src - i0
        for tap, wt in zip((i0 - 1, i0, i0 + 1, i0 + 2), (k2(t + 1), k1(t), k1(1 - t), k2(2 - t))):
            w[i, min(max(tap, 0), n_in - 1)] += wt
    return w


@dataclass
class Lin:
    name: str      # state_dict prefix (weight / bias), or a list of three for the fused q, k, v
    N: int
    K: int
    w_off: int = 0
    b_off: int = 0
    wd_off: int = 0


@dataclass
class LNP:
    name: str
    g_off: int = 0
    b_off: int = 0


class ViTPlan:
    def __init__(self, num_keypoints: int, downsample_factor: int, D: int, depth: int, heads: int, mlp: int, patch: int, n_pos: int,
                 num_views: int = 0, arch: str = "vit", registers: int = 0, window: int = 0, global_layers: tuple[int, ...] = (),
                 carried: tuple[tuple[str, tuple[int, ...]], ...] = ()):
        self.D, self.depth, self.heads, self.mlp, self.patch, self.n_pos = D, depth, heads, mlp, patch, n_pos
        self.arch, self.registers = arch, registers
        # SAM: tensors of the reference's state_dict that nothing reads (rel_pos_*, neck.*) - (name, shape, offset) into a buffer of their
        # own, outside the flat parameter / gradient buffers and so outside every optimiser group
        self.carried, c_off = [], 0
        for name, shape in carried:
            self.carried.append((name, tuple(shape), c_off))
            c_off += -(-math.prod(shape) // 4) * 4
        self.n_carried = c_off
        pre = "backbone.vision_encoder"
        off = wd = 0
        # multi-view mode: the (V, D) view embeddings lead the flat buffers.  Their gradient is, with the other embeddings', the LAST to
        # complete in a backward pass, and grad_progress(offset) promises that G[offset:] is final - a tail position would break that;
        # in front of the backbone range each of the three optimiser groups is still one contiguous range
        self.num_views, self.view_off = num_views, off
        off += num_views * D
        self.n_view = off

        def lin(name, N, K):
            nonlocal off, wd
            l = Lin(name, N, K, off, off + N * K, wd)
            off += N * K + N
            wd += N * K
            return l

        def ln(name):
            nonlocal off
            l = LNP(name, off, off + D)
            off += 2 * D
            return l

        def vec():
            nonlocal off
            off += D
            return off - D

        self.cls_off = None if arch == "sam" else vec()   # (SAM: no [CLS] token - the tokens are the patches)
        # DINOv2 (transformers Dinov2Model): embeddings.mask_token (1, D), which the forward pass never reads, and per layer the two
        # LayerScale vectors - all inside the backbone's range, each layer's own parameters still one contiguous run (grad_progress)
        self.mask_off = vec() if arch in ("dinov2", "dinov3") else None
        # DINOv3 (transformers DINOv3ViTModel): R register tokens behind [CLS], no position table at all (n_pos = 0), the Conv2d of the patch
        # embedding without a ``.projection`` level, ``model.layer.{i}`` / ``up_proj`` / ``down_proj`` / ``norm``
        self.reg_off = off
        off += registers * D
        self.pos_off = off
        off += n_pos * D
        # SAM (transformers SamVisionEncoder): ``pos_embed`` (1, g, g, D) at the fine-tuning grid (n_pos = g * g, no [CLS] row), ``patch_embed``,
        # ``layers.{i}`` with ONE fused ``attn.qkv`` Linear (columns [q | k | v], head h at h * 64: the fused layout of every arch here),
        # ``mlp.lin1`` / ``lin2``, and no final LayerNorm; "window": the layer's attention window (0: global)
        patch_name = {"dinov3": "embeddings.patch_embeddings", "sam": "patch_embed.projection"}.get(arch, "embeddings.patch_embeddings.projection")
        self.patch_lin = lin(f"{pre}.{patch_name}", D, 3 * patch * patch)
        self.layers = []
        for i in range(depth):
            if arch == "sam":
                p = f"{pre}.layers.{i}"
                self.layers.append(dict(
                    ln1=ln(f"{p}.layer_norm1"), qkv=lin(f"{p}.attn.qkv", 3 * D, D), proj=lin(f"{p}.attn.proj", D, D),
                    ln2=ln(f"{p}.layer_norm2"), fc1=lin(f"{p}.mlp.lin1", mlp, D), fc2=lin(f"{p}.mlp.lin2", D, mlp),
                    window=0 if i in global_layers else window))
                continue
            if arch == "dinov3":
                p = f"{pre}.model.layer.{i}"
                self.layers.append(dict(
                    ln1=ln(f"{p}.norm1"), qkv=lin(f"{p}.attention.qkv", 3 * D, D), proj=lin(f"{p}.attention.o_proj", D, D),
                    ls1=vec(), ln2=ln(f"{p}.norm2"), fc1=lin(f"{p}.mlp.up_proj", mlp, D), fc2=lin(f"{p}.mlp.down_proj", D, mlp), ls2=vec()))
                continue
            if arch == "dinov2":
                p = f"{pre}.encoder.layer.{i}"
                self.layers.append(dict(
                    ln1=ln(f"{p}.norm1"), qkv=lin(f"{p}.attention.attention.qkv", 3 * D, D), proj=lin(f"{p}.attention.output.dense", D, D),
                    ls1=vec(), ln2=ln(f"{p}.norm2"), fc1=lin(f"{p}.mlp.fc1", mlp, D), fc2=lin(f"{p}.mlp.fc2", D, mlp), ls2=vec()))
                continue
            p = f"{pre}.layers.{i}"
            self.layers.append(dict(
                ln1=ln(f"{p}.layernorm_before"), qkv=lin(f"{p}.attention.qkv", 3 * D, D), proj=lin(f"{p}.attention.o_proj", D, D),
                ln2=ln(f"{p}.layernorm_after"), fc1=lin(f"{p}.mlp.fc1", mlp, D), fc2=lin(f"{p}.mlp.fc2", D, mlp)))
        self.lnf = None if arch == "sam" else ln(f"{pre}.norm" if arch == "dinov3" else f"{pre}.layernorm")
        self.n_backbone = off
        self.head: list[ConvP] = build_head(D, patch, num_keypoints, downsample_factor)
        self.convs: list[ConvP] = list(self.head)
        self.n_total, self.n_wd = place_head(self.head, off, wd)
        self.n_running = 0

    def group_ranges(self) -> dict[str, tuple[int, int]]:
        """optimiser group name -> its range of the flat buffers (optim.FusedAdam)"""
        ranges = {"backbone": (self.n_view, self.n_backbone), "head": (self.n_backbone, self.n_total)}
        if self.num_views:
            ranges["view_embeddings"] = (0, self.n_view)
        return ranges

    def linears(self) -> list[Lin]:
        out = [self.patch_lin]
        for L in self.layers:
            out += [L["qkv"], L["proj"], L["fc1"], L["fc2"]]
        return out

    def norms(self) -> list[LNP]:
        out = []
        for L in self.layers:
            out += [L["ln1"], L["ln2"]]
        return out + ([self.lnf] if self.lnf is not None else [])


class ViTEngine(EngineCore):
    """ViT-S/16 defaults = facebook/dino-vits16 (hidden 384, 12 layers, 6 heads, MLP 1536, patch 16, 224-px position table).

    ``num_views`` = V > 0 selects the multi-view mode (reference models/heatmap_tracker_multiview.py:143-223, ``forward_vit``): the batch is
    B * V images, row b * V + v view v of sample b; the tokens carry no [CLS] row but a learned ``view_embeddings[v]`` (V, D), and the layers
    attend over the V * Np tokens of a sample at once (``lp_vit_mv_tokens_fwd`` / ``_bwd``; everything after the token assembly is the same
    kernels with B sequences of V * Np tokens).  ``cls_token`` and row 0 of the position table stay in the state dict with a zero gradient.

    ``arch="dinov2"`` is transformers' ``Dinov2Model`` (the reference's ``VisionEncoderDino``, models/backbones/vit_dino.py, behind
    "vits_dinov2" / "vitb_dinov2"; its 14-px patch projection arrives resampled to 16 px, models/backbones/dinov2.py): the same layers with
    a LayerScale on each branch output, LayerNorm eps 1e-6, a ``mask_token`` parameter the forward pass never reads, and that model's
    parameter names.  LayerScale costs no launch: ``lp_layernorm_ls_fwd`` scales the branch output inside the residual add,
    ``lp_layernorm_ls_bwd`` emits the scaled gradient, its column sums and the scale's own gradient; the tape keeps the two
    unscaled branch outputs of every layer for the latter.  Single-view only.

    ``arch="dinov3"`` is transformers' ``DINOv3ViTModel`` ("vits_dinov3" / "vitb_dinov3"): DINOv2's layers (LayerScale, eps 1e-5)
    with ``registers`` register tokens behind [CLS] (``lp_vit_reg_tokens_*``; the final LayerNorm drops the 1 + R prefix rows,
    ``lp_layernorm_ls_*_px``), NO position table - the patch tokens' queries and keys are rotated instead (``lp_rope_fwd`` on the fused qkv
    tensor of every layer, ``lp_rope_bwd`` on its gradient) - and no key bias: the key third of the fused bias vector is a slot that is not a
    parameter and stays exactly 0.  ``pretrain_grid`` does not apply (there is no table to resize) and must be left unset.  In a training
    forward the patch coordinates are drawn anew per part of the pass (``pos_embed_shift`` / ``_jitter`` / ``_rescale``, the released
    configs' rescale 2.0 by default) from the engine's own seeded generator; ``forward(..., rope=draws)`` replays given draws, and
    ``tape.meta["rope"]`` holds the ones a pass used.  Single-view only.

    ``arch="sam"`` is transformers' ``SamVisionEncoder`` as the reference's ``VisionEncoderSam`` runs it ("vitb_sam"):
    relative positions off, the neck skipped, ``pos_embed`` at exactly the fine-tuning grid (``image_size`` // patch squared - any other
    input size is an error), LayerNorm eps 1e-6, no [CLS] token and no final LayerNorm (``lp_vit_pos_tokens_*``, ``lp_resid_out_*``).
    Every layer outside ``global_layers`` attends inside ``window`` x ``window`` windows of the zero-padded token grid:
    ``lp_window_partition`` gathers the fused qkv tensor into B * nW sequences of window^2 tokens - pad rows hold the qkv bias, which is
    what a padded (zero) token projects to, and take part in the soft-max - the attention kernels run on those, ``lp_window_unpartition``
    scatters the result back; backward the same two moves on d_attn and dqkv, the pad rows' dK / dV summed into the qkv bias gradient.
    ``rel_pos_h`` / ``rel_pos_w`` of every layer ((2 * window - 1, 64), global layers (2 * ``pretrain_grid`` - 1, 64)) and ``neck.*``
    (``neck_channels``) are in the reference's state_dict although nothing reads them: they are carried in a buffer of their own - in
    ``state_dict()``, absent from ``grad_views()`` and the optimiser's ranges.  Single-view only."""

    # A/B switches (EngineCore.SWITCHES).  bias_fused: every LayerNorm / GELU backward leaves the column sums that are the next Linear
    # layer's bias gradient (0: the weight-gradient launches take them).  gelu_fused: GELU inside fc1's store pass and fc2's data gradient
    # (round 6); "bwd": only the latter; "0": neither - lp_gelu_fwd / lp_gemm_nt, then lp_gelu_bwd_colsum
    SWITCHES = (("bias_fused", "LP_VIT_BIAS_FUSED", True), ("gelu_fused", "LP_VIT_GELU_FUSED", "1"))
    _patch_dtype = torch.bfloat16
    _token_kernels = ("lp_vit_tokens_fwd", "lp_vit_tokens_bwd", "lp_vit_mv_tokens_fwd", "lp_vit_mv_tokens_bwd")
    _reg_token_kernels = ("lp_vit_reg_tokens_fwd", "lp_vit_reg_tokens_bwd")
    _rope_kernels = ("lp_rope_fwd", "lp_rope_bwd")
    _ln_px_kernels = ("lp_layernorm_ls_fwd_px", "lp_layernorm_ls_bwd_px")
    _window_kernels = ("lp_window_partition", "lp_window_unpartition")
    _pos_token_kernels = ("lp_vit_pos_tokens_fwd", "lp_vit_pos_tokens_bwd")
    _act_dtype = torch.bfloat16   # of the activations between the kernels
    _elem_bytes = 2.0    # of a token row's elements (the rope and window launches' byte counts)

    def __init__(self, num_keypoints: int, downsample_factor: int = 2, device: torch.device | str = "cuda:0", hidden: int = 384,
                 depth: int = 12, heads: int = 6, mlp: int = 1536, patch: int = 16, pretrain_grid: int | None = None, num_views: int = 0,
                 arch: str = "vit", registers: int | None = None, rope_theta: float = 100.0, pos_embed_shift: float | None = None,
                 pos_embed_jitter: float | None = None, pos_embed_rescale: float | None = 2.0, rope_seed: int = 0, window: int | None = None,
                 global_layers: tuple[int, ...] | None = None, image_size: int | None = None, neck_channels: int = 256):
        if hidden % 64 or (hidden // heads) != 64 or mlp % 64:
            raise NotImplementedError("ViT widths must be multiples of 64 with 64-wide heads (ViT-S/B)")
        if num_views < 0:
            raise ValueError(f"num_views must be positive (0: single-view tokens with [CLS]), got {num_views}")
        if arch not in ("vit", "dinov2", "dinov3", "sam"):
            raise ValueError(f'arch must be "vit", "dinov2", "dinov3" or "sam", got {arch!r}')
        if arch != "vit" and num_views:
            raise NotImplementedError("the multi-view token assembly (num_views > 0) is not implemented for the "
                                      f"{ {'dinov2': 'DINOv2', 'dinov3': 'DINOv3', 'sam': 'SAM'}[arch]} backbones")
        if arch != "sam" and (window is not None or global_layers is not None or image_size is not None):
            raise ValueError(f'window / global_layers / image_size belong to arch="sam", got them with arch={arch!r}')
        carried: list[tuple[str, tuple[int, ...]]] = []
        if arch == "sam":
            if registers:
                raise ValueError(f'register tokens belong to arch="dinov3", got registers={registers} with arch="sam"')
            if image_size is None or image_size <= 0 or image_size % patch:
                raise ValueError(f'arch="sam" needs image_size, a positive multiple of the patch size {patch}: its position table is resized '
                                 f"once, to the fine-tuning grid, and trained at that size; got image_size={image_size}")
            window = 14 if window is None else int(window)
            if window < 1:
                raise ValueError(f"window must be >= 1, got {window}")
            global_layers = (2, 5, 8, 11) if global_layers is None else tuple(int(i) for i in global_layers)
            if any(not 0 <= i < depth for i in global_layers):
                raise ValueError(f"global_layers must name layers in [0, {depth}), got {global_layers}")
            registers = 0
            pretrain_grid = 64 if pretrain_grid is None else int(pretrain_grid)   # (only the shapes of the carried rel_pos_* depend on it)
            self.sam_grid = image_size // patch
            n_pos = self.sam_grid * self.sam_grid
            pre = "backbone.vision_encoder"
            for i in range(depth):
                n_rel = 2 * (pretrain_grid if i in global_layers else window) - 1
                carried += [(f"{pre}.layers.{i}.attn.rel_pos_h", (n_rel, hidden // heads)), (f"{pre}.layers.{i}.attn.rel_pos_w", (n_rel, hidden // heads))]
            nc = int(neck_channels)
            carried += [(f"{pre}.neck.conv1.weight", (nc, hidden, 1, 1)), (f"{pre}.neck.layer_norm1.weight", (nc,)),
                        (f"{pre}.neck.layer_norm1.bias", (nc,)), (f"{pre}.neck.conv2.weight", (nc, nc, 3, 3)),
                        (f"{pre}.neck.layer_norm2.weight", (nc,)), (f"{pre}.neck.layer_norm2.bias", (nc,))]
        elif arch == "dinov3":
            if pretrain_grid is not None:
                raise ValueError('arch="dinov3" has no position table (its positions are rotary): pretrain_grid does not apply')
            registers = 4 if registers is None else int(registers)
            if registers < 0:
                raise ValueError(f"registers must be >= 0, got {registers}")
            n_pos, pretrain_grid = 0, 0
        else:
            if registers:
                raise ValueError(f'register tokens belong to arch="dinov3", got registers={registers} with arch={arch!r}')
            registers = 0
            pretrain_grid = 14 if pretrain_grid is None else pretrain_grid
            n_pos = 1 + pretrain_grid * pretrain_grid
        super().__init__(ViTPlan(num_keypoints, downsample_factor, hidden, depth, heads, mlp, patch, n_pos, num_views, arch, registers,
                                 window=window or 0, global_layers=tuple(global_layers or ()), carried=tuple(carried)),
                         num_keypoints, downsample_factor, device)
        self.grid0 = pretrain_grid
        self.arch = arch
        self.ln_eps = {"dinov2": DINOV2_LN_EPS, "dinov3": DINOV3_LN_EPS, "sam": SAM_LN_EPS}.get(arch, LN_EPS)
        self.carried = torch.zeros(self.plan.n_carried, device=self.device, dtype=torch.float32)   # (SAM: rel_pos_* / neck.*, never read)
        # rotary positions (DINOv3): the table of a grid is built on the host with DINOv3ViTRopePositionEmbedding's own torch operations
        self.rope_theta = float(rope_theta)
        self.rope_aug = dict(shift=pos_embed_shift, jitter=pos_embed_jitter, rescale=pos_embed_rescale)
        self._rope_gen = torch.Generator().manual_seed(int(rope_seed))   # (host generator: the draws never touch the device)
        self._rope_eval: dict[tuple[int, int], torch.Tensor] = {}        # (1, Np, 64) device tables of the plain coordinates, by patch grid
        self._rope_seq: dict[tuple, torch.Tensor] = {}                   # tab_of_seq arrays, by the part sizes of a pass
        for l in self.plan.norms():
            self.P[l.g_off:l.g_off + hidden] = 1.0
        for L in self.plan.layers:   # (Dinov2Config.layerscale_value = 1.0)
            for o in (L.get("ls1"), L.get("ls2")):
                if o is not None:
                    self.P[o:o + hidden] = 1.0
        self._interp: dict[tuple[int, int], torch.Tensor] = {}   # bicubic resize matrices of the position table, by patch grid
        self._wg_shape = (0, 0)   # (sequences, tokens) of the pass in flight: the image geometry _linear_bwd gives the weight-gradient kernel

    # ------------------------------------------------------------------------------------------------ params
    def _views(self, buf: torch.Tensor) -> dict[str, torch.Tensor]:
        pl, D = self.plan, self.plan.D
        pre = "backbone.vision_encoder"
        sd = {"view_embeddings": buf[pl.view_off:pl.n_view].view(pl.num_views, D)} if pl.num_views else {}
        if pl.cls_off is not None:
            sd[f"{pre}.embeddings.cls_token"] = buf[pl.cls_off:pl.cls_off + D].view(1, 1, D)
        if pl.mask_off is not None:
            sd[f"{pre}.embeddings.mask_token"] = buf[pl.mask_off:pl.mask_off + D].view(*((1, 1, D) if pl.arch == "dinov3" else (1, D)))
        if pl.arch == "sam":
            sd[f"{pre}.pos_embed"] = buf[pl.pos_off:pl.pos_off + pl.n_pos * D].view(1, self.sam_grid, self.sam_grid, D)
        elif pl.arch == "dinov3":
            sd[f"{pre}.embeddings.register_tokens"] = buf[pl.reg_off:pl.reg_off + pl.registers * D].view(1, pl.registers, D)
        else:
            sd[f"{pre}.embeddings.position_embeddings"] = buf[pl.pos_off:pl.pos_off + pl.n_pos * D].view(1, pl.n_pos, D)
        for l in pl.linears():
            w, b = buf[l.w_off:l.w_off + l.N * l.K], buf[l.b_off:l.b_off + l.N]
            if l.name.endswith("attention.qkv"):  # fused [q; k; v]: three reference parameters share one GEMM weight
                stem = l.name[:-len("qkv")]
                for j, nm in enumerate(("query", "key", "value") if pl.arch == "dinov2" else ("q_proj", "k_proj", "v_proj")):
                    sd[f"{stem}{nm}.weight"] = w[j * D * D:(j + 1) * D * D].view(D, D)
                    if pl.arch == "dinov3" and j == 1:
                        continue   # key_bias=False: that third of the fused bias vector is a slot, not a parameter - it stays 0 (_clear_key_bias)
                    sd[f"{stem}{nm}.bias"] = b[j * D:(j + 1) * D]
            elif l is pl.patch_lin:
                sd[f"{l.name}.weight"] = w.view(D, 3, pl.patch, pl.patch)
                sd[f"{l.name}.bias"] = b
            else:
                sd[f"{l.name}.weight"] = w.view(l.N, l.K)
                sd[f"{l.name}.bias"] = b
        for l in pl.norms():
            sd[f"{l.name}.weight"] = buf[l.g_off:l.g_off + D]
            sd[f"{l.name}.bias"] = buf[l.b_off:l.b_off + D]
        if pl.arch in ("dinov2", "dinov3"):
            layer = "encoder.layer" if pl.arch == "dinov2" else "model.layer"
            for i, L in enumerate(pl.layers):
                for nm in ("1", "2"):
                    sd[f"{pre}.{layer}.{i}.layer_scale{nm}.lambda1"] = buf[L["ls" + nm]:L["ls" + nm] + D]
        sd.update(self._head_views(buf))
        return sd

    def state_dict(self) -> dict[str, torch.Tensor]:
        sd = self._views(self.P)
        for name, shape, off in self.plan.carried:   # (SAM: loaded and saved unchanged; no gradient view, no optimiser range)
            sd[name] = self.carried[off:off + math.prod(shape)].view(shape)
        return sd

    def grad_views(self) -> dict[str, torch.Tensor]:
        return self._views(self.G)

    _LEGACY = (("encoder.layer.", "layers."), ("attention.attention.query", "attention.q_proj"),
               ("attention.attention.key", "attention.k_proj"), ("attention.attention.value", "attention.v_proj"),
               ("attention.output.dense", "attention.o_proj"), ("intermediate.dense", "mlp.fc1"), ("output.dense", "mlp.fc2"))

    @classmethod
    def canonical_key(cls, k: str) -> str:
        """transformers 4.x ViT parameter name -> the 5.x name used here (checkpoints saved by older reference installs)"""
        if ".encoder.layer." in k:
            for a, b in cls._LEGACY:
                k = k.replace(a, b)
        return k

    @torch.no_grad()
    def load_state_dict(self, sd: dict[str, torch.Tensor], strict: bool = True) -> None:
        if self.arch == "vit":   # (Dinov2Model's own names are the 4.x-style ones, DINOv3ViTModel's are its own: nothing to translate)
            sd = {self.canonical_key(k): v for k, v in sd.items()}
        EngineCore.load_state_dict(self, sd, strict)

    def refresh_dgrad_copies(self, lo: int = 0, hi: int | None = None) -> None:
        hi = self.plan.n_total if hi is None else hi
        for l in self.plan.linears():
            if lo <= l.w_off < hi:  # [N][K] -> [K][N]
                check(self._lib.lp_permute_cba(_p(self.Wb[l.w_off:]), l.N, 1, l.K, _p(self.Wd[l.wd_off:]), ops._stream()), "lp_permute_cba")
        EngineCore.refresh_dgrad_copies(self, lo, hi)   # (the head's convolutions)

    # ------------------------------------------------------------------------------------------------ kernels
    def _gemm(self, a, lda, b, ldb, M, N, K, out, ldc, n_store=0, bias=None, batch=None):
        gb = _lib.GemmBatch(*batch) if batch is not None else None
        check(self._lib.lp_gemm_nt(a, lda, b, ldb, _p(out), None, ldc, M, N, K, n_store, _p(bias), C.byref(gb) if gb else None,
                                   ops._stream()), "lp_gemm_nt")

    def _gemm_tn(self, x, ldx, y, ldy, M, J, N, out, ldo, batch):
        """out[z][j][n] = sum_m x[z][m][j] y[z][m][n] (both operands contracted over their rows; no transposed copies)"""
        gb = _lib.GemmBatch(*batch)
        check(self._lib.lp_gemm_tn(x, ldx, y, ldy, _p(out), ldo, M, J, N, C.byref(gb), ops._stream()), "lp_gemm_tn")

    def _linear(self, x: torch.Tensor, l: Lin, M: int) -> torch.Tensor:
        out = torch.empty(M, l.N, device=self.device, dtype=torch.bfloat16)
        self._timed("lp_gemm_nt<linear fwd>", 2.0 * M * l.N * l.K, lambda: self._gemm(
            _p(x), l.K, _p(self.Wb[l.w_off:]), l.K, M, l.N, l.K, out, l.N, bias=self.P[l.b_off:l.b_off + l.N]),
            nbytes=2.0 * (M * l.K + M * l.N + l.N * l.K))
        return out

    def _linear_gelu(self, x: torch.Tensor, l: Lin, M: int) -> tuple[torch.Tensor, torch.Tensor]:
        """(u, GELU(u)) for u = x W^T + b: one launch whose store pass writes both (lp_gemm_nt_gelu_fwd, round 6); LP_VIT_GELU_FUSED=0 or a
        shape the pipelined kernel does not tile: the Linear layer, then lp_gelu_fwd"""
        u = torch.empty(M, l.N, device=self.device, dtype=torch.bfloat16)
        act = torch.empty_like(u)
        if self.gelu_fused not in ("0", "bwd"):
            rc = self._timed("lp_gemm_nt<linear fwd+gelu>", 2.0 * M * l.N * l.K, lambda: self._lib.lp_gemm_nt_gelu_fwd(
                _p(x), _p(self.Wb[l.w_off:]), _p(self.P[l.b_off:l.b_off + l.N]), _p(u), _p(act), M, l.N, l.K, ops._stream()),
                nbytes=2.0 * (M * l.K + 2 * M * l.N + l.N * l.K))
            if rc == 0:
                return u, act
            if rc != -2:   # (LP_ERR_UNSUPPORTED)
                check(rc, "lp_gemm_nt_gelu_fwd")
        u = self._linear(x, l, M)
        check(self._lib.lp_gelu_fwd(_p(u), u.numel(), _p(act), ops._stream()), "lp_gelu_fwd")
        return u, act

    def _linear_bwd(self, l: Lin, x: torch.Tensor, dy: torch.Tensor, M: int, need_dx: bool = True, bias_done: bool = False,
                    gelu_of: tuple[torch.Tensor, torch.Tensor] | None = None):
        """bias / weight gradients into G; returns dX = dY W (bf16) if wanted.  ``bias_done``: the kernel that produced ``dy`` already left its
        column sums in G (lp_gelu_bwd_colsum / lp_layernorm_bwd_bf16_colsum), so the weight gradient runs without the bias pass - which lets the
        pipelined weight-gradient kernel take it."""
        rows, cols = self._wg_shape
        g = _lib.ConvGeom(1, rows, cols, l.K, rows, cols, l.N, 1, 1, 1, 0) if rows * cols == M else _lib.ConvGeom(1, 1, M, l.K, 1, M, l.N, 1, 1, 1, 0)
        # bias gradient = column sums of dy, same pass
        self._timed("conv_wgrad_kernel<linear wgrad" + ("" if bias_done else "+bias") + ">", 2.0 * M * l.N * l.K,
                    lambda: self._wgrad(x, dy, g, self.G[l.w_off:], dbias=None if bias_done else self.G[l.b_off:]),
                    nbytes=2.0 * (M * l.K + M * l.N) + 4.0 * l.N * l.K)
        if not need_dx:
            return None
        dx = torch.empty(M, l.K, device=self.device, dtype=torch.bfloat16)
        if gelu_of is not None:
            # this layer's input is GELU(u): the data gradient leaves the store pass as the gradient of u (lp_gemm_nt_gelu_bwd), its column sums
            # - the bias gradient of the layer that produced u - as fixed-point totals; a shape the pipelined kernel does not tile: two passes
            u, dbias_u = gelu_of
            sums = torch.zeros(4 * l.K, device=self.device, dtype=torch.int64)
            rc = self._timed("lp_gemm_nt<linear dgrad+gelu>", 2.0 * M * l.N * l.K, lambda: self._lib.lp_gemm_nt_gelu_bwd(
                _p(dy), _p(self.Wd[l.wd_off:]), _p(u), _p(dx), M, l.K, l.N, _p(sums), ops._stream()),
                nbytes=2.0 * (2 * M * l.K + M * l.N + l.N * l.K))
            if rc == 0:
                check(self._lib.lp_fxsum_accumulate(_p(sums), l.K, _p(dbias_u), ops._stream()), "lp_fxsum_accumulate")
                return dx
            if rc != -2:   # (LP_ERR_UNSUPPORTED, include/lp_hip.h: a shape outside the pipelined tiles)
                check(rc, "lp_gemm_nt_gelu_bwd")
            d_a = torch.empty_like(dx)
            self._gemm(_p(dy), l.N, _p(self.Wd[l.wd_off:]), l.N, M, l.K, l.N, d_a, l.K)
            check(self._lib.lp_gelu_bwd_colsum(_p(u), _p(d_a), M, l.K, _p(dx), _p(dbias_u), ops._stream()), "lp_gelu_bwd_colsum")
            return dx
        self._timed("lp_gemm_nt<linear dgrad>", 2.0 * M * l.N * l.K, lambda: self._gemm(_p(dy), l.N, _p(self.Wd[l.wd_off:]), l.N, M, l.K, l.N, dx, l.K),
                    nbytes=2.0 * (M * l.K + M * l.N + l.N * l.K))
        return dx

    def _ln(self, x, delta, l: LNP, M: int, drop_T: int = 0, ls: int | None = None, n_prefix: int = 1):
        """``ls``: offset of the LayerScale vector that scales ``delta`` in front of the residual add (DINOv2, DINOv3);
        ``n_prefix``: leading rows of every ``drop_T`` that do not reach y ([CLS]; DINOv3: [CLS] and the registers)"""
        D = self.plan.D
        xo = torch.empty_like(x) if delta is not None else None
        rows = M - (M // drop_T) * n_prefix if drop_T else M
        y = torch.empty(rows, D, device=self.device, dtype=torch.bfloat16)
        mean = torch.empty(M, device=self.device, dtype=torch.float32)
        rstd = torch.empty_like(mean)
        if drop_T and n_prefix != 1:   # (only the LayerScale walk has the prefix-taking form: every model with registers has LayerScale)
            assert ls is not None and delta is not None
            fwd = self._ln_px_kernels[0]
            check(getattr(self._lib, fwd)(_p(x), _p(delta), _p(self.P[ls:]), _p(xo), _p(self.P[l.g_off:]), _p(self.P[l.b_off:]), self.ln_eps, M, D,
                                          drop_T, n_prefix, _p(y), _p(mean), _p(rstd), ops._stream()), fwd)
            return y, mean, rstd, xo
        if ls is not None and delta is not None:
            check(self._lib.lp_layernorm_ls_fwd(_p(x), _p(delta), _p(self.P[ls:]), _p(xo), _p(self.P[l.g_off:]), _p(self.P[l.b_off:]), self.ln_eps,
                                                M, D, drop_T, _p(y), _p(mean), _p(rstd), ops._stream()), "lp_layernorm_ls_fwd")
            return y, mean, rstd, xo
        check(self._lib.lp_layernorm_fwd(_p(x), _p(delta), _p(xo), _p(self.P[l.g_off:]), _p(self.P[l.b_off:]), self.ln_eps, M, D, drop_T, _p(y),
                                         _p(mean), _p(rstd), ops._stream()), "lp_layernorm_fwd")
        return y, mean, rstd, (xo if xo is not None else x)

    def _ln_bwd(self, dy, x, mean, rstd, l: LNP, M: int, dx, drop_T: int = 0, want_bf16: bool = False, colsum: torch.Tensor | None = None,
                ls: int | None = None, branch: torch.Tensor | None = None, n_prefix: int = 1):
        """dx (fp32, the residual stream's gradient) += LayerNorm backward of dy; ``want_bf16``: also return the updated dx in bf16;
        ``colsum``: accumulate that bf16 tensor's column sums there (the bias gradient of the Linear layer it is the dy of);
        ``ls`` / ``branch`` (DINOv2): the returned tensor feeds a branch through the LayerScale vector at offset ``ls`` - it leaves scaled, and
        the scale's gradient (against ``branch``, that branch's unscaled forward output) is accumulated into G"""
        if drop_T and n_prefix != 1:
            assert want_bf16 and ls is not None
            bwd = self._ln_px_kernels[1]
            out = torch.empty(M, self.plan.D, device=self.device, dtype=torch.bfloat16)
            check(getattr(self._lib, bwd)(_p(dy), _p(x), _p(mean), _p(rstd), _p(self.P[l.g_off:]), _p(self.P[ls:]), _p(branch), M, self.plan.D,
                                          drop_T, n_prefix, _p(dx), _p(out), _p(self.G[l.g_off:]), _p(self.G[l.b_off:]), _p(colsum),
                                          _p(self.G[ls:]), ops._stream()), bwd)
            return out
        if want_bf16 and ls is not None:
            out = torch.empty(M, self.plan.D, device=self.device, dtype=torch.bfloat16)
            check(self._lib.lp_layernorm_ls_bwd(_p(dy), _p(x), _p(mean), _p(rstd), _p(self.P[l.g_off:]), _p(self.P[ls:]), _p(branch), M, self.plan.D,
                                                drop_T, _p(dx), _p(out), _p(self.G[l.g_off:]), _p(self.G[l.b_off:]), _p(colsum), _p(self.G[ls:]),
                                                ops._stream()), "lp_layernorm_ls_bwd")
            return out
        if want_bf16 and colsum is not None:
            out = torch.empty(M, self.plan.D, device=self.device, dtype=torch.bfloat16)
            check(self._lib.lp_layernorm_bwd_bf16_colsum(_p(dy), _p(x), _p(mean), _p(rstd), _p(self.P[l.g_off:]), M, self.plan.D, drop_T, _p(dx),
                                                         _p(out), _p(self.G[l.g_off:]), _p(self.G[l.b_off:]), _p(colsum), ops._stream()),
                  "lp_layernorm_bwd_bf16_colsum")
            return out
        if not want_bf16:
            check(self._lib.lp_layernorm_bwd(_p(dy), _p(x), _p(mean), _p(rstd), _p(self.P[l.g_off:]), M, self.plan.D, drop_T, _p(dx),
                                             _p(self.G[l.g_off:]), _p(self.G[l.b_off:]), ops._stream()), "lp_layernorm_bwd")
            return None
        out = torch.empty(M, self.plan.D, device=self.device, dtype=torch.bfloat16)
        check(self._lib.lp_layernorm_bwd_bf16(_p(dy), _p(x), _p(mean), _p(rstd), _p(self.P[l.g_off:]), M, self.plan.D, drop_T, _p(dx), _p(out),
                                              _p(self.G[l.g_off:]), _p(self.G[l.b_off:]), ops._stream()), "lp_layernorm_bwd_bf16")
        return out

    def _transpose(self, src_ptr, R, Cc, ldi, in_b, in_h, out, ldo, out_b, out_h, nb, nh):
        check(self._lib.lp_transpose_batched(src_ptr, R, Cc, ldi, in_b, in_h, _p(out), ldo, out_b, out_h, nb, nh, ops._stream()),
              "lp_transpose_batched")

    def _pos(self, gh: int, gw: int) -> torch.Tensor:
        """(1 + gh*gw, D) position embeddings: the [CLS] row + the pretraining grid resized bicubically (HF interpolate_pos_encoding)"""
        pl, D = self.plan, self.plan.D
        pos = self.P[pl.pos_off:pl.pos_off + pl.n_pos * D].view(pl.n_pos, D)
        if pl.arch == "sam":   # (gh * gw, D), no [CLS] row: the table IS the fine-tuning grid (_forward refuses every other input size)
            return pos
        if gh == self.grid0 and gw == self.grid0:
            return pos
        key = (gh, gw)
        if key not in self._interp:
            w = np.kron(bicubic_matrix(self.grid0, gh), bicubic_matrix(self.grid0, gw)).astype(np.float32)
            self._interp[key] = torch.from_numpy(w).to(self.device).contiguous()
        out = torch.empty(1 + gh * gw, D, device=self.device, dtype=torch.float32)
        out[0].copy_(pos[0])
        check(self._lib.lp_small_matmul(_p(self._interp[key]), _p(pos[1:]), gh * gw, pl.n_pos - 1, D, 0, 0, _p(out[1:]), ops._stream()),
              "lp_small_matmul")
        return out

    # ------------------------------------------------------------------------------------------------ rotary positions (DINOv3)
    def rope_draw(self) -> dict[str, torch.Tensor]:
        """One draw of the training-mode coordinate augmentation (transformers ``augment_patches_center_coordinates``: a shift per axis, a
        log-uniform factor per axis, one log-uniform factor) from the engine's generator, as float32 host tensors; only the knobs that are set"""
        a, g, d = self.rope_aug, self._rope_gen, {}
        if a["shift"] is not None:
            d["shift"] = torch.empty(1, 2).uniform_(-a["shift"], a["shift"], generator=g)
        if a["jitter"] is not None:
            r = float(np.log(a["jitter"]))
            d["jitter"] = torch.empty(1, 2).uniform_(-r, r, generator=g).exp()
        if a["rescale"] is not None:
            r = float(np.log(a["rescale"]))
            d["rescale"] = torch.empty(1).uniform_(-r, r, generator=g).exp()
        return d

    def rope_table_host(self, gh: int, gw: int, draw: dict[str, torch.Tensor] | None = None) -> torch.Tensor:
        """(gh * gw, 64) float32 on the host, per patch cos[0:32] | sin[0:32]: the 32 distinct columns of DINOv3ViTRopePositionEmbedding's
        (cos, sin), computed with its own torch operations in its own order (patch centres in [-1, 1], the draw's shift / jitter / rescale,
        angle = 2 pi * coordinate * inv_freq, [y angles | x angles]) - without a draw it is bit-equal to the HF module's eval output"""
        hd = self.plan.D // self.plan.heads
        inv_freq = 1 / self.rope_theta ** torch.arange(0, 1, 4 / hd, dtype=torch.float32)
        ch = torch.arange(0.5, gh, dtype=torch.float32) / gh
        cw = torch.arange(0.5, gw, dtype=torch.float32) / gw
        coords = 2.0 * torch.stack(torch.meshgrid(ch, cw, indexing="ij"), dim=-1).flatten(0, 1) - 1.0
        if draw:
            if draw.get("shift") is not None:
                coords = coords + draw["shift"]
            if draw.get("jitter") is not None:
                coords = coords * draw["jitter"]
            if draw.get("rescale") is not None:
                coords = coords * draw["rescale"]
        angles = (2 * math.pi * coords[:, :, None] * inv_freq[None, None, :]).flatten(1, 2)
        return torch.cat((torch.cos(angles), torch.sin(angles)), dim=1).contiguous()

    def _rope_tables(self, gh: int, gw: int, sizes: list[int], training: bool, rope):
        """(device table (n_tab, Np, 64), tab_of_seq or None, n_tab, the draws or None) of a pass over batches of ``sizes`` images: the cached
        plain table, or - a training forward with a knob set, or draws to replay - one table per part, built on the host and copied without
        blocking; nothing is read back"""
        if self.arch != "dinov3":
            return None, None, 0, None
        if rope is None and not (training and any(v is not None for v in self.rope_aug.values())):
            if (gh, gw) not in self._rope_eval:
                self._rope_eval[(gh, gw)] = self.rope_table_host(gh, gw)[None].to(self.device)
            return self._rope_eval[(gh, gw)], None, 1, None
        draws = [self.rope_draw() for _ in sizes] if rope is None else list(rope)
        if len(draws) != len(sizes):
            raise ValueError(f"rope= holds {len(draws)} draws for a pass of {len(sizes)} part(s)")
        host = torch.stack([self.rope_table_host(gh, gw, d) for d in draws])
        key = tuple(sizes)
        if key not in self._rope_seq:
            self._rope_seq[key] = torch.tensor([i for i, n in enumerate(sizes) for _ in range(n)], dtype=torch.int32).to(self.device)
        if self.device.type == "cuda":
            host = host.pin_memory()
        return host.to(self.device, non_blocking=True), self._rope_seq[key], len(draws), draws

    def _rope(self, bwd: int, t: torch.Tensor, ld: int, tab: torch.Tensor, seq: torch.Tensor | None, n_tab: int, Bs: int, Tn: int) -> None:
        """rotate the Q and K columns of the patch rows of the fused (M, 3 D) tensor ``t`` in place (``bwd``: the transposed rotation)"""
        D, nh, name = self.plan.D, self.plan.heads, self._rope_kernels[bwd]
        n = float(Bs * (Tn - self.n_prefix) * 2 * D)      # elements rotated: 2 products + 1 sum each, read once and written once
        self._timed(name, 3.0 * n, lambda: check(getattr(self._lib, name)(
            _p(t), ld, D, _p(tab), _p(seq), n_tab, Bs, Tn, self.n_prefix, nh, D // nh, ops._stream()), name), nbytes=2.0 * n * self._elem_bytes)

    def _clear_key_bias(self, l: Lin) -> None:
        """DINOv3 has no key bias: the key third of the fused bias vector is not a parameter.  Under the rotation a key bias would NOT be
        invisible to the soft-max, so the column sums the weight-gradient pass leaves there are non-zero - cleared here, before the layer's
        gradients are announced (grad_progress), so that the optimiser leaves the slot at exactly 0"""
        if self.wgrad_side_stream:
            self._join_side_stream()
        D = self.plan.D
        self.G[l.b_off + D:l.b_off + 2 * D].zero_()

    # ------------------------------------------------------------------------------------------------ windows (SAM)
    @staticmethod
    def window_rows(B: int, gh: int, gw: int, ws: int) -> tuple[int, int]:
        """(sequences, tokens per sequence) of a window layer: B * nW windows of ws * ws tokens over the zero-padded grid"""
        return B * (-(-gh // ws)) * (-(-gw // ws)), ws * ws

    def _qkv_pad_fill(self, l: Lin) -> torch.Tensor:
        """what the qkv Linear's store pass writes for an all-zero input row: the bias, rounded as that pass rounds it (the operand copy)"""
        return self.Wb[l.b_off:l.b_off + l.N]

    def _win_part(self, t: torch.Tensor, ld: int, cols: int, B: int, gh: int, gw: int, ws: int, fill: torch.Tensor | None) -> torch.Tensor:
        """grid layout (B * gh * gw rows, pitch ``ld``) -> window layout (B * nW * ws^2, cols); pad rows = ``fill`` (None: zeros)"""
        nseq, nt = self.window_rows(B, gh, gw, ws)
        out = torch.empty(nseq * nt, cols, device=self.device, dtype=self._act_dtype)
        name = self._window_kernels[0]
        self._timed("window_partition_kernel", 0.0, lambda: check(getattr(self._lib, name)(
            _p(t), ld, B, gh, gw, ws, cols, _p(fill), _p(out), ops._stream()), name),
            nbytes=self._elem_bytes * cols * (B * gh * gw + nseq * nt))   # real rows read once, every window row written once
        return out

    def _win_unpart(self, tw: torch.Tensor, cols: int, B: int, gh: int, gw: int, ws: int, pad_colsum: torch.Tensor | None = None) -> torch.Tensor:
        """window layout -> grid layout (B * gh * gw, cols); ``pad_colsum``: the pad rows' column sums are ADDED there (fp32)"""
        nseq, nt = self.window_rows(B, gh, gw, ws)
        out = torch.empty(B * gh * gw, cols, device=self.device, dtype=self._act_dtype)
        name = self._window_kernels[1]
        rows_read = nseq * nt if pad_colsum is not None else B * gh * gw
        self._timed("window_unpartition_kernel", 0.0, lambda: check(getattr(self._lib, name)(
            _p(tw), B, gh, gw, ws, cols, _p(out), cols, _p(pad_colsum), ops._stream()), name),
            nbytes=self._elem_bytes * cols * (rows_read + B * gh * gw))
        return out

    # ------------------------------------------------------------------------------------------------ tokens
    def _seq(self, parts: list[torch.Tensor], Np: int) -> tuple[int, int, int]:
        """(sequences, tokens per sequence, ``drop_T`` of the final LayerNorm) for these batches of images with Np patches each"""
        V = self.plan.num_views
        B = sum(p_.shape[0] for p_ in parts)
        if not V:   # one sequence per image, [CLS] (and DINOv3's registers: self.n_prefix rows) in front and dropped in front of the head
            return B, Np + self.n_prefix, (Np + self.n_prefix if self.n_prefix else 0)   # (SAM: no prefix, no final LayerNorm)
        if any(p_.shape[0] % V for p_ in parts):
            raise ValueError(f"a multi-view batch holds num_views = {V} images per sample, got {[p_.shape[0] for p_ in parts]} images")
        return B // V, V * Np, 0                # one sequence per sample: the patches of all its views, nothing dropped

    @property
    def n_prefix(self) -> int:
        """rows in front of the patch tokens of a single-view sequence: [CLS] and the register tokens (SAM: none)"""
        return 0 if self.plan.arch == "sam" else 1 + self.plan.registers

    def _tokens_fwd(self, pe: torch.Tensor, pos: torch.Tensor | None, B: int, Np: int, x: torch.Tensor) -> None:
        pl, (fwd, _, mv_fwd, _) = self.plan, self._token_kernels
        if pl.arch == "sam":   # patch embeddings + position table, no prefix rows
            fwd = self._pos_token_kernels[0]
            check(getattr(self._lib, fwd)(_p(pe), _p(pos), B, Np, pl.D, _p(x), ops._stream()), fwd)
        elif pl.arch == "dinov3":   # [CLS], the registers, the patch embeddings: nothing is added to the tokens
            fwd = self._reg_token_kernels[0]
            check(getattr(self._lib, fwd)(_p(pe), _p(self.P[pl.cls_off:]), _p(self.P[pl.reg_off:]) if pl.registers else None, B, pl.registers, Np,
                                          pl.D, _p(x), ops._stream()), fwd)
        elif pl.num_views:
            V = pl.num_views
            check(getattr(self._lib, mv_fwd)(_p(pe), _p(pos), _p(self.P[pl.view_off:]), B // V, V, Np, pl.D, _p(x), ops._stream()), mv_fwd)
        else:
            check(getattr(self._lib, fwd)(_p(pe), _p(self.P[pl.cls_off:]), _p(pos), B, Np, pl.D, _p(x), ops._stream()), fwd)

    def _tokens_bwd(self, dx: torch.Tensor, B: int, Np: int, gh: int, gw: int) -> torch.Tensor:
        """Gradient of the token assembly: returns d(patch embeddings) and accumulates the [CLS] token's / the view embeddings' and the
        position table's gradients (through the adjoint of its interpolation) into G"""
        pl, D, dev = self.plan, self.plan.D, self.device
        _, bwd, _, mv_bwd = self._token_kernels
        dpatch = torch.empty(B * Np, D, device=dev, dtype=self._patch_dtype)
        if pl.arch == "sam":   # the kernel WRITES the sums over the images; added to G here, at the table's own grid (nothing to interpolate)
            bwd = self._pos_token_kernels[1]
            dpos = torch.empty(Np, D, device=dev, dtype=torch.float32)
            check(getattr(self._lib, bwd)(_p(dx), B, Np, D, _p(dpatch), _p(dpos), ops._stream()), bwd)
            self.G[pl.pos_off:pl.pos_off + Np * D] += dpos.view(-1)
            return dpatch
        if pl.arch == "dinov3":   # the kernel WRITES the sums over the images; they are added to G here (a backward pass accumulates)
            R, bwd = pl.registers, self._reg_token_kernels[1]
            dpre = torch.empty(1 + R, D, device=dev, dtype=torch.float32)
            check(getattr(self._lib, bwd)(_p(dx), B, R, Np, D, _p(dpatch), _p(dpre), _p(dpre[1:]) if R else None, ops._stream()), bwd)
            self.G[pl.cls_off:pl.cls_off + D] += dpre[0]
            if R:
                self.G[pl.reg_off:pl.reg_off + R * D] += dpre[1:].reshape(-1)
            return dpatch
        dpos = torch.empty(Np + 1, D, device=dev, dtype=torch.float32)
        gpos = self.G[pl.pos_off:pl.pos_off + pl.n_pos * D].view(pl.n_pos, D)
        if pl.num_views:   # no [CLS] row: cls_token and gpos[0] keep their zero gradient
            V = pl.num_views
            dview = torch.empty(V, D, device=dev, dtype=torch.float32)
            nws = int(self._lib.lp_vit_mv_tokens_bwd_workspace_bytes(B // V, V, Np, D))
            ws = torch.empty(max(nws, 4) // 4, device=dev, dtype=torch.float32)
            check(getattr(self._lib, mv_bwd)(_p(dx), B // V, V, Np, D, _p(dpatch), _p(dpos), _p(dview), _p(ws), nws, ops._stream()), mv_bwd)
            self.G[pl.view_off:pl.n_view] += dview.view(-1)
        else:
            check(getattr(self._lib, bwd)(_p(dx), B, Np, D, _p(dpatch), _p(dpos), ops._stream()), bwd)
            self.G[pl.cls_off:pl.cls_off + D] += dpos[0]
            gpos[0] += dpos[0]
        if gh == self.grid0 and gw == self.grid0:
            gpos[1:] += dpos[1:]
        else:
            check(self._lib.lp_small_matmul(_p(self._interp[(gh, gw)]), _p(dpos[1:]), Np, pl.n_pos - 1, D, 1, 1, _p(gpos[1:]), ops._stream()),
                  "lp_small_matmul(adjoint)")
        return dpatch

    # ------------------------------------------------------------------------------------------------ forward
    def can_segment(self, n0: int, H: int, W: int) -> bool:
        """no batch statistics anywhere (LayerNorm is per token): two batches of equally sized images always share one pass"""
        return n0 > 0

    def forward(self, images, training: bool = True, rope=None) -> tuple[torch.Tensor, Tape]:
        """``images``: a tensor, or a pair (labeled, unlabeled frames) that runs as one batch.  ``rope`` (DINOv3): the coordinate draws to
        use, one dict per part as ``tape.meta["rope"]`` holds them, instead of new ones"""
        return self._forward(images, training, keep=True, rope=rope)

    def forward_infer(self, images: torch.Tensor) -> torch.Tensor:
        """Inference forward (predict_step under eval + no_grad): the attention probabilities are never written (lp_attn_fwd with
        p = NULL drops the 2 x 0.85 GB per layer the training pass stores for its backward) and no tape is kept."""
        return self._forward(images, False, keep=False)[0]

    def _forward(self, images, training: bool, keep: bool, rope=None) -> tuple[torch.Tensor, Tape]:
        pl = self.plan
        D, nh, pt = pl.D, pl.heads, pl.patch
        parts, B, H, W = image_parts(images, pt, None, of="the patch size ")
        gh, gw = H // pt, W // pt
        self._check_sam_input(H, W)
        Np = gh * gw
        Bs, Tn, drop_T = self._seq(parts, Np)   # (B images; the layers see Bs sequences of Tn tokens)
        M = Bs * Tn
        tp = Tape()
        T = tp.t
        dev = self.device
        self._wg_shape = (Bs, Tn)

        patches = torch.empty(B * Np, 3 * pt * pt, device=dev, dtype=torch.bfloat16)
        i0 = 0
        for p_ in parts:
            check(self._lib.lp_vit_patchify(_p(p_), p_.shape[0], H, W, pt, _p(patches[i0 * Np:]), ops._stream()), "lp_vit_patchify")
            i0 += p_.shape[0]
        pe = self._linear(patches, pl.patch_lin, B * Np)
        x = torch.empty(M, D, device=dev, dtype=torch.float32)
        pos = self._pos(gh, gw) if pl.n_pos else None  # (kept alive across the launch)
        self._tokens_fwd(pe, pos, B, Np, x)
        rope_tab, rope_seq, n_tab, draws = self._rope_tables(gh, gw, [p_.shape[0] for p_ in parts], training, rope)
        if keep:
            T["patches"] = patches
            if rope_tab is not None:
                T["rope_tab"], T["rope_seq"] = rope_tab, rope_seq
        delta = None
        scale = 1.0 / math.sqrt(D // nh)
        qs = 3 * D  # row pitch of the fused qkv tensor
        for i, L in enumerate(pl.layers):
            y1, m1, r1, x = self._ln(x, delta, L["ln1"], M, ls=pl.layers[i - 1].get("ls2") if i else None)
            qkv = self._linear(y1, L["qkv"], M)
            if rope_tab is not None:   # DINOv3: the patch tokens' q and k rotated in place; the tape keeps the rotated q and k, which is
                self._rope(0, qkv, qs, rope_tab, rope_seq, n_tab, Bs, Tn)   # what lp_attn_bwd_kv and dQ = dS K need
            # SAM's window layers: the attention sees aB windows of aT tokens, gathered from the qkv tensor AFTER the GEMM - the pad rows are
            # the qkv bias, so the GEMM itself runs on the real tokens only; the tape keeps the windowed qkv (what the backward kernels read)
            ws = L.get("window", 0)
            aB, aT = self.window_rows(B, gh, gw, ws) if ws else (Bs, Tn)
            if ws:
                qkv = self._win_part(qkv, qs, qs, B, gh, gw, ws, self._qkv_pad_fill(L["qkv"]))
            Tp = -(-aT // 64) * 64
            # P = softmax(Q K^T / 8) (bf16, row pitch Tp, pad columns zero; kept for the backward pass) and attn = P V in one kernel:
            # the scores themselves never reach memory
            S = torch.empty(aB * nh * aT, Tp, device=dev, dtype=torch.bfloat16) if keep else None
            attn = torch.empty(aB * aT, D, device=dev, dtype=torch.bfloat16)
            # scores + probabilities x values: 2 products of B * nh * Tn * Tn * (D / nh) MACs; the training pass computes the scores twice
            self._timed("attn_fwd_kernel", 4.0 * aB * aT * aT * D, lambda: check(self._lib.lp_attn_fwd(
                _p(qkv), qs, D, 2 * D, aB, nh, aT, scale, _p(S), Tp, _p(attn), D, ops._stream()), "lp_attn_fwd"),
                nbytes=2.0 * (3 * aB * aT * D + aB * aT * D) + (2.0 * aB * nh * aT * Tp if S is not None else 0.0))
            if ws:
                if keep:
                    T[f"l{i}.attn_w"] = attn   # (lp_attn_rowdot pairs it with the windowed d_attn)
                attn = self._win_unpart(attn, D, B, gh, gw, ws)
            proj = self._linear(attn, L["proj"], M)
            x_in = x
            y2, m2, r2, x = self._ln(x, proj, L["ln2"], M, ls=L.get("ls1"))
            h1, a1 = self._linear_gelu(y2, L["fc1"], M)
            delta = self._linear(a1, L["fc2"], M)
            if keep:
                for nm, v in (("x_in", x_in), ("m1", m1), ("r1", r1), ("y1", y1), ("qkv", qkv), ("P", S), ("attn", attn), ("x_mid", x),
                              ("m2", m2), ("r2", r2), ("y2", y2), ("h1", h1), ("a1", a1)):
                    T[f"l{i}.{nm}"] = v
                if "ls1" in L:   # the unscaled branch outputs: the LayerScale gradients are taken against them
                    T[f"l{i}.proj"], T[f"l{i}.fc2"] = proj, delta
        if pl.lnf is None:   # SAM: no final LayerNorm - the last residual add alone, its sum is the features
            feat = torch.empty(M, D, device=dev, dtype=torch.bfloat16)
            x_last = torch.empty_like(x)   # (not in place: x is the last layer's x_mid, which its LayerNorm backward reads from the tape)
            check(self._lib.lp_resid_out_fwd(_p(x), _p(delta), M * D, _p(x_last), _p(feat), ops._stream()), "lp_resid_out_fwd")
        else:
            feat, mf, rf, x = self._ln(x, delta, pl.lnf, M, drop_T=drop_T, ls=pl.layers[-1].get("ls2"), n_prefix=self.n_prefix)
            if keep:
                T["x_last"], T["mf"], T["rf"] = x, mf, rf
        heat = self._head_forward(feat.view(B, gh, gw, D), B, gh, gw, T if keep else {})
        tp.meta.update(B=B, H=H, W=W, gh=gh, gw=gw, training=training, seq=(Bs, Tn, drop_T), rope=draws)
        return heat, tp

    def _check_sam_input(self, H: int, W: int) -> None:
        """SAM's position table was resized once, to the fine-tuning grid, and is trained at that size (reference vit_sam.py): an image of
        another size, or a non-square one, has no table"""
        if self.plan.arch == "sam" and (H != self.sam_grid * self.plan.patch or W != self.sam_grid * self.plan.patch):
            side = self.sam_grid * self.plan.patch
            raise ValueError(f'arch="sam" was built for {side} x {side} images (image_size={side}: its position table holds exactly that '
                             f"grid); got {H} x {W}")

    # ------------------------------------------------------------------------------------------------ backward
    def backward(self, tp: Tape, g_heat: torch.Tensor, trace: dict | None = None) -> None:
        T, pl = tp.t, self.plan
        B, gh, gw = tp.meta["B"], tp.meta["gh"], tp.meta["gw"]
        D, nh = pl.D, pl.heads
        Np = gh * gw
        Bs, Tn, drop_T = tp.meta["seq"]
        M = Bs * Tn
        dev = self.device
        self._wg_shape = (Bs, Tn)
        scale = 1.0 / math.sqrt(D // nh)
        qs = 3 * D

        d_feat = self._head_backward(T, B, g_heat)                      # (B, gh, gw, D) bf16
        progress = self.grad_progress if (self.grad_progress is not None and self.single_backward) else None
        if progress is not None:
            progress(pl.n_backbone)  # the head's gradients (the tail of the flat buffer) are complete
        # gradient of the residual stream (SAM: lp_resid_out_bwd writes all of it)
        dx = (torch.empty if pl.lnf is None else torch.zeros)(M, D, device=dev, dtype=torch.float32)
        # every LayerNorm backward also leaves the updated stream gradient in bf16: it is the operand of the next Linear backward
        # ... and its column sums are the bias gradient of that layer (fc2 of the last block here), so no weight gradient needs a bias pass
        fuse_bias = self.bias_fused
        fuse_gelu = self.gelu_fused != "0"   # (0: A/B runs - lp_gemm_nt, then lp_gelu_bwd_colsum)
        bsum = (lambda lin: self.G[lin.b_off:lin.b_off + lin.N]) if fuse_bias else (lambda lin: None)
        # (DINOv2: each of them also applies the LayerScale of the branch its bf16 output feeds, and leaves that scale's gradient)
        def scaled(j: int, nm: str) -> dict:
            """_ln_bwd's LayerScale arguments for the gradient that feeds branch ``nm`` ("1": attention, "2": MLP) of layer j; {} for the ViT"""
            if "ls1" not in pl.layers[j]:
                return {}
            return dict(ls=pl.layers[j]["ls" + nm], branch=T[f"l{j}." + ("proj" if nm == "1" else "fc2")])

        if pl.lnf is None:
            # SAM: no final LayerNorm.  The head's gradient IS the operand of the last fc2's backward, and its fp32 copy starts the stream
            # gradient; no walk has left that layer's bias sums, so its weight-gradient launch takes them (last_fc2_bias)
            dx16 = d_feat.view(M, D)
            check(self._lib.lp_resid_out_bwd(_p(dx16), M * D, _p(dx), ops._stream()), "lp_resid_out_bwd")
        else:
            dx16 = self._ln_bwd(d_feat, T["x_last"], T["mf"], T["rf"], pl.lnf, M, dx, drop_T=drop_T, want_bf16=True,
                                colsum=bsum(pl.layers[-1]["fc2"]), n_prefix=self.n_prefix, **scaled(pl.depth - 1, "2"))
        rope_tab, rope_seq = T.get("rope_tab"), T.get("rope_seq")

        for i in range(pl.depth - 1, -1, -1):
            L = pl.layers[i]
            t = lambda nm: T[f"l{i}.{nm}"]  # noqa: E731
            if trace is not None:
                trace[f"l{i}.dout"] = dx.clone()
            # ---- MLP branch: x_out = x_mid + fc2(gelu(fc1(LN2(x_mid))))
            dmlp = dx16
            fc2_bias_done = fuse_bias and not (pl.lnf is None and i == pl.depth - 1)
            if fuse_bias and fuse_gelu:   # GELU's backward inside fc2's data gradient (round 6): d_a1 is never written
                d_h1 = self._linear_bwd(L["fc2"], t("a1"), dmlp, M, bias_done=fc2_bias_done, gelu_of=(t("h1"), bsum(L["fc1"])))
                d_a1 = None
            else:
                d_a1 = self._linear_bwd(L["fc2"], t("a1"), dmlp, M, bias_done=fc2_bias_done)
                d_h1 = torch.empty_like(d_a1)
            if d_a1 is None:
                pass
            elif fuse_bias:
                check(self._lib.lp_gelu_bwd_colsum(_p(t("h1")), _p(d_a1), M, pl.mlp, _p(d_h1), _p(bsum(L["fc1"])), ops._stream()), "lp_gelu_bwd_colsum")
            else:
                check(self._lib.lp_gelu_bwd(_p(t("h1")), _p(d_a1), d_a1.numel(), _p(d_h1), ops._stream()), "lp_gelu_bwd")
            d_y2 = self._linear_bwd(L["fc1"], t("y2"), d_h1, M, bias_done=fuse_bias)
            # (proj keeps the bias sums inside its weight-gradient launch: a 384 x 384 layer gains 5 us from the pipelined kernel, the
            #  column sums cost the LayerNorm backward 40 - profiles/archive/r03_final_vit_kernel_stats.txt)
            dx16 = self._ln_bwd(d_y2, t("x_mid"), t("m2"), t("r2"), L["ln2"], M, dx, want_bf16=True, **scaled(i, "1"))
            # ---- attention branch: x_mid = x_in + proj(softmax(Q K^T / 8) V)
            dproj = dx16
            d_attn = self._linear_bwd(L["proj"], t("attn"), dproj, M)
            qkv, Pm = t("qkv"), t("P")
            # SAM's window layers: the same kernels on aB windows of aT tokens - d_attn gathered into windows (pad rows zero: a pad query's
            # output was cropped, so its dS row and dQ are zero), dqkv scattered back behind them
            ws = L.get("window", 0)
            aB, aT = self.window_rows(B, gh, gw, ws) if ws else (Bs, Tn)
            aM, Tp = aB * aT, -(-aT // 64) * 64
            attn_o = t("attn")
            if ws:
                d_attn, attn_o = self._win_part(d_attn, D, D, B, gh, gw, ws, None), t("attn_w")
            dqkv = torch.empty(aM, qs, device=dev, dtype=torch.bfloat16)
            zP = (nh * aT * Tp, aT * Tp)       # batch strides of a [Bs][nh][Tn][Tp] tensor
            zT = (nh * 64 * Tp, 64 * Tp)       # ... of a [B][nh][64][Tp] transposed head slice
            # D = rowsum(dO o O) (== rowsum(dP o P) because O = P V), then ONE pass over the stored probabilities leaves
            # dS = scale * P o (dO V^T - D), dV = P^T dO and dK = dS^T Q (dP never exists; P and dS are touched once each here)
            drow = torch.empty(aM, nh, device=dev, dtype=torch.float32)
            check(self._lib.lp_attn_rowdot(_p(d_attn), _p(attn_o), aM, nh, D, _p(drow), ops._stream()), "lp_attn_rowdot")
            dS = torch.empty(aB * nh * aT, Tp, device=dev, dtype=torch.bfloat16)
            # dP = dO V^T, dV = P^T dO, dK = dS^T Q: 3 products of B * Tn * Tn * D MACs
            self._timed("attn_bwd_kv_kernel", 6.0 * aB * aT * aT * D, lambda: check(self._lib.lp_attn_bwd_kv(
                _p(qkv), qs, 2 * D, _p(d_attn), D, _p(Pm), Tp, _p(drow), aB, nh, aT, scale, _p(dS), _p(dqkv), qs, D, 2 * D, ops._stream()),
                "lp_attn_bwd_kv"), nbytes=2.0 * (2 * aB * nh * aT * Tp + 6 * aB * aT * D))
            # dQ = dS K
            tmpT = torch.empty(aB * nh * 64, Tp, device=dev, dtype=torch.bfloat16)      # a transposed [64][Tp] head slice
            self._transpose(qkv[:, D:].data_ptr(), aT, 64, qs, aT * qs, 64, tmpT, Tp, *zT, aB, nh)
            self._gemm(_p(dS), Tp, _p(tmpT), Tp, aT, 64, Tp, dqkv, qs, batch=(aB, nh, *zP, *zT, aT * qs, 64))
            if ws:   # the pad rows' dK / dV are gradient of the qkv bias (their k and v ARE the bias): summed into it by the same launch
                dqkv = self._win_unpart(dqkv, qs, B, gh, gw, ws, pad_colsum=self.G[L["qkv"].b_off:L["qkv"].b_off + qs])
            if trace is not None:
                trace[f"l{i}.dqkv"] = dqkv
            if rope_tab is not None:   # dqkv is complete: the transposed rotation of dQ / dK, before the qkv weight gradient reads it
                self._rope(1, dqkv, qs, rope_tab, rope_seq, rope_tab.shape[0], Bs, Tn)
            d_y1 = self._linear_bwd(L["qkv"], t("y1"), dqkv, M)
            if pl.arch == "dinov3":
                self._clear_key_bias(L["qkv"])
            dx16 = self._ln_bwd(d_y1, t("x_in"), t("m1"), t("r1"), L["ln1"], M, dx, want_bf16=i > 0,
                                colsum=bsum(pl.layers[i - 1]["fc2"]) if i > 0 else None, **(scaled(i - 1, "2") if i > 0 else {}))
            if progress is not None:
                progress(L["ln1"].g_off)  # everything from this layer's first parameter to the end of G is final
        if trace is not None:
            trace["tokens.dx"] = dx
        # ---- embeddings
        dpatch = self._tokens_bwd(dx, B, Np, gh, gw)
        self._wg_shape = (B, Np)
        self._linear_bwd(pl.patch_lin, T["patches"], dpatch, B * Np, need_dx=False)
        self._join_side_stream()
