"""fp32 VALIDATION executor of the ViT-S/16 heatmap tracker (config C4) - the ViT counterpart of engine_fp32.Fp32Engine.

The reference trains in fp32 only (lightning_pose/train.py:411-428); its ViT backbone is ``VisionEncoder`` over HuggingFace ``ViTModel``
(lightning_pose/models/backbones/vit.py:16-49).  ``ViTEngine`` (bf16-mixed) is the product and the measured path; this subclass runs the same
plan with every tensor and every contraction in fp32 so that a whole training step can be held to BASELINE.json's 1e-4.
"""

from __future__ import annotations

import ctypes as C
import math

import torch

from . import _lib, ops
from ._lib import check
from .engine import Tape, image_parts
from .engine_fp32 import Fp32Head
from .ops import _p
from .vit_engine import Lin, LNP, ViTEngine


class Fp32ViTEngine(Fp32Head, ViTEngine):
    """config C4 (ViT-S/16, reference models/backbones/vit.py:16-49 over HuggingFace ``ViTModel``) in the reference's own precision:
    the plan, flat buffers, state_dict names and optimiser of :class:`ViTEngine`, every tensor and contraction fp32
    (csrc/vit_f32.hip for LayerNorm / GELU / tokens / attention, lp_f32_conv_* with a 1x1 geometry for the Linear layers, the head of
    :class:`Fp32Engine`: ``Fp32Head``).  VALIDATION path: untuned, selected with ``precision="fp32"`` / ``LP_PRECISION=fp32``."""

    _patch_dtype = torch.float32
    _token_kernels = ("lp_f32_vit_tokens_fwd", "lp_f32_vit_tokens_bwd", "lp_f32_vit_mv_tokens_fwd", "lp_f32_vit_mv_tokens_bwd")
    _reg_token_kernels = ("lp_f32_vit_reg_tokens_fwd", "lp_f32_vit_reg_tokens_bwd")
    _rope_kernels = ("lp_f32_rope_fwd", "lp_f32_rope_bwd")
    _ln_px_kernels = ("lp_f32_layernorm_ls_fwd_px", "lp_f32_layernorm_ls_bwd_px")
    _window_kernels = ("lp_f32_window_partition", "lp_f32_window_unpartition")
    _pos_token_kernels = ("lp_f32_vit_pos_tokens_fwd", "lp_f32_vit_pos_tokens_bwd")
    _act_dtype = torch.float32
    _elem_bytes = 4.0

    def _qkv_pad_fill(self, l: Lin) -> torch.Tensor:
        """an all-zero input row leaves the fp32 Linear layer as the bias itself"""
        return self.P[l.b_off:l.b_off + l.N]

    @staticmethod
    def _lin_geom(l: Lin, M: int):
        return _lib.ConvGeom(1, 1, M, l.K, 1, M, l.N, 1, 1, 1, 0)

    def _linear(self, x: torch.Tensor, l: Lin, M: int) -> torch.Tensor:
        out = self._f32(M, l.N)
        check(self._lib.lp_f32_conv_fwd(_p(x), _p(self.P[l.w_off:]), C.byref(self._lin_geom(l, M)), 1, 1, l.K, _p(self.P[l.b_off:]), None,
                                        _p(out), ops._stream()), "lp_f32_conv_fwd(linear)")
        return out

    def _linear_bwd(self, l: Lin, x: torch.Tensor, dy: torch.Tensor, M: int, need_dx: bool = True):
        g = self._lin_geom(l, M)
        bsum = torch.zeros(2 * l.N, device=self.device, dtype=torch.float32)
        check(self._lib.lp_f32_bn_stats(_p(dy), M, l.N, _p(bsum), ops._stream()), "lp_f32_bn_stats(bias)")
        self.G[l.b_off:l.b_off + l.N] += bsum[:l.N]
        check(self._lib.lp_f32_conv_wgrad(_p(x), _p(dy), C.byref(g), 1, 1, l.K, _p(self.G[l.w_off:]), ops._stream()), "lp_f32_conv_wgrad(linear)")
        if not need_dx:
            return None
        dx = self._f32(M, l.K)
        check(self._lib.lp_f32_conv_dgrad(_p(dy), _p(self.P[l.w_off:]), C.byref(g), 1, 1, l.K, None, None, _p(dx), ops._stream()),
              "lp_f32_conv_dgrad(linear)")
        return dx

    def _ln(self, x, delta, l: LNP, M: int, drop_T: int = 0, ls: int | None = None, n_prefix: int = 1):
        D = self.plan.D
        xo = torch.empty_like(x) if delta is not None else None
        rows = M - (M // drop_T) * n_prefix if drop_T else M
        y = self._f32(rows, D)
        mean, rstd = self._f32(M), self._f32(M)
        if drop_T and n_prefix != 1:   # DINOv3: [CLS] and the registers dropped (the LayerScale walk's prefix-taking form)
            assert ls is not None and delta is not None
            check(self._lib.lp_f32_layernorm_ls_fwd_px(_p(x), _p(delta), _p(self.P[ls:]), _p(xo), _p(self.P[l.g_off:]), _p(self.P[l.b_off:]),
                                                       self.ln_eps, M, D, drop_T, n_prefix, _p(y), _p(mean), _p(rstd), ops._stream()),
                  "lp_f32_layernorm_ls_fwd_px")
            return y, mean, rstd, xo
        if ls is not None and delta is not None:   # DINOv2: x_out = x + (delta * LayerScale)
            check(self._lib.lp_f32_layernorm_ls_fwd(_p(x), _p(delta), _p(self.P[ls:]), _p(xo), _p(self.P[l.g_off:]), _p(self.P[l.b_off:]),
                                                    self.ln_eps, M, D, drop_T, _p(y), _p(mean), _p(rstd), ops._stream()), "lp_f32_layernorm_ls_fwd")
            return y, mean, rstd, xo
        check(self._lib.lp_f32_layernorm_fwd(_p(x), _p(delta), _p(xo), _p(self.P[l.g_off:]), _p(self.P[l.b_off:]), self.ln_eps, M, D, drop_T, _p(y),
                                             _p(mean), _p(rstd), ops._stream()), "lp_f32_layernorm_fwd")
        return y, mean, rstd, (xo if xo is not None else x)

    def _ln_bwd(self, dy, x, mean, rstd, l: LNP, M: int, dx, drop_T: int = 0, want_bf16: bool = False, ls: int | None = None, branch=None,
                n_prefix: int = 1):
        if drop_T and n_prefix != 1:
            assert want_bf16 and ls is not None
            out = self._f32(M, self.plan.D)
            check(self._lib.lp_f32_layernorm_ls_bwd_px(_p(dy), _p(x), _p(mean), _p(rstd), _p(self.P[l.g_off:]), _p(self.P[ls:]), _p(branch), M,
                                                       self.plan.D, drop_T, n_prefix, _p(dx), _p(out), _p(self.G[l.g_off:]), _p(self.G[l.b_off:]),
                                                       None, _p(self.G[ls:]), ops._stream()), "lp_f32_layernorm_ls_bwd_px")
            return out
        if want_bf16 and ls is not None:   # DINOv2: the operand of the next Linear backward leaves through the LayerScale at offset ``ls``
            out = self._f32(M, self.plan.D)
            check(self._lib.lp_f32_layernorm_ls_bwd(_p(dy), _p(x), _p(mean), _p(rstd), _p(self.P[l.g_off:]), _p(self.P[ls:]), _p(branch), M,
                                                    self.plan.D, drop_T, _p(dx), _p(out), _p(self.G[l.g_off:]), _p(self.G[l.b_off:]), None,
                                                    _p(self.G[ls:]), ops._stream()), "lp_f32_layernorm_ls_bwd")
            return out
        check(self._lib.lp_f32_layernorm_bwd(_p(dy), _p(x), _p(mean), _p(rstd), _p(self.P[l.g_off:]), M, self.plan.D, drop_T, _p(dx),
                                             _p(self.G[l.g_off:]), _p(self.G[l.b_off:]), ops._stream()), "lp_f32_layernorm_bwd")
        return dx.clone() if want_bf16 else None   # (the operand of the next Linear backward: dx itself moves on in place)

    def _forward(self, images, training: bool, keep: bool, rope=None):
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
        patches = self._f32(B * Np, 3 * pt * pt)
        i0 = 0
        for p_ in parts:
            check(self._lib.lp_f32_vit_patchify(_p(p_), p_.shape[0], H, W, pt, _p(patches[i0 * Np:]), ops._stream()), "lp_f32_vit_patchify")
            i0 += p_.shape[0]
        pe = self._linear(patches, pl.patch_lin, B * Np)
        x = self._f32(M, D)
        pos = self._pos(gh, gw) if pl.n_pos else None
        self._tokens_fwd(pe, pos, B, Np, x)
        T["patches"] = patches
        rope_tab, rope_seq, n_tab, draws = self._rope_tables(gh, gw, [p_.shape[0] for p_ in parts], training, rope)
        if rope_tab is not None:
            T["rope_tab"], T["rope_seq"] = rope_tab, rope_seq
        delta = None
        scale = 1.0 / math.sqrt(D // nh)
        qs = 3 * D
        for i, L in enumerate(pl.layers):
            y1, m1, r1, x = self._ln(x, delta, L["ln1"], M, ls=pl.layers[i - 1].get("ls2") if i else None)
            qkv = self._linear(y1, L["qkv"], M)
            if rope_tab is not None:   # DINOv3: the patch tokens' q and k rotated in place (the tape keeps them rotated)
                self._rope(0, qkv, qs, rope_tab, rope_seq, n_tab, Bs, Tn)
            ws = L.get("window", 0)   # SAM's window layers: aB windows of aT tokens, pad rows = the qkv bias (vit_engine.py)
            aB, aT = self.window_rows(B, gh, gw, ws) if ws else (Bs, Tn)
            if ws:
                qkv = self._win_part(qkv, qs, qs, B, gh, gw, ws, self._qkv_pad_fill(L["qkv"]))
            Pm = self._f32(aB * nh * aT, aT)
            attn = self._f32(aB * aT, D)
            check(self._lib.lp_f32_attn_fwd(_p(qkv), qs, D, 2 * D, aB, nh, aT, scale, _p(Pm), _p(attn), D, ops._stream()), "lp_f32_attn_fwd")
            if ws:
                attn = self._win_unpart(attn, D, B, gh, gw, ws)
            proj = self._linear(attn, L["proj"], M)
            x_in = x
            y2, m2, r2, x = self._ln(x, proj, L["ln2"], M, ls=L.get("ls1"))
            h1 = self._linear(y2, L["fc1"], M)
            a1 = torch.empty_like(h1)
            check(self._lib.lp_f32_gelu_fwd(_p(h1), h1.numel(), _p(a1), ops._stream()), "lp_f32_gelu_fwd")
            delta = self._linear(a1, L["fc2"], M)
            if keep:
                for nm, v in (("x_in", x_in), ("m1", m1), ("r1", r1), ("y1", y1), ("qkv", qkv), ("P", Pm), ("attn", attn), ("x_mid", x),
                              ("m2", m2), ("r2", r2), ("y2", y2), ("h1", h1), ("a1", a1)):
                    T[f"l{i}.{nm}"] = v
                if "ls1" in L:   # the unscaled branch outputs: the LayerScale gradients are taken against them
                    T[f"l{i}.proj"], T[f"l{i}.fc2"] = proj, delta
        if pl.lnf is None:   # SAM: no final LayerNorm - the features are the last residual add's sum
            feat = self._f32(M, D)
            check(self._lib.lp_f32_resid_out_fwd(_p(x), _p(delta), M * D, _p(feat), ops._stream()), "lp_f32_resid_out_fwd")
        else:
            feat, mf, rf, x = self._ln(x, delta, pl.lnf, M, drop_T=drop_T, ls=pl.layers[-1].get("ls2"), n_prefix=self.n_prefix)
            T["x_last"], T["mf"], T["rf"] = x, mf, rf
        heat = self._head_forward(feat.view(B, gh, gw, D), B, gh, gw, T)
        tp.meta.update(B=B, H=H, W=W, gh=gh, gw=gw, training=training, seq=(Bs, Tn, drop_T), rope=draws)
        return heat, tp

    def backward(self, tp: Tape, g_heat: torch.Tensor, trace: dict | None = None) -> None:
        T, pl = tp.t, self.plan
        B, gh, gw = tp.meta["B"], tp.meta["gh"], tp.meta["gw"]
        D, nh = pl.D, pl.heads
        Np = gh * gw
        Bs, Tn, drop_T = tp.meta["seq"]
        M = Bs * Tn
        scale = 1.0 / math.sqrt(D // nh)
        qs = 3 * D
        d_feat = self._head_backward(T, B, g_heat).contiguous()            # (B, gh, gw, D) fp32
        # gradient of the residual stream (SAM: lp_f32_resid_out_bwd writes all of it)
        dx = (torch.empty if pl.lnf is None else torch.zeros)(M, D, device=self.device, dtype=torch.float32)
        def scaled(j: int, nm: str) -> dict:
            """_ln_bwd's LayerScale arguments for the gradient that feeds branch ``nm`` ("1": attention, "2": MLP) of layer j; {} for the ViT"""
            if "ls1" not in pl.layers[j]:
                return {}
            return dict(ls=pl.layers[j]["ls" + nm], branch=T[f"l{j}." + ("proj" if nm == "1" else "fc2")])

        if pl.lnf is None:   # SAM: the head's gradient starts the stream gradient and is the operand of the last fc2's backward
            dcur = d_feat.view(M, D)
            check(self._lib.lp_f32_resid_out_bwd(_p(dcur), M * D, _p(dx), ops._stream()), "lp_f32_resid_out_bwd")
        else:
            dcur = self._ln_bwd(d_feat, T["x_last"], T["mf"], T["rf"], pl.lnf, M, dx, drop_T=drop_T, want_bf16=True, n_prefix=self.n_prefix,
                                **scaled(pl.depth - 1, "2"))
        rope_tab, rope_seq = T.get("rope_tab"), T.get("rope_seq")
        for i in range(pl.depth - 1, -1, -1):
            L = pl.layers[i]
            t = lambda nm: T[f"l{i}.{nm}"]  # noqa: E731
            if trace is not None:
                trace[f"l{i}.dout"] = dx.clone()
            d_a1 = self._linear_bwd(L["fc2"], t("a1"), dcur, M)
            d_h1 = torch.empty_like(d_a1)
            check(self._lib.lp_f32_gelu_bwd(_p(t("h1")), _p(d_a1), d_a1.numel(), _p(d_h1), ops._stream()), "lp_f32_gelu_bwd")
            d_y2 = self._linear_bwd(L["fc1"], t("y2"), d_h1, M)
            dcur = self._ln_bwd(d_y2, t("x_mid"), t("m2"), t("r2"), L["ln2"], M, dx, want_bf16=True, **scaled(i, "1"))
            d_attn = self._linear_bwd(L["proj"], t("attn"), dcur, M)
            ws = L.get("window", 0)
            aB, aT = self.window_rows(B, gh, gw, ws) if ws else (Bs, Tn)
            if ws:   # d_attn gathered into windows, pad rows zero
                d_attn = self._win_part(d_attn, D, D, B, gh, gw, ws, None)
            dqkv = self._f32(aB * aT, qs)
            dS = self._f32(aB * nh * aT, aT)
            check(self._lib.lp_f32_attn_bwd(_p(t("qkv")), qs, D, 2 * D, _p(d_attn), D, _p(t("P")), aB, nh, aT, scale, _p(dS), _p(dqkv), qs,
                                            ops._stream()), "lp_f32_attn_bwd")
            if ws:   # scattered back; the pad rows' dK / dV summed into the qkv bias gradient
                dqkv = self._win_unpart(dqkv, qs, B, gh, gw, ws, pad_colsum=self.G[L["qkv"].b_off:L["qkv"].b_off + qs])
            if trace is not None:
                trace[f"l{i}.dqkv"] = dqkv
            if rope_tab is not None:   # the transposed rotation of dQ / dK, before the qkv weight gradient reads them
                self._rope(1, dqkv, qs, rope_tab, rope_seq, rope_tab.shape[0], Bs, Tn)
            d_y1 = self._linear_bwd(L["qkv"], t("y1"), dqkv, M)
            if pl.arch == "dinov3":
                self._clear_key_bias(L["qkv"])
            dcur = self._ln_bwd(d_y1, t("x_in"), t("m1"), t("r1"), L["ln1"], M, dx, want_bf16=i > 0, **(scaled(i - 1, "2") if i > 0 else {}))
        if trace is not None:
            trace["tokens.dx"] = dx
        dpatch = self._tokens_bwd(dx, B, Np, gh, gw)
        self._linear_bwd(pl.patch_lin, T["patches"], dpatch, B * Np, need_dx=False)
