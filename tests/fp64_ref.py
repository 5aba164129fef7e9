"""float64 references of the step's contractions (convolutions, GEMMs, attention), computed from the same bf16 (or, for the fp32 validation
kernels, fp32) operands the kernels read.

Everything here runs in torch float64 on the operands' device: im2col (F.unfold) and torch.matmul, never an fp32 library convolution or GEMM
(those may take reduced-precision paths).  Beside every result r the helpers return S = sum |a b| over the products behind it (the same
matmul on |A| and |B|): the scale of the rounding error an fp32-accumulating kernel may make, whatever the signs.

Used by tests/test_step_contractions_fp64.py, from "fp32 validation kernels" down by tests/test_fp32_validation_kernels.py, and from
"bf16 ViT glue kernels" down by tests/test_vit_bf16_kernels.py.
"""

from __future__ import annotations

import math

import torch
import torch.nn.functional as F

F64 = torch.float64
CHUNK_BYTES = 1 << 30   # largest fp64 im2col block built at once


def fx_value(t: torch.Tensor) -> torch.Tensor:
    """lp_fxsum (int64 hi, lo) pairs -> float64 values: hi 2^-12 + lo 2^-60 (include/lp_hip.h)"""
    t = t.reshape(-1, 2)
    return t[:, 0].to(F64) * 2.0 ** -12 + t[:, 1].to(F64) * 2.0 ** -60


def bf16_bar(r: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """per element bar of a bf16 result: half an ulp of the stored value (2^-8 |r| covers the final rounding with room for the ulp of a
    neighbour) plus 2^-16 S for the fp32 accumulation"""
    return 2.0 ** -8 * r.abs() + 2.0 ** -16 * s


def f32_bar(s: torch.Tensor) -> torch.Tensor:
    """per element bar of an fp32 result (weight / bias gradients): 2^-18 S"""
    return 2.0 ** -18 * s


def worst(y: torch.Tensor, r: torch.Tensor, bar: torch.Tensor) -> float:
    """max |y - r| / bar (0 for an empty selection); a result that is not finite counts as infinitely far off"""
    if y.numel() == 0:
        return 0.0
    d = (y.to(F64) - r).abs() / bar.clamp_min(1e-300)
    d = torch.where(torch.isfinite(d), d, torch.full_like(d, math.inf))
    return float(d.max())


# ---------------------------------------------------------------------------------------------------------------- convolutions
class ConvOperand:
    """An NHWC bf16 activation seen through a convolution's taps as the rows of an im2col matrix A[m][k], k = (c, r, s) as F.unfold
    orders it, m = (b, y, x) over the output grid.

    ``dilate`` > 1 inserts dilate - 1 zero rows / columns between the pixels (the data gradient of a strided convolution runs as a
    stride-1 correlation over the dilated gradient); ``pads`` = (top, bottom, left, right), negative = crop."""

    def __init__(self, x: torch.Tensor, C: int, R: int, S: int, stride: int, pads: tuple[int, int, int, int], dilate: int = 1):
        self.x, self.C, self.R, self.S, self.stride, self.pads, self.dilate = x, C, R, S, stride, pads, dilate
        B, H, W = x.shape[0], x.shape[1], x.shape[2]
        self.B = B
        self.Hd, self.Wd = (H - 1) * dilate + 1, (W - 1) * dilate + 1   # the grid the taps walk (before padding)
        t, b, l, r = pads
        self.Ho = (self.Hd + t + b - R) // stride + 1
        self.Wo = (self.Wd + l + r - S) // stride + 1
        self.rows_per_image = self.Ho * self.Wo
        self.K = C * R * S
        self.plain = R == S == 1 and stride == 1 and dilate == 1 and pads == (0, 0, 0, 0)

    def grid(self, b0: int, b1: int) -> torch.Tensor:
        """images [b0, b1) as float64 NCHW on the tap grid (dilated, unpadded)"""
        x = self.x[b0:b1, ..., :self.C].to(F64).permute(0, 3, 1, 2)
        if self.dilate == 1:
            return x
        out = x.new_zeros(x.shape[0], self.C, self.Hd, self.Wd)
        out[:, :, ::self.dilate, ::self.dilate] = x
        return out

    def rows(self, b0: int, b1: int) -> torch.Tensor:
        """A for images [b0, b1): (b1 - b0) * Ho * Wo rows of K"""
        if self.plain:
            return self.x[b0:b1, ..., :self.C].reshape(-1, self.C).to(F64)
        t, b, l, r = self.pads
        g = F.pad(self.grid(b0, b1), (l, r, t, b))
        a = F.unfold(g, (self.R, self.S), stride=self.stride)      # (n, K, L)
        return a.transpose(1, 2).reshape(-1, self.K)

    def image_chunks(self):
        per = max(1, CHUNK_BYTES // max(1, 8 * self.rows_per_image * self.K * (1 if self.plain else 2)))
        for b0 in range(0, self.B, per):
            yield b0, min(self.B, b0 + per)

    def row_chunks(self, max_rows: int | None = None):
        """(m0, m1, A[m0:m1]) over all rows, whole images per chunk (1x1 layers: any row range)"""
        if self.plain:
            M = self.B * self.rows_per_image
            per = max(1, CHUNK_BYTES // (8 * self.K))
            for m0 in range(0, M, per):
                m1 = min(M, m0 + per)
                yield m0, m1, self.x.reshape(-1, self.x.shape[-1])[m0:m1, :self.C].to(F64)
            return
        for b0, b1 in self.image_chunks():
            yield b0 * self.rows_per_image, b1 * self.rows_per_image, self.rows(b0, b1)

    def row_block(self, m0: int, m1: int) -> torch.Tensor:
        """A[m0:m1] (any range)"""
        rpi = self.rows_per_image
        b0, b1 = m0 // rpi, (m1 - 1) // rpi + 1
        return self.rows(b0, b1)[m0 - b0 * rpi:m1 - b0 * rpi]

    def kstep(self, tap: int, c0: int, width: int = 64) -> torch.Tensor:
        """column indices of one K step of the kernels: channels [c0, c0 + width) of filter tap `tap` (= r S + s)"""
        c = torch.arange(c0, min(self.C, c0 + width), device=self.x.device)
        return c * (self.R * self.S) + tap

    def tap_shift_rows(self, tap_r: int, tap_s: int):
        """The rows of the last image's last output column and, per row, the A column block of tap (tap_r, tap_s) as a kernel would read it
        if that tap's pixel index ran one pixel past its position in the flattened (y, x) order - across the end of the image row.
        Returns (row indices m, original block (n, C), shifted block (n, C)); rows whose tap sits in a padding ROW are left out."""
        t, _, l, _ = self.pads
        b = self.B - 1
        g = self.grid(b, b + 1)[0]                                   # (C, Hd, Wd)
        flat = g.reshape(self.C, -1)
        ms, orig, shifted = [], [], []
        xo = self.Wo - 1
        xi = xo * self.stride - l + tap_s
        for yo in range(self.Ho):
            yi = yo * self.stride - t + tap_r
            if not 0 <= yi < self.Hd:
                continue
            f = yi * self.Wd + xi + 1
            if not (xi + 1 >= self.Wd and 0 <= f < flat.shape[1]):    # (the shifted read must cross the row end)
                continue
            o = g[:, yi, xi] if 0 <= xi < self.Wd else torch.zeros(self.C, dtype=F64, device=g.device)
            ms.append(b * self.rows_per_image + yo * self.Wo + xo)
            orig.append(o)
            shifted.append(flat[:, f])
        if not ms:
            return None
        return torch.tensor(ms, device=g.device), torch.stack(orig), torch.stack(shifted)


def conv_fwd_operand(x: torch.Tensor, C: int, R: int, S: int, stride: int, pad: int) -> ConvOperand:
    return ConvOperand(x, C, R, S, stride, (pad, pad, pad, pad))


def conv_dgrad_operand(dy: torch.Tensor, Co: int, R: int, S: int, stride: int, pad: int, Hi: int, Wi: int) -> ConvOperand:
    """dx[hi] = sum_r dy[ho] w[r] over ho * stride - pad + r == hi: a stride-1 correlation of the zero-dilated dy with the flipped
    filter, padded R - 1 - pad on the leading side and to an Hi x Wi result on the trailing side"""
    Ho, Wo = dy.shape[1], dy.shape[2]
    Hd, Wd = (Ho - 1) * stride + 1, (Wo - 1) * stride + 1
    pt, pl = R - 1 - pad, S - 1 - pad
    return ConvOperand(dy, Co, R, S, 1, (pt, Hi + R - 1 - pt - Hd, pl, Wi + S - 1 - pl - Wd), dilate=stride)


def weight_matrix_fwd(w: torch.Tensor, R: int, S: int, C: int) -> torch.Tensor:
    """[N][R][S][Cpitch] bf16 filter -> (N, C R S) float64 in unfold order"""
    return w[..., :R, :S, :C].to(F64).permute(0, 3, 1, 2).reshape(w.shape[0], -1)


def weight_matrix_dgrad(wd: torch.Tensor, R: int, S: int) -> torch.Tensor:
    """[Ci][R][S][Co] bf16 transposed filter -> (Ci, Co R S) float64 for conv_dgrad_operand (taps flipped)"""
    return wd.to(F64).flip(1, 2).permute(0, 3, 1, 2).reshape(wd.shape[0], -1)


# ---------------------------------------------------------------------------------------------------------------- GELU
def gelu(x: torch.Tensor) -> torch.Tensor:
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_grad(x: torch.Tensor) -> torch.Tensor:
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


# ---------------------------------------------------------------------------------------------------------------- fp32 validation kernels
# Written-out float64 forms of what csrc/fp32.hip / csrc/vit_f32.hip compute, on the same fp32 operands.  Where a result is a sum of
# products the helper also returns S = the same expression on absolute values (the scale of f32_bar).
def conv_weight_dgrad_from_storage(w: torch.Tensor, R: int, S: int, Ci: int) -> torch.Tensor:
    """[Co][KH][KW][CiS] storage -> the (Ci, Co R S) matrix of weight_matrix_dgrad (no transposed copy exists on the fp32 path)"""
    return weight_matrix_dgrad(w[:, :R, :S, :Ci].permute(3, 1, 2, 0), R, S)


def conv_wgrad(A: torch.Tensor, dy: torch.Tensor, Co: int, Ci: int, R: int, S: int):
    """dW[n][r][s][c] = sum_m A[m][(c, r, s)] dy[m][n] from im2col rows A (M, Ci R S): -> (dW, S) as (Co, R, S, Ci)"""
    d = dy.reshape(-1, Co).to(F64)
    shape = lambda t: t.reshape(Co, Ci, R, S).permute(0, 2, 3, 1)  # noqa: E731
    return shape(d.T @ A), shape(d.abs().T @ A.abs())


def attn_split(qkv: torch.Tensor, B: int, nh: int, T: int, k_off: int, v_off: int):
    """fused (B T, ld) tensor -> q, k, v (B, nh, T, 64) float64"""
    t = qkv.reshape(B, T, -1).to(F64)
    cut = lambda o: t[:, :, o:o + nh * 64].reshape(B, T, nh, 64).permute(0, 2, 1, 3)  # noqa: E731
    return cut(0), cut(k_off), cut(v_off)


def attn_fwd(q, k, v, scale: float):
    """-> (P, O, S_O): soft-max(scale q k^T), P v, |P| |v|"""
    p = torch.softmax(scale * torch.einsum("bhid,bhjd->bhij", q, k), dim=-1)
    return p, torch.einsum("bhij,bhjd->bhid", p, v), torch.einsum("bhij,bhjd->bhid", p, v.abs())


def attn_bwd(q, k, v, p, do, scale: float):
    """dQ, dK, dV from the STORED probabilities p (an operand of the backward kernels) and their scales: every product behind an
    element in absolute value, through the chain dP = dO V^T, dS = P o (dP - rowsum(P o dP))"""
    dp = torch.einsum("bhid,bhjd->bhij", do, v)
    dp_s = torch.einsum("bhid,bhjd->bhij", do.abs(), v.abs())
    ds = p * (dp - (p * dp).sum(-1, keepdim=True))
    ds_s = p * (dp_s + (p * dp_s).sum(-1, keepdim=True))
    dq, dq_s = scale * torch.einsum("bhij,bhjd->bhid", ds, k), scale * torch.einsum("bhij,bhjd->bhid", ds_s, k.abs())
    dk, dk_s = scale * torch.einsum("bhij,bhid->bhjd", ds, q), scale * torch.einsum("bhij,bhid->bhjd", ds_s, q.abs())
    dv, dv_s = torch.einsum("bhij,bhid->bhjd", p, do), torch.einsum("bhij,bhid->bhjd", p, do.abs())
    return (dq, dq_s), (dk, dk_s), (dv, dv_s)


def heads_to_rows(t: torch.Tensor) -> torch.Tensor:
    """(B, nh, T, 64) -> (B T, nh 64), the column block of a fused tensor"""
    B, nh, T, _ = t.shape
    return t.permute(0, 2, 1, 3).reshape(B * T, nh * 64)


def kept_rows(M: int, drop_T: int, device, shift: int = 0) -> torch.Tensor:
    """the rows a LayerNorm with drop_T writes, in output order: row % drop_T != 0 (shift = 1: the off-by-one mutant)"""
    r = torch.arange(M, device=device)
    return r if drop_T == 0 else r[(r % drop_T) != shift]


def maxpool_windows(x: torch.Tensor) -> torch.Tensor:
    """NHWC -> (B, C, 9, Ho Wo) float64 windows of the 3x3 / stride 2 / pad 1 pool, taps row-major, padding = -inf"""
    B, H, W, C_ = x.shape
    g = F.pad(x.to(F64).permute(0, 3, 1, 2), (1, 1, 1, 1), value=-math.inf)
    return F.unfold(g, 3, stride=2).reshape(B, C_, 9, -1)


def maxpool_fwd(x: torch.Tensor, last: bool = False):
    """-> (max (B, Ho, Wo, C), tap of the FIRST maximum in row-major order as uint8; last=True: of the last one - the tie mutant)"""
    B, H, W, C_ = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    win = maxpool_windows(x)
    m = win.amax(2, keepdim=True)
    taps = torch.arange(9, device=x.device).reshape(1, 1, 9, 1)
    hit = win == m
    arg = torch.where(hit, taps, torch.full_like(taps, -1 if last else 9))
    arg = arg.amax(2) if last else arg.amin(2)
    nhwc = lambda t: t.reshape(B, C_, Ho, Wo).permute(0, 2, 3, 1).contiguous()  # noqa: E731
    return nhwc(m.squeeze(2)), nhwc(arg).to(torch.uint8)


def maxpool_bwd(arg: torch.Tensor, dy: torch.Tensor, H: int, W: int):
    """dx[pixel] = sum of the dy of the windows whose arg-max tap is that pixel: -> (dx, sum |dy| likewise), NHWC"""
    B, Ho, Wo, C_ = dy.shape
    onehot = (arg.permute(0, 3, 1, 2).reshape(B, C_, 1, -1).long() == torch.arange(9, device=dy.device).reshape(1, 1, 9, 1)).to(F64)
    out = []
    for d in (dy.to(F64), dy.to(F64).abs()):
        cols = onehot * d.permute(0, 3, 1, 2).reshape(B, C_, 1, -1)
        out.append(F.fold(cols.reshape(B, C_ * 9, -1), (H, W), 3, stride=2, padding=1).permute(0, 2, 3, 1).contiguous())
    return out[0], out[1]


def pixel_shuffle(x: torch.Tensor, c_out: int) -> torch.Tensor:
    """(B, h, w, 4 c_out) -> (B, 2h, 2w, c_out): out[b][2y+i][2x+j][c] = in[b][y][x][4c + 2i + j]"""
    B, h, w, _ = x.shape
    return x.reshape(B, h, w, c_out, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(B, 2 * h, 2 * w, c_out)


def pixel_unshuffle(x: torch.Tensor) -> torch.Tensor:
    """the inverse: (B, 2h, 2w, c) -> (B, h, w, 4c)"""
    B, H, W, c = x.shape
    return x.reshape(B, H // 2, 2, W // 2, 2, c).permute(0, 1, 3, 5, 2, 4).reshape(B, H // 2, W // 2, 4 * c)


def patchify(img: torch.Tensor, P: int) -> torch.Tensor:
    """(B, 3, H, W) -> (B gh gw, 3 P P), k = (c, ky, kx)"""
    B, _, H, W = img.shape
    return img.reshape(B, 3, H // P, P, W // P, P).permute(0, 2, 4, 1, 3, 5).reshape(B * (H // P) * (W // P), 3 * P * P)


# ---------------------------------------------------------------------------------------------------------------- bf16 ViT glue kernels
# bf16 operands and results travel as int16 tensors of bits (tests/test_vit_bf16_kernels.py); integer arithmetic, no torch.bfloat16 cast.
def bf16_bits(x: torch.Tensor) -> torch.Tensor:
    """float32 -> bf16 bit patterns (int16), round to nearest even; +-inf stay, a NaN becomes a quiet NaN, an fp32 denormal rounds like any
    other value (to a bf16 denormal or to the smallest normal)"""
    u = x.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    r = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    r = torch.where((u & 0x7FFFFFFF) > 0x7F800000, (u >> 16) | 0x40, r)
    return (((r & 0xFFFF) ^ 0x8000) - 0x8000).to(torch.int16)


def bf16_f32(bits: torch.Tensor) -> torch.Tensor:
    """int16 bf16 bit patterns -> the float32 values they stand for (exact)"""
    return (bits.to(torch.int32) * 65536).view(torch.float32)


def bf16_value(bits: torch.Tensor) -> torch.Tensor:
    return bf16_f32(bits).to(F64)


def bf16_trunc(r: torch.Tensor) -> torch.Tensor:
    """the truncation mutant: the low 16 bits of r's fp32 image cleared (a bf16 store that chops instead of rounding), as float64"""
    return (r.to(torch.float32).contiguous().view(torch.int32) & -65536).view(torch.float32).to(F64)


def bf16_half_ulp(v: torch.Tensor) -> torch.Tensor:
    """half an ulp of bf16 at the magnitude v >= 0: 8 significant bits, so an ulp is 2^-7 of the binade's power of two and half of one is
    2^(floor(log2 v) - 8) - between 2^-9 v (top of a binade) and 2^-8 v (bottom); 2^-134 in the denormal range; 0 at 0"""
    ex = torch.frexp(v)[1].clamp_min(-125)                     # v = m 2^ex, m in [0.5, 1)
    return torch.where(v > 0, torch.ldexp(torch.ones_like(v), ex - 9), torch.zeros_like(v))


def bf16_store_bar(r: torch.Tensor, e: torch.Tensor) -> torch.Tensor:
    """bar of a bf16 result whose fp32 value before the store is within e of r: ONE round-to-nearest of a value of magnitude at most
    |r| + e moves it by at most half an ulp there - bf16_half_ulp(|r| + e) + e.  (2^-9 (|r| + e) + e is that only at the top of a binade: a
    correctly rounded 1 + 0.9 x 2^-8 -> 1 is off by 1.8 x 2^-9.)  A store that truncates errs by up to a whole ulp and fails this."""
    return bf16_half_ulp(r.abs() + e) + e


# The product GELU (csrc/lp_common.h gelu_f2 / gelu_df2) is not erff + expf: the forward is Numerical Recipes' erfcc (a Chebyshev fit of
# erfc, fractional error < 1.2e-7), the backward Abramowitz & Stegun 7.1.26 (absolute error < 1.5e-7) with one exponential for both terms.
# The two functions below evaluate THE SAME FORMULAS in torch float32 on the CPU, one operation per rounding (no fused multiply-add, no
# hardware reciprocal or exponential): an evaluation independent of the kernels, measured against float64 for the bars of the kernel test.
def gelu_erfcc_f32(x: torch.Tensor) -> torch.Tensor:
    x = x.to(torch.float32)
    z = x.abs() * 0.70710678118654752
    t = 1.0 / (z * 0.5 + 1.0)
    p = t * 0.17087277 - 0.82215223
    for c in (1.48851587, -1.13520398, 0.27886807, -0.18628806, 0.09678418, 0.37409196, 1.00002368, -1.26551223):
        p = p * t + c
    tail = t * 0.5 * torch.exp(p - z * z)
    return x * torch.where(x < 0, tail, 1.0 - tail)


def gelu_grad_as26_f32(x: torch.Tensor) -> torch.Tensor:
    x = x.to(torch.float32)
    t = 1.0 / (x.abs() * (0.3275911 * 0.70710678118654752) + 1.0)
    e = torch.exp(x * x * -0.5)
    p = t * 1.061405429 - 1.453152027
    for c in (1.421413741, -0.284496736, 0.254829592):
        p = p * t + c
    tail = p * t * 0.5 * e
    return x * 0.3989422804014327 * e + torch.where(x < 0, tail, 1.0 - tail)
