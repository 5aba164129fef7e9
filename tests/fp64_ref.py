"""float64 references of the step's contractions (convolutions, GEMMs, attention), computed from the same bf16 operands the kernels read.

Everything here runs in torch float64 on the operands' device: im2col (F.unfold) and torch.matmul, never an fp32 library convolution or GEMM
(those may take reduced-precision paths).  Beside every result r the helpers return S = sum |a b| over the products behind it (the same
matmul on |A| and |B|): the scale of the rounding error an fp32-accumulating kernel may make, whatever the signs.

Used by tests/test_step_contractions_fp64.py.
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
