"""The fp32 validation kernels (csrc/fp32.hip, csrc/vit_f32.hip, lp_bn_finalize_f32) held to float64, one entry point at a time.

Fp32Engine / ViTFp32Engine are what the bf16 product engines are judged against, and what holds a whole step to the reference at 1e-4; this
module is the kernel-level check of that yardstick.  Every reference is plain torch float64 on the same fp32 operands (tests/fp64_ref.py:
unfold + matmul, einsum, written-out formulas) - never an fp32 library call, never a bf16 product kernel.

entry point                          test
-----------------------------------  ---------------------------------------------------------------------------------------------
lp_f32_conv_fwd                      test_conv_fwd, test_argument_checks
lp_f32_conv_dgrad                    test_conv_dgrad, test_argument_checks
lp_f32_conv_wgrad                    test_conv_wgrad, test_argument_checks
lp_f32_bn_stats                      test_bn_stats                       (also tests/test_fp32_parity.py)
lp_f32_bn_stats_workspace_bytes      test_bn_stats
lp_f32_bn_stats_ordered              test_bn_stats                       (also tests/test_fp32_parity.py)
lp_bn_finalize_f32                   test_bn_finalize_f32, test_argument_checks
lp_f32_bn_apply                      test_bn_apply, test_argument_checks
lp_f32_bn_bwd_reduce                 test_bn_bwd_reduce
lp_f32_bn_bwd_apply                  test_bn_bwd_apply, test_argument_checks
lp_f32_maxpool_fwd / _bwd            test_maxpool, test_argument_checks
lp_f32_images_to_nhwc4               test_images_to_nhwc4
lp_f32_pixel_shuffle                 test_pixel_shuffle, test_argument_checks
lp_f32_softmax2d_bwd                 test_softmax2d_bwd, test_argument_checks
lp_f32_vit_patchify                  test_patchify, test_argument_checks
lp_f32_vit_tokens_fwd / _bwd         test_tokens
lp_f32_vit_mv_tokens_fwd / _bwd      tests/test_mvt_token_kernels.py     (precision "fp32")
lp_f32_layernorm_fwd                 test_layernorm_fwd, test_layernorm_fwd_without_delta_leaves_x_out_alone, test_argument_checks
lp_f32_layernorm_bwd                 test_layernorm_bwd
lp_f32_layernorm_ls_fwd / _bwd       tests/test_dinov2_layerscale_kernels.py
lp_f32_gelu_fwd / _bwd               test_gelu, test_argument_checks
lp_f32_attn_fwd / _bwd               test_attention, test_argument_checks

Bars.  Contractions and sums: |y - r| <= 2^-18 S, S = sum |a b| from the same float64 code (fp64_ref.f32_bar).  Stored probabilities:
|P - p| <= 2^-20 + 2^-18 p, rows summing to 1 within T 2^-23.  Data movement: exact.  Short formulas: c 2^-24 (sum of |terms|), c = the
roundings counted beside each bar.  GELU: see GELU_FWD_C.  Every family also builds a wrong reference from the same float64 code and
asserts that its bar REJECTS it (a bar that cannot fail proves nothing).  No element is excluded from any comparison.

Every case runs on the emulated build in the CPU suite and on the device under `-m gpu` (stack_backend) - the ones above 2^20 work items
and the 16770-row attention too: the emulator takes under two seconds for each.  MARGINS (entry point -> worst |y - r| / bar) is printed
at the end of the module with -s."""

from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass

import pytest
import torch

from lightning_pose_amd import _lib, ops
from tests import fp64_ref as R

F64 = torch.float64
U = 2.0 ** -24            # half an ulp of 1: the relative error of one fp32 rounding
SENT = 7.25               # what output buffers hold before a call: "untouched" means still this, bit for bit
LP_ERR_ARGUMENT, LP_ERR_UNSUPPORTED = -1, -2
MARGINS: dict = {}        # entry point (. output) -> worst |y - r| / bar over its cases

# GELU: the kernels call the device's erff / expf.  An independent fp32 evaluation - torch.nn.functional.gelu and its autograd in float32 on
# the CPU - of the inputs of test_gelu (1,053,700 values, N(0, 2^2), |x| up to 10.4) is off the float64 reference by at most
#     forward   5.26 units of 2^-24 (|y| + |x|)                    backward  9.08 units of 2^-24 |dy| (|gelu'(x)| + |x|)
# (measured with this module's _gelu_operands; the backward's unit is the forward's for dy = 1).  libm implementations differ by a couple
# of ulp, so the kernels get 4 x that.
GELU_FWD_C = 4 * 5.26
GELU_BWD_C = 4 * 9.08


@pytest.fixture(scope="module", autouse=True)
def _print_margins():
    yield
    print("\nMARGINS (worst |y - r| / bar):")
    for k in sorted(MARGINS):
        print(f"  {k:34s} {MARGINS[k]:.4f}")


# ---------------------------------------------------------------------------------------------------------------- helpers
def _t(dev, seed, *shape, scale=1.0, shift=0.0):
    """seeded fp32 operand, drawn on the host so that both backends see the same values"""
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale + shift).to(dev)


def _sent(dev, *shape):
    return torch.full(shape, SENT, device=dev)


def _call(name, *args):
    return getattr(_lib.lib(), name)(*[ops._p(a) if isinstance(a, torch.Tensor) else a for a in args], ops._stream())


def _run(name, *args):
    rc = _call(name, *args)
    assert rc == 0, (name, rc)


def _hold(name, y, r, bar):
    m = R.worst(y, r, bar)
    MARGINS[name] = max(MARGINS.get(name, 0.0), m)
    assert m <= 1.0, f"{name}: worst |y - r| / bar = {m:.3f}"


def _rejects(what, y, r_mutant, bar):
    m = R.worst(y, r_mutant, bar)
    assert m > 1.0, f"the bar accepts the mutant ({what}): worst = {m:.3f}"


def _twice(fn):
    """fn() -> tuple of fresh outputs; the same bits both times (kernels without floating-point atomics)"""
    a, b = fn(), fn()
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    return a


# ---------------------------------------------------------------------------------------------------------------- convolutions
@dataclass
class Geo:
    name: str
    B: int
    Hi: int
    Wi: int
    Ci: int
    Co: int
    k: int
    stride: int
    pad: int
    KH: int = 0
    KW: int = 0
    CiS: int = 0

    def __post_init__(self):
        self.KH, self.KW, self.CiS = self.KH or self.k, self.KW or self.k, self.CiS or self.Ci
        self.Ho = (self.Hi + 2 * self.pad - self.k) // self.stride + 1
        self.Wo = (self.Wi + 2 * self.pad - self.k) // self.stride + 1
        self.M = self.B * self.Ho * self.Wo

    def c(self):
        return _lib.ConvGeom(self.B, self.Hi, self.Wi, self.Ci, self.Ho, self.Wo, self.Co, self.k, self.k, self.stride, self.pad)

    def dims(self):
        return self.KH, self.KW, self.CiS


GEOS = [
    Geo("3x3s1_M35_Ci20_Co40", 1, 5, 7, 20, 40, 3, 1, 1),          # ragged M and N; forward: Ci % 8 != 0
    Geo("3x3s2_7x9to4x5_Ci16_Co33", 2, 7, 9, 16, 33, 3, 2, 1),     # Hi = 2 Ho - 1; data gradient: Co % 8 != 0, ragged N = 16
    Geo("3x3s2_8x10from4x5_op1", 2, 8, 10, 24, 20, 3, 2, 1),       # Hi = 2 Ho: the head's ConvTranspose k3 s2 p1 op1 as a data gradient
    Geo("1x1_M70_Ci72_Co33", 2, 5, 7, 72, 33, 1, 1, 0),
    Geo("stem_18x22_7x7in8x8x4", 1, 18, 22, 4, 64, 7, 2, 3, 8, 8, 4),   # Fp32Engine._wdims of the stem: KH, KW > R, S
    Geo("stem_18x22_Ci3in4", 1, 18, 22, 3, 64, 7, 2, 3, 8, 8, 4),       # ... and CiS > Ci
    Geo("3x3s1_M598_Ci5_Co7", 2, 13, 23, 5, 7, 3, 1, 1),           # weight gradient: three pixel slices of 200 / 200 / 198
]
GEO_IDS = [g.name for g in GEOS]


def _conv_epilogues(name, dev, seed, geom, dims, src, w, M, N, acc, s):
    """no epilogue; bias; bias + addend aliasing the output - each twice on fresh outputs, the same bits"""
    bias, addend = _t(dev, seed + 1, N), _t(dev, seed + 2, M, N)
    for ep in ("plain", "bias", "bias+addend=out"):
        def once():
            out = addend.clone() if "addend" in ep else _sent(dev, M, N)
            _run(name, src, w, C.byref(geom), *dims, bias if "bias" in ep else None, out if "addend" in ep else None, out)
            return (out,)
        out, = _twice(once)
        r, sb = acc.clone(), s.clone()
        if "bias" in ep:
            r, sb = r + bias.to(F64), sb + bias.to(F64).abs()
        if "addend" in ep:
            r, sb = r + addend.to(F64), sb + addend.to(F64).abs()
        _hold(name, out, r, R.f32_bar(sb))
        if ep == "plain":
            plain = out
    return plain


def _conv_mutants(name, A: R.ConvOperand, a, Wm, acc, s, y, want_shift):
    bar = R.f32_bar(s)
    taps = A.R * A.S
    if A.C % 8 != 0:   # the last channel of the ragged 8-channel step dropped (the `c < ck` guard)
        idx = torch.arange((A.C - 1) * taps, A.C * taps, device=a.device)
        _rejects(f"{name}: last channel dropped", y, acc - a[:, idx] @ Wm[:, idx].T, bar)
    # (over a zero-dilated gradient the neighbouring pixel is an inserted zero at either side of the row end: nothing to tell apart)
    sh = A.tap_shift_rows(1, A.S - 1) if A.R == A.S == 3 and A.dilate == 1 else None
    assert sh is not None or not want_shift, "no row end to shift a tap across"
    if sh is not None:
        m, orig, shifted = sh
        idx = A.kstep(1 * A.S + A.S - 1, 0, A.C)
        r = acc.clone()
        r[m] += (shifted - orig) @ Wm[:, idx].T
        _rejects(f"{name}: tap (1, {A.S - 1}) read across the row end", y, r, bar)


@pytest.mark.parametrize("g", GEOS, ids=GEO_IDS)
def test_conv_fwd(stack_backend, g):
    """f32_conv_kernel<0>: ragged M / N / channel step, storage dims larger than the filter, bias and aliased addend"""
    dev = stack_backend
    x, w = _t(dev, 11, g.B, g.Hi, g.Wi, g.Ci), _t(dev, 12, g.Co, g.KH, g.KW, g.CiS)   # (storage padding holds values too: none may be read)
    A = R.conv_fwd_operand(x, g.Ci, g.k, g.k, g.stride, g.pad)
    assert (A.Ho, A.Wo) == (g.Ho, g.Wo)
    a, Wm = A.rows(0, g.B), R.weight_matrix_fwd(w, g.k, g.k, g.Ci)
    acc, s = a @ Wm.T, a.abs() @ Wm.abs().T
    y = _conv_epilogues("lp_f32_conv_fwd", dev, 13, g.c(), g.dims(), x, w, g.M, g.Co, acc, s)
    _conv_mutants("lp_f32_conv_fwd", A, a, Wm, acc, s, y, want_shift=g.k == 3 and g.Wi % 2 == 1)


@pytest.mark.parametrize("g", GEOS, ids=GEO_IDS)
def test_conv_dgrad(stack_backend, g):
    """f32_conv_kernel<1>: the weight stride KH KW CiS over the contraction, stride 2 at both parities of Hi, bias (the head's ConvTranspose)"""
    dev = stack_backend
    dy, w = _t(dev, 21, g.B, g.Ho, g.Wo, g.Co), _t(dev, 22, g.Co, g.KH, g.KW, g.CiS)
    A = R.conv_dgrad_operand(dy, g.Co, g.k, g.k, g.stride, g.pad, g.Hi, g.Wi)
    assert (A.Ho, A.Wo) == (g.Hi, g.Wi)
    a, Wm = A.rows(0, g.B), R.conv_weight_dgrad_from_storage(w, g.k, g.k, g.Ci)
    acc, s = a @ Wm.T, a.abs() @ Wm.abs().T
    y = _conv_epilogues("lp_f32_conv_dgrad", dev, 23, g.c(), g.dims(), dy, w, g.B * g.Hi * g.Wi, g.Ci, acc, s)
    _conv_mutants("lp_f32_conv_dgrad", A, a, Wm, acc, s, y, want_shift=g.k == 3 and g.stride == 1)


def _wgrad_split(g: Geo) -> int:
    """the pixel slices lp_f32_conv_wgrad launches (its host formula)"""
    kw = g.k * g.k * g.Ci
    ntiles = -(-kw // 32) * -(-g.Co // 32)
    split = max(1, min(-(-2048 * 4 // ntiles), -(-g.M // 256), 65535))
    per = (-(-g.M // split) + 7) // 8 * 8
    return -(-g.M // per)


@pytest.mark.parametrize("g", GEOS, ids=GEO_IDS)
def test_conv_wgrad(stack_backend, g):
    """f32_wgrad_kernel: accumulated onto a non-zero dW, storage padding left bit for bit; M = 598 runs three slices, the last 198 rows
    (not a multiple of 8: the `m < m_end` guard).  fp32 atomics: no bit-identity asserted."""
    dev = stack_backend
    if g.M == 598:
        assert _wgrad_split(g) == 3
    x, dy = _t(dev, 31, g.B, g.Hi, g.Wi, g.Ci), _t(dev, 32, g.B, g.Ho, g.Wo, g.Co)
    dw0 = _t(dev, 33, g.Co, g.KH, g.KW, g.CiS)
    dw = dw0.clone()
    _run("lp_f32_conv_wgrad", x, dy, C.byref(g.c()), *g.dims(), dw)
    a = R.conv_fwd_operand(x, g.Ci, g.k, g.k, g.stride, g.pad).rows(0, g.B)
    inner = (slice(None), slice(0, g.k), slice(0, g.k), slice(0, g.Ci))
    r, s = R.conv_wgrad(a, dy, g.Co, g.Ci, g.k, g.k)
    r, s = r + dw0[inner].to(F64), s + dw0[inner].to(F64).abs()
    _hold("lp_f32_conv_wgrad", dw[inner], r, R.f32_bar(s))
    pad = torch.ones_like(dw0, dtype=torch.bool)
    pad[inner] = False
    assert torch.equal(dw[pad], dw0[pad])
    cut = a.clone()
    cut[-6:] = 0
    _rejects("weight gradient: last 6 pixel rows dropped", dw[inner], R.conv_wgrad(cut, dy, g.Co, g.Ci, g.k, g.k)[0] + dw0[inner].to(F64),
             R.f32_bar(s))


# ---------------------------------------------------------------------------------------------------------------- attention
def _attention(dev, B, nh, T):
    D3 = nh * 64
    ld, k_off, v_off, ldo = 3 * D3 + 24, D3 + 8, 2 * D3 + 16, D3 + 5     # q | 8 | k | 8 | v | 8: the blocks are not adjacent
    ldd, scale = ld, 0.125
    qkv = _t(dev, 41, B * T, ld)
    q, k, v = R.attn_split(qkv, B, nh, T, k_off, v_off)

    def fwd():
        p, o = _sent(dev, B * nh * T, T), _sent(dev, B * T, ldo)
        _run("lp_f32_attn_fwd", qkv, ld, k_off, v_off, B, nh, T, scale, p, o, ldo)
        return p, o
    p, o = _twice(fwd)
    P, O, So = R.attn_fwd(q, k, v, scale)
    pk = p.reshape(B, nh, T, T).to(F64)
    _hold("lp_f32_attn_fwd.p", pk, P, 2.0 ** -20 + 2.0 ** -18 * P)
    assert float((pk.sum(-1) - 1).abs().max()) <= T * 2.0 ** -23
    bar_o = R.f32_bar(R.heads_to_rows(So))
    _hold("lp_f32_attn_fwd.o", o[:, :D3], R.heads_to_rows(O), bar_o)
    assert bool((o[:, D3:] == SENT).all())
    if T > 1:
        P1, O1, _ = R.attn_fwd(q, k[:, :, :-1], v[:, :, :-1], scale)
        _rejects("attention: last key dropped (o)", o[:, :D3], R.heads_to_rows(O1), bar_o)
        _rejects("attention: last key dropped (p)", pk[..., :-1], P1, 2.0 ** -20 + 2.0 ** -18 * P1)

    dout = _t(dev, 42, B * T, ldo)

    def bwd():
        ds, dqkv = _sent(dev, B * nh * T, T), _sent(dev, B * T, ldd)
        _run("lp_f32_attn_bwd", qkv, ld, k_off, v_off, dout, ldo, p, B, nh, T, scale, ds, dqkv, ldd)
        return (dqkv,)
    dqkv, = _twice(bwd)
    do = dout[:, :D3].reshape(B, T, nh, 64).permute(0, 2, 1, 3).to(F64)
    (dq, dq_s), (dk, dk_s), (dv, dv_s) = R.attn_bwd(q, k, v, pk, do, scale)
    for what, off, r, s in (("dq", 0, dq, dq_s), ("dk", k_off, dk, dk_s), ("dv", v_off, dv, dv_s)):
        _hold("lp_f32_attn_bwd." + what, dqkv[:, off:off + D3], R.heads_to_rows(r), R.f32_bar(R.heads_to_rows(s)))
    gaps = torch.ones(ldd, dtype=torch.bool, device=dev)
    for off in (0, k_off, v_off):
        gaps[off:off + D3] = False
    assert bool((dqkv[:, gaps] == SENT).all())
    if T > 1:
        _rejects("attention: scale applied twice to dK", dqkv[:, k_off:k_off + D3], R.heads_to_rows(dk * scale), R.f32_bar(R.heads_to_rows(dk_s)))


@pytest.mark.parametrize("B,nh,T", [(1, 1, 65), (2, 2, 64), (1, 3, 1), (43, 6, 65)])
def test_attention(stack_backend, B, nh, T):
    """lp_f32_attn_fwd / _bwd: T = 65 (not a multiple of 64; 65 rows: three dead waves in the last workgroup, the `!live` path between
    the barriers), T = 64, T = 1 (3 rows); ld > 3 nh 64 with k_off / v_off not adjacent; ldo, ldd padded, pad columns untouched.
    43 x 6 x 65 = 16770 rows: more than 4096 workgroups x 4 waves, so workgroups make a second round with its barriers, and 16770 % 4 = 2
    leaves dead waves in the last one."""
    _attention(stack_backend, B, nh, T)


# ---------------------------------------------------------------------------------------------------------------- LayerNorm
LN_SHAPES = [(15, 100, 5), (7, 384, 0), (16400, 64, 0)]   # D % 64 != 0 with [CLS] rows dropped and 15 % 4 = 3; ViT-S; a second round of rows
LN_EPS = 1e-12


@pytest.mark.parametrize("M,D,drop_T", LN_SHAPES)
def test_layernorm_fwd(stack_backend, M, D, drop_T):
    """lp_f32_layernorm_fwd: delta NULL / given / given with x_out aliasing x; dropped rows still get mean and rstd; twice, the same bits"""
    dev = stack_backend
    x, delta = _t(dev, 51, M, D, shift=0.5), _t(dev, 52, M, D, scale=0.3)
    gamma, beta = _t(dev, 53, D, shift=1.0), _t(dev, 54, D)
    rows = R.kept_rows(M, drop_T, dev)
    for mode in ("plain", "delta", "delta, x_out = x"):
        def once():
            xin = x.clone()
            xo = None if mode == "plain" else (xin if "=" in mode else _sent(dev, M, D))
            y, mean, rstd = _sent(dev, len(rows), D), _sent(dev, M), _sent(dev, M)
            _run("lp_f32_layernorm_fwd", xin, None if mode == "plain" else delta, xo, gamma, beta, LN_EPS, M, D, drop_T, y, mean, rstd)
            return y, mean, rstd, xin if xo is None else xo
        y, mean, rstd, xo = _twice(once)
        # x_out = one fp32 sum: the correctly rounded float64 sum, bit for bit (plain: x is still what it was)
        xs32 = x if mode == "plain" else (x.to(F64) + delta.to(F64)).to(torch.float32)
        assert torch.equal(xo, xs32)
        xs = xs32.to(F64)
        mu = xs.mean(1)
        _hold("lp_f32_layernorm_fwd.mean", mean, mu, R.f32_bar(xs.abs().sum(1)) / D)
        # rstd = (var + eps)^-1/2: var is a sum of squares of differences, held to 2^-18 of the same sum on (|x| + |mean|) (the
        # cancellation in x - mean), which moves rstd by rstd / 2 * dvar / (var + eps); then three roundings (+ eps, sqrt, 1 / .)
        var = ((xs - mu[:, None]) ** 2).mean(1)
        rs = (var + LN_EPS) ** -0.5
        dvar = R.f32_bar(((xs.abs() + mu.abs()[:, None]) ** 2).sum(1)) / D
        _hold("lp_f32_layernorm_fwd.rstd", rstd, rs, rs * (0.5 * dvar / (var + LN_EPS) + 3 * U))
        # y = fma((x - mean) * rstd, gamma, beta) from the kernel's OWN mean / rstd (held above): the difference, the product and the
        # fused multiply-add round once each, so either term carries at most 3 roundings
        t = (xs - mean.to(F64)[:, None]) * rstd.to(F64)[:, None] * gamma.to(F64)
        yr, bar = t + beta.to(F64), 3 * U * (t.abs() + beta.to(F64).abs())
        _hold("lp_f32_layernorm_fwd.y", y, yr[rows], bar[rows])
        if drop_T:
            off = R.kept_rows(M, drop_T, dev, shift=1)
            _rejects("LayerNorm forward: drop_T mapping off by one row", y, yr[off], bar[off])


def test_layernorm_fwd_without_delta_leaves_x_out_alone(stack_backend):
    """The contract include/lp_hip.h states: with delta == NULL, lp_f32_layernorm_fwd never writes x_out (the caller keeps using x), while
    the bf16 form lp_layernorm_fwd copies x into a non-NULL x_out.  Neither engine passes an x_out without a delta."""
    dev = stack_backend
    M, D = 15, 100
    x, gamma, beta = _t(dev, 55, M, D), _t(dev, 56, D), _t(dev, 57, D)
    xo, y, mean, rstd = _sent(dev, M, D), _sent(dev, M, D), _sent(dev, M), _sent(dev, M)
    _run("lp_f32_layernorm_fwd", x, None, xo, gamma, beta, LN_EPS, M, D, 0, y, mean, rstd)
    assert bool((xo == SENT).all()) and not bool((y == SENT).any())
    xo, y16 = _sent(dev, M, D), torch.zeros(M, D, dtype=torch.int16, device=dev)
    _run("lp_layernorm_fwd", x, None, xo, gamma, beta, LN_EPS, M, D, 0, y16, mean, rstd)
    assert torch.equal(xo, x)


@pytest.mark.parametrize("M,D,drop_T", LN_SHAPES)
def test_layernorm_bwd(stack_backend, M, D, drop_T):
    """lp_f32_layernorm_bwd: dx_acc, dgamma and dbeta accumulated onto non-zero values; dropped rows' dx_acc stays bit for bit.
    dgamma / dbeta are fp32 atomics (no bit-identity asserted)."""
    dev = stack_backend
    x, gamma = _t(dev, 61, M, D, shift=0.5), _t(dev, 62, D, shift=1.0)
    rows = R.kept_rows(M, drop_T, dev)
    dy = _t(dev, 63, len(rows), D)
    xs = x.to(F64)
    mean = xs.mean(1).to(torch.float32)
    rstd = ((xs.var(1, unbiased=False) + LN_EPS) ** -0.5).to(torch.float32)
    dx0, dg0, db0 = _t(dev, 64, M, D), _t(dev, 65, D), _t(dev, 66, D)
    dx, dg, db = dx0.clone(), dg0.clone(), db0.clone()
    _run("lp_f32_layernorm_bwd", dy, x, mean, rstd, gamma, M, D, drop_T, dx, dg, db)
    xh_all = (xs - mean.to(F64)[:, None]) * rstd.to(F64)[:, None]

    def ref(sel):
        """dy row j belongs to input row sel[j]: -> (dx, bar) on the rows sel, dgamma, its S"""
        xh, rs, g = xh_all[sel], rstd.to(F64)[sel][:, None], dy.to(F64) * gamma.to(F64)
        a, b = g.mean(1, keepdim=True), (g * xh).mean(1, keepdim=True)
        a_s, b_s = g.abs().mean(1, keepdim=True), (g * xh).abs().mean(1, keepdim=True)
        r = dx0.to(F64)[sel] + rs * (g - a - xh * b)
        # the two row means are sums held to 2^-18 of their |terms|; around them dy gamma, xhat (two roundings), xhat b, the two
        # differences, the product with rstd and the sum onto dx_acc: no term passes through more than 7 roundings
        terms = rs * (g.abs() + a_s + xh.abs() * b_s) + dx0.to(F64)[sel].abs()
        bar = 2.0 ** -18 * rs * (a_s + xh.abs() * b_s) + 7 * U * terms
        return r, bar, dg0.to(F64) + (dy.to(F64) * xh).sum(0), dg0.to(F64).abs() + (dy.to(F64) * xh).abs().sum(0)
    r, bar, dgr, dgs = ref(rows)
    _hold("lp_f32_layernorm_bwd.dx", dx[rows], r, bar)
    _hold("lp_f32_layernorm_bwd.dgamma", dg, dgr, R.f32_bar(dgs))
    _hold("lp_f32_layernorm_bwd.dbeta", db, db0.to(F64) + dy.to(F64).sum(0), R.f32_bar(db0.to(F64).abs() + dy.to(F64).abs().sum(0)))
    if drop_T:
        dropped = torch.arange(0, M, drop_T, device=dev)
        assert torch.equal(dx[dropped], dx0[dropped])
        off = R.kept_rows(M, drop_T, dev, shift=1)
        rm, barm, dgm, _ = ref(off)
        full = dx0.to(F64).clone()
        full[off] = rm
        _rejects("LayerNorm backward: drop_T mapping off by one row (dx)", dx[rows], full[rows], bar)
        _rejects("LayerNorm backward: drop_T mapping off by one row (dgamma)", dg, dgm, R.f32_bar(dgs))


# ---------------------------------------------------------------------------------------------------------------- GELU
def _gelu_operands(dev):
    M, C_ = 4100, 257     # 1,053,700 > 2^20 elements: the grid-stride loop runs; nothing a multiple of 64
    return _t(dev, 71, M, C_, scale=2.0), _t(dev, 72, M, C_)


def _gelu(dev, x, dy):
    n = x.numel()

    def once():
        y, dx = _sent(dev, *x.shape), _sent(dev, *x.shape)
        _run("lp_f32_gelu_fwd", x, C.c_size_t(n), y)
        _run("lp_f32_gelu_bwd", x, dy, C.c_size_t(n), dx)
        return y, dx
    y, dx = _twice(once)
    xd, dyd = x.to(F64), dy.to(F64)
    r, gr = R.gelu(xd), R.gelu_grad(xd)
    _hold("lp_f32_gelu_fwd", y, r, GELU_FWD_C * U * (r.abs() + xd.abs()))
    _hold("lp_f32_gelu_bwd", dx, dyd * gr, GELU_BWD_C * U * dyd.abs() * (gr.abs() + xd.abs()))
    _rejects("GELU: tanh approximation", y, 0.5 * xd * (1 + torch.tanh(math.sqrt(2 / math.pi) * (xd + 0.044715 * xd ** 3))),
             GELU_FWD_C * U * (r.abs() + xd.abs()))


@pytest.mark.parametrize("n", [1000, 0], ids=["n1000", "above_2^20"])
def test_gelu(stack_backend, n):
    """lp_f32_gelu_fwd / _bwd on 1000 values with the edge ones among them, and above 2^20 elements (f32_grid's cap of 4096 workgroups:
    the grid-stride loop)"""
    dev = stack_backend
    x, dy = _gelu_operands(dev)
    if n:
        x, dy = x.reshape(-1)[:n].clone(), dy.reshape(-1)[:n].clone()
        x[:8] = torch.tensor([0.0, -0.0, 1e-30, -1e-30, 6.0, -6.0, 12.0, -12.0], device=dev)
    _gelu(dev, x, dy)


# ---------------------------------------------------------------------------------------------------------------- BatchNorm
BN_SHAPES = [(16500, 70), (3, 8)]    # M >= 16384: the row stripes are capped at 256; C no multiple of 64.  And the smallest.


@pytest.mark.parametrize("M,C_", BN_SHAPES)
def test_bn_stats(stack_backend, M, C_):
    """lp_f32_bn_stats (atomics) and lp_f32_bn_stats_ordered (the same bits twice), accumulated onto non-zero sums"""
    dev = stack_backend
    x, s0 = _t(dev, 81, M, C_, shift=0.5), _t(dev, 82, 2 * C_)
    xd = x.to(F64)
    r = s0.to(F64) + torch.cat([xd.sum(0), (xd * xd).sum(0)])
    bar = R.f32_bar(s0.to(F64).abs() + torch.cat([xd.abs().sum(0), (xd * xd).sum(0)]))
    s = s0.clone()
    _run("lp_f32_bn_stats", x, M, C_, s)
    _hold("lp_f32_bn_stats", s, r, bar)
    nws = int(_lib.lib().lp_f32_bn_stats_workspace_bytes(M, C_))
    assert nws == max(1, min(256, M // 64)) * 4 * 2 * C_ * 4

    def once():
        s, ws = s0.clone(), torch.full((nws // 4,), math.nan, device=dev)   # (every partial that is read must have been written)
        _run("lp_f32_bn_stats_ordered", x, M, C_, s, ws, C.c_size_t(nws))
        return (s,)
    s, = _twice(once)
    _hold("lp_f32_bn_stats_ordered", s, r, bar)
    cut = xd.clone()
    cut[-1] = 0
    _rejects("BatchNorm sums: last row dropped", s, s0.to(F64) + torch.cat([cut.sum(0), (cut * cut).sum(0)]), bar)


@pytest.mark.parametrize("count,running", [(37.0, True), (37.0, False), (1.0, True)])
def test_bn_finalize_f32(stack_backend, count, running):
    """lp_bn_finalize_f32: mean, invstd and the running statistics (momentum, unbiased variance; count = 1: the biased one)"""
    dev = stack_backend
    C_, eps, mom = 70, 1e-5, 0.1
    xd = _t(dev, 91, int(count), C_, shift=0.5).to(F64)
    sums = torch.cat([xd.sum(0), (xd * xd).sum(0)]).to(torch.float32)
    rm0, rv0 = _t(dev, 92, C_), _t(dev, 93, C_).abs() + 0.5
    rm, rv = rm0.clone(), rv0.clone()
    mean, invstd = _sent(dev, C_), _sent(dev, C_)
    _run("lp_bn_finalize_f32", sums, count, C_, eps, mom, mean, invstd, rm if running else None, rv if running else None)
    s1, s2 = sums[:C_].to(F64), sums[C_:].to(F64)
    mu = s1 / count                                              # one rounding
    _hold("lp_bn_finalize_f32.mean", mean, mu, U * mu.abs())
    # var = s2 / n - mu mu: the quotient rounds once, mu mu carries mu's rounding twice and its own, the difference rounds once
    var = (s2 / count - mu * mu).clamp_min(0)
    dvar = 4 * U * (s2 / count + mu * mu)
    inv = (var + eps) ** -0.5
    # ... which moves invstd by invstd / 2 * dvar / (var + eps); then + eps, sqrt and 1 / . round once each
    _hold("lp_bn_finalize_f32.invstd", invstd, inv, inv * (0.5 * dvar / (var + eps) + 3 * U))
    if not running:
        return
    # running = (1 - m) old + m new: 1 - m, either product and the sum round; new carries its own (mean: 1; variance: dvar, then
    # * n and / (n - 1)): at most 4 roundings per term
    _hold("lp_bn_finalize_f32.running_mean", rm, (1 - mom) * rm0.to(F64) + mom * mu, 4 * U * ((1 - mom) * rm0.to(F64).abs() + mom * mu.abs()))
    k = count / (count - 1) if count > 1 else 1.0
    _hold("lp_bn_finalize_f32.running_var", rv, (1 - mom) * rv0.to(F64) + mom * var * k,
          mom * k * dvar + 4 * U * ((1 - mom) * rv0.to(F64) + mom * var * k))
    if count > 1:
        _rejects("BatchNorm finalize: biased running variance", rv, (1 - mom) * rv0.to(F64) + mom * var,
                 mom * k * dvar + 4 * U * ((1 - mom) * rv0.to(F64) + mom * var * k))


def _bn_operands(dev, M, C_):
    x = _t(dev, 101, M, C_, shift=0.5)
    mean, invstd = _t(dev, 102, C_, scale=0.2, shift=0.5), _t(dev, 103, C_, scale=0.1).abs() + 0.8
    gamma, beta = _t(dev, 104, C_, shift=1.0), _t(dev, 105, C_)
    return x, mean, invstd, gamma, beta


def _bn_apply(dev, M, C_):
    x, mean, invstd, gamma, beta = _bn_operands(dev, M, C_)
    res = _t(dev, 106, M, C_)
    t = (x.to(F64) - mean.to(F64)) * invstd.to(F64) * gamma.to(F64)
    for residual, relu in ((None, 0), (res, 1), (None, 1)):
        def once():
            y = _sent(dev, M, C_)
            _run("lp_f32_bn_apply", x, mean, invstd, gamma, beta, residual, relu, M, C_, y)
            return (y,)
        y, = _twice(once)
        # (x - mean) invstd gamma + beta (+ residual): the difference, two products and one sum per further term round once each -
        # at most 5 roundings on any term; max(., 0) moves nothing further apart
        r, terms = t + beta.to(F64), t.abs() + beta.to(F64).abs()
        if residual is not None:
            r, terms = r + res.to(F64), terms + res.to(F64).abs()
        _hold("lp_f32_bn_apply", y, r.clamp_min(0) if relu else r, 5 * U * terms)
        if relu:
            _rejects("BatchNorm apply: no ReLU", y, r, 5 * U * terms)


@pytest.mark.parametrize("M,C_", [(3, 8), (130, 70), (4100, 257)])
def test_bn_apply(stack_backend, M, C_):
    """lp_f32_bn_apply with and without residual / ReLU; 4100 x 257 = 1,053,700 > 2^20 elements (the grid-stride loop), C odd"""
    _bn_apply(stack_backend, M, C_)


def _bn_bwd_operands(dev, M, C_):
    x, mean, invstd, gamma, _ = _bn_operands(dev, M, C_)
    dy = _t(dev, 111, M, C_)
    y_out = (_t(dev, 112, M, C_) * 2).round().clamp_min(0) / 2      # a ReLU output quantised to halves: exact zeros are common
    assert 0.3 < float((y_out == 0).double().mean()) < 0.9
    return x, mean, invstd, gamma, dy, y_out


@pytest.mark.parametrize("M,C_", BN_SHAPES)
def test_bn_bwd_reduce(stack_backend, M, C_):
    """lp_f32_bn_bwd_reduce: y_out NULL and given (an exact 0 masks the gradient), dbeta_acc / dgamma_acc NULL and accumulated onto
    non-zero values.  fp32 atomics: no bit-identity asserted."""
    dev = stack_backend
    x, mean, invstd, gamma, dy, y_out = _bn_bwd_operands(dev, M, C_)
    xh = (x.to(F64) - mean.to(F64)) * invstd.to(F64)
    s0, db0, dg0 = _t(dev, 113, 2 * C_), _t(dev, 114, C_), _t(dev, 115, C_)

    def sums(d):
        return torch.cat([d.sum(0), (d * xh).sum(0)]), torch.cat([d.abs().sum(0), (d * xh).abs().sum(0)])
    for masked, acc in ((False, False), (True, True), (True, False)):
        s, db, dg = s0.clone(), db0.clone(), dg0.clone()
        _run("lp_f32_bn_bwd_reduce", dy, y_out if masked else None, x, mean, invstd, M, C_, s, db if acc else None, dg if acc else None)
        d = dy.to(F64) * (y_out > 0) if masked else dy.to(F64)
        r, rs = sums(d)
        bar = R.f32_bar(s0.to(F64).abs() + rs)
        _hold("lp_f32_bn_bwd_reduce.sums", s, s0.to(F64) + r, bar)
        for name, got, g0, half in (("dbeta", db, db0, 0), ("dgamma", dg, dg0, 1)):
            if acc:
                sl = slice(half * C_, (half + 1) * C_)
                _hold("lp_f32_bn_bwd_reduce." + name, got, g0.to(F64) + r[sl], R.f32_bar(g0.to(F64).abs() + rs[sl]))
            else:
                assert torch.equal(got, g0)
        if masked:
            _rejects("BatchNorm backward reduce: y_out == 0 let through", s, s0.to(F64) + sums(dy.to(F64) * (y_out >= 0))[0], bar)


def _bn_bwd_apply(dev, M, C_):
    x, mean, invstd, gamma, dy, y_out = _bn_bwd_operands(dev, M, C_)
    xh = (x.to(F64) - mean.to(F64)) * invstd.to(F64)
    for masked, want_res in ((False, False), (True, True)):
        d32 = dy * (y_out > 0) if masked else dy
        d = d32.to(F64)
        sums = torch.cat([d.sum(0), (d * xh).sum(0)]).to(torch.float32)     # (an operand: whatever fp32 values the caller reduced)

        def once():
            dx, dres = _sent(dev, M, C_), _sent(dev, M, C_)
            _run("lp_f32_bn_bwd_apply", dy, y_out if masked else None, x, mean, invstd, gamma, sums, float(M), M, C_, dx, dres if want_res else None)
            return dx, dres
        dx, dres = _twice(once)
        assert torch.equal(dres, d32) if want_res else bool((dres == SENT).all())    # dres = the masked dy, a copy
        s1, s2, gi = sums[:C_].to(F64), sums[C_:].to(F64), gamma.to(F64) * invstd.to(F64)

        def ref(dd):
            return gi * (dd - s1 / M - xh * s2 / M), gi.abs() * (dd.abs() + s1.abs() / M + (xh * s2).abs() / M)
        r, terms = ref(d)
        # gamma invstd (d - s1 / n - xhat s2 / n): 1 / n rounds once and so does every product, difference and xhat's two steps - the
        # last term passes through 8 roundings (xhat 2, xhat s2, 1 / n, (.) / n, the difference, gamma invstd, the final product)
        _hold("lp_f32_bn_bwd_apply", dx, r, 8 * U * terms)
        if masked:
            _rejects("BatchNorm backward apply: y_out == 0 let through", dx, ref(dy.to(F64) * (y_out >= 0))[0], 8 * U * terms)


@pytest.mark.parametrize("M,C_", [(3, 8), (130, 70), (4100, 257)])
def test_bn_bwd_apply(stack_backend, M, C_):
    """lp_f32_bn_bwd_apply: y_out and dres NULL and given (an exact 0 in y_out masks the gradient; dres = the masked dy); 4100 x 257 >
    2^20 elements (the grid-stride loop), C odd"""
    _bn_bwd_apply(stack_backend, M, C_)


# ---------------------------------------------------------------------------------------------------------------- max-pool
def _maxpool(dev, B, H, W, C_):
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    x = _t(dev, 121, B, H, W, C_, scale=1.5).round()          # a few integer values: ties in most windows
    dy = _t(dev, 122, B, Ho, Wo, C_)

    def once():
        y, arg, dx = _sent(dev, B, Ho, Wo, C_), torch.full((B, Ho, Wo, C_), 255, dtype=torch.uint8, device=dev), _sent(dev, B, H, W, C_)
        _run("lp_f32_maxpool_fwd", x, B, H, W, C_, y, arg)
        _run("lp_f32_maxpool_bwd", arg, dy, B, H, W, C_, dx)
        return y, arg, dx
    y, arg, dx = _twice(once)
    m, first = R.maxpool_fwd(x)
    assert torch.equal(y.to(F64), m) and torch.equal(arg, first)
    r, s = R.maxpool_bwd(first, dy, H, W)
    # a pixel is the arg-max of up to four overlapping windows (odd rows / columns sit in two): three fp32 additions
    _hold("lp_f32_maxpool_bwd", dx, r, 3 * U * s)
    if H * W > 1:
        _, last = R.maxpool_fwd(x, last=True)
        assert float((last != first).double().mean()) > 0.2     # ties resolved to the last maximum: rejected by the equality above
        _rejects("max-pool backward: ties resolved to the last maximum", dx, R.maxpool_bwd(last, dy, H, W)[0], 3 * U * s)


@pytest.mark.parametrize("B,H,W,C_", [(2, 7, 9, 5), (1, 8, 6, 3), (1, 1, 1, 2), (1, 127, 131, 257)])
def test_maxpool(stack_backend, B, H, W, C_):
    """lp_f32_maxpool_fwd / _bwd: odd and even Hi, Wi (the backward's windows overlap at the odd input rows / columns, the last of an
    even size has one); values and arg-max bytes exact, first maximum in row-major order.  127 x 131 x 257 -> 64 x 66 x 257 =
    1,085,568 > 2^20 outputs (the grid-stride loop of both directions)."""
    _maxpool(stack_backend, B, H, W, C_)


# ---------------------------------------------------------------------------------------------------------------- data movement
def _pixel_shuffle(dev, B, h, w, c, ld):
    lo, hi = _t(dev, 131, B, h, w, 4 * c), _t(dev, 132, B, 2 * h, 2 * w, ld)

    def once():
        up, down = _sent(dev, B, 2 * h, 2 * w, ld), _sent(dev, B, h, w, 4 * c)
        _run("lp_f32_pixel_shuffle", lo, B, h, w, c, ld, 0, up)
        _run("lp_f32_pixel_shuffle", hi, B, h, w, c, ld, 1, down)
        return up, down
    up, down = _twice(once)
    assert torch.equal(up[..., :c], R.pixel_shuffle(lo, c)) and bool((up[..., c:] == SENT).all())
    assert torch.equal(down, R.pixel_unshuffle(hi[..., :c]))


@pytest.mark.parametrize("B,h,w,c,ld", [(2, 3, 5, 3, 8), (1, 2, 2, 5, 5), (1, 32, 33, 250, 257)])
def test_pixel_shuffle(stack_backend, B, h, w, c, ld):
    """lp_f32_pixel_shuffle, both directions, ld > c_out: exact, pad channels untouched; 32 x 33 x 1000 = 1,056,000 > 2^20 elements"""
    _pixel_shuffle(stack_backend, B, h, w, c, ld)


def _images_to_nhwc4(dev, B, H, W):
    img = _t(dev, 141, B, 3, H, W)

    def once():
        out = _sent(dev, B, H, W, 4)
        _run("lp_f32_images_to_nhwc4", img, B, H, W, out)
        return (out,)
    out, = _twice(once)
    assert torch.equal(out[..., :3], img.permute(0, 2, 3, 1)) and bool((out[..., 3] == 0).all())


@pytest.mark.parametrize("B,H,W", [(2, 5, 7), (1, 1, 1), (1, 1025, 1027)])
def test_images_to_nhwc4(stack_backend, B, H, W):
    """lp_f32_images_to_nhwc4: exact, channel 3 = 0; 1025 x 1027 = 1,052,675 > 2^20 pixels"""
    _images_to_nhwc4(stack_backend, B, H, W)


def _patchify(dev, B, H, W, P):
    img = _t(dev, 151, B, 3, H, W)

    def once():
        out = _sent(dev, B * (H // P) * (W // P), 3 * P * P)
        _run("lp_f32_vit_patchify", img, B, H, W, P, out)
        return (out,)
    out, = _twice(once)
    assert torch.equal(out, R.patchify(img, P))


@pytest.mark.parametrize("B,H,W,P", [(2, 32, 48, 16), (1, 6, 9, 3), (1, 592, 592, 16)])
def test_patchify(stack_backend, B, H, W, P):
    """lp_f32_vit_patchify: exact; 3 x 592 x 592 = 1,051,392 > 2^20 elements"""
    _patchify(stack_backend, B, H, W, P)


def _tokens(dev, B, Np, D):
    patch, cls, pos = _t(dev, 161, B * Np, D), _t(dev, 162, D), _t(dev, 163, Np + 1, D)

    def fwd():
        x = _sent(dev, B, Np + 1, D)
        _run("lp_f32_vit_tokens_fwd", patch, cls, pos, B, Np, D, x)
        return (x,)
    x, = _twice(fwd)
    tok = torch.cat([cls.to(F64).expand(B, 1, D), patch.to(F64).reshape(B, Np, D)], 1)
    assert torch.equal(x, (tok + pos.to(F64)).to(torch.float32))     # one fp32 sum: the correctly rounded float64 one
    dx = _t(dev, 164, B, Np + 1, D)

    def bwd():
        dpatch, dpos = _sent(dev, B * Np, D), _sent(dev, Np + 1, D)
        _run("lp_f32_vit_tokens_bwd", dx, B, Np, D, dpatch, dpos)
        return dpatch, dpos
    dpatch, dpos = _twice(bwd)
    assert torch.equal(dpatch, dx[:, 1:].reshape(B * Np, D))
    _hold("lp_f32_vit_tokens_bwd.dpos", dpos, dx.to(F64).sum(0), R.f32_bar(dx.to(F64).abs().sum(0)))
    if B > 1:
        _rejects("token backward: last image dropped from dpos", dpos, dx[:-1].to(F64).sum(0), R.f32_bar(dx.to(F64).abs().sum(0)))


@pytest.mark.parametrize("B,Np,D", [(3, 6, 100), (1, 1, 8), (2, 2051, 257)])
def test_tokens(stack_backend, B, Np, D):
    """lp_f32_vit_tokens_fwd (copy + one sum: exact) and _bwd (dpatch a copy, dpos a sum over the images); 2 x 2052 x 257 = 1,054,728 >
    2^20 elements"""
    _tokens(stack_backend, B, Np, D)


# ---------------------------------------------------------------------------------------------------------------- soft-max backward
@pytest.mark.parametrize("B,K,h,w,CPAD", [(2, 3, 15, 23, 8), (1, 1, 1, 1, 8)])
def test_softmax2d_bwd(stack_backend, B, K, h, w, CPAD):
    """lp_f32_softmax2d_bwd into the head's strided layout (B, n, CPAD), n = 345 not a multiple of 256; pad channels untouched"""
    dev = stack_backend
    n = h * w
    prob = torch.softmax(_t(dev, 171, B, K, n, scale=2.0).to(F64), -1).to(torch.float32)
    g = _t(dev, 172, B, K, n)

    def once():
        gin = _sent(dev, B, n, CPAD)
        _run("lp_f32_softmax2d_bwd", prob, g, B, K, n, gin, n * CPAD, CPAD, 1)
        return (gin,)
    gin, = _twice(once)
    p, gd = prob.to(F64), g.to(F64)
    dot, dot_s = (p * gd).sum(-1, keepdim=True), (p * gd).abs().sum(-1, keepdim=True)
    # p (g - dot): dot is a sum held to 2^-18 of its |terms|; the difference and the product round once each
    bar = p * 2.0 ** -18 * dot_s + 2 * U * p * (gd.abs() + dot.abs())
    _hold("lp_f32_softmax2d_bwd", gin[..., :K].permute(0, 2, 1), p * (gd - dot), bar)
    assert bool((gin[..., K:] == SENT).all())
    if n > 1:
        _rejects("soft-max backward: the row dot left out", gin[..., :K].permute(0, 2, 1), p * gd, bar)


# ---------------------------------------------------------------------------------------------------------------- argument checks
def test_argument_checks(stack_backend):
    """null required pointers, non-positive dims, KH < R, CiS < Ci, ld < nh 64, count <= 0: LP_ERR_ARGUMENT; patchify with H % patch != 0:
    LP_ERR_UNSUPPORTED; the output buffer unchanged every time"""
    dev = stack_backend
    a, out = _t(dev, 181, 4096), _sent(dev, 4096)
    u8 = torch.zeros(4096, dtype=torch.uint8, device=dev)
    g = Geo("ok", 1, 4, 4, 4, 4, 3, 1, 1)

    def geo(**kw):
        c = g.c()
        for k, v in kw.items():
            setattr(c, k, v)
        return C.byref(c)
    bad = [
        ("lp_f32_conv_fwd", (None, a, geo(), 3, 3, 4, None, None, out)),
        ("lp_f32_conv_fwd", (a, a, geo(), 3, 3, 4, None, None, None)),
        ("lp_f32_conv_fwd", (a, a, geo(B=0), 3, 3, 4, None, None, out)),
        ("lp_f32_conv_fwd", (a, a, geo(stride=0), 3, 3, 4, None, None, out)),
        ("lp_f32_conv_fwd", (a, a, geo(), 2, 3, 4, None, None, out)),          # KH < R
        ("lp_f32_conv_fwd", (a, a, geo(), 3, 2, 4, None, None, out)),          # KW < S
        ("lp_f32_conv_fwd", (a, a, geo(), 3, 3, 3, None, None, out)),          # CiS < Ci
        ("lp_f32_conv_dgrad", (a, None, geo(), 3, 3, 4, None, None, out)),
        ("lp_f32_conv_dgrad", (a, a, geo(Hi=-1), 3, 3, 4, None, None, out)),
        ("lp_f32_conv_dgrad", (a, a, geo(), 2, 3, 4, None, None, out)),
        ("lp_f32_conv_dgrad", (a, a, geo(), 3, 3, 3, None, None, out)),
        ("lp_f32_conv_wgrad", (a, None, geo(), 3, 3, 4, out)),
        ("lp_f32_conv_wgrad", (a, a, geo(Co=0), 3, 3, 4, out)),
        ("lp_f32_conv_wgrad", (a, a, geo(), 3, 3, 3, out)),
        ("lp_f32_bn_stats", (a, 0, 8, out)),
        ("lp_f32_bn_stats_ordered", (a, 8, 8, out, None, C.c_size_t(1 << 20))),
        ("lp_f32_bn_apply", (a, None, a, a, a, None, 0, 8, 8, out)),
        ("lp_f32_bn_apply", (a, a, a, a, a, None, 0, 8, 0, out)),
        ("lp_f32_bn_bwd_reduce", (a, None, a, a, None, 8, 8, out, None, None)),
        ("lp_f32_bn_bwd_apply", (a, None, a, a, a, a, a, 0.0, 8, 8, out, None)),       # count <= 0
        ("lp_f32_bn_bwd_apply", (a, None, a, a, a, a, a, -64.0, 8, 8, out, None)),
        ("lp_f32_bn_bwd_apply", (a, None, a, a, a, a, None, 64.0, 8, 8, out, None)),
        ("lp_bn_finalize_f32", (a, 0.0, 8, 1e-5, 0.1, out, out, None, None)),
        ("lp_bn_finalize_f32", (a, 8.0, 0, 1e-5, 0.1, out, out, None, None)),
        ("lp_bn_finalize_f32", (None, 8.0, 8, 1e-5, 0.1, out, out, None, None)),
        ("lp_f32_maxpool_fwd", (a, 1, 4, 4, 0, out, u8)),
        ("lp_f32_maxpool_fwd", (a, 1, 4, 4, 4, out, None)),
        ("lp_f32_maxpool_bwd", (None, a, 1, 4, 4, 4, out)),
        ("lp_f32_images_to_nhwc4", (a, 1, 0, 4, out)),
        ("lp_f32_pixel_shuffle", (a, 1, 2, 2, 4, 3, 0, out)),                  # ld < c_out
        ("lp_f32_pixel_shuffle", (a, 1, 2, -2, 4, 4, 1, out)),
        ("lp_f32_softmax2d_bwd", (a, a, 1, 3, 0, out, 80, 8, 1)),
        ("lp_f32_softmax2d_bwd", (a, None, 1, 3, 10, out, 80, 8, 1)),
        ("lp_f32_vit_patchify", (a, 1, 16, 16, 0, out)),
        ("lp_f32_vit_tokens_fwd", (a, a, None, 1, 4, 8, out)),
        ("lp_f32_vit_tokens_bwd", (a, 1, 0, 8, out, out)),
        ("lp_f32_layernorm_fwd", (a, None, None, None, a, 1e-6, 4, 8, 0, out, out, out)),
        ("lp_f32_layernorm_fwd", (a, None, None, a, a, 1e-6, 0, 8, 0, out, out, out)),
        ("lp_f32_layernorm_fwd", (a, None, None, a, a, 1e-6, 4, 8, -1, out, out, out)),
        ("lp_f32_layernorm_fwd", (a, a, None, a, a, 1e-6, 4, 8, 0, out, out, out)),     # delta without an x_out
        ("lp_f32_layernorm_bwd", (a, a, a, a, a, 4, 0, 0, out, out, out)),
        ("lp_f32_layernorm_bwd", (a, a, a, a, a, 4, 8, 0, out, None, out)),
        ("lp_f32_gelu_fwd", (a, C.c_size_t(0), out)),
        ("lp_f32_gelu_bwd", (a, None, C.c_size_t(8), out)),
        ("lp_f32_attn_fwd", (a, 63, 0, 0, 1, 1, 2, 0.125, out, out, 64)),      # ld < nh 64
        ("lp_f32_attn_fwd", (a, 192, 64, 128, 1, 1, 2, 0.125, out, out, 63)),  # ldo < nh 64
        ("lp_f32_attn_fwd", (a, 192, 64, 128, 1, 1, 0, 0.125, out, out, 64)),
        ("lp_f32_attn_fwd", (a, 192, 64, 128, 1, 1, 2, 0.125, None, out, 64)),
        ("lp_f32_attn_bwd", (a, 127, 0, 0, a, 128, a, 1, 2, 2, 0.125, out, out, 384)),
        ("lp_f32_attn_bwd", (a, 384, 128, 256, a, 128, a, 1, 2, 2, 0.125, out, out, 127)),
        ("lp_f32_attn_bwd", (a, 384, 128, 256, a, 128, a, 1, 2, 2, 0.125, None, out, 384)),
    ]
    for name, args in bad:
        assert _call(name, *args) == LP_ERR_ARGUMENT, (name, args)
    for H, W in ((17, 16), (16, 20)):
        assert _call("lp_f32_vit_patchify", a, 1, H, W, 16, out) == LP_ERR_UNSUPPORTED
    assert bool((out == SENT).all())
