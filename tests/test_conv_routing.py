"""Which kernel family every forward / data-gradient entry point of csrc/conv.hip launches: one row per shape rule and per switch, at the
smallest shape where the rule flips.  The expected lp_conv_last_kernel() id and return code of every row were RECORDED from the build of the
commit before route_conv() existed (its six separate if-ladders) and are literals here, so the table pins what the router must keep
deciding, not what it happens to decide.  Each row also checks that the launch wrote the whole output (finite and not all zero over a
NaN-filled buffer) or, for a refused call, that neither the output nor the last-kernel id was touched."""

import ctypes as C

import numpy as np
import pytest

from lightning_pose_amd import _lib
from tests.hipemu import emu

pytestmark = pytest.mark.usefixtures("kernel_backend")

IGEMM, PIPE, HALO, RES2D = _lib.CONV_KERNEL_IGEMM, _lib.CONV_KERNEL_PIPE, _lib.CONV_KERNEL_PIPE_HALO, _lib.CONV_KERNEL_RES2D
OK, UNSUPPORTED = 0, -2
NAN_BITS = 0x7FC0   # bf16 NaN: what every output buffer holds before the call


def _bits(rng, *shape, scale=1.0):
    """random bf16 values of about unit size, as their bit patterns"""
    v = (rng.standard_normal(shape) * scale).astype(np.float32)
    return (v.view(np.uint32) >> 16).astype(np.uint16)


def _f32(rng, *shape):
    return rng.standard_normal(shape).astype(np.float32)


def _sentinel(rows, cols):
    return emu.Buf(np.full((rows, cols), NAN_BITS, np.uint16))


def _values(bits):
    return (bits.astype(np.uint32) << 16).view(np.float32)


def _fuse(rng, M, Cn, z=False, mask_from_z=False, relu_bits=False, seg=0):
    """lp_bn_fuse for a launch whose output has M rows of Cn channels (buffers kept alive on the object)"""
    f = _lib.BnFuse()
    f.seg_images = seg
    nseg = 2 if seg else 1
    keep = {"sums": emu.ZX((nseg, 2, Cn))}
    f.sums = keep["sums"].p.value
    if z:
        keep.update(z=emu.Buf(_bits(rng, M, Cn)), mean=emu.Buf(_f32(rng, nseg, Cn) * 0.1),
                    invstd=emu.Buf(np.abs(_f32(rng, nseg, Cn)) + 0.5), gamma=emu.Buf(np.abs(_f32(rng, Cn)) + 0.5), beta=emu.Buf(_f32(rng, Cn) * 0.3))
        f.z, f.mean, f.invstd, f.gamma, f.beta = (keep[n].p.value for n in ("z", "mean", "invstd", "gamma", "beta"))
    f.mask_from_z = int(mask_from_z)
    if relu_bits:
        keep["bits"] = emu.Buf(rng.integers(0, 256, M * Cn // 8, dtype=np.uint8) | np.uint8(1))
        f.relu_bits = keep["bits"].p.value
    f.keep = keep
    return f


# ---- the entry points: each returns (return code, the output's bf16 bits restricted to the columns the call may write) ----
def fwd(rng, geom, bias=False, f32_out=False, ldo=None, bn_seg=None):
    """lp_conv_fwd, or lp_conv_fwd_bn with ``bn_seg`` (0 = one BatchNorm segment)"""
    g = emu.geom(*geom)
    M, ldo = g.B * g.Ho * g.Wo, ldo or g.Co
    x, w = emu.Buf(_bits(rng, g.B, g.Hi, g.Wi, g.Ci)), emu.Buf(_bits(rng, g.Co, g.R, g.S, g.Ci, scale=(g.R * g.S * g.Ci) ** -0.5))
    b, out = (emu.Buf(_f32(rng, g.Co)) if bias else None), _sentinel(M, ldo)
    if bn_seg is not None:
        f = _fuse(rng, M, g.Co, seg=bn_seg)
        rc = emu.lib().lp_conv_fwd_bn(x.p, w.p, C.byref(g), out.p, C.byref(f), emu.stream())
        return rc, out.np()
    of = emu.Buf(np.full((M, ldo), np.nan, np.float32)) if f32_out else None
    rc = emu.lib().lp_conv_fwd(x.p, w.p, C.byref(g), emu.ptr(b), None if f32_out else out.p, emu.ptr(of), ldo, 0, emu.stream())
    if f32_out:
        return rc, (of.np()[:, :g.Co].view(np.uint32) >> 16).astype(np.uint16)
    return rc, out.np()[:, :g.Co]


def fwd_act(rng, geom, residual=False):
    g = emu.geom(*geom)
    M = g.B * g.Ho * g.Wo
    x, w = emu.Buf(_bits(rng, g.B, g.Hi, g.Wi, g.Ci)), emu.Buf(_bits(rng, g.Co, g.R, g.S, g.Ci, scale=(g.R * g.S * g.Ci) ** -0.5))
    b, r, out = emu.Buf(_f32(rng, g.Co)), (emu.Buf(_bits(rng, M, g.Co)) if residual else None), _sentinel(M, g.Co)
    rc = emu.lib().lp_conv_fwd_act(x.p, w.p, C.byref(g), b.p, emu.ptr(r), 1, out.p, emu.stream())
    return rc, out.np()


def dgrad(rng, geom, form="plain", seg=0):
    """the data gradient of the convolution ``geom`` (dy has Co channels, dx has Ci).  form: plain | bias (lp_conv_dgrad), bits
    (lp_conv_dgrad_bits: kEkPB), z (lp_conv_dgrad_bn, mask recomputed from z: kEkZ), azb (addend + relu_bits: kEkAZB), zmask (the bf16
    activation as mask: no pipelined store pass)"""
    g = emu.geom(*geom)
    M, Cn = g.B * g.Hi * g.Wi, g.Ci
    dy, wd = emu.Buf(_bits(rng, g.B, g.Ho, g.Wo, g.Co)), emu.Buf(_bits(rng, g.Ci, g.R, g.S, g.Co, scale=(g.R * g.S * g.Co) ** -0.5))
    dx, lib, st = _sentinel(M, Cn), emu.lib(), emu.stream()
    if form in ("plain", "bias"):
        b = emu.Buf(_f32(rng, Cn)) if form == "bias" else None
        return lib.lp_conv_dgrad(dy.p, wd.p, C.byref(g), emu.ptr(b), None, None, dx.p, None, Cn, 0, 0, st), dx.np()
    if form == "bits":
        bits = emu.Buf(rng.integers(0, 256, M * Cn // 8, dtype=np.uint8) | np.uint8(1))
        return lib.lp_conv_dgrad_bits(dy.p, wd.p, C.byref(g), None, bits.p, dx.p, 0, st), dx.np()
    f = _fuse(rng, M, Cn, z=True, mask_from_z=form == "z", relu_bits=form == "azb", seg=seg)
    add = emu.Buf(_bits(rng, M, Cn)) if form == "azb" else None
    mask = emu.Buf(_bits(rng, M, Cn)) if form == "zmask" else None
    return lib.lp_conv_dgrad_bn(dy.p, wd.p, C.byref(g), emu.ptr(add), emu.ptr(mask), dx.p, C.byref(f), st), dx.np()


def gemm(rng, M, N, K, lda=None, batch=1, gelu=None):
    """lp_gemm_nt (``batch`` independent products, A rows of pitch ``lda``), or its GELU forms: gelu = "fwd" | "bwd" """
    lda = lda or K
    a, b = emu.Buf(_bits(rng, batch * M * lda)), emu.Buf(_bits(rng, batch * N * K, scale=K ** -0.5))
    c, lib, st = _sentinel(batch * M, N), emu.lib(), emu.stream()
    if gelu == "fwd":
        bias, act = emu.Buf(_f32(rng, N)), _sentinel(M, N)
        rc = lib.lp_gemm_nt_gelu_fwd(a.p, b.p, bias.p, c.p, act.p, M, N, K, st)
        return rc, np.concatenate([c.np(), act.np()])
    if gelu == "bwd":
        u, sums = emu.Buf(_bits(rng, M, N)), emu.ZX((2, N))
        return lib.lp_gemm_nt_gelu_bwd(a.p, b.p, u.p, c.p, M, N, K, sums.p, st), c.np()
    gb = _lib.GemmBatch(batch, 1, M * lda, 0, N * K, 0, M * N, 0) if batch > 1 else None
    return lib.lp_gemm_nt(a.p, lda, b.p, K, c.p, None, N, M, N, K, 0, None, C.byref(gb) if gb else None, st), c.np()


def stem(rng, B, Ho, Wo):
    g = emu.geom(B, 2 * Ho, 2 * Wo, 4, 64, 7, 7, 2, 3)
    x4 = _bits(rng, B, 2 * Ho, 2 * Wo, 4)
    x4[..., 3] = 0
    x, w, out = emu.Buf(x4), emu.Buf(_bits(rng, 64, 256, scale=147 ** -0.5)), _sentinel(B * Ho * Wo, 64)
    return emu.lib().lp_stem_fwd(x.p, w.p, C.byref(g), out.p, emu.stream()), out.np()


# geometries: (B, Hi, Wi, Ci, Co, R, S, stride, pad)
L1 = (1, 16, 16, 64, 64, 3, 3, 1, 1)        # layer1's 3x3 at one 16 x 16 tile: conv_res2d_kernel's shape
L1_H8 = (1, 8, 16, 64, 64, 3, 3, 1, 1)      # ... H no multiple of 16
L2 = (1, 16, 16, 64, 128, 3, 3, 1, 1)       # 128 output channels: the HALO form's 384-row cap
# a wide, short image: the first 256-pixel tile's neighbourhood is 262 + 2 * (255 // W) + 2 * W padded rows - 384 at W = 57, 386 at W = 58
WIDE57_128, WIDE58_128, WIDE58_64 = (1, 8, 57, 64, 128, 3, 3, 1, 1), (1, 8, 58, 64, 128, 3, 3, 1, 1), (1, 8, 58, 64, 64, 3, 3, 1, 1)
P64 = (1, 16, 16, 64, 64, 1, 1, 1, 0)       # a 1x1 layer, M = 256
D1 = (1, 16, 16, 64, 128, 1, 1, 1, 0)       # data gradient 128 -> 64 channels
S3 = (2, 18, 18, 64, 256, 3, 3, 2, 1)       # 3x3 stride 2: four parity classes
S1 = (5, 8, 8, 128, 128, 1, 1, 2, 0)        # 1x1 stride 2: the class the tap reaches, then three empty ones
# stride 2, 15 x 15, BatchNorm segments of 16 + 1 images: the classes have 64, 56, 56, 49 pixels per image - 16 * 49 rows is off the 128-row grid
S1_SEG = (17, 15, 15, 64, 64, 1, 1, 2, 0)

ROWS = [
    # id, entry point, arguments, switches, expected kernel (None: the call is refused), expected return code
    ("fwd-l1", fwd, dict(geom=L1), {}, RES2D, OK),
    ("fwd-l1-res2d0", fwd, dict(geom=L1), {"LP_CONV_RES2D": "0"}, HALO, OK),
    ("fwd-l1-res2d0-halo0", fwd, dict(geom=L1), {"LP_CONV_RES2D": "0", "LP_CONV_HALO": "0"}, PIPE, OK),
    ("fwd-l1-halo0", fwd, dict(geom=L1), {"LP_CONV_HALO": "0"}, RES2D, OK),
    ("fwd-l1-pipe0", fwd, dict(geom=L1), {"LP_CONV_PIPE": "0"}, IGEMM, OK),
    ("fwd-l1-bias", fwd, dict(geom=L1, bias=True), {}, HALO, OK),
    ("fwd-l1-h8", fwd, dict(geom=L1_H8), {}, HALO, OK),
    ("fwd-l2", fwd, dict(geom=L2), {}, HALO, OK),
    ("fwd-l2-halo0", fwd, dict(geom=L2), {"LP_CONV_HALO": "0"}, PIPE, OK),
    ("fwd-wide57-128", fwd, dict(geom=WIDE57_128), {}, HALO, OK),
    ("fwd-wide58-128", fwd, dict(geom=WIDE58_128), {}, PIPE, OK),
    ("fwd-wide58-64", fwd, dict(geom=WIDE58_64), {}, HALO, OK),
    ("fwd-co72", fwd, dict(geom=(1, 16, 16, 64, 72, 3, 3, 1, 1)), {}, IGEMM, OK),
    ("fwd-f32", fwd, dict(geom=L1, f32_out=True), {}, IGEMM, OK),
    ("fwd-ldo", fwd, dict(geom=L1, ldo=72), {}, IGEMM, OK),
    ("fwd-bn", fwd, dict(geom=L1, bn_seg=0), {}, RES2D, OK),
    ("fwd-bn-seg256", fwd, dict(geom=(2, 16, 16, 64, 64, 1, 1, 1, 0), bn_seg=1), {}, PIPE, OK),
    ("fwd-bn-seg128", fwd, dict(geom=(2, 8, 16, 64, 64, 1, 1, 1, 0), bn_seg=1), {}, IGEMM, OK),
    ("fwd-bn-seg64", fwd, dict(geom=(2, 8, 8, 64, 64, 1, 1, 1, 0), bn_seg=1), {}, None, UNSUPPORTED),
    ("act-l1", fwd_act, dict(geom=L1), {}, RES2D, OK),
    ("act-l1-residual", fwd_act, dict(geom=L1, residual=True), {}, HALO, OK),
    ("act-l1-infer0", fwd_act, dict(geom=L1), {"LP_INFER_PIPE": "0"}, IGEMM, OK),
    ("act-l1-pipe0", fwd_act, dict(geom=L1), {"LP_CONV_PIPE": "0"}, IGEMM, OK),
    ("act-l1-res2d0", fwd_act, dict(geom=L1), {"LP_CONV_RES2D": "0"}, HALO, OK),
    ("act-l2-residual", fwd_act, dict(geom=L2, residual=True), {}, HALO, OK),
    ("dgrad-plain", dgrad, dict(geom=D1), {}, PIPE, OK),
    ("dgrad-bits", dgrad, dict(geom=D1, form="bits"), {}, PIPE, OK),
    ("dgrad-z", dgrad, dict(geom=D1, form="z"), {}, PIPE, OK),
    ("dgrad-azb", dgrad, dict(geom=D1, form="azb"), {}, PIPE, OK),
    ("dgrad-zmask", dgrad, dict(geom=D1, form="zmask"), {}, IGEMM, OK),
    ("dgrad-bias", dgrad, dict(geom=D1, form="bias"), {}, IGEMM, OK),
    ("dgrad-pipe0", dgrad, dict(geom=D1), {"LP_CONV_PIPE": "0"}, IGEMM, OK),
    ("dgrad-z-l1", dgrad, dict(geom=L1, form="z"), {}, RES2D, OK),
    ("dgrad-z-l1-res2d0", dgrad, dict(geom=L1, form="z"), {"LP_CONV_RES2D": "0"}, HALO, OK),
    ("dgrad-plain-l1", dgrad, dict(geom=L1), {}, PIPE, OK),
    ("dgrad-s2-3x3", dgrad, dict(geom=S3), {}, PIPE, OK),
    ("dgrad-s2-1x1", dgrad, dict(geom=S1), {}, IGEMM, OK),
    ("dgrad-s2-1x1-z", dgrad, dict(geom=S1, form="z"), {}, IGEMM, OK),
    ("dgrad-s2-seg-last-class-off-grid", dgrad, dict(geom=S1_SEG, form="z", seg=16), {}, None, UNSUPPORTED),
    ("gemm-dense", gemm, dict(M=256, N=128, K=64), {}, PIPE, OK),
    ("gemm-lda", gemm, dict(M=256, N=128, K=64, lda=72), {}, IGEMM, OK),
    ("gemm-batch2", gemm, dict(M=256, N=128, K=64, batch=2), {}, IGEMM, OK),
    ("gemm-gemm-pipe0", gemm, dict(M=256, N=128, K=64), {"LP_GEMM_PIPE": "0"}, IGEMM, OK),
    ("gemm-pipe0", gemm, dict(M=256, N=128, K=64), {"LP_CONV_PIPE": "0"}, IGEMM, OK),
    ("gelu-fwd", gemm, dict(M=256, N=128, K=64, gelu="fwd"), {}, PIPE, OK),
    ("gelu-bwd", gemm, dict(M=256, N=128, K=64, gelu="bwd"), {}, PIPE, OK),
    ("gelu-fwd-n64", gemm, dict(M=256, N=64, K=64, gelu="fwd"), {}, None, UNSUPPORTED),
    ("gelu-bwd-n64", gemm, dict(M=256, N=64, K=64, gelu="bwd"), {}, None, UNSUPPORTED),
    ("gelu-fwd-gemm-pipe0", gemm, dict(M=256, N=128, K=64, gelu="fwd"), {"LP_GEMM_PIPE": "0"}, PIPE, OK),
    ("gelu-fwd-pipe0", gemm, dict(M=256, N=128, K=64, gelu="fwd"), {"LP_CONV_PIPE": "0"}, None, UNSUPPORTED),
    ("stem", stem, dict(B=1, Ho=32, Wo=32), {}, RES2D, OK),
    ("stem-2d0", stem, dict(B=1, Ho=32, Wo=32), {"LP_STEM_2D": "0"}, IGEMM, OK),
    ("stem-pipe0", stem, dict(B=1, Ho=32, Wo=32), {"LP_CONV_PIPE": "0"}, IGEMM, OK),
    ("stem-h24", stem, dict(B=1, Ho=24, Wo=32), {}, IGEMM, OK),
]


def run_row(entry, kwargs, seed=0):
    """-> (return code, lp_conv_last_kernel() after the call, the output bits).  A 1x1 weight gradient runs first, so that the id a refused
    call must leave alone is one no forward or data-gradient launch reports."""
    rng = np.random.default_rng(seed)
    emu.conv_wgrad(_bits(rng, 1, 8, 8, 64), _bits(rng, 1, 8, 8, 64), emu.geom(1, 8, 8, 64, 64, 1, 1, 1, 0))
    rc, out = entry(rng, **kwargs)
    return rc, emu.lib().lp_conv_last_kernel(), out


@pytest.mark.parametrize("entry,kwargs,env,kernel,rc", [pytest.param(*r[1:], id=r[0]) for r in ROWS])
def test_the_route_is_the_recorded_one(entry, kwargs, env, kernel, rc, monkeypatch):
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    before = (IGEMM, PIPE, HALO, RES2D)
    got_rc, got_kernel, out = run_row(entry, kwargs)
    assert got_rc == rc
    if kernel is None:   # refused: nothing was enqueued, the last-kernel id is still the weight gradient's
        assert got_kernel not in before
        assert np.all(out == NAN_BITS)
        return
    assert got_kernel == kernel
    v = _values(out)
    assert np.all(np.isfinite(v)) and np.abs(v).max() > 0
