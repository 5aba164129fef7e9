"""The weight-resident form of conv_pipe_kernel (csrc/conv_pipe.h: WRES - 1x1 / stride 1 / pad 0 with K * BN * 2 <= 64 KB, the BN x K weight
panel kept in LDS for the workgroup's whole walk, the ring's stages holding pixels alone) against the ring form on the same call.  The K
order, every rounding point and the per-thread BatchNorm partial sums are the ring's, so EVERYTHING is compared bitwise: the result tensor
and the raw fixed-point words of the fused BatchNorm sums, forward and backward.  LP_PIPE_WRES=0 keeps the ring, =2 takes the resident form
wherever its shape rule passes (=1, the default, also asks the performance rule, which is about speed and not under test here).

Shapes: the smallest at which the form can go wrong.  800 pixel rows = three full 256-row tiles and a ragged one; K = 64 / 128 / 256 = 1 / 2 / 4
panel slices at 128 columns and K = 512 = 8 slices at 64 columns (the limits); K = 320 does not fit and must stay on the ring; N = 128 is one
column block, N = 384 three - with the grid capped at two workgroups (LP_CONV_MAX_WGS) the stride 2 is no multiple of tiles_n = 3, so a
workgroup meets another column block in the middle of its walk and reloads the panel."""

import numpy as np
import pytest
import torch

from lightning_pose_amd import _lib
from tests.hipemu import emu

pytestmark = pytest.mark.usefixtures("kernel_backend")

PIPE = _lib.CONV_KERNEL_PIPE

# K, N, takes the resident form
SHAPES = [
    (64, 128, True),      # one panel slice, one column block
    (128, 128, True),     # two slices
    (256, 128, True),     # four slices: the 64-KB limit at 128 columns
    (256, 384, True),     # three column blocks: panel reloads under the workgroup cap
    (512, 64, True),      # eight slices of 8 KB: the limit at 64 columns
    (320, 128, False),    # 80 KB: falls back to the ring
]


def _ab(monkeypatch, fn, resident):
    """the same call on the ring (LP_PIPE_WRES=0) and with the resident form allowed (=2); both are conv_pipe_kernel launches"""
    lib = emu.lib()
    monkeypatch.setenv("LP_PIPE_WRES", "0")
    ring = fn()
    assert lib.lp_conv_last_kernel() == PIPE and lib.lp_conv_last_resident() == 0
    monkeypatch.setenv("LP_PIPE_WRES", "2")
    res = fn()
    assert lib.lp_conv_last_kernel() == PIPE and lib.lp_conv_last_resident() == int(resident)
    return ring, res


def _same(a, b):
    """bitwise, over every array of a result tuple"""
    a, b = (a, b) if isinstance(a, tuple) else ((a,), (b,))
    assert len(a) == len(b)
    for u, v in zip(a, b):
        if u is None:
            assert v is None
            continue
        assert u.dtype == v.dtype and u.shape == v.shape and np.array_equal(u, v)
    out = emu.from_bf16_bits(a[0])
    assert bool(torch.isfinite(out).all()) and float(out.abs().max()) > 0   # (something was computed)


def _operands(B, H, W, K, N, seed):
    """forward: x (B, H, W, K) * w (N, K) -> z (M, N); data gradient: dy (M, K) * wd (N, K) -> dx (M, N), i.e. a convolution with Ci = N, Co = K"""
    gen = torch.Generator().manual_seed(seed)
    M = B * H * W
    x = emu.to_bf16_bits(torch.randn(B, H, W, K, generator=gen))
    w = emu.to_bf16_bits(torch.randn(N, 1, 1, K, generator=gen) / K ** 0.5)
    zin = emu.to_bf16_bits(torch.randn(M, N, generator=gen))
    add = emu.to_bf16_bits(torch.randn(M, N, generator=gen))
    gamma, beta = (torch.rand(N, generator=gen) + 0.5).numpy(), (torch.randn(N, generator=gen) * 0.3).numpy()
    bits = np.random.default_rng(seed).integers(0, 256, M * N // 8, dtype=np.uint8)
    return x, w, zin, add, gamma, beta, bits


@pytest.mark.parametrize("wgs", ["0", "2"])
@pytest.mark.parametrize("K,N,resident", SHAPES)
def test_resident_form_equals_the_ring_bit_for_bit(K, N, resident, wgs, monkeypatch):
    if wgs != "0":
        monkeypatch.setenv("LP_CONV_MAX_WGS", wgs)
    B, H, W = 2, 20, 20
    M = B * H * W
    x, w, zin, add, gamma, beta, bits = _operands(B, H, W, K, N, 7 + K + N)
    gf, gd = emu.geom(B, H, W, K, N, 1, 1, 1, 0), emu.geom(B, H, W, N, K, 1, 1, 1, 0)
    # forward with the fused BatchNorm sums (raw fixed-point words), and plain
    _same(*_ab(monkeypatch, lambda: emu.conv_fwd_bn(x, w, gf, raw=True), resident))
    _same(*_ab(monkeypatch, lambda: emu.conv_fwd(x, w, gf)[0], resident))
    # the four training data gradients: BatchNorm-backward sums with the mask recomputed from z (kEkZ) and with mask bits + addend (kEkAZB);
    # lp_conv_dgrad with an addend (kEkPlain); lp_conv_dgrad_bits (kEkPB)
    mean = (torch.randn(N, generator=torch.Generator().manual_seed(K)) * 0.1).numpy()
    invstd = (torch.rand(N, generator=torch.Generator().manual_seed(N)) + 0.5).numpy()
    _same(*_ab(monkeypatch, lambda: emu.conv_dgrad_bn(x, w, gd, zin, mean, invstd, gamma, beta, raw=True)[:2], resident))
    _same(*_ab(monkeypatch, lambda: emu.conv_dgrad_bn(x, w, gd, zin, mean, invstd, addend_bits=add, relu_bits=bits, raw=True)[:2], resident))
    _same(*_ab(monkeypatch, lambda: emu.conv_dgrad(x, w, gd, addend_bits=add)[0], resident))
    _same(*_ab(monkeypatch, lambda: emu.conv_dgrad_bits(x, w, gd, bits, addend_bits=add), resident))
    assert x.shape == (B, H, W, K) and M == 800


@pytest.mark.parametrize("K,N", [(256, 128), (256, 384)])
def test_resident_form_with_a_batchnorm_segment_boundary_on_a_tile_edge(K, N, monkeypatch):
    """B = 4 of 16 x 16 with seg_images = 2: the segment changes at row 512, a tile edge - the sums are flushed there, the panel is not reloaded;
    with N = 384 under the cap of two workgroups column-block changes (panel reloads) and the segment change meet in one walk"""
    monkeypatch.setenv("LP_CONV_MAX_WGS", "2")
    B, H, W, seg = 4, 16, 16, 2
    x, w, zin, add, gamma, beta, bits = _operands(B, H, W, K, N, 3 + K + N)
    gf, gd = emu.geom(B, H, W, K, N, 1, 1, 1, 0), emu.geom(B, H, W, N, K, 1, 1, 1, 0)
    rng = np.random.default_rng(5)
    mean, invstd = (rng.normal(size=(2, N)) * 0.1).astype(np.float32), (rng.random((2, N)) + 0.5).astype(np.float32)
    ring, res = _ab(monkeypatch, lambda: emu.conv_fwd_bn(x, w, gf, seg=seg, raw=True), True)
    _same(ring, res)
    assert res[1].shape == (2, 2, N, 2) and not np.array_equal(res[1][0], res[1][1])   # two segments, each with its own sums
    _same(*_ab(monkeypatch, lambda: emu.conv_dgrad_bn(x, w, gd, zin, mean, invstd, gamma, beta, seg=seg, raw=True)[:2], True))
    _same(*_ab(monkeypatch, lambda: emu.conv_dgrad_bn(x, w, gd, zin, mean, invstd, addend_bits=add, relu_bits=bits, seg=seg, raw=True)[:2], True))


def test_only_short_k_1x1_training_launches_take_the_resident_form(monkeypatch):
    """routing: a 3x3, a stride-2, a K = 320 and an inference (lp_conv_fwd_act) problem stay off the form at LP_PIPE_WRES=1 and =2; a plain 1x1
    forward takes it at =2 (the positive control) and nothing takes it at =0"""
    lib = emu.lib()
    gen = torch.Generator().manual_seed(1)

    def fwd(B, H, W, Ci, Co, R, stride, pad, act=False):
        g = emu.geom(B, H, W, Ci, Co, R, R, stride, pad)
        x = emu.to_bf16_bits(torch.randn(B, H, W, Ci, generator=gen))
        w = emu.to_bf16_bits(torch.randn(Co, R, R, Ci, generator=gen) / (Ci * R * R) ** 0.5)
        if act:
            emu.conv_fwd_act(x, w, g, bias=np.zeros(Co, np.float32), relu=True)
        else:
            emu.conv_fwd(x, w, g)
        return lib.lp_conv_last_kernel(), lib.lp_conv_last_resident()

    for mode in ("1", "2"):
        monkeypatch.setenv("LP_PIPE_WRES", mode)
        assert fwd(1, 16, 16, 64, 128, 3, 1, 1) == (_lib.CONV_KERNEL_PIPE_HALO, 0)      # 3x3
        assert fwd(2, 16, 16, 64, 128, 1, 2, 0)[1] == 0                                  # 1x1 stride 2
        assert fwd(1, 16, 16, 320, 128, 1, 1, 0) == (PIPE, 0)                            # the panel does not fit
        assert fwd(1, 16, 16, 64, 128, 1, 1, 0, act=True) == (PIPE, 0)                   # inference keeps the ring
    assert fwd(1, 16, 16, 64, 128, 1, 1, 0) == (PIPE, 1)
    monkeypatch.setenv("LP_PIPE_WRES", "0")
    assert fwd(1, 16, 16, 64, 128, 1, 1, 0) == (PIPE, 0)
