"""conv_wgrad_nb_kernel (csrc/conv_wgrad_nb.h): the weight gradient of a 3x3 / stride 1 / pad 1 layer from operands staged once for all
nine filter taps - a circular window of the input in a padded raster with shared borders, 64 consecutive raster positions per K step.
Against torch's weight gradient of the same bf16-rounded operands and against conv_wgrad_kernel, on the emulator and (-m gpu) on the
device through the same C ABI call.  Shapes are the smallest at which the kernel can still go wrong."""

import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from lightning_pose_amd import _lib
from tests.hipemu import emu

pytestmark = pytest.mark.usefixtures("kernel_backend")

KERNEL_WGRAD, KERNEL_WGRAD_PIPE, KERNEL_WGRAD_NB = _lib.CONV_KERNEL_WGRAD, _lib.CONV_KERNEL_WGRAD_PIPE, _lib.CONV_KERNEL_WGRAD_NB

CASES = [
    # B, H, W, Ci, Co
    (3, 16, 16, 64, 128),     # 576 columns, the layer1 form; a slice boundary inside an image
    (1, 19, 15, 128, 64),     # odd width, M = 285 with a ragged last K step, two ci blocks, the 64-wide co block (two K halves)
    (2, 12, 12, 128, 128),    # 144-pixel images: a K step crosses images
    (2, 7, 9, 64, 256),       # images smaller than a K step, two co blocks, all four borders inside one K step
    (1, 24, 24, 256, 256),    # layer3's channel count at one image
]

_REF = {}


def _operands(case):
    """(x bits, dy bits, torch's weight gradient [Co][9 Ci], conv_wgrad_kernel's) of a case: computed once, shared by the splits and backends"""
    if case not in _REF:
        B, H, W, Ci, Co = case
        gen = torch.Generator().manual_seed(7 + sum(case))
        bf = lambda t: t.to(torch.bfloat16).float()  # noqa: E731
        x = bf(torch.randn(B, Ci, H, W, generator=gen))
        w = bf(torch.randn(Co, Ci, 3, 3, generator=gen) / (Ci * 9) ** 0.5).requires_grad_(True)
        y = F.conv2d(x, w, stride=1, padding=1)
        dy = bf(torch.randn(y.shape, generator=gen))
        y.backward(dy)
        xb, dyb = emu.to_bf16_bits(x.permute(0, 2, 3, 1).contiguous()), emu.to_bf16_bits(dy.permute(0, 2, 3, 1).contiguous())
        _REF[case] = (xb, dyb, w.grad.permute(0, 2, 3, 1).reshape(Co, -1).clone())
    return _REF[case]


@pytest.mark.parametrize("split", [0, 1, 3])
@pytest.mark.parametrize("case", CASES)
def test_neighbourhood_weight_gradient(case, split, monkeypatch):
    B, H, W, Ci, Co = case
    xb, dyb, want = _operands(case)
    g = emu.geom(B, H, W, Ci, Co, 3, 3, 1, 1)
    new = emu.conv_wgrad(xb, dyb, g, split=split)
    assert emu.lib().lp_conv_last_kernel() == KERNEL_WGRAD_NB      # under defaults
    again = emu.conv_wgrad(xb, dyb, g, split=split)
    assert np.array_equal(new, again)                              # a call repeats bit for bit
    torch.testing.assert_close(torch.from_numpy(new), want, atol=2e-3, rtol=2e-3)
    monkeypatch.setenv("LP_WGRAD_PIPE", "0")
    old = emu.conv_wgrad(xb, dyb, g, split=split)
    assert emu.lib().lp_conv_last_kernel() == KERNEL_WGRAD
    torch.testing.assert_close(torch.from_numpy(new), torch.from_numpy(old), atol=1e-3, rtol=1e-3)


@pytest.mark.parametrize("case", CASES)
def test_switch_brings_the_previous_kernel_back(case, monkeypatch):
    B, H, W, Ci, Co = case
    xb, dyb, _ = _operands(case)
    g = emu.geom(B, H, W, Ci, Co, 3, 3, 1, 1)
    emu.conv_wgrad(xb, dyb, g)
    before = emu.lib().lp_conv_last_kernel()
    assert before == KERNEL_WGRAD_NB
    monkeypatch.setenv("LP_WGRAD_NB", "0")
    off = emu.conv_wgrad(xb, dyb, g)
    prev = emu.lib().lp_conv_last_kernel()
    assert prev in (KERNEL_WGRAD, KERNEL_WGRAD_PIPE)
    monkeypatch.setenv("LP_WGRAD_PIPE", "2")     # the A/B arms keep their meaning whatever LP_WGRAD_NB says
    monkeypatch.setenv("LP_WGRAD_NB", "1")
    emu.conv_wgrad(xb, dyb, g)
    assert emu.lib().lp_conv_last_kernel() == (KERNEL_WGRAD if B * H * W < 256 else KERNEL_WGRAD_PIPE)   # (the pipelined kernel wants four K steps)
    monkeypatch.delenv("LP_WGRAD_PIPE")
    on = emu.conv_wgrad(xb, dyb, g)
    assert emu.lib().lp_conv_last_kernel() == KERNEL_WGRAD_NB
    torch.testing.assert_close(torch.from_numpy(on), torch.from_numpy(off), atol=1e-3, rtol=1e-3)


@pytest.mark.parametrize("B,H,W,Ci,Co,R,stride,pad", [
    (2, 18, 18, 64, 128, 3, 2, 1),    # 3x3 stride 2
    (2, 16, 16, 128, 128, 1, 1, 0),   # 1x1
    (1, 16, 16, 64, 72, 3, 1, 1),     # 3x3 "same", but Co is no multiple of 64
])
def test_other_shapes_are_not_routed_to_it(B, H, W, Ci, Co, R, stride, pad):
    gen = torch.Generator().manual_seed(B + H + Ci + Co)
    g = emu.geom(B, H, W, Ci, Co, R, R, stride, pad)
    xb = emu.to_bf16_bits(torch.randn(B, H, W, Ci, generator=gen))
    dyb = emu.to_bf16_bits(torch.randn(B, g.Ho, g.Wo, Co, generator=gen))
    dw = emu.conv_wgrad(xb, dyb, g)
    assert emu.lib().lp_conv_last_kernel() in (KERNEL_WGRAD, KERNEL_WGRAD_PIPE)
    assert np.isfinite(dw).all() and np.abs(dw).max() > 0


@pytest.mark.parametrize("switch", [None, ("LP_WGRAD_NB", "0"), ("LP_WGRAD_PIPE", "0"), ("LP_WGRAD_PIPE", "2")])
@pytest.mark.parametrize("stem", [False, True])
def test_the_routed_plans_workspace_is_required(stem, switch, monkeypatch):
    """A workspace smaller than the plan of the kernel the launch is routed to is LP_ERR_ARGUMENT before anything is launched - never a
    quiet move to a slower kernel: dw and lp_conv_last_kernel() stay as they were.  256 bytes are below every kernel's smallest plan (one
    slice of one 64-wide tile is 32 KB); exactly lp_conv_wgrad_workspace_bytes() succeeds under every switch setting."""
    if switch:
        monkeypatch.setenv(*switch)
    g = emu.geom(1, 128, 128, 4, 64, 7, 7, 2, 3) if stem else emu.geom(1, 16, 16, 64, 64, 3, 3, 1, 1)
    call = emu.lib().lp_stem_wgrad if stem else emu.lib().lp_conv_wgrad
    gen = torch.Generator().manual_seed(5)
    xb = emu.Buf(emu.to_bf16_bits(torch.randn(g.B, g.Hi, g.Wi, g.Ci, generator=gen)))
    db = emu.Buf(emu.to_bf16_bits(torch.randn(g.B, g.Ho, g.Wo, g.Co, generator=gen)))
    nws = emu.lib().lp_conv_wgrad_workspace_bytes(C.byref(g), 0)
    assert nws > 256
    ws = emu.Z(nws, np.uint8)
    # a forward call first: its kernel id (conv_igemm_kernel / conv_pipe_kernel) is none of the weight-gradient ids
    emu.conv_fwd(emu.to_bf16_bits(torch.randn(1, 4, 4, 64, generator=gen)), emu.to_bf16_bits(torch.randn(64, 64, generator=gen)),
                 emu.geom(1, 4, 4, 64, 64, 1, 1, 1, 0))
    before = emu.lib().lp_conv_last_kernel()
    assert before in (_lib.CONV_KERNEL_IGEMM, _lib.CONV_KERNEL_PIPE)
    sentinel = np.full((64, 256) if stem else (g.Co, 9 * g.Ci), -7.5, np.float32)
    dw = emu.Buf(sentinel)
    assert call(xb.p, db.p, C.byref(g), dw.p, 0, ws.p, 256, emu.stream()) == -1   # LP_ERR_ARGUMENT
    assert np.array_equal(dw.np(), sentinel)
    assert emu.lib().lp_conv_last_kernel() == before
    emu.ok(call(xb.p, db.p, C.byref(g), dw.p, 0, ws.p, nws, emu.stream()))
    assert emu.lib().lp_conv_last_kernel() not in (_lib.CONV_KERNEL_IGEMM, _lib.CONV_KERNEL_PIPE)
    assert np.isfinite(dw.np()).all() and not np.array_equal(dw.np(), sentinel)
