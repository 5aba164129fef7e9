"""Token assembly of the multi-view transformer tracker (lp_vit_mv_tokens_fwd / _bwd and their fp32 twins, csrc/vit_mv.h).

forward   x[b][v Np + p] = (patch[(b V + v) Np + p] + pos[1 + p]) + view[v]   - bit for bit against numpy float32 in that order
backward  dpatch = dx (rounded to nearest even bf16 in the product path), dpos[1 + p] = sum_{b,v} dx, dview[v] = sum_{b,p} dx: the sums
          against float64, each entry within n 2^-24 sum|terms| (n terms; the bound of ANY summation order), and the same bits in two calls.
"""

import ctypes as C

import numpy as np
import pytest

from tests.hipemu import emu

# (B, V, Np, D): the smallest; nothing a multiple of a wave; D / 8 = 48 is no power of two; several workgroups per reduced column
SHAPES = [(1, 2, 4, 64), (3, 3, 9, 128), (2, 4, 36, 384), (5, 4, 256, 384)]
PRECISIONS = ["bf16", "fp32"]


def _bf16_bits(a: np.ndarray) -> np.ndarray:
    """float32 -> bf16 bit patterns, round to nearest even (finite inputs)"""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def _bits_f32(b: np.ndarray) -> np.ndarray:
    return (b.astype(np.uint32) << 16).view(np.float32)


def _fwd(precision, patch, pos, view, B, V, Np, D):
    x = emu.Z((B * V * Np, D))
    patch, pos, view = emu.B(patch), emu.B(pos), emu.B(view)   # (named: a staged buffer lives as long as its Buf, so through the call)
    name = "lp_vit_mv_tokens_fwd" if precision == "bf16" else "lp_f32_vit_mv_tokens_fwd"
    emu.ok(getattr(emu.lib(), name)(patch.p, pos.p, view.p, B, V, Np, D, x.p, emu.stream()))
    return x.np()


def _bwd(precision, dx, B, V, Np, D):
    lib = emu.lib()
    nws = int(lib.lp_vit_mv_tokens_bwd_workspace_bytes(B, V, Np, D))
    assert nws > 0 and nws % 4 == 0
    ws = emu.B(np.full(nws // 4, np.nan, np.float32))   # (its contents are undefined on entry: nothing may be read before it is written)
    dpatch = emu.Z((B * V * Np, D), np.uint16 if precision == "bf16" else np.float32)
    dpos, dview = emu.B(np.full((Np + 1, D), np.nan, np.float32)), emu.B(np.full((V, D), np.nan, np.float32))
    dx = emu.B(dx)
    name = "lp_vit_mv_tokens_bwd" if precision == "bf16" else "lp_f32_vit_mv_tokens_bwd"
    emu.ok(getattr(lib, name)(dx.p, B, V, Np, D, dpatch.p, dpos.p, dview.p, ws.p, nws, emu.stream()))
    return dpatch.np().copy(), dpos.np().copy(), dview.np().copy()


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_forward_bit_exact_in_the_documented_order(kernel_backend, shape, precision):
    B, V, Np, D = shape
    rng = np.random.default_rng(1)
    patch = rng.standard_normal((B * V * Np, D)).astype(np.float32)
    pos = rng.standard_normal((Np + 1, D)).astype(np.float32)
    view = (0.02 * rng.standard_normal((V, D))).astype(np.float32)
    if precision == "bf16":
        bits = _bf16_bits(patch)
        patch, arg = _bits_f32(bits), bits
    else:
        arg = patch
    got = _fwd(precision, arg, pos, view, B, V, Np, D)
    p4 = patch.reshape(B, V, Np, D)
    want = (p4 + pos[None, None, 1:, :]) + view[None, :, None, :]      # float32 throughout, the two additions in the header's order
    assert want.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), want.reshape(B * V * Np, D).view(np.uint32))
    # ... and the order matters at this precision: the other association differs somewhere (so the check above can fail)
    other = p4 + (pos[None, None, 1:, :] + view[None, :, None, :])
    if B * V * Np * D >= 4096:
        assert not np.array_equal(other, want)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_backward_cast_sums_and_repeatability(kernel_backend, shape, precision):
    B, V, Np, D = shape
    rng = np.random.default_rng(2)
    # terms of mixed magnitude and sign, so that a sum's rounding depends on its order
    dx = (rng.standard_normal((B * V * Np, D)) * np.exp(3 * rng.standard_normal((B * V * Np, 1)))).astype(np.float32)
    dpatch, dpos, dview = _bwd(precision, dx, B, V, Np, D)
    if precision == "bf16":
        assert np.array_equal(dpatch, _bf16_bits(dx))
    else:
        assert np.array_equal(dpatch.view(np.uint32), dx.view(np.uint32))
    d4 = dx.reshape(B, V, Np, D).astype(np.float64)
    assert np.array_equal(dpos[0], np.zeros(D, np.float32))             # the [CLS] position takes no gradient
    want_pos, mag_pos, n_pos = d4.sum((0, 1)), np.abs(d4).sum((0, 1)), B * V
    want_view, mag_view, n_view = d4.sum((0, 2)), np.abs(d4).sum((0, 2)), B * Np
    err_pos, err_view = np.abs(dpos[1:] - want_pos), np.abs(dview - want_view)
    bound_pos, bound_view = n_pos * 2.0 ** -24 * mag_pos, n_view * 2.0 ** -24 * mag_view
    print(f"dpos max err/bound {np.max(err_pos / bound_pos):.3g}, dview max err/bound {np.max(err_view / bound_view):.3g}")
    assert np.all(err_pos <= bound_pos)
    assert np.all(err_view <= bound_view)
    again = _bwd(precision, dx, B, V, Np, D)
    for a, b in zip((dpatch, dpos, dview), again):
        assert np.array_equal(a.view(np.uint32 if a.dtype == np.float32 else np.uint16), b.view(np.uint32 if b.dtype == np.float32 else np.uint16))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_bad_arguments_return_the_documented_codes(kernel_backend, precision):
    lib = emu.lib()
    fwd = getattr(lib, "lp_vit_mv_tokens_fwd" if precision == "bf16" else "lp_f32_vit_mv_tokens_fwd")
    bwd = getattr(lib, "lp_vit_mv_tokens_bwd" if precision == "bf16" else "lp_f32_vit_mv_tokens_bwd")
    B, V, Np, D = 1, 2, 4, 64
    pdt = np.uint16 if precision == "bf16" else np.float32
    patch, pos, view, x = emu.Z((B * V * Np, 96), pdt), emu.Z((Np + 1, 96)), emu.Z((V, 96)), emu.Z((B * V * Np, 96))
    dpos, dview, ws = emu.Z((Np + 1, 96)), emu.Z((V, 96)), emu.Z(1 << 14)
    nws = int(lib.lp_vit_mv_tokens_bwd_workspace_bytes(B, V, Np, D))
    ARG, UNSUPPORTED = -1, -2     # LP_ERR_ARGUMENT, LP_ERR_UNSUPPORTED (include/lp_hip.h)
    st = emu.stream()
    # D not a multiple of 64: nothing is launched
    for d in (96, 32, 8):
        assert fwd(patch.p, pos.p, view.p, B, V, Np, d, x.p, st) == UNSUPPORTED
        assert bwd(x.p, B, V, Np, d, patch.p, dpos.p, dview.p, ws.p, 1 << 16, st) == UNSUPPORTED
        assert int(lib.lp_vit_mv_tokens_bwd_workspace_bytes(B, V, Np, d)) == 0
    # null pointers, non-positive dimensions, a workspace that is too small
    for args in ((None, pos.p, view.p), (patch.p, None, view.p), (patch.p, pos.p, None)):
        assert fwd(*args, B, V, Np, D, x.p, st) == ARG
    assert fwd(patch.p, pos.p, view.p, B, V, Np, D, None, st) == ARG
    for dims in ((0, V, Np, D), (B, 0, Np, D), (B, V, 0, D), (B, V, Np, 0), (B, -1, Np, D)):
        assert fwd(patch.p, pos.p, view.p, *dims, x.p, st) == ARG
        assert bwd(x.p, *dims, patch.p, dpos.p, dview.p, ws.p, 1 << 16, st) == ARG
    for i in range(5):
        args = [x.p, patch.p, dpos.p, dview.p, ws.p]
        args[i] = None
        assert bwd(args[0], B, V, Np, D, args[1], args[2], args[3], args[4], 1 << 16, st) == ARG
    assert bwd(x.p, B, V, Np, D, patch.p, dpos.p, dview.p, ws.p, C.c_size_t(nws - 4), st) == ARG
    assert bwd(x.p, B, V, Np, D, patch.p, dpos.p, dview.p, ws.p, C.c_size_t(nws), st) == 0
