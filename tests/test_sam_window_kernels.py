"""The kernels of the SAM backbone at kernel level (include/lp_hip.h, csrc/window.hip): window partition / un-partition in both element types,
the pad rows' column sums, the prefix-free token assembly and the final residual add.

Partition and un-partition are pure moves, so they are compared BIT FOR BIT with a numpy restatement of transformers' ``window_partition`` /
``window_unpartition`` (pad bottom / right to multiples of the window, window b * nW + wy * nWx + wx, token ty * ws + tx): random bit
patterns (NaN payloads included), -0.0, canaries in front of and behind every output, a source / destination pitch wider than the row.
The pad-row column sums are held to the float64 sum within  n_pad * 2^-24 * sum |x|  per column - the worst case of ANY fp32 summation
order - must repeat bit for bit, and ACCUMULATE into their target (the documented behaviour): one fp32 add of the sum to what was there."""

import ctypes as C

import numpy as np
import pytest

from tests.hipemu import emu

ARG, UNSUPPORTED = -1, -2     # LP_ERR_ARGUMENT, LP_ERR_UNSUPPORTED (include/lp_hip.h)
# (B, gh, gw, ws): four windows - full, ragged right, ragged bottom, corner; ViT-B's window on a 256-px grid (four ragged windows of 196
# tokens); one window that is mostly padding (180 of 196 rows); no padding at all; a single token
GEOMS = [(2, 5, 4, 3), (1, 16, 16, 14), (2, 4, 4, 14), (2, 6, 6, 3), (3, 1, 1, 2)]
COLS = [384, 2304]            # a ViT-S token row and a ViT-B fused qkv row (4608 B in bf16: 4.5 passes of a wave)
GUARD = 64                    # canary elements in front of and behind every output (keeps 16-byte alignment)
_ids = lambda s: "x".join(map(str, s))  # noqa: E731
DT = {"bf16": np.uint16, "fp32": np.uint32}      # the element as raw bits: a move must not care what they mean
NEG_ZERO = {"bf16": 0x8000, "fp32": 0x80000000}
NAN_PAYLOAD = {"bf16": 0x7FA5, "fp32": 0x7FA5C3E1}
CANARY = {"bf16": 0xBEEF, "fp32": 0xDEADBEEF}


def _index(B, gh, gw, ws):
    """window-layout row -> grid-layout row (-1: pad), as HF's pad + reshape + permute gives it"""
    nwy, nwx = -(-gh // ws), -(-gw // ws)
    grid = np.full((B, nwy * ws, nwx * ws), -1, np.int64)
    grid[:, :gh, :gw] = np.arange(B * gh * gw).reshape(B, gh, gw)
    return grid.reshape(B, nwy, ws, nwx, ws).transpose(0, 1, 3, 2, 4).reshape(-1)


def _name(precision, which):
    return ("lp_window_" if precision == "bf16" else "lp_f32_window_") + which


def _bits(rng, shape, precision):
    dt = DT[precision]
    a = rng.integers(0, np.iinfo(dt).max, size=shape, dtype=dt, endpoint=True)
    flat = a.reshape(-1)
    flat[0], flat[flat.size // 2], flat[-1] = NEG_ZERO[precision], NAN_PAYLOAD[precision], NEG_ZERO[precision]
    return a


def _staged(a):
    """Buf of raw bits (int views keep every bit pattern through the host <-> device copies)"""
    return emu.B(a.view(np.int32) if a.dtype == np.uint32 else a)


def _guarded(n, precision):
    full = np.full(n + 2 * GUARD, CANARY[precision], DT[precision])
    buf = _staged(full)
    body = C.c_void_p(buf.p.value + GUARD * full.itemsize)
    return buf, body


def _unguard(buf, n, precision):
    out = buf.np().view(DT[precision])
    assert np.all(out[:GUARD] == CANARY[precision]) and np.all(out[GUARD + n:] == CANARY[precision]), "a canary was overwritten"
    return out[GUARD:GUARD + n].copy()


def _partition(precision, src, ld, B, gh, gw, ws, cols, fill):
    idx = _index(B, gh, gw, ws)
    sbuf, fbuf = _staged(src), (_staged(fill) if fill is not None else None)
    obuf, optr = _guarded(idx.size * cols, precision)
    rc = getattr(emu.lib(), _name(precision, "partition"))(sbuf.p, ld, B, gh, gw, ws, cols, emu.ptr(fbuf), optr, emu.stream())
    return rc, _unguard(obuf, idx.size * cols, precision).reshape(idx.size, cols)


def _unpartition(precision, srcw, B, gh, gw, ws, cols, ld, colsum=None):
    sbuf = _staged(srcw)
    n = B * gh * gw * ld
    obuf, optr = _guarded(n, precision)
    cbuf = emu.B(colsum) if colsum is not None else None
    rc = getattr(emu.lib(), _name(precision, "unpartition"))(sbuf.p, B, gh, gw, ws, cols, optr, ld, emu.ptr(cbuf), emu.stream())
    return rc, _unguard(obuf, n, precision).reshape(B * gh * gw, ld), (cbuf.np().copy() if cbuf is not None else None)


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("geom", GEOMS, ids=_ids)
def test_partition_is_a_pure_move_with_both_fills(kernel_backend, geom, cols, precision):
    B, gh, gw, ws = geom
    rng = np.random.default_rng(0)
    idx = _index(B, gh, gw, ws)
    src = _bits(rng, (B * gh * gw, cols), precision)
    fill = _bits(rng, (cols,), precision)
    for f in (fill, None):
        rc, got = _partition(precision, src, cols, B, gh, gw, ws, cols, f)
        assert rc == 0
        want = np.where((idx >= 0)[:, None], src[np.maximum(idx, 0)], (f if f is not None else np.zeros(cols, src.dtype))[None, :])
        assert np.array_equal(got, want)
    assert (idx < 0).sum() == idx.size - B * gh * gw
    assert sorted(idx[idx >= 0]) == list(range(B * gh * gw))          # every real row lands in exactly one window row


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("geom", GEOMS, ids=_ids)
def test_unpartition_is_the_inverse_move(kernel_backend, geom, cols, precision):
    B, gh, gw, ws = geom
    rng = np.random.default_rng(1)
    idx = _index(B, gh, gw, ws)
    srcw = _bits(rng, (idx.size, cols), precision)
    rc, got, _ = _unpartition(precision, srcw, B, gh, gw, ws, cols, cols)
    assert rc == 0
    want = np.empty((B * gh * gw, cols), srcw.dtype)
    want[idx[idx >= 0]] = srcw[idx >= 0]
    assert np.array_equal(got, want)
    # ... and the round trip: partition(un-partition(w)) restores the real rows of w
    rc2, back = _partition(precision, got, cols, B, gh, gw, ws, cols, None)
    assert rc2 == 0 and np.array_equal(back[idx >= 0], srcw[idx >= 0]) and not back[idx < 0].any()


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_row_pitch_wider_than_the_row(kernel_backend, precision):
    """partition reads rows `ld_src` apart (the fused qkv tensor inside a wider allocation) and un-partition writes rows `ld_dst` apart,
    leaving the columns behind `cols` alone"""
    B, gh, gw, ws, cols, ld = 2, 5, 4, 3, 384, 384 + 16
    rng = np.random.default_rng(2)
    idx = _index(B, gh, gw, ws)
    src = _bits(rng, (B * gh * gw, ld), precision)
    fill = _bits(rng, (cols,), precision)
    rc, got = _partition(precision, src, ld, B, gh, gw, ws, cols, fill)
    assert rc == 0
    assert np.array_equal(got, np.where((idx >= 0)[:, None], src[np.maximum(idx, 0), :cols], fill[None, :]))
    srcw = _bits(rng, (idx.size, cols), precision)
    rc, out, _ = _unpartition(precision, srcw, B, gh, gw, ws, cols, ld)
    assert rc == 0
    want = np.full((B * gh * gw, ld), CANARY[precision], srcw.dtype)      # (the output starts as canaries)
    want[idx[idx >= 0], :cols] = srcw[idx >= 0]
    assert np.array_equal(out, want)


def _values(rng, shape, precision):
    """finite values of mixed sign and scale, as raw bits and as float64"""
    x = (rng.standard_normal(shape) * np.exp(rng.uniform(-3, 3, shape))).astype(np.float32)
    if precision == "bf16":
        bits = (x.view(np.uint32) >> 16).astype(np.uint16)
        return bits, (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    return x.view(np.uint32), x.astype(np.float64)


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("geom", GEOMS, ids=_ids)
def test_pad_row_column_sums(kernel_backend, geom, cols, precision):
    B, gh, gw, ws = geom
    rng = np.random.default_rng(3)
    idx = _index(B, gh, gw, ws)
    pad = idx < 0
    n_pad = int(pad.sum())
    bits, val = _values(rng, (idx.size, cols), precision)
    rc, moved, s0 = _unpartition(precision, bits, B, gh, gw, ws, cols, cols, colsum=np.zeros(cols, np.float32))
    assert rc == 0
    plain = _unpartition(precision, bits, B, gh, gw, ws, cols, cols)[1]
    assert np.array_equal(moved, plain)                                  # the move itself does not depend on the sums
    want = val[pad].sum(0)
    bound = n_pad * 2.0 ** -24 * np.abs(val[pad]).sum(0)
    err = np.abs(s0.astype(np.float64) - want)
    print(f"[{precision} {geom} cols {cols}] n_pad {n_pad}: max err / bound = {np.max(err / np.maximum(bound, 1e-300)) if n_pad else 0.0:.4f}")
    assert np.all(err <= bound)                                          # (n_pad = 0: the bound is 0 and the vector stays exactly 0)
    again = _unpartition(precision, bits, B, gh, gw, ws, cols, cols, colsum=np.zeros(cols, np.float32))[2]
    assert np.array_equal(again.view(np.uint32), s0.view(np.uint32))     # a second call: the same bits
    # ACCUMULATES: one fp32 add of the call's sum to what the vector held
    start = rng.standard_normal(cols).astype(np.float32)
    acc = _unpartition(precision, bits, B, gh, gw, ws, cols, cols, colsum=start)[2]
    assert np.array_equal(acc.view(np.uint32), ((start + s0) if n_pad else start).view(np.uint32))
    twice = _unpartition(precision, bits, B, gh, gw, ws, cols, cols, colsum=s0)[2]
    assert np.array_equal(twice.view(np.uint32), (s0 + s0).view(np.uint32))


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_refusals_leave_the_outputs_untouched(kernel_backend, precision):
    B, gh, gw, ws, cols = 2, 5, 4, 3, 384
    rng = np.random.default_rng(4)
    idx = _index(B, gh, gw, ws)
    src, srcw, fill = _bits(rng, (B * gh * gw, cols), precision), _bits(rng, (idx.size, cols), precision), _bits(rng, (cols,), precision)
    lib = emu.lib()
    part, unpart = getattr(lib, _name(precision, "partition")), getattr(lib, _name(precision, "unpartition"))
    sb, wb, fb = _staged(src), _staged(srcw), _staged(fill)
    n_out, n_back = idx.size * cols, B * gh * gw * cols
    sums = emu.B(np.full(cols, 7.0, np.float32))
    cases = [
        ("partition, null src", lambda o: part(None, cols, B, gh, gw, ws, cols, fb.p, o, emu.stream()), n_out, ARG),
        ("partition, window 0", lambda o: part(sb.p, cols, B, gh, gw, 0, cols, fb.p, o, emu.stream()), n_out, ARG),
        ("partition, window -3", lambda o: part(sb.p, cols, B, gh, gw, -3, cols, fb.p, o, emu.stream()), n_out, ARG),
        ("partition, pitch below the width", lambda o: part(sb.p, cols - 8, B, gh, gw, ws, cols, fb.p, o, emu.stream()), n_out, ARG),
        ("partition, no images", lambda o: part(sb.p, cols, 0, gh, gw, ws, cols, fb.p, o, emu.stream()), n_out, ARG),
        ("partition, a row that is no multiple of 16 bytes", lambda o: part(sb.p, cols, B, gh, gw, ws, cols - 2, fb.p, o, emu.stream()), n_out,
         UNSUPPORTED),
        ("un-partition, null src", lambda o: unpart(None, B, gh, gw, ws, cols, o, cols, sums.p, emu.stream()), n_back, ARG),
        ("un-partition, window 0", lambda o: unpart(wb.p, B, gh, gw, 0, cols, o, cols, sums.p, emu.stream()), n_back, ARG),
        ("un-partition, pitch below the width", lambda o: unpart(wb.p, B, gh, gw, ws, cols, o, cols - 8, sums.p, emu.stream()), n_back, ARG),
    ]
    for what, call, n, code in cases:
        obuf, optr = _guarded(n, precision)
        assert call(optr) == code, what
        assert np.all(_unguard(obuf, n, precision) == CANARY[precision]), what
    assert part(sb.p, cols, B, gh, gw, ws, cols, fb.p, None, emu.stream()) == ARG
    assert unpart(wb.p, B, gh, gw, ws, cols, None, cols, sums.p, emu.stream()) == ARG
    assert np.all(sums.np() == 7.0)                                       # no refused call reached the sums


# ---- the prefix-free token assembly and the last residual add -----------------------------------------------------------------------------
def _bf16_bits(a):
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def _bits_f32(b):
    return (b.astype(np.uint32) << 16).view(np.float32)


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_pos_tokens_forward_and_backward(kernel_backend, precision):
    """x[b][p] = float(patch[b][p]) + pos[p]: one fp32 add, exact against numpy;  backward: dpatch = dx (rounded to bf16 in the product
    form), dpos = sum over the images in ascending order - WRITTEN, whatever the target held"""
    B, Np, D = 3, 25, 128            # 400 lanes of work per image: a partial second workgroup
    rng = np.random.default_rng(5)
    lib = emu.lib()
    pre = "lp_vit_pos_tokens_" if precision == "bf16" else "lp_f32_vit_pos_tokens_"
    patch = rng.standard_normal((B * Np, D)).astype(np.float32)
    parg = _bf16_bits(patch) if precision == "bf16" else patch
    patch = _bits_f32(parg) if precision == "bf16" else patch
    pos = rng.standard_normal((Np, D)).astype(np.float32)
    x = emu.B(np.full((B * Np, D), np.nan, np.float32))
    pbuf, posbuf = emu.B(parg), emu.B(pos)            # (named: a buffer must outlive the launch that reads it)
    assert getattr(lib, pre + "fwd")(pbuf.p, posbuf.p, B, Np, D, x.p, emu.stream()) == 0
    assert np.array_equal(x.np(), (patch.reshape(B, Np, D) + pos[None]).reshape(B * Np, D))
    dx = rng.standard_normal((B * Np, D)).astype(np.float32)
    dpatch = emu.B(np.zeros((B * Np, D), np.uint16 if precision == "bf16" else np.float32))
    dpos = emu.B(np.full((Np, D), 99.0, np.float32))
    dxbuf = emu.B(dx)
    assert getattr(lib, pre + "bwd")(dxbuf.p, B, Np, D, dpatch.p, dpos.p, emu.stream()) == 0
    assert np.array_equal(dpatch.np(), _bf16_bits(dx) if precision == "bf16" else dx)
    want = np.zeros((Np, D), np.float32)
    for b in range(B):
        want = want + dx.reshape(B, Np, D)[b]
    assert np.array_equal(dpos.np(), want)
    assert getattr(lib, pre + "fwd")(None, posbuf.p, B, Np, D, x.p, emu.stream()) == ARG
    assert getattr(lib, pre + "fwd")(pbuf.p, posbuf.p, B, Np, 12, x.p, emu.stream()) == UNSUPPORTED


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_final_residual_add(kernel_backend, precision):
    n = 75 * 128
    rng = np.random.default_rng(6)
    lib = emu.lib()
    x = rng.standard_normal(n).astype(np.float32)
    delta = rng.standard_normal(n).astype(np.float32)
    dy = rng.standard_normal(n).astype(np.float32)
    xo, dxo = emu.B(np.full(n, np.nan, np.float32)), emu.B(np.full(n, np.nan, np.float32))
    xb = emu.B(x)                                      # (named: a buffer must outlive the launch that reads it)
    if precision == "bf16":
        dbits, gbits, ybuf = _bf16_bits(delta), _bf16_bits(dy), emu.B(np.zeros(n, np.uint16))
        db, gb = emu.B(dbits), emu.B(gbits)
        assert lib.lp_resid_out_fwd(xb.p, db.p, n, xo.p, ybuf.p, emu.stream()) == 0
        want = x + _bits_f32(dbits)
        assert np.array_equal(xo.np(), want) and np.array_equal(ybuf.np(), _bf16_bits(want))
        assert lib.lp_resid_out_bwd(gb.p, n, dxo.p, emu.stream()) == 0
        assert np.array_equal(dxo.np(), _bits_f32(gbits))
        assert lib.lp_resid_out_fwd(xb.p, db.p, n, xo.p, None, emu.stream()) == ARG
        assert lib.lp_resid_out_fwd(xb.p, db.p, n - 4, xo.p, ybuf.p, emu.stream()) == UNSUPPORTED
    else:
        db, gb = emu.B(delta), emu.B(dy)
        assert lib.lp_f32_resid_out_fwd(xb.p, db.p, n, xo.p, emu.stream()) == 0
        assert np.array_equal(xo.np(), x + delta)
        assert lib.lp_f32_resid_out_bwd(gb.p, n, dxo.p, emu.stream()) == 0
        assert np.array_equal(dxo.np(), dy)
        assert lib.lp_f32_resid_out_fwd(None, db.p, n, xo.p, emu.stream()) == ARG
