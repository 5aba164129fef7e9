"""The bf16 ViT glue kernels (csrc/vit.hip, and lp_cast_bf16 / lp_permute_cba of csrc/optim.hip) held to float64, one entry point at a time.

These kernels are the product path of every ViT, DINOv2, DINOv3 and multi-view tracker between its GEMMs; tests/test_emu_vit_ops.py runs
them on the emulated build against fp32 torch at 1e-2.  Here every reference is plain torch float64 on the same operands (bf16 operands are
float values rounded to bf16 on the host and handed over as int16 bits; the reference reads the same rounded values), on the emulated build
in the CPU suite and on the device under `-m gpu` (stack_backend).

entry point (csrc/vit.hip)               test
---------------------------------------  ----------------------------------------------------------------------------------------
lp_vit_patchify                          test_patchify, test_argument_checks
lp_vit_tokens_fwd / _bwd                 test_tokens, test_argument_checks
lp_vit_mv_tokens_fwd / _bwd              tests/test_mvt_token_kernels.py         (lp_vit_mv_tokens_bwd_workspace_bytes too)
lp_small_matmul                          test_small_matmul, test_argument_checks
lp_layernorm_fwd                         test_layernorm_fwd, test_argument_checks
lp_layernorm_bwd                         test_layernorm_bwd, test_argument_checks
lp_layernorm_bwd_bf16                    test_layernorm_bwd, test_argument_checks
lp_layernorm_bwd_bf16_colsum             test_layernorm_bwd, test_argument_checks
lp_layernorm_ls_fwd / _bwd               tests/test_dinov2_layerscale_kernels.py
lp_layernorm_ls_fwd_px / _bwd_px         tests/test_dinov3_rope_kernels.py
lp_gelu_fwd / _bwd                       test_gelu, test_gelu_constants, test_argument_checks
lp_gelu_bwd_colsum                       test_gelu_bwd_colsum, test_argument_checks
lp_softmax_rows_fwd / _bwd               test_softmax_rows, test_argument_checks
lp_attn_rowdot                           test_attn_rowdot, test_argument_checks  (also tests/test_step_contractions_fp64.py)
lp_transpose_batched                     test_transpose_batched, test_argument_checks
(csrc/optim.hip) lp_cast_bf16            test_cast_bf16, test_argument_checks
(csrc/optim.hip) lp_permute_cba          test_permute_cba, test_argument_checks
(csrc/attn.hip: lp_attn_fwd, lp_attn_bwd_kv, lp_attn_dscores - tests/test_step_contractions_fp64.py; csrc/rope.hip: lp_rope_fwd / _bwd,
lp_vit_reg_tokens_fwd / _bwd - tests/test_dinov3_rope_kernels.py)

Bars.  fp32 results: sums |y - r| <= 2^-18 S, S = sum |terms| (fp64_ref.f32_bar); short formulas c 2^-24 (sum of |terms|), c = the roundings
counted beside each bar; a single fp32 addition: the correctly rounded float64 sum, bit for bit.  bf16 results: |y - r| <= h(|r| + e) + e,
e = the fp32 bar of the value before the store and h(v) = half an ulp of bf16 at v = 2^(floor(log2 v) - 8) (fp64_ref.bf16_store_bar):
exactly one round-to-nearest to bf16.  (h runs from 2^-9 v at the top of a binade to 2^-8 v at its bottom - 8 significant bits - so a flat
2^-9 (|r| + e) + e fails a correctly rounding store: 1 + 0.9 x 2^-8 -> 1 is 1.8 times off it, and the kernels here measured 1.97.)  A bf16
result that can be
recomputed from the kernel's own fp32 output (dx_bf16 from dx_acc, dpatch, patchify, the cast): the round-to-nearest-even bits, bit for bit.
Stored soft-max probabilities: the attention bar of tests/test_step_contractions_fp64.py, |P - p| <= 2^-8 p + 2^-20, pad columns exactly 0,
rows summing to 1 within 2^-8 + n 2^-22 (derived in test_softmax_rows).  GELU: see GELU16_FWD_C.  Data movement: exact.  Every family builds
wrong references from the same float64 code and asserts that its bar REJECTS them; every family with a bf16 output has among them the
reference truncated to bf16 (the low 16 bits of its fp32 image cleared: off by up to a whole ulp) - for the soft-max it sits on the
backward, whose bar is the one-rounding one (the stored probabilities' 2^-8 p + 2^-20 is this project's attention bar, kept as it is).  No element is excluded from any comparison.  fp32 atomics (d gamma, d beta, the column
sums): no bit-identity across runs is asserted; everything else runs twice on fresh outputs and must give the same bits (_twice).

MARGINS (entry point -> worst |y - r| / bar) is printed at the end of the module with -s."""

from __future__ import annotations

import ctypes as C
import math

import pytest
import torch

from tests import fp64_ref as R
from tests.test_fp32_validation_kernels import LP_ERR_ARGUMENT, LP_ERR_UNSUPPORTED, SENT, U, _call, _rejects, _run, _sent, _t, _twice

F64 = torch.float64
SENT16 = 0x7FA5           # what bf16 output buffers hold before a call: a NaN pattern no kernel produces (worst() counts it as infinitely off)
BF16_MAX = 3.3895313892515355e38     # 0x7F7F, the largest finite bf16
MARGINS: dict = {}        # entry point (. output) -> worst |y - r| / bar over its cases

# GELU.  gelu8 / gelu8_bwd (csrc/lp_common.h, shared with the GEMM store passes) do NOT call erff / expf as the fp32 kernels do: the forward
# is the erfcc Chebyshev fit, the backward Abramowitz & Stegun 7.1.26, on v_rcp_f32 and __expf - so GELU_FWD_C / GELU_BWD_C of the fp32 module
# do not apply.  An independent fp32 evaluation of the same two formulas (fp64_ref.gelu_erfcc_f32 / gelu_grad_as26_f32: torch float32 on the
# CPU, one operation per rounding) on the operands of test_gelu - all 8,388,904 values of the large case and the 1000 of the small one with
# its edge values - is off the float64 GELU (erf, fp64_ref.gelu / gelu_grad) by at most
#     forward   1.998 units of 2^-24 (|y| + |x|)                   backward  9.372 units of 2^-24 |dy| (|gelu'(x)| + |x|)
# (the fits' own error included: the backward's 1.5e-7 is 2.5 units of 2^-24 on a gelu' of 0.5, and both maxima sit at |x| < 0.05;
# test_gelu_constants recomputes both figures).  The hardware reciprocal and exponential differ from the
# host's by an ulp or two, so the kernels get 4 x that, as in the fp32 module - for e, the fp32 error in front of the bf16 store.
GELU16_FWD_MEASURED, GELU16_BWD_MEASURED = 2.00, 9.38
GELU16_FWD_C = 4 * GELU16_FWD_MEASURED
GELU16_BWD_C = 4 * GELU16_BWD_MEASURED


@pytest.fixture(scope="module", autouse=True)
def _print_margins():
    yield
    print("\nMARGINS (worst |y - r| / bar):")
    for k in sorted(MARGINS):
        print(f"  {k:40s} {MARGINS[k]:.4f}")


# ---------------------------------------------------------------------------------------------------------------- helpers
def _hold(name, y, r, bar):
    m = R.worst(y, r, bar)
    MARGINS[name] = max(MARGINS.get(name, 0.0), m)
    assert m <= 1.0, f"{name}: worst |y - r| / bar = {m:.3f}"


def _t16(dev, seed, *shape, scale=1.0, shift=0.0):
    """seeded bf16 operand, rounded on the host: -> (int16 bits for the kernel, the float32 values those bits stand for)"""
    bits = R.bf16_bits(torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale + shift)
    return bits.to(dev), R.bf16_f32(bits).to(dev)


def _sent16(dev, *shape):
    return torch.full(shape, SENT16, dtype=torch.int16, device=dev)


def _untouched(t):
    return bool((t == (SENT16 if t.dtype == torch.int16 else SENT)).all())


# ---------------------------------------------------------------------------------------------------------------- LayerNorm
# M = 15 with drop_T = 5: odd (the last row's partner half is dead across the shuffles), a two-row pair straddles an image boundary.
# D = 4: one live lane per half; 100; 384; 640: five passes on the NP = 6 instance; 896: seven on NP = 8; 1024.  16400 x 64: more than 2048
# workgroups of 8 rows, every workgroup makes a second round.
LN_SHAPES = [(15, D, 5) for D in (4, 100, 384, 640, 896, 1024)] + [(16400, 64, 0)]
LN_EPS = 1e-6


def _ln_np(D):
    """the template width the launchers pick"""
    return {1: 1, 2: 2, 3: 3, 4: 4, 5: 6, 6: 6}.get(-(-D // 128), 8)


@pytest.mark.parametrize("M,D,drop_T", LN_SHAPES)
def test_layernorm_fwd(stack_backend, M, D, drop_T):
    """lp_layernorm_fwd: delta NULL / given / given with x_out aliasing x / NULL with an x_out (a copy, as the header says); dropped rows
    still get mean and rstd; y ends where it should (a guard row behind it); twice, the same bits"""
    dev = stack_backend
    x = _t(dev, 11, M, D, shift=0.5)
    dbits, delta = _t16(dev, 12, M, D, scale=0.3)
    gamma, beta = _t(dev, 13, D, shift=1.0), _t(dev, 14, D)
    g64, b64 = gamma.to(F64), beta.to(F64)
    rows = R.kept_rows(M, drop_T, dev)
    for mode in ("plain", "delta", "delta, x_out = x", "copy"):
        has_delta = mode.startswith("delta")

        def once():
            xin = x.clone()
            xo = None if mode == "plain" else (xin if "=" in mode else _sent(dev, M, D))
            y, mean, rstd = _sent16(dev, len(rows) + 1, D), _sent(dev, M), _sent(dev, M)
            _run("lp_layernorm_fwd", xin, dbits if has_delta else None, xo, gamma, beta, LN_EPS, M, D, drop_T, y, mean, rstd)
            return y, mean, rstd, xin if xo is None else xo, xin
        y, mean, rstd, xo, xin = _twice(once)
        # x_out = one fp32 sum: the correctly rounded float64 sum, bit for bit (no delta: x itself, and x is still what it was)
        xs32 = (x.to(F64) + delta.to(F64)).to(torch.float32) if has_delta else x
        assert torch.equal(xo, xs32)
        assert "=" in mode or torch.equal(xin, x)
        assert _untouched(y[-1])
        xs = xs32.to(F64)
        mu = xs.mean(1)
        bar_mu = R.f32_bar(xs.abs().sum(1)) / D
        _hold("lp_layernorm_fwd.mean", mean, mu, bar_mu)
        for cols in {128 * -(-D // 128), 128 * _ln_np(D)} - {D}:
            _rejects(f"LayerNorm forward: the mean over {cols} columns instead of D = {D}", mean, xs.sum(1) / cols, bar_mu)
        # rstd = (var + eps)^-1/2: var is a sum of squares of differences, held to 2^-18 of the same sum on (|x| + |mean|) (the
        # cancellation in x - mean), which moves rstd by rstd / 2 * dvar / (var + eps); then three roundings (+ eps, sqrt, 1 / .)
        var = ((xs - mu[:, None]) ** 2).mean(1)
        rs = (var + LN_EPS) ** -0.5
        dvar = R.f32_bar(((xs.abs() + mu.abs()[:, None]) ** 2).sum(1)) / D
        bar_rs = rs * (0.5 * dvar / (var + LN_EPS) + 3 * U)
        _hold("lp_layernorm_fwd.rstd", rstd, rs, bar_rs)
        _rejects("LayerNorm forward: rstd from the unbiased variance", rstd, (var * D / (D - 1) + LN_EPS) ** -0.5, bar_rs)
        # y = bf16(fma((x - mean) * rstd, gamma, beta)) from the kernel's OWN mean / rstd (held above): the difference, the product and
        # the fused multiply-add round once each in fp32 - e = 3 roundings on either term - then the one rounding of the store
        t = (xs - mean.to(F64)[:, None]) * rstd.to(F64)[:, None] * g64
        yr, e = t + b64, 3 * U * (t.abs() + b64.abs())
        bar = R.bf16_store_bar(yr, e)
        yv = R.bf16_value(y[:-1])
        _hold("lp_layernorm_fwd.y", yv, yr[rows], bar[rows])
        _rejects("LayerNorm forward: y truncated to bf16", yv, R.bf16_trunc(yr[rows]), bar[rows])
        if drop_T:
            off = R.kept_rows(M, drop_T, dev, shift=1)
            _rejects("LayerNorm forward: drop_T mapping off by one row", yv, yr[off], bar[off])


@pytest.mark.parametrize("M,D,drop_T", LN_SHAPES)
def test_layernorm_bwd(stack_backend, M, D, drop_T):
    """lp_layernorm_bwd, lp_layernorm_bwd_bf16, lp_layernorm_bwd_bf16_colsum on the same operands: dx_acc, d gamma, d beta and the column sums
    accumulated onto non-zero values; the three leave bit-identical dx_acc; dx_bf16 = the round-to-nearest-even cast of the updated dx_acc,
    bit for bit.  A dropped row ([CLS]: no dy) takes dy = 0, as include/lp_hip.h says of the LayerScale forms ("rows without a dy still carry
    stream gradient") and as ViTEngine._ln_bwd relies on: its dx_acc stays bit for bit, its dx_bf16 is the cast of that value, and it is part
    of the column sums (the bias gradient of the next Linear layer, whose dy has all M rows).  d gamma / d beta / column sums are fp32 atomics."""
    dev = stack_backend
    x, gamma = _t(dev, 21, M, D, shift=0.5), _t(dev, 22, D, shift=1.0)
    rows = R.kept_rows(M, drop_T, dev)
    dyb, dy = _t16(dev, 23, len(rows), D)
    xs, dyd, g64 = x.to(F64), dy.to(F64), gamma.to(F64)
    mean = xs.mean(1).to(torch.float32)
    rstd = ((xs.var(1, unbiased=False) + LN_EPS) ** -0.5).to(torch.float32)
    dx0, dg0, db0, cs0 = _t(dev, 24, M, D), _t(dev, 25, D), _t(dev, 26, D), _t(dev, 27, D)
    atomics = {}

    def once():
        out = []
        for name in ("lp_layernorm_bwd", "lp_layernorm_bwd_bf16", "lp_layernorm_bwd_bf16_colsum"):
            dx, dg, db, cs, d16 = dx0.clone(), dg0.clone(), db0.clone(), cs0.clone(), _sent16(dev, M + 1, D)
            tail = {"lp_layernorm_bwd": (dx, dg, db), "lp_layernorm_bwd_bf16": (dx, d16, dg, db)}.get(name, (dx, d16, dg, db, cs))
            _run(name, dyb, x, mean, rstd, gamma, M, D, drop_T, *tail)
            atomics[name] = (dg, db, cs)
            out += [dx, d16]
        return tuple(out)
    dx, untouched16, dx_b, d16_b, dx_c, d16_c = _twice(once)
    assert torch.equal(dx, dx_b) and torch.equal(dx, dx_c)
    assert _untouched(untouched16) and _untouched(d16_b[-1]) and _untouched(d16_c[-1])
    want16 = R.bf16_bits(dx)
    assert torch.equal(d16_b[:-1], want16) and torch.equal(d16_c[:-1], want16)
    assert not torch.equal(R.bf16_f32(want16).to(F64), R.bf16_trunc(dx.to(F64)))     # (... which a truncating store fails)
    xh_all = (xs - mean.to(F64)[:, None]) * rstd.to(F64)[:, None]

    def ref(sel):
        """dy row j belongs to input row sel[j]: -> (dx, bar) on the rows sel, dgamma, its S"""
        xh, rs, g = xh_all[sel], rstd.to(F64)[sel][:, None], dyd * g64
        a, b = g.mean(1, keepdim=True), (g * xh).mean(1, keepdim=True)
        a_s, b_s = g.abs().mean(1, keepdim=True), (g * xh).abs().mean(1, keepdim=True)
        r = dx0.to(F64)[sel] + rs * (g - a - xh * b)
        # the two row means are sums held to 2^-18 of their |terms|; around them dy gamma, xhat (two roundings), xhat b, the two
        # differences, the product with rstd and the sum onto dx_acc: no term passes through more than 7 roundings
        terms = rs * (g.abs() + a_s + xh.abs() * b_s) + dx0.to(F64)[sel].abs()
        bar = 2.0 ** -18 * rs * (a_s + xh.abs() * b_s) + 7 * U * terms
        return r, bar, dg0.to(F64) + (dyd * xh).sum(0), dg0.to(F64).abs() + (dyd * xh).abs().sum(0)
    r, bar, dgr, dgs = ref(rows)
    _hold("lp_layernorm_bwd.dx", dx[rows], r, bar)
    for name, (dg, db, cs) in atomics.items():
        _hold(name + ".dgamma", dg, dgr, R.f32_bar(dgs))
        bar_db = R.f32_bar(db0.to(F64).abs() + dyd.abs().sum(0))
        _hold(name + ".dbeta", db, db0.to(F64) + dyd.sum(0), bar_db)
        _rejects("LayerNorm backward: the last dy row left out of dbeta", db, db0.to(F64) + dyd[:-1].sum(0), bar_db)
        assert name.endswith("colsum") or torch.equal(cs, cs0)
    if drop_T:
        dropped = torch.arange(0, M, drop_T, device=dev)
        assert torch.equal(dx[dropped], dx0[dropped])
        off = R.kept_rows(M, drop_T, dev, shift=1)
        rm, _, dgm, _ = ref(off)
        full = dx0.to(F64).clone()
        full[off] = rm
        _rejects("LayerNorm backward: drop_T mapping off by one row (dx)", dx[rows], full[rows], bar)
        _rejects("LayerNorm backward: drop_T mapping off by one row (dgamma)", atomics["lp_layernorm_bwd"][0], dgm, R.f32_bar(dgs))
    # the column sums against the float64 sums of the kernel's OWN updated dx_acc, all M rows: only the accumulation is measured
    cs, dxd = atomics["lp_layernorm_bwd_bf16_colsum"][2], dx.to(F64)
    bar_cs = R.f32_bar(cs0.to(F64).abs() + dxd.abs().sum(0))
    _hold("lp_layernorm_bwd_bf16_colsum.colsum", cs, cs0.to(F64) + dxd.sum(0), bar_cs)
    _rejects("LayerNorm backward: column sums without the last 8-row block", cs, cs0.to(F64) + dxd[:(M - 1) // 8 * 8].sum(0), bar_cs)
    if M == 15:
        # M = 15: the roundings of 15 bf16 values add up to about sqrt(15) 2^-10 of a term, fifty times the bar 2^-18 x 15 terms; at
        # 16400 rows that random walk (sqrt(M) against M) sinks to the bar itself, so the mutant is built at M = 15 alone
        _rejects("LayerNorm backward: column sums of the bf16-rounded values", cs, cs0.to(F64) + R.bf16_value(want16).sum(0), bar_cs)


# ---------------------------------------------------------------------------------------------------------------- GELU
GELU_BIG = 8_388_608 + 8 * 37     # above vit_grid's 4096 workgroups x 256 lanes x 8 elements: 37 chunks are left for the stride loop
GELU_EDGES = [0.0, -0.0, 1e-30, -1e-30, 6.0, -6.0, 12.0, -12.0, BF16_MAX, -BF16_MAX]


def _gelu_operands(dev, n):
    """x ~ N(0, 2^2) and dy ~ N(0, 1) rounded to bf16; n = 1000: the edge values among them -> (x bits, x, dy bits, dy)"""
    gen = torch.Generator().manual_seed(31)
    xb, dyb = R.bf16_bits(torch.randn(n, generator=gen) * 2.0), R.bf16_bits(torch.randn(n, generator=gen))
    if n == 1000:
        xb[:len(GELU_EDGES)] = R.bf16_bits(torch.tensor(GELU_EDGES, dtype=torch.float32))
        assert int(xb[8]) == 0x7F7F and int(xb[1]) == -0x8000
    return xb.to(dev), R.bf16_f32(xb).to(dev), dyb.to(dev), R.bf16_f32(dyb).to(dev)


def _gelu_e(xd, dyd):
    """-> (gelu, e), (dy gelu', e): the float64 results and the fp32 bars in front of the store"""
    r, gr = R.gelu(xd), R.gelu_grad(xd)
    return (r, GELU16_FWD_C * U * (r.abs() + xd.abs())), (dyd * gr, GELU16_BWD_C * U * dyd.abs() * (gr.abs() + xd.abs()))


@pytest.mark.parametrize("n", [1000, GELU_BIG], ids=["n1000", "above_2^23"])
def test_gelu(stack_backend, n):
    """lp_gelu_fwd / _bwd on 1000 values with +-0, +-1e-30, +-6, +-12 and the largest finite bf16 among them, and on 8,388,904 (the
    grid-stride loop); a guard chunk behind either output"""
    dev = stack_backend
    xb, x, dyb, dy = _gelu_operands(dev, n)

    def once():
        y, dx = _sent16(dev, n + 8), _sent16(dev, n + 8)
        _run("lp_gelu_fwd", xb, C.c_size_t(n), y)
        _run("lp_gelu_bwd", xb, dyb, C.c_size_t(n), dx)
        return y, dx
    y, dx = _twice(once) if n == 1000 else once()
    assert _untouched(y[n:]) and _untouched(dx[n:])
    xd = x.to(F64)
    (r, e), (rb, eb) = _gelu_e(xd, dy.to(F64))
    yv, dxv = R.bf16_value(y[:n]), R.bf16_value(dx[:n])
    _hold("lp_gelu_fwd", yv, r, R.bf16_store_bar(r, e))
    _hold("lp_gelu_bwd", dxv, rb, R.bf16_store_bar(rb, eb))
    _rejects("GELU: tanh approximation", yv, 0.5 * xd * (1 + torch.tanh(math.sqrt(2 / math.pi) * (xd + 0.044715 * xd ** 3))),
             R.bf16_store_bar(r, e))
    _rejects("GELU forward: truncated to bf16", yv, R.bf16_trunc(r), R.bf16_store_bar(r, e))
    _rejects("GELU backward: truncated to bf16", dxv, R.bf16_trunc(rb), R.bf16_store_bar(rb, eb))


def test_gelu_constants(stack_backend):
    """GELU16_FWD_MEASURED / GELU16_BWD_MEASURED are what the independent fp32 evaluation of the kernels' formulas gives on this module's
    operands (on the host, whatever the backend; the first 2^20 values of the large case stand for it here)"""
    worst = [0.0, 0.0]
    for n in (1000, GELU_BIG):
        _, x, _, dy = _gelu_operands(torch.device("cpu"), n)
        x, dy = x[:1 << 20], dy[:1 << 20]
        xd, dyd = x.to(F64), dy.to(F64)
        r, gr = R.gelu(xd), R.gelu_grad(xd)
        worst[0] = max(worst[0], R.worst(R.gelu_erfcc_f32(x), r, U * (r.abs() + xd.abs())))
        worst[1] = max(worst[1], R.worst(dy * R.gelu_grad_as26_f32(x), dyd * gr, U * dyd.abs() * (gr.abs() + xd.abs())))
    print(f"\nindependent fp32 GELU: forward {worst[0]:.3f}, backward {worst[1]:.3f} units")
    assert worst[0] <= GELU16_FWD_MEASURED and worst[1] <= GELU16_BWD_MEASURED


@pytest.mark.parametrize("rows,cols", [(7, 520), (8200, 64), (1, 8)])
def test_gelu_bwd_colsum(stack_backend, rows, cols):
    """lp_gelu_bwd_colsum: 7 x 520 = 65 chunks (the second column group has one live lane) and rows % 4 = 3; 8200 rows: above the cap of
    2048 row blocks; 1 x 8.  dx = the bits of lp_gelu_bwd; the column sums of the UNROUNDED products added onto a non-zero start (fp32
    atomics: no bit-identity asserted)."""
    dev = stack_backend
    n = rows * cols
    xb, x = _t16(dev, 41, rows, cols, scale=2.0)
    dyb, dy = _t16(dev, 42, rows, cols)
    cs0 = _t(dev, 43, cols)
    want = _sent16(dev, n)
    _run("lp_gelu_bwd", xb, dyb, C.c_size_t(n), want)
    dx, cs = _sent16(dev, n + 8), cs0.clone()
    _run("lp_gelu_bwd_colsum", xb, dyb, rows, cols, dx, cs)
    assert torch.equal(dx[:n], want) and _untouched(dx[n:])
    prod = dy.to(F64) * R.gelu_grad(x.to(F64))
    bar = R.f32_bar(cs0.to(F64).abs() + prod.abs().sum(0))
    _hold("lp_gelu_bwd_colsum.colsum", cs, cs0.to(F64) + prod.sum(0), bar)
    _rejects("GELU backward column sums: the last row left out", cs, cs0.to(F64) + prod[:-1].sum(0), bar)


# ---------------------------------------------------------------------------------------------------------------- soft-max rows
# (rows, n, ld): the smallest; one chunk per lane with pads; 577 of 640: two chunks per lane, the second pass partly live; the widest
# row; 16390 rows: above 4096 workgroups x 4 rows, and 16390 % 4 = 2
SM_SHAPES = [(5, 1, 8), (21, 77, 128), (6, 577, 640), (5, 1024, 1024), (16390, 5, 8)]
SM_SCALE = 0.125


@pytest.mark.parametrize("rows,n,ld", SM_SHAPES)
def test_softmax_rows(stack_backend, rows, n, ld):
    """lp_softmax_rows_fwd / _bwd, in place.  Row 0 spans +-30 after the scale evenly, row 1 is N(0, 10^2) after it, the rest N(0, 1); the
    pad columns [n, ld) of the scores hold LARGE values (3 / scale above the row's maximum: a kernel that reads one shows at once) and must
    come back exactly 0, in both directions."""
    dev = stack_backend
    gen = torch.Generator().manual_seed(51)
    s = torch.randn(rows, ld, generator=gen) * 8.0
    s[0] = torch.linspace(-240.0, 240.0, ld)
    if rows > 1:
        s[1] *= 10.0
    s[:, n:] = s[:, :n].amax(1, keepdim=True) + 24.0
    sb = R.bf16_bits(s).to(dev)
    sd = R.bf16_value(sb)

    def fwd():
        p = torch.cat([sb.reshape(-1), _sent16(dev, 8)])
        _run("lp_softmax_rows_fwd", p, rows, n, ld, SM_SCALE)
        return (p,)
    pb, = _twice(fwd)
    assert _untouched(pb[rows * ld:])
    pb = pb[:rows * ld].reshape(rows, ld)
    assert bool((pb[:, n:] == 0).all())
    P, p = R.bf16_value(pb[:, :n]), torch.softmax(SM_SCALE * sd[:, :n], -1)
    bar = 2.0 ** -8 * p + 2.0 ** -20
    _hold("lp_softmax_rows_fwd", P, p, bar)
    # every stored probability is one round-to-nearest of an fp32 value (off by at most half an ulp, <= 2^-8 of it), and those fp32 values
    # are n products v_j inv with sum(v) inv = 1 up to the n roundings of the sum, of 1 / sum and of the n products: within n 2^-23, as the
    # fp32 module counts - so the stored row sums to 1 within 2^-8 (1 + n 2^-23) + n 2^-23 <= 2^-8 + n 2^-22
    assert float((P.sum(1) - 1).abs().max()) <= 2.0 ** -8 + n * 2.0 ** -22
    if ld > n:
        _rejects("soft-max forward: column n counted as valid", P, torch.softmax(SM_SCALE * sd[:, :n + 1], -1)[:, :n], bar)
    else:
        _rejects("soft-max forward: the last column left out", P[:, :-1], torch.softmax(SM_SCALE * sd[:, :n - 1], -1), bar[:, :-1])

    dpb, dp = _t16(dev, 52, rows, ld)        # (its pad columns hold values too: they must come back 0)

    def bwd():
        d = torch.cat([dpb.reshape(-1), _sent16(dev, 8)])
        _run("lp_softmax_rows_bwd", pb, d, rows, n, ld, SM_SCALE)
        return (d,)
    db, = _twice(bwd)
    assert _untouched(db[rows * ld:])
    db = db[:rows * ld].reshape(rows, ld)
    assert bool(((db[:, n:] & 0x7FFF) == 0).all())       # (a zero of either sign: 0 x (0 - dot) is -0 where dot > 0)
    dpd = dp.to(F64)[:, :n]
    dot, dot_s = (P * dpd).sum(1, keepdim=True), (P * dpd).abs().sum(1, keepdim=True)
    r = SM_SCALE * P * (dpd - dot)
    # scale p (dp - dot) from the STORED probabilities: dot is a sum held to 2^-18 of its |terms|; the difference and the two products round
    # once each in fp32 (3 roundings on either term); then the one rounding of the store
    e = SM_SCALE * P * (2.0 ** -18 * dot_s + 3 * U * (dpd.abs() + dot.abs()))
    bar = R.bf16_store_bar(r, e)
    ds = R.bf16_value(db[:, :n])
    _hold("lp_softmax_rows_bwd", ds, r, bar)
    if n > 1:     # (n = 1: p = 1 and dp - dot = 0, every result is 0)
        _rejects("soft-max backward: truncated to bf16", ds, R.bf16_trunc(r), bar)
        _rejects("soft-max backward: the scale left out", ds, r / SM_SCALE, bar)


# ---------------------------------------------------------------------------------------------------------------- per-head row dot
@pytest.mark.parametrize("rows,nh", [(7, 1), (7, 6), (7, 12), (7, 13), (16390, 1)])
def test_attn_rowdot(stack_backend, rows, nh):
    """lp_attn_rowdot: nh = 13 makes a second pass with 5 live heads (the lanes of dead chunks take part in the butterfly); ld > nh 64, the
    columns behind the heads hold values; 16390 rows: above 4096 workgroups x 4 rows, 16390 % 4 = 2"""
    dev = stack_backend
    ld = nh * 64 + 8
    ab, a = _t16(dev, 61, rows, ld)
    bb, b = _t16(dev, 62, rows, ld)

    def once():
        out = _sent(dev, rows * nh + 4)
        _run("lp_attn_rowdot", ab, bb, rows, nh, ld, out)
        return (out,)
    out, = _twice(once)
    assert _untouched(out[rows * nh:])
    prod = a.to(F64) * b.to(F64)
    heads = lambda t, o: t[:, o:o + nh * 64].reshape(rows, nh, 64).sum(-1)  # noqa: E731
    bar = R.f32_bar(heads(prod.abs(), 0))
    _hold("lp_attn_rowdot", out[:rows * nh].reshape(rows, nh), heads(prod, 0), bar)
    _rejects("row dot: the head boundary one 8-element chunk late", out[:rows * nh].reshape(rows, nh), heads(prod, 8), bar)


# ---------------------------------------------------------------------------------------------------------------- batched transpose
POISON = 0x7FC1   # bf16 NaN bits


# (R, Cc, ldi, in_b, in_h, ldo, out_b, out_h, nb, nh, element offset of the input's base pointer)
TR_CASES = {
    "vec_heads_77x64_ldo128": (77, 64, 200, 77 * 200, 64, 128, 3 * 64 * 128, 64 * 128, 2, 3, 0),   # heads side by side in token rows of pitch 200
    "vec_Cc13_tail": (20, 13, 32, 20 * 32, 16, 24, 2 * 13 * 24, 13 * 24, 1, 2, 0),                 # the `c + 8 > Cc` tail of the vector load
    "vec_R130_ldo136": (130, 40, 40, 130 * 40, 0, 136, 40 * 136, 0, 2, 1, 0),                      # the pad region ends inside the third 64-row tile
    "scalar_odd_pitches": (9, 7, 11, 2 * 99, 99, 13, 2 * 91, 91, 2, 2, 0),
    "scalar_base_plus_4": (77, 64, 200, 77 * 200, 64, 128, 3 * 64 * 128, 64 * 128, 2, 3, 4),       # even pitches, the base pointer 8 B off 16
}


@pytest.mark.parametrize("case", TR_CASES, ids=list(TR_CASES))
def test_transpose_batched(stack_backend, case):
    """lp_transpose_batched into an output poisoned with bf16 NaN bits: every element of [Cc][ldo] per matrix is written (the transposed
    values, zeros in [R, ldo)), anything outside - between the matrices, and a guard band behind the last one - is still poison"""
    dev = stack_backend
    Rr, Cc, ldi, in_b, in_h, ldo, out_b, out_h, nb, nh, base = TR_CASES[case]
    n_in = base + (nb - 1) * in_b + (nh - 1) * in_h + (Rr - 1) * ldi + Cc
    n_out = (nb - 1) * out_b + (nh - 1) * out_h + Cc * ldo
    src = torch.randint(-32768, 32768, (n_in + 8,), generator=torch.Generator().manual_seed(71)).to(torch.int16).to(dev)
    assert src.data_ptr() % 16 == 0

    def once():
        out = torch.full((n_out + 64,), POISON, dtype=torch.int16, device=dev)
        _run("lp_transpose_batched", src[base:], Rr, Cc, ldi, in_b, in_h, out, ldo, out_b, out_h, nb, nh)
        return (out,)
    out, = _twice(once)
    mats = src[base:].as_strided((nb, nh, Rr, Cc), (in_b, in_h, ldi, 1))
    got = out.as_strided((nb, nh, Cc, ldo), (out_b, out_h, ldo, 1))
    assert torch.equal(got[..., :Rr], mats.transpose(2, 3))
    assert bool((got[..., Rr:] == 0).all())
    written = torch.zeros(n_out + 64, dtype=torch.bool, device=dev)
    written.as_strided((nb, nh, Cc, ldo), (out_b, out_h, ldo, 1)).fill_(True)
    assert int(written.sum()) == nb * nh * Cc * ldo and bool((out[~written] == POISON).all())


# ---------------------------------------------------------------------------------------------------------------- patches and tokens
@pytest.mark.parametrize("B,H,W,P", [(2, 16, 40, 8), (1, 32, 48, 16)])
def test_patchify(stack_backend, B, H, W, P):
    """lp_vit_patchify, 8 x 8 and 16 x 16 patches of a non-square image: data movement and one rounding - the round-to-nearest-even bits of
    fp64_ref.patchify, bit for bit"""
    dev = stack_backend
    img = _t(dev, 81, B, 3, H, W)
    n = B * (H // P) * (W // P) * 3 * P * P

    def once():
        out = _sent16(dev, n + 8)
        _run("lp_vit_patchify", img, B, H, W, P, out)
        return (out,)
    out, = _twice(once)
    want = R.patchify(img, P).reshape(-1)
    assert torch.equal(out[:n], R.bf16_bits(want)) and _untouched(out[n:])
    assert not torch.equal(R.bf16_value(out[:n]), R.bf16_trunc(want.to(F64)))         # (a truncating store fails the line above)


@pytest.mark.parametrize("B,Np,D", [(3, 5, 8), (33, 255, 1024)])
def test_tokens(stack_backend, B, Np, D):
    """lp_vit_tokens_fwd (one fp32 sum per element: the correctly rounded float64 sum, bit for bit) and _bwd (dpatch the cast of dx, bit for
    bit; dpos a sum over the images, the [CLS] row with it); 33 x 256 x 128 chunks = 1,081,344 > 4096 x 256 work items"""
    dev = stack_backend
    pb, patch = _t16(dev, 91, B * Np, D)
    cls, pos = _t(dev, 92, D), _t(dev, 93, Np + 1, D)

    def fwd():
        x = _sent(dev, B * (Np + 1) * D + 8)
        _run("lp_vit_tokens_fwd", pb, cls, pos, B, Np, D, x)
        return (x,)
    x, = _twice(fwd)
    tok = torch.cat([cls.to(F64).expand(B, 1, D), patch.to(F64).reshape(B, Np, D)], 1)
    assert torch.equal(x[:-8].reshape(B, Np + 1, D), (tok + pos.to(F64)).to(torch.float32)) and _untouched(x[-8:])
    dx = _t(dev, 94, B, Np + 1, D)

    def bwd():
        dpatch, dpos = _sent16(dev, B * Np * D + 8), _sent(dev, Np + 1, D)
        _run("lp_vit_tokens_bwd", dx, B, Np, D, dpatch, dpos)
        return dpatch, dpos
    dpatch, dpos = _twice(bwd)
    want = dx[:, 1:].reshape(-1)
    assert torch.equal(dpatch[:-8], R.bf16_bits(want)) and _untouched(dpatch[-8:])
    assert not torch.equal(R.bf16_value(dpatch[:-8]), R.bf16_trunc(want.to(F64)))
    bar = R.f32_bar(dx.to(F64).abs().sum(0))
    _hold("lp_vit_tokens_bwd.dpos", dpos, dx.to(F64).sum(0), bar)
    _rejects("token backward: last image dropped from dpos", dpos, dx[:-1].to(F64).sum(0), bar)
    cut = dx.to(F64).sum(0)
    cut[0] = 0
    _rejects("token backward: no [CLS] row in dpos", dpos, cut, bar)


@pytest.mark.parametrize("transpose_w", [0, 1])
@pytest.mark.parametrize("accumulate", [0, 1])
def test_small_matmul(stack_backend, transpose_w, accumulate):
    """lp_small_matmul, y (+)= w x and y (+)= w^T x, R = 37, Q = 23, D = 101 (3737 or 2323 outputs: several workgroups, the last one ragged),
    accumulated onto non-zero values or written over the sentinel"""
    dev = stack_backend
    Rr, Q, D = 37, 23, 101
    w = _t(dev, 101, Rr, Q)
    wm = (w.T if transpose_w else w).to(F64)                   # (rows, inner)
    x, y0 = _t(dev, 102, wm.shape[1], D), _t(dev, 103, wm.shape[0], D)

    def once():
        y = torch.cat([(y0 if accumulate else _sent(dev, *y0.shape)).reshape(-1), _sent(dev, 8)])
        _run("lp_small_matmul", w, x, Rr, Q, D, transpose_w, accumulate, y)
        return (y,)
    y, = _twice(once)
    assert _untouched(y[-8:])
    y = y[:-8].reshape(y0.shape)
    base = y0.to(F64) if accumulate else torch.zeros_like(y0, dtype=F64)
    bar = R.f32_bar(base.abs() + wm.abs() @ x.to(F64).abs())
    _hold("lp_small_matmul", y, base + wm @ x.to(F64), bar)
    _rejects("small matmul: the last inner index dropped", y, base + wm[:, :-1] @ x.to(F64)[:-1], bar)
    if accumulate:
        _rejects("small matmul: written instead of accumulated", y, wm @ x.to(F64), bar)


# ---------------------------------------------------------------------------------------------------------------- the weight path
def test_cast_bf16(stack_backend):
    """lp_cast_bf16 on an odd n above 4096 x 256 (the stride loop): round to nearest even, bit for bit - ties in both directions, fp32
    denormals (to bf16 denormals, to zero and up to the smallest normal), +-inf, the largest fp32 (to inf), NaN (stays a NaN)"""
    dev = stack_backend
    n = (1 << 20) + 77
    bits = torch.randint(0, 1 << 32, (n,), generator=torch.Generator().manual_seed(111))
    bits[(bits & 0x7F800000) == 0x7F800000] = 0x3F800000      # (the random part: finite values only)
    edge = [0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,    # ties: to the even neighbour below, above, and the same negated
            0x3F807FFF, 0x3F808001,                            # either side of a tie
            0x00000001, 0x00008000, 0x00018000, 0x80018000, 0x007FFFFF, 0x00400000,   # denormals: -> 0, tie -> 0, tie -> 2, -> 0x0080, exact
            0x7F800000, 0xFF800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x00000000, 0x80000000]
    bits[:len(edge)] = torch.tensor(edge)
    nan_at = [len(edge), n - 1]
    bits[nan_at[0]], bits[nan_at[1]] = 0x7FC00000, 0xFF800001
    src = (((bits ^ 0x80000000) - 0x80000000).to(torch.int32)).view(torch.float32).to(dev)

    def once():
        out = _sent16(dev, n + 8)
        _run("lp_cast_bf16", src, C.c_size_t(n), out)
        return (out,)
    out, = _twice(once)
    assert _untouched(out[n:])
    want = R.bf16_bits(src)
    for i, w in zip(range(len(edge)), [0x3F80, 0x3F82, 0xBF80, 0xBF82, 0x3F80, 0x3F81, 0, 0, 2, 0x8002, 0x0080, 0x0040, 0x7F80, 0xFF80, 0x7F80,
                                       0xFF80, 0, 0x8000]):
        assert int(want[i]) & 0xFFFF == w, (i, hex(w))          # (the reference itself, on the values written out above)
    finite = torch.ones(n, dtype=torch.bool, device=dev)
    finite[nan_at] = False
    assert torch.equal(out[:n][finite], want[finite])
    assert bool(torch.isnan(R.bf16_f32(out[:n][~finite])).all())


def test_permute_cba(stack_backend):
    """lp_permute_cba: dst[c][b][a] = src[a][b][c], exact; A, B, C pairwise different, none a multiple of 8"""
    dev = stack_backend
    A, B, Cn = 5, 3, 7
    src = torch.randint(-32768, 32768, (A, B, Cn), generator=torch.Generator().manual_seed(121)).to(torch.int16).to(dev)

    def once():
        out = _sent16(dev, A * B * Cn + 8)
        _run("lp_permute_cba", src, A, B, Cn, out)
        return (out,)
    out, = _twice(once)
    assert torch.equal(out[:-8].reshape(Cn, B, A), src.permute(2, 1, 0)) and _untouched(out[-8:])


# ---------------------------------------------------------------------------------------------------------------- argument checks
def test_argument_checks(stack_backend):
    """null required pointers, non-positive sizes, ld < n, ld < nh 64, ldi < Cc, ldo < R, a delta without an x_out: LP_ERR_ARGUMENT; D > 1024 or
    D % 4 != 0 (LayerNorm), n / cols / D / ld % 8 != 0, ld > 1024 (soft-max), patch % 8 != 0 or H, W % patch != 0, nb nh > 65535:
    LP_ERR_UNSUPPORTED; every output buffer unchanged every time"""
    dev = stack_backend
    a, out = _t(dev, 131, 8192), _sent(dev, 8192)
    h, o16 = torch.zeros(8192, dtype=torch.int16, device=dev), _sent16(dev, 8192)
    z = C.c_size_t
    bad = [
        ("lp_vit_patchify", (None, 1, 16, 16, 8, o16)),
        ("lp_vit_patchify", (a, 1, 16, 16, 8, None)),
        ("lp_vit_patchify", (a, 0, 16, 16, 8, o16)),
        ("lp_vit_patchify", (a, 1, 16, 16, 0, o16)),
        ("lp_vit_tokens_fwd", (h, a, None, 1, 4, 8, out)),
        ("lp_vit_tokens_fwd", (h, None, a, 1, 4, 8, out)),
        ("lp_vit_tokens_fwd", (h, a, a, 1, 0, 8, out)),
        ("lp_vit_tokens_bwd", (a, 1, 0, 8, o16, out)),
        ("lp_vit_tokens_bwd", (a, 1, 4, 8, None, out)),
        ("lp_vit_tokens_bwd", (None, 1, 4, 8, o16, out)),
        ("lp_small_matmul", (a, a, 0, 3, 4, 0, 0, out)),
        ("lp_small_matmul", (None, a, 2, 3, 4, 0, 0, out)),
        ("lp_small_matmul", (a, a, 2, 3, -4, 1, 1, out)),
        ("lp_layernorm_fwd", (a, None, None, None, a, 1e-6, 4, 8, 0, o16, out, out)),
        ("lp_layernorm_fwd", (a, None, None, a, a, 1e-6, 0, 8, 0, o16, out, out)),
        ("lp_layernorm_fwd", (a, None, None, a, a, 1e-6, 4, 8, -1, o16, out, out)),
        ("lp_layernorm_fwd", (a, h, None, a, a, 1e-6, 4, 8, 0, o16, out, out)),          # delta without an x_out
        ("lp_layernorm_fwd", (a, None, None, a, a, 1e-6, 4, 8, 0, o16, None, out)),
        ("lp_layernorm_bwd", (h, a, a, a, a, 4, 0, 0, out, out, out)),
        ("lp_layernorm_bwd", (h, a, a, a, a, 4, 8, 0, out, None, out)),
        ("lp_layernorm_bwd", (None, a, a, a, a, 4, 8, 0, out, out, out)),
        ("lp_layernorm_bwd_bf16", (h, a, a, a, a, 4, 8, 0, out, None, out, out)),
        ("lp_layernorm_bwd_bf16", (h, a, a, a, a, 4, 8, -1, out, o16, out, out)),
        ("lp_layernorm_bwd_bf16_colsum", (h, a, a, a, a, 4, 8, 0, out, o16, out, out, None)),
        ("lp_layernorm_bwd_bf16_colsum", (h, a, a, a, a, 4, 8, 0, out, None, out, out, out)),
        ("lp_layernorm_bwd_bf16_colsum", (h, a, None, a, a, 4, 8, 0, out, o16, out, out, out)),
        ("lp_gelu_fwd", (h, z(0), o16)),
        ("lp_gelu_fwd", (None, z(8), o16)),
        ("lp_gelu_bwd", (h, None, z(8), o16)),
        ("lp_gelu_bwd", (h, h, z(8), None)),
        ("lp_gelu_bwd_colsum", (h, h, 0, 8, o16, out)),
        ("lp_gelu_bwd_colsum", (h, h, 4, 8, o16, None)),
        ("lp_gelu_bwd_colsum", (h, h, 4, -8, o16, out)),
        ("lp_softmax_rows_fwd", (None, 4, 5, 8, 0.125)),
        ("lp_softmax_rows_fwd", (o16, 0, 5, 8, 0.125)),
        ("lp_softmax_rows_fwd", (o16, 4, 0, 8, 0.125)),
        ("lp_softmax_rows_fwd", (o16, 4, 9, 8, 0.125)),                                  # ld < n
        ("lp_softmax_rows_bwd", (None, o16, 4, 5, 8, 0.125)),
        ("lp_softmax_rows_bwd", (h, o16, 4, 9, 8, 0.125)),
        ("lp_softmax_rows_bwd", (h, o16, -4, 5, 8, 0.125)),
        ("lp_attn_rowdot", (h, h, 4, 2, 120, out)),                                      # ld < nh 64
        ("lp_attn_rowdot", (h, h, 0, 1, 64, out)),
        ("lp_attn_rowdot", (h, h, 4, 1, 64, None)),
        ("lp_transpose_batched", (h, 8, 8, 7, 64, 0, o16, 8, 64, 0, 1, 1)),              # ldi < Cc
        ("lp_transpose_batched", (h, 8, 8, 8, 64, 0, o16, 7, 64, 0, 1, 1)),              # ldo < R
        ("lp_transpose_batched", (h, 8, 8, 8, 64, 0, o16, 8, 64, 0, 0, 1)),
        ("lp_transpose_batched", (None, 8, 8, 8, 64, 0, o16, 8, 64, 0, 1, 1)),
        ("lp_cast_bf16", (None, z(8), o16)),
        ("lp_cast_bf16", (a, z(8), None)),
        ("lp_permute_cba", (h, 0, 3, 7, o16)),
        ("lp_permute_cba", (h, 5, 3, 7, None)),
    ]
    unsupported = [
        ("lp_vit_patchify", (a, 1, 17, 16, 8, o16)),
        ("lp_vit_patchify", (a, 1, 16, 20, 8, o16)),
        ("lp_vit_patchify", (a, 1, 24, 24, 12, o16)),
        ("lp_vit_tokens_fwd", (h, a, a, 1, 4, 12, out)),
        ("lp_vit_tokens_bwd", (a, 1, 4, 12, o16, out)),
        ("lp_gelu_fwd", (h, z(12), o16)),
        ("lp_gelu_bwd", (h, h, z(1001), o16)),
        ("lp_gelu_bwd_colsum", (h, h, 4, 12, o16, out)),
        ("lp_softmax_rows_fwd", (o16, 2, 5, 1032, 0.125)),
        ("lp_softmax_rows_fwd", (o16, 4, 5, 12, 0.125)),
        ("lp_softmax_rows_bwd", (h, o16, 2, 5, 1032, 0.125)),
        ("lp_softmax_rows_bwd", (h, o16, 4, 5, 12, 0.125)),
        ("lp_attn_rowdot", (h, h, 4, 1, 68, out)),
        ("lp_transpose_batched", (h, 8, 8, 8, 0, 0, o16, 8, 0, 0, 256, 256)),            # nb nh = 65536
    ]
    for D in (1028, 6):
        unsupported += [
            ("lp_layernorm_fwd", (a, h, out, a, a, 1e-6, 4, D, 0, o16, out, out)),
            ("lp_layernorm_bwd", (h, a, a, a, a, 4, D, 0, out, out, out)),
            ("lp_layernorm_bwd_bf16", (h, a, a, a, a, 4, D, 0, out, o16, out, out)),
            ("lp_layernorm_bwd_bf16_colsum", (h, a, a, a, a, 4, D, 0, out, o16, out, out, out)),
        ]
    for want, table in ((LP_ERR_ARGUMENT, bad), (LP_ERR_UNSUPPORTED, unsupported)):
        for name, args in table:
            assert _call(name, *args) == want, (name, args)
            assert _untouched(out) and _untouched(o16), (name, args)
