"""LayerScale inside the two LayerNorm walks (lp_layernorm_ls_fwd / _bwd and their fp32 forms, include/lp_hip.h) - the only new arithmetic of the
DINOv2 backbones.

forward   x_out = x + (delta * ls): numpy float32, the product and the sum as two operations, bit for bit (one fused multiply-add differs);
          mean / rstd against float64; y against the float64 LayerNorm of the kernel's own x_out.
backward  dx_acc / d gamma / d beta against the float64 formula; the emitted gradient = round(float32(ls * o)) of the dx_acc the kernel returned,
          bit for bit; the column sums and the scale's gradient within n 2^-24 sum|terms| of float64 (the bound of ANY summation order - they
          are float atomics); every accumulator starts non-zero.
"""

import numpy as np
import pytest

from tests.hipemu import emu

U = 2.0 ** -24
# (M, D, drop_T): one live half-wave;  odd rows;  NP = 3 with [CLS] rows that carry no dy;  NP = 6, odd rows;  D = 384 and 16395 rows:
# both launches cap their grid at 2048 workgroups of 8 rows, so every workgroup walks a second set of rows and the last ones are ragged
SHAPES = [(1, 64, 0), (3, 128, 0), (10, 384, 5), (37, 768, 0), (16395, 384, 5)]
PRECISIONS = ["bf16", "fp32"]
_ids = lambda s: "x".join(map(str, s))  # noqa: E731


def _bf16_bits(a: np.ndarray) -> np.ndarray:
    """float32 -> bf16 bit patterns, round to nearest even (finite inputs)"""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def _bits_f32(b: np.ndarray) -> np.ndarray:
    return (b.astype(np.uint32) << 16).view(np.float32)


def _operand(a: np.ndarray, precision: str):
    """(the float32 values the kernel sees, the array handed to it)"""
    if precision == "fp32":
        return a, a
    bits = _bf16_bits(a)
    return _bits_f32(bits), bits


def _scales(rng, D):
    """away from 1 and of both signs: with ls = 1 a missing scale is invisible"""
    return (rng.uniform(0.2, 1.5, D) * rng.choice([-1.0, 1.0], D)).astype(np.float32)


def _rows_out(M, drop_T):
    return M - M // drop_T if drop_T else M


def _keep(M, drop_T):
    return np.arange(M) % drop_T != 0 if drop_T else np.ones(M, bool)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_forward_scales_then_adds_then_normalises(kernel_backend, shape, precision):
    M, D, drop_T = shape
    rng = np.random.default_rng(1)
    x = rng.standard_normal((M, D)).astype(np.float32)
    delta, delta_arg = _operand(rng.standard_normal((M, D)).astype(np.float32), precision)
    ls = _scales(rng, D)
    gamma = (1 + 0.3 * rng.standard_normal(D)).astype(np.float32)
    beta = (0.3 * rng.standard_normal(D)).astype(np.float32)
    eps = 1e-6
    out_dt = np.uint16 if precision == "bf16" else np.float32
    bx, bd, bl, bg, bb = emu.B(x), emu.B(delta_arg), emu.B(ls), emu.B(gamma), emu.B(beta)
    xo, y = emu.B(np.full((M, D), np.nan, np.float32)), emu.Z((_rows_out(M, drop_T), D), out_dt)
    mean, rstd = emu.B(np.full(M, np.nan, np.float32)), emu.B(np.full(M, np.nan, np.float32))
    name = "lp_layernorm_ls_fwd" if precision == "bf16" else "lp_f32_layernorm_ls_fwd"
    emu.ok(getattr(emu.lib(), name)(bx.p, bd.p, bl.p, xo.p, bg.p, bb.p, eps, M, D, drop_T, y.p, mean.p, rstd.p, emu.stream()))
    xo, y, mean, rstd = xo.np().copy(), y.np().copy(), mean.np().copy(), rstd.np().copy()

    prod = delta * ls[None, :]
    want = x + prod                                   # float32: two roundings, Dinov2LayerScale and then the residual add
    assert prod.dtype == want.dtype == np.float32
    assert np.array_equal(xo.view(np.uint32), want.view(np.uint32))
    fused = (x.astype(np.float64) + delta.astype(np.float64) * ls.astype(np.float64)[None, :]).astype(np.float32)   # (the product is exact in float64)
    if M * D >= 3840:
        assert not np.array_equal(fused, want)        # ... so the check above can fail: one fused multiply-add rounds differently somewhere

    x64 = xo.astype(np.float64)
    mu, var = x64.mean(1), x64.var(1)
    rs = 1.0 / np.sqrt(var + eps)
    # a sum of D float32 terms in any order is within D u sum|terms|; the variance is a sum of non-negative terms (relative error D u, its
    # inverse root half of that, plus the rounding of the root, the division and the store)
    err_mu, bound_mu = np.abs(mean - mu), D * U * np.abs(x64).mean(1)
    err_rs, bound_rs = np.abs(rstd - rs), (D / 2 + 4) * U * rs
    print(f"mean max err/bound {np.max(err_mu / bound_mu):.3g}, rstd max err/bound {np.max(err_rs / bound_rs):.3g}")
    assert np.all(err_mu <= bound_mu) and np.all(err_rs <= bound_rs)

    keep = _keep(M, drop_T)
    xh = ((x64 - mu[:, None]) * rs[:, None])[keep]
    want_y = xh * gamma.astype(np.float64) + beta.astype(np.float64)
    got_y = _bits_f32(y).astype(np.float64) if precision == "bf16" else y.astype(np.float64)
    # the float32 evaluation (the errors of mean and rstd above carried into xhat, four roundings) and, in the bf16 form, the one rounding of the store
    slack = (np.abs(gamma) * (rs[keep] * bound_mu[keep])[:, None] + ((D / 2 + 8) * U) * np.abs(xh * gamma) + 2 * U * np.abs(want_y))
    bound_y = slack + (2.0 ** -8 * np.abs(want_y) if precision == "bf16" else 0.0)
    err_y = np.abs(got_y - want_y)
    print(f"y max err/bound {np.max(err_y / bound_y):.3g}")
    assert np.all(err_y <= bound_y)


# colsum_acc = NULL (the A/B switch LP_VIT_BIAS_FUSED=0, and the attention branch, whose bias sums stay in the weight gradient) is another
# instantiation of the same walk: the shapes with NP = 3 and NP = 6 cover it
BWD_CASES = [(s, True) for s in SHAPES] + [((10, 384, 5), False), ((37, 768, 0), False)]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("shape,colsum", BWD_CASES, ids=lambda v: _ids(v) if isinstance(v, tuple) else ("colsum" if v else "nocolsum"))
def test_backward_scaled_gradient_and_the_four_sums(kernel_backend, shape, precision, colsum):
    M, D, drop_T = shape
    rng = np.random.default_rng(2)
    keep = _keep(M, drop_T)
    x = rng.standard_normal((M, D)).astype(np.float32)
    x64 = x.astype(np.float64)
    mean = x64.mean(1).astype(np.float32)
    rstd = (1.0 / np.sqrt(x64.var(1) + 1e-6)).astype(np.float32)
    dy, dy_arg = _operand(rng.standard_normal((_rows_out(M, drop_T), D)).astype(np.float32), precision)
    branch, branch_arg = _operand(rng.standard_normal((M, D)).astype(np.float32), precision)
    gamma = (1 + 0.3 * rng.standard_normal(D)).astype(np.float32)
    ls = _scales(rng, D)
    dx0 = (rng.standard_normal((M, D)) * np.exp(rng.standard_normal((M, 1)))).astype(np.float32)   # rows of mixed magnitude
    pre = {k: rng.standard_normal(D).astype(np.float32) for k in ("dgamma", "dbeta", "colsum", "dls")}  # accumulators start non-zero

    out_dt = np.uint16 if precision == "bf16" else np.float32
    b = {k: emu.B(v) for k, v in dict(dy=dy_arg, x=x, mean=mean, rstd=rstd, gamma=gamma, ls=ls, branch=branch_arg, dx=dx0, **pre).items()}
    out = emu.B(np.full((M, D), 0x7fc0 if precision == "bf16" else np.nan, out_dt))
    name = "lp_layernorm_ls_bwd" if precision == "bf16" else "lp_f32_layernorm_ls_bwd"
    emu.ok(getattr(emu.lib(), name)(b["dy"].p, b["x"].p, b["mean"].p, b["rstd"].p, b["gamma"].p, b["ls"].p, b["branch"].p, M, D, drop_T,
                                    b["dx"].p, out.p, b["dgamma"].p, b["dbeta"].p, b["colsum"].p if colsum else None, b["dls"].p, emu.stream()))
    got = {k: b[k].np().copy() for k in ("dx", "dgamma", "dbeta", "colsum", "dls")}
    emitted = out.np().copy()

    # ---- the float64 formula, from the operands the kernel was given
    mu, rs = mean.astype(np.float64)[:, None], rstd.astype(np.float64)[:, None]
    xh = (x64 - mu) * rs
    d64 = np.zeros((M, D))
    d64[keep] = dy                                  # [CLS] rows carry no dy
    g = d64 * gamma.astype(np.float64)
    s1, s2 = g.mean(1, keepdims=True), (g * xh).mean(1, keepdims=True)
    o64 = dx0.astype(np.float64) + rs * (g - s1 - xh * s2)
    # float32 evaluation: the two row means are sums of D terms (any order: D u mean|terms|), a handful of roundings on everything else
    bound_dx = 4 * U * (np.abs(dx0) + np.abs(o64)) + rs * (D + 8) * U * (np.abs(g) + np.abs(g).mean(1, keepdims=True)
                                                                          + np.abs(xh) * np.abs(g * xh).mean(1, keepdims=True))
    err_dx = np.abs(got["dx"] - o64)
    print(f"dx_acc max err/bound {np.max(err_dx / bound_dx):.3g}")
    assert np.all(err_dx <= bound_dx)
    if drop_T:
        assert np.array_equal(got["dx"][~keep].view(np.uint32), dx0[~keep].view(np.uint32))   # no dy: the stream gradient passes unchanged

    def check_sum(name, terms, term_roundings):
        """pre + sum_rows terms in any order: (rows + 1) u sum|terms|, plus the roundings inside each float32 term"""
        want = pre[name].astype(np.float64) + terms.sum(0)
        mag = np.abs(pre[name]) + np.abs(terms).sum(0)
        bound = (M + 1 + term_roundings) * U * mag
        err = np.abs(got[name] - want)
        print(f"{name} max err/bound {np.max(err / bound):.3g}")
        assert np.all(err <= bound), name

    check_sum("dgamma", d64 * xh, 4)       # (xhat is evaluated in float32: a difference, a product)
    check_sum("dbeta", d64, 0)

    # ---- what leaves through the scale, from the float32 stream gradient the kernel itself returned
    o = got["dx"]
    scaled = ls[None, :] * o
    assert scaled.dtype == np.float32
    if precision == "bf16":
        assert np.array_equal(emitted, _bf16_bits(scaled))
    else:
        assert np.array_equal(emitted.view(np.uint32), scaled.view(np.uint32))
    o_k = o.astype(np.float64)
    if colsum:
        check_sum("colsum", ls.astype(np.float64)[None, :] * o_k, 0)      # n u sum|terms|: the order-free bound, the start value one more term
    else:
        assert np.array_equal(got["colsum"], pre["colsum"])
    check_sum("dls", o_k * branch.astype(np.float64), 0)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_bad_arguments_return_the_documented_codes(kernel_backend, precision):
    lib = emu.lib()
    f32 = precision == "fp32"
    fwd = getattr(lib, "lp_f32_layernorm_ls_fwd" if f32 else "lp_layernorm_ls_fwd")
    bwd = getattr(lib, "lp_f32_layernorm_ls_bwd" if f32 else "lp_layernorm_ls_bwd")
    M, D = 2, 64
    z = emu.Z((M, D))
    v = emu.Z(D)
    r = emu.Z(M)
    st = emu.stream()
    ARG, UNSUPPORTED = -1, -2     # LP_ERR_ARGUMENT, LP_ERR_UNSUPPORTED (include/lp_hip.h)
    good_f = [z.p, z.p, v.p, z.p, v.p, v.p]
    assert fwd(*good_f, 1e-6, M, D, 0, z.p, r.p, r.p, st) == 0
    for i in range(6):            # x, delta, ls, x_out, gamma, beta: all required
        args = list(good_f)
        args[i] = None
        assert fwd(*args, 1e-6, M, D, 0, z.p, r.p, r.p, st) == ARG
    assert fwd(*good_f, 1e-6, 0, D, 0, z.p, r.p, r.p, st) == ARG
    good_b = [z.p, z.p, r.p, r.p, v.p, v.p, z.p]
    acc = [z.p, z.p, v.p, v.p, v.p, v.p]
    assert bwd(*good_b, M, D, 0, *acc, st) == 0
    for i in (5, 6):              # the scale and the branch output
        args = list(good_b)
        args[i] = None
        assert bwd(*args, M, D, 0, *acc, st) == ARG
    for i in (1, 5):              # the emitted gradient and the scale's gradient (the column sums alone are optional)
        a2 = list(acc)
        a2[i] = None
        assert bwd(*good_b, M, D, 0, *a2, st) == ARG
    if not f32:                   # the half-wave kernels cover D <= 1024, a multiple of 4
        big = emu.Z((1, 2048))
        assert fwd(big.p, big.p, big.p, big.p, big.p, big.p, 1e-6, 1, 2048, 0, big.p, r.p, r.p, st) == UNSUPPORTED
        assert fwd(*good_f, 1e-6, M, 62, 0, z.p, r.p, r.p, st) == UNSUPPORTED
        assert bwd(*good_b, M, 62, 0, *acc, st) == UNSUPPORTED
