"""The new arithmetic of the DINOv3 backbones at kernel level (include/lp_hip.h, csrc/rope.hip): the rotary position embedding on the fused
qkv rows (lp_rope_fwd / _bwd and their fp32 forms), the token assembly with register tokens (lp_vit_reg_tokens_*), and the prefix-dropping
forms of the LayerScale walks (lp_layernorm_ls_*_px).

The oracle of the rotation is the formula restated in numpy float64:  out[d] = x[d] cos[d] - x[d + 32] sin[d],
out[d + 32] = x[d + 32] cos[d] + x[d] sin[d]  (d < 32, rows t >= n_prefix, the Q and K blocks of every head).
bf16 forms: within one bf16 ulp of the float64 result rounded to bf16.  fp32 forms: at most 4 x the error of the same restatement evaluated in
float32 (the convention of tests/test_mv3d_kernels.py).  Everything the kernel must not touch is compared bit for bit."""

import math

import numpy as np
import pytest

from tests.hipemu import emu

U = 2.0 ** -24
ARG, UNSUPPORTED = -1, -2     # LP_ERR_ARGUMENT, LP_ERR_UNSUPPORTED (include/lp_hip.h)
# (B, nh, gh, gw, n_prefix, extra row pitch): a non-square grid and T = 17; six heads (not a power of two); one and no prefix row; a wider
# allocation.  Every shape is 576 lanes of work, 2.25 workgroups of 256: the last workgroup is partial
ROPE_SHAPES = [(3, 2, 3, 4, 5, 0), (2, 6, 2, 3, 5, 0), (3, 2, 3, 4, 1, 0), (3, 2, 3, 4, 0, 0), (3, 2, 3, 4, 5, 8)]
_ids = lambda s: "x".join(map(str, s))  # noqa: E731


def _bf16_bits(a):
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def _bits_f32(b):
    return (b.astype(np.uint32) << 16).view(np.float32)


def _table(gh, gw, n_tab, rng, theta=100.0):
    """(n_tab, gh * gw, 64) float32 cos[0:32] | sin[0:32]: the DINOv3 angles (y first, then x) of a grid whose coordinates are scaled
    differently per table, as the training-mode augmentation does"""
    inv = 1.0 / theta ** (np.arange(16) * 4 / 64)
    y = 2 * (np.arange(gh) + 0.5) / gh - 1
    x = 2 * (np.arange(gw) + 0.5) / gw - 1
    yy, xx = np.meshgrid(y, x, indexing="ij")
    tabs = []
    for i in range(n_tab):
        s = 1.0 if i == 0 else rng.uniform(0.5, 2.0)
        ang = 2 * math.pi * np.concatenate([(s * yy).reshape(-1, 1) * inv, (s * xx).reshape(-1, 1) * inv], 1)     # (Np, 32)
        tabs.append(np.concatenate([np.cos(ang), np.sin(ang)], 1))
    return np.stack(tabs).astype(np.float32)


def _rotate(x, table, seq, n_prefix, nh, k_off, bwd, dt):
    """the formula in dtype ``dt`` on a (B, T, ld) array; everything outside the rotated elements is copied"""
    out = x.astype(dt).copy()
    xs = x.astype(dt)
    for b in range(x.shape[0]):
        cos, sin = table[seq[b], :, :32].astype(dt), table[seq[b], :, 32:].astype(dt)
        if bwd:
            sin = -sin
        for base in [h * 64 for h in range(nh)] + [k_off + h * 64 for h in range(nh)]:
            lo, hi = xs[b, n_prefix:, base:base + 32], xs[b, n_prefix:, base + 32:base + 64]
            out[b, n_prefix:, base:base + 32] = lo * cos - hi * sin
            out[b, n_prefix:, base + 32:base + 64] = hi * cos + lo * sin
    return out


def _rotated_mask(B, T, ld, n_prefix, nh, k_off):
    m = np.zeros((B, T, ld), bool)
    m[:, n_prefix:, :nh * 64] = True
    m[:, n_prefix:, k_off:k_off + nh * 64] = True
    return m


def _setup(shape, precision, n_tab=1, seed=0):
    B, nh, gh, gw, n_prefix, extra = shape
    rng = np.random.default_rng(seed)
    D, Np = nh * 64, gh * gw
    T, ld = n_prefix + Np, 3 * D + extra
    x = rng.standard_normal((B, T, ld)).astype(np.float32)
    if precision == "bf16":
        bits = _bf16_bits(x)
        x, arg = _bits_f32(bits), bits
    else:
        arg = x
    table = _table(gh, gw, n_tab, rng)
    return B, nh, D, T, ld, n_prefix, x, arg, table


def _call(name, arg, ld, D, table, seq, B, T, n_prefix, nh, head_dim=64):
    buf, tab = emu.B(arg), emu.B(table)
    sq = emu.B(np.asarray(seq, np.int32)) if seq is not None else None
    rc = getattr(emu.lib(), name)(buf.p, ld, D, tab.p, emu.ptr(sq), table.shape[0], B, T, n_prefix, nh, head_dim, emu.stream())
    return rc, buf.np().copy()


def _name(precision, bwd):
    return ("lp_rope_" if precision == "bf16" else "lp_f32_rope_") + ("bwd" if bwd else "fwd")


@pytest.mark.parametrize("bwd", [False, True], ids=["fwd", "bwd"])
@pytest.mark.parametrize("shape", ROPE_SHAPES, ids=_ids)
def test_rope_bf16_within_one_ulp_and_nothing_else_touched(kernel_backend, shape, bwd):
    B, nh, D, T, ld, n_prefix, x, arg, table = _setup(shape, "bf16")
    seq = [0] * B
    rc, got = _call(_name("bf16", bwd), arg, ld, D, table, seq, B, T, n_prefix, nh)
    assert rc == 0
    want = _rotate(x, table, seq, n_prefix, nh, D, bwd, np.float64)
    m = _rotated_mask(B, T, ld, n_prefix, nh, D)
    assert np.array_equal(got[~m], arg[~m])                       # V columns, prefix rows, the bytes beyond 3 D: bit-identical
    want_r = _bits_f32(_bf16_bits(want.astype(np.float32)))[m].astype(np.float64)
    got_r = _bits_f32(got)[m].astype(np.float64)
    ulp = 2.0 ** (np.floor(np.log2(np.maximum(np.maximum(np.abs(want_r), np.abs(got_r)), 2.0 ** -126))) - 7)
    print(f"max |got - want| / ulp = {np.max(np.abs(got_r - want_r) / ulp):.3f}; {int(np.sum(got_r != want_r))} of {got_r.size} differ")
    assert np.all(np.abs(got_r - want_r) <= ulp)
    assert np.any(got[m] != arg[m])
    rc2, again = _call(_name("bf16", bwd), arg, ld, D, table, seq, B, T, n_prefix, nh)
    assert rc2 == 0 and np.array_equal(again, got)                # two runs: equal bits


@pytest.mark.parametrize("bwd", [False, True], ids=["fwd", "bwd"])
@pytest.mark.parametrize("shape", ROPE_SHAPES, ids=_ids)
def test_rope_fp32_within_four_times_the_float32_restatement(kernel_backend, shape, bwd):
    B, nh, D, T, ld, n_prefix, x, arg, table = _setup(shape, "fp32")
    seq = [0] * B
    rc, got = _call(_name("fp32", bwd), arg, ld, D, table, seq, B, T, n_prefix, nh)
    assert rc == 0
    want = _rotate(x, table, seq, n_prefix, nh, D, bwd, np.float64)
    own = _rotate(x, table, seq, n_prefix, nh, D, bwd, np.float32)
    m = _rotated_mask(B, T, ld, n_prefix, nh, D)
    assert np.array_equal(got[~m].view(np.uint32), arg[~m].view(np.uint32))
    err, bar = np.max(np.abs(got[m] - want[m])), np.max(np.abs(own[m] - want[m]))
    print(f"kernel max err {err:.3e}, float32 restatement max err {bar:.3e}")
    assert err <= 4 * bar
    rc2, again = _call(_name("fp32", bwd), arg, ld, D, table, seq, B, T, n_prefix, nh)
    assert rc2 == 0 and np.array_equal(again.view(np.uint32), got.view(np.uint32))


def test_rope_fp32_adjoint_and_inverse(kernel_backend):
    shape = ROPE_SHAPES[0]
    B, nh, D, T, ld, n_prefix, x, _, table = _setup(shape, "fp32", n_tab=2)
    seq = [0, 1, 0]
    g = np.random.default_rng(7).standard_normal(x.shape).astype(np.float32)
    m = _rotated_mask(B, T, ld, n_prefix, nh, D)
    fx = _call("lp_f32_rope_fwd", x, ld, D, table, seq, B, T, n_prefix, nh)[1]
    bg = _call("lp_f32_rope_bwd", g, ld, D, table, seq, B, T, n_prefix, nh)[1]
    fx32, bg32 = (_rotate(a, table, seq, n_prefix, nh, D, bw, np.float32) for a, bw in ((x, False), (g, True)))
    dot = lambda a, b: float(np.sum(a[m].astype(np.float64) * b[m].astype(np.float64)))  # noqa: E731
    gap, gap32 = abs(dot(fx, g) - dot(x, bg)), abs(dot(fx32, g) - dot(x, bg32))
    print(f"<fwd x, g> - <x, bwd g>: kernel {gap:.3e}, float32 restatement {gap32:.3e}, <fwd x, g> = {dot(fx, g):.6f}")
    assert gap <= 4 * gap32
    back = _call("lp_f32_rope_bwd", fx, ld, D, table, seq, B, T, n_prefix, nh)[1]
    back32 = _rotate(fx32, table, seq, n_prefix, nh, D, True, np.float32)
    err, bar = np.max(np.abs(back[m] - x[m])), np.max(np.abs(back32[m] - x[m]))
    print(f"bwd(fwd(x)) - x: kernel {err:.3e}, float32 restatement {bar:.3e}")
    assert err <= 4 * bar and bar < 1e-5                          # the rotation is orthogonal


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_rope_each_sequence_uses_its_own_table(kernel_backend, precision):
    B, nh, D, T, ld, n_prefix, x, arg, table = _setup(ROPE_SHAPES[0], precision, n_tab=2)
    seq = [0, 1, 0]
    got = _call(_name(precision, False), arg, ld, D, table, seq, B, T, n_prefix, nh)[1]
    for b in range(B):            # each sequence alone under its own table, through the same entry point with one table and no index array
        alone = _call(_name(precision, False), arg[b:b + 1], ld, D, table[seq[b]:seq[b] + 1], None, 1, T, n_prefix, nh)[1]
        assert np.array_equal(got[b], alone[0]), b
    other = _call(_name(precision, False), arg, ld, D, table, [0, 0, 0], B, T, n_prefix, nh)[1]
    assert np.array_equal(other[0], got[0]) and not np.array_equal(other[1], got[1])
    if precision == "fp32":
        want = _rotate(x, table, seq, n_prefix, nh, D, False, np.float64)
        own = _rotate(x, table, seq, n_prefix, nh, D, False, np.float32)
        assert np.max(np.abs(got - want)) <= 4 * np.max(np.abs(own - want))


def test_rope_more_lanes_than_one_grid_pass(kernel_backend):
    """the launch caps its grid at 4096 workgroups: 1 105 920 lanes of work walk the grid-stride loop a second time"""
    shape = (20, 12, 24, 24, 5, 0)
    B, nh, D, T, ld, n_prefix, x, arg, table = _setup(shape, "bf16")
    assert B * (T - n_prefix) * 2 * nh * 4 > 4096 * 256
    rc, got = _call("lp_rope_fwd", arg, ld, D, table, None, B, T, n_prefix, nh)
    assert rc == 0
    own = _bf16_bits(_rotate(x, table, [0] * B, n_prefix, nh, D, False, np.float32))
    m = _rotated_mask(B, T, ld, n_prefix, nh, D)
    assert np.array_equal(got[~m], arg[~m])
    # two products and one sum in float32, one rounding: the float32 restatement, bit for bit (NaN-free inputs)
    assert np.array_equal(got[m], own[m])


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_rope_argument_errors_leave_the_buffer_alone(kernel_backend, precision):
    B, nh, D, T, ld, n_prefix, x, arg, table = _setup(ROPE_SHAPES[0], precision)
    lib, st = emu.lib(), emu.stream()
    for name in (_name(precision, False), _name(precision, True)):
        fn = getattr(lib, name)
        buf, tab = emu.B(arg), emu.B(table)
        good = dict(q=buf.p, ld=ld, k=D, t=tab.p, s=None, n=1, B=B, T=T, p=n_prefix, nh=nh, hd=64)
        call = lambda **kw: fn(*{**good, **kw}.values(), st)  # noqa: E731
        assert call(q=None) == ARG and call(t=None) == ARG
        for kw in (dict(B=0), dict(T=0), dict(nh=0), dict(n=0), dict(ld=0), dict(p=-1), dict(p=T + 1), dict(k=D - 64), dict(k=2 * D + 64)):
            assert call(**kw) == ARG, kw
        assert call(hd=32) == UNSUPPORTED and call(hd=128) == UNSUPPORTED
        assert call(ld=ld + 1) == UNSUPPORTED and call(k=D + 1, ld=ld + 8) == UNSUPPORTED       # a pitch / offset off 16 bytes
        assert call(p=T) == 0                                                                  # no patch rows: nothing to do
        after = buf.np()
        assert np.array_equal(after.view(arg.dtype), arg)
        assert call() == 0 and not np.array_equal(buf.np(), arg)


# ---------------------------------------------------------------------------------------------------------------- token assembly
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("B,R,Np,D", [(3, 4, 12, 128), (2, 0, 6, 384), (37, 4, 6, 64)])
def test_reg_tokens_forward_and_backward(kernel_backend, precision, B, R, Np, D):
    rng = np.random.default_rng(3)
    T = 1 + R + Np
    patch = rng.standard_normal((B * Np, D)).astype(np.float32)
    if precision == "bf16":
        parg = _bf16_bits(patch)
        patch = _bits_f32(parg)
    else:
        parg = patch
    cls, reg = rng.standard_normal(D).astype(np.float32), rng.standard_normal((R, D)).astype(np.float32)
    pre = "lp_vit_reg_tokens_" if precision == "bf16" else "lp_f32_vit_reg_tokens_"
    lib, st = emu.lib(), emu.stream()
    bp, bc, br = emu.B(parg), emu.B(cls), emu.B(reg) if R else None
    x = emu.B(np.full((B, T, D), np.nan, np.float32))
    emu.ok(getattr(lib, pre + "fwd")(bp.p, bc.p, emu.ptr(br), B, R, Np, D, x.p, st))
    want = np.concatenate([np.broadcast_to(cls, (B, 1, D)), np.broadcast_to(reg, (B, R, D)), patch.reshape(B, Np, D)], 1)
    assert np.array_equal(x.np().view(np.uint32), want.view(np.uint32))          # copies and one widening: bit for bit

    dx = (rng.standard_normal((B, T, D)) * np.exp(rng.standard_normal((B, 1, 1)))).astype(np.float32)
    bdx = emu.B(dx)
    nan_patch = np.full((B * Np, D), 0x7fc0, np.uint16) if precision == "bf16" else np.full((B * Np, D), np.nan, np.float32)
    outs = []
    for _ in range(2):
        dp, dc = emu.B(nan_patch), emu.B(np.full(D, np.nan, np.float32))           # written, not accumulated: the outputs start as NaN
        dr = emu.B(np.full((R, D), np.nan, np.float32)) if R else None
        emu.ok(getattr(lib, pre + "bwd")(bdx.p, B, R, Np, D, dp.p, dc.p, emu.ptr(dr), st))
        outs.append((dp.np().copy(), dc.np().copy(), dr.np().copy() if R else np.zeros((0, D), np.float32)))
    dpatch, dcls, dreg = outs[0]
    rows = dx[:, 1 + R:].reshape(B * Np, D)
    if precision == "bf16":
        assert np.array_equal(dpatch, _bf16_bits(rows))
    else:
        assert np.array_equal(dpatch.view(np.uint32), rows.view(np.uint32))
    got = np.concatenate([dcls[None], dreg], 0)
    want64 = dx[:, :1 + R].astype(np.float64).sum(0)
    own = np.zeros((1 + R, D), np.float32)
    for b in range(B):            # the same sum in float32, images in ascending order
        own += dx[b, :1 + R]
    err, bar = np.max(np.abs(got - want64)), np.max(np.abs(own - want64))
    print(f"dcls / dreg: kernel max err {err:.3e}, float32 restatement {bar:.3e}")
    assert np.all(np.isfinite(got)) and err <= 4 * bar
    for a, b_ in zip(outs[0], outs[1]):
        assert np.array_equal(a.view(np.uint8), b_.view(np.uint8))               # repeatable bit for bit
    fwd, bwd = getattr(lib, pre + "fwd"), getattr(lib, pre + "bwd")
    assert fwd(None, bc.p, emu.ptr(br), B, R, Np, D, x.p, st) == ARG and fwd(bp.p, bc.p, emu.ptr(br), B, -1, Np, D, x.p, st) == ARG
    assert bwd(bdx.p, 0, R, Np, D, dp.p, dc.p, emu.ptr(dr), st) == ARG and fwd(bp.p, bc.p, emu.ptr(br), B, R, Np, 12, x.p, st) == UNSUPPORTED
    if R:
        assert fwd(bp.p, bc.p, None, B, R, Np, D, x.p, st) == ARG and bwd(bdx.p, B, R, Np, D, dp.p, dc.p, None, st) == ARG


# ---------------------------------------------------------------------------------------------------------------- LayerNorm, prefix dropped
def _ln_inputs(M, D, rows_out, precision, seed):
    rng = np.random.default_rng(seed)

    def operand(a):
        if precision == "fp32":
            return a, a
        bits = _bf16_bits(a)
        return _bits_f32(bits), bits

    d = dict(x=rng.standard_normal((M, D)).astype(np.float32))
    d["delta"], d["delta_arg"] = operand(rng.standard_normal((M, D)).astype(np.float32))
    d["branch"], d["branch_arg"] = operand(rng.standard_normal((M, D)).astype(np.float32))
    d["dy"], d["dy_arg"] = operand(rng.standard_normal((rows_out, D)).astype(np.float32))
    d["ls"] = (rng.uniform(0.2, 1.5, D) * rng.choice([-1.0, 1.0], D)).astype(np.float32)
    d["gamma"] = (1 + 0.3 * rng.standard_normal(D)).astype(np.float32)
    d["beta"] = (0.3 * rng.standard_normal(D)).astype(np.float32)
    x64 = d["x"].astype(np.float64)
    d["mean"] = x64.mean(1).astype(np.float32)
    d["rstd"] = (1.0 / np.sqrt(x64.var(1) + 1e-5)).astype(np.float32)
    d["dx0"] = (rng.standard_normal((M, D)) * np.exp(rng.standard_normal((M, 1)))).astype(np.float32)
    d["pre"] = {k: rng.standard_normal(D).astype(np.float32) for k in ("dgamma", "dbeta", "colsum", "dls")}
    return d


def _ln_fwd(d, M, D, drop_T, n_prefix, rows_out, precision, px):
    f32 = precision == "fp32"
    name = ("lp_f32_layernorm_ls_fwd" if f32 else "lp_layernorm_ls_fwd") + ("_px" if px else "")
    b = [emu.B(d[k]) for k in ("x", "delta_arg", "ls")]
    xo, y = emu.B(np.full((M, D), np.nan, np.float32)), emu.Z((rows_out, D), np.float32 if f32 else np.uint16)
    g, bt = emu.B(d["gamma"]), emu.B(d["beta"])
    mean, rstd = emu.B(np.full(M, np.nan, np.float32)), emu.B(np.full(M, np.nan, np.float32))
    extra = (n_prefix,) if px else ()
    emu.ok(getattr(emu.lib(), name)(b[0].p, b[1].p, b[2].p, xo.p, g.p, bt.p, 1e-5, M, D, drop_T, *extra, y.p, mean.p, rstd.p, emu.stream()))
    return dict(xo=xo.np().copy(), y=y.np().copy(), mean=mean.np().copy(), rstd=rstd.np().copy())


def _ln_bwd(d, M, D, drop_T, n_prefix, precision, px, colsum=True):
    f32 = precision == "fp32"
    name = ("lp_f32_layernorm_ls_bwd" if f32 else "lp_layernorm_ls_bwd") + ("_px" if px else "")
    b = {k: emu.B(v) for k, v in dict(dy=d["dy_arg"], x=d["x"], mean=d["mean"], rstd=d["rstd"], gamma=d["gamma"], ls=d["ls"],
                                      branch=d["branch_arg"], dx=d["dx0"], **d["pre"]).items()}
    out = emu.B(np.full((M, D), np.nan, np.float32) if f32 else np.full((M, D), 0x7fc0, np.uint16))
    extra = (n_prefix,) if px else ()
    emu.ok(getattr(emu.lib(), name)(b["dy"].p, b["x"].p, b["mean"].p, b["rstd"].p, b["gamma"].p, b["ls"].p, b["branch"].p, M, D, drop_T, *extra,
                                    b["dx"].p, out.p, b["dgamma"].p, b["dbeta"].p, b["colsum"].p if colsum else None, b["dls"].p, emu.stream()))
    return dict(emitted=out.np().copy(), **{k: b[k].np().copy() for k in ("dx", "dgamma", "dbeta", "colsum", "dls")})


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("M,D,drop_T", [(2, 128, 2), (8, 128, 4), (51, 384, 17)])
def test_px_forms_with_one_prefix_row_are_the_existing_forms(kernel_backend, precision, M, D, drop_T):
    """Every output that has ONE value is compared bit for bit at every shape.  d gamma / d beta / the column sums / dls are float atomics in
    both forms: their bits are defined only where the arrival order cannot matter, and are compared there - the bf16 walk with one workgroup
    (M <= 8: a fixed-order LDS sum, then the only atomic per column), and, for the fp32 walk (one atomic per row and column), two rows onto
    zeroed accumulators (0 + a + b = 0 + b + a).  With more workgroups those sums are held to float64 in the test below."""
    rows_out = M - M // drop_T
    d = _ln_inputs(M, D, rows_out, precision, 11)
    if M == 2:
        d["pre"] = {k: np.zeros(D, np.float32) for k in d["pre"]}
    a, b = _ln_fwd(d, M, D, drop_T, 1, rows_out, precision, True), _ln_fwd(d, M, D, drop_T, 1, rows_out, precision, False)
    for k in a:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
    a, b = _ln_bwd(d, M, D, drop_T, 1, precision, True), _ln_bwd(d, M, D, drop_T, 1, precision, False)
    for k in ("emitted", "dx"):
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
    if M == 2 or (M <= 8 and precision == "bf16"):
        for k in ("dgamma", "dbeta", "colsum", "dls"):
            assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("B,D", [(3, 128), (3, 384)])
def test_px_forms_drop_five_prefix_rows(kernel_backend, precision, B, D):
    """T = 17, n_prefix = 5 against float64, at the bars of tests/test_dinov2_layerscale_kernels.py for the same outputs"""
    T, n_prefix = 17, 5
    M, rows_out = B * T, B * (T - n_prefix)
    keep = np.arange(M) % T >= n_prefix
    d = _ln_inputs(M, D, rows_out, precision, 12)
    eps = 1e-5
    f = _ln_fwd(d, M, D, T, n_prefix, rows_out, precision, True)
    want_xo = d["x"] + d["delta"] * d["ls"][None, :]                       # float32: the product, then the sum
    assert np.array_equal(f["xo"].view(np.uint32), want_xo.view(np.uint32))
    x64 = f["xo"].astype(np.float64)
    mu, rs = x64.mean(1), 1.0 / np.sqrt(x64.var(1) + eps)
    bound_mu, bound_rs = D * U * np.abs(x64).mean(1), (D / 2 + 4) * U * rs
    assert np.all(np.abs(f["mean"] - mu) <= bound_mu) and np.all(np.abs(f["rstd"] - rs) <= bound_rs)
    xh = ((x64 - mu[:, None]) * rs[:, None])[keep]
    want_y = xh * d["gamma"].astype(np.float64) + d["beta"].astype(np.float64)
    assert f["y"].shape == (rows_out, D)                                    # exactly the B (T - 5) kept rows, in order
    got_y = _bits_f32(f["y"]).astype(np.float64) if precision == "bf16" else f["y"].astype(np.float64)
    slack = (np.abs(d["gamma"]) * (rs[keep] * bound_mu[keep])[:, None] + ((D / 2 + 8) * U) * np.abs(xh * d["gamma"]) + 2 * U * np.abs(want_y))
    bound_y = slack + (2.0 ** -8 * np.abs(want_y) if precision == "bf16" else 0.0)
    print(f"y max err/bound {np.max(np.abs(got_y - want_y) / bound_y):.3g}")
    assert np.all(np.abs(got_y - want_y) <= bound_y)

    for colsum in (True, False):
        g = _ln_bwd(d, M, D, T, n_prefix, precision, True, colsum=colsum)
        x64 = d["x"].astype(np.float64)
        mu, rs = d["mean"].astype(np.float64)[:, None], d["rstd"].astype(np.float64)[:, None]
        xh = (x64 - mu) * rs
        d64 = np.zeros((M, D))
        d64[keep] = d["dy"]                                                 # the prefix rows carry no dy
        gg = d64 * d["gamma"].astype(np.float64)
        s1, s2 = gg.mean(1, keepdims=True), (gg * xh).mean(1, keepdims=True)
        o64 = d["dx0"].astype(np.float64) + rs * (gg - s1 - xh * s2)
        bound_dx = 4 * U * (np.abs(d["dx0"]) + np.abs(o64)) + rs * (D + 8) * U * (np.abs(gg) + np.abs(gg).mean(1, keepdims=True)
                                                                                 + np.abs(xh) * np.abs(gg * xh).mean(1, keepdims=True))
        assert np.all(np.abs(g["dx"] - o64) <= bound_dx)
        assert np.array_equal(g["dx"][~keep].view(np.uint32), d["dx0"][~keep].view(np.uint32))   # no dy: the stream gradient passes unchanged

        def check_sum(name, terms, term_roundings):
            want = d["pre"][name].astype(np.float64) + terms.sum(0)
            mag = np.abs(d["pre"][name]) + np.abs(terms).sum(0)
            err = np.abs(g[name] - want)
            print(f"{name} max err/bound {np.max(err / ((M + 1 + term_roundings) * U * mag)):.3g}")
            assert np.all(err <= (M + 1 + term_roundings) * U * mag), name

        check_sum("dgamma", d64 * xh, 4)
        check_sum("dbeta", d64, 0)
        o = g["dx"]
        scaled = d["ls"][None, :] * o
        if precision == "bf16":
            assert np.array_equal(g["emitted"], _bf16_bits(scaled))
        else:
            assert np.array_equal(g["emitted"].view(np.uint32), scaled.view(np.uint32))
        o_k = o.astype(np.float64)
        if colsum:
            check_sum("colsum", d["ls"].astype(np.float64)[None, :] * o_k, 0)
        else:
            assert np.array_equal(g["colsum"], d["pre"]["colsum"])
        check_sum("dls", o_k * d["branch"].astype(np.float64), 0)
        # the dropped rows carry stream gradient into the sums: without them the scale's gradient misses its bound by far
        without = d["pre"]["dls"].astype(np.float64) + (o_k * d["branch"].astype(np.float64))[keep].sum(0)
        assert np.max(np.abs(g["dls"] - without)) > 1e-2


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_px_forms_argument_errors(kernel_backend, precision):
    f32 = precision == "fp32"
    lib, st = emu.lib(), emu.stream()
    fwd = getattr(lib, "lp_f32_layernorm_ls_fwd_px" if f32 else "lp_layernorm_ls_fwd_px")
    bwd = getattr(lib, "lp_f32_layernorm_ls_bwd_px" if f32 else "lp_layernorm_ls_bwd_px")
    M, D = 8, 64
    z, v, r = emu.Z((M, D)), emu.Z(D), emu.Z(M)
    assert fwd(z.p, z.p, v.p, z.p, v.p, v.p, 1e-5, M, D, 4, 2, z.p, r.p, r.p, st) == 0
    assert fwd(z.p, z.p, v.p, z.p, v.p, v.p, 1e-5, M, D, 4, 0, z.p, r.p, r.p, st) == 0          # nothing dropped
    assert fwd(z.p, z.p, v.p, z.p, v.p, v.p, 1e-5, M, D, 4, -1, z.p, r.p, r.p, st) == ARG
    assert fwd(z.p, z.p, v.p, z.p, v.p, v.p, 1e-5, M, D, 4, 5, z.p, r.p, r.p, st) == ARG
    good_b = [z.p, z.p, r.p, r.p, v.p, v.p, z.p]
    acc = [z.p, z.p, v.p, v.p, v.p, v.p]
    assert bwd(*good_b, M, D, 4, 2, *acc, st) == 0
    assert bwd(*good_b, M, D, 4, -1, *acc, st) == ARG and bwd(*good_b, M, D, 4, 5, *acc, st) == ARG


# ---------------------------------------------------------------------------------------------------------------- the host table (CPU only)
@pytest.mark.parametrize("gh,gw", [(3, 4), (16, 16), (24, 24)])
def test_host_table_is_bit_equal_to_the_hf_module(gh, gw, monkeypatch):
    torch = pytest.importorskip("torch")
    pytest.importorskip("transformers")
    from transformers import DINOv3ViTConfig
    from transformers.models.dinov3_vit.modeling_dinov3_vit import DINOv3ViTRopePositionEmbedding

    from lightning_pose_amd import _lib, ops
    from lightning_pose_amd.vit_engine import ViTEngine

    monkeypatch.setattr(_lib, "_lib", emu.emu_lib())
    monkeypatch.setattr(ops, "require_device_type", lambda d: None)
    monkeypatch.setattr(ops, "_stream", lambda: None)
    eng = ViTEngine(3, 2, "cpu", hidden=128, depth=1, heads=2, mlp=256, patch=16, arch="dinov3")
    cfg = DINOv3ViTConfig(hidden_size=128, num_hidden_layers=1, num_attention_heads=2, intermediate_size=256, num_register_tokens=4,
                          image_size=48, patch_size=16)
    cos, sin = DINOv3ViTRopePositionEmbedding(cfg).eval()(torch.zeros(1, 3, 16 * gh, 16 * gw))
    assert cos.shape == (gh * gw, 64) and torch.equal(cos[:, :32], cos[:, 32:]) and torch.equal(sin[:, :32], sin[:, 32:])
    table, _, n_tab, draws = eng._rope_tables(gh, gw, [2], False, None)
    assert n_tab == 1 and draws is None and table.shape == (1, gh * gw, 64) and table.dtype == torch.float32
    assert torch.equal(table[0, :, :32], cos[:, :32]) and torch.equal(table[0, :, 32:], sin[:, :32])
    assert eng._rope_tables(gh, gw, [5], False, None)[0] is table                # cached per grid
