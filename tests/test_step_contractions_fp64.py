"""Every convolution, GEMM and attention launch of a real training step, replayed on fresh operands and held against float64.

The kernels pick their launch plan from the problem size (split counts and rounds of the weight gradients, the HALO / res2d / ring forms,
the persistent tile walk), so the cases are not written by hand: a recording proxy around the kernel library captures every
lp_conv_* / lp_stem_* / lp_gemm_* / lp_attn_* call of one forward + backward pass - entry point, geometry, scalars, which optional
pointers were set, and lp_conv_last_kernel() after the call.  Each distinct case is then replayed with the same arguments on seeded bf16
operands (the plan is a function of geometry and device, so the replay reaches the plan the step used - asserted), and every output is
compared element by element with a float64 reference of the same bf16 operands (tests/fp64_ref.py):

    bf16 results (forward, data gradient, GEMM, attention O / dS)   |y - r| <= 2^-8 |r| + 2^-16 S      S = sum |a b| behind the element
    fp32 results (weight and bias gradients, attention row dots)    |y - r| <= 2^-18 S
    fused BatchNorm sums, per segment                                |s - r| <= 2^-16 sum |v|  (see SUMS_BAR)
    stored attention probabilities                                   |P - p| <= 2^-8 p + 2^-20, pad columns [T, ldp) exactly 0

Each case also builds mutant references from the same float64 code - a dropped 64-wide K step at the end and in the middle for the rows
of one output tile, a dropped 64-row block of M (end and middle) for the weight gradients, a 3x3 tap read one pixel across an image-row
end, a dropped last key / last query for attention - and asserts that the bar REJECTS each of them: a bar that cannot fail proves nothing.

The CPU suite runs the same capture -> replay -> fp64 -> mutant logic on the emulated kernel build at the small configurations of
tests/test_emu_engine.py / tests/test_emu_vit_engine.py; `-m gpu` adds the benchmark's configuration (ResNet-50, 64 labeled + 128
unlabeled images of 384 x 384 in two BatchNorm segments), a ragged one, and ViT-S/16 at 384 x 384 (T = 577 = 9 * 64 + 1 tokens)."""

from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass

import pytest
import torch

from lightning_pose_amd import _lib
from tests import fp64_ref as R

F64 = torch.float64
PREFIXES = ("lp_conv_", "lp_stem_", "lp_gemm_", "lp_attn_")
NOT_CASES = ("lp_conv_last_kernel", "lp_conv_wgrad_workspace_bytes")
# entry points that launch no convolution-family kernel: lp_conv_last_kernel() is not theirs after the call
NO_KERNEL_ID = ("lp_attn_fwd", "lp_attn_bwd_kv", "lp_attn_rowdot")
# Fused BatchNorm sums: the store passes add the STORED bf16 values (conv_pipe.h epilogue_fwd / rb_process: vr = bf16_to_f32(w[q])) into one
# fp32 partial per lane and channel, flushed (into the exact fixed-point totals) when the workgroup's column block or segment changes.  A chain
# of n fp32 additions of same-signed values errs by at most n/2 * 2^-24 of their |sum|; the bar 2^-16 sum |v| covers chains of 512 rows per
# lane, and the reference is summed from the kernel's own bf16 output, so nothing but that accumulation is measured.
SUMS_BAR = 2.0 ** -16
MARGINS: dict = {}     # entry point -> worst |y - r| / bar over its cases (printed with -s)


# ---------------------------------------------------------------------------------------------------------------- capture
@dataclass
class Case:
    name: str
    sig: tuple                      # per argument (stream and workspace sizes left out): ("p", set?), ("s", value) or (struct name, fields)
    alias: tuple                    # pairs of pointer arguments that were the same address
    kid: int
    n: int = 1                      # how often the step made this call
    rc: int = 0

    def key(self):
        return (self.name, self.sig, self.alias)


def _struct_fields(s) -> tuple:
    out = []
    for nm, _ in s._fields_:
        v = getattr(s, nm)
        if nm in ("z", "mean", "invstd", "gamma", "beta", "relu_bits", "sums"):
            v = bool(v)
        out.append((nm, v))
    return tuple(out)


class Recorder:
    """Forwards every attribute of the kernel library; the contraction entry points are wrapped to record their cases."""

    def __init__(self, lib):
        self._real = lib
        self.cases: dict = {}

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith(PREFIXES) or name in NOT_CASES:
            return fn
        argtypes = _lib.PROTOTYPES[name][1]

        def wrapped(*args):
            rc = fn(*args)
            sig, ptrs = [], {}
            for i, (t, a) in enumerate(zip(argtypes[:-1], args[:-1])):   # (the last argument is the stream)
                if t is C.c_size_t:
                    sig.append(("z", None))                                # workspace size: the replay asks the library
                elif t is C.c_void_p:
                    v = a.value if isinstance(a, C.c_void_p) else a
                    sig.append(("p", bool(v)))
                    if v:
                        ptrs.setdefault(v, []).append(i)
                elif hasattr(a, "_obj"):
                    sig.append((type(a._obj).__name__, _struct_fields(a._obj)))
                elif a is None:
                    sig.append((t.__name__, None))
                else:
                    sig.append(("s", a.value if hasattr(a, "value") else a))
            alias = tuple(tuple(v) for v in ptrs.values() if len(v) > 1)
            c = Case(name, tuple(sig), alias, int(self._real.lp_conv_last_kernel()) if name not in NO_KERNEL_ID else -1)
            c.rc = rc
            k = c.key()
            if k in self.cases:
                self.cases[k].n += 1
                assert name in NO_KERNEL_ID or self.cases[k].kid == c.kid, f"{name}: one geometry, two kernels ({self.cases[k].kid}, {c.kid})"
            else:
                self.cases[k] = c
            return rc
        return wrapped


def capture(monkeypatch, run) -> list[Case]:
    rec = Recorder(_lib.lib())
    monkeypatch.setattr(_lib, "_lib", rec)
    run()
    monkeypatch.setattr(_lib, "_lib", rec._real)
    return [c for c in rec.cases.values() if c.rc == 0]    # (an LP_ERR_UNSUPPORTED probe of a fused form is not a launch)


# ---------------------------------------------------------------------------------------------------------------- operands
class Ops:
    def __init__(self, dev, seed):
        self.dev = dev
        self.g = torch.Generator(device=dev if dev.type == "cuda" else "cpu").manual_seed(seed)

    def randn(self, *shape, scale=1.0, dtype=torch.bfloat16):
        return (torch.randn(*shape, generator=self.g, device=self.dev, dtype=torch.float32) * scale).to(dtype)

    def rand(self, *shape):
        return torch.rand(*shape, generator=self.g, device=self.dev, dtype=torch.float32)

    def bytes(self, n):
        return torch.randint(0, 256, (n,), generator=self.g, device=self.dev, dtype=torch.int32).to(torch.uint8)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    from lightning_pose_amd import ops
    return ops._stream()


def _sync(dev):
    if dev.type == "cuda":
        torch.cuda.synchronize()


def _args(case):
    return [v for _, v in case.sig]


def _geom(case) -> _lib.ConvGeom:
    for kind, v in case.sig:
        if kind == "ConvGeom":
            return _lib.ConvGeom(*[x for _, x in v])
    raise AssertionError(case.name)


def _bnf(case) -> dict | None:
    for kind, v in case.sig:
        if kind == "BnFuse":
            return dict(v)
    return None


class Result:
    """worst bar ratios of one case, per output, and the mutant ratios (must exceed 1)"""

    def __init__(self, case):
        self.case, self.ratio, self.mutants = case, {}, {}

    def check(self, what, y, r, bar):
        self.ratio[what] = max(self.ratio.get(what, 0.0), R.worst(y, r, bar))

    def mutant(self, what, y, r_m, bar_m):
        self.mutants[what] = R.worst(y, r_m, bar_m)


# ---------------------------------------------------------------------------------------------------------------- convolutions
def _kstep_mutants(res, what, A: R.ConvOperand, Wm, ep, y_of, M):
    """drop the last and a middle 64-wide K step (one tap, 64 channels) for the rows of the last and of a middle 128-row output tile"""
    taps = A.R * A.S
    nblk = (A.C + 63) // 64
    steps = [(taps - 1, nblk - 1), (taps // 2, nblk // 2)]
    tiles = [(max(0, M - 128), M), (M // 2 // 128 * 128, min(M, M // 2 // 128 * 128 + 128))]
    for (m0, m1), (tap, cb) in zip(tiles, steps):
        idx = A.kstep(tap, cb * 64)
        a = A.row_block(m0, m1)
        while not bool(a[:, idx].any()) and m0 >= 128:   # (a tap that reads only padding here: the nearest earlier tile it reaches)
            m0, m1 = m0 - 128, m1 - 128
            a = A.row_block(m0, m1)
        acc = a @ Wm.T
        s = a.abs() @ Wm.abs().T
        m = torch.arange(m0, m1, device=a.device)
        r_m = ep(acc - a[:, idx] @ Wm[:, idx].T, m)
        s = s[:, :r_m.shape[1]]
        res.mutant(f"{what}: K step (tap {tap}, channels {cb * 64}+) of rows {m0}..{m1}", y_of(m), r_m, R.bf16_bar(r_m, s))
    if A.R == A.S == 3:
        sh = A.tap_shift_rows(1, A.S - 1)
        assert sh is not None, "no row end to shift a tap across"
        m, orig, shifted = sh
        a = torch.cat([A.row_block(int(i), int(i) + 1) for i in m])
        idx = A.kstep(1 * A.S + A.S - 1, 0, A.C)
        acc = a @ Wm.T
        s = a.abs() @ Wm.abs().T
        r_m = ep(acc + (shifted - orig) @ Wm[:, idx].T, m)
        s = s[:, :r_m.shape[1]]
        res.mutant(f"{what}: tap (1, {A.S - 1}) read across the row end", y_of(m), r_m, R.bf16_bar(r_m, s))


def replay_conv_fwd(case, lib, ops, res):
    g = _geom(case)
    a = _args(case)
    name = case.name
    stem = name.startswith("lp_stem")
    bnf = _bnf(case)
    Cp = 4 if stem else g.Ci
    Cv = 3 if stem else g.Ci
    x = ops.randn(g.B, g.Hi, g.Wi, Cp)
    if stem:
        x[..., 3:] = 0
        w = torch.zeros(g.Co, 8, 8, 4, device=ops.dev, dtype=torch.bfloat16)
        w[:, :g.R, :g.S, :3] = ops.randn(g.Co, g.R, g.S, 3)
    else:
        w = ops.randn(g.Co, g.R, g.S, g.Ci)
    M, N = g.B * g.Ho * g.Wo, g.Co
    bias = out_f32 = None
    ldo, nst = N, N
    if name == "lp_conv_fwd":
        ldo, nst = a[6], (a[7] if a[7] > 0 else N)
        bias = ops.randn(N, dtype=torch.float32) if a[3] else None
        f32 = bool(a[5])
    else:
        f32 = False
    out = torch.zeros(M, ldo, device=ops.dev, dtype=torch.float32 if f32 else torch.bfloat16)
    sums = torch.zeros(4 * 2 * N, device=ops.dev, dtype=torch.int64) if bnf else None
    if bnf:
        f = _lib.BnFuse()
        f.sums, f.seg_images = sums.data_ptr(), bnf["seg_images"]
    st = _stream()
    if name == "lp_conv_fwd":
        rc = lib.lp_conv_fwd(_p(x), _p(w), C.byref(g), _p(bias), None if f32 else _p(out), _p(out) if f32 else None, ldo, a[7], st)
    elif name == "lp_conv_fwd_bn":
        rc = lib.lp_conv_fwd_bn(_p(x), _p(w), C.byref(g), _p(out), C.byref(f), st)
    elif name == "lp_stem_fwd":
        rc = lib.lp_stem_fwd(_p(x), _p(w), C.byref(g), _p(out), st)
    else:
        rc = lib.lp_stem_fwd_bn(_p(x), _p(w), C.byref(g), _p(out), C.byref(f), st)
    kid = int(lib.lp_conv_last_kernel())
    assert rc == 0, (name, rc)
    _sync(ops.dev)
    A = R.conv_fwd_operand(x, Cv, g.R, g.S, g.stride, g.pad)
    Wm = R.weight_matrix_fwd(w, g.R, g.S, Cv)
    assert (A.Ho, A.Wo) == (g.Ho, g.Wo)
    b64 = bias.to(F64) if bias is not None else None

    def ep(acc, m):
        r = acc if b64 is None else acc + b64
        return r[:, :nst]

    def y_of(m):
        return out[m, :nst]

    for m0, m1, arows in A.row_chunks():
        acc = arows @ Wm.T
        s = (arows.abs() @ Wm.abs().T)[:, :nst]
        r = ep(acc, None)
        res.check("out", out[m0:m1, :nst], r, R.bf16_bar(r, s))
    _kstep_mutants(res, "out", A, Wm, ep, y_of, M)
    if bnf:
        _check_sums(res, sums, out.to(F64), None, g.B, bnf["seg_images"], g.Ho * g.Wo)
    return kid


def _check_sums(res, sums, y, xhat_of, B, seg, rpi):
    """per BatchNorm segment: [sum y, sum y^2] (forward) or [sum y, sum y xhat] (backward) of the kernel's own bf16 output y"""
    nseg = 2 if seg else 1
    got = R.fx_value(sums)[:nseg * 2 * y.shape[1]].view(nseg, 2, -1)
    bounds = [(0, B)] if not seg else [(0, seg), (seg, B)]
    for si, (b0, b1) in enumerate(bounds):
        ys = y[b0 * rpi:b1 * rpi]
        second = ys * ys if xhat_of is None else ys * xhat_of(b0 * rpi, b1 * rpi, si)
        for comp, v in enumerate((ys, second)):
            res.check(f"BN sums seg {si}", got[si, comp], v.sum(0), SUMS_BAR * v.abs().sum(0) + 1e-30)


def replay_conv_dgrad(case, lib, ops, res):
    g = _geom(case)
    a = _args(case)
    name = case.name
    bnf = _bnf(case)
    M, N = g.B * g.Hi * g.Wi, g.Ci
    dy = ops.randn(g.B, g.Ho, g.Wo, g.Co)
    wd = ops.randn(g.Ci, g.R, g.S, g.Co)
    bias = addend = relu_mask = relu_bits = None
    skip, f32, ldo, nst = 0, False, N, N
    if name == "lp_conv_dgrad":
        bias = ops.randn(N, dtype=torch.float32) if a[3] else None
        has_add, has_mask, f32 = a[4], a[5], bool(a[7])
        ldo, nst, skip = a[8], (a[9] if a[9] > 0 else N), a[10]
    elif name == "lp_conv_dgrad_bits":
        has_add, has_mask, skip = a[3], False, a[6]
        relu_bits = ops.bytes(M * N // 8)
    else:
        has_add, has_mask = a[3], a[4]
        if bnf["relu_bits"]:
            relu_bits = ops.bytes(M * N // 8)
    half = bool(bnf and bnf["addend_half"])
    if has_add:
        addend = ops.randn(g.B, (g.Hi + 1) // 2, (g.Wi + 1) // 2, N) if half else ops.randn(g.B, g.Hi, g.Wi, N)
    if has_mask:
        relu_mask = ops.randn(g.B, g.Hi, g.Wi, N)
    aliased = any(set(p) == {4, 6} for p in case.alias) if name == "lp_conv_dgrad" else any(set(p) == {3, 5} for p in case.alias)
    out = torch.zeros(M, ldo, device=ops.dev, dtype=torch.float32 if f32 else torch.bfloat16)
    if aliased:
        out.view(-1)[:addend.numel()].copy_(addend.reshape(-1))
        addend_ptr = _p(out)
    else:
        addend_ptr = _p(addend)
    seg = bnf["seg_images"] if bnf else 0
    nseg = 2 if seg else 1
    st = _stream()
    if bnf:
        mean = ops.randn(nseg, N, scale=0.3, dtype=torch.float32)
        invstd = (0.5 + 1.5 * ops.rand(nseg, N)).float()
        gamma = ((0.5 + ops.rand(N)) * torch.where(ops.rand(N) < 0.2, -1.0, 1.0)).float()
        beta = ops.randn(N, scale=0.5, dtype=torch.float32)
        if bnf["mask_from_z"]:
            # z placed so that the recomputed mask bf16(gamma invstd (z - mean) + beta) is at least 0.05 away from its threshold: the
            # kernel's fp32 arithmetic and the fp64 reference then agree on every mask bit
            u = ops.randn(g.B, g.Hi * g.Wi, N, dtype=torch.float32)
            u = torch.where(u.abs() < 0.05, torch.copysign(torch.full_like(u, 0.05), u) + u, u)
            segrow = torch.zeros(g.B, 1, 1, dtype=torch.long, device=ops.dev)
            if seg:
                segrow[seg:] = 1
            mu, iv = mean[segrow.squeeze(-1)], invstd[segrow.squeeze(-1)]
            z = (mu + (u - beta) / (gamma * iv)).to(torch.bfloat16).view(g.B, g.Hi, g.Wi, N)
        else:
            z = ops.randn(g.B, g.Hi, g.Wi, N)
        sums = torch.zeros(4 * nseg * N, device=ops.dev, dtype=torch.int64)
        f = _lib.BnFuse()
        f.z, f.mean, f.invstd = z.data_ptr(), mean.data_ptr(), invstd.data_ptr()
        f.gamma, f.beta = (gamma.data_ptr() if bnf["gamma"] else None), (beta.data_ptr() if bnf["beta"] else None)
        f.mask_from_z, f.relu_bits = bnf["mask_from_z"], (relu_bits.data_ptr() if relu_bits is not None else None)
        f.sums, f.seg_images, f.addend_half = sums.data_ptr(), seg, bnf["addend_half"]
        rc = lib.lp_conv_dgrad_bn(_p(dy), _p(wd), C.byref(g), addend_ptr, _p(relu_mask), _p(out), C.byref(f), st)
    elif name == "lp_conv_dgrad_bits":
        rc = lib.lp_conv_dgrad_bits(_p(dy), _p(wd), C.byref(g), addend_ptr, _p(relu_bits), _p(out), skip, st)
    else:
        rc = lib.lp_conv_dgrad(_p(dy), _p(wd), C.byref(g), _p(bias), addend_ptr, _p(relu_mask), None if f32 else _p(out),
                               _p(out) if f32 else None, ldo, a[9], skip, st)
    kid = int(lib.lp_conv_last_kernel())
    assert rc == 0, (name, rc)
    _sync(ops.dev)
    A = R.conv_dgrad_operand(dy, g.Co, g.R, g.S, g.stride, g.pad, g.Hi, g.Wi)
    Wm = R.weight_matrix_dgrad(wd, g.R, g.S)
    assert (A.Ho, A.Wo) == (g.Hi, g.Wi), ((A.Ho, A.Wo), g.Hi, g.Wi)
    HWi = g.Hi * g.Wi
    b64 = bias.to(F64) if bias is not None else None
    add64 = addend.to(F64).reshape(-1, N) if addend is not None else None
    bits = None
    if relu_bits is not None:
        bits = ((relu_bits.view(-1, 1).long() >> torch.arange(8, device=ops.dev)) & 1).view(M, N).bool()
    maskz = None
    if bnf and bnf["mask_from_z"]:
        rows_seg = torch.zeros(M, dtype=torch.long, device=ops.dev)
        if seg:
            rows_seg[seg * HWi:] = 1
        t = gamma.to(F64) * invstd.to(F64)[rows_seg] * (z.to(F64).view(M, N) - mean.to(F64)[rows_seg]) + beta.to(F64)
        maskz = t > 0
    reached = None
    if skip and g.stride == 2:
        yy = torch.arange(g.Hi, device=ops.dev).view(-1, 1)
        xx = torch.arange(g.Wi, device=ops.dev).view(1, -1)
        reached = (((yy + g.pad) % 2 < g.R) & ((xx + g.pad) % 2 < g.S)).reshape(-1)

    def addend_rows(m):
        if add64 is None:
            return None
        if not half:
            return add64[m]
        b, rem = m // HWi, m % HWi
        yy, xx = rem // g.Wi, rem % g.Wi
        on = ((yy % 2) == 0) & ((xx % 2) == 0)
        hh, hw = (g.Hi + 1) // 2, (g.Wi + 1) // 2
        r = add64[((b * hh + yy // 2) * hw + xx // 2)]
        return r * on.view(-1, 1)

    def ep(acc, m):
        r = acc if b64 is None else acc + b64
        ad = addend_rows(m)
        if ad is not None:
            r = r + ad
        if relu_mask is not None:
            r = r * (relu_mask.view(M, N)[m] > 0)
        if bits is not None:
            r = r * bits[m]
        if maskz is not None:
            r = r * maskz[m]
        if reached is not None:
            keep = reached[m % HWi].view(-1, 1)
            r = torch.where(keep, r, add64[m])
        return r[:, :nst]

    def y_of(m):
        return out[m, :nst]

    for m0, m1, arows in A.row_chunks():
        m = torch.arange(m0, m1, device=ops.dev)
        acc = arows @ Wm.T
        s = (arows.abs() @ Wm.abs().T)[:, :nst]
        r = ep(acc, m)
        res.check("dx", out[m0:m1, :nst], r, R.bf16_bar(r, s))
    _kstep_mutants(res, "dx", A, Wm, ep, y_of, M)
    if bnf:
        z64, mean64, inv64 = z.to(F64).view(M, N), mean.to(F64), invstd.to(F64)

        def xhat_of(m0, m1, si):
            return (z64[m0:m1] - mean64[si]) * inv64[si]
        _check_sums(res, sums, out.to(F64), xhat_of, g.B, seg, HWi)
    return kid


def replay_conv_wgrad(case, lib, ops, res):
    g = _geom(case)
    name = case.name
    stem = name.startswith("lp_stem")
    Cp = 4 if stem else g.Ci
    Cv = 3 if stem else g.Ci
    x = ops.randn(g.B, g.Hi, g.Wi, Cp)
    if stem:
        x[..., 3:] = 0
    dy = ops.randn(g.B, g.Ho, g.Wo, g.Co)
    M = g.B * g.Ho * g.Wo
    dw = torch.zeros(g.Co, 8, 8, 4, device=ops.dev, dtype=torch.float32) if stem else \
        torch.zeros(g.Co, g.R, g.S, g.Ci, device=ops.dev, dtype=torch.float32)
    dbias = torch.zeros(g.Co, device=ops.dev, dtype=torch.float32) if name == "lp_conv_wgrad_bias" else None
    nws = int(lib.lp_conv_wgrad_workspace_bytes(C.byref(g), 0))
    ws = torch.empty(max(nws, 16), device=ops.dev, dtype=torch.uint8)
    st = _stream()
    if name == "lp_conv_wgrad_bias":
        rc = lib.lp_conv_wgrad_bias(_p(x), _p(dy), C.byref(g), _p(dw), _p(dbias), 0, _p(ws), ws.numel(), st)
    else:
        rc = getattr(lib, name)(_p(x), _p(dy), C.byref(g), _p(dw), 0, _p(ws), ws.numel(), st)
    kid = int(lib.lp_conv_last_kernel())
    assert rc == 0, (name, rc)
    _sync(ops.dev)
    A = R.conv_fwd_operand(x, Cv, g.R, g.S, g.stride, g.pad)
    assert (A.Ho, A.Wo) == (g.Ho, g.Wo)
    dy2 = dy.reshape(M, g.Co)
    ref = torch.zeros(g.Co, A.K, device=ops.dev, dtype=F64)
    S = torch.zeros_like(ref)
    for m0, m1, arows in A.row_chunks():
        d = dy2[m0:m1].to(F64)
        ref += d.T @ arows
        S += d.abs().T @ arows.abs()
    view = dw[:, :g.R, :g.S, :Cv].permute(0, 3, 1, 2).reshape(g.Co, -1)   # (Co, (c, r, s)) as unfold orders K
    res.check("dW", view, ref, R.f32_bar(S))
    if dbias is not None:
        bsum = dy2.to(F64).sum(0)
        bS = dy2.to(F64).abs().sum(0)
        res.check("dbias", dbias, bsum, R.f32_bar(bS))
    # mutants: the tail 64 pixel rows of M, and a 64-row block in the middle, left out
    for m0 in (M - 64, (M // 2) // 64 * 64):
        m1 = min(M, m0 + 64)
        arows = A.row_block(max(0, m0), m1)
        d = dy2[max(0, m0):m1].to(F64)
        r_m = ref - d.T @ arows
        res.mutant(f"dW without rows {m0}..{m1}", view, r_m, R.f32_bar(S))
    return kid


# ---------------------------------------------------------------------------------------------------------------- GEMMs
def _strided(flat, nb, nh, zb, zh, rows, cols, ld):
    return flat.as_strided((nb, nh, rows, cols), (zb, zh, ld, 1))


def _extent(nb, nh, zb, zh, rows, ld, cols):
    return (nb - 1) * zb + (nh - 1) * zh + (rows - 1) * ld + cols


def _gemm_mutants(res, what, a64, b64, y, ep, K, M):
    """drop the last and a middle 64-wide K step for the last and a middle 128-row tile (of the last batch entry)"""
    steps = [K - 64, (K // 64 // 2) * 64]
    tiles = [(max(0, M - 128), M), (M // 2 // 128 * 128, min(M, M // 2 // 128 * 128 + 128))]
    for (m0, m1), k0 in zip(tiles, steps):
        a, b = a64[m0:m1], b64
        acc = a @ b.T
        s = a.abs() @ b.abs().T
        r_m = ep(acc - a[:, k0:k0 + 64] @ b[:, k0:k0 + 64].T, m0, m1)
        res.mutant(f"{what}: K step {k0}+ of rows {m0}..{m1}", y[m0:m1], r_m, R.bf16_bar(r_m, s))


def replay_gemm_nt(case, lib, ops, res):
    a = _args(case)
    name = case.name
    st = _stream()
    if name == "lp_gemm_nt":
        lda, ldb, ldc, M, N, K, n_store = a[1], a[3], a[6], a[7], a[8], a[9], a[10]
        f32 = bool(a[5])
        gb = dict(a[12]) if a[12] is not None else dict(nb=1, nh=1, a_b=0, a_h=0, b_b=0, b_h=0, c_b=0, c_h=0)
        nb, nh = gb["nb"], gb["nh"]
        A = ops.randn(_extent(nb, nh, gb["a_b"], gb["a_h"], M, lda, K))
        Bm = ops.randn(_extent(nb, nh, gb["b_b"], gb["b_h"], N, ldb, K))
        Cb = torch.zeros(_extent(nb, nh, gb["c_b"], gb["c_h"], M, ldc, ldc), device=ops.dev, dtype=torch.float32 if f32 else torch.bfloat16)
        bias = ops.randn(N, dtype=torch.float32) if a[11] else None
        gbs = _lib.GemmBatch(nb, nh, gb["a_b"], gb["a_h"], gb["b_b"], gb["b_h"], gb["c_b"], gb["c_h"]) if a[12] is not None else None
        rc = lib.lp_gemm_nt(_p(A), lda, _p(Bm), ldb, None if f32 else _p(Cb), _p(Cb) if f32 else None, ldc, M, N, K, n_store, _p(bias),
                            C.byref(gbs) if gbs is not None else None, st)
        Av = _strided(A, nb, nh, gb["a_b"], gb["a_h"], M, K, lda)
        Bv = _strided(Bm, nb, nh, gb["b_b"], gb["b_h"], N, K, ldb)
        Cv = _strided(Cb, nb, nh, gb["c_b"], gb["c_h"], M, N, ldc)
        outs = [(Cv, bias, None)]
    else:
        M, N, K = a[5:8] if name == "lp_gemm_nt_gelu_fwd" else a[4:7]
        nb = nh = 1
        A = ops.randn(M, K)
        Bm = ops.randn(N, K)
        c = torch.zeros(M, N, device=ops.dev, dtype=torch.bfloat16)
        Av, Bv = A.view(1, 1, M, K), Bm.view(1, 1, N, K)
        if name == "lp_gemm_nt_gelu_fwd":
            bias = ops.randn(N, dtype=torch.float32) if a[2] else None
            act = torch.zeros_like(c)
            rc = lib.lp_gemm_nt_gelu_fwd(_p(A), _p(Bm), _p(bias), _p(c), _p(act), M, N, K, st)
            outs = [(c.view(1, 1, M, N), bias, None)]
        else:
            u = ops.randn(M, N, scale=1.5)
            colsum = torch.zeros(4 * N, device=ops.dev, dtype=torch.int64) if a[7] else None
            rc = lib.lp_gemm_nt_gelu_bwd(_p(A), _p(Bm), _p(u), _p(c), M, N, K, _p(colsum), st)
            outs = [(c.view(1, 1, M, N), None, R.gelu_grad(u.to(F64)))]
    kid = int(lib.lp_conv_last_kernel())
    assert rc == 0, (name, rc)
    _sync(ops.dev)
    Cv, bias, gscale = outs[0]
    # lp_gemm_nt_gelu_bwd rounds TWICE by its contract - the product to bf16 (what lp_gemm_nt would have stored), then the product with
    # GELU'(u) - and each rounding may cost half an ulp, up to 2^-8 of the value: its bar is 2^-7 |r| + 2^-16 S
    # GELU'(u) itself comes from an fp32 erf / exp evaluation, within 2^-22 absolute: that term is 2^-22 |a b^T| <= 2^-22 S
    bar = R.bf16_bar if gscale is None else (lambda r, s: 2.0 ** -7 * r.abs() + 2.0 ** -16 * s)
    b64 = bias.to(F64) if bias is not None else None
    for zb in range(nb):
        for zh in range(nh):
            a64, bb = Av[zb, zh].to(F64), Bv[zb, zh].to(F64)
            y = Cv[zb, zh]

            def ep(acc, m0, m1):
                r = acc if b64 is None else acc + b64
                return r if gscale is None else r * gscale[m0:m1]

            for m0 in range(0, M, 8192):
                m1 = min(M, m0 + 8192)
                acc = a64[m0:m1] @ bb.T
                s = a64[m0:m1].abs() @ bb.abs().T
                if gscale is not None:
                    s = s * (gscale[m0:m1].abs() + 2.0 ** -6)
                r = ep(acc, m0, m1)
                res.check("C", y[m0:m1], r, bar(r, s))
            if zb == nb - 1 and zh == nh - 1:
                def ep_m(acc, m0, m1):
                    return ep(acc, m0, m1)
                if gscale is None:
                    _gemm_mutants(res, "C", a64, bb, y, ep_m, K, M)
                else:
                    gs = gscale

                    def ep_g(acc, m0, m1):
                        return acc * gs[m0:m1]
                    steps = [K - 64, (K // 64 // 2) * 64]
                    for m0, k0 in zip((max(0, M - 128), M // 2 // 128 * 128), steps):
                        m1 = min(M, m0 + 128)
                        aa = a64[m0:m1]
                        s = (aa.abs() @ bb.abs().T) * (gs[m0:m1].abs() + 2.0 ** -6)
                        r_m = ep_g(aa @ bb.T - aa[:, k0:k0 + 64] @ bb[:, k0:k0 + 64].T, m0, m1)
                        res.mutant(f"C: K step {k0}+ of rows {m0}..{m1}", y[m0:m1], r_m, bar(r_m, s))
    if name == "lp_gemm_nt_gelu_fwd":
        cv = c.to(F64)
        # (a pointwise function of the stored C: its rounding, plus 2^-16 |C| for the fp32 erf near GELU's zero)
        res.check("GELU(C)", act, R.gelu(cv), 2.0 ** -8 * R.gelu(cv).abs() + 2.0 ** -16 * cv.abs() + 2.0 ** -133)
    if name == "lp_gemm_nt_gelu_bwd" and colsum is not None:
        cv = c.to(F64)
        got = R.fx_value(colsum)[:N]
        res.check("column sums", got, cv.sum(0), SUMS_BAR * cv.abs().sum(0) + 1e-30)
    return kid


def replay_gemm_tn(case, lib, ops, res):
    a = _args(case)
    ldx, ldy, ldo, M, J, N = a[1], a[3], a[5], a[6], a[7], a[8]
    gb = dict(a[9])
    nb, nh = gb["nb"], gb["nh"]
    X = ops.randn(_extent(nb, nh, gb["a_b"], gb["a_h"], M, ldx, J))
    Y = ops.randn(_extent(nb, nh, gb["b_b"], gb["b_h"], M, ldy, N))
    O = torch.zeros(_extent(nb, nh, gb["c_b"], gb["c_h"], J, ldo, ldo), device=ops.dev, dtype=torch.bfloat16)
    gbs = _lib.GemmBatch(nb, nh, gb["a_b"], gb["a_h"], gb["b_b"], gb["b_h"], gb["c_b"], gb["c_h"])
    rc = lib.lp_gemm_tn(_p(X), ldx, _p(Y), ldy, _p(O), ldo, M, J, N, C.byref(gbs), _stream())
    kid = int(lib.lp_conv_last_kernel())
    assert rc == 0
    _sync(ops.dev)
    Xv = _strided(X, nb, nh, gb["a_b"], gb["a_h"], M, J, ldx)
    Yv = _strided(Y, nb, nh, gb["b_b"], gb["b_h"], M, N, ldy)
    Ov = _strided(O, nb, nh, gb["c_b"], gb["c_h"], J, N, ldo)
    for zb in range(nb):
        for zh in range(nh):
            x64, y64 = Xv[zb, zh].to(F64), Yv[zb, zh].to(F64)
            r = x64.T @ y64
            s = x64.abs().T @ y64.abs()
            res.check("out", Ov[zb, zh], r, R.bf16_bar(r, s))
    m0 = M - 64
    r_m = r - x64[m0:].T @ y64[m0:]
    res.mutant(f"out without rows {m0}..{M}", Ov[nb - 1, nh - 1], r_m, R.bf16_bar(r_m, s))
    return kid


# ---------------------------------------------------------------------------------------------------------------- attention
def _softmax64(q, k, scale, drop_last=False):
    s = (q @ k.transpose(-1, -2)) * scale
    if drop_last:
        s[..., -1] = -math.inf
    return torch.softmax(s, dim=-1)


def replay_attn_fwd(case, lib, ops, res):
    a = _args(case)
    ld, k_off, v_off, B, nh, T, scale, ldp, ldo = a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[9], a[11]
    qkv = ops.randn(B * T, ld)
    # key T - 1 (the one valid row of the last key tile) carries a visible share of the mass for every query: its key is the mean query
    # direction, scaled
    q3 = qkv.view(B, T, ld)
    for h in range(nh):
        qm = q3[:, :, h * 64:(h + 1) * 64].float().mean(1)
        q3[:, T - 1, k_off + h * 64:k_off + (h + 1) * 64] = (qm / qm.norm(dim=-1, keepdim=True) * 16).to(torch.bfloat16)
    P = torch.full((B * nh * T, ldp), 7.0, device=ops.dev, dtype=torch.bfloat16) if a[8] else None
    out = torch.zeros(B * T, ldo, device=ops.dev, dtype=torch.bfloat16)
    rc = lib.lp_attn_fwd(_p(qkv), ld, k_off, v_off, B, nh, T, scale, _p(P), ldp, _p(out), ldo, _stream())
    assert rc == 0
    _sync(ops.dev)
    x = qkv.view(B, T, ld)
    for b in range(B):
        for h in range(nh):
            q = x[b, :, h * 64:(h + 1) * 64].to(F64)
            k = x[b, :, k_off + h * 64:k_off + (h + 1) * 64].to(F64)
            v = x[b, :, v_off + h * 64:v_off + (h + 1) * 64].to(F64)
            p = _softmax64(q, k, scale)
            o = out.view(B, T, ldo)[b, :, h * 64:(h + 1) * 64]
            if P is None:
                r, s = p @ v, p @ v.abs()
                res.check("O", o, r, R.bf16_bar(r, s) + 2.0 ** -9 * s)   # (P rounded to bf16 before the product, up to 2^-9 of each term)
                continue
            Pz = P.view(B, nh, T, ldp)[b, h]
            res.check("P", Pz[:, :T], p, 2.0 ** -8 * p + 2.0 ** -20)
            assert bool((Pz[:, T:] == 0).all()), "pad columns of P not zeroed"
            Pk = Pz[:, :T].to(F64)                    # O = P V with the stored (bf16) probabilities
            r, s = Pk @ v, Pk @ v.abs()
            res.check("O", o, r, R.bf16_bar(r, s))
            if b == B - 1 and h == nh - 1:
                pm = _softmax64(q, k, scale, drop_last=True)
                res.mutant("P without key T-1", Pz[:, :T], pm, 2.0 ** -8 * pm + 2.0 ** -20)
                r_m = Pk[:-1] @ v
                res.mutant("O without query row T-1", o[:-1], torch.cat([r_m[:-1], torch.zeros_like(r_m[:1])]),
                           R.bf16_bar(r_m, s[:-1]))
    return -1


def replay_attn_bwd_kv(case, lib, ops, res):
    a = _args(case)
    ld, v_off, ld_do, ldp, B, nh, T, scale, ld_dqkv, dk_off, dv_off = a[1], a[2], a[4], a[6], a[8], a[9], a[10], a[11], a[14], a[15], a[16]
    qkv = ops.randn(B * T, ld)
    dO = ops.randn(B * T, ld_do)
    # P: soft-max rows of random scores (spread as the step's are), pad columns zero
    P = torch.zeros(B * nh * T, ldp, device=ops.dev, dtype=torch.bfloat16)
    P.view(B * nh, T, ldp)[:, :, :T] = torch.softmax(ops.randn(B * nh, T, T, scale=2.0, dtype=torch.float32), -1).to(torch.bfloat16)
    Pv = P.view(B, nh, T, ldp)
    x, dov = qkv.view(B, T, ld), dO.view(B, T, ld_do)
    D = torch.zeros(B * T, nh, device=ops.dev, dtype=torch.float32)
    for b in range(B):
        for h in range(nh):
            dp = dov[b, :, h * 64:(h + 1) * 64].to(F64) @ x[b, :, v_off + h * 64:v_off + (h + 1) * 64].to(F64).T
            D.view(B, T, nh)[b, :, h] = (Pv[b, h, :, :T].to(F64) * dp).sum(-1).float()
    dS = torch.full((B * nh * T, ldp), 7.0, device=ops.dev, dtype=torch.bfloat16)
    dqkv = torch.zeros(B * T, ld_dqkv, device=ops.dev, dtype=torch.bfloat16)
    rc = lib.lp_attn_bwd_kv(_p(qkv), ld, v_off, _p(dO), ld_do, _p(P), ldp, _p(D), B, nh, T, scale, _p(dS), _p(dqkv), ld_dqkv, dk_off, dv_off,
                            _stream())
    assert rc == 0
    _sync(ops.dev)
    dq3, dS4 = dqkv.view(B, T, ld_dqkv), dS.view(B, nh, T, ldp)
    for b in range(B):
        for h in range(nh):
            q = x[b, :, h * 64:(h + 1) * 64].to(F64)
            v = x[b, :, v_off + h * 64:v_off + (h + 1) * 64].to(F64)
            do = dov[b, :, h * 64:(h + 1) * 64].to(F64)
            p = Pv[b, h, :, :T].to(F64)
            d = D.view(B, T, nh)[b, :, h].to(F64).view(-1, 1)
            r = scale * p * (do @ v.T - d)
            s = scale * p * (do.abs() @ v.abs().T + d.abs())
            res.check("dS", dS4[b, h, :, :T], r, R.bf16_bar(r, s))
            assert bool((dS4[b, h, :, T:] == 0).all()), "pad columns of dS not zeroed"
            dv, dvr, dvs = dq3[b, :, dv_off + h * 64:dv_off + (h + 1) * 64], p.T @ do, p.T @ do.abs()
            res.check("dV", dv, dvr, R.bf16_bar(dvr, dvs))
            dsk = dS4[b, h, :, :T].to(F64)         # dK = dS^T Q with the stored (bf16) score gradient
            dk, dkr, dks = dq3[b, :, dk_off + h * 64:dk_off + (h + 1) * 64], dsk.T @ q, dsk.abs().T @ q.abs()
            res.check("dK", dk, dkr, R.bf16_bar(dkr, dks))
            if b == B - 1 and h == nh - 1:
                for nm, y, rr, ss, lhs, rhs in (("dV", dv, dvr, dvs, p, do), ("dK", dk, dkr, dks, dsk, q)):
                    r_m = rr - lhs[-1:].T @ rhs[-1:]
                    res.mutant(f"{nm} without query row T-1", y, r_m, R.bf16_bar(r_m, ss))
    return -1


def replay_attn_rowdot(case, lib, ops, res):
    a = _args(case)
    rows, nh, ld = a[2], a[3], a[4]
    A = ops.randn(rows, ld)
    Bm = ops.randn(rows, ld)
    out = torch.zeros(rows, nh, device=ops.dev, dtype=torch.float32)
    rc = lib.lp_attn_rowdot(_p(A), _p(Bm), rows, nh, ld, _p(out), _stream())
    assert rc == 0
    _sync(ops.dev)
    pr = (A.to(F64) * Bm.to(F64))[:, :nh * 64].view(rows, nh, 64)
    r, s = pr.sum(-1), pr.abs().sum(-1)
    res.check("D", out, r, R.f32_bar(s))
    r_m = r - pr[..., 32:].sum(-1)
    res.mutant("D without products 32..63", out, r_m, R.f32_bar(s))
    return -1


REPLAY = {
    "lp_conv_fwd": replay_conv_fwd, "lp_conv_fwd_bn": replay_conv_fwd, "lp_stem_fwd": replay_conv_fwd, "lp_stem_fwd_bn": replay_conv_fwd,
    "lp_conv_dgrad": replay_conv_dgrad, "lp_conv_dgrad_bits": replay_conv_dgrad, "lp_conv_dgrad_bn": replay_conv_dgrad,
    "lp_conv_wgrad": replay_conv_wgrad, "lp_conv_wgrad_bias": replay_conv_wgrad, "lp_stem_wgrad": replay_conv_wgrad,
    "lp_gemm_nt": replay_gemm_nt, "lp_gemm_nt_gelu_fwd": replay_gemm_nt, "lp_gemm_nt_gelu_bwd": replay_gemm_nt,
    "lp_gemm_tn": replay_gemm_tn,
    "lp_attn_fwd": replay_attn_fwd, "lp_attn_bwd_kv": replay_attn_bwd_kv, "lp_attn_rowdot": replay_attn_rowdot,
}


def replay_all(cases: list[Case], dev, label: str) -> None:
    """replay every case, check bars, kernel ids and mutants; print the worst ratio per entry point"""
    lib = _lib.lib()
    missing = sorted({c.name for c in cases} - set(REPLAY))
    assert not missing, f"captured entry points without an fp64 replay: {missing}"
    failures, step_kids, replay_kids = [], set(), set()
    worst_by_name: dict = {}
    for i, c in enumerate(cases):
        res = Result(c)
        kid = REPLAY[c.name](c, lib, Ops(dev, 1000 + i), res)
        if c.name not in NO_KERNEL_ID:
            step_kids.add(c.kid)
            replay_kids.add(kid)
            if kid != c.kid:
                failures.append(f"{c.name} {dict(c.sig[2][1]) if c.sig[2][0] == 'ConvGeom' else c.sig}: step ran kernel {c.kid}, replay {kid}")
        for what, v in res.ratio.items():
            if not v <= 1.0:
                failures.append(f"{c.name} {_describe(c)} {what}: |y - r| / bar = {v:.3g}")
            k = f"{c.name} {what}"
            worst_by_name[k] = max(worst_by_name.get(k, 0.0), v)
        assert res.mutants, f"{c.name}: no mutant built"
        for what, v in res.mutants.items():
            if not v > 1.0:
                failures.append(f"{c.name} {_describe(c)}: mutant '{what}' PASSES the bar (ratio {v:.3g}) - the inputs are too weak")
    assert step_kids == replay_kids, (step_kids, replay_kids)
    MARGINS[label] = worst_by_name
    names = {}
    for c in cases:
        names[c.name] = names.get(c.name, 0) + 1
    print(f"\nMARGINS {label}: {len(cases)} distinct cases {names}, kernel ids {sorted(step_kids)}")
    for k, v in sorted(worst_by_name.items()):
        print(f"  {k}: worst |y - r| / bar {v:.3g}")
    assert not failures, "\n".join(failures[:40])


def _describe(c: Case) -> str:
    for kind, v in c.sig:
        if kind == "ConvGeom":
            return "geom(" + ",".join(str(x) for _, x in v) + ")"
    return str([v for k, v in c.sig if k == "s"])


# ---------------------------------------------------------------------------------------------------------------- the steps
def _resnet_engine_step(dev, B, HW, joint=None):
    from lightning_pose_amd.engine import Engine
    from lightning_pose_amd.models.backbones._init import seeded_state_dict

    K = 3
    torch.manual_seed(7)
    eng = Engine(K, 2, dev)
    eng.load_state_dict(seeded_state_dict(K, 2), strict=False)
    gen = torch.Generator().manual_seed(0)
    H, W = HW
    images = torch.randn(B, 3, H, W, generator=gen)
    x = images.to(dev) if joint is None else [images[:joint].to(dev), images[joint:].to(dev)]
    heat, tape = eng.forward(x, True)
    eng.zero_grad()
    eng.backward(tape, torch.randn(heat.shape, generator=gen).to(dev))
    _sync(dev)


def _vit_engine_step(dev, hidden, depth, heads, mlp, B, size):
    from lightning_pose_amd.vit_engine import ViTEngine

    torch.manual_seed(0)
    eng = ViTEngine(5, 2, dev, hidden=hidden, depth=depth, heads=heads, mlp=mlp, patch=16, pretrain_grid=3)
    gen = torch.Generator().manual_seed(1)
    for p in (eng.P,):
        p.copy_((torch.randn(p.shape, generator=gen) * 0.02).to(dev))
    eng.refresh_dgrad_copies() if hasattr(eng, "refresh_dgrad_copies") else None
    heat, tape = eng.forward(torch.randn(B, 3, size, size, generator=gen).to(dev), True)
    eng.zero_grad()
    eng.backward(tape, torch.randn(heat.shape, generator=gen).to(dev))
    _sync(dev)


def _bench_step(dev, backbone, size, n_lab, n_unlab):
    import bench

    model = bench.build_model(dev, 17, size, backbone=backbone)
    batch = bench.synth_batch(dev, 0, size, n_lab, n_unlab, 17)
    model.train()
    loss = model.training_step(batch, 0)["loss"]
    loss.backward()
    _sync(dev)


@pytest.mark.parametrize("cfg", ["single", "joint"])
def test_resnet_step_contractions_vs_fp64_small(stack_backend, monkeypatch, cfg):
    """tests/test_emu_engine.py's configurations: 4 images of 64 x 64, and 8 | 8 images of 128 x 128 in two BatchNorm segments"""
    dev = stack_backend
    if cfg == "single":
        cases = capture(monkeypatch, lambda: _resnet_engine_step(dev, 4, (64, 64)))
    else:
        cases = capture(monkeypatch, lambda: _resnet_engine_step(dev, 16, (128, 128), joint=8))
    replay_all(cases, dev, f"resnet50 {cfg} ({dev.type})")


def test_vit_step_contractions_vs_fp64_small(stack_backend, monkeypatch):
    """tests/test_emu_vit_engine.py's configuration: width 128, 2 layers, 2 heads, 2 images of 64 x 64 (T = 17)"""
    dev = stack_backend
    cases = capture(monkeypatch, lambda: _vit_engine_step(dev, 128, 2, 2, 256, 2, 64))
    replay_all(cases, dev, f"vit small ({dev.type})")


@pytest.mark.gpu
def test_resnet_benchmark_step_contractions_vs_fp64(monkeypatch):
    """the benchmark step: ResNet-50 at 384 x 384, 64 labeled + 128 unlabeled images in two BatchNorm segments (M up to 1.77 M rows)"""
    dev = torch.device("cuda:0")
    cases = capture(monkeypatch, lambda: _bench_step(dev, "resnet50", 384, 64, 128))
    torch.cuda.empty_cache()
    replay_all(cases, dev, "resnet50 384 64|128")


@pytest.mark.gpu
def test_resnet_ragged_step_contractions_vs_fp64(monkeypatch):
    """row counts that are not multiples of 64 or 256 at production channel counts: 3 labeled + 5 unlabeled images of 160 x 160 (5 x 5
    trunk pixels per image: the joint pass cannot keep its segments in one launch and runs them as two)"""
    dev = torch.device("cuda:0")
    cases = capture(monkeypatch, lambda: _bench_step(dev, "resnet50", 160, 3, 5))
    replay_all(cases, dev, "resnet50 160 3|5")


@pytest.mark.gpu
def test_vits_step_contractions_vs_fp64(monkeypatch):
    """ViT-S/16 at 384 x 384: T = 577 = 9 * 64 + 1, so the last query tile and the last key tile each hold one valid row"""
    dev = torch.device("cuda:0")
    cases = capture(monkeypatch, lambda: _bench_step(dev, "vits_dino", 384, 8, 16))
    replay_all(cases, dev, "vits_dino 384")
