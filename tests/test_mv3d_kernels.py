"""lp_mv3d_plan / lp_mv3d_fill / lp_mv3d_finish (csrc/mv3d.hip) against float64 restatements of include/lp_hip.h.

The plan's oracle is written here from ``tests/cameras_fp64.py`` (triangulate_pairs, project), ``numpy.nanmedian`` and the closed-form
similarity.  The bar of every comparison is measured, not chosen: the SAME oracle is run in float32 (torch / numpy, never the code under test)
and the kernel may be 4 x as far from float64 as that restatement is, with a floor of 1e-6 relative to the largest value.  Both distances are
printed (``profiles/mv3d_accuracy.txt`` keeps a run).  Runs on the CPU build of the kernel source and, under ``-m gpu``, on the device."""

import ctypes as C
import warnings

import numpy as np
import pytest
import torch

from lightning_pose_amd import _lib
from tests import cameras_fp64 as O
from tests.hipemu import emu

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
SHIFT = 0.25
NAN = float("nan")


# ---- plan: inputs -----------------------------------------------------------------------------------------------------------------
def plan_inputs(V, K, ndist, patterns, seed):
    """B = len(patterns) samples of a synthetic rig; labels in stored-image px; everything rounded to float32 (what the kernel is given)"""
    B = len(patterns)
    rig = O.make_rig(B, V, K, ndist, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    hs = torch.tensor([480.0, 512.0, 600.0, 384.0])[:V]
    ws = torch.tensor([640.0, 672.0, 800.0, 512.0])[:V]
    src_hw = torch.stack([hs, ws], -1)[None].repeat(B, 1, 1).double()                       # (B, V, 2)
    bb = rig["bbox"].reshape(B, V, 4)
    kp = torch.stack([(rig["points_2d"][..., 0] - bb[..., 0:1]) / bb[..., 3:4] * src_hw[..., 1:2],
                      (rig["points_2d"][..., 1] - bb[..., 1:2]) / bb[..., 2:3] * src_hw[..., 0:1]], -1)   # (B, V, K, 2)
    for b, pat in enumerate(patterns):
        if pat == "two_nan":          # two unlabeled points in two different views: every keypoint still has a pair
            kp[b, 1, 3] = NAN
            kp[b, 2, 5, 0] = NAN
        elif pat == "two_triangulable":   # keypoints 2.. are labeled in view 0 only
            kp[b, 1:, 2:] = NAN
        elif pat == "all_nan":
            kp[b] = NAN
        elif pat == "short_view":     # view 0 keeps two labels; every keypoint is still triangulated from the other views
            kp[b, 0, 2:] = NAN
        else:
            assert pat == "clean"
    draws = torch.cat([0.8 + 0.4 * torch.rand(B, 1, generator=g), 2 * torch.rand(B, 3, generator=g) - 1], 1)
    inp = dict(kp=kp, src_hw=src_hw, bbox=rig["bbox"], intr=rig["intrinsics"], extr=rig["extrinsics"], dist=O.dist12(rig["distortions"]),
               draws=draws.double())
    return {k: v.float().double() for k, v in inp.items()}


# ---- plan: the oracle, in any dtype -------------------------------------------------------------------------------------------------
def _nanmedian(a: np.ndarray, axis: int) -> np.ndarray:
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)   # (all-NaN slices give NaN, which is the specification)
        return np.nanmedian(a, axis=axis)


def oracle_plan(inp, dtype, augment, H, W):
    t = {k: v.to(dtype) for k, v in inp.items()}
    kp, src_hw = t["kp"], t["src_hw"]
    B, V, K, _ = kp.shape
    bb = t["bbox"].reshape(B, V, 4)
    hs, ws = src_hw[..., 0:1], src_hw[..., 1:2]
    pts = torch.stack([kp[..., 0] / ws * bb[..., 3:4] + bb[..., 0:1], kp[..., 1] / hs * bb[..., 2:3] + bb[..., 1:2]], -1)
    p3d = O.triangulate_pairs(pts, t["intr"], t["extr"], t["dist"])
    X = torch.from_numpy(_nanmedian(p3d.numpy(), axis=1))                                  # (B, K, 3)
    plain2d = torch.stack([kp[..., 0] / ws * W, kp[..., 1] / hs * H], -1)
    eye = torch.tensor([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], dtype=dtype)
    kp3d, kp2d, M, status = X.clone(), plain2d.clone(), eye.repeat(B, V, 1, 1), torch.zeros(B, dtype=torch.int32)
    for b in range(B):
        if bool(torch.isnan(kp[b]).all()):
            status[b] = 2
            continue
        if not augment or int((~torch.isnan(X[b]).any(-1)).sum()) < 3:
            status[b] = 1
            continue
        Xb = X[b].numpy()
        med = _nanmedian(Xb, axis=0)
        Xa = (Xb - med) * t["draws"][b, 0].numpy() + med
        extent = np.nanmax(Xa, axis=0) - np.nanmin(Xa, axis=0)
        Xa = torch.from_numpy(Xa + np.asarray(SHIFT, Xa.dtype) * extent * t["draws"][b, 1:].numpy())
        q = O.project(Xa[None], t["intr"][b:b + 1], t["extr"][b:b + 1], t["dist"][b:b + 1])[0]         # (V, K, 2) frame px
        Ms, short = [], False
        for v in range(V):
            o = kp[b, v]
            n = torch.stack([(q[v, :, 0] - bb[b, v, 0]) / bb[b, v, 3] * ws[b, v, 0], (q[v, :, 1] - bb[b, v, 1]) / bb[b, v, 2] * hs[b, v, 0]], -1)
            ok = torch.isfinite(o).all(-1) & torch.isfinite(n).all(-1)
            if int(ok.sum()) < 3:
                short = True
                break
            o, n = o[ok], n[ok]
            om, nm = o.mean(0), n.mean(0)
            oc, nc = o - om, n - nm
            den = (oc * oc).sum()
            if float(den) == 0.0:
                Ms.append(eye.clone())
                continue
            a = (oc * nc).sum() / den
            c = (oc[:, 0] * nc[:, 1] - oc[:, 1] * nc[:, 0]).sum() / den
            Ms.append(torch.stack([torch.stack([a, -c, nm[0] - (a * om[0] - c * om[1])]), torch.stack([c, a, nm[1] - (c * om[0] + a * om[1])])]))
        if short:
            status[b] = 3
            continue
        M[b] = torch.stack(Ms)
        kp3d[b] = Xa
        kp2d[b] = torch.stack([(q[..., 0] - bb[b, :, 0:1]) / bb[b, :, 3:4] * W, (q[..., 1] - bb[b, :, 1:2]) / bb[b, :, 2:3] * H], -1)
    return dict(kp3d=kp3d.double(), kp2d=kp2d.double(), affine=M.double(), status=status)


def run_plan(inp, augment, H, W, rc=False, null=None, V=None):
    kp = inp["kp"]
    B, Vn, K, _ = kp.shape
    V = Vn if V is None else V
    names = ["kp", "src_hw", "bbox", "intr", "extr", "dist", "draws"]
    bufs = {n: emu.B(inp[n].numpy(), np.float32) for n in names}
    outs = dict(kp3d=emu.Buf(np.full((B, K, 3), 7.0, np.float32)), kp2d=emu.Buf(np.full((B, Vn, K, 2), 7.0, np.float32)),
                affine=emu.Buf(np.full((B, Vn, 2, 3), 7.0, np.float32)), status=emu.Buf(np.full(B, -9, np.int32)))
    p = {n: (None if n == null else b.p) for n, b in {**bufs, **outs}.items()}
    code = emu.lib().lp_mv3d_plan(p["kp"], p["src_hw"], p["bbox"], p["intr"], p["extr"], p["dist"], p["draws"], int(augment), SHIFT, H, W, B, V, K,
                                  p["kp3d"], p["kp2d"], p["affine"], p["status"], emu.stream())
    if rc:
        return code
    emu.ok(code)
    return {n: torch.from_numpy(b.np().copy()) for n, b in outs.items()}


def _distance(got, want):
    """largest |got - want| over the entries that are finite in `want`; the NaN patterns must agree"""
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), "NaN pattern differs"
    if bool(nan.all()):
        return 0.0, 0.0
    return float((got.double() - want)[~nan].abs().max()), float(want[~nan].abs().max())


SETS = {"a": ["clean", "two_nan", "two_triangulable", "all_nan"], "b": ["clean", "two_nan", "short_view", "all_nan"]}
WANT_STATUS = {"clean": 0, "two_nan": 0, "two_triangulable": 1, "all_nan": 2, "short_view": 3}
_oracles: dict = {}


def _case(V, K, ndist, which, augment, H=256, W=384):
    key = (V, K, ndist, which, augment)
    if key not in _oracles:   # computed once, shared by the emulator and the device halves, never modified
        inp = plan_inputs(V, K, ndist, SETS[which], seed=100 + V)
        _oracles[key] = (inp, oracle_plan(inp, torch.float64, augment, H, W), oracle_plan(inp, torch.float32, augment, H, W))
    return _oracles[key] + (H, W)


@pytest.mark.parametrize("augment", [1, 0])
@pytest.mark.parametrize("which", ["a", "b"])
@pytest.mark.parametrize("V,K,ndist", [(3, 7, 5), (4, 17, 12)])
def test_plan_against_the_float64_oracle(kernel_backend, V, K, ndist, which, augment):
    inp, want, f32, H, W = _case(V, K, ndist, which, augment)
    got = run_plan(inp, augment, H, W)
    expect = [WANT_STATUS[p] if augment or WANT_STATUS[p] == 2 else 1 for p in SETS[which]]
    assert want["status"].tolist() == expect == f32["status"].tolist()      # (the patterns are what they are meant to be)
    assert got["status"].tolist() == expect
    for name in ("kp3d", "kp2d", "affine"):
        err, scale = _distance(got[name], want[name])
        ref, _ = _distance(f32[name], want[name])
        bar = max(4.0 * ref, 1e-6 * scale)
        print(f"plan V={V} K={K} ndist={ndist} set={which} augment={augment} {name}: kernel {err:.3g}  float32 oracle {ref:.3g}  "
              f"bar {bar:.3g}  largest value {scale:.3g}")
        assert err <= bar, (name, err, bar)
    if augment:
        b = SETS[which].index("two_nan")
        assert torch.isnan(inp["kp"][b, 1, 3]).all() and torch.isfinite(got["kp2d"][b, 1, 3]).all()   # unlabeled, yet reprojected
        assert not torch.equal(got["affine"][b, 0], torch.tensor([[1.0, 0, 0], [0, 1.0, 0]]))
    for b, s in enumerate(expect):
        if s != 0:   # not augmented: exactly the identity, and the labels in model px
            assert torch.equal(got["affine"][b], torch.tensor([[1.0, 0, 0], [0, 1.0, 0]]).repeat(V, 1, 1))
    if "all_nan" in SETS[which]:
        b = SETS[which].index("all_nan")
        assert torch.isnan(got["kp3d"][b]).all() and torch.isnan(got["kp2d"][b]).all()


def test_plan_gives_the_same_bits_twice(kernel_backend):
    inp, _, _, H, W = _case(4, 17, 12, "b", 1)
    one, two = run_plan(inp, 1, H, W), run_plan(inp, 1, H, W)
    for name in one:
        assert torch.equal(one[name].view(torch.int32), two[name].view(torch.int32)), name


def test_plan_refuses_what_it_cannot_do(kernel_backend):
    inp, _, _, H, W = _case(3, 7, 5, "a", 1)
    assert run_plan(inp, 1, H, W, rc=True, V=9) == -2            # LP_ERR_UNSUPPORTED (nothing is launched)
    for null in ("kp", "src_hw", "bbox", "intr", "extr", "dist", "draws", "kp3d", "kp2d", "affine", "status"):
        assert run_plan(inp, 1, H, W, rc=True, null=null) == -1, null   # LP_ERR_ARGUMENT
    big = {k: (v[:, :, :1].repeat(1, 1, 129, 1) if k == "kp" else v) for k, v in inp.items()}
    assert run_plan(big, 1, H, W, rc=True) == -2                 # K = 129


# ---- fill and finish --------------------------------------------------------------------------------------------------------------
def make_images(B, Hs, Ws, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:Hs, 0:Ws]
    smooth = 120 + 80 * np.sin(xx / 5.0)[None, :, :, None] * np.cos(yy / 7.0)[None, :, :, None]
    img = smooth + rng.integers(-30, 30, size=(B, Hs, Ws, 3))
    return np.clip(img, 3, 250).astype(np.uint8)


def normalised(src, dt):
    return ((src.astype(dt) / dt(255)) - np.asarray(MEAN, dt)) / np.asarray(STD, dt)     # (B, Hs, Ws, 3)


def _taps(n_out, n_in, dt):
    """torch.nn.functional.interpolate's bilinear source index (align_corners=False), its two taps and weights"""
    s = dt(n_in) / dt(n_out) * (np.arange(n_out).astype(dt) + dt(0.5)) - dt(0.5)
    s = np.maximum(s, dt(0))
    i0 = np.minimum(s.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = s - i0.astype(dt)
    return i0, i1, dt(1) - l1, l1


def restate_finish(src, M32, fill, H, W, dt):
    """normalise -> warp_affine(M, bilinear, align_corners=True, fill) -> resize(H, W, bilinear, half-pixel centres, no antialias) by
    gathering: (B, 3, H, W) in dtype `dt`, from the fp32 M and fill the kernel is given"""
    B, Hs, Ws, _ = src.shape
    nrm = normalised(src, dt)
    Y0, Y1, ly0, ly1 = _taps(H, Hs, dt)
    X0, X1, lx0, lx1 = _taps(W, Ws, dt)
    out = np.empty((B, 3, H, W), dt)
    for b in range(B):
        M = M32[b].astype(dt)
        det = M[0, 0] * M[1, 1] - M[0, 1] * M[1, 0]
        i00, i01, i10, i11 = M[1, 1] / det, -M[0, 1] / det, -M[1, 0] / det, M[0, 0] / det
        itx, ity = -(i00 * M[0, 2] + i01 * M[1, 2]), -(i10 * M[0, 2] + i11 * M[1, 2])
        f = dt(fill[b])

        def sample(Xs, Ys):   # integer warped pixels (W,), (H,) -> (H, W, 3)
            Xg, Yg = np.meshgrid(Xs.astype(dt), Ys.astype(dt))
            sx, sy = i00 * Xg + i01 * Yg + itx, i10 * Xg + i11 * Yg + ity
            inside = (sx > -1) & (sx < Ws) & (sy > -1) & (sy < Hs)
            sx, sy = np.where(inside, sx, 0), np.where(inside, sy, 0)
            fx, fy = np.floor(sx), np.floor(sy)
            x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
            wx1, wy1 = (sx - fx)[..., None], (sy - fy)[..., None]
            wx0, wy0 = dt(1) - wx1, dt(1) - wy1

            def px(yi, xi):
                ok = (xi >= 0) & (xi < Ws) & (yi >= 0) & (yi < Hs)
                return np.where(ok[..., None], nrm[b, np.clip(yi, 0, Hs - 1), np.clip(xi, 0, Ws - 1)], f)

            val = wy0 * (wx0 * px(y0, x0) + wx1 * px(y0, x0 + 1)) + wy1 * (wx0 * px(y0 + 1, x0) + wx1 * px(y0 + 1, x0 + 1))
            return np.where(inside[..., None], val, f)

        ly0_, ly1_, lx0_, lx1_ = ly0[:, None, None], ly1[:, None, None], lx0[None, :, None], lx1[None, :, None]
        res = ly0_ * (lx0_ * sample(X0, Y0) + lx1_ * sample(X1, Y0)) + ly1_ * (lx0_ * sample(X0, Y1) + lx1_ * sample(X1, Y1))
        out[b] = res.transpose(2, 0, 1)
    return out


def plain_resize(src, H, W, dt):
    """the resize alone, of the normalised image, in torch's order of operations"""
    nrm = normalised(src, dt)
    Hs, Ws = src.shape[1:3]
    Y0, Y1, ly0, ly1 = _taps(H, Hs, dt)
    X0, X1, lx0, lx1 = _taps(W, Ws, dt)
    g = lambda Y, X: nrm[:, Y][:, :, X]  # noqa: E731
    ly0, ly1, lx0, lx1 = ly0[None, :, None, None], ly1[None, :, None, None], lx0[None, None, :, None], lx1[None, None, :, None]
    return (ly0 * (lx0 * g(Y0, X0) + lx1 * g(Y0, X1)) + ly1 * (lx0 * g(Y1, X0) + lx1 * g(Y1, X1))).transpose(0, 3, 1, 2)


def run_fill(src, rc=False):
    B, Hs, Ws, _ = src.shape
    sb, fb = emu.Buf(src), emu.Buf(np.full(B, np.nan, np.float32))
    norm = emu.frame_norm(MEAN, STD)
    code = emu.lib().lp_mv3d_fill(sb.p, B, Hs, Ws, C.byref(norm), fb.p, emu.stream())
    if rc:
        return code
    emu.ok(code)
    return fb.np().copy()


def run_finish(src, M, fill, H, W, V=1, v=0, dst=None):
    B, Hs, Ws, _ = src.shape
    aff = np.tile(np.array([[1, 0, 0], [0, 1, 0]], np.float32), (B, V, 1, 1))
    aff[:, v] = M
    sb, ab, fb = emu.Buf(src), emu.Buf(aff), emu.Buf(np.asarray(fill, np.float32))
    db = emu.Buf(np.full((B, V, 3, H, W), np.nan, np.float32) if dst is None else dst)
    norm = emu.frame_norm(MEAN, STD)
    emu.ok(emu.lib().lp_mv3d_finish(sb.p, B, Hs, Ws, ab.p, fb.p, C.byref(norm), V, v, H, W, db.p, emu.stream()))
    return db.np().copy()


SHAPES = [(37, 53, 32, 32), (96, 128, 64, 64)]
IDENT = np.array([[1, 0, 0], [0, 1, 0]], np.float32)


def _matrices(Hs, Ws):
    th = np.deg2rad(9.0)
    m0 = np.array([[1.1 * np.cos(th), -1.1 * np.sin(th), 0.07 * Ws], [1.1 * np.sin(th), 1.1 * np.cos(th), -0.05 * Hs]])
    th = np.deg2rad(-4.0)
    m1 = np.array([[0.85 * np.cos(th), -0.85 * np.sin(th), -0.1 * Ws], [0.85 * np.sin(th), 0.85 * np.cos(th), 0.12 * Hs]])
    return np.stack([m0, m1]).astype(np.float32)


@pytest.mark.parametrize("Hs,Ws,H,W", SHAPES)
def test_fill_is_the_smallest_normalised_pixel(kernel_backend, Hs, Ws, H, W):
    src = make_images(2, Hs, Ws, seed=Hs)
    src[1, Hs // 2, Ws // 3, 1] = 0          # the minimum of one image sits in one channel of one pixel
    got = run_fill(src)
    want32 = normalised(src, np.float32).reshape(2, -1).min(1)
    want64 = normalised(src, np.float64).reshape(2, -1).min(1)
    print(f"fill {Hs}x{Ws}: kernel {got}  float32 {want32}  |kernel - float64| {np.abs(got - want64).max():.3g}")
    assert np.array_equal(got, want32)        # a minimum has no order, and the normalisation is three rounded operations
    assert np.abs(got - want64).max() <= max(4 * np.abs(want32 - want64).max(), 1e-6 * np.abs(want64).max())
    # an image whose bytes do not start 16-byte aligned and are fewer than one vector
    tiny = make_images(3, 1, 5, seed=1)
    assert np.array_equal(run_fill(tiny), normalised(tiny, np.float32).reshape(3, -1).min(1))


@pytest.mark.parametrize("Hs,Ws,H,W", SHAPES)
def test_finish_against_the_float64_gather(kernel_backend, Hs, Ws, H, W):
    src = make_images(2, Hs, Ws, seed=Hs + 1)
    M = _matrices(Hs, Ws)
    fill = run_fill(src)
    got = run_finish(src, M, fill, H, W)[:, 0]
    want = restate_finish(src, M, fill, H, W, np.float64)
    f32 = restate_finish(src, M, fill, H, W, np.float32)
    err, ref, scale = np.abs(got - want).max(), np.abs(f32 - want).max(), np.abs(want).max()
    bar = max(4 * ref, 1e-6 * scale)
    print(f"finish {Hs}x{Ws}->{H}x{W}: kernel {err:.3g}  float32 restatement {ref:.3g}  bar {bar:.3g}  largest value {scale:.3g}")
    assert err <= bar
    assert (got == fill[:, None, None, None]).any() and (got != fill[:, None, None, None]).any()   # the warp shows both image and padding


@pytest.mark.parametrize("Hs,Ws,H,W", SHAPES)
def test_finish_identity_is_the_plain_resize_bit_for_bit(kernel_backend, Hs, Ws, H, W):
    src = make_images(2, Hs, Ws, seed=Hs + 2)
    fill = run_fill(src)
    got = run_finish(src, np.stack([IDENT, IDENT]), fill, H, W)[:, 0]
    want = plain_resize(src, H, W, np.float32)
    assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(want).view(np.uint32))
    # ... and that restatement is torch's resize of the normalised image
    ref = torch.nn.functional.interpolate(torch.from_numpy(normalised(src, np.float32)).permute(0, 3, 1, 2), size=(H, W), mode="bilinear",
                                          align_corners=False, antialias=False).numpy()
    assert np.abs(want - ref).max() <= 4e-6 * np.abs(ref).max()


def test_finish_out_of_frame_is_the_fill_and_views_keep_to_their_slice(kernel_backend):
    Hs, Ws, H, W = SHAPES[0]
    src = make_images(2, Hs, Ws, seed=9)
    fill = run_fill(src)
    away = np.array([[1, 0, 10.0 * Ws], [0, 1, 0]], np.float32)
    out = run_finish(src, np.stack([away, away]), fill, H, W, V=3, v=1)
    assert np.isnan(out[:, 0]).all() and np.isnan(out[:, 2]).all()            # untouched
    # every tap reads exactly fill[b]; the resize then blends four equal values with weights l0 = 1 - l1 and l1, in torch's order: two
    # products, one sum and a weight sum of 1 +- 2^-24 per level, two levels -> within 8 * 2^-24 |fill| (4 ulp) of the constant
    f = fill[:, None, None, None]
    tol = 8 * 2.0 ** -24 * np.abs(f)
    assert (np.abs(out[:, 1] - f) <= tol).all()
    singular = np.zeros((2, 2, 3), np.float32)
    assert (np.abs(run_finish(src, singular, fill, H, W)[:, 0] - f) <= tol).all()
    # a width that is no multiple of 4 takes the 4-byte stores and stays inside its rows
    odd = run_finish(src, np.stack([IDENT, IDENT]), fill, 30, 27, V=2, v=0)
    assert np.isnan(odd[:, 1]).all()
    assert np.array_equal(odd[:, 0].view(np.uint32), np.ascontiguousarray(plain_resize(src, 30, 27, np.float32)).view(np.uint32))


def test_the_abi_names_the_new_entry_points():
    assert {"lp_mv3d_plan", "lp_mv3d_fill", "lp_mv3d_finish"} <= set(_lib.PROTOTYPES) and _lib.ABI_VERSION >= 148
