"""Every stage of csrc/labelaug.hip against an independent numpy / scipy restatement written here (imgaug and OpenCV are not installed:
parity with imgaug itself is unpinned, the operator DEFINITIONS are what is checked).

Integer-exact operators (Rot90 where no resize follows, the coarse masks, hist-eq, crop-and-pad) must match bit for bit.  Filtering and
interpolating operators are one real number computed in fp32 on the device and in fp64 here, then rounded: at most ONE grey level of
difference at any pixel is allowed, and only at rounding ties: a pixel may differ only where the fp64 value lies within 2e-3 (fp32's reach,
see TIE) of a .5 boundary.  The share of pixels that differ is printed by every such test (`pytest -s`); measured on the emulated build:
geom 5e-5 .. 7e-5, blur 0 .. 2e-3, emboss 0 .. 2.3e-2 (weights on a 1/20 lattice put 5 % of the real values EXACTLY on a tie), elastic gather
1e-4, CLAHE blend see `pytest -s`.
Batched = looped: each test runs >= 3 images with different parameters and the last test re-runs every image alone.
"""

import numpy as np
import pytest
import scipy.ndimage as ndi
import torch

from lightning_pose_amd import _lib, ops
from lightning_pose_amd.data import augmentations as A

H, W, B = 150, 203, 3
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


def images(seed=0, b=B, h=H, w=W):
    rng = np.random.default_rng(seed)
    smooth = ndi.gaussian_filter(rng.uniform(0, 255, (b, h, w, 3)), (0, 2, 2, 0)) * 4 - 384   # structure + full range, clipped
    return np.clip(smooth + rng.uniform(-20, 20, (b, h, w, 3)), 0, 255).astype(np.uint8)


def table(b=B):
    t = np.zeros(b, dtype=ops.LABELAUG_DTYPE)
    t["image_id"] = np.arange(b)
    return t


def dev(a, device):
    return torch.from_numpy(np.array(a, order="C", copy=True)).to(device)


TIE = 2e-3   # fp32 error of a sum of <= 25 products of weights O(1) with levels <= 255: 25 * 255 * 2^-23 = 7.6e-4, doubled and rounded up


def close_u8(got, want_real, what):
    """`want_real`: the fp64 value before rounding.  At most one level anywhere, and a pixel may differ at all only where the real value
    lies within fp32's reach (TIE) of a rounding boundary; the share of pixels that differ is printed."""
    want = np.clip(np.floor(want_real + 0.5), 0, 255)
    diff = np.abs(got.astype(np.int64) - want.astype(np.int64))
    share = float((diff > 0).mean())
    print(f"{what}: max |diff| = {diff.max()}, share of pixels that differ = {share:.2e}")
    assert diff.max() <= 1, (what, int(diff.max()))
    off_tie = np.abs(want_real - np.floor(want_real) - 0.5)[diff > 0]
    assert off_tie.size == 0 or off_tie.max() < TIE, (what, float(off_tie.max()))


# ---- Philox4x32-10 restated (Salmon et al. 2011), vectorised over counters ---------------------------------------------------------------
def philox(seed, c0, c1):
    m = np.uint64(0xFFFFFFFF)
    c0 = np.asarray(c0, dtype=np.uint64)
    x0, x1 = c0.copy(), np.broadcast_to(np.asarray(c1, dtype=np.uint64), c0.shape).copy()
    x2, x3 = np.zeros_like(x0), np.zeros_like(x0)
    ka, kb = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * x0, np.uint64(0xCD9E8D57) * x2
        x0, x1, x2, x3 = (p1 >> np.uint64(32)) ^ x1 ^ ka, p1 & m, (p0 >> np.uint64(32)) ^ x3 ^ kb, p0 & m
        ka, kb = (ka + np.uint64(0x9E3779B9)) & m, (kb + np.uint64(0xBB67AE85)) & m
    return x0, x1


def coarse_mask(seed, image_id, op, ch, gh, gw, thr, h=H, w=W):
    ys, xs = np.mgrid[0:h, 0:w]
    cell = (ys * gh // h) * gw + xs * gw // w
    w0, _ = philox(seed, cell, image_id | (op << 16) | (ch << 20))
    return (w0 >> np.uint64(8)) < thr


# ---- geom ------------------------------------------------------------------------------------------------------------------------------------
def test_rot90_is_exact_where_no_resize_follows(stack_backend):
    img = images(1)
    t = table()
    for i, k in enumerate((2, 0, 2)):
        if k:
            t["flags"][i] = _lib.AUG_GEOM
            t["geom"][i] = np.linalg.inv(A.rot90_matrix(k, H, W))[:2].reshape(-1)
    got = ops.labelaug_geom(dev(img, stack_backend), ops.labelaug_table(t, stack_backend)).cpu().numpy()
    for i, k in enumerate((2, 0, 2)):
        assert np.array_equal(got[i], np.rot90(img[i], -k, axes=(0, 1))), k
    sq = images(2, 3, 151, 151)
    t = table()
    for i, k in enumerate((1, 3, 2)):
        t["flags"][i] = _lib.AUG_GEOM
        t["geom"][i] = np.linalg.inv(A.rot90_matrix(k, 151, 151))[:2].reshape(-1)
    got = ops.labelaug_geom(dev(sq, stack_backend), ops.labelaug_table(t, stack_backend)).cpu().numpy()
    for i, k in enumerate((1, 3, 2)):
        assert np.array_equal(got[i], np.rot90(sq[i], -k, axes=(0, 1))), k   # np.rot90 turns counter-clockwise for positive k


def bilinear_zero_fill(img, fwd):
    """destination pixel centres through the inverse of `fwd`, order-1 spline with everything outside the image equal to 0"""
    inv = np.linalg.inv(fwd)
    ys, xs = np.mgrid[0:img.shape[0], 0:img.shape[1]].astype(np.float64)
    sx = inv[0, 0] * (xs + 0.5) + inv[0, 1] * (ys + 0.5) + inv[0, 2] - 0.5
    sy = inv[1, 0] * (xs + 0.5) + inv[1, 1] * (ys + 0.5) + inv[1, 2] - 0.5
    return np.stack([ndi.map_coordinates(img[..., c].astype(np.float64), [sy, sx], order=1, mode="grid-constant", cval=0.0) for c in range(3)], -1)


def test_affine_and_rot90_with_resize(stack_backend):
    img = images(3)
    t = table()
    mats = [A.affine_matrix(17.0, 1.0, (0.0, 0.0), H, W), A.affine_matrix(-25.0, 1.1, (0.05, -0.03), H, W) @ A.rot90_matrix(1, H, W),
            A.rot90_matrix(3, H, W)]
    for i, m in enumerate(mats):
        t["flags"][i] = _lib.AUG_GEOM
        t["geom"][i] = np.linalg.inv(m)[:2].reshape(-1)
    got = ops.labelaug_geom(dev(img, stack_backend), ops.labelaug_table(t, stack_backend)).cpu().numpy()
    for i, m in enumerate(mats):
        m32 = np.eye(3)
        m32[:2] = t["geom"][i].reshape(2, 3).astype(np.float64)      # the same real matrix the kernel was given
        close_u8(got[i], bilinear_zero_fill(img[i], np.linalg.inv(m32)), f"geom[{i}]")
    # the rotation turns clockwise on the screen: a point right of the centre moves down
    p = A.affine_matrix(20.0, 1.0, (0.0, 0.0), H, W) @ np.array([W / 2 + 10.0, H / 2, 1.0])
    assert p[1] > H / 2 and p[0] < W / 2 + 10.0


# ---- local -----------------------------------------------------------------------------------------------------------------------------------
def motion_blur_restated(k, angle, direction):
    """imgaug's definition with scipy: the centre column of a k x k uint8 image holds linspace(d, 1 - d) * 255, d = (direction + 1) / 2; the
    image is turned by `angle` (clockwise on the screen) about its centre with an order-1 spline and zero fill, rounded to levels, / sum"""
    d = (np.clip(direction, -1, 1) + 1) / 2
    line = np.zeros((k, k))
    line[:, k // 2] = np.floor(np.linspace(d, 1 - d, k) * 255 + 0.5)       # (levels: floor(v + 0.5), the rounding of every stage)
    c, s = np.cos(np.radians(angle)), np.sin(np.radians(angle))
    back = np.array([[c, -s], [s, c]])                      # output (row, col) -> input (row, col): the turn undone
    ctr = np.array([(k - 1) / 2, (k - 1) / 2])
    turned = np.floor(ndi.affine_transform(line, back, offset=ctr - back @ ctr, order=1, mode="grid-constant", cval=0.0) + 0.5)
    out = np.zeros((5, 5))
    o = (5 - k) // 2
    out[o:o + k, o:o + k] = turned / turned.sum()
    return out


def emboss_restated(alpha, s):
    return (1 - alpha) * np.array([[0, 0, 0], [0, 1, 0], [0, 0, 0.0]]) + alpha * np.array([[-1 - s, -s, 0], [-s, 1, s], [0, s, 1 + s]])


def test_motion_blur_and_emboss(stack_backend):
    img = images(4)
    t = table()
    cases_b, cases_e = [(5, 37.0, 0.4), (3, -80.0, -1.0), (5, 0.0, 0.0)], [(0.5, 1.5), (0.1, 0.5), (0.33, 1.0)]
    blur, emb = [A.motion_blur_weights(*c) for c in cases_b], [A.emboss_weights(*c) for c in cases_e]
    for c, got_w in zip(cases_b + [(5, 90.0, 1.0), (5, -45.0, 0.0), (3, 20.0, 0.3)], blur + [A.motion_blur_weights(5, 90.0, 1.0),
                                                                                         A.motion_blur_weights(5, -45.0, 0.0), A.motion_blur_weights(3, 20.0, 0.3)]):
        assert np.abs(got_w - motion_blur_restated(*c)).max() < 1e-12, c      # (uint8 levels on both sides: equal unless a level flips)
    turned = A.motion_blur_weights(5, 90.0, 1.0)       # direction 1 weights the TOP of the line; a quarter turn clockwise lays it to the right
    assert np.count_nonzero(turned[2]) >= 4 and not turned[[0, 1, 3, 4]].any() and turned[2, 4] > turned[2, 0]
    for c, got_w in zip(cases_e, emb):
        assert np.abs(got_w - emboss_restated(*c)).max() < 1e-15, c
    for i in range(B):
        t["flags"][i] = _lib.AUG_BLUR | _lib.AUG_EMBOSS
        t["blur"][i], t["emboss"][i] = blur[i].reshape(-1), emb[i].reshape(-1)
        assert abs(blur[i].sum() - 1.0) < 1e-12 and blur[i].min() >= 0.0
    v = blur[2][:, 2]
    assert np.allclose(v, 0.2, atol=2e-3) and np.count_nonzero(blur[2]) == 5      # angle 0, direction 0: the plain vertical line
    td = ops.labelaug_table(t, stack_backend)
    got_b = ops.labelaug_local(dev(img, stack_backend), td, _lib.AUG_LOCAL_BLUR_COARSE).cpu().numpy()
    got_e = ops.labelaug_local(dev(img, stack_backend), td, _lib.AUG_LOCAL_EMBOSS).cpu().numpy()
    for i in range(B):
        for got, wts, name in ((got_b, t["blur"][i].reshape(5, 5), "blur"), (got_e, t["emboss"][i].reshape(3, 3), "emboss")):
            want = np.stack([ndi.correlate(img[i, ..., c].astype(np.float64), wts.astype(np.float64), mode="mirror") for c in range(3)], -1)
            close_u8(got[i], want, f"{name}[{i}]")


def test_coarse_masks_bit_for_bit(stack_backend):
    img = images(5)
    seed = (123456 << 20) + 7
    t = table()
    t["flags"] = [_lib.AUG_DROPOUT | _lib.AUG_DROP_PER_CHANNEL | _lib.AUG_SALT, _lib.AUG_DROPOUT | _lib.AUG_PEPPER,
                  _lib.AUG_SALT | _lib.AUG_PEPPER | _lib.AUG_DROPOUT]
    t["coarse_gh"] = [[45, 9, 14], [45, 7, 15], [30, 11, 8]]
    t["coarse_gw"] = [[60, 12, 19], [60, 10, 20], [41, 15, 11]]
    t["coarse_thr"] = [[int(0.02 * 2 ** 24), int(0.05 * 2 ** 24), int(0.05 * 2 ** 24)], [int(0.1 * 2 ** 24)] * 3, [int(0.03 * 2 ** 24)] * 3]
    got = ops.labelaug_local(dev(img, stack_backend), ops.labelaug_table(t, stack_backend), _lib.AUG_LOCAL_BLUR_COARSE, seed).cpu().numpy()
    lut = ops.salt_quantiles()
    assert lut.min() >= 128 and lut.max() == 255 and abs(float(lut.mean()) - (127.5 + 127.5 * 2 / np.pi)) < 0.5   # E|cos| = 2 / pi
    ys, xs = np.mgrid[0:H, 0:W]
    hits = 0
    for i in range(B):
        want = img[i].copy()
        f = int(t["flags"][i])
        if f & _lib.AUG_DROPOUT:
            for c in range(3):
                m = coarse_mask(seed, i, _lib.AUG_OP_DROPOUT, c if f & _lib.AUG_DROP_PER_CHANNEL else 0, t["coarse_gh"][i][0], t["coarse_gw"][i][0],
                                t["coarse_thr"][i][0])
                want[..., c][m] = 0
                hits += int(m.sum())
        for op, flag in ((_lib.AUG_OP_SALT, _lib.AUG_SALT), (_lib.AUG_OP_PEPPER, _lib.AUG_PEPPER)):
            if f & flag:
                m = coarse_mask(seed, i, op, 0, t["coarse_gh"][i][op], t["coarse_gw"][i][op], t["coarse_thr"][i][op])
                w0, _ = philox(seed, ys * W + xs, i | (op << 16) | (1 << 24))
                val = lut[(w0 >> np.uint64(24)).astype(np.int64)]
                val = val if op == _lib.AUG_OP_SALT else 255 - val
                want[m] = val[m][:, None]
                hits += int(m.sum())
        assert np.array_equal(got[i], want), i
    assert hits > 1000   # the masks are not empty
    # per_channel: the three channels of image 0 are masked differently, those of image 1 alike
    z0 = [(got[0][..., c] == 0) & (img[0][..., c] != 0) for c in range(3)]
    assert not np.array_equal(z0[0], z0[1])


# ---- elastic ---------------------------------------------------------------------------------------------------------------------------------
def keys_bicubic_zero_fill(img, sx, sy):
    """Keys kernel (A = -0.75) at pixel-index coordinates (sx, sy); taps outside the image contribute 0"""
    a = -0.75

    def k(u):
        u = np.abs(u)
        return np.where(u <= 1, ((a + 2) * u - (a + 3)) * u * u + 1, np.where(u < 2, ((a * u - 5 * a) * u + 8 * a) * u - 4 * a, 0.0))

    h, w = img.shape[:2]
    x0, y0 = np.floor(sx).astype(int) - 1, np.floor(sy).astype(int) - 1
    out = np.zeros(sx.shape + (3,))
    for j in range(4):
        for i in range(4):
            xi, yi = x0 + i, y0 + j
            ok = (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h)
            wgt = k(sx - xi) * k(sy - yi) * ok
            out += wgt[..., None] * img[np.clip(yi, 0, h - 1), np.clip(xi, 0, w - 1)].astype(np.float64)
    return out


def test_elastic_field_and_gather(stack_backend):
    img = images(6)
    seed = (99 << 20) + 3
    t = table()
    t["flags"] = [_lib.AUG_ELASTIC, 0, _lib.AUG_ELASTIC]
    t["elastic_alpha"] = [10.0, 5.0, 3.5]
    td = ops.labelaug_table(t, stack_backend)
    field = ops.labelaug_elastic_field(td, B, H, W, 5.0, seed).cpu().numpy()
    ys, xs = np.mgrid[0:H, 0:W]
    for i in (0, 2):
        w0, w1 = philox(seed, ys * W + xs, i | (_lib.AUG_OP_ELASTIC << 16))
        for c, wd in enumerate((w0, w1)):
            noise = 2.0 * (((wd >> np.uint64(8)).astype(np.float64) + 0.5) / 2 ** 24) - 1.0
            want = float(t["elastic_alpha"][i]) * ndi.gaussian_filter(noise, 5.0, mode="mirror", truncate=4.0)
            err = np.abs(field[i, c] - want).max()
            print(f"elastic field[{i}][{c}]: max |err| = {err:.2e} px, std = {want.std():.3f} px")
            assert err < 1e-5 * max(1.0, float(t["elastic_alpha"][i])), err    # 41 + 41 fp32 products of O(0.1) terms
        assert 0.01 * t["elastic_alpha"][i] < field[i].std() < 0.06 * t["elastic_alpha"][i]   # ~0.03 alpha px for sigma = 5
    assert not field[1].any()
    # the gather, on a displacement of this test's own (larger than the presets': several pixels, leaving the frame at the border)
    rng = np.random.default_rng(0)
    own = ndi.gaussian_filter(rng.uniform(-1, 1, (B, 2, H, W)), (0, 0, 4, 4)) * 60
    got = ops.labelaug_elastic_apply(dev(img, stack_backend), td, dev(own.astype(np.float32), stack_backend)).cpu().numpy()
    own = own.astype(np.float32).astype(np.float64)
    for i in (0, 2):
        close_u8(got[i], keys_bicubic_zero_fill(img[i], xs + own[i, 0], ys + own[i, 1]), f"elastic[{i}]")
    assert np.array_equal(got[1], img[1])


# ---- histogram operators -------------------------------------------------------------------------------------------------------------------------
def test_histeq_bit_for_bit(stack_backend):
    img = images(7)
    img[2] = (img[2] // 3 + 60)        # a narrow histogram
    img[0, ..., 1] = 77                # one grey level only: unchanged
    t = table()
    t["flags"] = [_lib.AUG_HISTEQ, 0, _lib.AUG_HISTEQ]
    got, lut = ops.labelaug_histeq(dev(img, stack_backend), ops.labelaug_table(t, stack_backend))
    got, lut = got.cpu().numpy(), lut.cpu().numpy()
    for i in (0, 2):
        for c in range(3):
            hist = np.bincount(img[i, ..., c].reshape(-1), minlength=256).astype(np.int64)
            cdf = np.cumsum(hist)
            cmin = cdf[np.nonzero(hist)[0][0]]
            if H * W == cmin:
                want = np.arange(256)
            else:
                want = np.where(cdf >= cmin, np.floor(255.0 * (cdf - cmin) / (H * W - cmin) + 0.5), 0).clip(0, 255)
            assert np.array_equal(lut[i, c], want.astype(np.uint8)), (i, c)
            assert np.array_equal(got[i, ..., c], want.astype(np.uint8)[img[i, ..., c]])
    assert np.array_equal(got[1], img[1])
    assert got[2].min() == 0 and got[2].max() == 255    # equalisation stretches the narrow histogram over the whole range


def clahe_restated(ch, ty, tx, clip):
    """OpenCV's CLAHE on one channel, in fp64: returns the real value before the final rounding"""
    h, w = ch.shape
    th, tw = -(-h // ty), -(-w // tx)
    padded = np.pad(ch, ((0, ty * th - h), (0, tx * tw - w)), mode="reflect")      # numpy "reflect" = reflect-101
    luts = np.zeros((ty, tx, 256))
    for j in range(ty):
        for i in range(tx):
            hist = np.bincount(padded[j * th:(j + 1) * th, i * tw:(i + 1) * tw].reshape(-1), minlength=256).astype(np.int64)
            excess = int(np.maximum(hist - clip, 0).sum())
            hist = np.minimum(hist, clip) + excess // 256
            resid = excess % 256
            if resid:
                step = max(256 // resid, 1)
                k = 0
                while k < 256 and resid > 0:
                    hist[k] += 1
                    k += step
                    resid -= 1
            luts[j, i] = np.minimum(np.floor(255.0 * np.cumsum(hist) / (th * tw) + 0.5), 255)
    ys, xs = np.mgrid[0:h, 0:w]
    fy, fx = ys / th - 0.5, xs / tw - 0.5          # OpenCV: tyf = y * inv_th - 0.5
    y1, x1 = np.floor(fy).astype(int), np.floor(fx).astype(int)
    ay, ax = fy - y1, fx - x1
    y2, x2 = np.clip(y1 + 1, 0, ty - 1), np.clip(x1 + 1, 0, tx - 1)
    y1, x1 = np.clip(y1, 0, ty - 1), np.clip(x1, 0, tx - 1)
    v = ch.astype(np.int64)
    top = luts[y1, x1, v] * (1 - ax) + luts[y1, x2, v] * ax
    bot = luts[y2, x1, v] * (1 - ax) + luts[y2, x2, v] * ax
    return top * (1 - ay) + bot * ay


def test_clahe(stack_backend):
    img = images(8)
    t = table()
    geo = [A.clahe_geometry(H, W, 12, 8.0), None, A.clahe_geometry(H, W, 5, 2.5)]
    assert geo[0] == (12, 12, max(1, int(8.0 * 13 * 17 / 256))) and geo[2][:2] == (5, 5)     # tile counts; tiles of ceil(150 / 12) x ceil(203 / 12) px
    t["flags"] = [_lib.AUG_CLAHE, 0, _lib.AUG_CLAHE]
    for i, slot in ((0, 1), (2, 0)):   # (slots need not follow the image order)
        t["clahe_tiles_y"][i], t["clahe_tiles_x"][i], t["clahe_clip"][i] = geo[i]
        t["clahe_slot"][i] = slot
    got = ops.labelaug_clahe(dev(img, stack_backend), ops.labelaug_table(t, stack_backend), [2, 0], 12, 12).cpu().numpy()
    for i in (0, 2):
        want = np.stack([clahe_restated(img[i, ..., c], *geo[i]) for c in range(3)], -1)
        close_u8(got[i], want, f"clahe[{i}]")
        assert not np.array_equal(got[i], img[i])
    assert np.array_equal(got[1], img[1])


# ---- crop-and-pad + resize + normalise + mirror ----------------------------------------------------------------------------------------------
def test_crop_and_pad_matches_the_plain_resize_of_the_cropped_image(stack_backend):
    img = images(9)
    t = table()
    pads = [(-12, 20, 7, -30), (0, 0, 0, 0), (15, -9, -22, 11)]    # top, right, bottom, left
    t["flags"] = [_lib.AUG_CROPPAD, 0, _lib.AUG_CROPPAD | _lib.AUG_HFLIP]
    t["pad"] = pads
    got = ops.labelaug_finish(dev(img, stack_backend), ops.labelaug_table(t, stack_backend), 128, 256, MEAN, STD).cpu()
    for i, (top, right, bottom, left) in enumerate(pads):
        x = img[i][max(-top, 0):H - max(-bottom, 0), max(-left, 0):W - max(-right, 0)]
        x = np.pad(x, ((max(top, 0), max(bottom, 0)), (max(left, 0), max(right, 0)), (0, 0)))
        assert x.shape == (H + top + bottom, W + left + right, 3)
        want = ops.frames_resize(dev(x[None], stack_backend), 128, 256, "renorm", mean=MEAN, std=STD, interpolation="cubic").cpu()[0]
        if i == 2:
            want = want.flip(-1)
        assert torch.equal(got[i], want), i


def test_keypoints_follow_the_affine_and_the_field(stack_backend):
    t = table()
    t["flags"] = [_lib.AUG_ELASTIC, 0, _lib.AUG_ELASTIC]
    rng = np.random.default_rng(1)
    field = ndi.gaussian_filter(rng.uniform(-1, 1, (B, 2, H, W)), (0, 0, 5, 5)).astype(np.float32) * 30
    kp = rng.uniform(5, 140, (B, 6, 2)).astype(np.float32)
    kp[0, 1] = np.nan
    aff = np.stack([A.affine_matrix(10.0 * i, 1.0, (0.0, 0.0), H, W)[:2] for i in range(B)]).astype(np.float32)
    got = ops.labelaug_keypoints(dev(kp, stack_backend), dev(aff, stack_backend), ops.labelaug_table(t, stack_backend), dev(field, stack_backend),
                                 H, W).cpu().numpy()
    for i in range(B):
        moved = np.einsum("ij,kj->ki", aff[i].astype(np.float64), np.concatenate([kp[i], np.ones((6, 1))], 1))
        if t["flags"][i]:
            c = np.stack([np.clip(moved[:, 1] - 0.5, 0, H - 1), np.clip(moved[:, 0] - 0.5, 0, W - 1)])
            with np.errstate(invalid="ignore"):
                d = np.stack([ndi.map_coordinates(field[i, a].astype(np.float64), np.nan_to_num(c), order=1, mode="nearest") for a in range(2)], 1)
            moved = moved - d
        ok = ~np.isnan(kp[i, :, 0])
        assert np.abs(got[i][ok] - moved[ok]).max() < 2e-4
        assert np.isnan(got[i][~ok]).all()


def test_batched_equals_looped(stack_backend):
    """one launch for the batch computes what one launch per image computes (the Philox counters carry the image's number, not its position)"""
    img = images(10)
    pipe = A.imgaug_transform({k: {**v, "p": 1.0} for k, v in A.expand_imgaug_str_to_dict("dlc-top-down").items()}, seed=5)
    drawn = pipe.draw(B, H, W)
    assert all((drawn["table"]["flags"] & f).all() for f in (_lib.AUG_BLUR, _lib.AUG_DROPOUT, _lib.AUG_SALT, _lib.AUG_PEPPER, _lib.AUG_ELASTIC,
                                                     _lib.AUG_HISTEQ, _lib.AUG_CLAHE, _lib.AUG_EMBOSS, _lib.AUG_CROPPAD))
    whole, field = pipe.run(dev(img, stack_backend), drawn)
    whole_f = ops.labelaug_finish(whole, ops.labelaug_table(drawn["table"], stack_backend), 128, 128, MEAN, STD)
    kp = dev(np.random.default_rng(2).uniform(10, 140, (B, 5, 2)).astype(np.float32), stack_backend)
    aff = dev(drawn["affine"][:, :2].astype(np.float32), stack_backend)
    kp_whole = ops.labelaug_keypoints(kp, aff, ops.labelaug_table(drawn["table"], stack_backend), field, H, W)
    for i in range(B):
        one = {**drawn, "table": drawn["table"][i:i + 1].copy()}
        one["table"]["clahe_slot"] = 0
        alone, f1 = pipe.run(dev(img[i:i + 1], stack_backend), one)
        assert torch.equal(alone[0], whole[i]) and torch.equal(f1[0], field[i]), i
        kp1 = ops.labelaug_keypoints(kp[i:i + 1], aff[i:i + 1], ops.labelaug_table(one["table"], stack_backend), f1, H, W)
        assert torch.equal(kp1[0], kp_whole[i]), i
        assert torch.equal(ops.labelaug_finish(alone, ops.labelaug_table(one["table"], stack_backend), 128, 128, MEAN, STD)[0], whole_f[i])
