"""Crop-zoom prediction at kernel level (include/lp_hip.h, csrc/cropzoom.hip): lp_bbox_from_keypoints, lp_bbox_smooth, lp_frames_crop_resize.

Boxes: exact equality with the reference's own ``_compute_bbox_df`` (tests/golden/cropzoom.npz, written by tests/golden/make_golden_cropzoom.py)
AND with the rule restated here in numpy.  The keypoints lie on a 1/8-px grid below 4096: every sum is exact in double precision, so the
equality does not depend on the order of summation.
Smoothing: exact equality with pandas' ``rolling(window, center=True, min_periods=1).median().round(0).astype(int)`` and with the fixture.
Crop-resize: bit-for-bit equality with lp_frames_resize of the zero-padded crop materialised on the host, one frame at a time (every frame has
a box, hence a scale, of its own), in both border modes."""

import ctypes as C
import os

import numpy as np
import pandas as pd
import pytest

from lightning_pose_amd import _lib
from tests.hipemu import emu

ARG, UNSUPPORTED = -1, -2     # LP_ERR_ARGUMENT, LP_ERR_UNSUPPORTED (include/lp_hip.h)
MAX_ANCHORS, MAX_WINDOW = 64, 255  # LP_BBOX_MAX_ANCHORS, LP_BBOX_SMOOTH_MAX_WINDOW
GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cropzoom.npz"))
BBOX_CASES = sorted({k.split("/")[1] for k in GOLDEN.files if k.startswith("bbox/")})
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
BORDERS = {"clamp": _lib.BORDER_CLAMP, "renorm": _lib.BORDER_RENORM}


# ---------------------------------------------------------------------------------------------------------------- boxes
def _bbox(kp, anchors=(), ratio=None, ch=None, cw=None, rc=False):
    kp = np.asarray(kp, np.float32)
    n, k, _ = kp.shape
    kb, out = emu.Buf(kp), emu.Buf(np.full((n, 4), -77, np.int32))
    arr = (C.c_int * max(1, len(anchors)))(*[int(a) for a in anchors])
    code = emu.lib().lp_bbox_from_keypoints(kb.p, n, k, arr, len(anchors), 0.0 if ratio is None else float(ratio), ch or 0, cw or 0, out.p,
                                            emu.stream())
    if rc:
        return code
    emu.ok(code)
    return out.np()


def _bbox_numpy(kp, anchors, ratio, ch, cw):
    """the reference rule (utils/cropzoom.py:31-143) restated: float64, the mean over the anchors, one size from the larger span"""
    kp = np.asarray(kp, np.float64)
    sel = kp[:, list(anchors)] if len(anchors) else kp
    centroid = sel.mean(axis=1)
    if ratio is not None:
        span = np.maximum(sel[:, :, 0].max(1) - sel[:, :, 0].min(1), sel[:, :, 1].max(1) - sel[:, :, 1].min(1))
        size = np.ceil(span * ratio).astype(np.int64)
        size = size + size % 2
        sizes = np.column_stack([size, size])
    else:
        sizes = np.tile([ch + ch % 2, cw + cw % 2], (len(kp), 1))
    corner = np.trunc(centroid - sizes // 2).astype(np.int64)   # (sic) [x, y] - [h // 2, w // 2]
    return np.concatenate([corner, sizes], axis=1)


@pytest.mark.parametrize("case", BBOX_CASES)
def test_bbox_from_keypoints_equals_reference_and_restatement(kernel_backend, case):
    kp, anchors = GOLDEN[f"bbox/{case}/keypoints"], GOLDEN[f"bbox/{case}/anchors"].tolist()
    ratio, ch, cw = [None if np.isnan(v) else v for v in GOLDEN[f"bbox/{case}/params"]]
    ch, cw = (None, None) if ch is None else (int(ch), int(cw))
    assert np.array_equal(kp.astype(np.float32).astype(np.float64), kp)     # fp32 holds the 1/8-px grid exactly
    got = _bbox(kp, anchors, ratio, ch, cw)
    assert got.dtype == np.int32 and got.shape == (len(kp), 4)
    np.testing.assert_array_equal(got, GOLDEN[f"bbox/{case}/bbox"])
    np.testing.assert_array_equal(got, _bbox_numpy(kp, anchors, ratio, ch, cw))


def test_bbox_cases_cover_what_they_claim():
    """the fixture's cases hold the edge conditions their names promise (a fixture regenerated with other numbers would silently stop testing them)"""
    neg = GOLDEN["bbox/negative_corner/bbox"]
    assert neg[0].tolist() == [-6, -9, 20, 20] and neg[1].tolist() == [-9, -6, 20, 20] and neg[2].tolist() == [0, 0, 20, 20]  # -6.5 -> -6, -0.125 -> 0
    odd = GOLDEN["bbox/odd_size/bbox"]
    assert odd[:, 2].tolist() == [8, 8, 8]           # 7 -> 8, ceil(6.125) = 7 -> 8, 8 stays
    fixed = GOLDEN["bbox/fixed_odd/bbox"]
    assert (fixed[:, 2] == 102).all() and (fixed[:, 3] == 64).all()
    kp = GOLDEN["bbox/fixed_odd/keypoints"][:, [1, 4]].mean(1)
    np.testing.assert_array_equal(fixed[:, 0], np.trunc(kp[:, 0] - 51))   # x moves by h // 2
    np.testing.assert_array_equal(fixed[:, 1], np.trunc(kp[:, 1] - 32))   # y by w // 2
    assert len(GOLDEN["bbox/ratio_all/anchors"]) == 0 and len(GOLDEN["bbox/single_frame/keypoints"]) == 1


def test_bbox_degenerate_frames_are_zero(kernel_backend):
    """stated deviation: a span of 0 (one keypoint) or a non-finite anchor gives [0, 0, 0, 0]; a NaN outside the anchors does not matter"""
    one = np.array([[[100.5, 20.25]], [[7.0, 9.0]]])
    np.testing.assert_array_equal(_bbox(one, (), ratio=1.5), np.zeros((2, 4), np.int32))
    np.testing.assert_array_equal(_bbox(one, (), ch=10, cw=12), [[95, 14, 10, 12], [2, 3, 10, 12]])   # fixed mode has a size: a box
    kp = np.array([[[10.0, 10.0], [30.0, 50.0], [np.nan, 1.0]], [[10.0, 10.0], [30.0, 50.0], [2.0, 1.0]], [[10.0, np.inf], [30.0, 50.0], [2.0, 1.0]]])
    got = _bbox(kp, (0, 1), ratio=1.0)
    np.testing.assert_array_equal(got, [[0, 10, 40, 40], [0, 10, 40, 40], [0, 0, 0, 0]])
    np.testing.assert_array_equal(_bbox(kp, (), ratio=1.0), [[0, 0, 0, 0], [-11, -4, 50, 50], [0, 0, 0, 0]])   # spans 28, 49 -> 50; centroid (14, 20.33) - 25
    np.testing.assert_array_equal(_bbox(kp, (1, 2), ch=4, cw=4)[0], [0, 0, 0, 0])


def test_bbox_arguments(kernel_backend):
    kp = np.zeros((2, 3, 2), np.float32)
    assert _bbox(kp, (), ratio=1.0, ch=4, cw=4, rc=True) == ARG        # both modes
    assert _bbox(kp, (), rc=True) == ARG                                # neither
    assert _bbox(kp, (3,), ratio=1.0, rc=True) == ARG                   # anchor index out of range
    assert _bbox(np.zeros((2, 70, 2), np.float32), tuple(range(MAX_ANCHORS + 1)), ratio=1.0, rc=True) == UNSUPPORTED


# ---------------------------------------------------------------------------------------------------------------- smoothing
def _smooth(bbox, window, rc=False):
    bbox = np.asarray(bbox, np.int32)
    bb, out = emu.Buf(bbox), emu.Buf(np.full(bbox.shape, -77, np.int32))
    code = emu.lib().lp_bbox_smooth(bb.p, len(bbox), int(window), out.p, emu.stream())
    if rc:
        return code
    emu.ok(code)
    return out.np()


def _smooth_pandas(bbox, window):
    df = pd.DataFrame(np.asarray(bbox, np.int64), columns=["x", "y", "h", "w"])
    return df.rolling(window=window, center=True, min_periods=1).median().round(0).astype(int).to_numpy()


@pytest.mark.parametrize("tag", ["n10", "n3", "n1"])
@pytest.mark.parametrize("window", [1, 2, 3, 4, 5, 6])
def test_bbox_smooth_equals_pandas(kernel_backend, tag, window):
    raw = GOLDEN[f"smooth/{tag}/bbox"]
    got = _smooth(raw, window)
    np.testing.assert_array_equal(got, GOLDEN[f"smooth/{tag}/window{window}"])
    np.testing.assert_array_equal(got, _smooth_pandas(raw, window))
    np.testing.assert_array_equal(_smooth(raw, window), got)      # a second run: the same bits


def test_bbox_smooth_halves_round_to_even(kernel_backend):
    """the fixture's h column (w = -h) puts .5 medians with an even and an odd floor at the edges: 0.5 -> 0, 3.5 -> 4, -0.5 -> 0, -3.5 -> -4"""
    raw = GOLDEN["smooth/n10/bbox"]
    assert raw[:4, 2].tolist() == [0, 1, 3, 4] and raw[:4, 3].tolist() == [0, -1, -3, -4]
    got = _smooth(raw, 2)
    assert got[1, 2] == 0 and got[3, 2] == 4 and got[1, 3] == 0 and got[3, 3] == -4
    col = np.array([[1, -1, 0, 0], [2, -2, 0, 0], [3, -3, 0, 0], [2, -2, 5, 5]])   # 1.5 -> 2, 2.5 -> 2, -1.5 -> -2, -2.5 -> -2
    np.testing.assert_array_equal(_smooth(col, 2), _smooth_pandas(col, 2))
    assert _smooth(col, 2)[1:3, 0].tolist() == [2, 2] and _smooth(col, 2)[1:3, 1].tolist() == [-2, -2]


def test_bbox_smooth_long_window_and_bound(kernel_backend):
    rng = np.random.default_rng(5)
    raw = rng.integers(-500, 500, size=(300, 4))
    raw[:, 3] = rng.integers(0, 3, size=300)      # many ties
    for window in (31, MAX_WINDOW):
        np.testing.assert_array_equal(_smooth(raw, window), _smooth_pandas(raw, window))
    assert _smooth(raw, MAX_WINDOW + 1, rc=True) == UNSUPPORTED
    assert _smooth(raw, 0, rc=True) == ARG


# ---------------------------------------------------------------------------------------------------------------- crop-resize
def _norm():
    return emu.frame_norm(MEAN, STD)


def _crop(frame, box):
    """the zero-padded crop [y, y + h) x [x, x + w) of one (Hs, Ws, 3) frame"""
    x, y, h, w = [int(v) for v in box]
    hs, ws, _ = frame.shape
    out = np.zeros((h, w, 3), np.uint8)
    y0, y1, x0, x1 = max(y, 0), min(y + h, hs), max(x, 0), min(x + w, ws)
    if y1 > y0 and x1 > x0:
        out[y0 - y:y1 - y, x0 - x:x1 - x] = frame[y0:y1, x0:x1]
    return out


def _black(H, W):
    m, s = np.float32(MEAN), np.float32(STD)
    return np.broadcast_to((((np.float32(0) - m) * (np.float32(1) / s))[:, None, None]), (3, H, W))


def _crop_resize(src_buf, ptr, S, Hs, Ws, frame_stride, row_stride, boxes, H, W, border, pad=256):
    """-> (S, 3, H, W) planes; the destination sits between two canaries that must come back untouched"""
    n = S * 3 * H * W
    canary = np.float32(-12345.678)
    dst = emu.Buf(np.full(n + 2 * pad, canary, np.float32))
    bb = emu.Buf(np.asarray(boxes, np.int32).reshape(S, 4))
    nrm = _norm()
    emu.ok(emu.lib().lp_frames_crop_resize(ptr, S, Hs, Ws, frame_stride, row_stride, bb.p, H, W, border, C.byref(nrm),
                                           C.c_void_p(dst.p.value + 4 * pad), emu.stream()))
    full = dst.np()
    assert (full[:pad] == canary).all() and (full[n + pad:] == canary).all(), "wrote outside the destination"
    return full[pad:pad + n].reshape(S, 3, H, W).copy()


def _check_against_resize(frames, boxes, H, W, border):
    """one launch over all frames == lp_frames_resize of every frame's materialised crop, bit for bit"""
    S, Hs, Ws, _ = frames.shape
    src = emu.Buf(frames)
    got = _crop_resize(src, src.p, S, Hs, Ws, Hs * Ws * 3, Ws * 3, boxes, H, W, BORDERS[border])
    again = _crop_resize(src, src.p, S, Hs, Ws, Hs * Ws * 3, Ws * 3, boxes, H, W, BORDERS[border])
    np.testing.assert_array_equal(got.view(np.uint32), again.view(np.uint32))
    for s in range(S):
        if boxes[s][2] <= 0 or boxes[s][3] <= 0:
            want = _black(H, W)
        else:
            want = emu.frames_resize(_crop(frames[s], boxes[s])[None], H, W, BORDERS[border], _norm())[0]
        np.testing.assert_array_equal(got[s].view(np.uint32), np.ascontiguousarray(want).view(np.uint32), err_msg=f"frame {s} box {boxes[s]}")
    return got


# [x, y, h, w] on a 37 x 53 frame: inside; over the top-left corner; over the bottom-right corner; entirely outside; the whole frame;
# a 6 x 8 box (an up-scale: radius 1); no box (h = 0)
BOXES_37x53 = [[10, 5, 24, 30], [-7, -4, 20, 26], [35, 22, 28, 40], [80, 60, 12, 16], [0, 0, 37, 53], [20, 11, 6, 8], [3, 3, 0, 10]]


@pytest.fixture(scope="module")
def frames_37x53():
    return np.random.default_rng(11).integers(0, 256, size=(len(BOXES_37x53), 37, 53, 3), dtype=np.uint8)


@pytest.mark.parametrize("border", ["clamp", "renorm"])
def test_crop_resize_equals_resize_of_the_crop(kernel_backend, frames_37x53, border):
    """(18, 70): W is no multiple of 64 (a second, partial column tile), H no multiple of 4"""
    got = _check_against_resize(frames_37x53, BOXES_37x53, 18, 70, border)
    black = np.ascontiguousarray(_black(18, 70)).view(np.uint32)
    np.testing.assert_array_equal(got[3].view(np.uint32), black)      # a box entirely outside the frame: exactly the normalised black frame
    np.testing.assert_array_equal(got[6].view(np.uint32), black)      # h = 0
    whole = emu.frames_resize(frames_37x53[4:5], 18, 70, BORDERS[border], _norm())[0]
    np.testing.assert_array_equal(got[4].view(np.uint32), whole.view(np.uint32))   # the whole frame: lp_frames_resize of the frame itself


@pytest.mark.parametrize("border", ["clamp", "renorm"])
@pytest.mark.parametrize("size", [(18, 70), (7, 5), (33, 64)])
def test_crop_resize_random_boxes(kernel_backend, border, size):
    """16 random boxes (1 .. 70 x 1 .. 90 pixels, corners from 20 pixels outside the frame to beyond its far edge) on a 45 x 61 frame: scales from
    a 20-fold up-scale to an 18-fold down-scale, each frame its own.  Rounding coincidences between the two kernels (a product that goes
    unrounded into a sum in one and rounded in the other) show as one-ulp differences in a few pixels of a few boxes - this is the net for them."""
    rng = np.random.default_rng(21)
    frames = rng.integers(0, 256, size=(16, 45, 61, 3), dtype=np.uint8)
    boxes = np.column_stack([rng.integers(-20, 70, 16), rng.integers(-20, 50, 16), rng.integers(1, 71, 16), rng.integers(1, 91, 16)]).tolist()
    _check_against_resize(frames, boxes, size[0], size[1], border)


@pytest.mark.parametrize("border", ["clamp", "renorm"])
def test_crop_resize_heavy_downscale(kernel_backend, border):
    """64 x 96 -> (4, 6): a 16-fold down-scale, 32-row windows - several chunks of source rows per tile"""
    frames = np.random.default_rng(12).integers(0, 256, size=(2, 64, 96, 3), dtype=np.uint8)
    _check_against_resize(frames, [[0, 0, 64, 96], [-9, 5, 64, 96]], 4, 6, border)


@pytest.mark.parametrize("border", ["clamp", "renorm"])
def test_crop_resize_wide_tile_reads_global(kernel_backend, border):
    """8 x 1000 -> (3, 70): the first column tile spans 915 source pixels, more than the staging buffer holds - the tile reads its taps from
    global memory; the second tile (6 columns) is staged.  Also a non-square scale (2.7 down, 14.3 across)."""
    frames = np.random.default_rng(13).integers(0, 256, size=(2, 8, 1000, 3), dtype=np.uint8)
    _check_against_resize(frames, [[0, 0, 8, 1000], [-30, -2, 10, 1040]], 3, 70, border)


@pytest.mark.parametrize("border", ["clamp", "renorm"])
def test_crop_resize_strided_source(kernel_backend, frames_37x53, border):
    """the source is a view into a wider buffer: row_stride > 3 * Ws (odd: rows start at every alignment), frames every other slot"""
    S, Hs, Ws = 3, 37, 53
    row_stride, slot = 3 * Ws + 10, (3 * Ws + 10) * Hs + 7
    wide = np.random.default_rng(14).integers(0, 256, size=5 + 2 * S * slot, dtype=np.uint8)
    for s in range(S):
        base = 5 + 2 * s * slot
        view = wide[base:base + row_stride * Hs].reshape(Hs, row_stride)
        view[:, :3 * Ws] = frames_37x53[s].reshape(Hs, 3 * Ws)
    boxes = BOXES_37x53[:S]
    buf = emu.Buf(wide)
    got = _crop_resize(buf, C.c_void_p(buf.p.value + 5), S, Hs, Ws, 2 * slot, row_stride, boxes, 18, 70, BORDERS[border])
    np.testing.assert_array_equal(buf.np(), wide)        # the source is read only
    for s in range(S):
        want = emu.frames_resize(_crop(frames_37x53[s], boxes[s])[None], 18, 70, BORDERS[border], _norm())[0]
        np.testing.assert_array_equal(got[s].view(np.uint32), want.view(np.uint32))


def test_crop_resize_arguments(kernel_backend, frames_37x53):
    src, dst, bb, nrm = emu.Buf(frames_37x53[:1]), emu.Z((1, 3, 4, 4)), emu.Buf(np.array([[0, 0, 8, 8]], np.int32)), _norm()
    call = lambda *a: emu.lib().lp_frames_crop_resize(*a, emu.stream())  # noqa: E731
    assert call(src.p, 1, 37, 53, 37 * 53 * 3, 53 * 3 - 1, bb.p, 4, 4, 1, C.byref(nrm), dst.p) == ARG      # rows overlap
    assert call(src.p, 1, 37, 53, 37 * 53 * 3, 53 * 3, None, 4, 4, 1, C.byref(nrm), dst.p) == ARG           # no boxes
    assert call(src.p, 1, 37, 53, 37 * 53 * 3, 53 * 3, bb.p, 4, 4, 2, C.byref(nrm), dst.p) == ARG           # unknown border
    assert call(src.p, 1, 37, 53, 37 * 53 * 3, 53 * 3, bb.p, 4, 4, 1, None, dst.p) == ARG                   # the planes are always normalised
    bad = emu.frame_norm(MEAN, (0.2, 0.0, 0.2))
    assert call(src.p, 1, 37, 53, 37 * 53 * 3, 53 * 3, bb.p, 4, 4, 1, C.byref(bad), dst.p) == ARG
