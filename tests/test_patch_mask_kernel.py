"""lp_patch_mask_f32 (csrc/patchmask.hip) against a numpy restatement of its specification (include/lp_hip.h): the patch choice is the
rank of a Philox4x32-10 word, the output is the batch with the chosen patches set to +0.0 and every other pixel copied bit for bit.
Every comparison is exact - the kernel does no arithmetic on pixel values.  Runs on the CPU build of the kernel source and, under
``-m gpu``, on the device."""

import ctypes as C

import numpy as np
import pytest

from lightning_pose_amd import _lib
from tests.hipemu import emu

PATCH = 16
M32 = np.uint64(0xFFFFFFFF)


def philox_word(key: int, c0: np.ndarray, c1: int) -> np.ndarray:
    """first output word of Philox4x32-10 for key (lo, hi) = key and counter (c0, c1, 0, 0)"""
    x0 = np.asarray(c0, np.uint64) & M32
    x1 = np.full_like(x0, c1 & 0xFFFFFFFF)
    x2, x3 = np.zeros_like(x0), np.zeros_like(x0)
    ka, kb = key & 0xFFFFFFFF, (key >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * x0, np.uint64(0xCD9E8D57) * x2
        x0, x1, x2, x3 = (p1 >> np.uint64(32)) ^ x1 ^ np.uint64(ka), p1 & M32, (p0 >> np.uint64(32)) ^ x3 ^ np.uint64(kb), p0 & M32
        ka, kb = (ka + 0x9E3779B9) & 0xFFFFFFFF, (kb + 0xBB67AE85) & 0xFFFFFFFF
    return x0.astype(np.uint32)


def pack_key(seed: int, step: int) -> int:
    return (seed & 0xFFFFFFFF) | ((step & 0xFFFFFFFF) << 32)


def oracle_mask(bv: int, n: int, count: int, key: int) -> np.ndarray:
    """(bv, n) of 1 (keep) / 0 (mask): masked iff the rank of (word, p), ascending, is < count"""
    mask = np.ones((bv, n), np.float32)
    for i in range(bv):
        order = np.argsort(philox_word(key, np.arange(n), i), kind="stable")   # stable: equal words keep the order of p
        mask[i, order[:count]] = 0.0
    return mask


def oracle_images(images: np.ndarray, mask: np.ndarray, patch: int = PATCH) -> np.ndarray:
    """images (bv, C, H, W) as uint32 bits with the masked patches set to the bits of +0.0"""
    out = images.view(np.uint32).copy()
    nw = images.shape[3] // patch
    for i, p in zip(*np.nonzero(mask == 0)):
        y, x = (p // nw) * patch, (p % nw) * patch
        out[i, :, y:y + patch, x:x + patch] = 0
    return out


def make_images(bv: int, h: int, w: int, seed: int, c: int = 3) -> np.ndarray:
    """random values with NaNs (two payloads, both signs), +-Inf and -0.0 on ~10 % of the pixels: some fall inside masked patches, some outside"""
    rng = np.random.default_rng(seed)
    bits = rng.standard_normal((bv, c, h, w)).astype(np.float32).view(np.uint32)
    special = np.array([0x7FC12345, 0xFFC00001, 0x7F800000, 0xFF800000, 0x80000000], np.uint32)
    hit = rng.random(bits.shape) < 0.1
    bits[hit] = special[rng.integers(0, len(special), int(hit.sum()))]
    return bits.view(np.float32)


def patch_mask(images: np.ndarray, count: int, key: int, mask_in=None, in_place=False, patch=PATCH, rc=False, offset_floats=0):
    """-> (out bits, mask_out, images bits after the call).  ``offset_floats``: the image and output pointers start that many floats into
    their buffers (a 4-byte-aligned but not 16-byte-aligned call)."""
    bv, c, h, w = images.shape
    n = (h // patch) * (w // patch)
    pad = np.zeros(offset_floats, np.float32)
    ib = emu.Buf(np.concatenate([pad, images.reshape(-1)]))
    ob = ib if in_place else emu.Buf(np.concatenate([pad, np.full(images.size, np.nan, np.float32)]))
    mb, mo = emu.B(mask_in, np.float32), emu.Buf(np.full((bv, max(n, 1)), np.nan, np.float32))
    at = lambda b: C.c_void_p(b.p.value + 4 * offset_floats)  # noqa: E731
    code = emu.lib().lp_patch_mask_f32(at(ib), bv, c, h, w, patch, count, key, emu.ptr(mb), at(ob), mo.p, emu.stream())
    if rc:
        return code
    emu.ok(code)
    bits = lambda b: b.np()[offset_floats:].reshape(images.shape).view(np.uint32)  # noqa: E731
    return bits(ob), mo.np(), bits(ib)


def raise_for(code: int) -> None:
    """the Python side's mapping of a return code (_lib.check), with the library under test supplying the message"""
    with pytest.MonkeyPatch.context() as m:
        m.setattr(_lib, "_lib", emu.lib())
        _lib.check(code, "lp_patch_mask_f32")


SHAPES = [(1, 1, 16, 16), (2, 3, 48, 80), (1, 2, 40, 52), (1, 1, 33, 35), (2, 4, 256, 256), (1, 1, 512, 512)]
CASES = [(s, cnt) for s in SHAPES for cnt in sorted({0, 1, ((s[2] // PATCH) * (s[3] // PATCH)) // 2, (s[2] // PATCH) * (s[3] // PATCH)})]


@pytest.mark.parametrize("shape,count", CASES, ids=[f"{b}x{v}x{h}x{w}-count{c}" for (b, v, h, w), c in CASES])
def test_choice_and_output_match_the_specification(kernel_backend, shape, count):
    b, v, h, w = shape
    bv, n = b * v, (h // PATCH) * (w // PATCH)
    key = pack_key(11, 321)
    images = make_images(bv, h, w, seed=h * w + count)
    want_mask = oracle_mask(bv, n, count, key)
    want = oracle_images(images, want_mask)
    assert ((want_mask == 0).sum(1) == count).all()
    out, mask, after = patch_mask(images, count, key)
    assert np.array_equal(mask, want_mask)
    assert ((mask == 0).sum(1) == count).all()
    assert np.array_equal(out, want)
    assert np.array_equal(after, images.view(np.uint32))            # the input is not written
    if 0 < count:   # the fixture really puts a NaN inside a masked patch and a -0.0 outside one
        src = images.view(np.uint32)
        assert ((src & 0x7FFFFFFF) > 0x7F800000)[want != src].any() and (out[want != src] == 0).all()
    if count < n:
        assert (out == 0x80000000).any()
    out2, mask2, _ = patch_mask(images, count, key)                  # a second call: the same bits
    assert np.array_equal(out2, out) and np.array_equal(mask2, mask)
    out3, mask3, after3 = patch_mask(images, count, key, in_place=True)
    assert np.array_equal(out3, want) and np.array_equal(mask3, want_mask) and np.array_equal(after3, want)


@pytest.mark.parametrize("shape", [(2, 3, 48, 80), (1, 1, 33, 35), (2, 4, 256, 256)], ids=lambda s: "x".join(map(str, s)))
def test_a_supplied_mask_is_used_as_given(kernel_backend, shape):
    b, v, h, w = shape
    bv, n = b * v, (h // PATCH) * (w // PATCH)
    rng = np.random.default_rng(5)
    images = make_images(bv, h, w, seed=3)
    random_mask = (rng.random((bv, n)) < 0.5).astype(np.float32)
    ragged = np.ones((bv, n), np.float32)                            # image i loses its first i % (n + 1) patches: another number each
    for i in range(bv):
        ragged[i, :i % (n + 1)] = 0.0
    for given in (random_mask, ragged):
        for in_place in (False, True):
            out, mask, _ = patch_mask(images, count=n, key=pack_key(1, 2), mask_in=given, in_place=in_place)   # count is ignored
            assert np.array_equal(mask, given)
            assert np.array_equal(out, oracle_images(images, given))


def test_pointers_that_are_not_16_byte_aligned_take_the_scalar_path(kernel_backend):
    """W % 4 == 0 but the buffers start 4 bytes past a 16-byte boundary"""
    images = make_images(2, 32, 48, seed=8)
    key = pack_key(2, 9)
    want = oracle_images(images, oracle_mask(2, 6, 3, key))
    for in_place in (False, True):
        out, mask, _ = patch_mask(images, 3, key, offset_floats=1, in_place=in_place)
        assert np.array_equal(out, want) and np.array_equal(mask, oracle_mask(2, 6, 3, key))


def test_patch_sizes_other_than_16(kernel_backend):
    """patch 8 (vector path) and patch 6 (not a multiple of 4: a 16-byte piece would straddle a patch edge, so 4-byte accesses)"""
    images = make_images(2, 40, 44, seed=9)
    for patch in (8, 6):
        n = (40 // patch) * (44 // patch)
        key = pack_key(4, 4)
        m = oracle_mask(2, n, n // 3, key)
        out, mask, _ = patch_mask(images, n // 3, key, patch=patch)
        assert np.array_equal(mask, m) and np.array_equal(out, oracle_images(images, m, patch))


def test_step_and_seed_change_the_choice(kernel_backend):
    images = np.ones((1, 1, 256, 256), np.float32)
    keys = [pack_key(7, 100), pack_key(7, 101), pack_key(8, 100)]
    oracles = [oracle_mask(1, 256, 128, k) for k in keys]
    assert not np.array_equal(oracles[0], oracles[1]) and not np.array_equal(oracles[0], oracles[2])
    for k, want in zip(keys, oracles):
        assert np.array_equal(patch_mask(images, 128, k)[1], want)


def test_the_choice_depends_on_the_image_index_not_on_the_launch(kernel_backend):
    """2 x 3 images of 48 x 80 in one call, and the same images in calls of 1, 2 and 3 images: an image at index i of ITS call gets the
    choice of index i (the entry point has no image base), so the first image of every call agrees with image 0 of the batch - and the
    batch as a whole with the per-image oracle, whatever the grid"""
    key = pack_key(3, 77)
    images = make_images(6, 48, 80, seed=2)
    want = oracle_mask(6, 15, 7, key)
    _, whole, _ = patch_mask(images, 7, key)
    assert np.array_equal(whole, want)
    assert len({tuple(r) for r in want}) == 6                         # six images, six different choices
    for k in (1, 2, 3):
        _, part, _ = patch_mask(images[:k], 7, key)
        assert np.array_equal(part, want[:k])


def test_more_than_1024_patches_is_unsupported(kernel_backend):
    images = np.zeros((1, 1, 528, 512), np.float32)                   # N = 33 * 32 = 1056
    assert patch_mask(images, 1, 0, rc=True) == -2
    with pytest.raises(NotImplementedError):
        raise_for(patch_mask(images, 1, 0, rc=True))


def test_bad_arguments_fail_through_the_error_path(kernel_backend):
    images = np.zeros((1, 1, 32, 32), np.float32)                     # N = 4
    for count in (5, -1):
        assert patch_mask(images, count, 0, rc=True) == -1
    assert patch_mask(np.zeros((1, 1, 15, 32), np.float32), 0, 0, rc=True) == -1      # H < patch
    assert patch_mask(np.zeros((1, 1, 32, 15), np.float32), 0, 0, rc=True) == -1      # W < patch
    m = emu.Z((1, 4))
    assert emu.lib().lp_patch_mask_f32(None, 1, 1, 32, 32, 16, 0, 0, None, m.p, m.p, emu.stream()) == -1
    with pytest.raises(ValueError):
        raise_for(patch_mask(images, 5, 0, rc=True))


def test_every_patch_is_masked_equally_often():
    """The rule alone (the kernel equals it exactly): over steps 0 .. 399 at 2 x 3 images of 15 patches and count 7 every (image, patch) is
    masked with frequency 7 / 15 - over the 2400 draws of one patch the standard deviation of the frequency is
    sqrt(7/15 * 8/15 / 2400) = 0.0102, and 5 of them are 0.051.  The seed is fixed, so this is deterministic."""
    hits = np.zeros(15)
    for step in range(400):
        hits += (oracle_mask(6, 15, 7, pack_key(1234, step)) == 0).sum(0)
    freq = hits / 2400.0
    assert np.abs(freq - 7 / 15).max() < 5 * np.sqrt(7 / 15 * 8 / 15 / 2400), freq
