"""The labeled-frame augmentation from the public surface down: presets, parsing, draws, the dataset / datamodule wiring, images and labels
moving together, a few training steps, kernel resources.  (Operator-by-operator checks: tests/test_labeled_augmentation_kernels.py.)

Images and labels (test_images_and_labels_move_together): 32 seeded draws of the geometric chain of "dlc-top-down" + hflip; the bar is
2 x the worst centroid error of this file's own numpy / scipy chain on the same draws + 0.05 px for fp32.  Measured (emulated build):
restated chain worst 0.1368 px, device path worst 0.1368 px, bar 0.3236 px; 106 keypoints checked, 14 pushed out of the frame (NaN, zero map).
"Border" is the border of the image CONTENT: zero padding moves it inwards, and a blob cut by it (one draw: 1.3 px in both chains) is not measured.
"""

import os
import shutil
import sys

import numpy as np
import pytest
import scipy.ndimage as ndi
import torch

from lightning_pose_amd import _lib, ops
from lightning_pose_amd.data import augmentations as A
from lightning_pose_amd.data.datamodules import BaseDataModule
from lightning_pose_amd.data.datasets import HeatmapDataset
from lightning_pose_amd.data.producers import LabeledBatchProducer
from tests.test_labeled_augmentation_kernels import bilinear_zero_fill, keys_bicubic_zero_fill, philox

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DLC_TAIL = [
    ("MotionBlur", {"p": 0.5, "kwargs": {"k": 5, "angle": (-90, 90)}}),
    ("CoarseDropout", {"p": 0.5, "kwargs": {"p": 0.02, "size_percent": 0.3, "per_channel": 0.5}}),
    ("CoarseSalt", {"p": 0.5, "kwargs": {"p": 0.01, "size_percent": (0.05, 0.1)}}),
    ("CoarsePepper", {"p": 0.5, "kwargs": {"p": 0.01, "size_percent": (0.05, 0.1)}}),
    ("ElasticTransformation", {"p": 0.5, "kwargs": {"alpha": (0, 10), "sigma": 5}}),
    ("AllChannelsHistogramEqualization", {"p": 0.1, "kwargs": {}}),
    ("AllChannelsCLAHE", {"p": 0.1, "kwargs": {}}),
    ("Emboss", {"p": 0.1, "kwargs": {"alpha": (0, 0.5), "strength": (0.5, 1.5)}}),
    ("CropAndPad", {"p": 0.4, "kwargs": {"percent": (-0.15, 0.15), "keep_size": False}}),
]
AFFINE = ("Affine", {"p": 0.4, "kwargs": {"rotate": (-25, 25)}})
GEOMETRIC = {"Affine", "ElasticTransformation", "CropAndPad", "Rot90"}
EXPECTED = {
    "default": [], "none": [],
    "dlc": [AFFINE] + DLC_TAIL,
    "dlc-lr": [("Rot90", {"p": 1.0, "kwargs": {"k": [[0, 2]]}}), AFFINE] + DLC_TAIL,
    "dlc-top-down": [("Rot90", {"p": 1.0, "kwargs": {"k": [[0, 1, 2, 3]]}}), AFFINE] + DLC_TAIL,
    "dlc-mv": [kv for kv in DLC_TAIL if kv[0] not in GEOMETRIC],
}


# ---- 1. presets and parsing -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(EXPECTED))
def test_presets_are_the_references(name):
    got = A.expand_imgaug_str_to_dict(name)
    assert list(got.items()) == EXPECTED[name]       # keys in order, p, kwargs
    pipe = A.imgaug_transform(got)
    assert len(pipe) == len(EXPECTED[name]) and pipe.names == [k for k, _ in EXPECTED[name]]


def test_unknown_things_raise_and_name_the_offender():
    with pytest.raises(NotImplementedError, match="dlc-sideways"):
        A.expand_imgaug_str_to_dict("dlc-sideways")
    with pytest.raises(NotImplementedError, match="Fliplr"):
        A.imgaug_transform({"Fliplr": {"p": 0.5}})
    with pytest.raises(NotImplementedError, match="shear"):
        A.imgaug_transform({"Affine": {"p": 0.5, "kwargs": {"shear": (-5, 5)}}})
    with pytest.raises(NotImplementedError, match="keep_size"):
        A.imgaug_transform({"CropAndPad": {"kwargs": {"percent": (-0.1, 0.1), "keep_size": True}}})
    with pytest.raises(NotImplementedError, match="k="):
        A.imgaug_transform({"MotionBlur": {"kwargs": {"k": 7}}})
    with pytest.raises(NotImplementedError, match="Affine after ElasticTransformation"):     # the keypoint path is affine first, field second
        A.imgaug_transform({"ElasticTransformation": {"kwargs": {"alpha": 10, "sigma": 5}}, "Affine": {"kwargs": {"rotate": (20, 25)}}})
    with pytest.raises(NotImplementedError, match="Rot90 after ElasticTransformation"):
        A.imgaug_transform({"MotionBlur": {"kwargs": {"k": 5}}, "ElasticTransformation": {"kwargs": {"alpha": 10, "sigma": 5}},
                            "Rot90": {"p": 1.0, "kwargs": {"k": [[0, 2]]}}})
    with pytest.raises(NotImplementedError, match="last"):
        A.imgaug_transform({"CropAndPad": {"kwargs": {"percent": 0.1, "keep_size": False}}, "Emboss": {}})
    with pytest.raises(NotImplementedError, match="MotionBlur"):
        A.imgaug_transform({"CoarseSalt": {"kwargs": {"p": 0.1, "size_percent": 0.1}}, "Emboss": {}, "MotionBlur": {"kwargs": {"k": 5}}})
    # parsing rules: p defaults to 0.5, p == 0 drops the operator, one-item lists are the item, two-item lists are ranges
    pipe = A.imgaug_transform({"Emboss": {}, "Affine": {"p": 0, "kwargs": {"rotate": [-5, 5]}}, "Rot90": {"p": 1.0, "kwargs": {"k": [[0, 2]]}}})
    assert pipe.names == ["Emboss", "Rot90"] and pipe.operators[0][1] == 0.5 and pipe.operators[1][2]["k"] == [0, 2]
    assert A.imgaug_transform({"Affine": {"kwargs": {"rotate": [-5, 5]}}}).operators[0][2]["rotate"] == (-5, 5)


def test_get_imgaug_transform():
    cfg = {"training": {"imgaug": "dlc"}, "model": {"model_type": "heatmap"}, "data": {}}
    assert A.get_imgaug_transform(cfg).names == [k for k, _ in EXPECTED["dlc"]]
    mv = {"training": {"imgaug": "dlc"}, "model": {"model_type": "heatmap_multiview_transformer"}, "data": {"camera_params_file": "calib.toml"}}
    pipe = A.get_imgaug_transform(mv)
    assert pipe.names == [k for k, _ in EXPECTED["dlc-mv"]] and not GEOMETRIC & set(pipe.names)
    mv["training"]["imgaug_3d"] = False
    assert "Affine" in A.get_imgaug_transform(mv).names
    assert len(A.get_imgaug_transform({"training": {}, "model": {"model_type": "heatmap"}, "data": {}})) == 0
    assert A.get_imgaug_transform({"training": {"imgaug": {"Emboss": {"p": 1.0}}}, "model": {"model_type": "heatmap"}, "data": {}}).names == ["Emboss"]
    with pytest.raises(TypeError, match="must be str, dict, or DictConfig"):
        A.get_imgaug_transform({"training": {"imgaug": 3}, "model": {"model_type": "heatmap"}, "data": {}})


# ---- a small data set on disk -----------------------------------------------------------------------------------------------------------------
NAMES = ["paw_left", "paw_right", "nose", "tail"]
HS, WS = 150, 203


def blob_image(kps, h=HS, w=WS, sigma=2.0):
    ys, xs = np.mgrid[0:h, 0:w]
    img = np.zeros((h, w))
    for x, y in kps:
        if not np.isnan(x):
            img += 255.0 * np.exp(-((xs + 0.5 - x) ** 2 + (ys + 0.5 - y) ** 2) / (2 * sigma ** 2))
    return np.repeat(np.clip(img, 0, 255).astype(np.uint8)[..., None], 3, -1)


def make_dataset(tmp_path, n, device, textured=True, **kw):
    from PIL import Image

    rng = np.random.default_rng(3)
    base = np.array([[50.0, 40.0], [150.0, 45.0], [60.0, 110.0], [145.0, 105.0]])
    os.makedirs(tmp_path / "img", exist_ok=True)
    rows = ["scorer," + ",".join(["s"] * 8), "bodyparts," + ",".join(f"{k},{k}" for k in NAMES), "coords," + ",".join(["x", "y"] * 4)]
    for i in range(n):
        kp = base + rng.uniform(-8, 8, (4, 2))
        img = blob_image(kp)
        if textured:
            img = np.clip(img.astype(np.int64) + rng.integers(20, 90, img.shape), 0, 255).astype(np.uint8)
        Image.fromarray(img).save(tmp_path / "img" / f"f{i:03d}.png")
        rows.append(f"img/f{i:03d}.png," + ",".join(f"{v:.3f}" for v in kp.reshape(-1)))
    (tmp_path / "labels.csv").write_text("\n".join(rows) + "\n")
    return HeatmapDataset(str(tmp_path), "labels.csv", 128, 128, device=device, **kw)


# ---- 2. no behaviour change ----------------------------------------------------------------------------------------------------------------------
def test_nothing_changes_without_operators(stack_backend, tmp_path):
    plain = make_dataset(tmp_path, 5, stack_backend)
    want = plain.producer(plain.load_images(range(5)).to(stack_backend), plain.keypoints.to(stack_backend), idxs=torch.arange(5),
                          visibility=plain.visibility.to(stack_backend))           # the producer called the way the parent commit calls it
    all_off = {k: {**v, "p": 0} for k, v in A.expand_imgaug_str_to_dict("dlc").items()}
    for tf in (None, A.imgaug_transform(A.expand_imgaug_str_to_dict("default")), A.imgaug_transform(all_off)):
        ds = make_dataset(tmp_path, 5, stack_backend, imgaug_transform=tf)
        assert ds.imgaug_transform is tf
        got = ds.batch(range(5))
        for key in ("images", "keypoints", "heatmaps", "bbox", "idxs"):
            assert torch.equal(got[key].cpu(), want[key].cpu()), key
    # an image whose draw switched every operator off goes through the augmenting launches and still comes out the same
    pipe = A.imgaug_transform(A.expand_imgaug_str_to_dict("dlc"))
    drawn = pipe.draw(5, HS, WS)
    drawn["table"]["flags"] = 0
    drawn["affine"][:] = np.eye(3)
    got = plain.producer(plain.load_images(range(5)).to(stack_backend), plain.keypoints.to(stack_backend), idxs=torch.arange(5),
                         visibility=plain.visibility.to(stack_backend), augment=drawn)
    assert torch.equal(got["images"].cpu(), want["images"].cpu())
    assert torch.allclose(got["keypoints"].cpu(), want["keypoints"].cpu(), atol=1e-4) and torch.equal(got["heatmaps"].cpu() > 0, want["heatmaps"].cpu() > 0)
    # the positional order of the constructor still works
    assert HeatmapDataset(str(tmp_path), "labels.csv", 128, 128, [0, 1, 2], 2, False, False, False, stack_backend).imgaug_transform is None


# ---- 4. images and labels move together --------------------------------------------------------------------------------------------------------
def keys_resize(img, h, w):
    """cubic resize with half-pixel centres and the 4 x 4 taps clamped to the image (OpenCV INTER_CUBIC), fp64"""
    hs, ws = img.shape[:2]
    ys, xs = np.mgrid[0:h, 0:w]
    padded = np.pad(img.astype(np.float64), ((3, 3), (3, 3), (0, 0)), mode="edge")
    return keys_bicubic_zero_fill(padded, (xs + 0.5) * ws / w - 0.5 + 3, (ys + 0.5) * hs / h - 0.5 + 3)


def restated_chain(img, kp, row, fwd, seed, sigma, hflip, swap, size=128):
    """one image and its keypoints through Rot90 / Affine, Elastic, CropAndPad, Resize, hflip in numpy / scipy (fp64)"""
    h, w = img.shape[:2]
    f = int(row["flags"])
    x = img
    pts = (fwd @ np.concatenate([kp, np.ones((len(kp), 1))], 1).T).T[:, :2]
    if f & _lib.AUG_GEOM:
        x = np.clip(np.floor(bilinear_zero_fill(x, fwd) + 0.5), 0, 255)
    if f & _lib.AUG_ELASTIC:
        ys, xs = np.mgrid[0:h, 0:w]
        words = philox(seed, ys * w + xs, int(row["image_id"]) | (_lib.AUG_OP_ELASTIC << 16))
        d = [float(row["elastic_alpha"]) * ndi.gaussian_filter(2.0 * (((wd >> np.uint64(8)).astype(np.float64) + 0.5) / 2 ** 24) - 1.0, sigma,
                                                               mode="mirror", truncate=4.0) for wd in words]
        x = np.clip(np.floor(keys_bicubic_zero_fill(x, xs + d[0], ys + d[1]) + 0.5), 0, 255)
        at = [np.clip(pts[:, 1] - 0.5, 0, h - 1), np.clip(pts[:, 0] - 0.5, 0, w - 1)]
        pts = pts - np.stack([ndi.map_coordinates(d[a], at, order=1, mode="nearest") for a in range(2)], 1)
    top, right, bottom, left = [int(v) for v in row["pad"]] if f & _lib.AUG_CROPPAD else (0, 0, 0, 0)
    x = x[max(-top, 0):h - max(-bottom, 0), max(-left, 0):w - max(-right, 0)]
    x = np.pad(x, ((max(top, 0), max(bottom, 0)), (max(left, 0), max(right, 0)), (0, 0)))
    pts = (pts + [left, top]) / [x.shape[1], x.shape[0]] * size
    x = np.clip(np.floor(keys_resize(x, size, size) + 0.5), 0, 255)
    if hflip:
        x, pts = x[:, ::-1], np.stack([size - pts[:, 0], pts[:, 1]], 1)[swap]
    out = (pts[:, 0] < 0) | (pts[:, 1] < 0) | (pts[:, 0] >= size) | (pts[:, 1] >= size)
    pts[out] = np.nan
    return x, pts


def content_box(row, hflip, size=128):
    """the part of the model frame that shows image content: zero padding moves the image's border inwards"""
    top, right, bottom, left = [int(v) for v in row["pad"]] if int(row["flags"]) & _lib.AUG_CROPPAD else (0, 0, 0, 0)
    hc, wc = HS + top + bottom, WS + left + right
    x_lo, x_hi = max(left, 0) / wc * size, (wc - max(right, 0)) / wc * size
    if hflip:
        x_lo, x_hi = size - x_hi, size - x_lo
    return x_lo, max(top, 0) / hc * size, x_hi, (hc - max(bottom, 0)) / hc * size


def centroid_errors(img, pts, box, size=128, margin=6, radius=7):
    """only keypoints more than `margin` model px from the border of the image content (a blob cut by that border has no centroid to speak of)"""
    errs = []
    ys, xs = np.mgrid[0:size, 0:size]
    for x, y in pts:
        if np.isnan(x) or min(x - box[0], y - box[1], box[2] - x, box[3] - y) <= margin:
            continue
        win = ((xs + 0.5 - x) ** 2 + (ys + 0.5 - y) ** 2 <= radius ** 2) * img[..., 0].astype(np.float64)
        assert win.sum() > 0, (x, y)
        errs.append(float(np.hypot((win * (xs + 0.5)).sum() / win.sum() - x, (win * (ys + 0.5)).sum() / win.sum() - y)))
    return errs


def test_images_and_labels_move_together(stack_backend):
    geo = {k: v for k, v in A.expand_imgaug_str_to_dict("dlc-top-down").items() if k in GEOMETRIC}
    assert list(geo) == ["Rot90", "Affine", "ElasticTransformation", "CropAndPad"]
    geo["Affine"]["p"] = geo["ElasticTransformation"]["p"] = geo["CropAndPad"]["p"] = 0.8      # (more of the 32 draws exercise each operator)
    pipe = A.imgaug_transform(geo, seed=11)
    swap = [1, 0, 2, 3]
    prod = LabeledBatchProducer(128, 128, hflip_swap_indices=swap)
    rng = np.random.default_rng(5)
    mean, std = np.array(prod.mean), np.array(prod.std)
    worst_dev, worst_ref, n_nan, n_checked = 0.0, 0.0, 0, 0
    for _ in range(4):
        kp = np.array([[50.0, 40.0], [150.0, 45.0], [60.0, 110.0], [145.0, 105.0]])[None] + rng.uniform(-8, 8, (8, 4, 2))
        kp[:, 3] = np.where(rng.random((8, 1)) < 0.5, [[196.0, 143.0]], kp[:, 3])     # near the corner: rotations and crops push it out
        imgs = np.stack([blob_image(k) for k in kp])
        hflip = rng.random(8) < 0.5
        drawn = pipe.draw(8, HS, WS)
        got = prod(torch.from_numpy(imgs).to(stack_backend), torch.from_numpy(kp.astype(np.float32)).to(stack_backend),
                   hflip=torch.from_numpy(hflip), augment=drawn)
        out = np.floor((got["images"].cpu().numpy().transpose(0, 2, 3, 1) * std + mean) * 255.0 + 0.5)
        kps, hms = got["keypoints"].cpu().numpy().reshape(8, 4, 2), got["heatmaps"].cpu().numpy()
        for i in range(8):
            ref_img, ref_pts = restated_chain(imgs[i], kp[i], drawn["table"][i], drawn["affine"][i], drawn["seed"], 5.0, hflip[i], swap)
            assert np.array_equal(np.isnan(ref_pts), np.isnan(kps[i])), i
            both = ~np.isnan(ref_pts[:, 0])
            if both.any():
                assert np.abs(ref_pts[both] - kps[i][both]).max() < 1e-3, i      # the two keypoint chains agree
            box = content_box(drawn["table"][i], hflip[i])
            worst_ref = max([worst_ref] + centroid_errors(ref_img, ref_pts, box))
            errs = centroid_errors(out[i], kps[i], box)
            worst_dev = max([worst_dev] + errs)
            n_checked += len(errs)
            for k in range(4):
                if np.isnan(kps[i, k, 0]):
                    n_nan += 1
                    assert not hms[i, k].any()          # pushed out of the frame: NaN and an all-zero target
                else:
                    assert hms[i, k].max() > 0.05
    bar = 2.0 * worst_ref + 0.05
    print(f"centroid error: restated chain worst = {worst_ref:.4f} px, device worst = {worst_dev:.4f} px, bar = {bar:.4f} px; "
          f"{n_checked} keypoints checked, {n_nan} out of frame")
    assert n_nan >= 1 and n_checked >= 80
    assert worst_dev <= bar, (worst_dev, bar)


# ---- 5. draws ------------------------------------------------------------------------------------------------------------------------------------
def test_draw_statistics_and_reproducibility(stack_backend, monkeypatch):
    spec = A.expand_imgaug_str_to_dict("dlc")
    pipe = A.imgaug_transform(spec, seed=7)
    d = pipe.draw(4000, HS, WS)
    raw, flags = d["raw"], d["table"]["flags"]
    for name, v in spec.items():
        n, p = int(np.nansum(raw[name])), v["p"]
        assert abs(n - 4000 * p) <= 4 * np.sqrt(4000 * p * (1 - p)), (name, n)
    ranges = {"Affine.rotate": (-25, 25), "MotionBlur.angle": (-90, 90), "MotionBlur.direction": (-1, 1), "CoarseDropout.p": (0.02, 0.02),
              "CoarseDropout.size_percent": (0.3, 0.3), "CoarseSalt.p": (0.01, 0.01), "CoarseSalt.size_percent": (0.05, 0.1),
              "CoarsePepper.p": (0.01, 0.01), "CoarsePepper.size_percent": (0.05, 0.1), "ElasticTransformation.alpha": (0, 10), "AllChannelsCLAHE.clip_limit": (0.1, 8),
              "AllChannelsCLAHE.tile_grid_size_px": (3, 12), "Emboss.alpha": (0, 0.5), "Emboss.strength": (0.5, 1.5),
              "CropAndPad.top": (-0.15, 0.15), "CropAndPad.left": (-0.15, 0.15), "CropAndPad.right": (-0.15, 0.15), "CropAndPad.bottom": (-0.15, 0.15)}
    for key, (lo, hi) in ranges.items():
        v = raw[key][~np.isnan(raw[key])]
        assert len(v) > 100 and v.min() >= lo and v.max() <= hi, key
        if hi > lo:
            assert v.max() - v.min() > 0.8 * (hi - lo), key
    pc = raw["CoarseDropout.per_channel"]
    pc = pc[~np.isnan(pc)]
    assert abs(pc.sum() - 0.5 * len(pc)) <= 4 * np.sqrt(0.25 * len(pc))
    assert ((flags & _lib.AUG_DROP_PER_CHANNEL) != 0).sum() == pc.sum()
    on = (flags & _lib.AUG_CROPPAD) != 0
    assert np.abs(d["table"]["pad"][on]).max() <= round(0.15 * WS) and not d["table"]["pad"][~on].any()
    # same seed: the same table and the same images, twice; another rank: another table; a kept draw replays bit for bit
    rng = np.random.default_rng(0)
    imgs = torch.from_numpy(rng.integers(0, 255, (4, HS, WS, 3), dtype=np.uint8)).to(stack_backend)
    kp = torch.from_numpy(rng.uniform(20, 130, (4, 8)).astype(np.float32)).to(stack_backend)
    prod = LabeledBatchProducer(128, 128)
    runs = []
    for _ in range(2):
        p2 = A.imgaug_transform(spec, seed=7)
        d2 = p2.draw(4, HS, WS)
        runs.append((d2, prod(imgs, kp, augment=d2)))
    assert runs[0][0]["table"].tobytes() == runs[1][0]["table"].tobytes() and runs[0][0]["seed"] == runs[1][0]["seed"]
    for key in ("images", "keypoints", "heatmaps"):
        assert torch.equal(runs[0][1][key], runs[1][1][key]), key
    assert runs[0][0]["table"]["flags"].any()
    replay = prod(imgs, kp, augment=runs[0][0])
    assert torch.equal(replay["images"], runs[0][1]["images"]) and torch.equal(replay["keypoints"], runs[0][1]["keypoints"])
    monkeypatch.setenv("LOCAL_RANK", "1")
    other = A.imgaug_transform(spec, seed=7).draw(4, HS, WS)
    assert other["table"].tobytes() != runs[0][0]["table"].tobytes() and other["seed"] != runs[0][0]["seed"]


# ---- 6. splits -----------------------------------------------------------------------------------------------------------------------------------
def test_only_the_training_loader_augments(stack_backend, tmp_path):
    spec = {k: {**v, "p": 1.0} for k, v in A.expand_imgaug_str_to_dict("dlc").items() if k in ("MotionBlur", "Affine", "Emboss")}
    aug = make_dataset(tmp_path, 20, stack_backend, imgaug_transform=A.imgaug_transform(spec, seed=1))
    plain = make_dataset(tmp_path, 20, stack_backend)
    dm = BaseDataModule(aug, train_batch_size=4, val_batch_size=2, test_batch_size=1, train_probability=0.5, val_probability=0.25)
    for loader, idx in ((dm.val_dataloader(), dm.val_dataset.indices), (dm.test_dataloader(), dm.test_dataset.indices),
                        (dm.full_labeled_dataloader(), list(range(20)))):
        got = list(loader)
        assert torch.equal(torch.cat([g["idxs"] for g in got]), torch.as_tensor(list(idx)))
        for g in got:
            want = plain.batch(g["idxs"].tolist())
            assert torch.equal(g["images"], want["images"]) and torch.equal(g["keypoints"], want["keypoints"]) and torch.equal(g["heatmaps"], want["heatmaps"])
    n = 0
    for g in dm.train_dataloader():
        want = plain.batch(g["idxs"].tolist())
        assert not torch.equal(g["images"], want["images"]) and not torch.equal(g["keypoints"], want["keypoints"])
        assert torch.isfinite(g["images"]).all()
        n += len(g["idxs"])
    assert n == len(dm.train_dataset.indices) == 10


# ---- 7. end to end ---------------------------------------------------------------------------------------------------------------------------------
def test_three_training_steps_on_augmented_batches(stack_backend, tmp_path):
    from lightning_pose_amd.losses import LossFactory
    from lightning_pose_amd.models import HeatmapTracker

    gpu = stack_backend.type == "cuda"
    from PIL import Image  # noqa: F401  (make_dataset writes PNG files)

    ds = make_dataset(tmp_path, 8, stack_backend, imgaug_transform=A.imgaug_transform(A.expand_imgaug_str_to_dict("dlc"), seed=2))
    if gpu:
        ds.producer = LabeledBatchProducer(256, 256)
    dm = BaseDataModule(ds, train_batch_size=4, train_probability=0.75, val_probability=0.125)
    model = HeatmapTracker(num_keypoints=4, loss_factory=LossFactory({"heatmap_mse": {"log_weight": 0.0}}, None), pretrained=False, torch_seed=0,
                           device=stack_backend)
    model.train()
    opt = model.configure_optimizers()["optimizer"]
    steps = 0
    while steps < 3:
        for batch in dm.train_dataloader():
            opt.zero_grad()
            loss = model.training_step(batch, steps)["loss"]
            loss.backward()
            opt.step()
            assert torch.isfinite(loss).item()
            assert torch.isfinite(model.net.G).all() and float(model.net.G.abs().sum()) > 0
            steps += 1
            if steps == 3:
                break
    mv = A.imgaug_transform(A.expand_imgaug_str_to_dict("dlc-mv"))
    assert len(mv) == 7 and not GEOMETRIC & set(mv.names) and "geom" not in mv.stages and "elastic" not in mv.stages


# ---- 8. resources --------------------------------------------------------------------------------------------------------------------------------
SO = os.path.join(ROOT, "lightning-pose_amd", "liblp_hip.so")
LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin")


@pytest.mark.skipif(not (os.path.exists(SO) and os.path.exists(os.path.join(LLVM, "llvm-readelf")) and shutil.which("c++filt")),
                    reason="needs the built liblp_hip.so and the ROCm LLVM tools")
def test_no_labelaug_kernel_uses_scratch():
    sys.path.insert(0, os.path.join(ROOT, "profiles"))
    try:
        import kernel_resources as KR
    finally:
        sys.path.pop(0)
    ks = [k for k in KR.kernels(SO) if k["name"].startswith("lp::labelaug_")]
    names = {k["name"].split("(")[0] for k in ks}
    assert len(names) >= 11, names
    bad = [(k["name"], k["scratch"], k["vgpr_spill"]) for k in ks if k["scratch"] or k["vgpr_spill"]]
    assert not bad, bad
