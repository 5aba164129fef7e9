"""MultiviewHeatmapDataset / CameraGroup / MultiviewLabeledBatchProducer on a 3-view, 6-frame dataset written into tmp_path: PNGs with a bright
blob at every label, DLC label files, an anipose calibration from a synthetic rig, one view with a bounding-box file.  Runs on the CPU build of
the kernels and, under ``-m gpu``, on the device."""

import os
import shutil

import numpy as np
import pandas as pd
import pytest
import torch
from PIL import Image

from tests import cameras_fp64 as O

VIEWS = ["top", "side", "front"]
KP = ["nose", "ear", "paw", "hip", "knee", "tail"]
N, K, V = 6, len(KP), len(VIEWS)
H, W = 128, 256
FRAME_HW = [(256, 320), (256, 320), (240, 336)]          # the cameras' full frames (height, width)
BBOX_SIDE = (32.0, 24.0, 200.0, 260.0)                    # x, y, h, w: view "side" is stored as this crop ...
STORED_HW = [(256, 320), (100, 130), (240, 336)]          # ... at half its size
BG, RADIUS = 30, 2


def _rotvec(R: np.ndarray) -> np.ndarray:
    """the rotation vector of a rotation matrix (angle well inside (0, pi))"""
    th = np.arccos(np.clip((np.trace(R) - 1.0) / 2.0, -1.0, 1.0))
    return th / (2.0 * np.sin(th)) * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])


def _rig():
    """one synthetic rig of tests/cameras_fp64.make_rig; its focal lengths and principal points are set for the small frames above: a
    point 1.2 units off the axis at the camera's distance from the origin lands 0.15 of the frame's width off the centre"""
    rig = O.make_rig(1, V, K, 5, seed=5)
    intr = rig["intrinsics"][0].clone()
    for v, (fh, fw) in enumerate(FRAME_HW):
        f = 0.15 * fw * float(rig["extrinsics"][0, v, :, 3].norm()) / 1.2
        intr[v, 0, 0], intr[v, 1, 1] = f, f * float(intr[v, 1, 1] / intr[v, 0, 0])
        intr[v, 0, 2], intr[v, 1, 2] = fw / 2.0 + 3.0 * v, fh / 2.0 - 2.0 * v
    return intr, rig["extrinsics"][0], rig["distortions"][0] * 0.5


def _toml(intr, extr, dist) -> str:
    out = []
    for v, name in enumerate(VIEWS):
        fmt = lambda a: "[" + ", ".join(repr(float(x)) for x in a) + "]"  # noqa: E731
        out += [f"[cam_{v}]", f'name = "{name}"', f"size = [{FRAME_HW[v][1]}, {FRAME_HW[v][0]}]",
                "matrix = [" + ", ".join(fmt(r) for r in intr[v].numpy()) + "]", f"distortions = {fmt(dist[v].numpy())}",
                f"rotation = {fmt(_rotvec(extr[v, :, :3].numpy()))}", f"translation = {fmt(extr[v, :, 3].numpy())}", ""]
    out += ["[metadata]", "adjusted = false", 'error = 0.0', ""]
    return "\n".join(out)


def _blob_image(hs, ws, labels):
    yy, xx = np.mgrid[0:hs, 0:ws].astype(np.float64)
    img = np.full((hs, ws), float(BG))
    for lx, ly in labels:
        if np.isnan(lx):
            continue
        near = (np.abs(xx - np.round(lx)) <= RADIUS) & (np.abs(yy - np.round(ly)) <= RADIUS)             # a 5 x 5 px blob
        img = np.where(near, np.maximum(img, BG + (255 - BG) * np.exp(-((xx - lx) ** 2 + (yy - ly) ** 2) / (2 * 1.2 ** 2))), img)
    return np.repeat(np.round(img).astype(np.uint8)[:, :, None], 3, axis=2)


def write_dataset(root, calibration=True, seed=3):
    """-> dict(labels (N, V, K, 2) stored px, X (N, K, 3), bbox (N, 4 V), rig)"""
    g = torch.Generator().manual_seed(seed)
    intr, extr, dist = _rig()
    spread = torch.tensor([[1.2, 0.4, 0.6], [-1.0, 0.9, -0.5], [0.3, -1.2, 0.9], [-0.6, -0.8, -1.0], [0.9, -0.3, -0.9], [-0.2, 1.1, 1.0]], dtype=torch.float64)
    X = spread + (torch.rand(N, K, 3, generator=g, dtype=torch.float64) - 0.5) * 0.4      # well apart in every view, another pose per frame
    frame_px = O.project(X, intr[None].repeat(N, 1, 1, 1), extr[None].repeat(N, 1, 1, 1), dist[None].repeat(N, 1, 1))    # (N, V, K, 2)
    bbox = torch.zeros(N, V, 4, dtype=torch.float64)
    for v in range(V):
        bbox[:, v] = torch.tensor(BBOX_SIDE if VIEWS[v] == "side" else (0.0, 0.0, float(FRAME_HW[v][0]), float(FRAME_HW[v][1])))
    hs = torch.tensor([float(s[0]) for s in STORED_HW])[None, :, None]
    ws = torch.tensor([float(s[1]) for s in STORED_HW])[None, :, None]
    labels = torch.stack([(frame_px[..., 0] - bbox[..., 0:1]) / bbox[..., 3:4] * ws, (frame_px[..., 1] - bbox[..., 1:2]) / bbox[..., 2:3] * hs], -1)
    labels[1, 2, 4] = float("nan")                       # one unlabeled point
    labels[4, 0, 1] = float("nan")
    labels = labels.float().double()                     # (the label files keep float32 precision)
    os.makedirs(os.path.join(root, "calibrations"), exist_ok=True)
    for v, view in enumerate(VIEWS):
        folder = os.path.join("labeled-data", f"sess_{view}")
        os.makedirs(os.path.join(root, folder), exist_ok=True)
        names = [f"{folder}/img{i:03d}.png" for i in range(N)]
        for i in range(N):
            Image.fromarray(_blob_image(*STORED_HW[v], labels[i, v].numpy())).save(os.path.join(root, names[i]))
        cols = pd.MultiIndex.from_product([["scorer"], KP, ["x", "y"]], names=["scorer", "bodyparts", "coords"])
        pd.DataFrame(labels[:, v].reshape(N, 2 * K).numpy(), index=names, columns=cols).to_csv(os.path.join(root, f"{view}.csv"))
        if view == "side":
            pd.DataFrame(np.tile(np.array(BBOX_SIDE), (N, 1)), index=names, columns=["x", "y", "h", "w"]).to_csv(os.path.join(root, "bbox_side.csv"))
    if calibration:
        with open(os.path.join(root, "calibrations", "sess.toml"), "w") as f:
            f.write(_toml(intr, extr, dist))
    return dict(labels=labels, X=X, bbox=bbox.reshape(N, 4 * V), rig=(intr, extr, dist))


def make_dataset(root, dev, **kw):
    from lightning_pose_amd.data.datasets import MultiviewHeatmapDataset

    args = dict(root_directory=str(root), csv_paths=[f"{v}.csv" for v in VIEWS], view_names=VIEWS, image_resize_height=H, image_resize_width=W,
                bbox_paths=[None, "bbox_side.csv", None], device=dev)
    args.update(kw)
    return MultiviewHeatmapDataset(**args)


@pytest.fixture(scope="module")
def disk(tmp_path_factory):
    root = tmp_path_factory.mktemp("mv3d")
    plain = tmp_path_factory.mktemp("mv3d_plain")
    return dict(root=root, truth=write_dataset(str(root)), plain=plain, plain_truth=write_dataset(str(plain), calibration=False))


# ---- the classes ------------------------------------------------------------------------------------------------------------------
def test_rodrigues_against_known_rotations():
    from lightning_pose_amd.data.cameras import rodrigues_to_matrix

    assert np.allclose(rodrigues_to_matrix([0, 0, np.pi / 2]), [[0, -1, 0], [1, 0, 0], [0, 0, 1]], atol=1e-15)
    assert np.allclose(rodrigues_to_matrix(np.ones(3) * 2 * np.pi / 3 / np.sqrt(3)), [[0, 0, 1], [1, 0, 0], [0, 1, 0]], atol=1e-15)
    assert np.array_equal(rodrigues_to_matrix([0, 0, 0]), np.eye(3))
    R = rodrigues_to_matrix([0.3, -0.2, 0.9])
    assert np.allclose(R @ R.T, np.eye(3), atol=1e-15) and np.isclose(np.linalg.det(R), 1.0) and np.allclose(_rotvec(R), [0.3, -0.2, 0.9])


def test_camera_group_reads_the_calibration(disk, stack_backend):
    from lightning_pose_amd.data.cameras import CameraGroup

    intr, extr, dist = disk["truth"]["rig"]
    cg = CameraGroup.load(os.path.join(disk["root"], "calibrations", "sess.toml"), device=stack_backend)
    assert cg.get_names() == VIEWS and len(cg.cameras) == V
    for v, cam in enumerate(cg.cameras):
        assert np.allclose(cam.get_camera_matrix(), intr[v].numpy(), atol=1e-12) and np.allclose(cam.get_distortions(), dist[v].numpy(), atol=1e-15)
        E = cam.get_extrinsics_mat()
        assert E.shape == (4, 4) and np.allclose(E[:3], extr[v].numpy(), atol=1e-9) and np.array_equal(E[3], [0, 0, 0, 1])
    # project and triangulate_fast: the reference's shapes, the oracle's values
    X = disk["truth"]["X"][0]
    p2 = cg.project(X.numpy())
    want = O.project(X[None], intr[None], extr[None], dist[None])[0].numpy()
    assert p2.shape == (V, K, 2) and np.abs(p2 - want).max() <= 1e-3          # (fp32 pixels of a few hundred: 3e-5 per ulp)
    back = cg.triangulate_fast(p2)
    assert back.shape == (K, 3) and np.abs(back - X.numpy()).max() <= 1e-3
    p2[1, 2] = np.nan                                                         # one view less for one keypoint; one keypoint seen by one view only
    p2[1:, 4] = np.nan
    back = cg.triangulate_fast(p2)
    assert np.isnan(back[4]).all() and np.abs(np.delete(back, 4, 0) - np.delete(X.numpy(), 4, 0)).max() <= 1e-3
    assert cg.triangulate_fast(p2[:, 0]).shape == (3,)
    many = np.tile(p2, (1, 40, 1))                                            # more points than one workgroup takes
    assert np.array_equal(cg.triangulate_fast(many)[:K], back, equal_nan=True) and cg.triangulate_fast(many).shape == (40 * K, 3)


def test_dataset_attributes_and_checks(disk, stack_backend):
    from lightning_pose_amd.data.cameras import CameraGroup
    from lightning_pose_amd.data.datasets import HeatmapDataset

    ds = make_dataset(disk["root"], stack_backend)
    assert list(ds.dataset) == VIEWS and all(isinstance(d, HeatmapDataset) for d in ds.dataset.values())
    assert ds.keypoint_names == {v: KP for v in VIEWS}
    assert (ds.num_keypoints, ds.num_targets, ds.num_views, ds.data_length, len(ds)) == (V * K, 2 * V * K, V, N, N)
    assert (ds.height, ds.width, ds.output_shape, ds.imgaug_hflip, ds.do_context) == (H, W, (H // 4, W // 4), False, False)
    assert list(ds.cam_params_df.file) == [os.path.join("calibrations", "sess.toml")] * N                     # found by session
    assert list(ds.cam_params_file_to_camgroup) == [os.path.join("calibrations", "sess.toml")]
    assert isinstance(ds.cam_params_file_to_camgroup[os.path.join("calibrations", "sess.toml")], CameraGroup)
    # the fall-back file, and a CSV that maps the frames to files
    other = str(disk["root"]) + "_fallback"
    shutil.copytree(disk["root"], other)
    shutil.move(os.path.join(other, "calibrations", "sess.toml"), os.path.join(other, "calibration.toml"))
    fb = make_dataset(other, stack_backend)
    assert list(fb.cam_params_df.file) == ["calibration.toml"] * N
    pd.DataFrame({"file": ["calibration.toml"] * N}, index=fb.dataset["top"].image_names).to_csv(os.path.join(other, "cams.csv"))
    assert list(make_dataset(other, stack_backend, camera_params_path=os.path.join(other, "cams.csv")).cam_params_file_to_camgroup) == ["calibration.toml"]
    # without any calibration: both None
    plain = make_dataset(disk["plain"], stack_backend)
    assert plain.cam_params_df is None and plain.cam_params_file_to_camgroup is None
    # the reference's refusals
    with pytest.raises(ValueError, match="number of names does not match"):
        make_dataset(disk["root"], stack_backend, view_names=VIEWS[:2])
    with pytest.raises(NotImplementedError):
        make_dataset(disk["root"], stack_backend, do_context=True)
    with pytest.raises(AssertionError, match="same camera order"):
        make_dataset(disk["root"], stack_backend, view_names=["top", "front", "side"], csv_paths=["top.csv", "front.csv", "side.csv"],
                     bbox_paths=None)
    with pytest.raises(FileNotFoundError, match="Could not find bbox file"):
        make_dataset(disk["root"], stack_backend, bbox_paths=[None, "nowhere.csv", None])
    short = pd.read_csv(os.path.join(other, "front.csv"), header=[0, 1, 2], index_col=0)
    short.iloc[:-1].to_csv(os.path.join(other, "front_short.csv"))
    with pytest.raises(ImportError, match="do not match in row numbers"):
        make_dataset(other, stack_backend, csv_paths=["top.csv", "side.csv", "front_short.csv"])
    swapped = short.copy()
    swapped.columns = pd.MultiIndex.from_product([["scorer"], KP[::-1], ["x", "y"]], names=short.columns.names)
    swapped.to_csv(os.path.join(other, "front_swapped.csv"))
    with pytest.raises(ImportError, match="not in correct order"):
        make_dataset(other, stack_backend, csv_paths=["top.csv", "side.csv", "front_swapped.csv"])
    renamed = short.copy()
    renamed.index = [n.replace("img003", "img103") for n in renamed.index]
    renamed.to_csv(os.path.join(other, "front_renamed.csv"))
    with pytest.raises(ImportError, match="Discrepancy in image file names"):
        make_dataset(other, stack_backend, csv_paths=["top.csv", "side.csv", "front_renamed.csv"])
    with pytest.raises(ValueError, match="not supported for multi-view"):
        ds.batch([0, 1], hflip=torch.tensor([True, False]))


PARAMS = np.array([[1.15, 0.3, -0.2, 0.3], [0.85, -0.3, 0.2, -0.2], [1.1, 0.1, 0.3, 0.2]], np.float32)
IDX = [0, 1, 4]


def test_batch_keys_shapes_and_dtypes(disk, stack_backend):
    from lightning_pose_amd.data.datatypes import MultiviewHeatmapLabeledBatchDict

    ds = make_dataset(disk["root"], stack_backend)
    batch = ds.batch(IDX, params=PARAMS)
    B = len(IDX)
    assert set(batch) == set(MultiviewHeatmapLabeledBatchDict.__annotations__)
    want = dict(images=(B, V, 3, H, W), keypoints=(B, 2 * V * K), heatmaps=(B, V * K, H // 4, W // 4), bbox=(B, 4 * V), idxs=(B,), num_views=(B,),
                keypoints_3d=(B, K, 3), intrinsic_matrix=(B, V, 3, 3), extrinsic_matrix=(B, V, 3, 4), distortions=(B, V, 5))
    for name, shape in want.items():
        assert tuple(batch[name].shape) == shape, name
        if name not in ("idxs", "num_views"):
            assert batch[name].dtype == torch.float32 and batch[name].device.type == stack_backend.type, name
    assert batch["idxs"].tolist() == IDX and batch["num_views"].tolist() == [V] * B
    assert batch["concat_order"] == VIEWS == batch["view_names"]
    assert torch.equal(batch["bbox"].cpu(), disk["truth"]["bbox"][IDX].float())
    assert ds.producer.last_plan["status"].tolist() == [0, 0, 0]
    assert torch.isfinite(batch["images"]).all() and torch.isfinite(batch["keypoints_3d"]).all()
    # the unlabeled point of frame 1 is reprojected; its target stays empty, as its visibility says (reference :1099)
    kp = batch["keypoints"].reshape(B, V, K, 2)
    assert torch.isfinite(kp).all()
    assert not batch["heatmaps"].reshape(B, V, K, -1)[1, 2, 4].any() and batch["heatmaps"].reshape(B, V, K, -1)[1, 2, 3].any()
    # the same params give the same batch bit for bit; other params another one
    again = ds.batch(IDX, params=PARAMS)
    for name in want:
        assert torch.equal(batch[name], again[name]), name
    assert not torch.equal(ds.batch(IDX, params=PARAMS[::-1].copy())["images"], batch["images"])
    # drawn on the host from the seeded generator: scale in (0.8, 1.2), the shifts in (-1, 1)
    d = ds.producer.draw(1000)
    assert d.shape == (1000, 4) and d.dtype == np.float32 and 0.8 <= d[:, 0].min() < 0.82 and 1.18 < d[:, 0].max() <= 1.2
    assert -1 <= d[:, 1:].min() < -0.98 and 0.98 < d[:, 1:].max() <= 1


def test_placeholders_without_calibration(disk, stack_backend):
    ds = make_dataset(disk["plain"], stack_backend)
    batch = ds.batch(IDX)
    B = len(IDX)
    assert torch.equal(batch["keypoints_3d"].cpu(), torch.ones(B, 1))                                   # the reference's tensor([1]) per sample
    assert torch.equal(batch["intrinsic_matrix"].cpu(), torch.eye(3).repeat(B, 1, 1, 1))
    assert torch.equal(batch["extrinsic_matrix"].cpu(), torch.zeros(B, 1, 3, 4)) and torch.equal(batch["distortions"].cpu(), torch.zeros(B, 1, 5))
    assert tuple(batch["images"].shape) == (B, V, 3, H, W) and ds.producer.last_plan is None


def test_without_augmentation_every_view_is_the_heatmap_dataset(disk, stack_backend):
    from lightning_pose_amd.data.datasets import HeatmapDataset

    ds = make_dataset(disk["root"], stack_backend)
    batch = ds.batch(IDX, augment=False)
    B = len(IDX)
    for v, view in enumerate(VIEWS):
        one = HeatmapDataset(str(disk["root"]), f"{view}.csv", H, W, device=stack_backend).batch(IDX)
        assert torch.equal(batch["images"][:, v], one["images"]), view
        assert torch.equal(batch["keypoints"].reshape(B, V, 2 * K)[:, v].view(torch.int32), one["keypoints"].view(torch.int32)), view   # (NaN kept)
        assert torch.equal(batch["heatmaps"].reshape(B, V, K, H // 4, W // 4)[:, v], one["heatmaps"]), view
    # keypoints_3d: the plain triangulation - against the float64 oracle, allowed 4 x the float32 oracle's own distance from it
    truth = disk["truth"]
    intr, extr, dist = (t[None].repeat(B, *([1] * t.dim())) for t in truth["rig"])
    bb = truth["bbox"][IDX].reshape(B, V, 4)
    hs = torch.tensor([float(s[0]) for s in STORED_HW])[None, :, None].double()
    ws = torch.tensor([float(s[1]) for s in STORED_HW])[None, :, None].double()
    lab = truth["labels"][IDX]
    pts = torch.stack([lab[..., 0] / ws * bb[..., 3:4] + bb[..., 0:1], lab[..., 1] / hs * bb[..., 2:3] + bb[..., 1:2]], -1)
    want = torch.from_numpy(np.nanmedian(O.triangulate_pairs(pts, intr, extr, dist).numpy(), axis=1))
    f32 = torch.from_numpy(np.nanmedian(O.triangulate_pairs(pts.float(), intr.float(), extr.float(), dist.float()).numpy(), axis=1)).double()
    err, ref = float((batch["keypoints_3d"].double().cpu() - want).abs().max()), float((f32 - want).abs().max())
    print(f"plain triangulation: kernel {err:.3g}  float32 oracle {ref:.3g}  largest value {float(want.abs().max()):.3g}")
    assert err <= max(4 * ref, 1e-6 * float(want.abs().max()))
    assert float((want - truth["X"][IDX]).abs().max()) < 1e-2                          # (and the oracle finds the points the labels were made from)


def test_the_warped_blobs_sit_where_the_similarity_puts_the_labels(disk, stack_backend):
    """an inverted or transposed M, a wrong bbox or a swapped axis moves every blob by many pixels"""
    ds = make_dataset(disk["root"], stack_backend)
    batch = ds.batch(IDX, params=PARAMS)
    M = ds.producer.last_plan["affine"].double().cpu()                      # (B, V, 2, 3) stored px -> warped px
    assert ds.producer.last_plan["status"].tolist() == [0, 0, 0]
    assert float((M - torch.tensor([[1.0, 0, 0], [0, 1.0, 0]])).abs().max()) > 3.0     # the draws move the image by pixels
    lab = disk["truth"]["labels"][IDX]
    img = batch["images"][:, :, 0].double().cpu()                           # one channel (the three are equal up to the normalisation)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    worst, checked = 0.0, 0
    for b in range(len(IDX)):
        for v in range(V):
            hs, ws = STORED_HW[v]
            warped = torch.einsum("rc,kc->kr", M[b, v, :, :2], lab[b, v]) + M[b, v, :, 2]                 # (K, 2) stored px of the warped image
            model = torch.stack([warped[:, 0] / ws * W, warped[:, 1] / hs * H], -1)
            ok = ~torch.isnan(model).any(-1)
            # precondition: every labeled blob stays inside the frame, clear of the border and of the other blobs of its view
            assert bool(((model[ok, 0] > 8) & (model[ok, 0] < W - 8) & (model[ok, 1] > 8) & (model[ok, 1] < H - 8)).all()), (b, v, model)
            dist = torch.cdist(model[ok], model[ok]) + 1e9 * torch.eye(int(ok.sum()), dtype=torch.float64)
            assert float(dist.min()) > 12.0, (b, v, float(dist.min()))
            background = img[b, v].min()
            for k in torch.nonzero(ok).flatten().tolist():
                near = ((xx - model[k, 0]).abs() <= 6) & ((yy - model[k, 1]).abs() <= 6)
                wgt = (img[b, v] - background) * near
                assert float(wgt.max()) > 0.5 * float(img[b, v].max() - background), (b, v, k)           # the blob is there at all
                cx, cy = float((wgt * xx).sum() / wgt.sum()), float((wgt * yy).sum() / wgt.sum())
                worst = max(worst, float(np.hypot(cx - float(model[k, 0]), cy - float(model[k, 1]))))
                checked += 1
    print(f"blob centroids: {checked} blobs, largest distance from M . label {worst:.3f} model px")
    assert checked == len(IDX) * V * K - 2 and worst <= 0.75


def test_it_runs_through_the_data_module(disk, stack_backend):
    from lightning_pose_amd.data.augmentations import imgaug_transform
    from lightning_pose_amd.data.datamodules import BaseDataModule

    ds = make_dataset(disk["root"], stack_backend, imgaug_transform=imgaug_transform({"MotionBlur": {"p": 1.0, "kwargs": {"k": 5, "angle": (-90, 90)}}}))
    dm = BaseDataModule(ds, train_batch_size=2, val_batch_size=1, train_probability=0.67, val_probability=0.17, torch_seed=1)
    seen = 0
    for batch in dm.train_dataloader():
        b = len(batch["idxs"])
        assert tuple(batch["images"].shape) == (b, V, 3, H, W) and tuple(batch["keypoints_3d"].shape) == (b, K, 3)
        assert ds.producer.last_plan is not None                             # training batches are augmented in 3-D ...
        seen += b
    assert seen == len(dm.train_dataset)
    for batch in dm.val_dataloader():
        assert tuple(batch["images"].shape) == (1, V, 3, H, W) and ds.producer.last_plan is None        # ... validation batches are not
