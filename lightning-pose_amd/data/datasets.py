"""Labeled dataset for the heatmap trackers: DLC-style label files + image files in, device-built labeled batches out.

Mirror of the part of ``lightning_pose/data/datasets.py`` (``BaseTrackingDataset`` :78-376, ``HeatmapDataset`` :380-550) and
``lightning_pose/utils/io.py`` (``parse_label_csv`` :208-279, ``LabeledData`` :190-205) that the labeled half of the training step
consumes - same constructor arguments, attributes (``keypoints``, ``visibility``, ``image_names``, ``keypoint_names``, ``num_keypoints``,
``num_targets``, ``height`` / ``width``, ``output_shape``, ``output_sigma``) and label-file semantics (three-row DLC header, optional
``visible`` column with values 0 / 1 / 2, an all-NaN first row is a data row, visibility synthesised from NaN labels otherwise).

What differs is where the work happens: the reference transforms one sample at a time in DataLoader workers (PIL -> imgaug -> ToTensor ->
Normalize -> ``generate_heatmaps`` on the CPU) and ships fp32 images plus fp32 targets to the GPU; here only the decoded uint8 images cross
PCIe and ``LabeledBatchProducer`` builds the whole ``HeatmapLabeledBatchDict`` on the device (resize + normalise, keypoint projection,
optional flip with the left / right swap, out-of-frame -> NaN, Gaussian targets).  ``imgaug_transform`` is the device pipeline that
``data.augmentations.imgaug_transform`` / ``get_imgaug_transform`` build from ``cfg.training.imgaug`` (the reference's ``iaa.Sequential``
in the same argument): it is drawn once per batch on the host and applied to the uint8 images on the device before the resize; the
validation / test / prediction loaders ask for ``augment=False``.  Context (5-frame) loading is outside this path.

``MultiviewHeatmapDataset`` (reference :553-1228) holds one ``HeatmapDataset`` per view, the per-view bounding-box files and the anipose
calibration of every frame, and hands ``MultiviewLabeledBatchProducer`` whole batches: with a calibration, a training batch goes through the
reference's 3-D augmentation (``apply_3d_transforms``) on the device.
"""

from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Iterator, Sequence

import numpy as np
import pandas as pd
import torch

from pathlib import Path

from .. import ops
from .augmentations import LabeledAugmentation
from .cameras import CameraGroup
from .datatypes import HeatmapLabeledBatchDict, MultiviewHeatmapLabeledBatchDict
from .producers import HostStager, LabeledBatchProducer, MultiviewLabeledBatchProducer


@dataclass
class LabeledData:
    """Result of parsing a label file (reference utils/io.py:190-205)."""

    keypoint_names: list[str]
    image_names: list[str]
    keypoints: torch.Tensor            # (N, K, 2) float32, NaN where unlabeled
    visibility: torch.Tensor | None    # (N, K) int64 in {0, 1, 2}, or None without a ``visible`` column


def parse_label_csv(csv_file: str, header_rows: list[int] | None = None) -> LabeledData:
    """Read a DLC-style label CSV once (reference utils/io.py:208-279)."""
    if header_rows is None:
        header_rows = [0, 1, 2]
    if not os.path.exists(csv_file):
        raise FileNotFoundError(f"could not find csv file at {csv_file}")
    df = pd.read_csv(csv_file, header=header_rows, index_col=0)
    if df.index.name is not None:  # pandas took an all-NaN first data row for the index name (reference :529-554)
        first = pd.DataFrame({c: np.nan for c in df.columns}, index=pd.Index([df.index.name]), columns=df.columns, dtype="float64")
        df = pd.concat([first, df])
    if header_rows in ([1, 2], [0, 1]):
        keypoint_names = [c[0] for c in df.columns if c[1] == "x"]
    else:
        keypoint_names = [c[1] for c in df.columns if c[2] == "x"]
    raw = torch.tensor(df.to_numpy(), dtype=torch.float32)
    if header_rows == [0, 1, 2] and any(c[2] == "visible" for c in df.columns):
        raw = raw.reshape(raw.shape[0], -1, 3)
        vis = raw[:, :, 2]
        invalid = set(vis[~torch.isnan(vis)].unique().tolist()) - {0.0, 1.0, 2.0}
        if invalid:
            raise ValueError(f"visibility column contains invalid values {invalid}; expected values in {{0, 1, 2}}")
        return LabeledData(keypoint_names, list(df.index), raw[:, :, :2].contiguous(), vis.long())
    return LabeledData(keypoint_names, list(df.index), raw.reshape(raw.shape[0], -1, 2), None)


def build_hflip_swap_indices(keypoint_names: Sequence[str]) -> np.ndarray:
    """Entry i = the keypoint that fills position i after a horizontal flip: ``*_left`` <-> ``*_right`` partners swap, everything else
    stays (reference data/datasets.py:203-245).  Unmatched partners raise ValueError."""
    idx = list(range(len(keypoint_names)))
    left = {n[:-5]: i for i, n in enumerate(keypoint_names) if n.endswith("_left")}
    right = {n[:-6]: i for i, n in enumerate(keypoint_names) if n.endswith("_right")}
    lonely_l = sorted(f"{b}_left" for b in set(left) - set(right))
    lonely_r = sorted(f"{b}_right" for b in set(right) - set(left))
    if lonely_l:
        raise ValueError(f"imgaug_hflip requires matching _left/_right pairs, but found _left keypoints with no _right partner: {lonely_l}")
    if lonely_r:
        raise ValueError(f"imgaug_hflip requires matching _left/_right pairs, but found _right keypoints with no _left partner: {lonely_r}")
    for base, i in left.items():
        idx[i], idx[right[base]] = right[base], i
    return np.array(idx, dtype=np.intp)


class HeatmapDataset:
    """Labels in memory, images on disk, batches built on the device."""

    def __init__(self, root_directory: str, csv_path: str, image_resize_height: int, image_resize_width: int,
                 header_rows: list[int] | None = [0, 1, 2], downsample_factor: int = 2, do_context: bool = False,
                 uniform_heatmaps: bool = False, imgaug_hflip: bool = False, device: torch.device | str | None = None,
                 imgaug_transform=None) -> None:
        if do_context:
            raise NotImplementedError("context (5-frame) datasets belong to the MHCRNN models, outside the MI355X heatmap-tracker path")
        self.root_directory = str(root_directory)
        csv_file = csv_path if os.path.isfile(csv_path) else os.path.join(self.root_directory, csv_path)
        data = parse_label_csv(csv_file, header_rows=header_rows)
        self.keypoint_names, self.image_names, self.keypoints = data.keypoint_names, data.image_names, data.keypoints
        self.num_keypoints = int(self.keypoints.shape[1])
        self.num_targets = 2 * self.num_keypoints
        self.do_context = False
        self.downsample_factor = int(downsample_factor)
        self.output_sigma = 1.25
        self.uniform_heatmaps = bool(uniform_heatmaps)
        if data.visibility is None:  # synthesised from the NaN labels (reference :465-472)
            nan = torch.isnan(self.keypoints[:, :, 0])
            self.visibility = torch.where(nan, torch.full_like(nan, 1 if uniform_heatmaps else 0, dtype=torch.long),
                                          torch.full_like(nan, 2, dtype=torch.long))
        else:
            self.visibility = data.visibility
        self.imgaug_hflip = bool(imgaug_hflip)
        swap = build_hflip_swap_indices(self.keypoint_names) if imgaug_hflip else None
        self.producer = LabeledBatchProducer(image_resize_height, image_resize_width, downsample_factor=downsample_factor,
                                             uniform_heatmaps=uniform_heatmaps, hflip_swap_indices=None if swap is None else swap.tolist())
        self.device = torch.device(device) if device is not None else torch.device(f"cuda:{int(os.environ.get('LOCAL_RANK', '0'))}")
        self._stage = HostStager(self.device)
        self._rng = np.random.default_rng(0)
        if imgaug_transform is not None and not (hasattr(imgaug_transform, "draw") and hasattr(imgaug_transform, "run")):
            raise TypeError(f"imgaug_transform must be a data.augmentations.LabeledAugmentation, got {type(imgaug_transform)}")
        self.imgaug_transform = imgaug_transform

    @property
    def height(self) -> int:
        return self.producer.height

    @property
    def width(self) -> int:
        return self.producer.width

    @property
    def output_shape(self) -> tuple[int, int]:
        return self.producer.output_shape

    def __len__(self) -> int:
        return len(self.image_names)

    def load_images(self, indices: Sequence[int]) -> torch.Tensor:
        """(B, H, W, 3) uint8 on the host: each file decoded as RGB (single-channel images are replicated, reference :277)."""
        from PIL import Image

        frames = []
        for i in indices:
            with Image.open(os.path.join(self.root_directory, self.image_names[int(i)])) as im:
                frames.append(np.asarray(im.convert("RGB")))
        if len({f.shape for f in frames}) != 1:
            raise ValueError(f"images of one batch must share a size, got {sorted({f.shape for f in frames})}")
        return torch.from_numpy(np.stack(frames))

    def image_sizes(self, indices: Sequence[int]) -> torch.Tensor:
        """(B, 2) float32 stored (height, width) of these examples' images, read from the file headers: no image is decoded."""
        from PIL import Image

        sizes = []
        for i in indices:
            with Image.open(os.path.join(self.root_directory, self.image_names[int(i)])) as im:
                w, h = im.size
            sizes.append([float(h), float(w)])
        return torch.tensor(sizes, dtype=torch.float32).reshape(-1, 2)

    def unaugmented_keypoints(self, indices: Sequence[int]) -> torch.Tensor:
        """(B, 2K) model-px keypoints of these examples, NaN where unlabeled or out of frame: the ``keypoints`` of ``batch(indices,
        hflip=None-or-zeros, augment=False)`` bit for bit (the same ``lp_labeled_keypoints`` launch), without loading an image."""
        idx = torch.as_tensor(list(indices), dtype=torch.long)
        if len(idx) == 0:
            return torch.empty(0, self.num_targets, device=self.device)
        kp_model, _ = ops.labeled_keypoints(self.keypoints[idx].to(self.device), self.image_sizes(idx.tolist()).to(self.device),
                                            self.height, self.width, swap=self.producer.swap, visibility=self.visibility[idx].to(self.device),
                                            uniform_heatmaps=self.uniform_heatmaps)
        return kp_model.reshape(len(idx), self.num_targets)

    def batch(self, indices: Sequence[int], hflip: torch.Tensor | None = None, augment: bool = True) -> HeatmapLabeledBatchDict:
        """The labeled batch of the step for these examples; ``hflip`` (B,) overrides the random flip decisions of ``imgaug_hflip``;
        ``augment=False`` leaves ``imgaug_transform`` out (validation, test, prediction)."""
        idx = torch.as_tensor(list(indices), dtype=torch.long)
        images = self._stage(self.load_images(idx.tolist()))   # pinned staging + copy stream: overlaps the step that is running
        if hflip is None and self.imgaug_hflip:
            hflip = torch.from_numpy(self._rng.random(len(idx)) < 0.5)  # each sample flips with probability 0.5 (reference :275)
        drawn = None
        if augment and self.imgaug_transform is not None and len(self.imgaug_transform) > 0:  # (0 operators: resize only)
            drawn = self.imgaug_transform.draw(len(idx), int(images.shape[1]), int(images.shape[2]))
        return self.producer(images, self.keypoints[idx].to(self.device), idxs=idx, visibility=self.visibility[idx].to(self.device),
                             hflip=hflip, augment=drawn)

    def batches(self, batch_size: int, shuffle: bool = True, seed: int = 0, drop_last: bool = False) -> Iterator[HeatmapLabeledBatchDict]:
        order = np.random.default_rng(seed).permutation(len(self)) if shuffle else np.arange(len(self))
        for lo in range(0, len(order), batch_size):
            chunk = order[lo:lo + batch_size]
            if drop_last and len(chunk) < batch_size:
                return
            yield self.batch(chunk.tolist())


class MultiviewHeatmapDataset:
    """One ``HeatmapDataset`` per camera view at ``self.dataset[view]``; batches of all views built on the device.

    Constructor arguments in the reference's order and meaning (data/datasets.py:571-617); ``resize`` is accepted and has nothing to do (the
    resize is always the last step of the device path); ``imgaug_hflip`` is always False (not supported for multi-view).  ``imgaug_transform``
    is the ``LabeledAugmentation`` of ``cfg.training.imgaug``: with a calibration it must hold pixel operators only (the "dlc-mv" preset) -
    the geometry is the 3-D augmentation's.  The reference augments in 3-D when the imgaug pipeline has no Resize (training) and only
    triangulates otherwise; here ``batch(..., augment=True / False)`` says which, as for ``HeatmapDataset``."""

    def __init__(self, root_directory: str, csv_paths: list[str], view_names: list[str], image_resize_height: int, image_resize_width: int,
                 header_rows: list[int] | None = [0, 1, 2], imgaug_transform=None, downsample_factor: int = 2, do_context: bool = False,
                 resize: bool = False, uniform_heatmaps: bool = False, camera_params_path: str | None = None,
                 bbox_paths: list[str] | None = None, device: torch.device | str | None = None) -> None:
        if len(view_names) != len(csv_paths):
            raise ValueError("number of names does not match with the number of files!")
        if do_context:
            raise NotImplementedError("context (5-frame) datasets belong to the MHCRNN models, outside the MI355X heatmap-tracker path")
        self.imgaug_hflip = False
        self.root_directory = str(root_directory)
        self.csv_paths = list(csv_paths)
        self.bbox_paths = list(bbox_paths) if bbox_paths else [None] * len(view_names)
        if len(self.bbox_paths) != len(view_names):
            raise ValueError("zip() argument: bbox_paths must have one entry per view")   # (the reference's zip(..., strict=True))
        self.view_names = list(view_names)
        self.image_resize_height, self.image_resize_width = int(image_resize_height), int(image_resize_width)
        self.do_context = False
        self.resize = bool(resize)
        # (never None: BaseDataModule asks for augment=False on validation / test batches of a dataset that HAS a transform, and the 3-D
        # augmentation is one; an empty pipeline is 'resize only')
        self.imgaug_transform = imgaug_transform if imgaug_transform is not None else LabeledAugmentation([])
        self.downsample_factor = int(downsample_factor)
        self.uniform_heatmaps = bool(uniform_heatmaps)
        self.device = torch.device(device) if device is not None else torch.device(f"cuda:{int(os.environ.get('LOCAL_RANK', '0'))}")
        self.dataset: dict[str, HeatmapDataset] = {}
        self.keypoint_names: dict[str, list[str]] = {}
        self.bboxes: dict[str, np.ndarray | None] = {}
        data_length_by_view, num_keypoints_by_view = {}, {}
        for view, csv_path, bbox_path in zip(self.view_names, self.csv_paths, self.bbox_paths):
            ds = HeatmapDataset(root_directory=root_directory, csv_path=csv_path, image_resize_height=image_resize_height,
                                image_resize_width=image_resize_width, header_rows=header_rows, imgaug_transform=imgaug_transform,
                                downsample_factor=downsample_factor, do_context=False, uniform_heatmaps=uniform_heatmaps, device=self.device)
            self.dataset[view] = ds
            self.keypoint_names[view] = ds.keypoint_names
            data_length_by_view[view] = len(ds)
            num_keypoints_by_view[view] = ds.num_keypoints
            self.bboxes[view] = self._load_bboxes(bbox_path, ds.image_names)
        self.num_keypoints = sum(num_keypoints_by_view.values())
        self.check_data_images_names(data_length_by_view)
        self.num_targets = self.num_keypoints * 2
        if camera_params_path is not None:
            self.cam_params_df, self.cam_params_file_to_camgroup = self._load_cam_params_from_csv(camera_params_path)
        else:
            self.cam_params_df, self.cam_params_file_to_camgroup = self._discover_cam_params_from_image_paths()
        self.producer = MultiviewLabeledBatchProducer(image_resize_height, image_resize_width, downsample_factor=downsample_factor,
                                                      uniform_heatmaps=uniform_heatmaps)
        self._rigs: dict[str, tuple] = {}   # calibration file -> host (intrinsics, extrinsics, distortions) of one sample

    # ---- files ------------------------------------------------------------------------------------------------------------------
    def _load_bboxes(self, bbox_path: str | None, image_names: list[str]) -> np.ndarray | None:
        """(image_path, x, y, h, w) rows in the order of the label file (reference :189-201)"""
        if not bbox_path:
            return None
        bbox_file = bbox_path if os.path.isfile(bbox_path) else os.path.join(self.root_directory, bbox_path)
        if not os.path.exists(bbox_file):
            raise FileNotFoundError(f"Could not find bbox file at {bbox_file}!")
        df = pd.read_csv(bbox_file, header=[0], index_col=0)
        assert df.index.tolist() == image_names
        return df.to_numpy().astype(np.float32)

    def _load_camgroup(self, calib_file: str) -> CameraGroup:
        camgroup = CameraGroup.load(os.path.join(self.root_directory, calib_file), device=self.device)
        cam_names = camgroup.get_names()
        assert list(cam_names) == list(self.view_names), (
            "cfg.data.view_names must have same camera order as camera calibration file; "
            f"instead found {self.view_names} and {cam_names}.")
        return camgroup

    def _load_cam_params_from_csv(self, camera_params_path: str):
        """a CSV that maps every frame to a calibration TOML (reference :702-724)"""
        path = camera_params_path if os.path.isfile(camera_params_path) else os.path.join(self.root_directory, camera_params_path)
        cam_params_df = pd.read_csv(path, index_col=0, header=[0])
        img_idxs_labels = [i.split("/")[-1] for i in self.dataset[self.view_names[0]].image_names]
        img_idxs_calib = [i.split("/")[-1] for i in cam_params_df.index]
        assert img_idxs_labels == img_idxs_calib
        return cam_params_df, {f: self._load_camgroup(f) for f in cam_params_df.file.unique()}

    def _discover_cam_params_from_image_paths(self):
        """labeled-data/<session>_<view>/img<frameidx>.ext -> calibrations/<session>.toml, then calibration.toml (reference :726-786);
        (None, None) if no calibration is found, or not for every frame"""
        image_names = self.dataset[self.view_names[0]].image_names
        groups: dict[str, CameraGroup] = {}
        calib_files, all_found = [], True
        for img_name in image_names:
            parts = Path(img_name).parts
            if "labeled-data" not in parts:
                raise ValueError(f"Image path '{img_name}' does not match expected pattern labeled-data/<session>_<view>/img<frameidx>.ext")
            folder_name = parts[parts.index("labeled-data") + 1]
            if "_" not in folder_name:
                raise ValueError(f"Folder '{folder_name}' in image path '{img_name}' does not match expected pattern <session>_<view>")
            session_id = folder_name.rsplit("_", 1)[0]
            if (Path(self.root_directory) / "calibrations" / f"{session_id}.toml").exists():
                calib_file = str(Path("calibrations") / f"{session_id}.toml")
            elif (Path(self.root_directory) / "calibration.toml").exists():
                calib_file = "calibration.toml"
            else:
                all_found = False
                calib_files.append(None)
                continue
            calib_files.append(calib_file)
            if calib_file not in groups:
                groups[calib_file] = self._load_camgroup(calib_file)
        if groups and all_found:
            return pd.DataFrame({"file": calib_files}, index=image_names), groups
        return None, None   # (some frames without a calibration: 3-D is off for the whole dataset, as in the reference)

    def check_data_images_names(self, data_length_by_view: dict[str, int]) -> None:
        """the label files must agree in rows, keypoint order and image file names (reference :788-820)"""
        if len(set(data_length_by_view.values())) != 1:
            raise ImportError("the CSV files do not match in row numbers!")
        first = self.keypoint_names[self.view_names[0]]
        for key_num, keypoint in enumerate(first):
            for view, names in self.keypoint_names.items():
                if key_num >= len(names) or keypoint != names[key_num]:
                    raise ImportError(f"the keypoints are not in correct order! view: {self.view_names[0]} vs {view} | {keypoint} != {names}")
        self.data_length = list(data_length_by_view.values())[0]
        for idx in range(self.data_length):
            names = {Path(ds.image_names[idx]).name for ds in self.dataset.values()}
            if len(names) > 1:
                raise ImportError(f"Discrepancy in image file names across CSV files! index:{idx}, image file names:{names}")

    # ---- attributes -------------------------------------------------------------------------------------------------------------
    @property
    def height(self) -> int:
        return self.image_resize_height

    @property
    def width(self) -> int:
        return self.image_resize_width

    @property
    def output_shape(self) -> tuple[int, int]:
        return self.height // 2 ** self.downsample_factor, self.width // 2 ** self.downsample_factor

    @property
    def num_views(self) -> int:
        return len(self.view_names)

    def __len__(self) -> int:
        return self.data_length

    # ---- batches ----------------------------------------------------------------------------------------------------------------
    def _rig(self, calib_file: str):
        if calib_file not in self._rigs:
            self._rigs[calib_file] = tuple(t[0] for t in self.cam_params_file_to_camgroup[calib_file].rig(1, device="cpu"))
        return self._rigs[calib_file]

    def unaugmented_keypoints(self, indices: Sequence[int]) -> torch.Tensor:
        """(B, 2 V K) model-px keypoints, the views side by side in ``view_names`` order: the ``keypoints`` of ``batch(indices,
        augment=False)`` (every view takes ``HeatmapDataset``'s path there), without loading an image."""
        return torch.cat([self.dataset[v].unaugmented_keypoints(indices) for v in self.view_names], dim=1)

    def batch(self, indices: Sequence[int], hflip: torch.Tensor | None = None, augment: bool = True,
              params: np.ndarray | None = None) -> MultiviewHeatmapLabeledBatchDict:
        """The labeled batch of these examples.  ``augment=True``: the pixel operators of ``imgaug_transform`` per view and, with a
        calibration, the 3-D augmentation (``params`` (B, 4) overrides its draw); ``augment=False``: resize only (validation, test,
        prediction), ``keypoints_3d`` the plain triangulation.  ``hflip`` must be None: multi-view flips are not supported."""
        if hflip is not None and bool(torch.as_tensor(hflip).any()):
            raise ValueError("imgaug_hflip is not supported for multi-view datasets")
        idx = torch.as_tensor(list(indices), dtype=torch.long)
        views = [self.dataset[v] for v in self.view_names]
        images = [ds._stage(ds.load_images(idx.tolist())) for ds in views]
        kp = torch.stack([ds.keypoints[idx] for ds in views], dim=1)            # (B, V, K, 2)
        vis = torch.stack([ds.visibility[idx] for ds in views], dim=1)          # (B, V, K)
        rows = []
        for ds, view, im in zip(views, self.view_names, images):
            bb = self.bboxes[view]
            rows.append(torch.tensor([0.0, 0.0, float(im.shape[1]), float(im.shape[2])]).repeat(len(idx), 1) if bb is None
                        else torch.from_numpy(bb[idx.numpy()]))
        bbox = torch.cat(rows, dim=1)                                           # (B, 4 V)
        rig = {}
        if self.cam_params_file_to_camgroup:
            per = [self._rig(self.cam_params_df.iloc[int(i)].file) for i in idx]
            n = max(p[2].shape[-1] for p in per)
            rig = dict(intrinsics=torch.stack([p[0] for p in per]), extrinsics=torch.stack([p[1] for p in per]),
                       distortions=torch.stack([torch.nn.functional.pad(p[2], (0, n - p[2].shape[-1])) for p in per]))
        drawn = None
        tf = self.imgaug_transform
        if augment and tf is not None and len(tf) > 0:
            drawn = [tf.draw(len(idx), int(im.shape[1]), int(im.shape[2])) for im in images]
        return self.producer(images, kp, self.view_names, idxs=idx, visibility=vis, bbox=bbox, augment=augment, params=params,
                             pixel_augment=drawn, **rig)

    def batches(self, batch_size: int, shuffle: bool = True, seed: int = 0, drop_last: bool = False) -> Iterator[MultiviewHeatmapLabeledBatchDict]:
        order = np.random.default_rng(seed).permutation(len(self)) if shuffle else np.arange(len(self))
        for lo in range(0, len(order), batch_size):
            chunk = order[lo:lo + batch_size]
            if drop_last and len(chunk) < batch_size:
                return
            yield self.batch(chunk.tolist())
