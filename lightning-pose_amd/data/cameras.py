"""Camera geometry for multi-view 2D-to-3D projection and triangulation (reference: lightning_pose/data/cameras.py:22-171).

``project_camera_pairs_to_3d`` and ``project_3d_to_2d`` keep the reference's names, arguments, shapes and NaN rules and are differentiable in
the points only.  Underneath, each is ONE kernel launch (``csrc/cameras.hip``): every (sample, pair, keypoint) - a 4 x 4 homogeneous DLT - is
solved in one lane's registers, where the reference loops in Python over pairs and samples with a host read and a small batched SVD per
iteration.  The tracker uses the fused form ``ops.camera_chain`` (triangulate every pair, average, reproject into every view, map to model px).

The arithmetic restates what the reference calls from kornia (``undistort_points``, ``triangulate_points``, ``PinholeCamera.project``,
``distort_points``); it is written out in ``include/lp_hip.h``.  kornia is not a dependency of this package: the 5 fixed-point iterations of
the undistortion and the 1e-8 guard of the homogeneous divisions are kornia's defaults AS RECOLLECTED - they could not be read when this was
written.  The restatement reproduces the reference's own anipose-fly fixture within the reference's bars (``tests/test_cameras_reference_cases.py``).

``CameraGroup`` is the subset of aniposelib's class that ``MultiviewHeatmapDataset`` uses: ``load`` reads an anipose calibration TOML
(``name``, ``size``, ``matrix``, ``distortions``, ``rotation`` as a Rodrigues vector, ``translation`` per ``[cam_*]`` table),
``triangulate_fast`` and ``project`` keep the reference's shapes (data/cameras.py:174-215) and go through the same kernels as everything else
here - the median over the camera pairs is ``lp_mv3d_plan``'s.

Not here: the rest of aniposelib's ``CameraGroup`` (calibration, bundle adjustment, the fisheye model, ``dump``) - ``aniposelib`` and ``cv2`` are
not dependencies.
"""

from __future__ import annotations

import os

import numpy as np
import torch

from .. import ops

__all__: list[str] = []


def rodrigues_to_matrix(rvec) -> np.ndarray:
    """Rotation vector (axis * angle, what anipose stores and ``cv2.Rodrigues`` reads) -> (3, 3) rotation matrix, float64:
    R = I + sin(t) K + (1 - cos(t)) K^2 with K the cross-product matrix of the unit axis; the identity below 1e-12 rad."""
    r = np.asarray(rvec, dtype=np.float64).reshape(3)
    theta = float(np.linalg.norm(r))
    if theta < 1e-12:
        return np.eye(3)
    x, y, z = r / theta
    k = np.array([[0.0, -z, y], [z, 0.0, -x], [-y, x, 0.0]])
    return np.eye(3) + np.sin(theta) * k + (1.0 - np.cos(theta)) * (k @ k)


class Camera:
    """One calibrated camera of an anipose file: the getters ``MultiviewHeatmapDataset`` calls."""

    def __init__(self, name: str, size, matrix, distortions, rotation, translation) -> None:
        self.name = str(name)
        self.size = None if size is None else tuple(int(v) for v in size)
        self.matrix = np.asarray(matrix, dtype=np.float64).reshape(3, 3)
        self.dist = np.asarray(distortions, dtype=np.float64).reshape(-1)
        if self.dist.size not in (4, 5, 8, 12):
            raise ValueError(f"camera {self.name}: {self.dist.size} distortion parameters (OpenCV sets of 4, 5, 8 or 12 are understood)")
        self.rvec = np.asarray(rotation, dtype=np.float64).reshape(3)
        self.tvec = np.asarray(translation, dtype=np.float64).reshape(3)

    def get_name(self) -> str:
        return self.name

    def get_camera_matrix(self) -> np.ndarray:
        return self.matrix

    def get_distortions(self) -> np.ndarray:
        return self.dist

    def get_extrinsics_mat(self) -> np.ndarray:
        """(4, 4) world -> camera"""
        out = np.eye(4)
        out[:3, :3] = rodrigues_to_matrix(self.rvec)
        out[:3, 3] = self.tvec
        return out


class CameraGroup:
    """The cameras of one calibration file, in file order."""

    def __init__(self, cameras: list, metadata: dict | None = None, device: torch.device | str | None = None) -> None:
        self.cameras = list(cameras)
        self.metadata = dict(metadata or {})
        self.device = torch.device(device) if device is not None else torch.device(f"cuda:{int(os.environ.get('LOCAL_RANK', '0'))}")

    @classmethod
    def load(cls, path, device: torch.device | str | None = None) -> "CameraGroup":
        try:
            import tomllib as toml_reader
        except ModuleNotFoundError:
            import tomli as toml_reader
        with open(path, "rb") as f:
            doc = toml_reader.load(f)
        keys = sorted((k for k in doc if k != "metadata"), key=lambda k: (len(k), k))   # cam_0 ... cam_10, as aniposelib orders them
        cams = [Camera(doc[k]["name"], doc[k].get("size"), doc[k]["matrix"], doc[k]["distortions"], doc[k]["rotation"], doc[k]["translation"])
                for k in keys]
        return cls(cams, doc.get("metadata"), device=device)

    def get_names(self) -> list[str]:
        return [c.get_name() for c in self.cameras]

    def rig(self, batch: int = 1, device: torch.device | str | None = None) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """intrinsics (batch, V, 3, 3), extrinsics (batch, V, 3, 4), distortions (batch, V, n) in fp32 on ``device`` (host tensors if "cpu")"""
        n = max(c.dist.size for c in self.cameras)
        intr = np.stack([c.get_camera_matrix() for c in self.cameras])
        extr = np.stack([c.get_extrinsics_mat()[:3] for c in self.cameras])
        dist = np.stack([np.pad(c.dist, (0, n - c.dist.size)) for c in self.cameras])
        dev = self.device if device is None else torch.device(device)
        return tuple(torch.from_numpy(a.astype(np.float32))[None].repeat(batch, *([1] * a.ndim)).to(dev) for a in (intr, extr, dist))

    def triangulate_fast(self, points: np.ndarray, undistort: bool = True) -> np.ndarray:
        """(V, N, 2) frame px -> (N, 3): every camera pair triangulated, numpy's nanmedian over the pairs"""
        if not undistort:
            raise NotImplementedError("triangulate_fast(undistort=False) is not built: the kernels undistort")
        pts = np.asarray(points, dtype=np.float32)
        assert pts.shape[0] == len(self.cameras), \
            f"Invalid points shape, first dim should be equal to number of cameras ({len(self.cameras)}), but shape is {pts.shape}"
        one_point = pts.ndim == 2
        if one_point:
            pts = pts.reshape(-1, 1, 2)
        v, n, _ = pts.shape
        kmax = ops.MV3D_MAX_KEYPOINTS
        b = max(1, -(-n // kmax))
        padded = np.full((v, b * kmax, 2), np.nan, dtype=np.float32)
        padded[:, :n] = pts
        kp = torch.from_numpy(np.ascontiguousarray(padded.reshape(v, b, kmax, 2).transpose(1, 0, 2, 3))).to(self.device)
        intr, extr, dist = self.rig(b)
        unit = torch.tensor([0.0, 0.0, 1.0, 1.0], device=self.device).repeat(b, v)   # src_hw = (1, 1), bbox = [0, 0, 1, 1]: px pass through
        kp3d = ops.mv3d_plan(kp, torch.ones(b, v, 2, device=self.device), unit, intr, extr, dist, torch.zeros(b, 4, device=self.device), 1, 1,
                             augment=False)[0]
        out = kp3d.reshape(b * kmax, 3)[:n].cpu().numpy().astype(np.float64)
        return out[0] if one_point else out

    def project(self, points: np.ndarray) -> np.ndarray:
        """(N, 3) -> (V, N, 2) frame px, distortion applied"""
        p3 = torch.from_numpy(np.asarray(points, dtype=np.float32).reshape(1, -1, 3)).to(self.device)
        intr, extr, dist = self.rig(1)
        return ops.camera_project(p3, intr, extr, dist)[0].cpu().numpy().astype(np.float64)


def project_camera_pairs_to_3d(points: torch.Tensor, intrinsics: torch.Tensor, extrinsics: torch.Tensor, dist: torch.Tensor) -> torch.Tensor:
    """Project 2D keypoints from each pair of cameras into 3D world space.

    points (batch, num_views, num_keypoints, 2), intrinsics (batch, num_views, 3, 3), extrinsics (batch, num_views, 3, 4), dist (batch,
    num_views, 4 | 5 | 8 | 12 OpenCV parameters) -> (batch, cam_pair, num_keypoints, 3), pairs in ``itertools.combinations`` order; a keypoint
    that is NaN in either view of a pair is NaN for that pair.
    """
    return ops.camera_pairs_to_3d(points, intrinsics, extrinsics, dist)


def project_3d_to_2d(points_3d: torch.Tensor, intrinsics: torch.Tensor, extrinsics: torch.Tensor, dist: torch.Tensor) -> torch.Tensor:
    """Project 3D keypoints (batch, num_keypoints, 3) to 2D in every camera view -> (batch, num_views, num_keypoints, 2); a NaN 3-D point
    gives a NaN 2-D point."""
    return ops.camera_project(points_3d, intrinsics, extrinsics, dist)
