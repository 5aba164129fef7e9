"""Camera geometry for multi-view 2D-to-3D projection and triangulation (reference: lightning_pose/data/cameras.py:22-171).

``project_camera_pairs_to_3d`` and ``project_3d_to_2d`` keep the reference's names, arguments, shapes and NaN rules and are differentiable in
the points only.  Underneath, each is ONE kernel launch (``csrc/cameras.hip``): every (sample, pair, keypoint) - a 4 x 4 homogeneous DLT - is
solved in one lane's registers, where the reference loops in Python over pairs and samples with a host read and a small batched SVD per
iteration.  The tracker uses the fused form ``ops.camera_chain`` (triangulate every pair, average, reproject into every view, map to model px).

The arithmetic restates what the reference calls from kornia (``undistort_points``, ``triangulate_points``, ``PinholeCamera.project``,
``distort_points``); it is written out in ``include/lp_hip.h``.  kornia is not a dependency of this package: the 5 fixed-point iterations of
the undistortion and the 1e-8 guard of the homogeneous divisions are kornia's defaults AS RECOLLECTED - they could not be read when this was
written.  The restatement reproduces the reference's own anipose-fly fixture within the reference's bars (``tests/test_cameras_reference_cases.py``).

Not here: ``CameraGroup`` (the anipose / OpenCV calibration loader) and the dataset code that reads ``camera_params_file`` - ``aniposelib`` and
``cv2`` are not dependencies.  The feature starts at the batch dict: ``keypoints_3d``, ``intrinsic_matrix``, ``extrinsic_matrix``,
``distortions`` (``data.datatypes.MultiviewHeatmapLabeledBatchDict``).
"""

from __future__ import annotations

import torch

from .. import ops

__all__: list[str] = []


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
