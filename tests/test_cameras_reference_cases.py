"""The reference's eight camera tests (tests/data/test_cameras.py) restated on its anipose-fly fixture (tests/golden/cameras_fly.npz), with
their own bars, through this package's data.cameras / data.bboxes surface."""

import pytest
import torch

from tests import cameras_fp64 as O


@pytest.fixture
def fly(stack_backend):
    f = {k: v.float().to(stack_backend) for k, v in O.fly_fixture().items()}
    f["points_3d_pairs"] = f["points_3d"][:, None].expand(1, 3, 2, 3)   # the same 3-D points from each of the three camera pairs
    return f


def _cam(f):
    return dict(intrinsics=f["intrinsics"], extrinsics=f["extrinsics"], dist=f["distortions"])


def test_pairs_to_3d_basic(fly):
    from lightning_pose_amd.data.cameras import project_camera_pairs_to_3d

    p3d = project_camera_pairs_to_3d(points=fly["points_2d"], **_cam(fly))
    assert p3d.shape == (1, 3, 2, 3)  # batch, pairs, keypoints, coords
    assert torch.allclose(p3d, fly["points_3d_pairs"], rtol=1e-2)


def test_pairs_to_3d_nan_handling(fly):
    from lightning_pose_amd.data.cameras import project_camera_pairs_to_3d

    pts = fly["points_2d"].clone()
    pts[0, 0, 0, :] = float("nan")
    p3d = project_camera_pairs_to_3d(points=pts, **_cam(fly))
    want = fly["points_3d_pairs"]
    assert p3d.shape == (1, 3, 2, 3)
    assert torch.all(torch.isnan(p3d[0, 0, 0, :]))
    assert torch.allclose(p3d[0, 0, 1, :], want[0, 0, 1, :], rtol=1e-2)
    assert torch.all(torch.isnan(p3d[0, 1, 0, :]))
    assert torch.allclose(p3d[0, 1, 1, :], want[0, 1, 1, :], rtol=1e-2)
    assert torch.allclose(p3d[0, 2], want[0, 2], rtol=1e-3)


def test_3d_to_2d_basic(fly):
    from lightning_pose_amd.data.cameras import project_3d_to_2d

    p2d = project_3d_to_2d(points_3d=fly["points_3d"], **_cam(fly))
    assert p2d.shape == (1, 3, 2, 2)  # batch, views, keypoints, coords
    assert torch.allclose(p2d, fly["points_2d"], rtol=1e-4)


def test_3d_to_2d_nan_handling(fly):
    from lightning_pose_amd.data.cameras import project_3d_to_2d

    x = fly["points_3d"].clone()
    x[0, 0, 0] = float("nan")  # make first keypoint invalid
    p2d = project_3d_to_2d(points_3d=x, **_cam(fly))
    assert p2d.shape == (1, 3, 2, 2)
    assert torch.all(torch.isnan(p2d[0, :, 0, :]))
    assert torch.allclose(p2d[0, :, 1, :], fly["points_2d"][0, :, 1, :], rtol=1e-4)


def test_3d_to_2d_all_nan_input(fly):
    from lightning_pose_amd.data.cameras import project_3d_to_2d

    p2d = project_3d_to_2d(points_3d=torch.full_like(fly["points_3d"], float("nan")), **_cam(fly))
    assert p2d.shape == (1, 3, 2, 2)
    assert torch.all(torch.isnan(p2d))


def test_3d_to_2d_batch_dim(fly):
    from lightning_pose_amd.data.cameras import project_3d_to_2d

    p2d = project_3d_to_2d(points_3d=fly["points_3d"].repeat(2, 1, 1), intrinsics=fly["intrinsics"].repeat(2, 1, 1, 1),
                           extrinsics=fly["extrinsics"].repeat(2, 1, 1, 1), dist=fly["distortions"].repeat(2, 1, 1))
    assert p2d.shape == (2, 3, 2, 2)
    assert torch.allclose(p2d[0], p2d[1], rtol=1e-6)


def test_camera_round_trip_accuracy(fly):
    """2D -> 3D (every pair) -> mean -> 2D: under one pixel"""
    from lightning_pose_amd.data.cameras import project_3d_to_2d, project_camera_pairs_to_3d

    p3d = project_camera_pairs_to_3d(points=fly["points_2d"], **_cam(fly))
    recovered = project_3d_to_2d(points_3d=torch.mean(p3d, dim=1), **_cam(fly))
    error = torch.norm(fly["points_2d"] - recovered, dim=-1)
    print(f"round-trip error, px: {error.flatten().tolist()}")
    assert error.max() < 1.0, f"Round-trip error too large: {error.max()}"


def test_full_coordinate_pipeline_roundtrip(fly, stack_backend):
    """frame -> model -> frame px (0.1 px), then 3-D, mean, reprojection and back to model px: under 5 px over all coordinates; the fused
    chain (ops.camera_chain) gives what the step-by-step functions give"""
    from lightning_pose_amd import ops
    from lightning_pose_amd.data.bboxes import frame_to_model_batch, model_to_frame_batch
    from lightning_pose_amd.data.cameras import project_3d_to_2d, project_camera_pairs_to_3d

    dev = stack_backend
    bbox = torch.tensor([[100, 50, 600, 600, 200, 100, 500, 500, 50, 75, 700, 700]]).float().to(dev)
    batch = {"images": torch.zeros(1, 3, 3, 256, 256, device=dev), "bbox": bbox, "intrinsic_matrix": fly["intrinsics"],
             "extrinsic_matrix": fly["extrinsics"], "distortions": fly["distortions"], "is_multiview": True}
    world = fly["points_2d"]
    model_2d = frame_to_model_batch(batch_dict=batch, frame_keypoints=world)
    assert model_2d.shape == (1, 3, 2, 2)
    flat = model_2d.reshape(1, 12)
    recovered = model_to_frame_batch(batch, flat, in_place=False).reshape(1, 3, 2, 2)
    assert torch.norm(world - recovered, dim=-1).max() < 0.1
    p3d = project_camera_pairs_to_3d(points=recovered, intrinsics=batch["intrinsic_matrix"], extrinsics=batch["extrinsic_matrix"],
                                     dist=batch["distortions"])
    reproj_world = project_3d_to_2d(points_3d=torch.mean(p3d, dim=1), intrinsics=batch["intrinsic_matrix"],
                                    extrinsics=batch["extrinsic_matrix"], dist=batch["distortions"])
    reproj_model = frame_to_model_batch(batch_dict=batch, frame_keypoints=reproj_world)
    err = torch.norm(flat - reproj_model.reshape(1, 12), dim=-1)
    print(f"full pipeline model-coordinate error: {float(err):.4f}")
    assert err < 5.0, f"Full pipeline round-trip failed: {err.item()}"
    fused_3d, fused_2d = ops.camera_chain(recovered, batch["intrinsic_matrix"], batch["extrinsic_matrix"], batch["distortions"], bbox, 256, 256)
    assert torch.equal(fused_3d, p3d)
    assert torch.allclose(fused_2d, reproj_model, rtol=1e-5, atol=1e-3)
