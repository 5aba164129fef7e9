"""Oracle of the camera geometry (csrc/cameras.hip): the formulas of include/lp_hip.h in torch, with torch.linalg.svd and autograd.

Run in float64 it is the truth the kernels are measured against; the SAME code in float32 is "the reference's precision" (the reference
runs kornia's float32 torch ops).  Vectorised over samples, pairs and keypoints; NaN inputs are masked the way the reference does it
(cameras.py:45-79: a pair with a NaN point is filled with a NaN constant, so it takes no gradient).  Also: synthetic calibrated rigs.
"""

from __future__ import annotations

import itertools
import os

import numpy as np
import torch

GUARD = 1e-8
ITERS = 5


def dist12(dist: torch.Tensor) -> torch.Tensor:
    n = dist.shape[-1]
    assert n in (4, 5, 8, 12), n
    return torch.nn.functional.pad(dist, (0, 12 - n))


def _coeffs(d: torch.Tensor):
    """(..., 12) -> k1 k2 p1 p2 k3 k4 k5 k6 s1 s2 s3 s4, each (..., 1) to broadcast over the keypoints"""
    return [d[..., i:i + 1] for i in range(12)]


def undistort(points, intrinsics, dist):
    """points (B, V, K, 2) px -> normalised undistorted (x, y), each (B, V, K)"""
    k1, k2, p1, p2, k3, k4, k5, k6, s1, s2, s3, s4 = _coeffs(dist12(dist))
    fx, fy, cx, cy = (intrinsics[..., 0, 0:1], intrinsics[..., 1, 1:2], intrinsics[..., 0, 2:3], intrinsics[..., 1, 2:3])
    x0, y0 = (points[..., 0] - cx) / fx, (points[..., 1] - cy) / fy
    x, y = x0, y0
    for _ in range(ITERS):
        r2 = x * x + y * y
        inv = (1 + k4 * r2 + k5 * r2 ** 2 + k6 * r2 ** 3) / (1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3)
        dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x) + s1 * r2 + s2 * r2 ** 2
        dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y + s3 * r2 + s4 * r2 ** 2
        x, y = (x0 - dx) * inv, (y0 - dy) * inv
    return x, y


def _guarded_recip(w):
    return torch.where(w.abs() > GUARD, 1.0 / torch.where(w.abs() > GUARD, w, torch.ones_like(w)), torch.ones_like(w))


def triangulate_pairs(points, intrinsics, extrinsics, dist):
    """(B, V, K, 2) -> (B, P, K, 3): homogeneous DLT of every camera pair (itertools.combinations order); NaN where either view is NaN"""
    nan = torch.isnan(points).any(-1)                                        # (B, V, K)
    clean = torch.where(nan[..., None], torch.zeros_like(points), points)    # (the masked pairs are computed on zeros and thrown away)
    x, y = undistort(clean, intrinsics, dist)
    out = []
    for j1, j2 in itertools.combinations(range(points.shape[1]), 2):
        P1, P2 = extrinsics[:, j1, None], extrinsics[:, j2, None]            # (B, 1, 3, 4)
        A = torch.stack([x[:, j1, :, None] * P1[..., 2, :] - P1[..., 0, :], y[:, j1, :, None] * P1[..., 2, :] - P1[..., 1, :],
                         x[:, j2, :, None] * P2[..., 2, :] - P2[..., 0, :], y[:, j2, :, None] * P2[..., 2, :] - P2[..., 1, :]], dim=-2)
        h = torch.linalg.svd(A)[2][..., -1, :]                               # (B, K, 4)
        X = h[..., :3] * _guarded_recip(h[..., 3:4])
        bad = (nan[:, j1] | nan[:, j2])[..., None]
        out.append(torch.where(bad, torch.full_like(X, float("nan")), X))
    return torch.stack(out, dim=1)


def project(points_3d, intrinsics, extrinsics, dist, bbox=None, model_h=1.0, model_w=1.0):
    """(B, K, 3) -> (B, V, K, 2) px (model px with bbox (B, 4 V) rows [x, y, h, w] per view)"""
    k1, k2, p1, p2, k3, k4, k5, k6, s1, s2, s3, s4 = _coeffs(dist12(dist))
    R, t = extrinsics[..., :3], extrinsics[..., 3]                           # (B, V, 3, 3), (B, V, 3)
    Xc = torch.einsum("bvrc,bkc->bvkr", R, points_3d) + t[:, :, None, :]
    s = _guarded_recip(Xc[..., 2])
    x, y = Xc[..., 0] * s, Xc[..., 1] * s
    r2 = x * x + y * y
    rad = (1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3) / (1 + k4 * r2 + k5 * r2 ** 2 + k6 * r2 ** 3)
    xd = x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x * x) + s1 * r2 + s2 * r2 ** 2
    yd = y * rad + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y + s3 * r2 + s4 * r2 ** 2
    u = intrinsics[..., 0, 0:1] * xd + intrinsics[..., 0, 2:3]
    v = intrinsics[..., 1, 1:2] * yd + intrinsics[..., 1, 2:3]
    if bbox is not None:
        bb = bbox.reshape(bbox.shape[0], -1, 4)
        u = (u - bb[..., 0:1]) / bb[..., 3:4] * model_w
        v = (v - bb[..., 1:2]) / bb[..., 2:3] * model_h
    return torch.stack([u, v], dim=-1)


def chain(points, intrinsics, extrinsics, dist, bbox=None, model_h=1.0, model_w=1.0):
    """-> every pair's triangulation (B, P, K, 3) and the mean of the pairs (one NaN pair makes it NaN) reprojected into every view (B, V, K, 2).
    A NaN mean is projected as zeros and masked afterwards, so that autograd passes it no gradient instead of 0 * NaN."""
    p3d = triangulate_pairs(points, intrinsics, extrinsics, dist)
    mean = torch.mean(p3d, dim=1)
    bad = torch.isnan(mean).any(-1, keepdim=True)                            # (B, K, 1)
    p2d = project(torch.where(bad, torch.zeros_like(mean), mean), intrinsics, extrinsics, dist, bbox, model_h, model_w)
    return p3d, torch.where(bad[:, None], torch.full_like(p2d, float("nan")), p2d)


def pairwise_loss(targ, pred):
    """reference losses/losses.py:1014-1126, NaN-safe as there"""
    bad = torch.isnan(targ).any(-1)[:, None] | torch.isnan(pred).any(-1)     # (B, P, K)
    ct = torch.where(torch.isnan(targ).any(-1)[..., None], torch.zeros_like(targ), targ)
    cp = torch.where(bad[..., None], torch.zeros_like(pred), pred)
    d = torch.linalg.norm(ct[:, None] - cp, ord=2, dim=-1)
    valid = ~bad
    if not bool(valid.any()):
        return torch.where(valid, d, torch.zeros_like(d)).sum()
    return d[valid].mean()


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def fly_fixture() -> dict:
    """the anipose-fly calibration and points of the reference's tests/data/test_cameras.py (tests/golden/cameras_fly.npz), float64"""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cameras_fly.npz")
    with np.load(path, allow_pickle=False) as z:
        return {k: torch.from_numpy(z[k].astype(np.float64)) for k in z.files}


def make_rig(B: int, V: int, K: int, ndist: int, seed: int, noise_px: float = 2.0) -> dict:
    """Synthetic calibrated rig, float64: cameras on a ring around the origin at distance 10 - 50, >= 30 degrees apart and all 20 - 35 degrees
    above the plane (so no two look along the same line), looking at the origin; f in 1000 - 2000; points in a unit cube; ``noise_px`` of noise on
    the projected points, so the DLT residual is non-zero.  ``ndist`` in {0, 5, 8, 12}: 0 = five all-zero parameters."""
    g = torch.Generator().manual_seed(seed)

    def U(lo, hi, *shape):
        return lo + (hi - lo) * torch.rand(*shape, generator=g, dtype=torch.float64)

    step = min(360.0 / V, 70.0)
    az = torch.deg2rad(torch.arange(V, dtype=torch.float64)[None] * step + U(-5, 5, B, V))
    el = torch.deg2rad(U(20, 35, B, V))
    C = U(10, 50, B, V)[..., None] * torch.stack([az.cos() * el.cos(), az.sin() * el.cos(), el.sin()], -1)   # camera centres
    fwd = -C / C.norm(dim=-1, keepdim=True)
    up = torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64).expand_as(fwd)
    right = torch.linalg.cross(fwd, up)
    right = right / right.norm(dim=-1, keepdim=True)
    down = torch.linalg.cross(fwd, right)
    R = torch.stack([right, down, fwd], dim=-2)
    extr = torch.cat([R, -(R @ C[..., None])], dim=-1)
    intr = torch.zeros(B, V, 3, 3, dtype=torch.float64)
    f = U(1000, 2000, B, V)
    intr[..., 0, 0], intr[..., 1, 1], intr[..., 2, 2] = f, f * U(0.98, 1.02, B, V), 1.0
    intr[..., 0, 2], intr[..., 1, 2] = 640 + U(-20, 20, B, V), 512 + U(-20, 20, B, V)
    scale = torch.tensor([0.3, 0.1, 0.01, 0.01, 0.05, 0.1, 0.1, 0.1, 0.01, 0.01, 0.01, 0.01], dtype=torch.float64)
    n = ndist if ndist else 5
    dist = U(-1, 1, B, V, n) * scale[:n] * (1.0 if ndist else 0.0)
    X = U(-0.5, 0.5, B, K, 3)
    pts = project(X, intr, extr, dist) + noise_px * torch.randn(B, V, K, 2, generator=g, dtype=torch.float64)
    bbox = torch.stack([U(0, 200, B, V), U(0, 200, B, V), U(600, 900, B, V), U(700, 1000, B, V)], -1).reshape(B, 4 * V)
    return {"points_2d": pts, "points_3d": X, "intrinsics": intr, "extrinsics": extr, "distortions": dist, "bbox": bbox}
