"""The camera-geometry kernels (csrc/cameras.hip: lp_cam_chain_fwd / _bwd, lp_cam_project_fwd / _bwd, lp_cam_pairwise_fwd_bwd) against the
float64 oracle tests/cameras_fp64.py.

Error measure, per tensor: max |got - want64| / max |want64|.  Bar: 4 x the same measure of the oracle run in float32 (the reference's
precision; the factor 4 is the trajectory test's convention for two correct fp32 orderings), never below 2^-24.  No case is skipped or
filtered.  Every figure is printed before it is asserted (run with -s; lines "cam3d_accuracy ..."): profiles/cam3d_accuracy.txt keeps
them per backend.
"""

import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import cameras_fp64 as O
from tests.hipemu import emu

FLOOR = 2.0 ** -24
# (name, B, V, K, distortion parameters; 0 = all-zero): 1 lane; the fly fixture; 150 lanes; 306; 816 = several waves per workgroup, 8 workgroups
CASES = [("one", 1, 2, 1, 5), ("fly", 1, 3, 2, 5), ("v6", 2, 6, 5, 8), ("k17", 3, 4, 17, 12), ("b8", 8, 4, 17, 0)]
MODEL_H, MODEL_W = 256.0, 320.0


@functools.lru_cache(maxsize=None)
def rig(name: str) -> dict:
    """inputs (float64) of a case, its cotangents, and the oracle's results in float64 and float32 - computed once, shared, never modified"""
    _, B, V, K, nd = next(c for c in CASES if c[0] == name)
    if name == "fly":
        r = O.fly_fixture()
        r["bbox"] = torch.tensor([[100, 50, 600, 600, 200, 100, 500, 500, 50, 75, 700, 700]], dtype=torch.float64)
        # the fixture's points are exact projections: 2 px of noise, as on the synthetic rigs, so that the DLT residual is non-zero
        r["points_2d"] = r["points_2d"] + 2.0 * torch.randn(r["points_2d"].shape, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    else:
        r = O.make_rig(B, V, K, nd, seed=B * 100 + V * 10 + K)
    g = torch.Generator().manual_seed(7)
    P = V * (V - 1) // 2
    r["g3d"] = torch.randn(B, P, K, 3, generator=g, dtype=torch.float64)
    r["g2d"] = torch.randn(B, V, K, 2, generator=g, dtype=torch.float64)
    r["targ3d"] = r["points_3d"] + 0.1 * torch.randn(B, K, 3, generator=g, dtype=torch.float64)
    for dt, tag in ((torch.float64, "64"), (torch.float32, "32")):
        r["want" + tag] = {k: v.double() for k, v in oracle(r, dt).items()}
    return r


def oracle(r: dict, dt, points=None, targ3d=None) -> dict:
    c = {k: v.to(dt) for k, v in r.items() if torch.is_tensor(v)}
    pts = (c["points_2d"] if points is None else points.to(dt)).clone().requires_grad_(True)
    targ = c["targ3d"] if targ3d is None else targ3d.to(dt)
    cam = (c["intrinsics"], c["extrinsics"], c["distortions"])
    p3d, p2d = O.chain(pts, *cam, c["bbox"], MODEL_H, MODEL_W)
    out = {"tri": p3d.detach(), "chain2d": p2d.detach()}
    nan3, nan2 = torch.isnan(p3d), torch.isnan(p2d)   # (cotangents only where the forward is defined: a NaN output takes no gradient)
    (torch.where(nan3, 0, p3d) * c["g3d"]).sum().backward(retain_graph=True)
    out["tri_grad"] = pts.grad.clone()
    pts.grad = None
    ((torch.where(nan3, 0, p3d) * c["g3d"]).sum() + (torch.where(nan2, 0, p2d) * c["g2d"]).sum()).backward()
    out["chain_grad"] = pts.grad.clone()
    X = c["points_3d"].clone().requires_grad_(True)
    q = O.project(X, *cam)
    out["proj"] = q.detach()
    (torch.where(torch.isnan(q), 0, q) * c["g2d"]).sum().backward()
    out["proj_grad"] = X.grad.clone()
    pred = p3d.detach().clone().requires_grad_(True)
    loss = O.pairwise_loss(targ, pred)
    loss.backward()
    out["pair_loss"], out["pair_grad"] = loss.detach().reshape(1), pred.grad.clone()
    return out


# ---- the kernels through the C ABI -------------------------------------------------------------------------------------------
def _f(t):
    return None if t is None else emu.B(np.ascontiguousarray(t.detach().numpy(), dtype=np.float32))


def kernels(r: dict, points=None, targ3d=None) -> dict:
    lib, st = emu.lib(), emu.stream()
    pts64 = r["points_2d"] if points is None else points
    B, V, K, _ = pts64.shape
    P = V * (V - 1) // 2
    d12 = O.dist12(r["distortions"])
    pts, intr, extr, dist, bbox = _f(pts64), _f(r["intrinsics"]), _f(r["extrinsics"]), _f(d12), _f(r["bbox"])
    p3d, p2d = emu.B(np.full((B, P, K, 3), 7.0, np.float32)), emu.B(np.full((B, V, K, 2), 7.0, np.float32))
    emu.ok(lib.lp_cam_chain_fwd(pts.p, intr.p, extr.p, dist.p, bbox.p, MODEL_H, MODEL_W, B, V, K, p3d.p, p2d.p, st))
    out = {"tri": p3d.np().copy(), "chain2d": p2d.np().copy()}
    tri_only = emu.B(np.full((B, P, K, 3), 7.0, np.float32))
    emu.ok(lib.lp_cam_chain_fwd(pts.p, intr.p, extr.p, dist.p, None, 1.0, 1.0, B, V, K, tri_only.p, None, st))
    assert np.array_equal(tri_only.np().view(np.uint32), out["tri"].view(np.uint32))
    nws = int(lib.lp_cam_chain_workspace_bytes(B, V, K))
    assert nws == 4 * (B * K * 3 + B * P * K * 4)
    g3, g2 = _f(r["g3d"]), _f(r["g2d"])
    for name, a3, a2 in (("tri_grad", g3, None), ("chain_grad", g3, g2)):
        ws = emu.B(np.full(nws // 4, np.nan, np.float32))   # (contents undefined on entry: nothing may be read before it is written)
        gp = emu.B(np.full((B, V, K, 2), np.nan, np.float32))
        emu.ok(lib.lp_cam_chain_bwd(pts.p, intr.p, extr.p, dist.p, bbox.p, MODEL_H, MODEL_W, B, V, K, p3d.p, emu.ptr(a3), emu.ptr(a2), ws.p,
                                    C.c_size_t(nws), gp.p, st))
        out[name] = gp.np().copy()
    X = _f(r["points_3d"])
    q, gX = emu.B(np.full((B, V, K, 2), 7.0, np.float32)), emu.B(np.full((B, K, 3), np.nan, np.float32))
    emu.ok(lib.lp_cam_project_fwd(X.p, intr.p, extr.p, dist.p, None, 1.0, 1.0, B, V, K, q.p, st))
    emu.ok(lib.lp_cam_project_bwd(X.p, intr.p, extr.p, dist.p, None, 1.0, 1.0, B, V, K, g2.p, gX.p, st))
    out["proj"], out["proj_grad"] = q.np().copy(), gX.np().copy()
    targ = _f(r["targ3d"] if targ3d is None else targ3d)
    loss, grad = emu.B(np.full(1, np.nan, np.float32)), emu.B(np.full((B, P, K, 3), np.nan, np.float32))
    emu.ok(lib.lp_cam_pairwise_fwd_bwd(targ.p, p3d.p, B, P, K, loss.p, grad.p, st))
    out["pair_loss"], out["pair_grad"] = loss.np().copy(), grad.np().copy()
    return out


def rel_err(got, want64: torch.Tensor) -> float:
    got = torch.as_tensor(np.asarray(got, dtype=np.float64)).reshape(want64.shape)
    assert not torch.isnan(want64).any()
    return float((got - want64).abs().max() / want64.abs().max())


TENSORS = ["tri", "chain2d", "proj", "tri_grad", "chain_grad", "proj_grad", "pair_loss", "pair_grad"]


@pytest.mark.parametrize("case", [c[0] for c in CASES])
def test_forward_and_gradients_within_four_times_the_fp32_oracle(kernel_backend, case):
    r = rig(case)
    got = kernels(r)
    lines, bad = [], []
    for name in TENSORS:
        # the pairwise loss's own input is the kernel's triangulation; the oracle's is its own: both are compared with the fp64 chain
        e_k, e_32 = rel_err(got[name], r["want64"][name]), rel_err(r["want32"][name].numpy(), r["want64"][name])
        bar = max(4.0 * e_32, FLOOR)
        lines.append(f"cam3d_accuracy {kernel_backend} {case:4s} {name:10s} kernel {e_k:.3e}  fp32-oracle {e_32:.3e}  ratio {e_k / max(e_32, 1e-300):.2f}  bar {bar:.3e}")
        if not e_k <= bar:
            bad.append(lines[-1])
    print("\n".join(lines))
    assert not bad, "\n".join(bad)


def _nan_points(r, pattern):
    pts = r["points_2d"].clone()
    targ = r["targ3d"].clone()
    if pattern == "one_view_of_one_keypoint":
        pts[0, 1, 0, 0] = float("nan")          # (x only: a half-NaN point is a NaN point)
    elif pattern == "whole_view":
        pts[:, 2] = float("nan")
    elif pattern == "every_view":
        pts[:] = float("nan")
    elif pattern == "nan_targets":
        targ[0, 1] = float("nan")
        targ[-1, :, 2] = float("nan")
    elif pattern == "nothing_valid":
        targ[:] = float("nan")
    return pts, targ


@pytest.mark.parametrize("pattern", ["one_view_of_one_keypoint", "whole_view", "every_view", "nan_targets", "nothing_valid"])
def test_nan_patterns(kernel_backend, pattern):
    r = rig("k17")
    pts, targ = _nan_points(r, pattern)
    got = kernels(r, points=pts, targ3d=targ)
    want = oracle(r, torch.float64, points=pts, targ3d=targ)
    for name in ("tri", "chain2d", "proj", "pair_loss"):       # outputs: NaN exactly where the oracle's are, the rest as accurate as ever
        w, g = want[name], torch.as_tensor(np.asarray(got[name], np.float64)).reshape(want[name].shape)
        assert torch.equal(torch.isnan(g), torch.isnan(w)), name
        ok = ~torch.isnan(w)
        if ok.any():
            assert float((g[ok] - w[ok]).abs().max()) <= 1e-4 * float(w[ok].abs().max()), name
    for name in ("tri_grad", "chain_grad", "proj_grad", "pair_grad"):   # gradients: never NaN, and the oracle's (a masked entry takes none)
        w, g = want[name], torch.as_tensor(np.asarray(got[name], np.float64)).reshape(want[name].shape)
        assert not torch.isnan(g).any(), name
        assert not torch.isnan(w).any(), name
        assert float((g - w).abs().max()) <= 1e-3 * max(float(w.abs().max()), 1e-30), name
    if pattern in ("every_view", "nothing_valid"):
        assert float(got["pair_loss"][0]) == 0.0 and not np.any(got["pair_grad"])
    if pattern == "every_view":
        assert not np.any(got["tri_grad"]) and not np.any(got["chain_grad"])


@pytest.mark.parametrize("case", ["v6", "b8"])
def test_two_calls_give_the_same_bits(kernel_backend, case):
    r = rig(case)
    a, b = kernels(r), kernels(r)
    for name in TENSORS:
        assert np.array_equal(a[name].view(np.uint32), b[name].view(np.uint32)), name


def test_bad_arguments_return_the_documented_codes(kernel_backend):
    lib, st = emu.lib(), emu.stream()
    ARG, UNSUPPORTED = -1, -2
    z = emu.Z(4096)
    assert int(lib.lp_cam_chain_workspace_bytes(1, 1, 3)) == 0 and int(lib.lp_cam_chain_workspace_bytes(1, 33, 3)) == 0
    assert lib.lp_cam_chain_fwd(z.p, z.p, z.p, z.p, None, 1.0, 1.0, 1, 1, 1, z.p, None, st) == ARG          # one view: no pair
    assert lib.lp_cam_chain_fwd(None, z.p, z.p, z.p, None, 1.0, 1.0, 1, 2, 1, z.p, None, st) == ARG
    assert lib.lp_cam_chain_fwd(z.p, z.p, z.p, z.p, None, 1.0, 1.0, 1, 33, 1, z.p, None, st) == UNSUPPORTED
    assert lib.lp_cam_chain_bwd(z.p, z.p, z.p, z.p, None, 1.0, 1.0, 1, 2, 1, z.p, None, None, z.p, C.c_size_t(4096), z.p, st) == ARG   # no cotangent
    assert lib.lp_cam_chain_bwd(z.p, z.p, z.p, z.p, None, 1.0, 1.0, 1, 2, 1, z.p, z.p, None, z.p, C.c_size_t(8), z.p, st) == ARG        # workspace too small
    assert lib.lp_cam_project_fwd(z.p, z.p, z.p, z.p, None, 1.0, 1.0, 0, 2, 1, z.p, st) == ARG
    assert lib.lp_cam_pairwise_fwd_bwd(z.p, z.p, 1, 0, 1, z.p, z.p, st) == ARG
