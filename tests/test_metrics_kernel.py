"""Prediction metrics at kernel level (include/lp_hip.h, csrc/metrics.hip): lp_kp_metrics.

Oracle: the four tables restated here in numpy and run in float64 on the kernel's own fp32 inputs.  Tolerance, per table and per case: 4 x
the largest distance of THE SAME restatement run in float32 from its float64 run on the same inputs (the margin tests/test_mv3d_kernels.py
and the camera tests use) - nothing is taken from what the kernel returns.  NaN patterns must equal the oracle's exactly.
The reference's own outputs (tests/golden/metrics.npz, written by tests/golden/make_golden_metrics.py) are checked as well, with that bar
plus the reference's own measured distance from float64: its add-the-mean-back reprojection loses digits at frame scale.
Inputs are frame scale: coordinates in 0 - 1300 px, residuals of a few px off a low-dimensional pose model.

``measure()`` returns the distances of every case; profiles/metrics_accuracy.py writes them to profiles/metrics_accuracy.txt."""

import ctypes as C
import itertools
import os

import numpy as np
import pytest

from lightning_pose_amd import _lib
from tests.hipemu import emu

ARG, UNSUPPORTED = -1, -2     # LP_ERR_ARGUMENT, LP_ERR_UNSUPPORTED (include/lp_hip.h)
TABLES = ("pixel_error", "temporal_norm", "pca_singleview", "pca_multiview")
CANARY, GUARD = np.float32(-54321.0), 96      # floats in front of and behind every output
GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metrics.npz"))


# ------------------------------------------------------------------------------------------------------------ the restatement
def restated(pred, labels, sv, mv, dtype):
    """the four (T, K) tables in ``dtype`` arithmetic; sv / mv: dict(index (rows, P), mean (2P), kept (ncomp, 2P)) or None"""
    pred = np.asarray(pred).astype(dtype)
    t, k, _ = pred.shape
    out = {}
    if labels is not None:
        d = np.asarray(labels).astype(dtype) - pred
        out["pixel_error"] = np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1])
    d = pred[1:] - pred[:-1]
    out["temporal_norm"] = np.concatenate([np.full((1, k), np.nan, dtype), np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1])])
    for name, spec in (("pca_singleview", sv), ("pca_multiview", mv)):
        if spec is None:
            continue
        table = np.full((t, k), np.nan, dtype)
        mean, kept = spec["mean"].astype(dtype), spec["kept"].astype(dtype)
        for row in np.asarray(spec["index"]):                       # one sample per frame and index row
            x = pred[:, row].reshape(t, -1) - mean
            r = x.copy()
            for v in kept:                                          # r = x - sum_c <x, v_c> v_c, one component after the other
                r = r - (x * v).sum(axis=1, keepdims=True) * v      # (a NaN coordinate reaches every entry through the sum)
            r = r.reshape(t, -1, 2)
            table[:, row] = np.sqrt(r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1])   # a column listed twice keeps its last entry
        out[name] = table
    return out


# ------------------------------------------------------------------------------------------------------------ calling the kernel
class _Spec:
    def __init__(self, spec, device_index=None):
        self.host = np.ascontiguousarray(spec["index"], dtype=np.int32)
        self.index = emu.Buf(self.host if device_index is None else np.ascontiguousarray(device_index, dtype=np.int32))
        self.mean, self.kept = emu.Buf(emu.f32(spec["mean"])), emu.Buf(emu.f32(spec["kept"]).reshape(-1) if spec["kept"].size else np.zeros(1, np.float32))
        rows, pts = self.host.shape
        self.struct = _lib.PcaSpec(self.index.p, self.host.ctypes.data, int(rows), int(pts), self.mean.p, self.kept.p,
                                   int(spec.get("ncomp", spec["kept"].shape[0])))


def run(pred, labels=None, sv=None, mv=None, want=TABLES, rc=False, dims=None):
    """-> {table: (T, K) float32}; every output sits between two guards of CANARY, which must come back untouched.  rc=True: the return code
    (and every output must be untouched).  ``want`` chooses the non-NULL output pointers."""
    pred = emu.f32(pred)
    t, k = dims or pred.shape[:2]
    pb, lb = emu.Buf(pred), None if labels is None else emu.Buf(emu.f32(labels))
    specs = {"pca_singleview": None if sv is None else _Spec(sv), "pca_multiview": None if mv is None else _Spec(mv)}
    n = int(pred.shape[0] * pred.shape[1])
    bufs = {name: emu.Buf(np.full(n + 2 * GUARD, CANARY, np.float32)) for name in want}
    ptr = lambda name: C.c_void_p(bufs[name].p.value + 4 * GUARD) if name in bufs else None   # noqa: E731
    ref = lambda name: None if specs[name] is None else C.byref(specs[name].struct)            # noqa: E731
    code = emu.lib().lp_kp_metrics(pb.p, None if lb is None else lb.p, int(t), int(k), ref("pca_singleview"), ref("pca_multiview"),
                                   ptr("pixel_error"), ptr("temporal_norm"), ptr("pca_singleview"), ptr("pca_multiview"), emu.stream())
    raw = {name: b.np() for name, b in bufs.items()}
    if rc:
        assert all((a == CANARY).all() for a in raw.values()), "a refused call wrote to an output"
        return code
    emu.ok(code)
    for name, a in raw.items():
        assert (a[:GUARD] == CANARY).all() and (a[-GUARD:] == CANARY).all(), f"{name}: written outside the table"
    return {name: a[GUARD:-GUARD].reshape(pred.shape[0], pred.shape[1]).copy() for name, a in raw.items()}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ------------------------------------------------------------------------------------------------------------ inputs
def pose_model(rng, k, latent=3):
    return rng.uniform(100.0, 1200.0, size=2 * k), rng.normal(scale=40.0, size=(latent, 2 * k))


def poses(rng, n, model):
    base, mixing = model
    return (base + rng.normal(size=(n, mixing.shape[0])) @ mixing + rng.normal(scale=2.0, size=(n, base.size))).astype(np.float32)


def fit(samples, ncomp):
    """mean and the first ``ncomp`` principal axes of (N, D) samples, fp32 (numpy SVD: the fit itself is not under test here)"""
    mean = samples.astype(np.float64).mean(axis=0)
    _, _, vt = np.linalg.svd(samples.astype(np.float64) - mean, full_matrices=True)
    return mean.astype(np.float32), vt[:ncomp].astype(np.float32)


def make_spec(train, index, ncomp):
    """index (rows, P) -> dict for ``run`` / ``restated``, fitted on the training poses (N, K, 2) formatted as the samples are"""
    index = np.asarray(index, dtype=np.int32).reshape(len(index), -1)
    samples = np.concatenate([train[:, row].reshape(len(train), -1) for row in index])
    mean, kept = fit(samples, ncomp)
    return dict(index=index, mean=mean, kept=kept)


def case_inputs(t, k, sv_cols, mv_views, ncomp_sv, ncomp_mv, seed):
    """sv_cols: list | "all" | None;  mv_views: V | None - the first V * (K // V) keypoints view-major, so K % V keypoints belong to no sample"""
    rng = np.random.default_rng(seed)
    model = pose_model(rng, k)
    train = poses(rng, max(4 * k, 16), model).reshape(-1, k, 2)
    pred = poses(rng, t, model).reshape(t, k, 2)
    labels = (pred + rng.normal(scale=30.0, size=pred.shape)).astype(np.float32)
    sv = mv = None
    if sv_cols is not None:
        cols = list(range(k)) if sv_cols == "all" else list(sv_cols)
        sv = make_spec(train, [cols], min(ncomp_sv if ncomp_sv > 0 else 2 * len(cols) - 1, 2 * len(cols)))
    if mv_views is not None:
        j = k // mv_views
        index = np.arange(mv_views * j).reshape(mv_views, j).T        # (rows = matched keypoints, points = views)
        mv = make_spec(train, index, min(ncomp_mv if ncomp_mv > 0 else 2 * mv_views - 1, 2 * mv_views))
    return pred, labels, sv, mv


# (T, K, single-view columns, multi-view V, ncomp single-view, ncomp multi-view); ncomp 0 stands for 2 P - 1
#   T: one row, wave boundaries (4 waves take frames in turn), one 64-frame chunk + 1, several chunks, 4099 = 64 chunks + 3
#   K: 1, 3, 17, 64 (P = 64: every lane a point);  V in {2, 4} with keypoints left out (K = 3: one, K = 17: one, K = 64 with V = 4: none)
SHAPES = [
    (1, 1, "all", None, 1, 0), (2, 1, "all", None, 0, 0), (3, 3, "all", 2, 3, 0), (65, 1, "all", None, 1, 0),
    (1, 17, "all", 4, 3, 3), (2, 17, [0, 3, 4, 9, 16], 2, 0, 1), (3, 17, [5], 4, 1, 0), (65, 17, "all", 4, 0, 3),
    (257, 17, [0, 3, 4, 9, 16], 2, 3, 3), (4099, 17, "all", 4, 3, 3), (4099, 3, [1], 2, 0, 0), (257, 3, "all", 2, 1, 1),
    (1, 64, "all", 4, 0, 0), (3, 64, "all", 2, 3, 3), (65, 64, list(range(1, 64, 2)), 4, 1, 3), (257, 64, "all", 2, 3, 0), (2, 3, [0, 2], 2, 1, 3),
]


def distances(pred, labels, sv, mv, got):
    """per table: (bar = 4 x |fp32 restatement - fp64 restatement|_max, |kernel - fp64|_max, NaN masks equal)"""
    want, low = restated(pred, labels, sv, mv, np.float64), restated(pred, labels, sv, mv, np.float32)
    out = {}
    for name, g in got.items():
        w = want[name]
        same_nan = np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(np.isnan(low[name]), np.isnan(w))
        fin = ~np.isnan(w)
        bar = 4.0 * float(np.abs(low[name].astype(np.float64) - w)[fin].max()) if fin.any() else 0.0
        err = float(np.abs(g.astype(np.float64) - w)[fin & ~np.isnan(g)].max()) if (fin & ~np.isnan(g)).any() else 0.0
        out[name] = (bar, err, same_nan)
    return out


def measure():
    """[(case label, {table: (bar, err, same_nan)})] over SHAPES on the current backend (profiles/metrics_accuracy.py)"""
    rows = []
    for i, (t, k, cols, views, nsv, nmv) in enumerate(SHAPES):
        pred, labels, sv, mv = case_inputs(t, k, cols, views, nsv, nmv, seed=100 + i)
        rows.append((f"T={t} K={k} sv={'all' if cols == 'all' else len(cols)} V={views}", distances(pred, labels, sv, mv, run(pred, labels, sv, mv,
                     [n for n in TABLES if n != "pca_multiview" or mv is not None]))))
    return rows


@pytest.mark.parametrize("case", range(len(SHAPES)), ids=[f"T{s[0]}-K{s[1]}-{i}" for i, s in enumerate(SHAPES)])
def test_tables_against_float64(kernel_backend, case):
    t, k, cols, views, nsv, nmv = SHAPES[case]
    pred, labels, sv, mv = case_inputs(t, k, cols, views, nsv, nmv, seed=100 + case)
    want = [n for n in TABLES if n != "pca_multiview" or mv is not None]
    got = run(pred, labels, sv, mv, want)
    assert sorted(got) == sorted(want)
    for name, (bar, err, same_nan) in distances(pred, labels, sv, mv, got).items():
        print(f"{name}: |kernel - fp64| = {err:.3e}, bar = {bar:.3e}")
        assert same_nan, f"{name}: NaN pattern differs from the oracle's"
        assert err <= bar, f"{name}: {err:.3e} > {bar:.3e}"
    assert np.isnan(got["temporal_norm"][0]).all() and not np.isnan(got["temporal_norm"][1:]).any() and not np.isnan(got["pixel_error"]).any()
    if cols != "all":
        unselected = sorted(set(range(k)) - set(cols))
        assert np.isnan(got["pca_singleview"][:, unselected]).all() and not np.isnan(got["pca_singleview"][:, cols]).any()
    if mv is not None:
        used = views * (k // views)
        assert np.isnan(got["pca_multiview"][:, used:]).all() and not np.isnan(got["pca_multiview"][:, :used]).any()


def test_golden_reference_outputs(kernel_backend):
    """the reference's own four functions on the fixture's inputs, with its own fitted parameters"""
    g = GOLDEN
    sv = dict(index=g["sv_columns"].reshape(1, -1), mean=g["sv_mean"], kept=g["sv_kept"])
    mv = dict(index=np.ascontiguousarray(g["mv_matches"].T), mean=g["mv_mean"], kept=g["mv_kept"])
    got = run(g["pred"], g["labels"], sv, mv)
    want = restated(g["pred"], g["labels"], sv, mv, np.float64)
    dist = distances(g["pred"], g["labels"], sv, mv, got)
    for name in TABLES:
        ref = g["ref_" + name]
        assert np.array_equal(np.isnan(ref), np.isnan(want[name])), f"{name}: the restatement's NaN pattern is not the reference's"
        fin = ~np.isnan(ref)
        ref_own = float(np.abs(ref - want[name])[fin].max())                 # the reference's own distance from float64
        bar, err, same_nan = dist[name]
        vs_ref = float(np.abs(got[name].astype(np.float64) - ref)[fin].max())
        print(f"{name}: |kernel - ref| = {vs_ref:.3e}, |ref - fp64| = {ref_own:.3e}, |kernel - fp64| = {err:.3e}, bar = {bar:.3e}")
        assert same_nan and np.array_equal(np.isnan(got[name]), np.isnan(ref))
        assert err <= bar and vs_ref <= bar + ref_own
    # what the fixture is meant to hold: one NaN prediction coordinate (frame 11, keypoint 1) and what the reference makes of it
    assert np.isnan(g["pred"]).sum() == 1 and np.isnan(g["pred"][11, 1, 0])
    assert np.isnan(g["ref_pca_singleview"][11]).all() and np.isnan(g["ref_pca_singleview"]).sum() == 3 * 37 + 5
    assert np.isnan(g["ref_pca_multiview"][11, [1, 5]]).all() and np.isnan(g["ref_pca_multiview"]).sum() == 2 * 37 + 2


def _nan_case():
    pred, labels, sv, mv = case_inputs(65, 17, [0, 3, 4, 9, 16], 4, 3, 3, seed=7)
    return pred.copy(), labels.copy(), sv, mv


def test_nan_patterns_equal_the_oracles(kernel_backend):
    pred, labels, sv, mv = _nan_case()
    labels[2, 5, 0] = np.nan                 # one label coordinate
    labels[9, 1] = np.nan                    # a whole label
    pred[20, 4, 1] = np.nan                  # selected single-view; multi-view: matched keypoint 0 of view 1 (columns 0, 4, 8, 12)
    pred[30, 2, 0] = np.nan                  # NOT selected single-view; multi-view: matched keypoint 2 of view 0 (columns 2, 6, 10, 14)
    pred[31, 16, 0] = np.nan                 # selected single-view; in no multi-view sample
    pred[40] = np.nan                        # an all-NaN frame
    got = run(pred, labels, sv, mv)
    want = restated(pred, labels, sv, mv, np.float64)
    for name in TABLES:
        assert np.array_equal(np.isnan(got[name]), np.isnan(want[name])), name
    nan_at = lambda a: {tuple(int(v) for v in i) for i in np.argwhere(np.isnan(a))}   # noqa: E731
    frames = (20, 30, 31, 40)
    assert nan_at(got["pixel_error"]) == {(2, 5), (9, 1), (20, 4), (30, 2), (31, 16)} | {(40, c) for c in range(17)}
    assert nan_at(got["temporal_norm"]) == ({(0, c) for c in range(17)} | {(20, 4), (21, 4), (30, 2), (31, 2), (31, 16), (32, 16)}
                                            | {(t, c) for t in (40, 41) for c in range(17)})
    sel, unsel = [0, 3, 4, 9, 16], sorted(set(range(17)) - {0, 3, 4, 9, 16})
    assert nan_at(got["pca_singleview"]) == {(t, c) for t in range(65) for c in unsel} | {(t, c) for t in (20, 31, 40) for c in sel}
    assert nan_at(got["pca_multiview"]) == ({(t, 16) for t in range(65)} | {(20, c) for c in (0, 4, 8, 12)} | {(30, c) for c in (2, 6, 10, 14)}
                                            | {(40, c) for c in range(16)})
    for t in frames:                          # the frames around them are finite where they should be
        assert not np.isnan(got["pca_singleview"][t - 2, sel]).any()


def test_every_subset_of_outputs_gives_the_same_bits(kernel_backend):
    pred, labels, sv, mv = case_inputs(67, 17, [0, 3, 4, 9, 16], 4, 3, 3, seed=11)
    full = run(pred, labels, sv, mv)
    again = run(pred, labels, sv, mv)
    for name in TABLES:
        assert np.array_equal(bits(full[name]), bits(again[name])), f"{name}: two runs differ"
    for n in range(1, 4):
        for want in itertools.combinations(TABLES, n):
            got = run(pred, labels if "pixel_error" in want else None, sv if "pca_singleview" in want else None,
                      mv if "pca_multiview" in want else None, want)
            assert sorted(got) == sorted(want)
            for name in want:
                assert np.array_equal(bits(got[name]), bits(full[name])), (want, name)
    # specs and labels may also be passed without their table being wanted
    got = run(pred, labels, sv, mv, ("temporal_norm",))
    assert np.array_equal(bits(got["temporal_norm"]), bits(full["temporal_norm"]))


def test_rows_do_not_depend_on_the_launch_geometry(kernel_backend):
    """T = 4099 (65 chunks) equals the T = 4098 call on the first rows + the last row of a T = 2 call on the last two rows"""
    pred, labels, sv, mv = case_inputs(4099, 17, [0, 3, 4, 9, 16], 4, 3, 3, seed=13)
    full, head, tail = run(pred, labels, sv, mv), run(pred[:4098], labels[:4098], sv, mv), run(pred[4097:], labels[4097:], sv, mv)
    for name in TABLES:
        assert np.array_equal(bits(full[name]), bits(np.concatenate([head[name], tail[name][1:]]))), name


def test_a_column_listed_twice_keeps_its_last_entry(kernel_backend):
    pred, labels, _, _ = case_inputs(5, 6, None, None, 0, 0, seed=17)
    rng = np.random.default_rng(3)
    sv = dict(index=np.array([[2, 4, 2]], np.int32), mean=rng.uniform(100, 1200, 6).astype(np.float32),
              kept=np.linalg.qr(rng.normal(size=(6, 2)))[0].T.astype(np.float32))
    got = run(pred, None, sv, None, ("pca_singleview",))["pca_singleview"]
    want, low = restated(pred, None, sv, None, np.float64)["pca_singleview"], restated(pred, None, sv, None, np.float32)["pca_singleview"]
    assert np.array_equal(np.isnan(got), np.isnan(want)) and not np.isnan(got[:, [2, 4]]).any()
    assert np.abs(got - want)[:, [2, 4]].max() <= 4.0 * np.abs(low - want)[:, [2, 4]].max()


def test_refusals_launch_nothing(kernel_backend):
    pred, labels, sv, mv = case_inputs(9, 70, list(range(64)), 2, 3, 3, seed=19)
    bad = lambda **kw: dict(sv, **kw)   # noqa: E731
    wide = dict(index=np.arange(65, dtype=np.int32).reshape(1, 65), mean=np.zeros(130, np.float32), kept=np.zeros((1, 130), np.float32))
    assert run(pred, labels, wide, mv, rc=True) == ARG                                            # P = 65
    for value in (70, -1):                                                                        # an index equal to K, a negative index
        index = sv["index"].copy()
        index[0, 17] = value
        assert run(pred, labels, bad(index=index), mv, rc=True) == ARG
        index = mv["index"].copy()
        index[3, 1] = value
        assert run(pred, labels, sv, dict(mv, index=index), rc=True) == ARG
    small = make_spec(np.zeros((8, 70, 2), np.float32) + np.arange(8, dtype=np.float32)[:, None, None], [[1, 2]], 4)
    assert run(pred, labels, dict(small, ncomp=5), mv, rc=True) == ARG                             # ncomp > 2 P
    assert run(pred, labels, dict(small, ncomp=-1), mv, rc=True) == ARG
    assert run(pred, labels, dict(small, index=np.array([[1, 2], [3, 4]], np.int32)), None, ("pca_singleview",), rc=True) == ARG   # rows != 1
    assert run(pred, None, sv, mv, rc=True) == ARG                                                 # pixel error without labels
    assert run(pred, labels, None, mv, rc=True) == ARG                                             # a PCA table without its spec
    assert run(pred, labels, sv, mv, (), rc=True) == ARG                                           # no output
    assert run(pred, labels, sv, mv, rc=True, dims=(0, 70)) == ARG
    assert run(pred, labels, sv, mv, rc=True, dims=(9, 0)) == ARG
    assert run(pred, labels, None, None, ("temporal_norm",), rc=True, dims=(1 << 24, 64)) == UNSUPPORTED   # 2 T K = 2^31 elements
    # eigenvectors + owner maps beyond one workgroup's LDS: 2 x (127 x 128 + K) words is 130 KB at K = 70 and 202 KB at K = 9000
    big = dict(index=np.arange(64, dtype=np.int32).reshape(1, 64), mean=np.zeros(128, np.float32), kept=np.zeros((127, 128), np.float32))
    wide_pred = np.zeros((1, 9000, 2), np.float32)
    assert run(wide_pred, None, big, big, ("pca_singleview", "pca_multiview"), rc=True) == UNSUPPORTED
