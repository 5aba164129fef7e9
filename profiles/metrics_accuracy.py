"""Measured distances behind the tolerances of tests/test_metrics_kernel.py, written to ``--out`` (default profiles/metrics_accuracy.txt).

Per case of the test's shape list and per table: |fp32 restatement - fp64 restatement|_max (the test's bar is 4 x this), |kernel - fp64|_max,
and whether the NaN patterns agree.  Then the fixture tests/golden/metrics.npz: the reference's own outputs against float64 (its
add-the-mean-back reprojection loses digits at frame scale) and the kernel against both.  ``--backend gpu`` runs the product library on the
device, the default ``emu`` the host build of the same kernel sources (same arithmetic: the kernel contracts no product into an FMA).

    python profiles/metrics_accuracy.py [--backend gpu]
"""

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import _lp_bootstrap  # noqa: E402,F401
from tests import test_metrics_kernel as K  # noqa: E402
from tests.hipemu import emu  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--backend", choices=["emu", "gpu"], default="emu")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metrics_accuracy.txt"))
    a = ap.parse_args()
    emu.BACKEND = a.backend
    where = "the device (product library)" if a.backend == "gpu" else "the host build of the kernel sources (tests/hipemu); NOT measured on the device"
    lines = [f"lp_kp_metrics against float64, on {where}.  px; bar = 4 x |fp32 restatement - fp64|_max of the same inputs", ""]
    worst = {}
    for label, dist in K.measure():
        for name, (bar, err, same_nan) in dist.items():
            lines.append(f"{label:32s} {name:15s} fp32-fp64 {bar / 4:.3e}  kernel-fp64 {err:.3e}  bar {bar:.3e}  NaN pattern {'equal' if same_nan else 'DIFFERS'}"
                         f"  {'ok' if err <= bar and same_nan else 'MISSED'}")
            worst[name] = max(worst.get(name, 0.0), err)
    lines += ["", "largest |kernel - fp64| over the cases: " + ", ".join(f"{n} {v:.3e}" for n, v in worst.items()), ""]
    g = K.GOLDEN
    sv = dict(index=g["sv_columns"].reshape(1, -1), mean=g["sv_mean"], kept=g["sv_kept"])
    mv = dict(index=np.ascontiguousarray(g["mv_matches"].T), mean=g["mv_mean"], kept=g["mv_kept"])
    got, want = K.run(g["pred"], g["labels"], sv, mv), K.restated(g["pred"], g["labels"], sv, mv, np.float64)
    lines.append("tests/golden/metrics.npz (the reference's own functions and fit; T = 37, K = 8; largest finite value per table in brackets):")
    for name in K.TABLES:
        ref = g["ref_" + name]
        fin = ~np.isnan(ref)
        lines.append(f"  {name:15s} [{ref[fin].max():8.3f}]  reference-fp64 {np.abs(ref - want[name])[fin].max():.3e}  kernel-fp64 "
                     f"{np.abs(got[name] - want[name])[fin].max():.3e}  kernel-reference {np.abs(got[name] - ref)[fin].max():.3e}")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
