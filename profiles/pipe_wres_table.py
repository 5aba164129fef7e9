"""Per launch class (layer x first / later block x 1x1 convolution x forward / data gradient): the ring form of conv_pipe_kernel against its
weight-resident form, from the per-launch dumps bench.py writes with LP_DUMP_LAUNCHES (see profiles/layer_table.py).

    python profiles/pipe_wres_table.py parent=p.json ring=r1.json ring=r2.json resident=w1.json resident=w2.json

`ring` = this tree with LP_PIPE_WRES=0, `resident` = with LP_PIPE_WRES=2, `parent` = the commit before (optional).  A class is marked
faster only if the mean of its resident runs is below the mean of its ring runs by more than the spread the ring shows between its own
runs; the performance rule of route_conv() (conv.hip: wres_tuned) admits exactly those classes."""
import json
import sys

from layer_table import short

PLANES = {1: 64, 2: 128, 3: 256, 4: 512}


def shape(li: int, first: bool, conv: str, kind: str):
    """(K, N, stride) of the GEMM a ResNet-50 1x1 launch runs (the data gradient contracts over the output channels)"""
    p = PLANES[li]
    cin = (64 if li == 1 else 2 * p) if first else 4 * p
    ci, co, stride = {"c1": (cin, p, 1), "c3": (p, 4 * p, 1), "down": (cin, 4 * p, 1 if li == 1 else 2)}[conv]
    return (ci, co, stride) if kind == "fwd" else (co, ci, stride)


def admits(K: int, N: int, stride: int) -> bool:
    return stride == 1 and K * (128 if N > 64 else 64) * 2 <= 64 * 1024


def classes(path: str) -> dict:
    out: dict = {}
    for tag, _gflop, us, _mb, layer in json.load(open(path)):
        if not layer.startswith("backbone.") or "wgrad" in tag:
            continue
        name = short(layer)
        if name == "stem" or name.split(".")[2] == "c2":
            continue
        li, blk, conv = name.split(".")
        key = (int(li[1:]), blk == "0", conv, "dgrad" if "dgrad" in tag else "fwd")
        rec = out.setdefault(key, [0.0, 0])
        rec[0] += us
        rec[1] += 1
    return out


def main():
    runs: dict = {"parent": [], "ring": [], "resident": []}
    for arg in sys.argv[1:]:
        label, path = arg.split("=", 1)
        runs[label].append(classes(path))
    keys = sorted(runs["ring"][0])
    cols = [(lab, i) for lab in ("parent", "ring", "resident") for i in range(len(runs[lab]))]
    print("us per launch class and step (sum over the class's launches; n = launches)")
    print(f"{'class':22s} {'K':>4s} {'N':>5s} {'n':>3s} | " + " ".join(f"{lab[:6] + str(i + 1):>9s}" for lab, i in cols) + " | ring spread   gain   verdict")
    tot = {"ring": 0.0, "resident": 0.0, "tuned": 0.0}
    for key in keys:
        li, first, conv, kind = key
        K, N, stride = shape(li, first, conv, kind)
        vals = [runs[lab][i].get(key, [0.0, 0])[0] for lab, i in cols]
        ring = [r[key][0] for r in runs["ring"]]
        res = [r[key][0] for r in runs["resident"]]
        spread = max(ring) - min(ring)
        gain = sum(ring) / len(ring) - sum(res) / len(res)
        ok = admits(K, N, stride)
        verdict = "not eligible" if not ok else "FASTER" if gain > spread else "not faster"
        tot["ring"] += sum(ring) / len(ring)
        tot["resident"] += sum(res) / len(res)
        tot["tuned"] += sum(res) / len(res) if verdict == "FASTER" else sum(ring) / len(ring)
        name = f"l{li}.{'0' if first else 'x'}.{conv} {kind}"
        print(f"{name:22s} {K:4d} {N:5d} {runs['ring'][0][key][1]:3d} | " + " ".join(f"{v:9.1f}" for v in vals) + f" | {spread:11.1f} {gain:6.1f}   {verdict}")
    print(f"totals (ms per step): ring {tot['ring'] / 1e3:.3f}  resident everywhere {tot['resident'] / 1e3:.3f}  resident where FASTER {tot['tuned'] / 1e3:.3f}")


if __name__ == "__main__":
    main()
