"""Cost of ops/metrics.average_precision_device against auc_radix on the same scores (device
events, the two alternating, median of --reps after a warm-up).  Prints one JSON line.

    python tools/pr_cost.py [--rows 2000000] [--reps 30] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fraud_detection_amd.ops import metrics as M  # noqa: E402
from fraud_detection_amd.ops import reference as ref  # noqa: E402


def one(fn) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--rows", type=int, default=2_000_000)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("pr_cost needs a GPU: a CPU timing says nothing about the kernels")
    dev = torch.device("cuda", 0)
    n = a.rows
    g = np.random.default_rng(0)
    y = (g.random(n) < 0.0017).astype(np.uint8)
    s = (g.standard_normal(n) + 2.0 * y).astype(np.float32)
    res = {"rows": n, "reps": a.reps}
    for name, sc in (("distinct", s), ("tied_1_64", (np.round(s * 64) / 64).astype(np.float32))):
        st, yt = torch.from_numpy(sc).to(dev), torch.from_numpy(y).to(dev)
        ws = M.pr_workspace(n, dev)
        _, r = M.average_precision_device(st, yt, ws=ws)
        assert r.cpu().tolist()[:3] == list(ref.average_precision_q(sc, y))
        fns = {"auc_radix": lambda: M.auc_radix(st, yt),
               "average_precision_device": lambda: M.average_precision_device(st, yt),
               "average_precision_device_ws": lambda: M.average_precision_device(st, yt, ws=ws),
               "pr_curve": lambda: M.pr_curve(st, yt)}  # kernels + output allocation + the two read-backs
        for _ in range(5):
            for fn in fns.values():
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in fns}
        for _ in range(a.reps):
            for k, fn in fns.items():
                ms[k].append(one(fn))
        out = {k: {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(np.min(v)), 4),
                   "max_ms": round(float(np.max(v)), 4)} for k, v in ms.items()}
        out["groups"] = int(r[3].item())
        out["ratio_ap_over_auc"] = round(out["average_precision_device"]["median_ms"] / out["auc_radix"]["median_ms"], 3)
        res[name] = out
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
