"""Device timing of the partial-dependence kernel (csrc/kernels/tree_pd.hip) against what a user
did before it existed, on the same rows in one session:

* new: all ``d`` single-feature curves of a ``--trees``-tree depth-5 model over ``--rows`` x 30 rows,
  one ``ops.pdp.partial_dependence`` call per feature (scaler pass + one kernel launch each);
* baseline: per feature one copy of X and, per cell, the column overwritten with the cell's value,
  one ``gbdt_predict`` launch and a float mean on the device.

Medians of HIP-event times around a whole sweep over the 30 features, after warm-up sweeps; the
two sweeps alternate.  Also checks that both give the same curves (the baseline's float mean
against the exact integer mean).  Prints one JSON line (and writes it to ``--json``).

    python tools/pdp_bench.py [--rows 100000] [--reps 5] [--json out.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fraud_detection_amd.models.explainers import TreePartialDependence  # noqa: E402
from fraud_detection_amd.ops import gbdt as gb  # noqa: E402
from fraud_detection_amd.ops import reference_gbdt as R  # noqa: E402
from fraud_detection_amd.ops.pdp import partial_dependence  # noqa: E402


def random_ensemble(d, depth, T, seed):
    rng = np.random.default_rng(seed)
    ni = (1 << depth) - 1
    feat = rng.integers(0, d, (T, ni)).astype(np.int32)
    thr = rng.normal(0, 0.7, (T, ni)).astype(np.float32)
    leaf = rng.normal(0, 0.1, (T, 1 << depth)).astype(np.float32)
    return gb.TreeEnsemble(depth=depth, feat=feat, bin=np.zeros_like(feat), thr=thr, gain=np.zeros(feat.shape),
                           leaf=leaf, cuts=np.zeros((d, 256), np.float32), nbins=np.full(d, 256, np.int32))


def timed_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    res = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), res


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--trees", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    d, depth = 30, 5
    ens = random_ensemble(d, depth, a.trees, 1)
    X = torch.from_numpy(np.random.default_rng(0).normal(size=(a.rows, d)).astype(np.float32)).to(dev)
    dens = gb.DeviceEnsemble(ens, dev)
    expl = TreePartialDependence(ens, np.zeros(d), np.ones(d), device="cuda:0")
    reps = [torch.from_numpy(R.pd_cells(ens, f)[0]).to(dev) for f in range(d)]
    cells = [int(r.shape[0]) for r in reps]

    def new_sweep():
        return [partial_dependence(X, expl, f, sync=False)[0] for f in range(d)]

    def old_sweep():
        out = []
        for f in range(d):
            Xc = X.clone()
            means = torch.empty(cells[f], dtype=torch.float32, device=dev)
            for c in range(cells[f]):
                Xc[:, f] = reps[f][c]
                means[c] = gb.predict_margin(Xc, ens, dens).mean()
            out.append(means)
        return out

    for _ in range(a.warmup):
        new_sweep()
        old_sweep()
    torch.cuda.synchronize()
    t_new, t_old = [], []
    for _ in range(a.reps):
        ms, q = timed_ms(new_sweep)
        t_new.append(ms)
        ms, m = timed_ms(old_sweep)
        t_old.append(ms)
    err = max(float((qi.double() / R.PD_SCALE / a.rows - mi.double()).abs().max()) for qi, mi in zip(q, m))

    def stats(ts):
        return {"median": round(float(np.median(ts)), 3), "min": round(float(np.min(ts)), 3),
                "max": round(float(np.max(ts)), 3)}

    out = {"config": {"rows": a.rows, "trees": a.trees, "depth": depth, "d": d, "reps": a.reps, "warmup": a.warmup},
           "cells_total": int(sum(cells)), "cells_min": int(min(cells)), "cells_max": int(max(cells)),
           "tree_pd_sweep_ms": stats(t_new), "predict_per_cell_sweep_ms": stats(t_old),
           "speedup": round(float(np.median(t_old) / np.median(t_new)), 2),
           "max_abs_diff_of_the_means": err}
    line = json.dumps(out)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
