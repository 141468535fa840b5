"""Device timings of the path-dependent TreeSHAP kernel and the node-cover kernel, in one session:

* 1000 explanations x 100 trees x depth 5 x d = 30 with ``treeshap_path`` next to the
  interventional ``treeshap`` kernel at 100 background rows on the same rows;
* ``tree_cover`` on 1M rows, both kinds.

Medians of HIP-event times over ``--reps`` launches after a warm-up long enough for the clock to
ramp.  Prints one JSON line (and writes it to ``--json``).

    python tools/treeshap_path_bench.py [--reps 50] [--json out.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fraud_detection_amd.models.explainers import TreeExplainer, TreePathExplainer  # noqa: E402
from fraud_detection_amd.ops import gbdt as gb  # noqa: E402
from fraud_detection_amd.ops.treeshap import treeshap, treeshap_path  # noqa: E402


def random_ensemble(d, depth, T, seed):
    rng = np.random.default_rng(seed)
    ni = (1 << depth) - 1
    feat = rng.integers(0, d, (T, ni)).astype(np.int32)
    thr = rng.normal(0, 0.7, (T, ni)).astype(np.float32)
    leaf = rng.normal(0, 0.1, (T, 1 << depth)).astype(np.float32)
    return gb.TreeEnsemble(depth=depth, feat=feat, bin=np.zeros_like(feat), thr=thr, gain=np.zeros(feat.shape),
                           leaf=leaf, cuts=np.zeros((d, 256), np.float32), nbins=np.full(d, 256, np.int32))


def median_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--explanations", type=int, default=1000)
    ap.add_argument("--trees", type=int, default=100)
    ap.add_argument("--cover-rows", type=int, default=1_000_000)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    d, depth = 30, 5
    rng = np.random.default_rng(0)
    ens = random_ensemble(d, depth, a.trees, 1)
    rows = torch.from_numpy(rng.normal(size=(a.cover_rows, d)).astype(np.float32)).to(dev)
    dens = gb.DeviceEnsemble(ens, dev)
    out = {"config": {"explanations": a.explanations, "trees": a.trees, "depth": depth, "d": d,
                      "background": 100, "cover_rows": a.cover_rows, "reps": a.reps}}
    for kind in ("count", "hessian"):
        med, lo, hi = median_ms(lambda: gb.node_cover(rows, ens, kind, dens), max(5, a.reps // 5), 3)
        out[f"tree_cover_{kind}_ms"] = {"median": round(med, 4), "min": round(lo, 4), "max": round(hi, 4)}
    # same rows at both ends of the wave: the fraud-like case where a wave agrees on its leaves
    same = rows[:1].expand(a.cover_rows, d).contiguous()
    med, lo, hi = median_ms(lambda: gb.node_cover(same, ens, "hessian", dens), max(5, a.reps // 5), 3)
    out["tree_cover_hessian_identical_rows_ms"] = {"median": round(med, 4), "min": round(lo, 4), "max": round(hi, 4)}
    ens = ens.with_cover(gb.node_cover(rows, ens, "hessian", dens).cpu().numpy(), "hessian")
    X = rng.normal(size=(a.explanations, d)).astype(np.float32)
    B = rng.normal(size=(100, d)).astype(np.float32)
    Xd = torch.from_numpy(X).to(dev)
    tp = TreePathExplainer(ens, np.zeros(d), np.ones(d), device="cuda:0")
    ti = TreeExplainer(ens, np.zeros(d), np.ones(d), B, device="cuda:0")
    for name, fn in (("treeshap_path_ms", lambda: treeshap_path(Xd, tp, sync=False)),
                     ("treeshap_interventional_ms", lambda: treeshap(Xd, ti, sync=False))):
        med, lo, hi = median_ms(fn, a.reps, 200)
        out[name] = {"median": round(med, 4), "min": round(lo, 4), "max": round(hi, 4)}
    line = json.dumps(out)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
