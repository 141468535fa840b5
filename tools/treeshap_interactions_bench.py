"""Device timings of the SHAP interaction kernel (csrc/kernels/treeshap_interact.hip) next to the
path-dependent TreeSHAP kernel on the same rows, in one session:

* 1000 explanations x 100 trees x depth 5 x d = 30, random trees;
* the same shape with every split feature drawn from 4 of the 30 columns -- the contention case: a
  fitted model that concentrates on a few features sends all threads to the same few cells.

Each model is timed as the launcher runs it (``config.trees_in_lds`` says where the per-tree
constants sit) and with the constants streamed from L2 (``stream_trees``; identical results).
Medians of HIP-event times over ``--reps`` launches after a warm-up long enough for the clock to
ramp.  Prints one JSON line (and writes it to ``--json``).

    python tools/treeshap_interactions_bench.py [--reps 50] [--json out.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fraud_detection_amd.models.explainers import TreePathExplainer  # noqa: E402
from fraud_detection_amd.ops import gbdt as gb  # noqa: E402
from fraud_detection_amd.ops.treeshap import (treeshap_interactions, treeshap_interactions_lds_resident,  # noqa: E402
                                              treeshap_path)


def random_ensemble(d, depth, T, seed, columns=None):
    """Random full trees; ``columns``: the features the splits are drawn from (None = all d)."""
    rng = np.random.default_rng(seed)
    ni = (1 << depth) - 1
    cols = np.arange(d) if columns is None else np.asarray(columns)
    feat = cols[rng.integers(0, len(cols), (T, ni))].astype(np.int32)
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
    return {"median": round(float(np.median(ts)), 4), "min": round(float(np.min(ts)), 4),
            "max": round(float(np.max(ts)), 4)}


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--explanations", type=int, default=1000)
    ap.add_argument("--trees", type=int, default=100)
    ap.add_argument("--cover-rows", type=int, default=100_000)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    d, depth = 30, 5
    rng = np.random.default_rng(0)
    rows = torch.from_numpy(rng.normal(size=(a.cover_rows, d)).astype(np.float32)).to(dev)
    X = rng.normal(size=(a.explanations, d)).astype(np.float32)
    Xd = torch.from_numpy(X).to(dev)
    out = {"config": {"explanations": a.explanations, "trees": a.trees, "depth": depth, "d": d,
                      "cover_rows": a.cover_rows, "reps": a.reps, "warmup": a.warmup,
                      "trees_in_lds": treeshap_interactions_lds_resident(d, a.trees, depth)}}
    for name, cols in (("random", None), ("four_columns", [3, 11, 17, 26])):
        ens = random_ensemble(d, depth, a.trees, 1, cols)
        ens = ens.with_cover(gb.node_cover(rows, ens, "hessian").cpu().numpy(), "hessian")
        te = TreePathExplainer(ens, np.zeros(d), np.ones(d), device="cuda:0")
        res = {"treeshap_path_ms": median_ms(lambda: treeshap_path(Xd, te, sync=False), a.reps, a.warmup)}
        ref = treeshap_interactions(Xd, te)
        got = treeshap_interactions(Xd, te, stream_trees=True)
        res["streamed_equal_bits"] = bool(np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]))
        res["interactions_ms"] = median_ms(lambda: treeshap_interactions(Xd, te, sync=False), a.reps, a.warmup)
        res["interactions_streamed_ms"] = median_ms(
            lambda: treeshap_interactions(Xd, te, sync=False, stream_trees=True), a.reps, a.warmup)
        res["ratio_to_path"] = round(res["interactions_ms"]["median"] / res["treeshap_path_ms"]["median"], 2)
        out[name] = res
    line = json.dumps(out)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
