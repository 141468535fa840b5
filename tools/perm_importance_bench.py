"""Device timing of permutation importance (csrc/kernels/tree_perm.hip + the metric kernels) against
what a user did before it existed, on the same rows and the same fitted model in one session:

* (a) ``ops.perm_importance.permutation_scores`` end to end: scaler pass, the tree_perm launch(es),
  one ``auc_radix`` per column into one table, one read-back;
* (b) the tree_perm launch(es) of (a) alone;
* (c) the naive loop: per column an index-select of one column into a copy of X,
  ``gb.predict_margin`` and ``ops.metrics.auc_radix``, one read-back at the end (the donor indices are
  computed and uploaded beforehand, outside the timed window);
* (d) the metric kernels of (a) alone, on a filled margin buffer.

The model is a GBDTClassifier fitted on the device on ``data.synthetic.separable`` rows.  Medians of
host-clock times around whole calls that end in a device synchronise, after warm-up calls; (a) and
(c) alternate.  Also checks that (a) and (c) give the same integers.  Prints one JSON line (and
writes it to ``--json``).

    python tools/perm_importance_bench.py [--rows 284807] [--trees 100] [--repeats 5] [--reps 7] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fraud_detection_amd.data.synthetic import separable  # noqa: E402
from fraud_detection_amd.models.explainers import TreePermutationImportance  # noqa: E402
from fraud_detection_amd.models.gbdt import GBDTClassifier  # noqa: E402
from fraud_detection_amd.ops import gbdt as gb  # noqa: E402
from fraud_detection_amd.ops import perm_importance as PI  # noqa: E402
from fraud_detection_amd.ops import reference_gbdt as R  # noqa: E402
from fraud_detection_amd.ops.metrics import auc_radix  # noqa: E402
from fraud_detection_amd.ops.native import native, ptr, stream_of  # noqa: E402
from fraud_detection_amd.ops.scaler import scale_cast  # noqa: E402


def timed_ms(fn):
    t0 = time.perf_counter()
    res = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), res


def summary(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=284_807)
    ap.add_argument("--trees", type=int, default=100)
    ap.add_argument("--depth", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("perm_importance_bench needs a GPU: a CPU timing says nothing about the kernels")
    dev = torch.device("cuda", 0)
    n, d, seed = a.rows, 30, 0
    X, y = separable(n, seed=1, device=dev, n_features=d)
    ens = GBDTClassifier(n_estimators=a.trees, max_depth=a.depth, device="auto").fit(X, y).ensemble
    expl = TreePermutationImportance(ens, np.zeros(d), np.ones(d), device="cuda:0")
    fm = PI.feature_masks(ens)

    def new():
        return PI.permutation_scores(X, y, expl, None, "auc", a.repeats, seed)

    dens = gb.DeviceEnsemble(ens, dev)
    donors = {(f, r): torch.from_numpy(R.permutation_donors(n, seed, f, r)).to(dev)
              for f in range(d) for r in range(a.repeats)}

    def naive():
        out = [auc_radix(gb.predict_margin(X, ens, dens), y)[1]]
        for f in range(d):
            for r in range(a.repeats):
                Xp = X.clone()
                Xp[:, f] = X[:, f].index_select(0, donors[(f, r)])
                out.append(auc_radix(gb.predict_margin(Xp, ens, dens), y)[1])
        return torch.stack(out).cpu().numpy()

    # the launches of (a) taken apart: the same column list, one group
    t = PI._device_ensemble(expl, dev)
    used = fm.any(0)
    cols = [(-1, 0)] + [(f, r) for f in range(d) if used[f] for r in range(a.repeats)]
    Xs = scale_cast(X, t["stats"], out_dtype="f32")
    buf = torch.empty((len(cols), n), dtype=torch.float32, device=dev)
    m = native()
    ws = torch.empty(int(m.auc_radix_workspace_bytes(n)), dtype=torch.uint8, device=dev)
    table = torch.zeros((len(cols), 4), dtype=torch.int64, device=dev)
    fl = torch.empty(len(cols), dtype=torch.float64, device=dev)

    def walks():
        PI._launch(Xs, t, ens, d, cols, seed, buf)

    def metrics():
        s = stream_of(X)
        for j in range(len(cols)):
            m.auc_radix(ptr(buf) + 4 * n * j, ptr(y), n, ptr(ws), ptr(table) + 32 * j, ptr(fl) + 8 * j, s)

    for _ in range(a.warmup):
        new(), naive(), walks(), metrics()
    torch.cuda.synchronize()
    ta, tb, tc, td = [], [], [], []
    for _ in range(a.reps):
        ms, res_a = timed_ms(new)
        ta.append(ms)
        ms, res_c = timed_ms(naive)
        tc.append(ms)
        tb.append(timed_ms(walks)[0])
        td.append(timed_ms(metrics)[0])
    raw, base_raw, P = res_a
    same = bool(base_raw == int(res_c[0, 0]) and np.array_equal(raw.ravel(), res_c[1:, 0]))
    A, B, C, D = summary(ta), summary(tb), summary(tc), summary(td)
    out = {"rows": n, "features": d, "trees": ens.n_trees, "depth": ens.depth, "repeats": a.repeats,
           "columns_launched": len(cols), "tree_feature_masks_nonzero": int((fm[:, :d] != 0).sum()),
           "a_permutation_scores": A, "b_tree_perm": B, "c_naive_loop": C, "d_metric_kernels": D,
           "ratio_c_over_a": C["median_ms"] / A["median_ms"], "metric_share_of_a": D["median_ms"] / A["median_ms"],
           "same_integers_as_naive": same, "baseline_auc": base_raw / (2.0 * P * (n - P)),
           "timed_reps": a.reps, "warmup": a.warmup}
    print(json.dumps(out))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)
    if not same:
        raise SystemExit("the naive loop and permutation_scores disagree")


if __name__ == "__main__":
    main()
