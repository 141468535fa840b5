#!/usr/bin/env python3
"""What per-round evaluation costs a GBDT fit: ms per tree of ops/gbdt.fit_binned on a hole-shaped
table (a CV fold: the table minus one fifth) at the bench's GBDT row count, hipEvent medians over
repeated fits after a warm-up, for

  off   -- no evaluation (the path every fit took before evaluation existed);
  hole  -- eval_set="hole", eval_metric="logloss": one gbdt_eval launch per round over the hole.

Run it once per tree to compare: ``--package-root`` points at the checkout whose package is
imported (a checkout without evaluation runs ``off`` only), ``--label`` names the row.

    python tools/gbdt_eval_overhead.py [--rows 8000000] [--trees 100] [--repeats 7] [--label this]
        [--package-root DIR] [--cv | --cv-only] [--cv-lr 0.1] [--cv-patience 10] [--json out.json]

``--cv`` adds the DeviceGBDTCV job unstopped, with logloss curves, and with early stopping on
logloss, on error and on auc.
"""
from __future__ import annotations

import argparse
import inspect
import json
import os
import statistics
import sys

import torch


def timed(fn, repeats: int):
    """Device ms of fn(): hipEvents around each call, after one warm-up call."""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def stats(ms, per: int = 1) -> dict:
    v = sorted(x / per for x in ms)
    return {"median": round(statistics.median(v), 4), "min": round(v[0], 4), "max": round(v[-1], 4), "n": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=8_000_000, help="table rows (bench: 10M raw rows, 80%% train)")
    ap.add_argument("--trees", type=int, default=100)
    ap.add_argument("--depth", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--label", default="this")
    ap.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--cv", action="store_true")
    ap.add_argument("--cv-only", action="store_true", help="skip the fit_binned timings")
    ap.add_argument("--cv-rows", type=int, default=1_000_000)
    ap.add_argument("--cv-lr", type=float, default=0.1, help="learning rate of the CV job's fits (bench: 0.1)")
    ap.add_argument("--cv-patience", type=int, default=10)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.package_root))
    from fraud_detection_amd.data.synthetic import separable
    from fraud_detection_amd.ops import gbdt as gb

    dev = torch.device("cuda", 0)
    has_eval = "eval_set" in inspect.signature(gb.fit_binned).parameters
    out = {"label": a.label, "trees": a.trees, "depth": a.depth}
    if not a.cv_only:
        out.update(fit_timings(a, gb, separable, dev, has_eval))
    if (a.cv or a.cv_only) and has_eval:
        out["gbdt_cv"] = cv_timings(a, gb, separable, dev)
    line = json.dumps(out)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")
    return 0


def fit_timings(a, gb, separable, dev, has_eval) -> dict:
    n = a.rows
    X, y = separable(n, seed=1000, device=dev)
    pos = int(y.sum())
    p = gb.GBDTParams(n_estimators=a.trees, max_depth=a.depth, learning_rate=0.1,
                      scale_pos_weight=(n - pos) / max(pos, 1))
    cuts = gb.quantile_cuts(X, p.max_bin, p.cut_sample_rows)
    bins = gb.bin_rows(X, cuts[0], cuts[1])
    del X
    hole = (2 * (n // 5), n // 5)
    out = {"rows": n, "hole": list(hole), "ms_per_tree": {}}
    out["ms_per_tree"]["off"] = stats(timed(lambda: gb.fit_binned(bins, y, cuts, p, hole=hole, return_margin=True),
                                            a.repeats), a.trees)
    if has_eval:
        out["ms_per_tree"]["hole"] = stats(timed(lambda: gb.fit_binned(
            bins, y, cuts, p, hole=hole, return_margin=True, eval_set="hole", eval_metric="logloss"), a.repeats), a.trees)
    return out


def cv_timings(a, gb, separable, dev) -> dict:
    from fraud_detection_amd.models.gbdt_cv import DeviceGBDTCV
    from fraud_detection_amd.models.pipeline import TrainConfig

    Xc, yc = separable(a.cv_rows, seed=1000, device=dev)
    pc = gb.GBDTParams(n_estimators=a.trees, max_depth=a.depth, learning_rate=a.cv_lr)
    stop = {"early_stopping_rounds": a.cv_patience}
    cv = {"rows": a.cv_rows, "learning_rate": a.cv_lr, "patience": a.cv_patience}
    for name, kw in (("plain", {}), ("logloss", {"eval_metric": "logloss"}),
                     ("early_stopping_logloss", {"eval_metric": "logloss", **stop}),
                     ("early_stopping_error", {"eval_metric": ("logloss", "error"), **stop}),
                     ("early_stopping_auc", {"eval_metric": ("logloss", "auc"), **stop})):
        DeviceGBDTCV(TrainConfig(), pc, **kw).run(Xc, yc)  # warm-up
        runs = [DeviceGBDTCV(TrainConfig(), pc, **kw).run(Xc, yc) for _ in range(3)]
        r = runs[-1]
        cv[name] = {"total_ms": stats([q.total_ms for q in runs]), "cv_auc_mean": round(r.cv_auc_mean, 6),
                    "fold_best_iteration": list(r.fold_best_iteration), "final_n_estimators": r.final_n_estimators}
    return cv


if __name__ == "__main__":
    raise SystemExit(main())
