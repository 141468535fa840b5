#!/usr/bin/env python3
"""GBDT (K11) throughput on one GPU: xgboost-config boosting (100 trees, depth 5, eta 0.1) on
credit_card-shaped synthetic rows after SMOTE, plus test AUC and inference rate.

    python tools/gbdt_bench.py [--rows 10000000] [--trees 100] [--json out.json]
                               [--subsample 0.8] [--colsample-bytree 0.5] [--seed 0] [--weights]
                               [--monotone "1:-1,2:1,3:-1,4:1,29:1"]
                               [--interaction "0,29;1,2,3,4,5;6,7,8"]
                               [--gbdt-reg-alpha 1.0] [--gbdt-max-delta-step 1.0]

--weights: every table row of the boosting call gets a sample weight (a time decay from 0.25 for the
first row to 1.0 for the last, SMOTE's rows included), to measure what the weighted kernels cost on
the same rows.  The pipeline itself takes no weights: the tool hands them to its ops/gbdt.fit call.
--monotone: feature index : sign pairs (GBDTParams.monotone_constraints as a dict), to measure what
the constrained split scan costs against the same fit without it.
--interaction: groups of feature indices, ';' between groups and ',' between indices
(GBDTParams.interaction_constraints), to measure what carrying the path words and filtering the
eligible features costs against the same fit without it.
--gbdt-reg-alpha / --gbdt-max-delta-step: GBDTParams.reg_alpha / max_delta_step, to measure what the
regularised weight / term form of the split scan costs against the same fit without it.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2_000_000)
    ap.add_argument("--trees", type=int, default=100)
    ap.add_argument("--depth", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--subsample", type=float, default=1.0)
    ap.add_argument("--colsample-bytree", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--weights", action="store_true")
    ap.add_argument("--monotone", default=None)
    ap.add_argument("--interaction", default=None)
    ap.add_argument("--gbdt-reg-alpha", type=float, default=0.0)
    ap.add_argument("--gbdt-max-delta-step", type=float, default=0.0)
    a = ap.parse_args()
    from fraud_detection_amd.data.synthetic import separable
    from fraud_detection_amd.models.gbdt import GBDTPipeline
    from fraud_detection_amd.models.pipeline import TrainConfig
    from fraud_detection_amd.ops import gbdt as gb

    dev = torch.device("cuda", 0)
    if a.weights:
        fit = gb.fit

        def weighted_fit(rows, labels, params, **kw):
            w = torch.linspace(0.25, 1.0, rows.shape[0], dtype=torch.float32, device=rows.device)
            return fit(rows, labels, params, sample_weight=w, **kw)

        gb.fit = weighted_fit  # models/gbdt.py calls gb.fit: the pipeline's rows, plus a weight each
    n_test = a.rows // 5
    X, y = separable(a.rows - n_test, seed=1000, device=dev)
    Xt, yt = separable(n_test, seed=5000, device=dev)
    sampling = dict(subsample=a.subsample, colsample_bytree=a.colsample_bytree, seed=a.seed)
    mono = {int(k): int(v) for k, v in (item.split(":") for item in a.monotone.split(","))} if a.monotone else None
    if mono:
        sampling["monotone_constraints"] = mono
    inter = [[int(f) for f in g.split(",")] for g in a.interaction.split(";")] if a.interaction else None
    if inter:
        sampling["interaction_constraints"] = inter
    if a.gbdt_reg_alpha or a.gbdt_max_delta_step:
        sampling.update(reg_alpha=a.gbdt_reg_alpha, max_delta_step=a.gbdt_max_delta_step)
    pipe = GBDTPipeline(TrainConfig(), gb.GBDTParams(n_estimators=a.trees, max_depth=a.depth, **sampling))
    GBDTPipeline(TrainConfig(), gb.GBDTParams(n_estimators=2, max_depth=a.depth, **sampling)).fit(X, y)  # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = pipe.fit(X, y)
    torch.cuda.synchronize()
    fit_s = time.perf_counter() - t0
    ev = res.evaluate(Xt, yt)
    Xs = res.standardize(Xt)
    res.predict_margin(Xt)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    for _ in range(5):
        gb.predict_margin(Xs, res.ensemble, res._dens)
    torch.cuda.synchronize()
    pred_s = (time.perf_counter() - t1) / 5
    out = {"rows_train_post_smote": res.n_train_rows, "trees": a.trees, "depth": a.depth,
           "fit_s": round(fit_s, 4), "prep_s": round(res.timings["prep"], 4), "boost_s": round(res.timings["boost"], 4),
           "ms_per_tree": round(1000 * res.timings["boost"] / max(a.trees, 1), 3),
           "row_trees_per_s": round(res.n_train_rows * a.trees / res.timings["boost"], 1),
           "auc": round(ev["auc"], 6), "predict_rows_per_s": round(n_test / pred_s, 1),
           "scale_pos_weight": round(res.scale_pos_weight, 3)}
    if pipe.params.sampled:
        out.update({k: v for k, v in sampling.items()
                    if k not in ("monotone_constraints", "interaction_constraints", "reg_alpha", "max_delta_step")})
    if pipe.params.reg is not None:
        out.update(reg_alpha=a.gbdt_reg_alpha, max_delta_step=a.gbdt_max_delta_step)
    if mono:
        out["monotone"] = a.monotone
    if inter:
        out["interaction"] = a.interaction
    if a.weights:
        out["weights"] = "linspace(0.25, 1.0)"
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f)


if __name__ == "__main__":
    main()
