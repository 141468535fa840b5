"""Exact precision-recall curve, average precision and operating points on the CPU oracle path
(ops/reference.pr_curve / average_precision_q, ops/metrics, the GBDT's eval_metric="aucpr")."""
import numpy as np
import pytest
import torch

from fraud_detection_amd.ops import gbdt as gb
from fraud_detection_amd.ops import metrics as M
from fraud_detection_amd.ops import reference as ref
from fraud_detection_amd.ops import reference_gbdt as R

Q = 2 ** 30
AP_BOUND = 2.0 ** -31 + 1e-12  # half a unit of the 2^-30 fixed point per positive / P, + sklearn's fp64 sum


def make(n, rate, ties, seed):
    g = np.random.default_rng(seed)
    y = (g.random(n) < rate).astype(np.uint8)
    y[0], y[-1] = 1, 0  # both classes present (sklearn needs a positive)
    s = (g.standard_normal(n) + 1.5 * y).astype(np.float32)
    if ties:
        s = (np.round(s * 4) / 4).astype(np.float32)
    return s, y


# ---- the oracle against sklearn ----------------------------------------------------------------
@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("rate", [0.5, 0.05, 0.002])
@pytest.mark.parametrize("n", [2, 3, 257, 65537])
def test_oracle_matches_sklearn(n, rate, ties):
    from sklearn.metrics import average_precision_score, precision_recall_curve

    s, y = make(n, rate, ties, seed=n + int(rate * 1000) + ties)
    thr, tp, fp = ref.pr_curve(s, y)
    assert thr.dtype == np.float32 and tp.dtype == np.int64 and fp.dtype == np.int64
    prec, rec = M.precision_recall(thr, tp, fp)
    sp, sr, st = precision_recall_curve(y, s)
    # sklearn: ascending thresholds, and one appended (precision 1, recall 0) point
    assert np.array_equal(thr, st[::-1].astype(np.float32))
    assert np.max(np.abs(prec - sp[:-1][::-1])) <= 1e-15
    assert np.max(np.abs(rec - sr[:-1][::-1])) <= 1e-15
    q, P, N = ref.average_precision_q(s, y)
    assert (P, N) == (int(y.sum()), int(n - y.sum()))
    assert abs(q / Q / P - average_precision_score(y, s)) <= AP_BOUND
    assert ref.average_precision(s, y) == q / Q / P
    assert M.average_precision(torch.from_numpy(s), torch.from_numpy(y)) == q / Q / P
    got = M.pr_curve(torch.from_numpy(s), torch.from_numpy(y))
    assert all(np.array_equal(a, b) for a, b in zip(got, (thr, tp, fp)))


def test_formula_is_the_sum_over_tie_groups():
    s = np.array([3, 3, 2, 2, 2, 1, 0, 0], np.float32)
    y = np.array([1, 0, 1, 1, 0, 0, 1, 0], np.uint8)
    thr, tp, fp = ref.pr_curve(s, y)
    assert thr.tolist() == [3, 2, 1, 0] and tp.tolist() == [1, 3, 3, 4] and fp.tolist() == [1, 2, 3, 4]
    want = sum(int(np.rint(d * (t / (t + f)) * Q)) for d, t, f in ((1, 1, 1), (2, 3, 2), (0, 3, 3), (1, 4, 4)))
    assert ref.average_precision_q(s, y) == (want, 4, 4)
    p = np.random.default_rng(0).permutation(8)  # order independent
    assert ref.average_precision_q(s[p], y[p]) == (want, 4, 4)


def test_degenerate_inputs():
    g = np.random.default_rng(1)
    s = g.standard_normal(1000).astype(np.float32)
    zeros, ones = np.zeros(1000, np.uint8), np.ones(1000, np.uint8)
    assert ref.average_precision_q(s, zeros) == (0, 0, 1000)
    assert np.isnan(ref.average_precision(s, zeros))
    assert np.isnan(M.average_precision(torch.from_numpy(s), torch.from_numpy(zeros)))
    assert ref.average_precision_q(s, ones) == (1000 * Q, 1000, 0)
    assert ref.average_precision(s, ones) == 1.0
    # one tie group: AP = P / n
    y = (g.random(1000) < 0.3).astype(np.uint8)
    flat = np.full(1000, 0.25, np.float32)
    thr, tp, fp = ref.pr_curve(flat, y)
    assert thr.tolist() == [0.25] and tp.tolist() == [int(y.sum())] and fp.tolist() == [1000 - int(y.sum())]
    assert abs(ref.average_precision(flat, y) - y.sum() / 1000) <= 2.0 ** -31
    # empty
    e = ref.pr_curve(np.zeros(0, np.float32), np.zeros(0, np.uint8))
    assert all(a.shape == (0,) for a in e)
    assert ref.average_precision_q(np.zeros(0, np.float32), np.zeros(0, np.uint8)) == (0, 0, 0)
    assert M.precision_recall(*e)[0].shape == (0,)


def test_infinities_and_signed_zero():
    inf = np.float32(np.inf)
    s = np.array([inf, -inf, 0.0, -0.0, 1.0, inf, -inf, -0.0], np.float32)
    y = np.array([1, 0, 1, 0, 0, 0, 1, 1], np.uint8)
    thr, tp, fp = ref.pr_curve(s, y)
    assert thr.tolist() == [inf, 1.0, 0.0, -inf]
    assert not np.signbit(thr[2])  # the -0 / +0 class is one group, reported as +0.0
    assert tp.tolist() == [1, 1, 3, 4] and fp.tolist() == [1, 2, 3, 4]
    for g in range(4):  # the counts are those of score >= thr
        assert tp[g] == int(((s >= thr[g]) & (y != 0)).sum()) and fp[g] == int(((s >= thr[g]) & (y == 0)).sum())
    want = int(np.rint(0.5 * Q)) + int(np.rint(2 * (3 / 6) * Q)) + int(np.rint(1 * (4 / 8) * Q))
    assert ref.average_precision_q(s, y) == (want, 4, 4)
    k = ref.order_key(s)
    assert k[2] == k[3] and np.array_equal(ref.order_key_inv(k)[[0, 1, 4]], s[[0, 1, 4]])


# ---- operating points --------------------------------------------------------------------------
@pytest.mark.parametrize("ties", [False, True])
def test_operating_point_against_brute_force(ties):
    s, y = make(4001, 0.05, ties, seed=7)
    thr, tp, fp = ref.pr_curve(s, y)
    pos = y != 0
    P = int(pos.sum())
    # brute force over the distinct thresholds, with direct counts of score >= threshold
    cand = []
    for t in np.unique(s):
        a = s >= t
        cand.append((float(t), int((a & pos).sum()), int((a & ~pos).sum())))

    def check(op, want):
        assert (op["threshold"], op["tp"], op["fp"]) == want
        a = s >= np.float32(op["threshold"])
        assert op["tp"] == int((a & pos).sum()) and op["fp"] == int((a & ~pos).sum())
        assert op["alerts"] == op["tp"] + op["fp"]
        assert op["precision"] == op["tp"] / op["alerts"] and op["recall"] == op["tp"] / P

    reached = 0
    for target in (0.06, 0.2, 0.35, 0.5, 0.9):
        ok = [c for c in cand if c[1] / (c[1] + c[2]) >= target]
        if ok:
            check(M.operating_point(thr, tp, fp, min_precision=target), min(ok))  # the lowest threshold
            reached += 1
        else:  # the brute force finds no threshold either
            with pytest.raises(ValueError, match="no threshold"):
                M.operating_point(thr, tp, fp, min_precision=target)
    assert reached >= 2
    for target in (0.1, 0.5, 1.0):
        ok = [c for c in cand if c[1] / P >= target]
        check(M.operating_point(thr, tp, fp, min_recall=target), max(ok))     # the highest threshold
    for budget in (1 if not ties else int(tp[0] + fp[0]), 100, 4001):
        ok = [c for c in cand if c[1] + c[2] <= budget]
        check(M.operating_point(thr, tp, fp, max_alerts=budget), min(ok))


def test_operating_point_errors():
    s, y = make(500, 0.1, True, seed=8)
    c = ref.pr_curve(s, y)
    with pytest.raises(ValueError, match="exactly one"):
        M.operating_point(*c)
    with pytest.raises(ValueError, match="exactly one"):
        M.operating_point(*c, min_precision=0.5, max_alerts=10)
    with pytest.raises(ValueError, match="no threshold"):
        M.operating_point(*c, min_precision=1.5)
    with pytest.raises(ValueError, match="no threshold"):
        M.operating_point(*c, min_recall=1.5)
    with pytest.raises(ValueError, match="no threshold"):
        M.operating_point(*c, max_alerts=0)


# ---- the histogram form ------------------------------------------------------------------------
def test_hist_curve_equals_exact_curve_on_separated_values():
    g = np.random.default_rng(9)
    # 256 distinct values k / 4 - 20 (k / 4 and 20 need <= 7 mantissa bits between them: one 16-bit bin each)
    vals = (np.arange(256, dtype=np.float32) / 4 - 20).astype(np.float32)
    assert len(np.unique(ref.order_key(vals) >> 16)) == 256
    s = vals[g.integers(0, 256, 20_000)]
    y = (g.random(20_000) < 0.1 + 0.3 * (s > 10)).astype(np.uint8)
    st, yt = torch.from_numpy(s), torch.from_numpy(y)
    thr, tp, fp = ref.pr_curve(s, y)
    ht, htp, hfp = M.pr_curve_hist(st, yt, bits=16)
    assert np.array_equal(htp, tp) and np.array_equal(hfp, fp)
    assert htp.dtype == np.int64 and ht.dtype == np.float32
    assert np.array_equal(ht[thr >= 0], thr[thr >= 0])   # a bin's lower edge: the score itself where s >= 0
    assert np.all(ht <= thr) and np.all(ht[:-1] > thr[1:])  # and below it, above the next group, elsewhere
    assert M.average_precision_hist(st, yt, bits=16) == ref.average_precision(s, y)
    z = torch.zeros(20_000, dtype=torch.uint8)
    assert np.isnan(M.average_precision_hist(st, z))
    neg = torch.tensor([-np.inf, 1.0], dtype=torch.float32)
    assert M.pr_curve_hist(neg, torch.tensor([0, 1], dtype=torch.uint8))[0].tolist() == [1.0, -np.inf]


# ---- the evaluation script ---------------------------------------------------------------------
def test_evaluate_model_script_reports_precision_recall(tmp_path):
    import os
    import re
    import shutil
    import subprocess
    import sys

    from sklearn.metrics import average_precision_score

    from fraud_detection_amd.compat.sklearn_export import load_artifacts

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    shutil.copytree(os.path.join(root, "models"), tmp_path / "models")
    os.makedirs(tmp_path / "data")
    g = np.random.default_rng(0)
    X = g.normal(0, 1, (3000, 30)).astype(np.float32)
    y = (X @ g.normal(0, 1, 30) + g.normal(0, 1, 3000) > 2.5).astype(np.int64)
    np.savez_compressed(tmp_path / "data" / "preprocessed_data.npz", X_res=X, y_res=y, X_test=X, y_test=y)
    env = dict(os.environ, PYTHONPATH=root, MPLBACKEND="Agg", FDX_DEVICE="cpu")
    r = subprocess.run([sys.executable, os.path.join(root, "evaluate_model.py")], cwd=tmp_path, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert (tmp_path / "plots" / "pr_curve.png").exists() and (tmp_path / "plots" / "roc_curve.png").exists()
    ap = float(re.search(r"Average precision: ([0-9.]+)", r.stdout).group(1))
    art = load_artifacts(str(tmp_path / "models" / "logistic_model.joblib"), str(tmp_path / "models" / "scaler.joblib"),
                         str(tmp_path / "models" / "feature_names.json"))
    z = X.astype(np.float64) @ np.asarray(art.coef, np.float64) + float(art.intercept)
    assert abs(ap - average_precision_score(y, z)) < 2e-4  # four printed decimals; fp32 scores against fp64
    m = re.search(r"Operating point at p > 0.8: precision ([0-9.a-z]+), recall ([0-9.]+), alerts (\d+)", r.stdout)
    alerts = z > np.log(4.0)
    assert abs(int(m.group(3)) - int(alerts.sum())) <= 2  # scores within fp32 rounding of the level may flip
    assert abs(float(m.group(2)) - (alerts & (y != 0)).sum() / (y != 0).sum()) < 0.02
    assert "Confusion Matrix" in r.stdout and "AUC" in r.stdout  # nothing that existed is gone


# ---- the GBDT's aucpr --------------------------------------------------------------------------
def noisy(n, seed, d=8, noise=1.5):
    g = np.random.default_rng(seed)
    X = g.standard_normal((n, d)).astype(np.float32)
    s = X[:, 0] + 0.5 * X[:, 1] * X[:, 2] + noise * g.standard_normal(n)
    return torch.from_numpy(X), torch.from_numpy((s > 0.8).astype(np.uint8))


@pytest.fixture(scope="module")
def overfit():
    X, y = noisy(1500, 31)
    Xv, yv = noisy(900, 32)
    p = gb.GBDTParams(n_estimators=40, max_depth=5, learning_rate=0.5)
    cuts = gb.quantile_cuts(X, p.max_bin)
    ens, rec = gb.fit(X, y, p, cuts=cuts, eval_set=(Xv, yv), eval_metric=("logloss", "aucpr"))
    return dict(X=X, y=y, Xv=Xv, yv=yv, p=p, cuts=cuts, ens=ens, rec=rec)


def test_gbdt_aucpr_history_equals_the_oracle(overfit):
    from sklearn.metrics import average_precision_score

    o = overfit
    ens, rec = o["ens"], o["rec"]
    bv = R.bin_rows(o["Xv"].numpy(), *o["cuts"])
    yv = o["yv"].numpy()
    P = int(yv.sum())
    assert rec.n_rounds == 40 and rec.metrics == ("logloss", "aucpr") and rec.twice_pairs is None
    for t in range(40):
        m = R.predict_margin_bins(bv, ens.feat[:t + 1], ens.bin[:t + 1], ens.leaf[:t + 1], ens.depth, ens.base_margin)
        assert rec.ap_q[t] == R.ap_q(m, yv)
        assert rec.history["aucpr"][t] == rec.ap_q[t] / Q / P
    assert abs(rec.history["aucpr"][39] - average_precision_score(yv, m)) <= AP_BOUND
    assert rec.best_iteration == int(np.argmax(rec.ap_q)) and rec.best_score == rec.history["aucpr"][rec.best_iteration]
    assert ens.n_trees == 40
    plain = gb.fit(o["X"], o["y"], o["p"], cuts=o["cuts"])
    assert all(np.array_equal(getattr(ens, f), getattr(plain, f)) for f in ("feat", "bin", "thr", "gain", "leaf"))


def test_gbdt_early_stopping_on_aucpr(overfit):
    o = overfit
    best, stop = gb.stop_round([-int(v) for v in o["rec"].ap_q], 3)
    assert stop is not None and stop < 39  # the setup overfits: the rule fires
    ens, rec = gb.fit(o["X"], o["y"], o["p"], cuts=o["cuts"], eval_set=(o["Xv"], o["yv"]),
                      eval_metric=("logloss", "aucpr"), early_stopping_rounds=3)
    assert rec.stopped and (rec.best_iteration, rec.n_rounds, ens.n_trees) == (best, stop + 1, best + 1)
    assert np.array_equal(rec.ap_q, o["rec"].ap_q[:stop + 1])
    assert all(np.array_equal(getattr(ens, f), getattr(o["ens"], f)[:best + 1]) for f in ("feat", "leaf"))


def test_gbdt_aucpr_without_positives_is_nan(overfit):
    o = overfit
    _, rec = gb.fit(o["X"], o["y"], gb.GBDTParams(n_estimators=2, max_depth=2), cuts=o["cuts"],
                    eval_set=(o["Xv"], torch.zeros_like(o["yv"])), eval_metric="aucpr")
    assert rec.ap_q.tolist() == [0, 0] and all(np.isnan(v) for v in rec.history["aucpr"])


class _TwoRanks:
    world_size, rank = 2, 0


def test_gbdt_aucpr_is_refused_under_data_parallel(overfit):
    o = overfit
    with pytest.raises(NotImplementedError, match="aucpr"):
        gb.fit(o["X"], o["y"], o["p"], cuts=o["cuts"], comm=_TwoRanks(), eval_set=(o["Xv"], o["yv"]),
               eval_metric=("logloss", "aucpr"))
