"""Permutation importance on the CPU: the donor permutation, the oracle margins against the
partial-dependence oracle, the scorers' integers and the estimator's interface."""
from __future__ import annotations

import pickle

import numpy as np
import pytest
import torch

import _pd_cases as PC
import _perm_cases as QC
import _tree_cases as TC
from fraud_detection_amd.models.explainers import PermutationImportance, TreePermutationImportance
from fraud_detection_amd.ops import reference_gbdt as R
from fraud_detection_amd.ops.perm_importance import feature_masks, permutation_scores, permuted_margins
from fraud_detection_amd.ops.pdp import override_words


def _expl(ens):
    d = ens.n_features
    return TreePermutationImportance(ens, np.zeros(d), np.ones(d), device="cpu")


# ---- donors ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 63, 64, 65, 1000, 65537])
def test_donors_are_a_bijection(n):
    p = R.permutation_donors(n, 7, 3, 2)
    assert p.dtype == np.int64 and p.shape == (n,)
    assert np.array_equal(np.sort(p), np.arange(n))


def test_donors_differ_between_features_repeats_and_seeds():
    base = R.permutation_donors(1000, 5, 2, 1)
    assert not np.array_equal(base, np.arange(1000))
    for other in (R.permutation_donors(1000, 5, 3, 1), R.permutation_donors(1000, 5, 2, 0),
                  R.permutation_donors(1000, 6, 2, 1)):
        assert not np.array_equal(base, other)
    assert np.array_equal(base, R.permutation_donors(1000, 5, 2, 1))


def test_a_repeat_does_not_depend_on_the_repeat_count_or_the_feature_list():
    ens, Xs = PC.random_case(d=4, depth=3, T=5, n=50, seed=3)
    two, _ = R.permuted_margins_reference(Xs, ens, (0, 2), 2, 9)
    seven, _ = R.permuted_margins_reference(Xs, ens, (2,), 7, 9)
    assert PC.bits_equal(two[1, 1], seven[0, 1])


@pytest.mark.parametrize("n,seed,f,r", [(11, 0, 0, 0), (37, 123456789, 29, 4), (64, 2 ** 32 - 1, 5, 70), (1, 1, 1, 1)])
def test_donors_match_the_written_out_rounds(n, seed, f, r):
    assert R.permutation_donors(n, seed, f, r).tolist() == QC.loop_donors(n, seed, f, r)


def test_donor_arguments_are_checked():
    for bad in ((5, -1, 0, 0), (5, 2 ** 32, 0, 0), (5, 0, 32, 0), (5, 0, -1, 0), (5, 0, 0, -1), (-1, 0, 0, 0)):
        with pytest.raises(ValueError):
            R.permutation_donors(*bad)


# ---- margins ---------------------------------------------------------------------------------------
def _hand_rows():
    rng = np.random.default_rng(4)
    Xs = rng.normal(0, 1.5, (90, 4)).astype(np.float32)
    Xs[rng.random(Xs.shape) < 0.15] = np.nan
    Xs[:6, 0] = [0.5, -0.5, 1.5, 0.5, -0.5, 1.5]          # values on the thresholds
    return Xs


@pytest.mark.parametrize("case", ["hand", "random"])
def test_permuted_margin_is_the_ice_value_at_the_donors_cell(case):
    if case == "hand":
        ens, Xs = PC.hand_ensemble(), _hand_rows()
    else:
        ens, Xs = PC.random_case(d=5, depth=4, T=9, n=120, seed=5, learn=True, nan_rows=True)
    assert ens.has_default_left and np.isnan(Xs).any()
    n, d = Xs.shape
    pm, base = R.permuted_margins_reference(Xs, ens, None, 3, 17)
    assert pm.shape == (d, 3, n) and PC.bits_equal(base, PC.margin(Xs, ens))
    assert PC.bits_equal(pm, QC.explicit_margins(Xs, ens, range(d), 3, 17))
    for f in range(d):
        ice = PC.loop_ice(Xs, ens, f)
        for r in range(3):
            donor = R.permutation_donors(n, 17, f, r)
            assert PC.bits_equal(pm[f, r], ice[np.arange(n), PC.own_cell(ens, f, Xs[donor, f])]), (f, r)


def test_feature_masks_are_the_override_masks():
    for ens in (PC.hand_ensemble(), PC.random_case(d=30, depth=5, T=7, n=4, seed=6)[0]):
        fm = feature_masks(ens)
        assert fm.shape == (ens.n_trees, 32) and fm.dtype == np.uint32 and not fm[:, ens.n_features:].any()
        for f in range(ens.n_features):
            assert np.array_equal(fm[:, f], override_words(ens, f)[0])


def test_ops_cpu_path_is_the_oracle_on_standardized_rows():
    from fraud_detection_amd.models.explainers import _standardize

    ens, Xs = PC.random_case(d=3, depth=3, T=5, n=70, seed=7, learn=True, nan_rows=True)
    mean, scale = np.array([1.0, -2.0, 0.5]), np.array([2.0, 0.5, 4.0])
    X = (Xs.astype(np.float64) * scale + mean).astype(np.float32)
    expl = TreePermutationImportance(ens, mean, scale, device="cpu")
    pm, base = permuted_margins(torch.from_numpy(X), expl, (2, 0), 2, 3)
    want, wbase = R.permuted_margins_reference(_standardize(X, mean, scale), ens, (2, 0), 2, 3)
    assert PC.bits_equal(pm, want) and PC.bits_equal(base, wbase)
    tp, tb = permuted_margins(torch.from_numpy(X), expl, (2, 0), 2, 3, sync=False)
    assert isinstance(tp, torch.Tensor) and PC.bits_equal(tp.numpy(), want) and PC.bits_equal(tb.numpy(), wbase)


# ---- invariants ------------------------------------------------------------------------------------
def test_one_row_has_importance_zero():
    ens, Xs = PC.random_case(d=4, depth=3, T=5, n=1, seed=8)
    res = _expl(ens).permutation_importance(Xs, np.array([1]), scoring="logloss", n_repeats=3)
    assert np.all(res.raw == res.baseline_raw) and not res.importances.any() and not res.importances_std.any()


def test_unused_feature_baseline_and_the_summary_statistics():
    ens, Xs = PC.random_case(d=4, depth=3, T=9, n=200, seed=9, learn=True, nan_rows=True)
    ens = TC.make_ensemble(4, 3, np.where(ens.feat == 3, -1, ens.feat), ens.thr, ens.leaf)    # nothing on feature 3
    y = QC.labels(Xs, ens, 10)
    expl = _expl(ens)
    pm, base = permuted_margins(torch.from_numpy(Xs), expl, None, 2, 0)
    assert PC.bits_equal(base, PC.margin(Xs, ens)) and PC.bits_equal(pm[3], np.stack([base, base]))
    for scoring in ("auc", "aucpr", "logloss"):
        res = expl.permutation_importance(Xs, y, scoring=scoring, n_repeats=4, seed=11)
        assert isinstance(res, PermutationImportance) and res.features == (0, 1, 2, 3)
        assert res.raw.dtype == np.int64 and res.raw.shape == (4, 4) and isinstance(res.baseline_raw, int)
        assert np.all(res.raw[3] == res.baseline_raw) and not res.importances[3].any()
        assert np.array_equal(res.importances, res.baseline_score - res.scores)
        assert np.array_equal(res.importances_mean, res.importances.mean(1))
        assert np.array_equal(res.importances_std, res.importances.std(1, ddof=0))
        assert (res.scoring, res.n_repeats, res.seed) == (scoring, 4, 11)


@pytest.mark.parametrize("scoring", ["auc", "aucpr", "logloss"])
def test_raw_is_the_reference_scorer_on_the_oracle_margins(scoring):
    ens, Xs = PC.random_case(d=4, depth=3, T=9, n=300, seed=12, learn=True, nan_rows=True)
    y = QC.labels(Xs, ens, 13)
    P, n = int(y.sum()), len(y)
    raw, base_raw, pos = permutation_scores(torch.from_numpy(Xs), torch.from_numpy(y), _expl(ens), (1, 3), scoring, 3, 5)
    want, wbase = QC.oracle_raw(Xs, y, ens, (1, 3), 3, 5, scoring)
    assert np.array_equal(raw, want) and base_raw == wbase and pos == P
    res = _expl(ens).permutation_importance(Xs, y, scoring=scoring, n_repeats=3, seed=5, features=(1, 3))
    assert np.array_equal(res.raw, want) and res.baseline_raw == wbase
    to_score = {"auc": lambda q: q / (2.0 * P * (n - P)), "aucpr": lambda q: q / 2.0 ** 30 / P,
                "logloss": lambda q: -q / 2.0 ** 30 / n}[scoring]
    assert res.baseline_score == to_score(wbase) and np.array_equal(res.scores, to_score(want.astype(np.float64)))
    if scoring == "auc":
        from fraud_detection_amd.ops.reference import roc_auc

        assert abs(res.baseline_score - roc_auc(PC.margin(Xs, ens), y.astype(bool))) < 1e-12


# ---- estimator -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fitted():
    from fraud_detection_amd.models.gbdt import GBDTClassifier

    rng = np.random.default_rng(14)
    X = rng.normal(size=(600, 4)).astype(np.float32)
    y = (X[:, 0] + 0.25 * rng.normal(size=600) > 0).astype(np.uint8)
    return GBDTClassifier(n_estimators=6, max_depth=3, device="cpu").fit(X, y), X, y


@pytest.mark.parametrize("scoring", ["auc", "aucpr", "logloss"])
def test_the_informative_feature_ranks_first(fitted, scoring):
    m, X, y = fitted
    res = m.permutation_importance(X, y, scoring=scoring)
    assert res.raw.shape == (4, 5) and res.features == (0, 1, 2, 3)
    assert int(np.argmax(res.importances_mean)) == 0 and res.importances_mean[0] > 0.05
    want, wbase = QC.oracle_raw(X, y, m.ensemble, (0, 1, 2, 3), 5, 0, scoring)
    assert np.array_equal(res.raw, want) and res.baseline_raw == wbase


def test_iteration_range_is_the_truncated_model(fitted):
    m, X, y = fitted
    res = m.permutation_importance(X, y, n_repeats=2, seed=3, iteration_range=(0, 1))
    want, wbase = QC.oracle_raw(X, y, m.ensemble.head(1), (0, 1, 2, 3), 2, 3, "auc")
    assert np.array_equal(res.raw, want) and res.baseline_raw == wbase
    full = m.permutation_importance(X, y, n_repeats=2, seed=3)
    assert full.baseline_raw != res.baseline_raw


def test_errors(fitted):
    m, X, y = fitted
    for kw in (dict(scoring="f1"), dict(n_repeats=0), dict(features=[4]), dict(features=[-1]), dict(features=[1, 1]),
               dict(seed=-1), dict(seed=2 ** 32)):
        with pytest.raises(ValueError):
            m.permutation_importance(X, y, **kw)
    with pytest.raises(ValueError):
        m.permutation_importance(X, y[:-1])
    for scoring in ("auc", "aucpr"):
        for yy in (np.zeros(600, np.uint8), np.ones(600, np.uint8)):
            with pytest.raises(ValueError):
                m.permutation_importance(X, yy, scoring=scoring)
    assert m.permutation_importance(X, np.zeros(600, np.uint8), scoring="logloss", n_repeats=1).raw.shape == (4, 1)


def test_a_pickled_classifier_gives_equal_results(fitted):
    m, X, y = fitted
    a = m.permutation_importance(X, y, scoring="aucpr", n_repeats=2, features=[0, 2])
    assert getattr(m, "_piexpl", None) is not None
    m2 = pickle.loads(pickle.dumps(m))
    assert getattr(m2, "_piexpl", None) is None
    b = m2.permutation_importance(X, y, scoring="aucpr", n_repeats=2, features=[0, 2])
    assert np.array_equal(a.raw, b.raw) and a.baseline_raw == b.baseline_raw
    assert np.array_equal(a.importances, b.importances) and a.features == b.features == (0, 2)
