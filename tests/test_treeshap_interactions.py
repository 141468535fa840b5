"""SHAP interaction values of the path-dependent game on the host: the per-leaf oracle
(models/explainers.treeshap_interactions_reference) against the brute-force interaction index over
all coalitions, the helpers the device tests stand on (tests/_tree_interaction_cases.py: masses,
bounds and mutants), the identities of shap's and xgboost's convention, NaN routing and the
estimator's ``predict_interactions`` on the CPU path."""
import numpy as np
import pytest

import _tree_cases as TC
import _tree_interaction_cases as IC
import _tree_path_cases as PC
from fraud_detection_amd.models.explainers import (TreePathExplainer, _standardize, treeshap_interactions_reference,
                                                   treeshap_path_reference)
from fraud_detection_amd.models.gbdt import GBDTClassifier

CASES = [(1, 3), (3, 2), (4, 6), (5, 4), (5, 7)]


def _nan_case():
    ens, Xs, Bs = PC.covered_case(4, 6)
    ens = PC.with_count_cover(PC.with_default_left(ens, 5), Bs)
    Xs = Xs.copy()
    Xs[0, 1] = Xs[1, :] = np.nan
    return ens, Xs


@pytest.fixture(scope="module")
def solved():
    """Per case: (ens, Xs, interaction_stats, brute force), computed once and left unchanged."""
    out = {}
    for key in CASES + ["tie", "nan"]:
        if key == "tie":
            ens, Xs, _ = PC.covered_tie_case()
        elif key == "nan":
            ens, Xs = _nan_case()
        else:
            ens, Xs, _ = PC.covered_case(*key)
        out[key] = (ens, Xs, IC.interaction_stats(Xs, ens), IC.brute_force_interactions(Xs, ens))
    return out


def _fp64_bound(ens, Xs, st):
    return IC.fp64_bound(st["S2"], st["S"], ens.n_trees, ens.depth, IC.oracle_term(ens, Xs.shape[1]))


def _device_bound(ens, Xs, st):
    return IC.inter_bound(st["S2"], st["S"], st["e"], ens.n_trees, ens.depth, IC.oracle_term(ens, Xs.shape[1]))


# ---------------------------------------------------------------------------------------------
# the per-leaf form against brute force
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", CASES + ["tie"], ids=str)
def test_reference_matches_brute_force(solved, key):
    ens, Xs, st, (binter, bphi, bfx, bf0) = solved[key]
    inter, phi, fx, f0 = treeshap_interactions_reference(Xs, ens)
    bound = _fp64_bound(ens, Xs, st)
    IC.assert_within(inter, binter, bound, f"{key} reference vs brute force")
    IC.assert_within(st["inter"], binter, bound, f"{key} instrumented form vs brute force")
    pphi, pfx, pf0 = treeshap_path_reference(Xs, ens)
    np.testing.assert_allclose(phi, pphi, rtol=0, atol=1e-13)
    assert np.array_equal(fx, pfx) and f0 == pf0
    assert abs(f0 - bf0) <= 1e-12


@pytest.mark.parametrize("key", CASES + ["tie", "nan"], ids=str)
def test_symmetry_row_sums_and_total(solved, key):
    ens, Xs, st, _ = solved[key]
    inter, phi, fx, f0 = treeshap_interactions_reference(Xs, ens)
    d = Xs.shape[1]
    assert inter.shape == (len(Xs), d, d)
    assert np.array_equal(inter, inter.transpose(0, 2, 1))
    pphi = treeshap_path_reference(Xs, ens)[0]
    mass = st["S"] + st["S2"].sum(2)
    # d + 2 roundings of the diagonal and the row sum; the two references order phi's own sum over
    # leaves and subsets differently (T 2^D + 5 D + 3 roundings each, as fp64_bound counts them)
    n = d + 2 + 2 * (ens.n_trees * (1 << ens.depth) + 5 * ens.depth + 3)
    IC.assert_within(inter.sum(2), pphi, n * 2.0 ** -53 * mass, f"{key} rows sum to phi")
    # efficiency: the exact values satisfy it; fx is the fp32 tree-order sum
    tol = _fp64_bound(ens, Xs, st).sum((1, 2)) + ens.n_trees * TC.U * st["fx_abs"] + 1e-12
    IC.assert_within(inter.sum((1, 2)), fx - f0, tol, f"{key} total sums to fx - f0")


def test_depth_one_has_no_interactions(solved):
    ens, Xs, st, (binter, _, _, _) = solved[(1, 3)]
    inter = treeshap_interactions_reference(Xs, ens)[0]
    off = ~np.eye(3, dtype=bool)
    assert np.all(inter[:, off] == 0.0) and np.all(st["S2"] == 0.0)
    assert np.any(inter[:, ~off] != 0.0)
    # the brute-force second difference leaves fp64 noise there: the oracle's own term covers it
    assert np.all(np.abs(binter[:, off]) <= IC.oracle_term(ens, 3))


def test_nan_follows_default_left(solved):
    ens, Xs, st, (binter, _, _, _) = solved["nan"]
    assert st["nan_default_left"] > 0 and np.all(np.isnan(Xs[1]))
    inter = treeshap_interactions_reference(Xs, ens)[0]
    assert np.all(np.isfinite(inter))
    IC.assert_within(inter, binter, _fp64_bound(ens, Xs, st), "NaN rows: reference vs brute force")


# ---------------------------------------------------------------------------------------------
# mutants fail the assertion the device tests make, at the same bound
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutant", IC.MUTANTS)
def test_device_assertions_reject_mutants(solved, mutant):
    ens, Xs, st, (binter, _, _, _) = solved["nan" if mutant == "ignore_default_left" else (5, 4)]
    if mutant == "no_merge":
        assert st["repeats"] > 0
    elif mutant == "phi_weight":
        assert st["max_m"] >= 3        # the two weights agree at m = 2
    bound = _device_bound(ens, Xs, st)
    IC.assert_within(st["inter"], binter, bound, f"faithful per-leaf form ({mutant} inputs)")
    bad = IC.interaction_stats(Xs, ens, mutant)["inter"]
    off = ~np.eye(Xs.shape[1], dtype=bool)
    with pytest.raises(AssertionError, match="exceeds the derived bound"):
        IC.assert_within(bad[:, off], binter[:, off], bound[:, off], f"mutant {mutant}, off the diagonal")
    with pytest.raises(AssertionError, match="exceeds the derived bound"):
        IC.assert_within(bad, binter, bound, f"mutant {mutant}")


def test_restated_lds_rule():
    assert IC.interactions_lds_boundary(4, 5) == 61
    assert IC.interactions_lds_boundary(30, 5) == 54
    assert IC.interactions_lds_boundary(30, 2) == 437      # the 2048-tree model of the device tests streams


# ---------------------------------------------------------------------------------------------
# explainer and estimator on the CPU path
# ---------------------------------------------------------------------------------------------
def test_explainer_cpu_path(solved):
    ens, Xs, _, _ = solved[(4, 6)]
    mean, scale = np.full(6, 0.25), np.full(6, 2.0)
    X = (Xs * 2.0 + 0.25).astype(np.float32)
    te = TreePathExplainer(ens, mean, scale, device="cpu")
    inter, phi, fx, f0 = te.explain_interactions(X)
    want = treeshap_interactions_reference(_standardize(X, mean, scale), ens)
    assert np.array_equal(inter, want[0]) and np.array_equal(phi, want[1]) and f0 == te.f0
    assert np.array_equal(te.shap_interaction_values(X), inter)
    np.testing.assert_allclose(phi, te.explain(X)[0], rtol=0, atol=1e-13)   # the same sums in another order
    e0 = te.explain_interactions(X[:0])
    assert e0[0].shape == (0, 6, 6) and e0[1].shape == (0, 6) and e0[2].shape == (0,) and e0[3] == te.f0


def test_classifier_predict_interactions_cpu():
    rng = np.random.default_rng(5)
    X = rng.normal(size=(500, 4)).astype(np.float32)
    y = (X[:, 0] * X[:, 2] + 0.5 * X[:, 1] > 0.2).astype(np.uint8)
    clf = GBDTClassifier(n_estimators=5, max_depth=3, device="cpu").fit(X, y, record_cover=True)
    Xe = X[:6]
    inter = clf.predict_interactions(Xe)
    contrib = clf.predict_contribs(Xe)
    d = 4
    assert inter.shape == (6, d + 1, d + 1) and inter.dtype == np.float64
    assert np.all(inter[:, d, d] == contrib[:, d]) and np.all(inter[:, d, :d] == 0) and np.all(inter[:, :d, d] == 0)
    assert np.array_equal(inter[:, :d, :d], treeshap_interactions_reference(Xe, clf.ensemble)[0])
    assert np.any(inter[:, 0, 2] != 0.0)
    np.testing.assert_allclose(inter.sum(2), contrib, rtol=0, atol=1e-13)
    np.testing.assert_allclose(inter.sum((1, 2)), clf.predict_margin(Xe), rtol=0, atol=1e-6)
    assert clf._pexpl is not None and clf._pexpl[0][0] == 5   # one explainer, shared with predict_contribs
    k3 = clf.predict_interactions(Xe, iteration_range=(0, 3))
    assert np.array_equal(k3[:, :d, :d], treeshap_interactions_reference(Xe, clf.ensemble.head(3))[0])
    np.testing.assert_allclose(k3.sum(2), clf.predict_contribs(Xe, iteration_range=(0, 3)), rtol=0, atol=1e-13)
    plain = GBDTClassifier(n_estimators=2, max_depth=2, device="cpu").fit(X, y)
    with pytest.raises(ValueError, match="node_cover"):
        plain.predict_interactions(Xe)
