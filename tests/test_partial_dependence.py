"""Partial dependence and ICE of the GBDT margin on the CPU: the grid definition, the numpy oracle
(ops/reference_gbdt.partial_dependence_reference) against plain predict_margin loops, the override
words of the device formulation (ops/pdp.ice_from_words) against the oracle, the identities the
curves must satisfy, recursion, and the refusals."""
from __future__ import annotations

from dataclasses import replace

import numpy as np
import pytest

import _pd_cases as PC
import _tree_cases as TC
import _tree_path_cases as TPC
from fraud_detection_amd.models.explainers import (TreePartialDependence, partial_dependence_recursion,
                                                   path_expected_value)
from fraud_detection_amd.models.gbdt import GBDTClassifier
from fraud_detection_amd.ops import reference_gbdt as R
from fraud_detection_amd.ops.pdp import ice_from_words, override_words


# ---- the grid -------------------------------------------------------------------------------------
def test_grid_of_a_hand_built_ensemble():
    ens = PC.hand_ensemble()
    assert R.pd_grid(ens, 0).tolist() == [-0.5, 0.5, 1.5]          # 0.5 sits in two trees: one edge
    assert R.pd_grid(ens, 1).tolist() == [1.0]
    assert R.pd_grid(ens, 2).tolist() == [2.0]                     # the -inf node adds no edge
    assert R.pd_grid(ens, 3).tolist() == []                        # unused
    reps, missing = R.pd_cells(ens, 0)
    assert missing and len(reps) == 5 and reps[0] == -np.inf and np.isnan(reps[-1])
    assert reps[1:4].tolist() == [-0.5, 0.5, 1.5]
    assert len(R.pd_cells(ens, 3)[0]) == 2                         # one value cell and the missing cell
    plain = PC.hand_ensemble(default_left=False)
    assert len(R.pd_cells(plain, 3)[0]) == 1                       # a feature no tree uses: one cell
    assert len(R.pd_cells(plain, 0)[0]) == 4
    with pytest.raises(ValueError):
        R.pd_grid(ens, 4)


def test_override_words_of_a_hand_built_ensemble():
    ens = PC.hand_ensemble()
    mask, words = override_words(ens, 2)
    assert mask.tolist() == [0, 2 << 2, 2 << 0]
    # cells of feature 2: -inf, 2.0, missing.  Tree 1 node 2 (thr 2.0): right from the edge on and for
    # missing (its default_left is 0); tree 2 node 0 (thr -inf, default_left): every value goes right,
    # missing goes left
    assert words[1].tolist() == [0, 2 << 2, 2 << 2]
    assert words[2].tolist() == [2 << 0, 2 << 0, 0]
    mask0, words0 = override_words(ens, 0)
    assert mask0.tolist() == [(2 << 0) | (2 << 2), 2 << 0, (2 << 1) | (2 << 2)]
    # tree 0: node 0 thr 0.5, node 2 thr -0.5 with default_left; cells -inf, -0.5, 0.5, 1.5, missing
    assert words0[0].tolist() == [0, 2 << 2, (2 << 0) | (2 << 2), (2 << 0) | (2 << 2), 2 << 0]
    assert override_words(ens, 3)[0].tolist() == [0, 0, 0]


# ---- the oracle -----------------------------------------------------------------------------------
CASES = [dict(d=4, depth=3, T=7, n=40, seed=1), dict(d=4, depth=3, T=7, n=40, seed=2, learn=True, nan_rows=True),
         dict(d=3, depth=5, T=5, n=25, seed=3, nan_rows=True), dict(d=1, depth=2, T=4, n=9, seed=4),
         dict(d=6, depth=1, T=9, n=30, seed=5, learn=True, nan_rows=True)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"d{c['d']}D{c['depth']}s{c['seed']}")
def test_oracle_equals_predict_margin_loops_and_the_word_form(case):
    ens, Xs = PC.random_case(**case)
    d = case["d"]
    feats = list(range(min(d, 3))) + ([(0, d - 1), (d - 1, 0)] if d > 1 else [])
    for f in feats:
        want = PC.loop_ice(Xs, ens, f)
        q, ice = R.partial_dependence_reference(Xs, ens, f)
        assert PC.bits_equal(ice, want), f
        assert np.array_equal(q, PC.pd_q_of(want)), f
        assert R.partial_dependence_reference(Xs, ens, f, ice=False)[1] is None
        assert PC.bits_equal(ice_from_words(Xs, ens, f), want), f


def test_pair_is_flattened_row_major():
    ens, Xs = PC.random_case(d=4, depth=3, T=7, n=10, seed=1)
    pd = TreePartialDependence(ens, np.zeros(4), np.ones(4), device="cpu").partial_dependence(Xs, (0, 2), ice=True)
    ca, cb = len(pd.edges[0]) + 1, len(pd.edges[1]) + 1
    assert pd.average.shape == (ca, cb) and pd.ice.shape == (10, ca, cb) and pd.pd_q.shape == (ca, cb)
    Xm = Xs.copy()
    Xm[:, 0], Xm[:, 2] = pd.edges[0][1], -np.inf                    # cell (2, 0)
    assert PC.bits_equal(pd.ice[:, 2, 0], PC.margin(Xm, ens))
    assert np.array_equal(pd.average, pd.pd_q / 2.0 ** 30 / 10)


# ---- identities on fitted models ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def fits():
    rng = np.random.default_rng(0)
    X = rng.normal(size=(700, 4)).astype(np.float32)
    y = (X[:, 0] - X[:, 2] + 0.5 * X[:, 1] * X[:, 3] + 0.3 * rng.normal(size=700) > 0).astype(np.uint8)
    Xn = X.copy()
    Xn[rng.random(X.shape) < 0.1] = np.nan
    kw = dict(n_estimators=7, max_depth=3, device="cpu")
    return {"plain": (GBDTClassifier(**kw).fit(X, y), X),
            "learn": (GBDTClassifier(missing_policy="learn", **kw).fit(Xn, y), Xn),
            "mono": (GBDTClassifier(monotone_constraints=(1, 0, -1, 0), **kw).fit(X, y), X)}


@pytest.mark.parametrize("name", ["plain", "learn", "mono"])
def test_own_cell_is_the_models_margin(fits, name):
    m, X = fits[name]
    fx = m.predict_margin(X)
    for f in range(4):
        pd = m.partial_dependence(X, f, kind="both")
        assert pd.has_missing_cell == (name == "learn")
        c = PC.own_cell(m.ensemble, f, X[:, f])
        nan = np.isnan(X[:, f])
        assert nan.any() == (name == "learn")
        assert np.all(c[nan] == pd.ice.shape[1] - 1)                # a NaN lands in the missing cell
        assert PC.bits_equal(pd.ice[np.arange(len(X)), c], fx), (name, f)


def test_monotone_fit_has_monotone_curves(fits):
    m, X = fits["mono"]
    for f, sign in ((0, 1), (2, -1)):
        pd = m.partial_dependence(X, f, kind="both")
        assert pd.ice.shape[1] > 3
        assert np.all(sign * np.diff(pd.ice, axis=1) >= 0), f       # exact: no tolerance
        assert np.all(sign * np.diff(pd.pd_q) >= 0), f
        assert sign * (pd.pd_q[-1] - pd.pd_q[0]) > 0


def test_classifier_iteration_range_and_kinds(fits):
    m, X = fits["plain"]
    head = m.partial_dependence(X, 0, kind="individual", iteration_range=(0, 3))
    want = R.partial_dependence_reference(X, m.ensemble.head(3), 0)
    assert np.array_equal(head.pd_q, want[0]) and PC.bits_equal(head.ice, want[1])
    avg = m.partial_dependence(X, 0)
    assert avg.ice is None and avg.method == "brute" and avg.n_rows == 700
    with pytest.raises(ValueError):
        m.partial_dependence(X, 0, kind="mean")
    with pytest.raises(ValueError):
        m.partial_dependence(X, 0, method="exact")


def test_raw_units_go_through_the_scaler():
    ens, Xs = PC.random_case(d=3, depth=3, T=5, n=20, seed=9)
    mean, scale = np.array([1.0, -2.0, 0.5]), np.array([2.0, 0.5, 4.0])
    te = TreePartialDependence(ens, mean, scale, device="cpu")
    e, raw = te.grid(1)
    assert np.array_equal(e, R.pd_grid(ens, 1)) and np.array_equal(raw, e.astype(np.float64) * 0.5 - 2.0)
    X = (Xs.astype(np.float64) * scale + mean).astype(np.float32)
    from fraud_detection_amd.models.explainers import _standardize

    pd = te.partial_dependence(X, 1, ice=True)
    assert PC.bits_equal(pd.ice, PC.loop_ice(_standardize(X, mean, scale), ens, 1))


# ---- recursion ------------------------------------------------------------------------------------------
def test_recursion_at_depth_one_is_the_brute_mean():
    """Depth 1, count covers over the same NaN-free rows: both are base + sum_t (the mean leaf of the
    rows, or the side's leaf at a node on f).  The two fp64 sums round differently by at most
    n 2^-52 sum_t max |leaf_t|."""
    n = 900
    ens, Xs = PC.random_case(d=4, depth=1, T=40, n=n, seed=11)
    ens = TPC.with_count_cover(ens, Xs)
    bound = n * 2.0 ** -52 * float(np.abs(ens.leaf.astype(np.float64)).max(1).sum())
    for f in range(4):
        rec = partial_dependence_recursion(ens, f)
        reps = R.pd_cells(ens, f)[0]
        assert rec.shape == reps.shape
        for c, v in enumerate(reps):
            Xm = Xs.copy()
            Xm[:, f] = v
            mean = float(np.mean(TC.margins64(Xm, ens)[0]))
            assert abs(rec[c] - mean) <= bound, (f, c, rec[c] - mean, bound)


def test_recursion_differs_from_brute_where_features_interact(fits):
    m, X = fits["plain"]
    m.compute_cover(X, "count")
    rec = m.partial_dependence(None, 0, method="recursion")
    brute = m.partial_dependence(X, 0)
    assert rec.pd_q is None and rec.n_rows == 0 and rec.average.shape == brute.average.shape
    assert 1e-6 < np.abs(rec.average - brute.average).max() < 0.5
    with pytest.raises(ValueError):
        m.partial_dependence(None, 0, method="recursion", kind="both")


def test_recursion_of_an_unused_feature_is_the_expected_value():
    """No node on f: every factor is a path fraction, so rec = f0.  Both sum T 2^D products of D
    fractions and a leaf in fp64; weights of a tree sum to 1, so the sums differ by at most
    (T 2^D + D) 2^-52 (|base| + sum_t max |leaf_t|)."""
    ens, Xs = PC.random_case(d=5, depth=4, T=12, n=60, seed=13, learn=True)
    ens = replace(ens, feat=np.where(ens.feat == 4, 0, ens.feat))
    ens = TPC.with_count_cover(ens, Xs)
    rec = partial_dependence_recursion(ens, 4)
    assert rec.shape == (2,)                                         # the value cell and the missing cell
    bound = (12 * 16 + 4) * 2.0 ** -52 * TC.leaf_mass(ens)
    assert np.all(np.abs(rec - path_expected_value(ens)) <= bound)
    # and a pair with it is the other feature's curve, repeated
    pair = partial_dependence_recursion(ens, (4, 1)).reshape(2, -1)
    assert np.array_equal(pair[0], pair[1]) and np.array_equal(pair[0], partial_dependence_recursion(ens, 1))


# ---- explain_model.py --pdp ---------------------------------------------------------------------------
def test_explain_model_writes_pdp_plots(tmp_path, monkeypatch):
    import json
    import os
    import shutil

    import explain_model

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    shutil.copytree(os.path.join(root, "models"), tmp_path / "models")
    os.makedirs(tmp_path / "data")
    rng = np.random.default_rng(0)
    X = rng.normal(0, 1, (300, 30)).astype(np.float32)
    y = (X[:, 0] > 0).astype(np.int64)
    np.savez_compressed(tmp_path / "data" / "preprocessed_data.npz", X_res=X, y_res=y, X_test=X, y_test=y)
    ens = replace(TC.random_ensemble(30, 4, 12, 5), default_left=None)
    with open(tmp_path / "models" / "xgb_model.json", "w") as f:
        json.dump(ens.to_dict(), f)
    monkeypatch.chdir(tmp_path)
    out = explain_model.main(["--pdp", "Amount,Feature_3,5", "--pdp-rows", "120"])
    assert out["pdp_rows"] == 120
    assert out["pdp_cells"] == {"Amount": len(R.pd_grid(ens, 29)) + 1, "Feature_3": len(R.pd_grid(ens, 3)) + 1,
                                "5": len(R.pd_grid(ens, 5)) + 1}
    for name in ("Amount", "Feature_3", "5"):
        assert (tmp_path / "plots" / f"pdp_{name}.png").stat().st_size > 1000
    with pytest.raises(SystemExit, match="no feature named"):
        explain_model.pdp_explain(X, [f"f{i}" for i in range(30)], ["Amount"], 10)


# ---- refusals ---------------------------------------------------------------------------------------------
def test_refusals():
    ens, Xs = PC.random_case(d=4, depth=3, T=7, n=10, seed=1)
    te = TreePartialDependence(ens, np.zeros(4), np.ones(4), device="cpu")
    for bad in (4, -1, (0, 4), (1, 1), (0, 1, 2), ()):
        with pytest.raises(ValueError):
            te.partial_dependence(Xs, bad)
        with pytest.raises(ValueError):
            R.partial_dependence_reference(Xs, ens, bad)
    with pytest.raises(ValueError, match="needs the model's node covers"):
        te.partial_dependence(None, 0, method="recursion")
    with pytest.raises(ValueError, match="no node cover"):
        partial_dependence_recursion(ens, 0)
    with pytest.raises(ValueError):
        te.partial_dependence(Xs[:0], 0)
    # the cell cap: 256 x 256 cells pass the check, 257 x 256 do not
    assert R.pd_check(PC.cap_ensemble(255, 255), (0, 1), 1)[0] == (0, 1)
    with pytest.raises(ValueError, match="cells"):
        R.pd_check(PC.cap_ensemble(256, 255), (0, 1), 1)
    # the int64 guard: n (Mb + 1) 2^30 >= 2^63
    big = replace(ens, leaf=(ens.leaf * np.float32(1e9)))
    with pytest.raises(ValueError, match="overflow"):
        R.partial_dependence_reference(np.repeat(Xs, 4, 0), big, 0)
    mb = TC.leaf_mass(ens)
    assert R.pd_check(ens, 0, int(2.0 ** 33 / (mb + 1.0)) - 1)
    with pytest.raises(ValueError, match="overflow"):
        R.pd_check(ens, 0, int(2.0 ** 33 / (mb + 1.0)) + 1)
    # depth 6 is outside the family
    deep = TC.random_ensemble(4, 6, 2, 3)
    with pytest.raises(ValueError, match="depth 1..5"):
        TreePartialDependence(deep, np.zeros(4), np.ones(4), device="cpu")
    with pytest.raises(ValueError, match="depth 1..5"):
        R.partial_dependence_reference(Xs, deep, 0)
    m = GBDTClassifier(n_estimators=2, max_depth=6, device="cpu").fit(Xs, (Xs[:, 0] > 0).astype(np.uint8))
    with pytest.raises(ValueError, match="depth 1..5"):
        m.partial_dependence(Xs, 0)
    with pytest.raises(ValueError, match="needs the model's node covers"):
        GBDTClassifier(n_estimators=2, max_depth=2, device="cpu").fit(Xs, (Xs[:, 0] > 0).astype(np.uint8)) \
            .partial_dependence(None, 0, method="recursion")
