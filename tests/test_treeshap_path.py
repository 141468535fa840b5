"""Path-dependent TreeSHAP and node covers on the host: the per-leaf oracle
(models/explainers.treeshap_path_reference) against brute force over all coalitions of the EXPVALUE
game, the helpers the device tests stand on (tests/_tree_path_cases.py: coverage and mutants), the
identities of the game, NaN routing, reference_gbdt.node_cover, serialisation and the public
interface's errors."""
import json

import numpy as np
import pytest
import torch

import _tree_cases as TC
import _tree_path_cases as PC
from fraud_detection_amd.models.explainers import TreeExplainer, TreePathExplainer, treeshap_path_reference
from fraud_detection_amd.models.gbdt import GBDTClassifier
from fraud_detection_amd.ops import gbdt as gb
from fraud_detection_amd.ops import reference_gbdt as R

CASES = [(1, 3), (3, 2), (4, 6), (5, 4), (5, 7)]
# split nodes of cover 0 in the four deeper cases (40 rows thin out quickly below the root)
ZERO_COVER = {(3, 2): 3, (4, 6): 19, (5, 4): 63, (5, 7): 60}


@pytest.fixture(scope="module")
def solved():
    """Per case: (ens, Xs, Bs, path_stats, brute force), computed once and left unchanged."""
    out = {}
    for depth, d in CASES:
        ens, Xs, Bs = PC.covered_case(depth, d)
        out[(depth, d)] = (ens, Xs, Bs, PC.path_stats(Xs, ens), PC.brute_force(Xs, ens))
    return out


def _as_device(phi):
    """What a correct kernel would hand back at best: the exact values rounded to fp32."""
    return phi.astype(np.float32).astype(np.float64)


# ---------------------------------------------------------------------------------------------
# the per-leaf form against brute force, and what the cases reach
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth,d", CASES)
def test_reference_matches_brute_force(solved, depth, d):
    ens, Xs, Bs, st, (bphi, bfx, bf0) = solved[(depth, d)]
    phi, fx, f0 = treeshap_path_reference(Xs, ens)
    np.testing.assert_allclose(phi, bphi, rtol=0, atol=1e-12)
    np.testing.assert_allclose(st["phi"], bphi, rtol=0, atol=1e-12)
    assert abs(f0 - bf0) <= 1e-12 and abs(st["f0"] - bf0) <= 1e-12
    np.testing.assert_allclose(st["fx"], bfx, rtol=0, atol=1e-12)
    np.testing.assert_allclose(fx, bfx, rtol=0, atol=ens.n_trees * TC.U * st["fx_abs"].max())  # fp32 tree-order sum


def test_cases_reach_what_they_are_there_for(solved):
    for key, want in ZERO_COVER.items():
        ens, _, _, st, _ = solved[key]
        D = ens.depth
        split0 = (ens.feat >= 0) & (ens.cover[:, 1: 1 << D] == 0)
        assert int(split0.sum()) == want and st["zero_cover"] > 0, key
    assert solved[(3, 2)][3]["repeats"] > 0 and solved[(5, 4)][3]["repeats"] > 0
    assert all(solved[k][3]["dead"] > 0 for k in ZERO_COVER)
    assert solved[(5, 7)][3]["max_m"] == 5


# ---------------------------------------------------------------------------------------------
# mutants fail the assertion the device tests make, at the same bound
# ---------------------------------------------------------------------------------------------
def _mutant_inputs(mutant):
    if mutant == "ignore_default_left":
        ens, Xs, Bs = PC.covered_case(4, 6)
        ens = PC.with_count_cover(PC.with_default_left(ens, 5), Bs)
        Xs = Xs.copy()
        Xs[0, 1] = Xs[1, :] = np.nan
        return ens, Xs
    ens, Xs, _ = PC.covered_case(5, 4)
    return ens, Xs


@pytest.mark.parametrize("mutant", PC.MUTANTS)
def test_device_assertions_reject_mutants(mutant):
    ens, Xs = _mutant_inputs(mutant)
    st = PC.path_stats(Xs, ens)
    if mutant == "no_merge":
        assert st["repeats"] > 0
    elif mutant == "ignore_default_left":
        assert st["nan_default_left"] > 0
    oracle = PC.brute_force(Xs, ens)[0]
    bound = PC.phi_bound(st["S"], ens.n_trees, ens.depth)
    PC.assert_within(_as_device(st["phi"]), oracle, bound, f"faithful per-leaf form ({mutant} inputs)")
    bad = PC.path_stats(Xs, ens, mutant)["phi"]
    with pytest.raises(AssertionError, match="exceeds the derived bound"):
        PC.assert_within(_as_device(bad), oracle, bound, f"mutant {mutant}")


# ---------------------------------------------------------------------------------------------
# identities
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth,d", CASES)
def test_efficiency_and_count_identity(solved, depth, d):
    ens, Xs, Bs, st, _ = solved[(depth, d)]
    np.testing.assert_allclose(st["phi"].sum(1), st["fx"] - st["f0"], rtol=0, atol=1e-13)
    # count covers: the expected value is the mean margin of the rows the cover was taken over
    assert abs(st["f0"] - TC.margins64(Bs, ens)[0].mean()) <= 1e-13


def test_unsplit_feature_gets_exactly_zero():
    ens, Xs, Bs = TC.oracle_case(4, 6, T=6, n_bg=40)
    feat = np.where(ens.feat == 2, 3, ens.feat)
    ens = PC.with_count_cover(TC.make_ensemble(6, 4, feat, ens.thr, ens.leaf, ens.base_score), Bs)
    phi = treeshap_path_reference(Xs, ens)[0]
    assert np.all(phi[:, 2] == 0.0) and np.any(phi[:, 3] != 0.0)


# ---------------------------------------------------------------------------------------------
# NaN
# ---------------------------------------------------------------------------------------------
def test_nan_follows_default_left_both_ways():
    """One split on feature 0: a NaN lands left with default_left set and right without."""
    feat = np.array([[0]], np.int32)
    thr, leaf = np.zeros((1, 1), np.float32), np.array([[-1.0, 2.0]], np.float32)
    rows = np.array([[-1.0], [-1.0], [-1.0], [1.0]], np.float32)  # cover 3 left, 1 right
    x = np.array([[np.nan]], np.float32)
    for dl, want_leaf in ((1, -1.0), (0, 2.0)):
        from dataclasses import replace

        ens = replace(TC.make_ensemble(1, 1, feat, thr, leaf), default_left=np.array([[dl]], np.uint8))
        ens = PC.with_count_cover(ens, rows)
        phi, fx, f0 = treeshap_path_reference(x, ens)
        assert f0 == pytest.approx(ens.base_margin + 0.75 * -1.0 + 0.25 * 2.0, abs=1e-15)
        assert fx[0] == pytest.approx(ens.base_margin + want_leaf, abs=1e-6)
        assert phi[0, 0] == pytest.approx(ens.base_margin + want_leaf - f0, abs=1e-15)
        b = PC.brute_force(x, ens)
        np.testing.assert_allclose(phi, b[0], rtol=0, atol=1e-15)


def test_all_nan_row_and_brute_force_with_default_left():
    ens, Xs = _mutant_inputs("ignore_default_left")
    assert np.all(np.isnan(Xs[1])) and ens.has_default_left
    phi, fx, f0 = treeshap_path_reference(Xs, ens)
    bphi, bfx, bf0 = PC.brute_force(Xs, ens)
    assert np.all(np.isfinite(phi))
    np.testing.assert_allclose(phi, bphi, rtol=0, atol=1e-12)
    np.testing.assert_allclose(phi.sum(1), bfx - bf0, rtol=0, atol=1e-12)
    m = R.predict_margin(Xs, ens.feat, ens.thr, ens.leaf, ens.depth, ens.base_margin, ens.default_left)
    np.testing.assert_allclose(fx, m.astype(np.float64), rtol=0, atol=0)


def test_learned_missing_directions_explain_on_the_cpu_path():
    rng = np.random.default_rng(3)
    X = rng.normal(size=(600, 5)).astype(np.float32)
    y = (X[:, 0] + 0.5 * X[:, 1] > 0.3).astype(np.uint8)
    X[rng.random(X.shape) < 0.15] = np.nan
    clf = GBDTClassifier(n_estimators=5, max_depth=3, missing_policy="learn", device="cpu")
    clf.fit(X, y, record_cover=True)
    assert clf.ensemble.has_default_left and clf.ensemble.cover_kind == "hessian"
    te = TreePathExplainer(clf.ensemble, np.zeros(5), np.ones(5), device="cpu")
    phi, fx, f0 = te.explain(X[:8])
    assert np.isnan(X[:8]).any() and np.all(np.isfinite(phi))
    np.testing.assert_allclose(phi.sum(1), fx - f0, rtol=0, atol=1e-6)
    np.testing.assert_allclose(fx, clf.predict_margin(X[:8]), rtol=0, atol=0)
    contrib = clf.predict_contribs(X[:8])
    assert contrib.shape == (8, 6)
    np.testing.assert_allclose(contrib.sum(1), clf.predict_margin(X[:8]), rtol=0, atol=1e-6)
    np.testing.assert_allclose(contrib[:, -1], te.expected_value, rtol=0, atol=0)


# ---------------------------------------------------------------------------------------------
# reference_gbdt.node_cover
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["count", "hessian"])
def test_node_cover_oracle(kind):
    ens, Xs, Bs = TC.oracle_case(4, 6, T=7, n_bg=300)
    ens = PC.with_default_left(ens, 9)
    Bs = Bs.copy()
    Bs[::7, 2] = np.nan
    q = R.node_cover(Bs, ens.feat, ens.thr, ens.leaf, ens.depth, ens.base_margin, ens.default_left, kind)
    nl = 1 << ens.depth
    assert q.dtype == np.int64 and q.shape == (7, 2 * nl) and np.all(q[:, 0] == 0)
    for k in range(1, nl):
        assert np.array_equal(q[:, k], q[:, 2 * k] + q[:, 2 * k + 1])
    if kind == "count":
        assert np.all(q[:, 1] == len(Bs))
        assert np.array_equal(q, PC.count_cover(ens, Bs))
    else:
        for t in range(ens.n_trees):  # the root's sum is the hessian of predict_margin(..., n_trees = t)
            m = gb.predict_margin(torch.from_numpy(Bs), ens, n_trees=t).numpy().astype(np.float64)
            p = 1.0 / (1.0 + np.exp(-m))
            assert q[t, 1] == np.rint(p * (1.0 - p) * 2.0 ** 30).astype(np.int64).sum()
    assert np.array_equal(gb.node_cover(torch.from_numpy(Bs), ens, kind).numpy(), q)
    with pytest.raises(ValueError, match="cover kind"):
        gb.node_cover(torch.from_numpy(Bs), ens, "gain")


# ---------------------------------------------------------------------------------------------
# serialisation
# ---------------------------------------------------------------------------------------------
def test_cover_round_trip_and_absent_key(tmp_path):
    ens, Xs, Bs = TC.oracle_case(3, 4, T=5, n_bg=50)
    o = ens.to_dict()
    assert "cover" not in o and "cover_kind" not in o
    q = R.node_cover(Bs, ens.feat, ens.thr, ens.leaf, ens.depth, ens.base_margin, None, "hessian")
    ec = ens.with_cover(q, "hessian")
    assert np.array_equal(ec.cover, q / 2.0 ** 30)
    back = gb.TreeEnsemble.from_dict(json.loads(json.dumps(ec.to_dict())))
    assert back.cover_kind == "hessian" and np.array_equal(back.cover, ec.cover) and back.cover.dtype == np.float64
    assert gb.TreeEnsemble.from_dict(json.loads(json.dumps(o))).cover is None
    # a model without cover writes the file it always wrote: dropping the cover restores the bytes
    clf = GBDTClassifier(device="cpu")
    clf.ensemble = ens
    clf.save_model(str(tmp_path / "plain.json"))
    clf.ensemble = ec
    clf.save_model(str(tmp_path / "cover.json"))
    plain = (tmp_path / "plain.json").read_bytes()
    assert plain == json.dumps({**ens.to_dict(), "feature_names": None}).encode()
    with_cover = json.loads((tmp_path / "cover.json").read_text())
    for k in ("cover", "cover_kind"):
        with_cover.pop(k)
    assert list(with_cover) == list(json.loads(plain)) and json.dumps(with_cover).encode() == plain
    loaded = GBDTClassifier.load_model(str(tmp_path / "cover.json"), device="cpu")
    contrib = loaded.predict_contribs(Xs)
    np.testing.assert_allclose(contrib.sum(1), loaded.predict_margin(Xs), rtol=0, atol=1e-6)
    np.testing.assert_allclose(contrib[:, :-1], treeshap_path_reference(Xs, ec)[0], rtol=0, atol=0)
    k2 = loaded.predict_contribs(Xs, iteration_range=(0, 2))
    np.testing.assert_allclose(k2.sum(1), loaded.predict_margin(Xs, iteration_range=(0, 2)), rtol=0, atol=1e-6)
    np.testing.assert_allclose(k2[:, :-1], treeshap_path_reference(Xs, ec.head(2))[0], rtol=0, atol=0)


def test_cover_importances():
    ens, Xs, Bs = PC.covered_case(3, 4, T=5, n_bg=50)
    tot = ens.feature_importance("total_cover")
    want = np.zeros(4)
    for t, n in zip(*np.nonzero(ens.feat >= 0)):
        want[ens.feat[t, n]] += ens.cover[t, n + 1]
    assert np.array_equal(tot, want)
    cnt = ens.feature_importance("weight")
    np.testing.assert_allclose(ens.feature_importance("cover"), np.where(cnt > 0, want / np.maximum(cnt, 1), 0))
    np.testing.assert_allclose(ens.feature_importance("total_gain"), ens.feature_importance("gain") * cnt)
    with pytest.raises(ValueError, match="node_cover"):
        TC.oracle_case(3, 4)[0].feature_importance("cover")


# ---------------------------------------------------------------------------------------------
# interface errors
# ---------------------------------------------------------------------------------------------
def test_missing_cover_is_refused_by_name():
    ens, Xs, Bs = TC.oracle_case(3, 4, T=5, n_bg=50)
    with pytest.raises(ValueError, match="node_cover"):
        TreePathExplainer(ens, np.zeros(4), np.ones(4), device="cpu")
    clf = GBDTClassifier(device="cpu")
    clf.ensemble = ens
    with pytest.raises(ValueError, match="node_cover"):
        clf.predict_contribs(Xs)
    assert clf.compute_cover(Bs, kind="count") is clf and clf.ensemble.cover_kind == "count"
    assert clf.predict_contribs(Xs).shape == (3, 5)
    with pytest.raises(ValueError):
        TreePathExplainer(PC.with_count_cover(TC.random_ensemble(3, 6, 2, 0), Bs[:, :3]), np.zeros(3), np.ones(3),
                          device="cpu")


def test_engine_serves_tree_path_without_background():
    from fraud_detection_amd.serve.engine import TreeInferenceEngine

    ens, Xs, Bs = PC.covered_case(4, 6)
    d = 6
    mean, scale = np.full(d, 0.25), np.full(d, 2.0)
    names = [f"f{i}" for i in range(d)]
    plain = TreeInferenceEngine(TC.oracle_case(4, 6, T=6, n_bg=40)[0], mean, scale ** 2, scale, names, device="cpu")
    with pytest.raises(ValueError, match="node covers"):
        plain.explain(Xs, "tree_path")
    with pytest.raises(ValueError, match="background"):
        plain.explain(Xs, "auto")  # auto is still KernelSHAP, and still needs its background
    eng = TreeInferenceEngine(ens, mean, scale ** 2, scale, names, device="cpu")
    assert eng.default_method == "kernel" and "tree_path" in eng.methods and not eng.has_background
    with pytest.raises(ValueError, match="background"):
        eng.explain(Xs, "auto")
    with pytest.raises(ValueError, match="background"):
        eng.explain(Xs, "tree")
    ex = eng.explain(Xs, "tree_path")
    assert (ex.method, ex.space) == ("tree_path", "log-odds") and ex.phi.shape == (3, d)
    want = TreePathExplainer(ens, mean, scale, device="cpu").explain(Xs)
    assert np.array_equal(ex.phi, want[0]) and np.array_equal(ex.logit, want[1]) and ex.base_value == want[2]
    np.testing.assert_allclose(ex.phi.sum(1), ex.logit - ex.base_value, rtol=0, atol=1e-6)
    np.testing.assert_allclose(ex.prob, eng.predict_proba(Xs)[0], rtol=0, atol=1e-12)
    e0 = eng.explain(Xs[:0], "tree_path")
    assert e0.phi.shape == (0, d) and e0.method == "tree_path"


def test_interventional_explainers_still_refuse_default_left():
    ens, Xs, Bs = PC.covered_case(3, 4)
    ens = PC.with_default_left(ens, 1)
    with pytest.raises(NotImplementedError):
        TreeExplainer(ens, np.zeros(4), np.ones(4), Bs, device="cpu")
    TreePathExplainer(ens, np.zeros(4), np.ones(4), device="cpu").explain(Xs)
