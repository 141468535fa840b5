"""treeshap_path.hip on the device against brute-force Shapley values of the EXPVALUE game.

Every case drives the public wrapper ops.treeshap.treeshap_path through TreePathExplainer(ens,
mean = 0, scale = 1): (x - 0) * 1 is exact and keeps a NaN, so the oracle sees bit-identical fp32
rows.  The oracle is tests/_tree_path_cases.brute_force (all 2^d coalitions, fp64, its own
traversal), the tolerances the derived bounds of _tree_path_cases.phi_bound / fx_bound /
efficiency_bound; tests/test_treeshap_path.py shows that the same assertion at the same bound rejects
a form that does not merge repeated features, takes the sibling's fraction or ignores default_left.
Each case prints its largest error / bound."""
import numpy as np
import pytest
import torch

import _tree_cases as TC
import _tree_path_cases as PC
from fraud_detection_amd.models.explainers import TreePathExplainer, _standardize
from fraud_detection_amd.ops.treeshap import treeshap_path, treeshap_path_lds_resident

pytestmark = pytest.mark.gpu


def _explainer(ens, dev):
    d = ens.n_features
    return TreePathExplainer(ens, np.zeros(d), np.ones(d), device=str(dev))


def _check(dev, ens, Xs, what, oracle=None, st=None):
    """Run the kernel and hold phi, fx, f0 and efficiency to the derived bounds."""
    te = _explainer(ens, dev)
    phi, fx, f0 = te.explain(Xs)
    T, D = ens.n_trees, ens.depth
    st = st if st is not None else PC.path_stats(Xs, ens)
    bphi, bfx, bf0 = oracle if oracle is not None else PC.brute_force(Xs, ens)
    assert phi.shape == Xs.shape and fx.shape == (len(Xs),)
    PC.assert_within(phi, bphi, PC.phi_bound(st["S"], T, D), f"{what} phi vs brute force")
    PC.assert_within(fx, bfx, PC.fx_bound(st["fx_abs"], T, ens.base_margin), f"{what} fx")
    assert f0 == te.f0
    PC.assert_within(f0, bf0, PC.f0_bound(st["f0_abs"], T, D), f"{what} f0")
    PC.assert_within(phi.sum(1), fx - f0, PC.efficiency_bound(st["S"], st["fx_abs"], st["f0_abs"], T, D,
                                                             ens.base_margin), f"{what} efficiency")
    return st, (phi, fx, f0)


@pytest.mark.parametrize("depth,d", [(1, 3), (3, 2), (4, 6), (5, 4), (5, 7)])
def test_matches_brute_force(dev, depth, d):
    ens, Xs, _ = PC.covered_case(depth, d)
    st, _ = _check(dev, ens, Xs, f"depth {depth} d {d}")
    if depth > 1:
        assert st["zero_cover"] > 0 and st["dead"] > 0
    if d < depth:
        assert st["repeats"] > 0
    if (depth, d) == (5, 7):
        assert st["max_m"] == 5


def test_rows_exactly_on_thresholds(dev):
    ens, Xs, _ = PC.covered_tie_case()
    on = (Xs[:, np.maximum(ens.feat, 0)] == ens.thr[None]) & (ens.feat >= 0)[None]
    assert on.any()
    _check(dev, ens, Xs, "ties")


@pytest.fixture(scope="module")
def long_ensemble():
    """300 trees of depth 5 over 4 features with count covers; the tests take its first T trees."""
    d = 4
    ens = TC.random_ensemble(d, 5, 300, 970)
    Xs, Bs = TC.random_rows(d, 3, 40, 971)
    return PC.with_count_cover(ens, Bs), Xs


@pytest.mark.parametrize("T", [1, 118, 119, 300])
def test_tree_counts_and_both_memory_paths(dev, long_ensemble, T):
    """T* = 118 trees keep leaves, split features and fractions in LDS at d = 4, depth 5; T* + 1
    and 300 stream them from global memory."""
    full, Xs = long_ensemble
    Ts = PC.path_lds_boundary(4, 5)
    assert Ts == 118
    assert treeshap_path_lds_resident(4, Ts, 5) and not treeshap_path_lds_resident(4, Ts + 1, 5)
    assert treeshap_path_lds_resident(4, T, 5) == (T <= Ts)
    _check(dev, full.head(T), Xs, f"T {T}")


@pytest.mark.parametrize("depth,T", [(5, 66), (5, 67), (2, 2048)])
def test_widest_model(dev, depth, T):
    """d = 30 (the phi table's 30 KiB): both sides of its LDS boundary at depth 5 and the tree
    limit.  2^30 coalitions are out of reach: the oracle is the per-leaf form, which
    test_treeshap_path.py holds to brute force, plus efficiency."""
    assert PC.path_lds_boundary(30, 5) == 66
    assert treeshap_path_lds_resident(30, T, depth) == (T == 66)
    ens = TC.random_ensemble(30, depth, T, 980, p_pass=0.05)
    Xs, Bs = TC.random_rows(30, 2, 30, 981)
    ens = PC.with_count_cover(ens, Bs)
    st = PC.path_stats(Xs, ens)
    phi, fx, f0 = _explainer(ens, dev).explain(Xs)
    PC.assert_within(phi, st["phi"], PC.phi_bound(st["S"], T, depth), f"d 30 T {T} phi vs per-leaf reference")
    PC.assert_within(phi.sum(1), fx - f0, PC.efficiency_bound(st["S"], st["fx_abs"], st["f0_abs"], T, depth,
                                                             ens.base_margin), f"d 30 T {T} efficiency")


def test_nan_inputs_follow_default_left(dev):
    ens, Xs, Bs = PC.covered_case(4, 6)
    ens = PC.with_count_cover(PC.with_default_left(ens, 5), Bs)
    Xs = Xs.copy()
    Xs[0, 1] = np.nan
    Xs[1, :] = np.nan
    st, (phi, _, _) = _check(dev, ens, Xs, "NaN rows")
    assert st["nan_default_left"] > 0 and np.all(np.isfinite(phi))
    bad = PC.path_stats(Xs, ens, "ignore_default_left")["phi"]
    with pytest.raises(AssertionError, match="exceeds the derived bound"):
        PC.assert_within(bad, PC.brute_force(Xs, ens)[0], PC.phi_bound(st["S"], ens.n_trees, ens.depth),
                         "a walk that ignores default_left")


def test_no_rows_deterministic_and_async_form(dev):
    ens, Xs, _ = PC.covered_case(5, 7, E=4)
    te = _explainer(ens, dev)
    phi, fx, f0 = te.explain(Xs[:0])
    assert phi.shape == (0, 7) and fx.shape == (0,) and f0 == te.f0
    got = treeshap_path(torch.empty((0, 7), device=dev), te, sync=False)
    assert got[0].shape == (0, 7) and got[1].shape == (0,) and got[0].device.type == "cuda"
    Xd = torch.from_numpy(Xs).to(dev)
    phi, fx, f0 = treeshap_path(Xd, te)
    phi2, fx2, _ = treeshap_path(Xd, te)
    assert np.array_equal(phi, phi2) and np.array_equal(fx, fx2)
    out = (torch.full((4, 7), float("nan"), device=dev), torch.full((4,), float("nan"), device=dev),
           torch.full((6,), float("nan"), device=dev))
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        res = treeshap_path(Xd, te, sync=False, out=out)
    side.synchronize()
    assert all(g is o for g, o in zip(res, out))
    assert np.array_equal(out[0].cpu().numpy().astype(np.float64), phi)
    assert np.array_equal(out[1].cpu().numpy().astype(np.float64), fx)
    f0o = out[2].cpu().numpy()
    assert np.all(f0o[:4] == np.float32(te.f0)) and np.all(np.isnan(f0o[4:]))


def test_launcher_limits_raise_before_any_launch(dev):
    from fraud_detection_amd.ops.native import native, ptr, stream_of

    n = 2049 * 128
    z = torch.zeros(n, device=dev)
    zi = torch.zeros(n, device=dev, dtype=torch.int32)

    def launch(T=2, depth=2, d=2, ldx=32):
        native().treeshap_path(ptr(z), ldx, 1, d, ptr(zi), ptr(z), ptr(z), ptr(z), 0, T, depth, 0.0, 0.0, ptr(z),
                               ptr(z), ptr(z), stream_of(z))

    for kw, msg in (({"T": 2049}, "trees"), ({"T": 0}, "trees"), ({"depth": 6}, "depth"), ({"depth": 0}, "depth"),
                    ({"d": 31}, "d <= 30"), ({"d": 4, "ldx": 3}, "stride")):
        with pytest.raises(Exception, match=msg):
            launch(**kw)
    torch.cuda.synchronize(dev)
    ens, Xs, Bs = PC.covered_case(3, 3)
    with pytest.raises(ValueError):
        _explainer(PC.with_count_cover(TC.random_ensemble(3, 6, 2, 0), Bs), dev)


def test_device_equals_cpu_through_explainer_and_engine(dev, monkeypatch):
    from fraud_detection_amd.serve.engine import TreeInferenceEngine

    monkeypatch.setenv("FDX_HOST_MAX_ROWS", "0")
    ens, Xs, Bs = PC.covered_case(5, 7)
    d = 7
    mean, scale = np.full(d, 0.25), np.full(d, 2.0)
    X = (Xs * 2.0 + 0.25).astype(np.float32)
    rows = _standardize(X, mean, scale)
    st = PC.path_stats(rows, ens)
    pb = PC.phi_bound(st["S"], ens.n_trees, ens.depth)
    fb = PC.fx_bound(st["fx_abs"], ens.n_trees, ens.base_margin)
    cpu = TreePathExplainer(ens, mean, scale, device="cpu").explain(X)
    gpu = TreePathExplainer(ens, mean, scale, device=str(dev)).explain(X)
    PC.assert_within(gpu[0], cpu[0], pb, "explainer: device phi vs cpu")
    PC.assert_within(gpu[1], cpu[1], fb + ens.n_trees * TC.U * st["fx_abs"], "explainer: device fx vs cpu (fp32 sums)")
    assert gpu[2] == cpu[2]
    names = [f"f{i}" for i in range(d)]
    eng = TreeInferenceEngine(ens, mean, scale ** 2, scale, names, device=str(dev))
    assert not eng.has_background
    ex = eng.explain(X, "tree_path")
    assert (ex.method, ex.space) == ("tree_path", "log-odds")
    assert np.array_equal(ex.phi, gpu[0]) and np.array_equal(ex.logit, gpu[1]) and ex.base_value == cpu[2]
    with pytest.raises(ValueError, match="background"):
        eng.explain(X, "auto")


def test_classifier_records_cover_and_predicts_contribs(dev):
    from fraud_detection_amd.models.gbdt import GBDTClassifier
    from fraud_detection_amd.ops import gbdt as gb

    rng = np.random.default_rng(11)
    X = rng.normal(size=(2000, 6)).astype(np.float32)
    y = (X[:, 0] - 0.7 * X[:, 3] + 0.3 * rng.normal(size=2000) > 0.8).astype(np.uint8)
    kw = dict(n_estimators=8, max_depth=3, device=str(dev))
    plain = GBDTClassifier(**kw).fit(X, y)
    clf = GBDTClassifier(**kw).fit(X, y, record_cover=True)
    assert plain.ensemble.cover is None and clf.ensemble.cover_kind == "hessian"
    for a in ("feat", "bin", "thr", "gain", "leaf"):
        assert np.array_equal(getattr(plain.ensemble, a), getattr(clf.ensemble, a)), a
    ens = clf.ensemble
    q = gb.node_cover(torch.from_numpy(X).to(dev), ens, "hessian").cpu().numpy()
    assert np.array_equal(ens.cover, q / 2.0 ** 30)
    Xe = X[:48]
    contrib = clf.predict_contribs(Xe)
    assert contrib.shape == (48, 7)
    st = PC.path_stats(Xe, ens)
    T, D = ens.n_trees, ens.depth
    margin = clf.predict_margin(Xe).astype(np.float64)
    # the margin is gbdt_predict's fp32 sum in tree order: T additions of at most |base| + fx_abs
    bound = (PC.phi_bound(st["S"], T, D).sum(1) + PC.f0_bound(st["f0_abs"], T, D)
             + T * TC.U * (abs(ens.base_margin) + st["fx_abs"]))
    PC.assert_within(contrib.sum(1), margin, bound, "predict_contribs rows sum to predict_margin")
    PC.assert_within(contrib[:, :-1], st["phi"], PC.phi_bound(st["S"], T, D), "predict_contribs vs per-leaf form")
    k3 = clf.predict_contribs(Xe, iteration_range=(0, 3))
    st3 = PC.path_stats(Xe, ens.head(3))
    PC.assert_within(k3[:, :-1], st3["phi"], PC.phi_bound(st3["S"], 3, D), "first 3 trees")
    assert np.all(clf.feature_importance("total_cover") >= 0) and clf.feature_importance("cover").shape == (6,)
