"""GBDT reg_alpha / max_delta_step on the CPU path: the rules of ops/reference_gbdt.py checked on their
own (closed-form gain, the weight as a constrained minimiser in exact rational arithmetic, boundary
cases -- none of them through best_split), then whole fits: the two estimator-level properties, the
defaults, data parallelism, checkpoints, validation and serialisation."""
from __future__ import annotations

import json
import os
import pickle
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from fraud_detection_amd.models.gbdt import GBDTClassifier
from fraud_detection_amd.ops import gbdt as gb
from fraud_detection_amd.ops import reference_gbdt as R

TREE_KEYS = ("feat", "bin", "thr", "gain", "leaf")
INF = np.inf
U = 2.0 ** -53  # unit roundoff of fp64 (round to nearest)


def same_trees(a, b, keys=TREE_KEYS):
    return all(getattr(a, k).tobytes() == getattr(b, k).tobytes() for k in keys)


# ---- the rules, on their own -------------------------------------------------------------------------------
def _scale(G, H, lam, w, alpha):
    return abs(2.0 * G * w) + (H + lam) * w * w + 2.0 * alpha * abs(w)


def test_gain_equals_closed_form():
    """m = 0, no bounds: (term(L, wl) + term(R, wr)) - term(node, w) against
    T(GL)^2 / (HL + l) + T(GR)^2 / (HR + l) - T(G)^2 / (H + l), both in fp64.

    Tolerance, first order in u = 2^-53, per side with S = |2 G w| + (H + l) w^2 + 2 a |w| at the
    computed w.  Both expressions start from the same fp64 t = T(G) and dn = H + l.
      * the term: 2 G and 2 a are exact; 2 G w is rounded once and passes two additions (3 u), dn w w
        is rounded twice and passes two additions (4 u), 2 a |w| is rounded once and passes one
        addition (2 u): at most 4 u S.  The rounding of w = -t / dn itself does not count: w sits at
        the stationary point of the side's quadratic up to the rounding of t, so its effect is
        second order;
      * t is G -+ a rounded, t = tau (1 + delta): the objective's reduction at -t / dn is
        tau^2 (1 - delta^2) / dn while the closed form squares t, tau^2 (1 + delta)^2 / dn: 2 u t^2 / dn,
        and t^2 / dn = dn w^2 <= S;
      * the closed form's side: one product, one quotient, 2 u t^2 / dn <= 2 u S.
    That is 8 u S per side.  Each expression then adds two terms and subtracts the third: two
    roundings, each at most u (|tL| + |tR| + |tN|) <= u sum(S), for both expressions 4 u sum(S).
    tol = 12 u sum(S) from the count, taken as 13 u sum(S): the thirteenth unit stands for every
    second-order term.  Nothing here was fitted to the observed error."""
    rng = np.random.default_rng(0)
    worst = 0.0
    n_zero = 0
    for i in range(4000):
        lam = (0.0, 1.0, 10.0)[i % 3]
        alpha = float(rng.uniform(0.0, 3.0)) if i % 5 else 0.0
        GL, GR = (float(v) for v in rng.normal(0.0, 4.0, 2))
        HL, HR = (float(v) for v in rng.uniform(0.05, 20.0, 2))
        G, H = GL + GR, HL + HR  # the node's sums: any fp64 pair will do, the identity is per term
        reg = (alpha, 0.0)
        w = [R.mono_weight(g, h, lam, 0.0, -INF, INF, reg) for g, h in ((GL, HL), (GR, HR), (G, H))]
        t = [R.mono_term(g, h, lam, wi, reg) for (g, h), wi in zip(((GL, HL), (GR, HR), (G, H)), w)]
        gain = (t[0] + t[1]) - t[2]
        T = [R.soft_threshold(g, alpha) for g in (GL, GR, G)]
        n_zero += sum(1 for v in T if v == 0.0)
        closed = (T[0] * T[0] / (HL + lam) + T[1] * T[1] / (HR + lam)) - T[2] * T[2] / (H + lam)
        S = sum(_scale(g, h, lam, wi, alpha) for (g, h), wi in zip(((GL, HL), (GR, HR), (G, H)), w))
        tol = 13.0 * U * S
        err = abs(gain - closed)
        if i < 5:
            print(f"case {i}: |gain - closed| = {err:.3e}, tol = {tol:.3e}")
        assert err <= tol, (i, gain, closed, err, tol)
        worst = max(worst, err / tol if tol else 0.0)
    assert n_zero > 100  # sides inside [-alpha, alpha] took part
    print(f"largest |gain - closed| / tol = {worst:.3f}")


def _objective(G, H, lam, alpha, w):
    """G w + (H + lam) w^2 / 2 + alpha |w| in exact rational arithmetic."""
    G, H, lam, alpha, w = (Fraction(float(v)) for v in (G, H, lam, alpha, w))
    return G * w + (H + lam) * w * w / 2 + alpha * abs(w)


def _grid(rng, lo, hi, size=None):
    """Multiples of 2^-10 in [lo, hi]: sums and differences of two of them below 2^20 are exact, so
    T(G) and H + lam carry no rounding and the weight is the correctly rounded -T / (H + lam)."""
    return rng.integers(int(lo * 1024), int(hi * 1024) + 1, size) / 1024.0


def test_weight_minimises_the_objective_over_the_interval():
    """Where the bounds meet [-m, m] the weight is the minimiser of the regularised objective over
    [max(lo, -m), min(hi, m)]: no fp64 neighbour inside the interval and neither end does better,
    the objective evaluated exactly (fractions).  With the inputs on a grid the unclamped weight is
    the correctly rounded stationary point, the nearest fp64 to the vertex of a parabola, so the
    comparison with its neighbours holds exactly and needs no tolerance."""
    rng = np.random.default_rng(1)
    seen = {"free": 0, "cap": 0, "bound": 0, "zero": 0}
    for i in range(3000):
        lam = float((0.0, 1.0, 4.0)[i % 3])
        G, H = float(_grid(rng, -8.0, 8.0)), float(_grid(rng, 0.25, 16.0))
        alpha = float(_grid(rng, 0.0, 4.0)) if i % 4 else 0.0
        m = float(rng.uniform(0.01, 2.0)) if i % 3 else 0.0
        cap = m if m > 0.0 else INF
        kind = i % 5
        lo, hi = -INF, INF
        if kind in (1, 3):
            lo = float(rng.uniform(-cap if m else -2.0, cap if m else 2.0))
        if kind in (2, 3):
            hi = float(rng.uniform(max(lo, -cap) if np.isfinite(lo) else (-cap if m else -2.0), cap if m else 2.0))
        a, b = max(lo, -cap), min(hi, cap)
        assert a <= b
        w = R.mono_weight(G, H, lam, 0.0, lo, hi, (alpha, m))
        assert a <= w <= b
        f_w = _objective(G, H, lam, alpha, w)
        others = [x for x in (np.nextafter(w, -INF), np.nextafter(w, INF)) if a <= x <= b]
        others += [x for x in (a, b) if np.isfinite(x)]
        for x in others:
            assert f_w <= _objective(G, H, lam, alpha, x), (i, G, H, lam, alpha, m, lo, hi, w, x)
        free = R.mono_weight(G, H, lam, 0.0, -INF, INF, (alpha, 0.0))
        seen["zero"] += int(w == 0.0 and abs(G) <= alpha)
        seen["free"] += int(w == free and w != 0.0)
        seen["cap"] += int(m > 0.0 and abs(w) == m and abs(free) > m)
        seen["bound"] += int(w in (lo, hi) and w != free)
    assert all(v > 50 for v in seen.values()), seen


def test_clamp_order_when_a_bound_lies_outside_the_cap():
    """lo > m or hi < -m: [max(lo, -m), min(hi, m)] is empty and the written order decides -- the cap
    first, the monotone clamp last, so the weight is the bound itself (xgboost's CalcWeight, then
    the evaluator's bounds)."""
    rng = np.random.default_rng(2)
    for i in range(500):
        G, H = float(rng.normal(0.0, 4.0)), float(rng.uniform(0.1, 10.0))
        alpha, m = float(rng.uniform(0.0, 2.0)), float(rng.uniform(0.01, 1.0))
        out = m * float(rng.uniform(1.01, 3.0))
        assert R.mono_weight(G, H, 1.0, 0.0, out, out + 1.0, (alpha, m)) == out        # lo above the cap
        assert R.mono_weight(G, H, 1.0, 0.0, out, INF, (alpha, m)) == out
        assert R.mono_weight(G, H, 1.0, 0.0, -out - 1.0, -out, (alpha, m)) == -out     # hi below -cap
        assert R.mono_weight(G, H, 1.0, 0.0, -INF, -out, (alpha, m)) == -out
        # and the vector form, which the scan uses, agrees bit for bit
        v = R._mono_weight_v(np.array([G]), np.array([H]), 1.0, 0.0, out, INF, (alpha, m))
        assert v[0] == out


def test_boundary_cases():
    free = (-INF, INF)
    for alpha in (0.5, 3.0):
        for G in (alpha, -alpha, 0.0, np.nextafter(alpha, 0.0)):
            w = R.mono_weight(G, 2.0, 1.0, 1.0, *free, (alpha, 0.0))
            assert w == 0.0 and R.mono_term(G, 2.0, 1.0, w, (alpha, 0.0)) == 0.0
        assert R.mono_weight(np.nextafter(alpha, INF), 2.0, 1.0, 1.0, *free, (alpha, 0.0)) < 0.0
        assert R.mono_weight(np.nextafter(-alpha, -INF), 2.0, 1.0, 1.0, *free, (alpha, 0.0)) > 0.0
    # |w| == m exactly: T = -2, H + lam = 4, w = 0.5 = m is left alone; one ulp more is capped to m
    assert R.mono_weight(-2.5, 3.0, 1.0, 1.0, *free, (0.5, 0.5)) == 0.5
    assert R.mono_weight(2.5, 3.0, 1.0, 1.0, *free, (0.5, 0.5)) == -0.5
    assert R.mono_weight(-2.5, 3.0, 1.0, 1.0, *free, (0.5, 0.0)) == 0.5
    assert R.mono_weight(np.nextafter(-2.5, -INF), 3.0, 1.0, 1.0, *free, (0.5, 0.0)) > 0.5
    assert R.mono_weight(np.nextafter(-2.5, -INF), 3.0, 1.0, 1.0, *free, (0.5, 0.5)) == 0.5
    assert R.mono_weight(-2.5, 3.0, 1.0, 1.0, *free, (0.5, np.nextafter(0.5, 0.0))) == np.nextafter(0.5, 0.0)
    # H < min_child_weight (and H <= 0): 0 whatever G is, then only the monotone clamp
    for reg in ((0.0, 0.0), (0.5, 0.0), (0.0, 0.25), (0.5, 0.25)):
        assert R.mono_weight(-100.0, 0.999, 1.0, 1.0, *free, reg) == 0.0
        assert R.mono_weight(-100.0, 0.0, 1.0, 0.0, *free, reg) == 0.0
        assert R.mono_weight(-100.0, 0.999, 1.0, 1.0, 0.125, INF, reg) == 0.125
        assert R.mono_weight(-100.0, 1.0, 1.0, 1.0, *free, reg) != 0.0
    # the vector forms are the scalar ones, bit for bit
    rng = np.random.default_rng(3)
    G, H = rng.normal(0.0, 3.0, 200), rng.uniform(0.0, 5.0, 200)
    for reg in ((0.7, 0.0), (0.0, 0.3), (0.7, 0.3)):
        for lo, hi in (free, (-0.2, 0.1)):
            wv = R._mono_weight_v(G, H, 1.0, 1.0, lo, hi, reg)
            ws = np.array([R.mono_weight(float(g), float(h), 1.0, 1.0, lo, hi, reg) for g, h in zip(G, H)])
            assert wv.tobytes() == ws.tobytes()
            tv = R._mono_term_v(G, H, 1.0, wv, reg)
            ts = np.array([R.mono_term(float(g), float(h), 1.0, float(w), reg) for g, h, w in zip(G, H, ws)])
            assert tv.tobytes() == ts.tobytes()


def test_reg_none_is_the_old_arithmetic():
    rng = np.random.default_rng(4)
    H = np.zeros((5, 256, 2), np.int64)
    H[:, :40, 0] = rng.integers(-(1 << 18), 1 << 18, (5, 40))
    H[:, :40, 1] = rng.integers(0, 1 << 18, (5, 40))
    H[1:, :, :] = H[0][rng.permutation(256)][None]  # every feature the same totals
    nb = np.full(5, 256, np.int32)
    gi, hi = 1.0 / 16384, 1.0 / 65536
    a = R.best_split(H, nb, gi, hi, 1.0, 1.0)
    assert a == R.best_split(H, nb, gi, hi, 1.0, 1.0, reg=None)
    mono = (np.array([1, -1, 0, 0, 1]), -0.5, 0.25)
    assert R.best_split(H, nb, gi, hi, 1.0, 1.0, mono=mono) == R.best_split(H, nb, gi, hi, 1.0, 1.0, mono=mono, reg=None)
    assert R.best_split(H, nb, gi, hi, 1.0, 1.0, reg=(0.25, 0.0))[0] < a[0]  # L1 only takes gain away


# ---- whole fits ----------------------------------------------------------------------------------------------
N, D = 2000, 6
FIT_KW = dict(n_estimators=4, max_depth=3, max_bin=32, learning_rate=0.3)
REG_KW = dict(reg_alpha=1.5, max_delta_step=0.4)


def fixture_data(n=N, seed=7):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, D)).astype(np.float32)
    z = 1.4 * X[:, 0] - 1.1 * X[:, 1] + 0.8 * X[:, 2] * X[:, 3] + 0.5 * rng.normal(size=n)
    y = (z > np.quantile(z, 0.93)).astype(np.uint8)  # 7 % positives
    return X, y


@pytest.fixture(scope="module")
def fits():
    X, y = fixture_data()
    Xt, yt = torch.from_numpy(X), torch.from_numpy(y)
    return X, y, gb.fit(Xt, yt, gb.GBDTParams(**FIT_KW)), gb.fit(Xt, yt, gb.GBDTParams(**FIT_KW, **REG_KW))


def replay(X, y, ens, p: gb.GBDTParams):
    """The fit again, one R.build_tree per round on the ensemble's own cuts: yields (round, tree,
    leaf index per row, quantised gradients, (ginv, hinv)) and checks that the ensemble is that tree."""
    bins = R.bin_rows(X, ens.cuts, ens.nbins)
    gs, hs = R.grad_scales(p.scale_pos_weight)
    margin = np.full(X.shape[0], np.float32(np.log(p.base_score / (1.0 - p.base_score))), np.float32)
    for t in range(ens.feat.shape[0]):
        q = R.gradients(margin, y, p.scale_pos_weight, gs, hs)
        tr, node = R.build_tree(bins, q, ens.cuts, ens.nbins, p.max_depth, p.reg_lambda, p.min_child_weight, p.gamma,
                                p.learning_rate, gs, hs, reg=p.reg)
        assert all(getattr(tr, k).tobytes() == getattr(ens, k)[t].tobytes() for k in TREE_KEYS)
        yield t, tr, node, q, (1.0 / gs, 1.0 / hs)
        margin = (margin + tr.leaf[node]).astype(np.float32)


def test_regularised_fit_differs_and_names_its_parameters(fits):
    X, y, plain, reg = fits
    assert not same_trees(plain, reg)
    assert reg.params["reg_alpha"] == 1.5 and reg.params["max_delta_step"] == 0.4
    assert (plain.feat >= 0).any() and (reg.feat >= 0).any()
    p = gb.GBDTParams(**FIT_KW, **REG_KW)
    assert sum(1 for _ in replay(X, y, reg, p)) == 4
    for only in ({"reg_alpha": 1.5}, {"max_delta_step": 0.4}):
        one = gb.fit(torch.from_numpy(X), torch.from_numpy(y), gb.GBDTParams(**FIT_KW, **only))
        assert not same_trees(one, plain) and not same_trees(one, reg)
        assert set(one.params) - set(plain.params) == set(only)


@pytest.mark.parametrize("spw", [1.0, 13.0])
def test_large_alpha_leaves_every_tree_empty(spw):
    """alpha >= 2 n max(scale_pos_weight, 1) exceeds every node's |G| (|g_i| <= w_eff): T(G) = 0 at every
    node, no candidate gains, every leaf is exactly 0 and every margin the base margin."""
    X, y = fixture_data()
    alpha = 2.0 * N * max(spw, 1.0)
    clf = GBDTClassifier(device="cpu", scale_pos_weight=spw, base_score=0.3, reg_alpha=alpha, **FIT_KW).fit(X, y)
    ens = clf.ensemble
    assert np.all(ens.feat == -1) and np.all(ens.gain == 0.0)
    assert np.all(ens.leaf == 0.0)
    assert np.all(clf.predict_margin(X) == np.float32(np.log(0.3 / 0.7)))
    assert ens.params["reg_alpha"] == alpha and "max_delta_step" not in ens.params


def test_leaf_bound_and_its_coverage():
    """|leaf| <= float32(eta m); with m = 1e-3 the cap is at work in every tree: the oracle's
    unclamped weight of at least one leaf per tree lies above m."""
    X, y = fixture_data()
    for m_, eta in ((1e-3, 0.3), (0.05, 1.0), (0.4, 0.3)):
        p = gb.GBDTParams(**{**FIT_KW, "learning_rate": eta}, max_delta_step=m_)
        ens = gb.fit(torch.from_numpy(X), torch.from_numpy(y), p)
        assert np.all(np.abs(ens.leaf) <= np.float32(eta * m_))
        for t, tr, node, q, (ginv, hinv) in replay(X, y, ens, p):
            over = 0
            for leaf in range(1 << p.max_depth):
                G, H = float(q[node == leaf, 0].sum()) * ginv, float(q[node == leaf, 1].sum()) * hinv
                w = R.mono_weight(G, H, p.reg_lambda, p.min_child_weight, -INF, INF, (0.0, 0.0))
                over += int(abs(w) > m_)
                if abs(w) > m_:
                    assert tr.leaf[leaf] == np.float32(eta * np.copysign(m_, w))
            if m_ == 1e-3:
                assert over >= 1, t


def test_defaults_are_the_fit_as_it_is(fits):
    X, y, plain, _ = fits
    Xt, yt = torch.from_numpy(X), torch.from_numpy(y)
    for kw in (dict(reg_alpha=0, max_delta_step=0), dict(reg_alpha=0.0), dict(max_delta_step=0.0),
               dict(reg_alpha=-0.0, max_delta_step=0.0)):
        zero = gb.fit(Xt, yt, gb.GBDTParams(**FIT_KW, **kw))
        assert zero.to_dict() == plain.to_dict()
    assert "reg_alpha" not in plain.params and "max_delta_step" not in plain.params
    a = GBDTClassifier(device="cpu", **FIT_KW).fit(X, y)
    b = GBDTClassifier(device="cpu", reg_alpha=0, max_delta_step=0, **FIT_KW).fit(X, y)
    assert a.ensemble.to_dict() == b.ensemble.to_dict() == plain.to_dict()
    assert a.get_params()["reg_alpha"] == 0.0 and a.get_params()["max_delta_step"] == 0.0


def test_classifier_no_longer_swallows_the_arguments(fits):
    X, y, plain, reg = fits
    clf = GBDTClassifier(device="cpu", **FIT_KW, **REG_KW).fit(X, y)
    assert same_trees(clf.ensemble, reg) and not same_trees(clf.ensemble, plain)
    assert clf.get_params()["reg_alpha"] == 1.5 and clf.get_params()["max_delta_step"] == 0.4
    # xgboost-only knobs the reference passes are still accepted and ignored
    ign = GBDTClassifier(device="cpu", objective="binary:logistic", n_jobs=-1, **FIT_KW).fit(X, y)
    assert ign.ensemble.to_dict() == plain.to_dict()
    both = GBDTClassifier(device="cpu", objective="binary:logistic", n_jobs=4, **FIT_KW, **REG_KW).fit(X, y)
    assert same_trees(both.ensemble, reg)


@pytest.mark.parametrize("name", ["reg_alpha", "max_delta_step"])
@pytest.mark.parametrize("bad", [-1.0, -1e-300, float("nan"), float("inf"), float("-inf")], ids=str)
def test_bad_values_raise(name, bad):
    with pytest.raises(ValueError, match=f"{name} must be finite and >= 0"):
        gb.GBDTParams(**{name: bad}).validate()
    X, y = fixture_data(64)
    with pytest.raises(ValueError, match=name):
        GBDTClassifier(device="cpu", n_estimators=1, max_depth=1, **{name: bad}).fit(X, y)


def test_json_and_pickle_round_trip(tmp_path, fits):
    X, y, plain, reg = fits
    clf = GBDTClassifier(device="cpu", **FIT_KW, **REG_KW).fit(X, y)
    want = clf.predict_margin(X)
    path = str(tmp_path / "m.json")
    clf.save_model(path)
    with open(path) as f:
        o = json.load(f)
    assert o["params"]["reg_alpha"] == 1.5 and o["params"]["max_delta_step"] == 0.4
    assert set(o) == set(plain.to_dict()) | {"feature_names"}  # a regularised tree is an ordinary tree
    back = GBDTClassifier.load_model(path, device="cpu")
    assert back.get_params()["reg_alpha"] == 1.5 and back.get_params()["max_delta_step"] == 0.4
    assert same_trees(back.ensemble, reg) and np.array_equal(back.predict_margin(X), want)
    assert same_trees(back.fit(X, y).ensemble, reg)  # the loaded estimator refits regularised
    again = pickle.loads(pickle.dumps(clf))
    assert again.get_params()["reg_alpha"] == 1.5 and np.array_equal(again.predict_margin(X), want)
    assert same_trees(again.fit(X, y).ensemble, reg)
    # a default model serialises as it always did
    p2 = str(tmp_path / "p.json")
    GBDTClassifier(device="cpu", **FIT_KW).fit(X, y).save_model(p2)
    with open(p2) as f:
        assert not {"reg_alpha", "max_delta_step"} & set(json.load(f)["params"])
    assert GBDTClassifier.load_model(p2, device="cpu").get_params()["reg_alpha"] == 0.0


# ---- checkpoints -----------------------------------------------------------------------------------------------
class _Recorder:
    """A checkpoint manager's interface that records the signatures a fit asks for."""

    def __init__(self):
        self.sigs = []

    def latest(self, sig):
        self.sigs.append(sig)
        return None

    def save(self, step, tensors, meta):
        self.sigs.append(meta["signature"])


def test_checkpoint_signature_names_them_only_off_their_defaults():
    from fraud_detection_amd.utils.checkpoint import config_signature

    X, y = fixture_data(600)
    Xt, yt = torch.from_numpy(X), torch.from_numpy(y)
    kw = dict(n_estimators=2, max_depth=2, max_bin=8)
    cuts = gb.quantile_cuts(Xt, 8)

    def sig_of(**extra):
        rec = _Recorder()
        gb.fit(Xt, yt, gb.GBDTParams(**kw, **extra), cuts=cuts, checkpoint=rec, checkpoint_every=2)
        assert len(set(rec.sigs)) == 1
        return rec.sigs[0]

    # the signature of a fit from before the two fields existed: spelled out, not read from the class
    old = {"learning_rate": 0.1, "max_depth": 2, "reg_lambda": 1.0, "min_child_weight": 1.0, "gamma": 0.0,
           "max_bin": 8, "scale_pos_weight": 1.0, "base_score": 0.5, "cut_sample_rows": 1 << 20}
    want = config_signature(params=old, spw=1.0, cuts=cuts[0], nbins=cuts[1], n=600, d=D)
    assert sig_of() == want == sig_of(reg_alpha=0.0, max_delta_step=0.0) == sig_of(reg_alpha=0)
    a = sig_of(reg_alpha=0.5)
    m = sig_of(max_delta_step=0.5)
    both = sig_of(reg_alpha=0.5, max_delta_step=0.5)
    assert len({want, a, m, both, sig_of(reg_alpha=0.25)}) == 5


def test_checkpoint_resume_equals_uninterrupted(tmp_path):
    from fraud_detection_amd.utils.checkpoint import CheckpointManager

    X, y = fixture_data()
    Xt, yt = torch.from_numpy(X), torch.from_numpy(y)
    kw = dict(max_depth=3, max_bin=32, learning_rate=0.3, **REG_KW)
    full = gb.fit(Xt, yt, gb.GBDTParams(n_estimators=6, **kw))
    mgr = CheckpointManager(str(tmp_path), prefix="g")
    gb.fit(Xt, yt, gb.GBDTParams(n_estimators=3, **kw), checkpoint=mgr, checkpoint_every=3)
    saved = []
    save = mgr.save
    mgr.save = lambda step, *a, **k: (saved.append(step), save(step, *a, **k))[1]
    res = gb.fit(Xt, yt, gb.GBDTParams(n_estimators=6, **kw), checkpoint=mgr, checkpoint_every=1)
    assert saved == [4, 5, 6]
    assert same_trees(res, full)
    # the two values are part of the signature: a fit with others does not pick these trees up
    for other_kw in ({**kw, "reg_alpha": 0.5}, {**kw, "max_delta_step": 0.0}, {**kw, "reg_alpha": 0.0, "max_delta_step": 0.0}):
        saved.clear()
        other = gb.fit(Xt, yt, gb.GBDTParams(n_estimators=6, **other_kw), checkpoint=mgr, checkpoint_every=6)
        assert saved == [6]
        assert same_trees(other, gb.fit(Xt, yt, gb.GBDTParams(n_estimators=6, **other_kw)))
        assert not same_trees(other, full)


# ---- composition on the CPU path ---------------------------------------------------------------------------------
def test_composes_with_everything_on_the_cpu_path():
    """Sampling, weights, learned missing directions, monotone and interaction constraints, an eval
    set with early stopping and the row hole, all at once: the fit runs, respects the leaf bound and
    a fold around a hole equals the fit on the kept rows."""
    X, y = fixture_data()
    rng = np.random.default_rng(11)
    Xn = X.copy()
    Xn[rng.random(N) < 0.1, 0] = np.nan
    w = torch.from_numpy(rng.uniform(0.25, 2.0, N).astype(np.float32))
    Xt, yt = torch.from_numpy(Xn), torch.from_numpy(y)
    p = gb.GBDTParams(missing_policy="learn", subsample=0.8, colsample_bynode=0.5, seed=3,
                      monotone_constraints=(1, -1, 0, 0, 0, 0), interaction_constraints=[[0, 1], [2, 3, 4]],
                      reg_alpha=0.5, max_delta_step=0.2, **{**FIT_KW, "n_estimators": 12})
    ens, rec = gb.fit(Xt, yt, p, sample_weight=w, eval_set=(Xt[:500], yt[:500]), early_stopping_rounds=3)
    assert ens.n_trees == rec.best_iteration + 1
    assert np.all(np.abs(ens.leaf) <= np.float32(0.3 * 0.2)) and (ens.feat >= 0).any()
    free = gb.fit(Xt, yt, gb.GBDTParams(**{**p.__dict__, "reg_alpha": 0.0, "max_delta_step": 0.0}), sample_weight=w)
    assert not same_trees(free, gb.fit(Xt, yt, p, sample_weight=w))
    cuts = gb.quantile_cuts(Xt, 32, missing=True)
    bins = gb.bin_rows(Xt, cuts[0], cuts[1], missing=True)
    q = gb.GBDTParams(**{**p.__dict__, "subsample": 1.0})
    hole = gb.fit_binned(bins, yt, cuts, q, hole=(300, 450))
    keep = np.r_[0:300, 750:N]
    assert same_trees(hole, gb.fit_binned(bins[keep].contiguous(), yt[keep].contiguous(), cuts, q))


def test_pipeline_and_cv_job_params_carry_them():
    """GBDTPipeline and DeviceGBDTCV copy their GBDTParams field by field: the two fields are fields."""
    p = gb.GBDTParams(**FIT_KW, **REG_KW)
    q = gb.GBDTParams(**{**p.__dict__, "scale_pos_weight": 3.0})
    assert (q.reg_alpha, q.max_delta_step) == (1.5, 0.4) and q.reg == (1.5, 0.4)
    assert gb.GBDTParams().reg is None and gb.GBDTParams(max_delta_step=1).reg == (0.0, 1.0)


def test_train_flags():
    from fraud_detection_amd import train

    import inspect

    sig = inspect.signature(train.run)
    assert sig.parameters["gbdt_reg_alpha"].default == 0.0 and sig.parameters["gbdt_max_delta_step"].default == 0.0
    src = inspect.getsource(train.main)
    assert "--gbdt-reg-alpha" in src and "--gbdt-max-delta-step" in src


# ---- data parallelism ----------------------------------------------------------------------------------------------
DP_KW = dict(**FIT_KW, **REG_KW, monotone_constraints=(1, -1, 0, 0, 0, 0))


def _dp_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    from fraud_detection_amd.parallel.comm import Communicator

    comm = Communicator(backend="gloo")
    X, y = fixture_data()
    sh = slice(0, 1001) if rank == 0 else slice(1001, N)
    ens = gb.fit(torch.from_numpy(X[sh].copy()), torch.from_numpy(y[sh].copy()), gb.GBDTParams(**DP_KW), comm=comm)
    np.savez(os.path.join(out_dir, f"m{rank}.npz"), **{k: getattr(ens, k) for k in TREE_KEYS}, cuts=ens.cuts)
    comm.close()


def test_dp_equals_single_process(tmp_path):
    """The histograms are all-reduced before the scan: every rank computes the same weights."""
    from test_distributed import _free_port

    mp.start_processes(_dp_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, start_method="spawn")
    X, y = fixture_data()
    ref = gb.fit(torch.from_numpy(X), torch.from_numpy(y), gb.GBDTParams(**DP_KW))
    assert not same_trees(ref, gb.fit(torch.from_numpy(X), torch.from_numpy(y),
                                      gb.GBDTParams(**{**DP_KW, "reg_alpha": 0.0, "max_delta_step": 0.0})))
    for r in range(2):
        o = np.load(os.path.join(tmp_path, f"m{r}.npz"))
        assert np.array_equal(o["cuts"], ref.cuts)
        assert all(o[k].tobytes() == getattr(ref, k).tobytes() for k in TREE_KEYS)
