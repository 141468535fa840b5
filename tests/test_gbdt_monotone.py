"""GBDT monotone constraints (xgboost's monotone_constraints), CPU side: the numpy oracle
(ops/reference_gbdt.py) against an independent row-level brute force, the exact monotonicity of the
fitted margins, the parameter forms, serialisation and checkpoint resume."""
from __future__ import annotations

import json
import os
import pickle

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from fraud_detection_amd.models.gbdt import GBDTClassifier
from fraud_detection_amd.ops import gbdt as gb
from fraud_detection_amd.ops import reference_gbdt as R

TREE_KEYS = ("feat", "bin", "thr", "gain", "leaf")
CONS = (1, -1, 0, 0)
FIT_KW = dict(n_estimators=20, max_depth=3, max_bin=16, learning_rate=0.3)


def same_trees(a, b, keys=TREE_KEYS):
    return all(getattr(a, k).tobytes() == getattr(b, k).tobytes() for k in keys)


def fixture_data():
    rng = np.random.default_rng(5)
    X = rng.normal(size=(600, 4)).astype(np.float32)
    p = 1.0 / (1.0 + np.exp(-(2.5 * np.sin(2.0 * X[:, 0]) - 1.5 * X[:, 1] + 0.8 * X[:, 2] * X[:, 0])))
    y = (rng.random(600) < p).astype(np.uint8)
    return X, y


def sweep_grid(cuts_f: np.ndarray) -> np.ndarray:
    """Every cut, the fp32 value just below every cut, and +-10, ascending."""
    cuts_f = np.asarray(cuts_f, np.float32)
    return np.unique(np.concatenate([cuts_f, np.nextafter(cuts_f, np.float32(-np.inf)), np.float32([-10.0, 10.0])]))


def sweep_steps(predict, X: np.ndarray, cuts: np.ndarray, nbins: np.ndarray, f: int, rows: int = 64) -> np.ndarray:
    """fp32 margin differences between adjacent grid values of feature f, [rows, len(grid) - 1], for
    the first ``rows`` rows of X with feature f swept over sweep_grid.  ``predict``: rows -> margins."""
    grid = sweep_grid(cuts[f, : int(nbins[f]) - 1])
    base = np.asarray(X[:rows], np.float32)
    tab = np.repeat(base, len(grid), 0)
    tab[:, f] = np.tile(grid, base.shape[0])
    m = np.asarray(predict(tab), np.float32).reshape(base.shape[0], len(grid))
    return m[:, 1:] - m[:, :-1]


def violations(predict, X, cuts, nbins, cons) -> dict:
    """feature -> (count of adjacent grid steps that move the wrong way, the worst step)."""
    out = {}
    for f, c in enumerate(cons):
        if c:
            step = sweep_steps(predict, X, cuts, nbins, f) * np.float32(c)
            out[f] = (int((step < 0).sum()), float(step.min()))
    return out


def ens_predict(ens):
    return lambda rows: gb.predict_margin(torch.from_numpy(np.ascontiguousarray(rows)), ens).numpy()


@pytest.fixture(scope="module")
def fits():
    X, y = fixture_data()
    Xt, yt = torch.from_numpy(X), torch.from_numpy(y)
    free = gb.fit(Xt, yt, gb.GBDTParams(**FIT_KW))
    mono = gb.fit(Xt, yt, gb.GBDTParams(monotone_constraints=CONS, **FIT_KW))
    return X, y, free, mono


# ---- the guarantee ------------------------------------------------------------------------------------
def test_constrained_fit_is_monotone_and_not_vacuous(fits):
    X, _, free, mono = fits
    v = violations(ens_predict(mono), X, mono.cuts, mono.nbins, CONS)
    print("constrained:", v)
    assert v[0][0] == 0 and v[1][0] == 0, v
    # the guarantee is not vacuous: the constrained features are still split on
    assert int((mono.feat == 0).sum()) >= 1 and int((mono.feat == 1).sum()) >= 1
    assert mono.params["monotone_constraints"] == list(CONS)


def test_unconstrained_fit_violates(fits):
    """The data can show a failure: without constraints both features move the wrong way somewhere."""
    X, _, free, _ = fits
    v = violations(ens_predict(free), X, free.cuts, free.nbins, CONS)
    print("unconstrained:", v)
    assert v[0][0] > 0 and v[1][0] > 0, v
    assert "monotone_constraints" not in free.params


def test_classifier_takes_the_constraints(fits):
    X, y, _, mono = fits
    clf = GBDTClassifier(monotone_constraints=CONS, device="cpu", **FIT_KW).fit(X, y)
    assert clf.get_params()["monotone_constraints"] == CONS
    assert same_trees(clf.ensemble, mono)
    v = violations(clf.predict_margin, X, clf.ensemble.cuts, clf.ensemble.nbins, CONS)
    assert v[0][0] == 0 and v[1][0] == 0, v


# ---- the oracle against a brute force over the rows ---------------------------------------------------
def _brute_tree(bins, q, nbins, depth, lam, mcw, gamma, eta, ginv, hinv, cons, missing):
    """No histograms and no cumsum: per node, per feature, per cut (and direction) the sums over the
    node's rows, then the documented weight / term / gain expressions on Python floats.  Candidates
    are tried in tie order and replaced only by a strictly larger gain."""
    n, d = bins.shape[0], len(nbins)
    ni = (1 << depth) - 1
    feat, binv, dleft, gain = np.full(ni, -1), np.full(ni, 255), np.zeros(ni, np.uint8), np.zeros(ni)
    sums, rows_of, bounds = {}, {0: np.arange(n)}, {0: (-np.inf, np.inf)}
    g, h = q[:, 0].astype(np.int64), q[:, 1].astype(np.int64)

    def weight(Gq, Hq, lo, hi):
        G, H = float(Gq) * ginv, float(Hq) * hinv
        w = 0.0 if (H < mcw or H <= 0.0) else -G / (H + lam)
        return lo if w < lo else (hi if w > hi else w)

    def term(Gq, Hq, w):
        G, H = float(Gq) * ginv, float(Hq) * hinv
        return -(2.0 * G * w + (H + lam) * w * w) if H + lam > 0.0 else 0.0

    for node in range(ni):
        rows = rows_of[node]
        lo, hi = bounds[node]
        Gq, Hq = int(g[rows].sum()), int(h[rows].sum())
        if node == 0:
            sums[0] = (Gq, Hq)
        root = term(Gq, Hq, weight(Gq, Hq, lo, hi))
        best = (-np.inf, None)
        for f in range(d):
            v = bins[rows, f].astype(np.int64)
            miss = (v == 255) if missing else np.zeros(len(rows), bool)
            cands = [(-1, 1, miss)] if missing else []
            for b in range(int(nbins[f]) - 1):
                cands.append((b, 0, (v <= b) & ~miss))
                if missing:
                    cands.append((b, 1, (v <= b) | miss))
            for b, dl, left in cands:
                GLq, HLq = int(g[rows][left].sum()), int(h[rows][left].sum())
                if not (float(HLq) * hinv >= mcw and float(Hq - HLq) * hinv >= mcw):
                    continue
                wl, wr = weight(GLq, HLq, lo, hi), weight(Gq - GLq, Hq - HLq, lo, hi)
                if (cons[f] > 0 and not wl <= wr) or (cons[f] < 0 and not wl >= wr):
                    continue
                gn = (term(GLq, HLq, wl) + term(Gq - GLq, Hq - HLq, wr)) - root
                if gn > best[0]:
                    best = (gn, (f, b, dl, left, GLq, HLq, wl, wr))
        lc, rc = 2 * node + 1, 2 * node + 2
        bounds[lc] = bounds[rc] = (lo, hi)
        if best[1] is not None and best[0] > 1e-6 and not best[0] < gamma:
            f, b, dl, left, GLq, HLq, wl, wr = best[1]
            feat[node], binv[node], dleft[node], gain[node] = f, b, dl, best[0]
            rows_of[lc], rows_of[rc] = rows[left], rows[~left]
            sums[lc], sums[rc] = (GLq, HLq), (Gq - GLq, Hq - HLq)
            mid = (wl + wr) / 2.0
            if cons[f] > 0:
                bounds[lc], bounds[rc] = (lo, mid), (mid, hi)
            elif cons[f] < 0:
                bounds[lc], bounds[rc] = (mid, hi), (lo, mid)
        else:
            rows_of[lc], rows_of[rc] = rows, rows[:0]
            sums[lc], sums[rc] = (Gq, Hq), (0, 0)
    leaf = np.zeros(1 << depth, np.float32)
    where = np.zeros(n, np.int64)
    for i in range(1 << depth):
        leaf[i] = np.float32(eta * weight(*sums[ni + i], *bounds[ni + i]))
        where[rows_of[ni + i]] = i
    return feat, binv, dleft, gain, leaf, where


BRUTE_CONS = {"up_down": (1, -1, 0), "down_up": (-1, 1, 0), "all_up": (1, 1, 1), "all_down": (-1, -1, -1)}


@pytest.mark.parametrize("missing", [False, True], ids=["plain", "missing"])
@pytest.mark.parametrize("reg", [(0.0, 0.0, 0.0), (1.0, 1.0, 0.0), (1.0, 0.0, 0.5), (2.5, 1.0, 0.0)],
                         ids=lambda r: "l%g_w%g_g%g" % r)
@pytest.mark.parametrize("cons", list(BRUTE_CONS))
def test_build_tree_matches_row_brute_force(cons, reg, missing):
    lam, mcw, gamma = reg
    cons = BRUTE_CONS[cons]
    clamped = splits = 0
    for seed in (0, 1, 2):
        rng = np.random.default_rng(seed)
        n, d, depth = 80, 3, 3
        X = rng.integers(-3, 4, size=(n, d)).astype(np.float32)  # few distinct values: ties between candidates
        if missing:
            X[rng.random(n) < 0.3, 0] = np.nan
            X[rng.random(n) < 0.1, 2] = np.nan
        cuts, nbins = R.quantile_cuts(X, 6, missing=missing)
        bins = R.bin_rows(X, cuts, nbins, missing=missing)
        gs, hs = R.grad_scales(1.0)
        q = np.stack([rng.integers(-(1 << 14), (1 << 14) + 1, n), rng.integers(0, (1 << 14) + 1, n)], 1).astype(np.int32)
        q[rng.random(n) < 0.2, 1] = 0  # zero-Hessian rows: reg_lambda = 0 meets a zero denominator
        tr, node = R.build_tree(bins, q, cuts, nbins, depth, lam, mcw, gamma, 0.3, gs, hs, missing=missing,
                                monotone=cons)
        feat, binv, dleft, gain, leaf, where = _brute_tree(bins[:, :d], q, nbins, depth, lam, mcw, gamma, 0.3,
                                                           1 / gs, 1 / hs, cons, missing)
        assert np.array_equal(tr.feat, feat) and np.array_equal(tr.bin, binv), (tr.feat, feat, tr.bin, binv)
        if missing:
            assert np.array_equal(tr.default_left, dleft)
        assert tr.gain.tobytes() == gain.tobytes()
        assert tr.leaf.tobytes() == leaf.tobytes()
        assert np.array_equal(node, where)
        free, _ = R.build_tree(bins, q, cuts, nbins, depth, lam, mcw, gamma, 0.3, gs, hs, missing=missing)
        clamped += int(not same_trees(tr, free, ("feat", "bin", "leaf")))
        splits += int((tr.feat >= 0).sum())
    assert clamped > 0 and splits > 0  # the constraints bite, and constrained trees still split


# ---- parameter forms -------------------------------------------------------------------------------------
def test_forms_resolve_to_the_same_signs():
    want = (1, 0, -1, 0)
    for form in (want, list(want), np.array(want), "(1,0,-1,0)", "1, 0, -1, 0", {0: 1, 2: -1}, {"0": 1, 2: -1, 3: 0}):
        p = gb.GBDTParams(monotone_constraints=form).validate()
        assert p.monotone_signs(4).tolist() == list(want), form
    assert gb.GBDTParams().validate().monotone_signs(4) is None
    assert gb.GBDTParams(monotone_constraints=(0, 0, 0, 0)).validate().monotone_signs(4) is None
    assert gb.GBDTParams(monotone_constraints={}).validate().monotone_signs(4) is None
    assert gb.GBDTParams(monotone_constraints="(0,0,0,0)").validate().monotone_signs(4) is None


def test_all_zero_equals_default_bit_for_bit(fits):
    X, y, free, mono = fits
    Xt, yt = torch.from_numpy(X), torch.from_numpy(y)
    for form in ((0, 0, 0, 0), "(0,0,0,0)", {1: 0}):
        zero = gb.fit(Xt, yt, gb.GBDTParams(monotone_constraints=form, **FIT_KW))
        assert same_trees(zero, free)
        assert zero.to_dict() == free.to_dict()
    for form in ("(1,-1,0,0)", {0: 1, 1: -1}):
        assert same_trees(gb.fit(Xt, yt, gb.GBDTParams(monotone_constraints=form, **FIT_KW)), mono)
    assert not same_trees(mono, free)


@pytest.mark.parametrize("bad", [(2, 0, 0, 0), (1.0, 0, 0, 0), (True, 0, 0, 0), "(1,x,0,0)", "(1,0.5,0,0)", 7,
                                 {-1: 1}, {0: 2}, {0: 1, "0": -1}, {"Amount": 1}, {0.5: 1}],
                         ids=lambda b: repr(b).replace(" ", ""))
def test_bad_values_raise(bad):
    with pytest.raises(ValueError, match="monotone_constraints"):
        gb.GBDTParams(monotone_constraints=bad).validate()
    with pytest.raises(ValueError, match="monotone_constraints"):
        GBDTClassifier(monotone_constraints=bad)


@pytest.mark.parametrize("bad", [(1, 0, 0), (1, 0, 0, 0, 0), (0, 0, 0), "(1,-1)", {4: 1}, {0: 1, 30: 0}],
                         ids=lambda b: repr(b).replace(" ", ""))
def test_wrong_length_or_out_of_range_raises(bad):
    X, y = fixture_data()
    with pytest.raises(ValueError, match="monotone_constraints"):
        gb.fit(torch.from_numpy(X), torch.from_numpy(y), gb.GBDTParams(monotone_constraints=bad, **FIT_KW))
    with pytest.raises(ValueError, match="monotone_constraints"):
        GBDTClassifier(monotone_constraints=bad, device="cpu", **FIT_KW).fit(X, y)


# ---- serialisation ---------------------------------------------------------------------------------------
def test_json_and_pickle_round_trip(tmp_path, fits):
    X, y, free, mono = fits
    clf = GBDTClassifier(monotone_constraints="(1,-1,0,0)", device="cpu", **FIT_KW).fit(X, y)
    want = clf.predict_margin(X)
    path = str(tmp_path / "m.json")
    clf.save_model(path)
    with open(path) as f:
        o = json.load(f)
    assert o["params"]["monotone_constraints"] == [1, -1, 0, 0]
    assert set(o) == set(free.to_dict()) | {"feature_names"}  # a constrained tree is an ordinary tree: no new field
    back = GBDTClassifier.load_model(path, device="cpu")
    assert back.get_params()["monotone_constraints"] == CONS
    assert same_trees(back.ensemble, mono) and np.array_equal(back.predict_margin(X), want)
    again = pickle.loads(pickle.dumps(clf))
    assert again.get_params()["monotone_constraints"] == CONS
    assert np.array_equal(again.predict_margin(X), want)
    assert same_trees(again.fit(X, y).ensemble, mono)  # the unpickled estimator refits constrained
    # an unconstrained model serialises as it always did
    plain = GBDTClassifier(device="cpu", **FIT_KW).fit(X, y)
    assert "monotone_constraints" not in plain.ensemble.to_dict()["params"]
    assert plain.get_params()["monotone_constraints"] is None


# ---- checkpoints -----------------------------------------------------------------------------------------
class _Recorder:
    """A checkpoint manager's interface that records the signatures a fit asks for."""

    def __init__(self):
        self.sigs = []

    def latest(self, sig):
        self.sigs.append(sig)
        return None

    def save(self, step, tensors, meta):
        self.sigs.append(meta["signature"])


def test_checkpoint_signature_unchanged_when_unconstrained():
    from fraud_detection_amd.utils.checkpoint import config_signature

    X, y = fixture_data()
    Xt, yt = torch.from_numpy(X), torch.from_numpy(y)
    kw = dict(n_estimators=2, max_depth=2, max_bin=8)
    cuts = gb.quantile_cuts(Xt, 8)

    def sig_of(**extra):
        rec = _Recorder()
        gb.fit(Xt, yt, gb.GBDTParams(**kw, **extra), cuts=cuts, checkpoint=rec, checkpoint_every=2)
        assert len(set(rec.sigs)) == 1
        return rec.sigs[0]

    # the signature of a fit from before the field existed: the non-default parameters only
    p = gb.GBDTParams(**kw)
    old = {k: v for k, v in p.__dict__.items()
           if k not in ("n_estimators", "monotone_constraints") and not (k in p.SAMPLING_DEFAULTS and v == p.SAMPLING_DEFAULTS[k])}
    want = config_signature(params=old, spw=1.0, cuts=cuts[0], nbins=cuts[1], n=600, d=4)
    assert sig_of() == want
    assert sig_of(monotone_constraints=(0, 0, 0, 0)) == want
    assert sig_of(monotone_constraints={}) == want
    mono = sig_of(monotone_constraints=CONS)
    assert mono != want
    assert sig_of(monotone_constraints="(1,-1,0,0)") == mono == sig_of(monotone_constraints={0: 1, 1: -1})
    assert sig_of(monotone_constraints=(1, 1, 0, 0)) != mono


def test_checkpoint_resume_equals_uninterrupted(tmp_path):
    from fraud_detection_amd.utils.checkpoint import CheckpointManager

    X, y = fixture_data()
    Xt, yt = torch.from_numpy(X), torch.from_numpy(y)
    kw = dict(max_depth=3, max_bin=16, learning_rate=0.3, monotone_constraints=CONS)
    full = gb.fit(Xt, yt, gb.GBDTParams(n_estimators=6, **kw))
    mgr = CheckpointManager(str(tmp_path), prefix="g")
    gb.fit(Xt, yt, gb.GBDTParams(n_estimators=3, **kw), checkpoint=mgr, checkpoint_every=3)
    saved = []
    save = mgr.save
    mgr.save = lambda step, *a, **k: (saved.append(step), save(step, *a, **k))[1]
    res = gb.fit(Xt, yt, gb.GBDTParams(n_estimators=6, **kw), checkpoint=mgr, checkpoint_every=1)
    assert saved == [4, 5, 6]
    assert same_trees(res, full)
    # the constraints are part of the signature: an unconstrained fit does not pick these up
    free_kw = {**kw, "monotone_constraints": None}
    other = gb.fit(Xt, yt, gb.GBDTParams(n_estimators=6, **free_kw), checkpoint=mgr, checkpoint_every=6)
    assert same_trees(other, gb.fit(Xt, yt, gb.GBDTParams(n_estimators=6, **free_kw)))
    assert not same_trees(other, full)


# ---- composition on the CPU path ---------------------------------------------------------------------------
def test_composes_with_sampling_weights_missing_hole_and_eval(fits):
    X, y, _, _ = fits
    rng = np.random.default_rng(11)
    Xn = X.copy()
    Xn[rng.random(600) < 0.1, 0] = np.nan
    Xn[rng.random(600) < 0.1, 2] = np.nan
    w = torch.from_numpy(rng.uniform(0.25, 2.0, 600).astype(np.float32))
    Xt, yt = torch.from_numpy(Xn), torch.from_numpy(y)
    p = gb.GBDTParams(monotone_constraints=CONS, missing_policy="learn", subsample=0.8, colsample_bynode=0.5, seed=3,
                      **FIT_KW)
    ens, rec = gb.fit(Xt, yt, p, sample_weight=w, eval_set=(Xt[:200], yt[:200]), early_stopping_rounds=3)
    assert ens.n_trees == rec.best_iteration + 1
    v = violations(ens_predict(ens), X, ens.cuts, ens.nbins, CONS)  # non-NaN rows: the guarantee's domain
    assert v[0][0] == 0 and v[1][0] == 0, v
    cuts = gb.quantile_cuts(Xt, 16, missing=True)
    bins = gb.bin_rows(Xt, cuts[0], cuts[1], missing=True)
    q = gb.GBDTParams(**{**p.__dict__, "subsample": 1.0})  # a fold around a row hole = the fit on the kept rows
    hole = gb.fit_binned(bins, yt, cuts, q, hole=(100, 150))
    keep = np.r_[0:100, 250:600]
    assert same_trees(hole, gb.fit_binned(bins[keep].contiguous(), yt[keep].contiguous(), cuts, q))
    v = violations(ens_predict(hole), X, hole.cuts, hole.nbins, CONS)
    assert v[0][0] == 0 and v[1][0] == 0, v


def test_train_entry_point_resolves_names():
    from fraud_detection_amd.train import parse_gbdt_monotone

    cols = ["Time", "V1", "V14", "Amount"]
    assert parse_gbdt_monotone("Amount=1,V14=-1", cols) == {3: 1, 2: -1}
    assert parse_gbdt_monotone(" Amount = +1 ", cols) == {3: 1}
    assert parse_gbdt_monotone(None, cols) is None and parse_gbdt_monotone("", cols) is None
    for bad in ("Amonut=1", "Amount", "Amount=2", "Amount=1,Amount=-1", "Amount=up"):
        with pytest.raises(ValueError, match="gbdt-monotone"):
            parse_gbdt_monotone(bad, cols)


# ---- data parallelism ------------------------------------------------------------------------------------
DP_KW = dict(n_estimators=4, max_depth=3, max_bin=16, learning_rate=0.3, monotone_constraints=CONS)


def _dp_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    from fraud_detection_amd.parallel.comm import Communicator

    comm = Communicator(backend="gloo")
    X, y = fixture_data()
    sh = slice(0, 301) if rank == 0 else slice(301, 600)
    ens = gb.fit(torch.from_numpy(X[sh].copy()), torch.from_numpy(y[sh].copy()), gb.GBDTParams(**DP_KW), comm=comm)
    np.savez(os.path.join(out_dir, f"m{rank}.npz"), **{k: getattr(ens, k) for k in TREE_KEYS}, cuts=ens.cuts)
    comm.close()


def test_dp_equals_single_process(tmp_path):
    """The histograms are all-reduced before the scan: every rank computes the same bounds."""
    from test_distributed import _free_port

    mp.start_processes(_dp_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, start_method="spawn")
    X, y = fixture_data()
    ref = gb.fit(torch.from_numpy(X), torch.from_numpy(y), gb.GBDTParams(**DP_KW))
    assert not same_trees(ref, gb.fit(torch.from_numpy(X), torch.from_numpy(y),
                                      gb.GBDTParams(**{**DP_KW, "monotone_constraints": None})))
    for r in range(2):
        o = np.load(os.path.join(tmp_path, f"m{r}.npz"))
        assert np.array_equal(o["cuts"], ref.cuts)
        assert all(o[k].tobytes() == getattr(ref, k).tobytes() for k in TREE_KEYS)


def test_train_entry_point_takes_constraints(tmp_path, monkeypatch):
    from fraud_detection_amd import train
    from fraud_detection_amd.config import Settings
    from fraud_detection_amd.data.synthetic import reference_frame
    import fraud_detection_amd.models.gbdt as mg

    df = reference_frame(3000, seed=5)
    csv = tmp_path / "cc.csv"
    df.to_csv(csv, index=False)
    monkeypatch.setenv("DATA_CSV", str(csv))
    monkeypatch.setenv("MLFLOW_TRACKING_URI", str(tmp_path / "mlruns"))
    monkeypatch.setenv("MLFLOW_AUC_THRESHOLD", "0.0")
    orig = gb.GBDTParams
    monkeypatch.setattr(mg.gb, "GBDTParams", lambda **kw: orig(**{"n_estimators": 5, "max_depth": 3, "max_bin": 16, **kw}))
    run = lambda **kw: train.run(Settings.load(), cv_folds=2, model_dir=str(tmp_path / "models"), verbose=False, **kw)  # noqa: E731
    with pytest.raises(ValueError, match="gbdt-monotone"):
        run(model_type="gbdt", gbdt_monotone="Amonut=1")
    with pytest.raises(ValueError, match="needs --model gbdt"):
        run(model_type="logistic", gbdt_monotone="Amount=1")
    out = run(model_type="gbdt", gbdt_monotone="Amount=1,V14=-1")
    assert out["gbdt_monotone"] == {"V14": -1, "Amount": 1}
    clf = GBDTClassifier.load_model(str(tmp_path / "models" / "xgb_model.json"), device="cpu")
    names = [c for c in df.columns if c != "Class"]
    cons = [0] * len(names)
    cons[names.index("Amount")], cons[names.index("V14")] = 1, -1
    assert clf.ensemble.params["monotone_constraints"] == cons
    import joblib

    Xs = joblib.load(tmp_path / "models" / "scaler.joblib").transform(df[names].to_numpy()[:64]).astype(np.float32)
    v = violations(clf.predict_margin, Xs, clf.ensemble.cuts, clf.ensemble.nbins, cons)
    assert all(n == 0 for n, _ in v.values()), v
