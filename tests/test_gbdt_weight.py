"""Per-row sample weights of the GBDT fit on the CPU path: the numpy oracle (ops/reference_gbdt.py)
through ops/gbdt.fit / fit_binned and models/gbdt.GBDTClassifier.

A weight is one more exact factor in front of the gradient quantisation, so every statement here is
an identity between two fits, bit for bit: all-ones = no weights, {0, 1} = the kept rows, 2 = every
row twice, class weights = scale_pos_weight.  Evaluation weights are checked the same way on the
exact integer records."""
import os
import warnings

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from fraud_detection_amd.models.gbdt import GBDTClassifier
from fraud_detection_amd.ops import gbdt as gb
from fraud_detection_amd.ops import reference_gbdt as R

TREE_ARRAYS = ("feat", "bin", "thr", "gain", "leaf")
N, D, DEPTH, ROUNDS, SPW = 4099, 7, 3, 4, 3.0
DYADIC = np.array([0.0, 0.25, 0.5, 1.0, 1.5, 4.0], np.float32)


def _same(a, b) -> bool:
    return all(np.array_equal(getattr(a, k), getattr(b, k)) for k in TREE_ARRAYS)


def _data(n=N, d=D, seed=11):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, d)).astype(np.float32)
    y = (X[:, 0] + 0.5 * X[:, 1] ** 2 + rng.normal(size=n) > 1.2).astype(np.uint8)
    return X, y


@pytest.fixture(scope="module")
def case():
    X, y = _data()
    cuts = R.quantile_cuts(X, 64)
    rng = np.random.default_rng(3)
    dyadic = DYADIC[rng.integers(0, len(DYADIC), N)]
    dyadic[:6] = DYADIC  # every value is there
    plain, mplain = _fit(X, y, cuts, return_margin=True)
    return dict(X=X, y=y, cuts=cuts, dyadic=dyadic, plain=plain, mplain=mplain.numpy())


def _params(**kw):
    kw.setdefault("n_estimators", ROUNDS)
    kw.setdefault("max_depth", DEPTH)
    kw.setdefault("scale_pos_weight", SPW)
    return gb.GBDTParams(**kw)


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a))


def _fit(X, y, cuts, w=None, return_margin=False, fit_kw=None, **kw):
    return gb.fit(_t(X), _t(y), _params(**kw), cuts=cuts, sample_weight=_t(w), return_margin=return_margin,
                  **(fit_kw or {}))


# ---- 1-4: identities between fits -----------------------------------------------------------------
def test_all_ones_is_the_unweighted_fit(case):
    ens, margin = _fit(case["X"], case["y"], case["cuts"], np.ones(N, np.float32), return_margin=True)
    assert _same(ens, case["plain"])
    assert np.array_equal(margin.numpy().view(np.uint32), case["mplain"].view(np.uint32))
    assert (case["plain"].feat >= 0).any()


def test_zero_one_weights_are_the_fit_on_the_kept_rows(case):
    X, y, cuts = case["X"], case["y"], case["cuts"]
    keep = np.random.default_rng(5).random(N) < 0.6
    ens, margin = _fit(X, y, cuts, keep.astype(np.float32), return_margin=True)
    sub, msub = _fit(X[keep], y[keep], cuts, return_margin=True)
    assert _same(ens, sub)
    assert np.array_equal(margin.numpy()[keep].view(np.uint32), msub.numpy().view(np.uint32))
    assert not _same(ens, case["plain"])
    # a zero-weight row still takes every margin update: its margin is the ensemble's walk
    walk = R.predict_margin_bins(R.bin_rows(X, *cuts), ens.feat, ens.bin, ens.leaf, DEPTH, ens.base_margin)
    assert np.array_equal(margin.numpy(), walk)


def test_uniform_two_is_every_row_twice(case):
    X, y, cuts = case["X"], case["y"], case["cuts"]
    ens, margin = _fit(X, y, cuts, np.full(N, 2.0, np.float32), return_margin=True)
    twice, mtwice = _fit(np.repeat(X, 2, axis=0), np.repeat(y, 2), cuts, return_margin=True)
    assert _same(ens, twice)
    assert np.array_equal(margin.numpy().view(np.uint32), mtwice.numpy()[::2].view(np.uint32))
    assert not _same(ens, case["plain"])  # (min_child_weight and lambda do not scale with the weights)


def test_class_weights_are_scale_pos_weight(case):
    X, y, cuts = case["X"], case["y"], case["cuts"]
    w = np.where(y != 0, 3.0, 1.0).astype(np.float32)
    ens, margin = _fit(X, y, cuts, w, return_margin=True, scale_pos_weight=1.0)
    assert _same(ens, case["plain"])
    assert np.array_equal(margin.numpy().view(np.uint32), case["mplain"].view(np.uint32))


# ---- 5: mixed dyadic weights ----------------------------------------------------------------------
def test_dyadic_round_one_gradients_are_the_closed_form(case):
    y, w = case["y"], case["dyadic"]
    gs, hs = R.grad_scales(SPW, float(w.max()))
    assert (gs, hs) == (1024.0, 4096.0)
    assert R.grad_scales(SPW) == R.grad_scales(SPW, 1.0) == (4096.0, 16384.0)
    w_eff = w.astype(np.float64) * np.where(y != 0, SPW, 1.0)
    q = R.gradients(np.zeros(N, np.float32), y, SPW, gs, hs, w)
    assert np.array_equal(q[:, 0], ((0.5 - y) * w_eff * gs).astype(np.int64))
    assert np.array_equal(q[:, 1], (0.25 * w_eff * hs).astype(np.int64))
    assert np.abs(q).max() <= 1 << 14 and (q[w == 0] == 0).all()
    assert ((0.5 - y) * w_eff * gs == np.rint((0.5 - y) * w_eff * gs)).all()  # exactly representable
    assert not _same(_fit(case["X"], y, case["cuts"], w), case["plain"])


def test_dyadic_with_subsample_is_the_oracle_composition(case):
    """Round by round: the weighted gradients, an out-of-sample row's pair zeroed whatever its weight."""
    X, y, cuts, w = case["X"], case["y"], case["cuts"], case["dyadic"]
    seed, sub = 5, 0.37
    ens, margin = _fit(X, y, cuts, w, return_margin=True, subsample=sub, seed=seed)
    b = R.bin_rows(X, *cuts)
    gs, hs = R.grad_scales(SPW, 4.0)
    m = np.zeros(N, np.float32)
    for t in range(ROUNDS):
        q = R.gradients(m, y, SPW, gs, hs, w)
        q[~R.row_sample_mask(seed, t, np.arange(N), sub)] = 0
        tr, node = R.build_tree(b, q, cuts[0], cuts[1], DEPTH, 1.0, 1.0, 0.0, 0.1, gs, hs)
        assert all(np.array_equal(getattr(tr, k), getattr(ens, k)[t]) for k in TREE_ARRAYS), t
        m = (m + tr.leaf[node]).astype(np.float32)
    assert np.array_equal(margin.numpy(), m)
    assert not _same(ens, _fit(X, y, cuts, w))


def test_dyadic_with_a_hole_is_the_fit_without_the_block(case):
    """The hole's weights are ignored for training, its largest one included (wmax is the fit rows')."""
    X, y, cuts = case["X"], case["y"], case["cuts"]
    w = case["dyadic"].copy()
    at, ln = 1001, 777
    w[at:at + ln] = 64.0
    keep = np.r_[0:at, at + ln:N]
    assert w[keep].max() == 4.0
    bins = torch.from_numpy(R.bin_rows(X, *cuts))
    ens, margin = gb.fit_binned(bins, _t(y), cuts, _params(), hole=(at, ln), sample_weight=_t(w), return_margin=True)
    ref, mref = gb.fit_binned(bins[keep], _t(y[keep]), cuts, _params(), sample_weight=_t(w[keep]), return_margin=True)
    assert _same(ens, ref)
    assert np.array_equal(margin.numpy()[keep], mref.numpy())
    assert not _same(ens, gb.fit_binned(bins, _t(y), cuts, _params(), hole=(at, ln)))


# ---- 6: evaluation weights ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def evcase(case):
    Xv, yv = _data(n=1203, seed=12)
    kw = dict(eval_set=(_t(Xv), _t(yv)), eval_metric=("error", "logloss"))
    plain_ens, plain = _fit(case["X"], case["y"], case["cuts"], case["dyadic"], fit_kw=kw, n_estimators=6)
    return dict(Xv=Xv, yv=yv, kw=kw, plain_ens=plain_ens, plain=plain)


def test_eval_record_weighted_unit_weights_are_the_unweighted_terms():
    rng = np.random.default_rng(0)
    m = rng.normal(0, 3, 501).astype(np.float32)
    y = rng.integers(0, 2, 501).astype(np.uint8)
    ref = R.eval_record(m, y)
    for c in (1.0, 0.375, 1e-20, 3e30):  # any common weight: wscale brings u to (2^15, 2^16]
        w = np.full(501, c, np.float32)
        ws = R.eval_weight_scale(float(w.max()))
        u = float(np.float32(c)) * ws
        assert 2.0 ** 15 < u <= 2.0 ** 16
        rec = R.eval_record_weighted(m, y, w, ws)
        assert rec[2:].tolist() == ref[2:].tolist()
        assert rec[1] == ref[1] * int(u * 2 ** 14)
        assert R.eval_weight_q(w, ws).sum() == 501 * int(u * 2 ** 14)
    w = np.ones(501, np.float32)
    assert R.eval_weight_scale(1.0) == 2.0 ** 16
    assert R.eval_record_weighted(m, y, w, 2.0 ** 16)[0] == ref[0]  # the loss terms bit for bit


def test_all_ones_eval_weights_reproduce_the_unweighted_history(case, evcase):
    """Every float of the history and every integer of the records: loss_q, n_pos, n_rows as they
    are; the error column is eval_record_weighted's err_q = n_err * 2^30 at unit weights (u = 2^16
    times 2^14), over weight_q = n_rows * 2^30."""
    m = len(evcase["yv"])
    ens, rec = _fit(case["X"], case["y"], case["cuts"], case["dyadic"], n_estimators=6,
                    fit_kw=dict(evcase["kw"], eval_sample_weight=torch.ones(m)))
    ref = evcase["plain"]
    assert _same(ens, evcase["plain_ens"])
    assert rec.history == ref.history
    assert rec.weight_q == m << 30 and ref.weight_q is None
    assert np.array_equal(rec.records[:, [0, 2, 3]], ref.records[:, [0, 2, 3]])
    assert np.array_equal(rec.records[:, 1], ref.records[:, 1] << 30)
    assert (rec.best_iteration, rec.best_score) == (ref.best_iteration, ref.best_score)


def test_zero_one_eval_weights_are_evaluation_on_the_subset(case, evcase):
    Xv, yv = evcase["Xv"], evcase["yv"]
    keep = np.random.default_rng(9).random(len(yv)) < 0.5
    _, rec = _fit(case["X"], case["y"], case["cuts"], case["dyadic"], n_estimators=6,
                  fit_kw=dict(evcase["kw"], eval_sample_weight=_t(keep.astype(np.float32))))
    _, sub = _fit(case["X"], case["y"], case["cuts"], case["dyadic"], n_estimators=6,
                  fit_kw=dict(evcase["kw"], eval_set=(_t(Xv[keep]), _t(yv[keep]))))
    assert rec.history == sub.history
    assert np.array_equal(rec.records[:, 0], sub.records[:, 0])
    assert np.array_equal(rec.records[:, 1], sub.records[:, 1] << 30)
    assert rec.weight_q == int(keep.sum()) << 30
    assert (rec.records[:, 3] == len(yv)).all() and (rec.records[:, 2] == int(yv.sum())).all()  # counts as today
    assert rec.history != evcase["plain"].history


@pytest.mark.parametrize("metric", ["logloss", "error"])
def test_early_stopping_with_eval_weights_stops_where_the_subset_stops(case, evcase, metric):
    Xv, yv = evcase["Xv"], evcase["yv"]
    keep = np.random.default_rng(9).random(len(yv)) < 0.5
    kw = dict(eval_metric=metric, early_stopping_rounds=2)
    args = dict(n_estimators=40, learning_rate=1.0)
    ens, rec = _fit(case["X"], case["y"], case["cuts"], case["dyadic"], **args,
                    fit_kw=dict(kw, eval_set=(_t(Xv), _t(yv)), eval_sample_weight=_t(keep.astype(np.float32))))
    sub_ens, sub = _fit(case["X"], case["y"], case["cuts"], case["dyadic"], **args,
                        fit_kw=dict(kw, eval_set=(_t(Xv[keep]), _t(yv[keep]))))
    assert rec.stopped and sub.stopped and rec.n_rounds < 40
    assert (rec.n_rounds, rec.best_iteration, rec.best_score) == (sub.n_rounds, sub.best_iteration, sub.best_score)
    assert _same(ens, sub_ens) and ens.n_trees == rec.best_iteration + 1


def test_hole_eval_weights_are_indexed_by_hole_row(case):
    X, y, cuts = case["X"], case["y"], case["cuts"]
    at, ln = 1001, 777
    bins = torch.from_numpy(R.bin_rows(X, *cuts))
    wv = case["dyadic"][:ln].copy()
    kw = dict(hole=(at, ln), sample_weight=_t(case["dyadic"]), eval_metric=("logloss", "error"))
    _, rec = gb.fit_binned(bins, _t(y), cuts, _params(), eval_set="hole", eval_sample_weight=_t(wv), **kw)
    keep = np.r_[0:at, at + ln:N]
    _, ref = gb.fit_binned(bins, _t(y), cuts, _params(), eval_set=(bins[at:at + ln], _t(y[at:at + ln])),
                           eval_sample_weight=_t(wv), **kw)
    assert np.array_equal(rec.records, ref.records) and rec.history == ref.history and rec.weight_q == ref.weight_q
    ws = R.eval_weight_scale(4.0)
    assert rec.weight_q == int(R.eval_weight_q(wv, ws).sum())
    ens, margin = gb.fit_binned(bins, _t(y), cuts, _params(), return_margin=True, **{k: kw[k] for k in ("hole", "sample_weight")})
    last = R.eval_record_weighted(margin.numpy()[at:at + ln], y[at:at + ln], wv, ws)
    assert rec.records[-1].tolist() == last.tolist()
    assert rec.history["logloss"][-1] == last[0] / rec.weight_q and rec.history["error"][-1] == last[1] / rec.weight_q
    assert keep.size == N - ln


# ---- 7: what is refused, and the resolution warning -----------------------------------------------
def test_bad_weights_are_refused(case, tmp_path):
    X, y, cuts = case["X"], case["y"], case["cuts"]
    ones = np.ones(N, np.float32)

    def fit(w, **kw):
        return gb.fit(_t(X), _t(y), _params(n_estimators=1), cuts=cuts, sample_weight=w, **kw)

    with pytest.raises(ValueError, match="shape"):
        fit(torch.ones(N - 1))
    with pytest.raises(ValueError, match="shape"):
        fit(torch.ones(N, 1))
    with pytest.raises(ValueError, match="float32"):
        fit(torch.ones(N, dtype=torch.float64))
    with pytest.raises(ValueError, match="device"):
        fit(torch.ones(N, device="meta"))
    for bad in (np.nan, np.inf, -np.inf, -1.0, -1e-30):
        w = ones.copy()
        w[N - 2] = bad
        with pytest.raises(ValueError, match="finite and >= 0"):
            fit(_t(w))
    with pytest.raises(ValueError, match="no row has a positive weight"):
        fit(torch.zeros(N))
    w = np.zeros(N, np.float32)
    w[100:200] = 1.0  # positive weights inside the hole only
    bins = torch.from_numpy(R.bin_rows(X, *cuts))
    with pytest.raises(ValueError, match="no row has a positive weight"):
        gb.fit_binned(bins, _t(y), cuts, _params(n_estimators=1), hole=(100, 100), sample_weight=_t(w))
    w = ones.copy()
    w[100:200] = np.nan  # what the hole holds is not looked at
    gb.fit_binned(bins, _t(y), cuts, _params(n_estimators=1), hole=(100, 100), sample_weight=_t(w))
    fit(_t(np.where(np.arange(N) % 2, -0.0, 1.0).astype(np.float32)))  # -0.0 is a zero weight

    from fraud_detection_amd.utils.checkpoint import CheckpointManager

    with pytest.raises(NotImplementedError, match="checkpoint"):
        fit(_t(ones), checkpoint=CheckpointManager(str(tmp_path), prefix="g"))


def test_bad_eval_weights_are_refused(case, evcase):
    X, y, cuts, yv = case["X"], case["y"], case["cuts"], evcase["yv"]
    m = len(yv)

    def fit(w, **kw):
        kw.setdefault("eval_set", evcase["kw"]["eval_set"])
        return gb.fit(_t(X), _t(y), _params(n_estimators=1), cuts=cuts, eval_sample_weight=w, **kw)

    with pytest.raises(ValueError, match="needs an eval_set"):
        fit(torch.ones(m), eval_set=None)
    with pytest.raises(ValueError, match="shape"):
        fit(torch.ones(m + 1))
    with pytest.raises(ValueError, match="device"):
        fit(torch.ones(m, device="meta"))
    for bad in (np.nan, np.inf, -2.0):
        w = torch.ones(m)
        w[3] = bad
        with pytest.raises(ValueError, match="finite and >= 0"):
            fit(w)
    with pytest.raises(ValueError, match="no row has a positive weight"):
        fit(torch.zeros(m))
    for metric in ("auc", "aucpr", ("logloss", "auc")):
        with pytest.raises(NotImplementedError, match="evaluation weights"):
            fit(torch.ones(m), eval_metric=metric)
    bins = torch.from_numpy(R.bin_rows(X, *cuts))
    with pytest.raises(ValueError, match="shape"):  # [hole_len], not [n]
        gb.fit_binned(bins, _t(y), cuts, _params(n_estimators=1), hole=(10, 50), eval_set="hole",
                      eval_sample_weight=torch.ones(N))


def test_resolution_warning(case):
    X, y, cuts = case["X"], case["y"], case["cuts"]
    w = np.ones(N, np.float32)
    w[::7] = 2.0 ** -9  # w_eff * gscale = 2^-9 * 4096 = 8 < 16 (a negative row: w_eff = w)
    w[y != 0] = 1.0
    with pytest.warns(UserWarning, match=r"8 < 16") as rec:
        _fit(X, y, cuts, w, n_estimators=2)
    assert len([r for r in rec if "sample_weight" in str(r.message)]) == 1  # once per fit, not per round
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        w[::7] = 2.0 ** -8  # exactly 16 quanta: fine
        w[y != 0] = 1.0
        _fit(X, y, cuts, w, n_estimators=1)
        _fit(X, y, cuts, case["dyadic"], n_estimators=1)  # 0.25 * 1024 = 256; zero weights do not count
        _fit(X, y, cuts, n_estimators=1)


# ---- the estimator --------------------------------------------------------------------------------
def test_classifier_takes_sample_weight_and_sample_weight_eval_set(case, evcase):
    X, y, cuts, w = case["X"], case["y"], case["cuts"], case["dyadic"]
    Xv, yv = evcase["Xv"], evcase["yv"]
    wv = case["dyadic"][:len(yv)]
    kw = dict(n_estimators=5, max_depth=DEPTH, scale_pos_weight=SPW, max_bin=64)
    clf = GBDTClassifier(eval_metric=["error", "logloss"], early_stopping_rounds=3, device="cpu", **kw)
    clf.fit(X, y, sample_weight=w, eval_set=[(Xv, yv)], sample_weight_eval_set=[wv])  # numpy
    cuts64 = gb.quantile_cuts(_t(X), 64)
    ens, rec = gb.fit(_t(X), _t(y), gb.GBDTParams(**kw), cuts=cuts64, sample_weight=_t(w), eval_set=(_t(Xv), _t(yv)),
                      eval_metric=["error", "logloss"], early_stopping_rounds=3, eval_sample_weight=_t(wv))
    assert _same(clf.ensemble, ens)
    assert clf.evals_result() == {"validation_0": rec.history} and clf.best_iteration == rec.best_iteration
    # torch tensors, float64 weights, the sklearn positional form fit(X, y, sample_weight)
    clf2 = GBDTClassifier(device="cpu", **kw).fit(_t(X), _t(y), torch.from_numpy(w.astype(np.float64)))
    assert _same(clf2.ensemble, GBDTClassifier(device="cpu", **kw).fit(X, y, sample_weight=list(w)).ensemble)
    assert not _same(clf2.ensemble, GBDTClassifier(device="cpu", **kw).fit(X, y).ensemble)
    assert _same(GBDTClassifier(device="cpu", **kw).fit(X, y, sample_weight=None, sample_weight_eval_set=None).ensemble,
                 GBDTClassifier(device="cpu", **kw).fit(X, y).ensemble)
    with pytest.raises(ValueError, match="needs an eval_set"):
        GBDTClassifier(device="cpu", **kw).fit(X, y, sample_weight_eval_set=[wv])
    with pytest.raises(ValueError, match="exactly one"):
        GBDTClassifier(device="cpu", **kw).fit(X, y, eval_set=[(Xv, yv)], sample_weight_eval_set=[wv, wv])


# ---- 8: data parallel -----------------------------------------------------------------------------
DP_KW = dict(n_estimators=4, max_depth=3, scale_pos_weight=SPW)
DP_SPLIT = 1501


def _dp_data():
    X, y = _data(n=3002, d=5, seed=12)
    rng = np.random.default_rng(4)
    w = DYADIC[rng.integers(0, 5, 3002)]          # rank 0's shard: weights up to 1.5
    w[DP_SPLIT + 7] = 4.0                          # rank 1's shard carries the global maximum
    Xv, yv = _data(n=801, d=5, seed=13)
    wv = DYADIC[rng.integers(0, 5, 801)]
    wv[5] = 4.0                                    # rank 0's eval shard carries the eval maximum
    return X, y, R.quantile_cuts(X, 64), w, Xv, yv, wv


def _dp_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    from fraud_detection_amd.parallel.comm import Communicator

    comm = Communicator(backend="gloo")
    X, y, cuts, w, Xv, yv, wv = _dp_data()
    sh = slice(0, DP_SPLIT) if rank == 0 else slice(DP_SPLIT, 3002)
    shv = slice(0, 400) if rank == 0 else slice(400, 801)
    assert w[sh].max() == (1.5 if rank == 0 else 4.0) and wv[shv].max() == (4.0 if rank == 0 else 1.5)
    ens, rec = gb.fit(_t(X[sh].copy()), _t(y[sh].copy()), gb.GBDTParams(**DP_KW), comm=comm, cuts=cuts,
                      sample_weight=_t(w[sh].copy()), eval_set=(_t(Xv[shv].copy()), _t(yv[shv].copy())),
                      eval_metric=("error", "logloss"), eval_sample_weight=_t(wv[shv].copy()))
    np.savez(os.path.join(out_dir, f"g{rank}.npz"), feat=ens.feat, bin=ens.bin, leaf=ens.leaf, thr=ens.thr,
             gain=ens.gain, records=rec.records, weight_q=np.int64(rec.weight_q),
             logloss=np.array(rec.history["logloss"]))
    comm.close()


def test_dp_weighted_trees_equal_single_process(tmp_path):
    """Two gloo ranks whose shards carry different largest weights: wmax (and the eval set's) is a
    global maximum, so both ranks quantise with the single-process scale and the trees are equal."""
    from test_distributed import _free_port

    mp.start_processes(_dp_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, start_method="spawn")
    X, y, cuts, w, Xv, yv, wv = _dp_data()
    ref, rrec = gb.fit(_t(X), _t(y), gb.GBDTParams(**DP_KW), cuts=cuts, sample_weight=_t(w), eval_set=(_t(Xv), _t(yv)),
                       eval_metric=("error", "logloss"), eval_sample_weight=_t(wv))
    assert (ref.feat >= 0).any()
    for r in range(2):
        o = np.load(os.path.join(tmp_path, f"g{r}.npz"))
        assert all(np.array_equal(o[k], getattr(ref, k)) for k in TREE_ARRAYS)
        assert np.array_equal(o["records"], rrec.records) and int(o["weight_q"]) == rrec.weight_q
        assert o["logloss"].tolist() == rrec.history["logloss"]
