"""Per-round validation metrics and early stopping of the GBDT family on the CPU oracle path
(ops/gbdt.fit / fit_binned eval_set, ops/reference_gbdt.eval_record, models/gbdt.GBDTClassifier)."""
import os
import pickle
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from fraud_detection_amd.models.gbdt import GBDTClassifier
from fraud_detection_amd.ops import gbdt as gb
from fraud_detection_amd.ops import reference_gbdt as R

CAP_Q = int(np.rint(-np.log(1e-16) * 2.0 ** 30))


def noisy(n, seed, d=8, noise=1.5):
    """Rows whose label is mostly noise: deep trees at a high learning rate overfit them fast."""
    g = np.random.default_rng(seed)
    X = g.standard_normal((n, d)).astype(np.float32)
    s = X[:, 0] + 0.5 * X[:, 1] * X[:, 2] + noise * g.standard_normal(n)
    return torch.from_numpy(X), torch.from_numpy((s > 0.8).astype(np.uint8))


OVERFIT = dict(n_estimators=200, max_depth=6, learning_rate=0.5)
PATIENCE = 5


def trees_equal(a, b, k=None):
    return all(np.array_equal(getattr(a, f)[:k], getattr(b, f)[:k]) for f in ("feat", "bin", "thr", "gain", "leaf"))


# ---- the oracle ------------------------------------------------------------------------------
def test_eval_record_matches_sklearn_log_loss():
    from sklearn.metrics import log_loss

    g = np.random.default_rng(0)
    n = 5000
    m = np.concatenate([g.normal(0.0, 3.0, n), [20.0, -20.0, 20.0, -20.0]]).astype(np.float32)
    y = np.concatenate([g.integers(0, 2, n), [0, 0, 1, 1]]).astype(np.uint8)
    rec = R.eval_record(m, y)
    p = 1.0 / (1.0 + np.exp(-m.astype(np.float64)))
    ours = rec[0] / 2.0 ** 30 / rec[3]
    # quantisation half-unit of the 2^-30 fixed point + fp64 slack
    assert abs(ours - log_loss(y, p, labels=[0, 1])) <= 2.0 ** -31 + 1e-12
    assert rec[1] == int(((m > 0) != (y != 0)).sum())
    assert rec[2] == int(y.sum()) and rec[3] == n + 4
    assert rec.dtype == np.int64


def test_eval_record_cap():
    inf = np.float32(np.inf)
    m = np.array([80.0, -80.0, 80.0, -80.0, inf, -inf, inf, -inf], np.float32)
    y = np.array([0, 0, 1, 1, 0, 0, 1, 1], np.uint8)
    rec = R.eval_record(m, y)
    assert rec.tolist() == [4 * CAP_Q, 4, 4, 8]  # the wrong side pays -ln(1e-16), the right side 0
    assert R.eval_record(m[:1], y[:1])[0] == CAP_Q
    assert R.eval_record(m[1:2], y[1:2])[0] == 0
    assert R.eval_record(np.zeros(0, np.float32), np.zeros(0, np.uint8)).tolist() == [0, 0, 0, 0]


# ---- curves ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    X, y = noisy(1500, 11)
    Xv, yv = noisy(701, 12)
    p = gb.GBDTParams(n_estimators=6, max_depth=3, learning_rate=0.3)
    cuts = gb.quantile_cuts(X, p.max_bin)
    plain = gb.fit(X, y, p, cuts=cuts)
    ens, rec = gb.fit(X, y, p, cuts=cuts, eval_set=(Xv, yv), eval_metric=("logloss", "error", "auc"))
    return dict(X=X, y=y, Xv=Xv, yv=yv, p=p, cuts=cuts, plain=plain, ens=ens, rec=rec)


def test_curve_equals_partial_predict(small):
    s = small
    ens, rec = s["ens"], s["rec"]
    bv = R.bin_rows(s["Xv"].numpy(), *s["cuts"])
    assert rec.n_rounds == 6 and not rec.stopped
    for t in range(6):
        m = R.predict_margin_bins(bv, ens.feat[:t + 1], ens.bin[:t + 1], ens.leaf[:t + 1], ens.depth, ens.base_margin)
        assert rec.records[t].tolist() == R.eval_record(m, s["yv"].numpy()).tolist()
        assert rec.twice_pairs[t] == R.twice_pairs(m, s["yv"].numpy())
        # the walk on raw rows (thresholds) is the walk on bins
        assert np.array_equal(gb.predict_margin(s["Xv"], ens, n_trees=t + 1).numpy(), m)
        assert rec.history["logloss"][t] == rec.records[t, 0] / 2.0 ** 30 / 701
        assert rec.history["error"][t] == rec.records[t, 1] / 701
    assert set(rec.history) == {"logloss", "error", "auc"} and all(len(v) == 6 for v in rec.history.values())
    assert rec.best_iteration == int(np.argmax(rec.twice_pairs))  # the last metric decides (first best)
    assert rec.best_score == rec.history["auc"][rec.best_iteration]


def test_auc_metric_matches_sklearn(small):
    from sklearn.metrics import roc_auc_score

    s = small
    for t in (0, 3, 5):
        m = gb.predict_margin(s["Xv"], s["ens"], n_trees=t + 1).numpy()
        assert s["rec"].history["auc"][t] == pytest.approx(roc_auc_score(s["yv"].numpy(), m), abs=1e-12)


def test_eval_set_leaves_the_trees_alone(small):
    assert small["ens"].n_trees == 6
    assert trees_equal(small["ens"], small["plain"])


def test_partial_predict_is_slicing(small):
    s = small
    ens = s["ens"]
    for k in (0, 1, 4, 6):
        cut = gb.TreeEnsemble(depth=ens.depth, feat=ens.feat[:k], bin=ens.bin[:k], thr=ens.thr[:k], gain=ens.gain[:k],
                              leaf=ens.leaf[:k], cuts=ens.cuts, nbins=ens.nbins, base_score=ens.base_score)
        assert np.array_equal(gb.predict_margin(s["Xv"], ens, n_trees=k).numpy(), gb.predict_margin(s["Xv"], cut).numpy())
    with pytest.raises(ValueError):
        gb.predict_margin(s["Xv"], ens, n_trees=7)


def test_hole_curve_equals_explicit_set(small):
    s = small
    bins = gb.bin_rows(s["X"], *s["cuts"])
    hole = (400, 301)
    e0, m0 = gb.fit_binned(bins, s["y"], s["cuts"], s["p"], hole=hole, return_margin=True)
    e1, m1, r1 = gb.fit_binned(bins, s["y"], s["cuts"], s["p"], hole=hole, return_margin=True, eval_set="hole",
                               eval_metric=("error", "logloss"))
    e2, r2 = gb.fit_binned(bins, s["y"], s["cuts"], s["p"], hole=hole, eval_metric=("error", "logloss"),
                           eval_set=(bins[400:701], s["y"][400:701]))
    assert trees_equal(e0, e1) and trees_equal(e0, e2) and torch.equal(m0, m1)
    assert np.array_equal(r1.records, r2.records) and r1.records[0, 3] == 301
    assert r1.records[-1].tolist() == R.eval_record(m0[400:701].numpy(), s["y"][400:701].numpy()).tolist()


# ---- early stopping --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def overfit():
    X, y = noisy(2000, 1)
    Xv, yv = noisy(2000, 2)
    p = gb.GBDTParams(**OVERFIT)
    cuts = gb.quantile_cuts(X, p.max_bin)
    full, rec = gb.fit(X, y, p, cuts=cuts, eval_set=(Xv, yv), eval_metric=("auc", "error", "logloss"))
    return dict(X=X, y=y, Xv=Xv, yv=yv, p=p, cuts=cuts, full=full, rec=rec)


def test_early_stopping_follows_the_rule(overfit):
    o = overfit
    assert o["rec"].n_rounds == 200 and o["full"].n_trees == 200
    best, stop = gb.stop_round([int(v) for v in o["rec"].records[:, 0]], PATIENCE)
    assert stop is not None and stop < 199 and stop - best == PATIENCE  # this setup overfits: the rule fires
    ens, margin, rec = gb.fit(o["X"], o["y"], o["p"], cuts=o["cuts"], eval_set=[(o["Xv"], o["yv"])],
                              early_stopping_rounds=PATIENCE, return_margin=True)
    assert rec.stopped and rec.best_iteration == best and rec.n_rounds == stop + 1
    assert rec.history["logloss"] == o["rec"].history["logloss"][:stop + 1]
    assert rec.best_score == min(rec.history["logloss"])
    assert ens.n_trees == best + 1 and trees_equal(ens, o["full"], best + 1)
    bt = R.bin_rows(o["X"].numpy(), *o["cuts"])
    assert np.array_equal(margin.numpy(), R.predict_margin_bins(bt, ens.feat, ens.bin, ens.leaf, ens.depth, ens.base_margin))


def test_early_stopping_on_auc_and_error(overfit):
    o = overfit
    for metric, keys in (("auc", [-int(v) for v in o["rec"].twice_pairs]), ("error", [int(v) for v in o["rec"].records[:, 1]])):
        best, stop = gb.stop_round(keys, 3)
        assert stop is not None
        ens, rec = gb.fit(o["X"], o["y"], o["p"], cuts=o["cuts"], eval_set=(o["Xv"], o["yv"]),
                          eval_metric=("logloss", metric), early_stopping_rounds=3)
        assert (rec.best_iteration, rec.n_rounds, ens.n_trees) == (best, stop + 1, best + 1)
        assert rec.best_score == o["rec"].history[metric][best]


def test_stop_rule():
    assert gb.stop_round([5, 4, 4, 4, 3], 2) == (1, 3)   # equal is no improvement
    assert gb.stop_round([5, 4, 4, 3, 3, 3], 3) == (3, None)
    assert gb.stop_round([5, 6, 7], None) == (0, None)
    assert gb.stop_round([5, 6, 7], 1) == (0, 1)


# ---- the estimator ---------------------------------------------------------------------------
def test_classifier_eval_and_iteration_range(overfit):
    o = overfit
    clf = GBDTClassifier(device="cpu", eval_metric=["error", "logloss"], early_stopping_rounds=PATIENCE, **OVERFIT)
    clf.fit(o["X"].numpy(), o["y"].numpy(), eval_set=[(o["Xv"].numpy(), o["yv"].numpy())], verbose=False)
    res = clf.evals_result()
    assert list(res) == ["validation_0"] and list(res["validation_0"]) == ["error", "logloss"]
    best, stop = gb.stop_round([int(v) for v in o["rec"].records[:, 0]], PATIENCE)
    assert len(res["validation_0"]["logloss"]) == stop + 1 == len(res["validation_0"]["error"])
    assert clf.best_iteration == best and clf.best_score == res["validation_0"]["logloss"][best]
    assert clf.ensemble.n_trees == best + 1
    Xv = o["Xv"].numpy()
    for k in (1, 3, best + 1):
        cut = GBDTClassifier(device="cpu")
        e = clf.ensemble
        cut.ensemble = gb.TreeEnsemble(depth=e.depth, feat=e.feat[:k], bin=e.bin[:k], thr=e.thr[:k], gain=e.gain[:k],
                                       leaf=e.leaf[:k], cuts=e.cuts, nbins=e.nbins, base_score=e.base_score)
        assert np.array_equal(clf.predict_margin(Xv, iteration_range=(0, k)), cut.predict_margin(Xv))
        assert np.array_equal(clf.predict_proba(Xv, iteration_range=(0, k)), cut.predict_proba(Xv))
        assert np.array_equal(clf.predict(Xv, iteration_range=(0, k)), cut.predict(Xv))
    assert np.array_equal(clf.predict_margin(Xv, iteration_range=(0, 0)), clf.predict_margin(Xv))
    back = pickle.loads(pickle.dumps(clf))
    assert back.evals_result() == res and back.best_iteration == best and back.best_score == clf.best_score
    assert back.eval_metric == ["error", "logloss"] and back.early_stopping_rounds == PATIENCE
    assert np.array_equal(back.predict_margin(Xv), clf.predict_margin(Xv))


def test_classifier_reference_call_evaluates_nothing(small):
    s = small
    # train_model.py:69-80
    clf = GBDTClassifier(objective="binary:logistic", eval_metric="logloss", n_estimators=6, learning_rate=0.3,
                         max_depth=3, random_state=42, n_jobs=-1, device="cpu")
    clf.fit(s["X"].numpy(), s["y"].numpy())
    assert trees_equal(clf.ensemble, s["plain"])
    assert clf.best_iteration is None and clf.best_score is None
    with pytest.raises(RuntimeError):
        clf.evals_result()
    clf.fit(s["X"].numpy(), s["y"].numpy(), eval_set=[(s["Xv"].numpy(), s["yv"].numpy())])
    assert clf.evals_result()["validation_0"]["logloss"] == s["rec"].history["logloss"]
    assert trees_equal(clf.ensemble, s["plain"])


# ---- errors ----------------------------------------------------------------------------------
def test_error_cases(small, tmp_path):
    from fraud_detection_amd.utils.checkpoint import CheckpointManager

    s = small
    ev = (s["Xv"], s["yv"])
    with pytest.raises(NotImplementedError, match="checkpoint"):
        gb.fit(s["X"], s["y"], s["p"], eval_set=ev, checkpoint=CheckpointManager(str(tmp_path), prefix="gbdt"))
    bins = gb.bin_rows(s["X"], *s["cuts"])
    with pytest.raises(ValueError, match="hole"):
        gb.fit_binned(bins, s["y"], s["cuts"], s["p"], eval_set="hole")
    with pytest.raises(ValueError, match="hole"):
        gb.fit(s["X"], s["y"], s["p"], eval_set="hole")
    with pytest.raises(ValueError, match="one eval set"):
        gb.fit(s["X"], s["y"], s["p"], eval_set=[ev, ev])
    with pytest.raises(ValueError, match="eval_metric"):
        gb.fit(s["X"], s["y"], s["p"], eval_set=ev, eval_metric=("rmse",))
    with pytest.raises(ValueError, match="eval_set"):
        gb.fit(s["X"], s["y"], s["p"], early_stopping_rounds=3)
    with pytest.raises(ValueError):
        GBDTClassifier(device="cpu", early_stopping_rounds=3).fit(s["X"].numpy(), s["y"].numpy())


# ---- data parallel (two gloo ranks on the CPU oracle path) -------------------------------------
DP = dict(n_estimators=40, max_depth=4, learning_rate=0.5)


def _free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dp_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    from fraud_detection_amd.parallel.comm import Communicator

    comm = Communicator(backend="gloo")
    X, y = noisy(1200, 21)
    Xv, yv = noisy(800, 22)
    p = gb.GBDTParams(**DP)
    cuts = R.quantile_cuts(X.numpy(), p.max_bin)
    sh = slice(rank * 1200 // world, (rank + 1) * 1200 // world)
    shv = slice(rank * 800 // world, (rank + 1) * 800 // world)
    ens, rec = gb.fit(X[sh].contiguous(), y[sh].contiguous(), p, comm=comm, cuts=cuts,
                      eval_set=(Xv[shv].contiguous(), yv[shv].contiguous()), eval_metric=("error", "logloss"),
                      early_stopping_rounds=3)
    try:
        gb.fit(X[sh].contiguous(), y[sh].contiguous(), p, comm=comm, cuts=cuts,
               eval_set=(Xv[shv].contiguous(), yv[shv].contiguous()), eval_metric=("auc",))
        auc_raises = False
    except NotImplementedError:
        auc_raises = True
    np.savez(os.path.join(out_dir, f"r{rank}.npz"), records=rec.records, best=rec.best_iteration, stopped=rec.stopped,
             n_trees=ens.n_trees, leaf=ens.leaf, feat=ens.feat, auc_raises=auc_raises)
    comm.barrier()
    comm.close()


def test_data_parallel_ranks_agree_and_match_single_process(tmp_path):
    mp.start_processes(_dp_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, start_method="spawn")
    outs = [dict(np.load(os.path.join(tmp_path, f"r{r}.npz"))) for r in range(2)]
    X, y = noisy(1200, 21)
    Xv, yv = noisy(800, 22)
    p = gb.GBDTParams(**DP)
    ens, rec = gb.fit(X, y, p, cuts=R.quantile_cuts(X.numpy(), p.max_bin), eval_set=(Xv, yv),
                      eval_metric=("error", "logloss"), early_stopping_rounds=3)
    assert rec.stopped and rec.n_rounds < 40  # the rule fired: the ranks had a stop round to agree on
    for o in outs:
        assert np.array_equal(o["records"], rec.records)
        assert int(o["best"]) == rec.best_iteration and bool(o["stopped"]) and int(o["n_trees"]) == ens.n_trees
        assert np.array_equal(o["leaf"], ens.leaf) and np.array_equal(o["feat"], ens.feat)
        assert bool(o["auc_raises"])
