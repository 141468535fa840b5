"""Per-round validation metrics and early stopping on the device: gbdt.hip gbdt_eval_kernel (both
variants) against the numpy oracle, and the fits, the hole path and the CV job built on it."""
import numpy as np
import pytest
import torch

from fraud_detection_amd.data.synthetic import separable
from fraud_detection_amd.models.gbdt_cv import DeviceGBDTCV
from fraud_detection_amd.models.pipeline import TrainConfig
from fraud_detection_amd.ops import gbdt as gb
from fraud_detection_amd.ops import reference_gbdt as R
from fraud_detection_amd.ops.native import native, ptr, stream_of

pytestmark = pytest.mark.gpu

FIELDS = ("feat", "bin", "thr", "gain", "leaf")


def trees_equal(a, b, k=None):
    return all(np.array_equal(getattr(a, f)[:k], getattr(b, f)[:k]) for f in FIELDS)


def noisy(n, seed, dev, d=8, noise=1.5):
    g = np.random.default_rng(seed)
    X = g.standard_normal((n, d)).astype(np.float32)
    s = X[:, 0] + 0.5 * X[:, 1] * X[:, 2] + noise * g.standard_normal(n)
    return torch.from_numpy(X).to(dev), torch.from_numpy((s > 0.8).astype(np.uint8)).to(dev)


def device_record(margin, label, r0, r1):
    rec = torch.zeros(4, dtype=torch.int64, device=margin.device)
    native().gbdt_eval(ptr(margin), ptr(label), r0, r1, ptr(rec), stream_of(margin))
    return rec.cpu().numpy()


def check_record(got, margin_np, label_np):
    """Counts exact; the loss within one rounding flip per row (device and numpy libm may differ in
    the last bit of exp / log1p, which can move a row's rint by one unit and by nothing larger)."""
    ref = R.eval_record(margin_np, label_np)
    assert got[1:].tolist() == ref[1:].tolist()
    assert abs(int(got[0]) - int(ref[0])) <= int(ref[3]), (got, ref)


# ---- the kernel ------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 262_147])
def test_eval_kernel_matches_the_oracle(dev, n):
    g = np.random.default_rng(n)
    r0, pad = 3, 5
    m = g.normal(0.0, 3.0, r0 + n + pad).astype(np.float32)
    y = g.integers(0, 2, r0 + n + pad).astype(np.uint8)
    special = np.array([50.0, -50.0, np.inf, -np.inf, 50.0, -50.0, np.inf, -np.inf], np.float32)
    k = min(n, 8)
    m[r0:r0 + k] = special[:k]
    y[r0:r0 + k] = np.array([0, 0, 0, 0, 1, 1, 1, 1], np.uint8)[:k]
    # poison outside the range: the kernel must not read it into the sums
    m[:r0], m[r0 + n:] = np.inf, -np.inf
    y[:r0], y[r0 + n:] = 0, 1
    md, yd = torch.from_numpy(m).to(dev), torch.from_numpy(y).to(dev)
    got = device_record(md, yd, r0, r0 + n)
    check_record(got, m[r0:r0 + n], y[r0:r0 + n])
    assert got[3] == n
    assert np.array_equal(device_record(md, yd, r0, r0 + n), got)  # integer sums: bitwise reproducible
    # an all-negative range
    zd = torch.zeros_like(yd)
    check_record(device_record(md, zd, r0, r0 + n), m[r0:r0 + n], np.zeros(n, np.uint8))
    # the kernel adds into the record, and an empty range adds nothing
    rec = torch.from_numpy(got.copy()).to(dev)
    native().gbdt_eval(ptr(md), ptr(yd), r0, r0 + n, ptr(rec), stream_of(md))
    native().gbdt_eval(ptr(md), ptr(yd), r0, r0, ptr(rec), stream_of(md))
    assert np.array_equal(rec.cpu().numpy(), 2 * got)


def test_eval_kernel_row_limit(dev):
    rec = torch.zeros(4, dtype=torch.int64, device=dev)
    one = torch.zeros(1, dtype=torch.float32, device=dev)
    lab = torch.zeros(1, dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError, match="2\\^27"):  # thrown before anything is launched
        native().gbdt_eval(ptr(one), ptr(lab), 0, (1 << 27) + 1, ptr(rec), stream_of(one))
    with pytest.raises(RuntimeError):
        native().gbdt_eval(ptr(one), ptr(lab), 1, 0, ptr(rec), stream_of(one))


@pytest.mark.parametrize("depth", [1, 5, 7])
def test_eval_walk_matches_margin_kernel_and_plain_record(dev, depth):
    m = native()
    X, y = separable(20_011, fraud_rate=0.05, seed=71, device=dev)
    Xv, yv = separable(10_007, fraud_rate=0.05, seed=72, device=dev)
    p = gb.GBDTParams(n_estimators=3, max_depth=depth, learning_rate=0.3)
    cuts = gb.quantile_cuts(X, p.max_bin)
    ens = gb.fit(X, y, p, cuts=cuts)
    nv, d = Xv.shape
    bins_v = gb.bin_rows(Xv, *cuts)
    ldt = (nv + 255) // 256 * 256
    binsT = torch.empty(d * ldt, dtype=torch.uint8, device=dev)
    st = stream_of(Xv)
    m.gbdt_transpose(ptr(bins_v), nv, d, ptr(binsT), ldt, st)
    feat, binv, leaf = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (ens.feat, ens.bin, ens.leaf))
    walk = torch.full((nv,), ens.base_margin, dtype=torch.float32, device=dev)
    plain = walk.clone()
    for t in range(3):
        rec = torch.zeros(4, dtype=torch.int64, device=dev)
        m.gbdt_eval_walk(ptr(binsT), ldt, nv, ptr(feat[t]), ptr(binv[t]), ptr(leaf[t]), depth, ptr(walk), ptr(yv),
                         ptr(rec), st)
        m.gbdt_margin(ptr(binsT), ldt, nv, ptr(feat[t]), ptr(binv[t]), ptr(leaf[t]), depth, ptr(plain), ptr(yv), 1.0,
                      1.0, 1.0, 0, st)
        assert torch.equal(walk, plain)
        assert np.array_equal(rec.cpu().numpy(), device_record(plain, yv, 0, nv))
    check_record(rec.cpu().numpy(), plain.cpu().numpy(), yv.cpu().numpy())


# ---- fits ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def table(dev):
    X, y = separable(20_011, fraud_rate=0.05, seed=81, device=dev)
    Xv, yv = separable(10_007, fraud_rate=0.05, seed=82, device=dev)
    p = gb.GBDTParams(n_estimators=8, max_depth=5, learning_rate=0.3)
    cuts = gb.quantile_cuts(X, p.max_bin)
    return dict(X=X, y=y, Xv=Xv, yv=yv, p=p, cuts=cuts, plain=gb.fit(X, y, p, cuts=cuts))


def test_device_fit_with_eval_set(dev, table):
    from sklearn.metrics import roc_auc_score

    s = table
    ens, rec = gb.fit(s["X"], s["y"], s["p"], cuts=s["cuts"], eval_set=(s["Xv"], s["yv"]),
                      eval_metric=("auc", "error", "logloss"))
    assert trees_equal(ens, s["plain"]) and ens.n_trees == 8
    assert rec.n_rounds == 8 and not rec.stopped
    yv = s["yv"].cpu().numpy()
    for t in range(8):
        mt = gb.predict_margin(s["Xv"], ens, n_trees=t + 1).cpu().numpy()
        check_record(rec.records[t], mt, yv)
        assert rec.twice_pairs[t] == R.twice_pairs(mt, yv)
    assert rec.history["auc"][7] == pytest.approx(roc_auc_score(yv, mt), abs=1e-12)
    assert rec.history["logloss"][7] == rec.records[7, 0] / 2.0 ** 30 / 10_007


def test_hole_curve_equals_explicit_set(dev, table):
    s = table
    bins = gb.bin_rows(s["X"], *s["cuts"])
    ha, hl = 5_003, 4_001
    e0, m0 = gb.fit_binned(bins, s["y"], s["cuts"], s["p"], hole=(ha, hl), return_margin=True)
    e1, m1, r1 = gb.fit_binned(bins, s["y"], s["cuts"], s["p"], hole=(ha, hl), return_margin=True, eval_set="hole",
                               eval_metric=("error", "auc", "logloss"))
    e2, r2 = gb.fit_binned(bins, s["y"], s["cuts"], s["p"], hole=(ha, hl), eval_metric=("error", "auc", "logloss"),
                           eval_set=(bins[ha:ha + hl], s["y"][ha:ha + hl]))
    assert trees_equal(e0, e1) and trees_equal(e0, e2) and torch.equal(m0, m1)
    assert np.array_equal(r1.records, r2.records) and np.array_equal(r1.twice_pairs, r2.twice_pairs)
    assert r1.records[:, 3].tolist() == [hl] * 8
    check_record(r1.records[7], m0[ha:ha + hl].cpu().numpy(), s["y"][ha:ha + hl].cpu().numpy())


def test_graph_replay_falls_back_to_eager_under_evaluation(dev, table):
    s = table
    ens, rec = gb.fit(s["X"], s["y"], s["p"], cuts=s["cuts"], eval_set=(s["Xv"], s["yv"]), use_graph=True)
    ref, rref = gb.fit(s["X"], s["y"], s["p"], cuts=s["cuts"], eval_set=(s["Xv"], s["yv"]), use_graph=False)
    assert trees_equal(ens, s["plain"]) and trees_equal(ref, s["plain"])
    assert np.array_equal(rec.records, rref.records) and rec.n_rounds == 8


def test_early_stopping_on_device(dev):
    X, y = noisy(2000, 1, dev)
    Xv, yv = noisy(2000, 2, dev)
    p = gb.GBDTParams(n_estimators=200, max_depth=6, learning_rate=0.5)
    cuts = gb.quantile_cuts(X, p.max_bin)
    full, rfull = gb.fit(X, y, p, cuts=cuts, eval_set=(Xv, yv))
    best, stop = gb.stop_round([int(v) for v in rfull.records[:, 0]], 5)
    assert full.n_trees == 200 and stop is not None and stop < 199  # the setup overfits: the rule fires
    ens, margin, rec = gb.fit(X, y, p, cuts=cuts, eval_set=(Xv, yv), early_stopping_rounds=5, return_margin=True)
    assert rec.stopped and (rec.best_iteration, rec.n_rounds) == (best, stop + 1)
    assert np.array_equal(rec.records, rfull.records[:stop + 1])
    assert ens.n_trees == best + 1 and trees_equal(ens, full, best + 1)
    bt = gb.bin_rows(X, *cuts).cpu().numpy()
    walk = R.predict_margin_bins(bt, ens.feat, ens.bin, ens.leaf, ens.depth, ens.base_margin)
    assert np.array_equal(margin.cpu().numpy(), walk)
    again, rec2 = gb.fit(X, y, p, cuts=cuts, eval_set=(Xv, yv), early_stopping_rounds=5)
    assert rec2.best_iteration == rec.best_iteration and trees_equal(again, ens)
    assert np.array_equal(rec2.records, rec.records)


def test_train_entry_point_writes_the_curves(tmp_path, monkeypatch):
    """train.py --gbdt-eval-metric / --gbdt-early-stopping reach the device CV job and the curves,
    best rounds and the final round count land in the --json summary."""
    import json

    from fraud_detection_amd import train
    from fraud_detection_amd.data.synthetic import reference_frame

    csv = tmp_path / "cc.csv"
    reference_frame(20000, seed=5).to_csv(csv, index=False)
    monkeypatch.setenv("DATA_CSV", str(csv))
    monkeypatch.setenv("FDX_DEVICE", "cuda")
    monkeypatch.setenv("MLFLOW_TRACKING_URI", str(tmp_path / "mlruns"))
    monkeypatch.setenv("MLFLOW_AUC_THRESHOLD", "0.0")
    orig = gb.GBDTParams
    monkeypatch.setattr(gb, "GBDTParams", lambda **kw: orig(**{"n_estimators": 6, "max_depth": 3, **kw}))
    out = tmp_path / "summary.json"
    assert train.main(["--model", "gbdt", "--cv-folds", "3", "--model-dir", str(tmp_path / "models"), "--json", str(out),
                       "--gbdt-eval-metric", "error,logloss", "--gbdt-early-stopping", "2"]) == 0
    ge = json.loads(out.read_text())["gbdt_eval"]
    assert ge["metrics"] == ["error", "logloss"] and ge["early_stopping_rounds"] == 2
    assert len(ge["fold_history"]) == 3 and len(ge["fold_best_iteration"]) == 3
    for h, best in zip(ge["fold_history"], ge["fold_best_iteration"]):
        assert set(h) == {"error", "logloss"} and best < len(h["logloss"]) <= 6
    assert ge["final_n_estimators"] == int(round(np.mean([b + 1 for b in ge["fold_best_iteration"]])))
    model = json.loads((tmp_path / "models" / "xgb_model.json").read_text())
    assert len(model["leaf"]) == ge["final_n_estimators"]


# ---- the CV job ------------------------------------------------------------------------------
def test_cv_job_with_evaluation_and_early_stopping(dev):
    X, y = separable(30_011, fraud_rate=0.02, seed=91, device=dev)
    p = gb.GBDTParams(n_estimators=12, max_depth=3, learning_rate=0.5)
    plain = DeviceGBDTCV(TrainConfig(), p).run(X, y)
    assert plain.fold_evals == [] and plain.final_n_estimators is None
    ev = DeviceGBDTCV(TrainConfig(), p, eval_metric=("logloss", "error")).run(X, y)
    assert ev.fold_aucs == plain.fold_aucs
    assert trees_equal(ev.final.ensemble, plain.final.ensemble)
    assert len(ev.fold_evals) == 5 and ev.final_n_estimators == 12
    for r in ev.fold_evals:
        assert all(len(v) == 12 for v in r.history.values()) and set(r.history) == {"logloss", "error"}
    es = DeviceGBDTCV(TrainConfig(), p, eval_metric=("logloss", "error"), early_stopping_rounds=2).run(X, y)
    want = int(round(float(np.mean([b + 1 for b in es.fold_best_iteration]))))
    assert es.final_n_estimators == want and es.final.ensemble.n_trees == want
    assert [r.best_iteration for r in es.fold_evals] == es.fold_best_iteration and len(es.fold_aucs) == 5
    for r, full in zip(es.fold_evals, ev.fold_evals):  # a stopped fold's curve is the full curve's head
        assert np.array_equal(r.records, full.records[:r.n_rounds])
        best, stop = gb.stop_round([int(v) for v in full.records[:, 1]], 2)
        assert r.best_iteration == best and r.n_rounds == (12 if stop is None else stop + 1)
