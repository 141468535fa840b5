"""Stochastic boosting of the GBDT family on the CPU oracle path: the stateless Philox row and
feature draws (ops/reference_gbdt.row_sample_mask / feature_masks), the masked split, and what
the draws being stateless buys -- repeatable fits, a bit-identical checkpoint resume, and
data-parallel trees equal to the single-process ones."""
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from fraud_detection_amd.ops import gbdt as gb
from fraud_detection_amd.ops import reference_gbdt as R

TREE_ARRAYS = ("feat", "bin", "thr", "gain", "leaf")


def _same(a, b) -> bool:
    return all(np.array_equal(getattr(a, k), getattr(b, k)) for k in TREE_ARRAYS)


def _data(n=3000, d=5, seed=11):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, d)).astype(np.float32)
    y = (X[:, 0] + 0.5 * X[:, 1] ** 2 + rng.normal(size=n) > 1.2).astype(np.uint8)
    return X, y, R.quantile_cuts(X, 64)


def _fit(X, y, cuts, **kw):
    kw.setdefault("n_estimators", 4)
    kw.setdefault("max_depth", 3)
    return gb.fit(torch.from_numpy(X), torch.from_numpy(y), gb.GBDTParams(**kw), cuts=cuts)


# ---- the parameter surface ----------------------------------------------------------------------
def test_params_have_the_sampling_fields():
    names = set(gb.GBDTParams.__dataclass_fields__)
    assert {"subsample", "colsample_bytree", "colsample_bylevel", "colsample_bynode", "seed"} <= names
    p = gb.GBDTParams()
    assert (p.subsample, p.colsample_bytree, p.colsample_bylevel, p.colsample_bynode, p.seed) == (1.0, 1.0, 1.0, 1.0, 0)


@pytest.mark.parametrize("name", ["subsample", "colsample_bytree", "colsample_bylevel", "colsample_bynode"])
@pytest.mark.parametrize("bad", [0.0, -0.1, 1.0001, float("nan")])
def test_validate_rejects_fractions_outside_unit_interval(name, bad):
    with pytest.raises(ValueError, match=name):
        gb.GBDTParams(**{name: bad}).validate()
    gb.GBDTParams(**{name: 1.0}).validate()
    gb.GBDTParams(**{name: 1e-9}).validate()


@pytest.mark.parametrize("bad", [-1, 1 << 64, 0.5])
def test_validate_rejects_bad_seed(bad):
    with pytest.raises(ValueError, match="seed"):
        gb.GBDTParams(seed=bad).validate()
    gb.GBDTParams(seed=(1 << 64) - 1).validate()


# ---- row masks ------------------------------------------------------------------------------------
def test_row_mask_is_a_function_of_seed_round_and_row():
    rows = np.arange(5000, dtype=np.int64)
    a = R.row_sample_mask(7, 3, rows, 0.5)
    assert a.dtype == np.bool_ and a.shape == (5000,)
    assert np.array_equal(a, R.row_sample_mask(7, 3, rows, 0.5))
    # another round or seed: an independent draw, so about half the rows differ (5 sigma of n / 2)
    for other in (R.row_sample_mask(7, 2, rows, 0.5), R.row_sample_mask(8, 3, rows, 0.5),
                  R.row_sample_mask(7 + (1 << 32), 3, rows, 0.5)):  # the seed's high word counts
        assert abs(int((a != other).sum()) - 2500) < 5 * np.sqrt(5000 * 0.25)


def test_row_mask_matches_the_definition_word_by_word():
    from fraud_detection_amd.ops.reference import philox4x32_10

    seed, t, s = (5 << 32) | 9, 6, 0.37
    thr = int(np.floor(s * 2.0 ** 32))
    assert R.sample_threshold(s) == thr
    for r in (0, 1, 2, 3, 4, 1023, (1 << 34) - 6, (1 << 34) + 1):
        w = philox4x32_10([(r >> 2) & 0xFFFFFFFF], [(r >> 2) >> 32], [t], [R.TAG_ROW], seed & 0xFFFFFFFF, seed >> 32)
        assert bool(R.row_sample_mask(seed, t, np.array([r]), s)[0]) == (int(w[r & 3][0]) < thr)
    assert len({R.TAG_ROW, R.TAG_TREE, R.TAG_LEVEL, R.TAG_NODE}) == 4


def test_row_mask_shards_concatenate_to_the_global_mask():
    whole = R.row_sample_mask(1, 2, np.arange(5000), 0.8)
    parts = [R.row_sample_mask(1, 2, np.arange(0, 2501), 0.8), R.row_sample_mask(1, 2, np.arange(2501, 5000), 0.8)]
    assert 2501 % 4 != 0 and np.array_equal(np.concatenate(parts), whole)


def test_row_mask_uses_the_counter_high_word():
    off = (1 << 34) - 6  # the rows straddle group index 2^32: groups 2^32 - 2 .. 2^32 + 1
    rows = off + np.arange(4096, dtype=np.int64)
    a = R.row_sample_mask(3, 1, rows, 0.5)
    assert np.array_equal(a[:1000], R.row_sample_mask(3, 1, rows[:1000], 0.5))
    # dropping the high word would repeat the draws of the rows 2^34 below
    low = R.row_sample_mask(3, 1, rows - (1 << 34), 0.5)
    assert not np.array_equal(a[6:], low[6:])
    assert abs(int((a[6:] != low[6:]).sum()) - 2045) < 5 * np.sqrt(4090 * 0.25)


@pytest.mark.parametrize("s", [0.5, 0.8, 0.1])
@pytest.mark.parametrize("seed,t", [(0, 0), (0, 1), (7, 3)])
def test_row_mask_share_is_binomial(s, seed, t):
    n = 1 << 20
    share = R.row_sample_mask(seed, t, np.arange(n, dtype=np.int64), s).mean()
    assert abs(share - s) < 5 * np.sqrt(s * (1 - s) / n)


def test_row_mask_full_sample_keeps_every_row():
    assert R.row_sample_mask(0, 0, np.arange(10_000), 1.0).all()
    assert R.row_sample_mask(0, 0, np.zeros(0, np.int64), 0.5).shape == (0,)


# ---- feature masks ------------------------------------------------------------------------------
def _pop(v) -> int:
    return bin(int(v)).count("1")


@pytest.mark.parametrize("d,counts", [(30, (24, 12, 3)), (5, (4, 2, 1)), (1, (1, 1, 1))])
def test_feature_mask_popcounts_and_nesting(d, counts):
    """0.8 by tree, 0.5 by level, 0.3 by node: max(1, int(c * |C|)) features at every stage, each
    stage inside the one above."""
    depth = 4
    ni = (1 << depth) - 1
    for t in range(3):
        tree = R.feature_masks(9, t, d, depth, 0.8, 1.0, 1.0)
        level = R.feature_masks(9, t, d, depth, 0.8, 0.5, 1.0)
        node = R.feature_masks(9, t, d, depth, 0.8, 0.5, 0.3)
        assert tree.dtype == np.uint32 and tree.shape == (ni,)
        assert len(set(tree.tolist())) == 1 and _pop(tree[0]) == counts[0]
        for lv in range(depth):
            ids = range((1 << lv) - 1, (2 << lv) - 1)
            assert len({int(level[i]) for i in ids}) == 1  # one draw per level
        for i in range(ni):
            assert (_pop(tree[i]), _pop(level[i]), _pop(node[i])) == counts
            assert int(level[i]) & ~int(tree[i]) == 0 and int(node[i]) & ~int(level[i]) == 0
            assert int(node[i]) != 0 and int(tree[i]) >> d == 0
    if d == 30:  # levels and nodes draw on their own: not one set repeated
        assert len({int(v) for v in level}) > 1 and len({int(v) for v in node}) > depth


def test_feature_mask_stage_counts_follow_python_truncation():
    for c, k in ((0.8, 24), (0.5, 15), (0.3, 9), (0.1, 3)):
        assert int(c * 30) == k
        assert _pop(R.feature_masks(0, 0, 30, 2, c)[0]) == k
        assert _pop(R.feature_masks(0, 0, 30, 2, 1.0, c)[0]) == k
        assert _pop(R.feature_masks(0, 0, 30, 2, 1.0, 1.0, c)[0]) == k


def test_feature_mask_fraction_one_is_the_identity():
    full = R.feature_masks(4, 2, 7, 3)
    assert np.array_equal(full, np.full(7, (1 << 7) - 1, np.uint32))
    only_node = R.feature_masks(4, 2, 7, 3, 1.0, 1.0, 0.5)
    assert np.array_equal(R.feature_masks(4, 2, 7, 3, 1.0, 1.0, 0.5), only_node)
    # a stage at 1.0 draws nothing: the node stage sees the same candidates and keys either way
    tree_only = R.feature_masks(4, 2, 7, 3, 0.5)
    assert np.array_equal(R.feature_masks(4, 2, 7, 3, 0.5, 1.0, 1.0), tree_only) and len(set(tree_only.tolist())) == 1


def test_feature_mask_keeps_the_smallest_keys():
    from fraud_detection_amd.ops.reference import philox4x32_10

    seed, t, d = (3 << 32) | 1, 5, 11
    keys = [int(philox4x32_10([f], [0], [t], [R.TAG_TREE], seed & 0xFFFFFFFF, seed >> 32)[0][0]) for f in range(d)]
    want = sorted(range(d), key=lambda f: (keys[f], f))[:int(0.5 * d)]
    assert int(R.feature_masks(seed, t, d, 2, 0.5)[0]) == sum(1 << f for f in want)
    assert R.feature_masks(seed, t + 1, d, 2, 0.5)[0] != R.feature_masks(seed, t, d, 2, 0.5)[0] or \
        R.feature_masks(seed, t + 2, d, 2, 0.5)[0] != R.feature_masks(seed, t, d, 2, 0.5)[0]


@pytest.mark.parametrize("d,depth", [(30, 5), (5, 3), (1, 2), (17, 1), (30, 7)])
@pytest.mark.parametrize("fracs", [(0.5, 1.0, 1.0), (1.0, 0.3, 1.0), (1.0, 1.0, 0.8), (0.8, 0.5, 0.3), (0.1, 0.1, 0.1),
                                   (1.0, 1.0, 1.0)])
def test_feature_mask_table_is_the_per_round_masks(d, depth, fracs):
    """What a fit uploads (all rounds drawn at a time) against the per-round definition."""
    seed = (7 << 32) | 11
    table = R.feature_mask_table(seed, 4, d, depth, *fracs)
    assert table.dtype == np.uint32 and table.shape == (4, (1 << depth) - 1)
    assert table.flags.c_contiguous  # the device reads round t's masks at row t's address
    assert np.array_equal(table, np.stack([R.feature_masks(seed, t, d, depth, *fracs) for t in range(4)]))
    assert R.feature_mask_table(seed, 0, d, depth, *fracs).shape == (0, (1 << depth) - 1)


# ---- split level ----------------------------------------------------------------------------------
def _node_hist(rng, d, nbins):
    H = np.zeros((d, 256, 2), np.int64)
    for f in range(d):
        nb = int(nbins[f])
        H[f, :nb, 1] = np.diff(np.concatenate([[0], np.sort(rng.integers(0, 1 << 22, nb - 1)), [1 << 22]])) if nb > 1 \
            else [1 << 22]
        g = rng.integers(-(1 << 18), 1 << 18, nb)
        g[nb - 1] += 12345 - int(g.sum())
        H[f, :nb, 0] = g
    return H


def test_best_split_masked_winner_yields_the_runner_up():
    rng = np.random.default_rng(3)
    d = 6
    nbins = np.full(d, 32, np.int32)
    H = _node_hist(rng, d, nbins)
    gs, hs = R.grad_scales(1.0)
    args = (nbins, 1.0 / gs, 1.0 / hs, 1.0, 1.0)
    full = R.best_split(H, *args)
    assert R.best_split(H, *args, fmask=(1 << d) - 1) == full
    per_feature = [R.best_split(H, *args, fmask=1 << f) for f in range(d)]
    assert all(r[1] == f for f, r in enumerate(per_feature))
    order = sorted(range(d), key=lambda f: (-per_feature[f][0], f))
    assert full[1] == order[0] and full == per_feature[order[0]]
    second = R.best_split(H, *args, fmask=((1 << d) - 1) & ~(1 << order[0]))
    assert second == per_feature[order[1]] and second[0] <= full[0]
    # the node totals are feature 0's sums whether or not feature 0 is allowed
    assert all(r[5:] == full[5:] for r in per_feature)


def test_best_split_only_constant_features_allowed_means_no_split():
    rng = np.random.default_rng(4)
    nbins = np.array([32, 1, 32, 1], np.int32)
    H = _node_hist(rng, 4, nbins)
    gs, hs = R.grad_scales(1.0)
    got = R.best_split(H, nbins, 1.0 / gs, 1.0 / hs, 1.0, 1.0, fmask=0b1010)
    assert got[0] == -np.inf and not R.accepts_split(got[0], 0.0)
    assert got[5:] == R.best_split(H, nbins, 1.0 / gs, 1.0 / hs, 1.0, 1.0)[5:]


def test_tree_splits_only_on_allowed_features():
    X, y, cuts = _data()
    ens = _fit(X, y, cuts, n_estimators=5, colsample_bytree=0.6, colsample_bynode=0.5, seed=3)
    for t in range(5):
        fm = R.feature_masks(3, t, 5, 3, 0.6, 1.0, 0.5)
        for node, f in enumerate(ens.feat[t]):
            assert f < 0 or (int(fm[node]) >> int(f)) & 1
    assert (ens.feat >= 0).any()


# ---- fit behaviour --------------------------------------------------------------------------------
def test_subsampled_fit_differs_and_repeats():
    X, y, cuts = _data()
    full = _fit(X, y, cuts)
    a = _fit(X, y, cuts, subsample=0.5)
    assert not _same(a, full)
    assert _same(a, _fit(X, y, cuts, subsample=0.5))
    assert not _same(a, _fit(X, y, cuts, subsample=0.5, seed=1))
    assert not _same(_fit(X, y, cuts, colsample_bytree=0.5), full)


def test_seed_alone_changes_nothing():
    X, y, cuts = _data()
    assert _same(_fit(X, y, cuts, seed=123), _fit(X, y, cuts))


def test_subsampled_fit_is_the_oracle_on_zeroed_gradients():
    """Round by round: q[~mask] = 0, every row's margin updated by every tree."""
    X, y, cuts = _data(n=2000)
    p = gb.GBDTParams(n_estimators=3, max_depth=3, subsample=0.5, seed=5, scale_pos_weight=2.0)
    ens, margin = gb.fit(torch.from_numpy(X), torch.from_numpy(y), p, cuts=cuts, return_margin=True)
    b = R.bin_rows(X, *cuts)
    gs, hs = R.grad_scales(2.0)
    m = np.zeros(2000, np.float32)
    for t in range(3):
        q = R.gradients(m, y, 2.0, gs, hs)
        q[~R.row_sample_mask(5, t, np.arange(2000), 0.5)] = 0
        tr, node = R.build_tree(b, q, cuts[0], cuts[1], 3, 1.0, 1.0, 0.0, 0.1, gs, hs)
        assert np.array_equal(tr.feat, ens.feat[t]) and np.array_equal(tr.leaf, ens.leaf[t])
        m = (m + tr.leaf[node]).astype(np.float32)
    assert np.array_equal(margin.numpy(), m)


def test_hole_rows_keep_their_table_index():
    """A fit around a hole draws by TABLE row: it equals the fit of the same rows placed at the
    same global ids without a hole -- the rows after the hole through row_offset."""
    X, y, cuts = _data(n=1500)
    bins = torch.from_numpy(R.bin_rows(X, *cuts))
    yt = torch.from_numpy(y)
    p = gb.GBDTParams(n_estimators=3, max_depth=3, subsample=0.5, seed=2)
    head = gb.fit_binned(bins, yt, cuts, p, hole=(1000, 500))                     # rows [0, 1000)
    assert _same(head, gb.fit_binned(bins[:1000], yt[:1000], cuts, p))
    tail = gb.fit_binned(bins, yt, cuts, p, hole=(0, 1003))                       # rows [1003, 1500)
    assert _same(tail, gb.fit_binned(bins[1003:], yt[1003:], cuts, p, row_offset=1003))
    assert not _same(tail, gb.fit_binned(bins[1003:], yt[1003:], cuts, p))
    with pytest.raises(ValueError, match="row_offset"):
        gb.fit_binned(bins, yt, cuts, p, row_offset=-1)


def test_classifier_takes_the_sampling_arguments(tmp_path):
    import joblib

    from fraud_detection_amd.models.gbdt import GBDTClassifier

    X, y, _ = _data()
    kw = dict(n_estimators=4, max_depth=3, device="cpu", subsample=0.5, colsample_bynode=0.5)
    a = GBDTClassifier(random_state=1, **kw).fit(X, y)
    b = GBDTClassifier(random_state=2, **kw).fit(X, y)
    assert a.params.seed == 1 and a.params.subsample == 0.5 and a.params.colsample_bynode == 0.5
    assert not np.array_equal(a.predict_margin(X), b.predict_margin(X))
    assert np.array_equal(GBDTClassifier(random_state=1, **kw).fit(X, y).predict_margin(X), a.predict_margin(X))
    assert GBDTClassifier(seed=5, random_state=1).params.seed == 5  # seed wins over random_state
    assert GBDTClassifier(objective="binary:logistic", n_jobs=4).params == gb.GBDTParams()  # still ignored
    assert a.get_params()["subsample"] == 0.5
    path = str(tmp_path / "m.json")
    a.save_model(path)
    m2 = GBDTClassifier.load_model(path, device="cpu")
    assert m2.params == a.params and np.array_equal(m2.predict_margin(X), a.predict_margin(X))
    joblib.dump(a, tmp_path / "m.joblib")
    m3 = joblib.load(tmp_path / "m.joblib")
    assert m3.params == a.params and np.array_equal(m3.predict_margin(X), a.predict_margin(X))
    # a model pickled before the sampling fields existed loads with their defaults
    st = a.__getstate__()
    for k in gb.GBDTParams.SAMPLING_DEFAULTS:
        st["params"].pop(k)
    old = GBDTClassifier.__new__(GBDTClassifier)
    old.__setstate__(st)
    assert (old.params.subsample, old.params.seed) == (1.0, 0) and not old.params.sampled


def test_cv_job_params_keep_the_sampling_fields():
    """DeviceGBDTCV.one_fit and GBDTPipeline rebuild GBDTParams from __dict__ plus overrides."""
    p = gb.GBDTParams(subsample=0.7, colsample_bylevel=0.4, seed=11)
    q = gb.GBDTParams(**{**p.__dict__, "scale_pos_weight": 3.0, "n_estimators": 7})
    assert (q.subsample, q.colsample_bylevel, q.seed, q.scale_pos_weight, q.n_estimators) == (0.7, 0.4, 11, 3.0, 7)


def test_train_entry_point_passes_the_sampling_flags(tmp_path, monkeypatch):
    """--gbdt-subsample / --gbdt-colsample-bytree / --gbdt-seed reach every CV fold's fit and the
    final fit, the saved model and the run summary."""
    import json

    from fraud_detection_amd import train
    from fraud_detection_amd.config import Settings
    from fraud_detection_amd.data.synthetic import reference_frame
    import fraud_detection_amd.models.gbdt as mg

    csv = tmp_path / "cc.csv"
    reference_frame(3000, seed=5).to_csv(csv, index=False)
    monkeypatch.setenv("DATA_CSV", str(csv))
    monkeypatch.setenv("MLFLOW_TRACKING_URI", str(tmp_path / "mlruns"))
    monkeypatch.setenv("MLFLOW_AUC_THRESHOLD", "0.0")
    orig = gb.GBDTParams
    monkeypatch.setattr(mg.gb, "GBDTParams", lambda **kw: orig(**{**kw, "n_estimators": 3, "max_depth": 3}))
    seen = []
    fit = train._fit
    monkeypatch.setattr(train, "_fit", lambda *a, **kw: (seen.append(kw.get("gbdt_params")), fit(*a, **kw))[1])
    logged = {}
    monkeypatch.setattr(train.mlf, "log_param", lambda k, v: logged.__setitem__(k, v))
    out = train.run(Settings.load(), model_type="gbdt", cv_folds=2, model_dir=str(tmp_path / "models"), verbose=False,
                    gbdt_subsample=0.5, gbdt_colsample_bytree=0.6, gbdt_seed=3)
    assert len(seen) == 3  # two folds and the final fit
    assert all((p.subsample, p.colsample_bytree, p.seed) == (0.5, 0.6, 3) for p in seen)
    assert out["gbdt_sampling"] == {"subsample": 0.5, "colsample_bytree": 0.6, "seed": 3}
    saved = json.load(open(tmp_path / "models" / "xgb_model.json"))["params"]
    assert (saved["subsample"], saved["colsample_bytree"], saved["seed"]) == (0.5, 0.6, 3)
    assert (logged["gbdt_subsample"], logged["gbdt_colsample_bytree"], logged["gbdt_seed"]) == (0.5, 0.6, 3)
    with pytest.raises(ValueError, match="gbdt"):
        train.run(Settings.load(), model_type="logistic", cv_folds=0, model_dir=str(tmp_path / "m2"), verbose=False,
                  gbdt_subsample=0.5)


def test_train_command_line_reaches_run(tmp_path, monkeypatch):
    """argparse -> run(gbdt_subsample=, gbdt_colsample_bytree=, gbdt_seed=); defaults without the flags."""
    from fraud_detection_amd import train

    got = []
    monkeypatch.setattr(train, "run", lambda *a, **kw: (got.append(kw), {"test_auc": 0.5, "eval": {}})[1])
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    train.main(["--model", "gbdt", "--gbdt-subsample", "0.8", "--gbdt-colsample-bytree", "0.5", "--gbdt-seed", "7"])
    train.main(["--model", "gbdt"])
    assert (got[0]["gbdt_subsample"], got[0]["gbdt_colsample_bytree"], got[0]["gbdt_seed"]) == (0.8, 0.5, 7)
    assert (got[1]["gbdt_subsample"], got[1]["gbdt_colsample_bytree"], got[1]["gbdt_seed"]) == (1.0, 1.0, 0)


# ---- checkpoint -----------------------------------------------------------------------------------
def test_resume_is_bit_identical_under_sampling(tmp_path):
    from fraud_detection_amd.utils.checkpoint import CheckpointManager

    X, y, cuts = _data()
    Xt, yt = torch.from_numpy(X), torch.from_numpy(y)
    kw = dict(max_depth=3, subsample=0.5, colsample_bynode=0.5, seed=4)
    full = gb.fit(Xt, yt, gb.GBDTParams(n_estimators=6, **kw), cuts=cuts)
    mgr = CheckpointManager(str(tmp_path), prefix="g")
    gb.fit(Xt, yt, gb.GBDTParams(n_estimators=3, **kw), cuts=cuts, checkpoint=mgr, checkpoint_every=3)
    res = gb.fit(Xt, yt, gb.GBDTParams(n_estimators=6, **kw), cuts=cuts, checkpoint=mgr, checkpoint_every=3)
    assert _same(res, full)
    assert np.array_equal(res.feat[:3], gb.fit(Xt, yt, gb.GBDTParams(n_estimators=3, **kw), cuts=cuts).feat)
    # another seed is another configuration: its checkpoint is not picked up
    other = gb.fit(Xt, yt, gb.GBDTParams(n_estimators=6, **{**kw, "seed": 5}), cuts=cuts, checkpoint=mgr,
                   checkpoint_every=3)
    assert _same(other, gb.fit(Xt, yt, gb.GBDTParams(n_estimators=6, **{**kw, "seed": 5}), cuts=cuts))


def test_checkpoint_signature_unchanged_without_sampling(tmp_path):
    """The signature names the sampling fields only off their defaults, so a checkpoint written
    before they existed (no such keys) still resumes an unsampled fit."""
    from fraud_detection_amd.utils.checkpoint import CheckpointManager, config_signature

    X, y, cuts = _data()
    Xt, yt = torch.from_numpy(X), torch.from_numpy(y)
    mgr = CheckpointManager(str(tmp_path), prefix="g")
    p = gb.GBDTParams(n_estimators=2, max_depth=3)
    gb.fit(Xt, yt, p, cuts=cuts, checkpoint=mgr, checkpoint_every=2)
    legacy = {k: v for k, v in p.__dict__.items() if k != "n_estimators" and k not in gb.GBDTParams.SAMPLING_DEFAULTS}
    sig = config_signature(params=legacy, spw=1.0, cuts=cuts[0], nbins=cuts[1], n=len(X), d=5)
    assert mgr.latest(sig) is not None


# ---- data parallel --------------------------------------------------------------------------------
DP_KW = dict(n_estimators=4, max_depth=3, subsample=0.5, colsample_bytree=0.6, seed=6)


def _dp_data():
    rng = np.random.default_rng(12)
    X = rng.normal(size=(3002, 5)).astype(np.float32)
    y = (X[:, 0] + 0.5 * X[:, 1] ** 2 + rng.normal(size=3002) > 1.2).astype(np.uint8)
    return X, y, R.quantile_cuts(X, 64)


def _dp_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    from fraud_detection_amd.parallel.comm import Communicator

    comm = Communicator(backend="gloo")
    X, y, cuts = _dp_data()
    sh = slice(0, 1501) if rank == 0 else slice(1501, 3002)  # the boundary is no multiple of 4
    ens = gb.fit(torch.from_numpy(X[sh].copy()), torch.from_numpy(y[sh].copy()), gb.GBDTParams(**DP_KW), comm=comm,
                 cuts=cuts)
    np.savez(os.path.join(out_dir, f"g{rank}.npz"), feat=ens.feat, bin=ens.bin, leaf=ens.leaf)
    comm.close()


def _dp_resume_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    from fraud_detection_amd.parallel.comm import Communicator
    from fraud_detection_amd.utils.checkpoint import CheckpointManager

    comm = Communicator(backend="gloo")
    X, y, cuts = _dp_data()
    sh = slice(0, 1501) if rank == 0 else slice(1501, 3002)
    Xs, ys = torch.from_numpy(X[sh].copy()), torch.from_numpy(y[sh].copy())
    mgr = CheckpointManager(os.path.join(out_dir, "ck"), prefix="g", rank=rank)  # rank 0 writes, all ranks load
    kw = {**DP_KW, "colsample_bynode": 0.5}
    gb.fit(Xs, ys, gb.GBDTParams(**{**kw, "n_estimators": 3}), comm=comm, cuts=cuts, checkpoint=mgr, checkpoint_every=3)
    comm.barrier()
    saved = []  # the rounds the second fit checkpoints: it starts where it resumed
    save = mgr.save
    mgr.save = lambda step, *a, **k: (saved.append(step), save(step, *a, **k))[1]
    ens = gb.fit(Xs, ys, gb.GBDTParams(**{**kw, "n_estimators": 6}), comm=comm, cuts=cuts, checkpoint=mgr,
                 checkpoint_every=1)
    np.savez(os.path.join(out_dir, f"r{rank}.npz"), feat=ens.feat, bin=ens.bin, leaf=ens.leaf, saved=np.array(saved))
    comm.close()


def test_dp_sampled_resume_equals_uninterrupted_and_single_process(tmp_path):
    """Two ranks, interrupted after 3 of 6 rounds: every rank computes the same checkpoint signature
    (its own row offset is NOT in it), so both resume at round 3 and the trees equal the
    uninterrupted single-process fit."""
    from test_distributed import _free_port

    mp.start_processes(_dp_resume_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, start_method="spawn")
    X, y, cuts = _dp_data()
    ref = gb.fit(torch.from_numpy(X), torch.from_numpy(y),
                 gb.GBDTParams(**{**DP_KW, "colsample_bynode": 0.5, "n_estimators": 6}), cuts=cuts)
    for r in range(2):
        o = np.load(os.path.join(tmp_path, f"r{r}.npz"))
        assert o["saved"].tolist() == [4, 5, 6], (r, o["saved"])  # resumed after round 3, on BOTH ranks
        assert np.array_equal(o["feat"], ref.feat) and np.array_equal(o["bin"], ref.bin)
        assert np.array_equal(o["leaf"], ref.leaf)


def test_dp_sampled_trees_equal_single_process(tmp_path):
    """Rank 1's rows draw as global rows 1501 ..: row_offset defaults to the lower ranks' row count."""
    from test_distributed import _free_port

    mp.start_processes(_dp_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, start_method="spawn")
    X, y, cuts = _dp_data()
    ref = gb.fit(torch.from_numpy(X), torch.from_numpy(y), gb.GBDTParams(**DP_KW), cuts=cuts)
    assert (ref.feat >= 0).any()
    for r in range(2):
        o = np.load(os.path.join(tmp_path, f"g{r}.npz"))
        assert np.array_equal(o["feat"], ref.feat) and np.array_equal(o["bin"], ref.bin)
        assert np.array_equal(o["leaf"], ref.leaf)
