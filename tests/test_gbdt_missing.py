"""missing_policy="learn": a learned default direction for NaN (sparsity-aware split finding).

CPU side: the oracle (ops/reference_gbdt.py, also the CPU execution path) against a brute force
over the ROWS written here, the public interface, the round trips and the refusals.  Everything is
compared exactly (integers, or floats bit for bit)."""
from __future__ import annotations

import json
import os
import pickle

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from fraud_detection_amd.models.gbdt import GBDTClassifier, GBDTPipeline
from fraud_detection_amd.ops import gbdt as gb
from fraud_detection_amd.ops import reference_gbdt as R

NEG_NAN = np.array([0xFFC00001], np.uint32).view(np.float32)[0]
TREE_KEYS = ("feat", "bin", "thr", "gain", "leaf")


def _same_trees(a, b, keys=TREE_KEYS):
    return all(getattr(a, k).tobytes() == getattr(b, k).tobytes() for k in keys)


def _dl(ens):
    return np.zeros_like(ens.feat, dtype=np.uint8) if ens.default_left is None else ens.default_left


# ---- the oracle against a brute force over the rows ---------------------------------------------------
def _brute_tree(bins, q, nbins, depth, lam, mcw, gamma, eta, ginv, hinv):
    """Every (feature, b, direction) of every node by partitioning the node's rows directly: int64
    sums of the quantised gradients, then the gain in the documented fp64 order.  Candidates are
    tried in tie order and replaced only by a strictly larger gain."""
    n, d = bins.shape[0], len(nbins)
    ni = (1 << depth) - 1
    feat, binv, dleft = np.full(ni, -1), np.full(ni, 255), np.zeros(ni, np.uint8)
    gain = np.zeros(ni)
    sums = {}
    rows_of = {0: np.arange(n)}
    g, h = q[:, 0].astype(np.int64), q[:, 1].astype(np.int64)

    def term(Gq, Hq):
        G, H = float(Gq) * ginv, float(Hq) * hinv
        return G * G / (H + lam) if H + lam > 0.0 else 0.0

    for node in range(ni):
        rows = rows_of[node]
        Gq, Hq = int(g[rows].sum()), int(h[rows].sum())
        if node == 0:
            sums[0] = (Gq, Hq)
        best = (-np.inf, None)
        for f in range(d):
            v = bins[rows, f].astype(np.int64)
            miss = v == 255
            cands = [(-1, 1, miss)]
            for b in range(int(nbins[f]) - 1):
                cands.append((b, 0, (v <= b) & ~miss))
                cands.append((b, 1, (v <= b) | miss))
            for b, dl, left in cands:
                GLq, HLq = int(g[rows][left].sum()), int(h[rows][left].sum())
                if float(HLq) * hinv >= mcw and float(Hq - HLq) * hinv >= mcw:
                    gn = (term(GLq, HLq) + term(Gq - GLq, Hq - HLq)) - term(Gq, Hq)
                    if gn > best[0]:
                        best = (gn, (f, b, dl, left, GLq, HLq))
        lc, rc = 2 * node + 1, 2 * node + 2
        if best[1] is not None and best[0] > 1e-6 and not best[0] < gamma:
            f, b, dl, left, GLq, HLq = best[1]
            feat[node], binv[node], dleft[node], gain[node] = f, b, dl, best[0]
            rows_of[lc], rows_of[rc] = rows[left], rows[~left]
            sums[lc], sums[rc] = (GLq, HLq), (Gq - GLq, Hq - HLq)
        else:
            rows_of[lc], rows_of[rc] = rows, rows[:0]
            sums[lc], sums[rc] = (Gq, Hq), (0, 0)
    leaf = np.zeros(1 << depth, np.float32)
    where = np.zeros(n, np.int64)
    for i in range(1 << depth):
        G, H = float(sums[ni + i][0]) * ginv, float(sums[ni + i][1]) * hinv
        leaf[i] = np.float32(eta * (0.0 if (H < mcw or H <= 0.0) else -G / (H + lam)))
        where[rows_of[ni + i]] = i
    return feat, binv, dleft, gain, leaf, where


@pytest.mark.parametrize("reg", [(0.0, 0.0, 0.0), (0.0, 1.0, 0.0), (1.0, 0.0, 0.0), (1.0, 1.0, 0.5), (2.5, 1.0, 0.0)],
                         ids=lambda r: "l%g_w%g_g%g" % r)
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_build_tree_matches_row_brute_force(reg, seed):
    lam, mcw, gamma = reg
    rng = np.random.default_rng(seed)
    n, d, depth = (60, 3, 3) if seed else (23, 2, 2)
    X = rng.integers(-3, 4, size=(n, d)).astype(np.float32)  # few distinct values: ties between candidates
    X[rng.random(n) < 0.3, 0] = np.nan
    X[:, 1] = np.nan                      # entirely missing
    if d > 2:
        X[rng.random(n) < 0.2, 2] = np.inf  # NaN-free, with an infinity
    cuts, nbins = R.quantile_cuts(X, 6, missing=True)
    assert nbins[1] == 1
    bins = R.bin_rows(X, cuts, nbins, missing=True)
    gs, hs = R.grad_scales(1.0)
    q = np.stack([rng.integers(-(1 << 14), (1 << 14) + 1, n), rng.integers(0, (1 << 14) + 1, n)], 1).astype(np.int32)
    q[rng.random(n) < 0.2, 1] = 0  # zero-Hessian rows: reg_lambda = 0 meets a zero denominator
    tr, node = R.build_tree(bins, q, cuts, nbins, depth, lam, mcw, gamma, 0.3, gs, hs, missing=True)
    feat, binv, dleft, gain, leaf, where = _brute_tree(bins[:, :d], q, nbins, depth, lam, mcw, gamma, 0.3, 1 / gs, 1 / hs)
    assert np.array_equal(tr.feat, feat) and np.array_equal(tr.bin, binv), (tr.feat, feat, tr.bin, binv)
    assert np.array_equal(tr.default_left, dleft)
    assert tr.gain.tobytes() == gain.tobytes()
    assert tr.leaf.tobytes() == leaf.tobytes()
    assert np.array_equal(node, where)
    split = tr.feat >= 0
    assert np.array_equal(np.isneginf(tr.thr), split & (tr.bin == -1))
    assert np.all(tr.thr[split & (tr.bin >= 0)] == cuts[tr.feat, np.maximum(tr.bin, 0)][split & (tr.bin >= 0)])


def test_brute_force_cases_use_every_candidate_kind():
    """The cases above are not vacuous: b = -1 splits, default-left and missing-right splits occur."""
    kinds = set()
    for seed in (0, 1, 2):
        rng = np.random.default_rng(seed)
        n, d, depth = (60, 3, 3) if seed else (23, 2, 2)
        X = rng.integers(-3, 4, size=(n, d)).astype(np.float32)
        X[rng.random(n) < 0.3, 0] = np.nan
        cuts, nbins = R.quantile_cuts(X, 6, missing=True)
        bins = R.bin_rows(X, cuts, nbins, missing=True)
        y = (np.isnan(X[:, 0]) ^ (rng.random(n) < 0.2)).astype(np.uint8)
        q = R.gradients(np.zeros(n, np.float32), y, 1.0, *R.grad_scales(1.0))
        tr, _ = R.build_tree(bins, q, cuts, nbins, depth, 0.0, 0.0, 0.0, 0.3, *R.grad_scales(1.0), missing=True)
        for f, b, dl in zip(tr.feat, tr.bin, tr.default_left):
            if f >= 0:
                kinds.add("present|missing" if b < 0 else ("left" if dl else "right"))
    assert kinds == {"present|missing", "left", "right"}, kinds


# ---- NaN-free data: "learn" is "last_bin" ----------------------------------------------------------------
def _plain(n=700, d=5, seed=3):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, d)).astype(np.float32)
    y = (X[:, 0] + 0.5 * X[:, 1] ** 2 + rng.normal(size=n) > 1.0).astype(np.uint8)
    return X, y


@pytest.mark.parametrize("max_bin", [2, 37, 255])
def test_nan_free_learn_equals_last_bin(max_bin):
    X, y = _plain()
    Xt, yt = torch.from_numpy(X), torch.from_numpy(y)
    kw = dict(n_estimators=5, max_depth=4, max_bin=max_bin)
    a, ma = gb.fit(Xt, yt, gb.GBDTParams(**kw), return_margin=True)
    b, mb = gb.fit(Xt, yt, gb.GBDTParams(missing_policy="learn", **kw), return_margin=True)
    assert (a.feat >= 0).any()
    assert _same_trees(a, b) and np.array_equal(ma.numpy(), mb.numpy())
    assert not np.any(_dl(b)) and not b.has_default_left
    da, db = a.to_dict(), b.to_dict()
    assert set(da) == set(db)
    for k in da:
        if k != "params":
            assert da[k] == db[k], k
    assert "missing_policy" not in da["params"] and db["params"]["missing_policy"] == "learn"


# ---- crafted signals -----------------------------------------------------------------------------------------
def _fit1(X, y, policy, depth=1, max_bin=16):
    p = gb.GBDTParams(n_estimators=1, max_depth=depth, max_bin=max_bin, missing_policy=policy, learning_rate=1.0)
    return gb.fit(torch.from_numpy(X), torch.from_numpy(y), p, return_margin=True)


def test_signal_is_missingness():
    rng = np.random.default_rng(0)
    X = rng.normal(size=(400, 2)).astype(np.float32)
    X[rng.random(400) < 0.3, 0] = np.nan
    y = np.isnan(X[:, 0]).astype(np.uint8)  # x0's largest values are class 0
    ens, m = _fit1(X, y, "learn")
    assert (ens.feat[0, 0], ens.bin[0, 0], ens.default_left[0, 0]) == (0, -1, 1) and np.isneginf(ens.thr[0, 0])
    assert np.array_equal(m.numpy() > 0, y != 0)
    old, mo = _fit1(X, y, "last_bin")
    assert not np.array_equal(mo.numpy() > 0, y != 0)  # NaN shares the last bin with the largest values
    assert old.default_left is None


@pytest.mark.parametrize("high", [False, True], ids=["nan_low_side", "nan_high_side"])
def test_signal_missing_joins_one_side(high):
    rng = np.random.default_rng(1)
    X = rng.normal(size=(600, 2)).astype(np.float32)
    X[:, 0] = rng.choice(np.array([-3, -2, -1, 1, 2, 3], np.float32), 600)
    X[rng.random(600) < 0.25, 0] = np.nan
    y = (((X[:, 0] > 0) if high else (X[:, 0] < 0)) | np.isnan(X[:, 0])).astype(np.uint8)
    ens, m = _fit1(X, y, "learn")
    # the cut nearest 0: x < 1 <=> x < 0 on these values
    assert (ens.feat[0, 0], ens.thr[0, 0], ens.default_left[0, 0]) == (0, 1.0, 0 if high else 1)
    assert ens.cuts[0, ens.bin[0, 0]] == 1.0
    assert np.array_equal(m.numpy() > 0, y != 0)


# ---- train / predict consistency ---------------------------------------------------------------------------
def _messy(n=900, d=4, seed=5, max_bin=12):
    """NaN of both signs, +-inf, -0.0 and values exactly on cuts; feature 3's missingness carries
    signal, so present-versus-missing splits occur."""
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, d)).astype(np.float32)
    X[rng.random(n) < 0.15, 0] = np.nan
    X[rng.random(n) < 0.1, 0] = NEG_NAN
    X[rng.random(n) < 0.05, 1] = np.inf
    X[rng.random(n) < 0.05, 1] = -np.inf
    X[rng.random(n) < 0.1, 1] = np.nan
    X[rng.random(n) < 0.1, 2] = -0.0
    X[rng.random(n) < 0.1, 2] = 0.0
    X[rng.random(n) < 0.3, 3] = NEG_NAN
    X[rng.random(n) < 0.02, 3] = np.inf
    X[rng.random(n) < 0.02, 3] = -np.inf
    y = (np.isnan(X[:, 3]) ^ (np.nan_to_num(X[:, 0], nan=1.0, posinf=0, neginf=0) > 0.3)).astype(np.uint8)
    cuts = R.quantile_cuts(X, max_bin, missing=True)
    for f in range(d):  # values exactly on cuts
        fin = cuts[0][f, :cuts[1][f] - 1]
        if len(fin):
            idx = rng.choice(n, 40, replace=False)
            keep = ~np.isnan(X[idx, f])
            X[idx[keep], f] = rng.choice(fin, int(keep.sum()))
    return X, y, cuts


def test_predict_on_rows_equals_fit_margin():
    X, y, cuts = _messy()
    p = gb.GBDTParams(n_estimators=8, max_depth=4, max_bin=12, missing_policy="learn", min_child_weight=0.0)
    ens, margin = gb.fit(torch.from_numpy(X), torch.from_numpy(y), p, cuts=cuts, return_margin=True)
    split = ens.feat >= 0
    assert (split & (ens.bin == -1)).any() and (split & (ens.bin >= 0) & (ens.default_left == 1)).any()
    assert (split & (ens.default_left == 0)).any()
    got = gb.predict_margin(torch.from_numpy(X), ens)
    assert got.numpy().tobytes() == margin.numpy().tobytes()
    for k in (0, 3):
        part = gb.predict_margin(torch.from_numpy(X), ens, n_trees=k).numpy()
        bins = R.bin_rows(X, *cuts, missing=True)
        ref = R.predict_margin_bins(bins, ens.feat[:k], ens.bin[:k], ens.leaf[:k], ens.depth, ens.base_margin,
                                    ens.default_left[:k])
        assert part.tobytes() == ref.tobytes()


def test_bin_words_round_trip_and_walk_rule():
    """The device's split words: old words keep their meaning, and the one-line walk rule equals the
    direction rule for every (byte, bin, direction)."""
    b = np.array([-1, 0, 5, 253, 0, 17, 253, 255, -1], np.int32)  # the last two: pass-through, "all right"
    dl = np.array([1, 1, 1, 1, 0, 0, 0, 0, 0], np.uint8)
    w = gb.encode_bin_words(b, dl)
    assert np.array_equal(w[4:], b[4:]) and np.all(w[:4] >= 0x200)
    b2, dl2 = gb.decode_bin_words(w)
    assert np.array_equal(b2, b) and np.array_equal(dl2, dl)
    assert gb.encode_bin_words(b[4:], None) is not None and np.array_equal(gb.encode_bin_words(b[4:], None), b[4:])
    v = np.arange(256)[:, None]
    s = ((w.astype(np.uint32) >> 9) == 1).astype(np.int64)
    walk = ((v + s) & 0xFF) > (w - (s << 9))
    assert np.array_equal(walk, R.bins_go_right(v, b[None, :], dl[None, :]))
    assert np.array_equal(walk[:, 4:], v > b[None, 4:])  # the old words: v > w, byte 255 included


# ---- cuts --------------------------------------------------------------------------------------------------------
def test_cuts_skip_nan():
    rng = np.random.default_rng(7)
    X = rng.normal(size=(5000, 4)).astype(np.float32)
    clean = X.copy()
    X[rng.random(5000) < 0.3, 0] = np.nan
    X[rng.random(5000) < 0.3, 0] = NEG_NAN
    X[:, 2] = np.nan
    for max_bin in (2, 37, 256):
        cuts, nbins = R.quantile_cuts(X, max_bin, missing=True)
        B = min(max_bin, 255)
        assert nbins.max() <= 255 and nbins[2] == 1 and np.all(np.isposinf(cuts[2]))
        for f in (0, 1, 3):  # the cuts of the feature's non-NaN values alone
            col = X[:, f][~np.isnan(X[:, f])]
            one, nb1 = R.quantile_cuts(col[:, None], B)
            assert nbins[f] == nb1[0] and np.array_equal(cuts[f], one[0])
        assert not np.isnan(cuts).any()
    c255, n255 = R.quantile_cuts(clean, 255, missing=True)
    r255, m255 = R.quantile_cuts(clean, 255)
    assert np.array_equal(c255, r255) and np.array_equal(n255, m255)
    assert R.quantile_cuts(clean, 256, missing=True)[1].max() == 255 and R.quantile_cuts(clean, 256)[1].max() == 256
    e_c, e_n = R.quantile_cuts(np.zeros((0, 3), np.float32), 16, missing=True)
    assert np.all(e_n == 1) and np.all(np.isposinf(e_c))


def test_nan_outside_the_cut_sample():
    """A feature whose NaN lie outside the strided sample: NaN-free cuts, and its NaN rows still take
    the missing slot and a learned side."""
    rng = np.random.default_rng(8)
    X = rng.normal(size=(1000, 2)).astype(np.float32)
    odd = np.arange(1000) % 2 == 1
    X[odd & (rng.random(1000) < 0.5), 0] = np.nan
    y = np.isnan(X[:, 0]).astype(np.uint8)
    Xt = torch.from_numpy(X)
    cuts = gb.quantile_cuts(Xt, 16, sample_rows=500, missing=True)  # rows 0, 2, 4, ...
    ref = R.quantile_cuts(X[::2], 16)
    assert np.array_equal(cuts[0], ref[0]) and np.array_equal(cuts[1], ref[1])
    bins = gb.bin_rows(Xt, *cuts, missing=True).numpy()
    assert np.array_equal(bins[:, 0] == 255, np.isnan(X[:, 0])) and bins[~np.isnan(X[:, 0]), 0].max() < cuts[1][0]
    p = gb.GBDTParams(n_estimators=1, max_depth=1, max_bin=16, missing_policy="learn", cut_sample_rows=500)
    ens = gb.fit(Xt, torch.from_numpy(y), p)
    assert (ens.feat[0, 0], ens.bin[0, 0], ens.default_left[0, 0]) == (0, -1, 1)


def test_bin_rows_missing_slot():
    X, _, cuts = _messy()
    old = R.bin_rows(X, *cuts)
    new = R.bin_rows(X, *cuts, missing=True)
    nan = np.isnan(X)
    assert np.all(new[:, :4][nan] == 255) and np.array_equal(new[:, :4][~nan], old[:, :4][~nan])
    assert not new[:, 4:].any()
    with pytest.raises(ValueError):
        gb.fit_binned(torch.from_numpy(new), torch.zeros(len(X), dtype=torch.uint8),
                      (cuts[0], np.full(4, 256, np.int32)), gb.GBDTParams(missing_policy="learn"))


# ---- round trips ---------------------------------------------------------------------------------------------------
def _learned(n_estimators=6):
    X, y, _ = _messy(seed=9)
    m = GBDTClassifier(n_estimators=n_estimators, max_depth=3, max_bin=12, min_child_weight=0.0,
                       missing_policy="learn", device="cpu").fit(X, y)
    assert (m.ensemble.bin == -1).any() and m.ensemble.has_default_left
    return m, X, y


def test_json_and_pickle_round_trip(tmp_path):
    m, X, _ = _learned()
    assert m.get_params()["missing_policy"] == "learn"
    o = m.ensemble.to_dict()
    txt = json.dumps(o)
    assert '"-inf"' in txt and "default_left" in o and "NaN" not in txt and "Infinity" not in txt
    back = gb.TreeEnsemble.from_dict(json.loads(txt))
    assert _same_trees(back, m.ensemble) and np.array_equal(back.default_left, m.ensemble.default_left)
    path = str(tmp_path / "m.json")
    m.save_model(path)
    m2 = GBDTClassifier.load_model(path, device="cpu")
    assert m2.params == m.params and m2.params.missing_policy == "learn"
    assert m2.predict_margin(X).tobytes() == m.predict_margin(X).tobytes()
    m3 = pickle.loads(pickle.dumps(m))
    assert m3.params == m.params and m3.predict_margin(X).tobytes() == m.predict_margin(X).tobytes()
    assert np.array_equal(m3.ensemble.default_left, m.ensemble.default_left)


def test_old_json_and_old_pickle_state_load_unchanged(tmp_path):
    X, y, _ = _messy(seed=9)
    m = GBDTClassifier(n_estimators=4, max_depth=3, max_bin=12, device="cpu").fit(X, y)
    want = m.predict_margin(X)
    o = m.ensemble.to_dict()
    assert "default_left" not in o and "missing_policy" not in o["params"]
    assert all(v != "-inf" for row in o["thr"] for v in row)
    path = str(tmp_path / "old.json")
    m.save_model(path)
    old = GBDTClassifier.load_model(path, device="cpu")
    assert old.params.missing_policy == "last_bin" and old.ensemble.default_left is None
    assert old.predict_margin(X).tobytes() == want.tobytes()
    st = m.__getstate__()
    st["params"].pop("missing_policy")
    ens = pickle.loads(pickle.dumps(st["ensemble"]))
    del ens.__dict__["default_left"]  # a TreeEnsemble pickled before the field existed
    st["ensemble"] = ens
    old = GBDTClassifier.__new__(GBDTClassifier)
    old.__setstate__(st)
    assert old.params.missing_policy == "last_bin" and not old.ensemble.has_default_left
    assert old.predict_margin(X).tobytes() == want.tobytes()
    assert old.ensemble.to_dict() == o


def test_checkpoint_resume_equals_uninterrupted(tmp_path):
    from fraud_detection_amd.utils.checkpoint import CheckpointManager, load_checkpoint

    X, y, cuts = _messy(seed=9)
    Xt, yt = torch.from_numpy(X), torch.from_numpy(y)
    kw = dict(max_depth=3, max_bin=12, min_child_weight=0.0, missing_policy="learn")
    full = gb.fit(Xt, yt, gb.GBDTParams(n_estimators=6, **kw), cuts=cuts)
    mgr = CheckpointManager(str(tmp_path), prefix="g")
    gb.fit(Xt, yt, gb.GBDTParams(n_estimators=3, **kw), cuts=cuts, checkpoint=mgr, checkpoint_every=3)
    tensors, _ = load_checkpoint(str(tmp_path / "g-3.safetensors"))
    assert np.array_equal(tensors["default_left"].numpy(), full.default_left[:3])
    assert np.array_equal(tensors["bin"].numpy(), full.bin[:3])
    assert full.default_left[:3].any()
    saved = []
    save = mgr.save
    mgr.save = lambda step, *a, **k: (saved.append(step), save(step, *a, **k))[1]
    res = gb.fit(Xt, yt, gb.GBDTParams(n_estimators=6, **kw), cuts=cuts, checkpoint=mgr, checkpoint_every=1)
    assert saved == [4, 5, 6]
    assert _same_trees(res, full) and np.array_equal(res.default_left, full.default_left)
    # the policy is part of the signature: a "last_bin" fit does not pick these checkpoints up
    other = gb.fit(Xt, yt, gb.GBDTParams(n_estimators=6, **{**kw, "missing_policy": "last_bin"}), cuts=cuts,
                   checkpoint=mgr, checkpoint_every=6)
    assert _same_trees(other, gb.fit(Xt, yt, gb.GBDTParams(n_estimators=6, **{**kw, "missing_policy": "last_bin"}),
                                     cuts=cuts))


# ---- composition ---------------------------------------------------------------------------------------------------
def test_composes_with_sampling_weights_hole_and_eval():
    X, y, cuts = _messy(seed=11)
    n = len(X)
    Xt, yt = torch.from_numpy(X), torch.from_numpy(y)
    kw = dict(n_estimators=5, max_depth=3, max_bin=12, min_child_weight=0.0, missing_policy="learn")
    base, mb = gb.fit(Xt, yt, gb.GBDTParams(**kw), cuts=cuts, return_margin=True)
    # sampling: deterministic, a different model, margins still those of the fp32 walk
    for extra in (dict(subsample=0.6, seed=3), dict(colsample_bynode=0.5, seed=3)):
        a, ma = gb.fit(Xt, yt, gb.GBDTParams(**kw, **extra), cuts=cuts, return_margin=True)
        b = gb.fit(Xt, yt, gb.GBDTParams(**kw, **extra), cuts=cuts)
        assert _same_trees(a, b) and np.array_equal(a.default_left, b.default_left) and not _same_trees(a, base)
        assert gb.predict_margin(Xt, a).numpy().tobytes() == ma.numpy().tobytes()
    # unit weights are no weights; other weights change the model
    w1, m1 = gb.fit(Xt, yt, gb.GBDTParams(**kw), cuts=cuts, return_margin=True, sample_weight=torch.ones(n))
    assert _same_trees(w1, base) and np.array_equal(w1.default_left, base.default_left)
    w2, m2 = gb.fit(Xt, yt, gb.GBDTParams(**kw), cuts=cuts, return_margin=True,
                    sample_weight=torch.from_numpy(np.where(y != 0, 3.0, 0.5).astype(np.float32)))
    assert gb.predict_margin(Xt, w2).numpy().tobytes() == m2.numpy().tobytes() and not _same_trees(w2, base)
    # hole: the trees of the rows outside it, the margins of every row
    bins = gb.bin_rows(Xt, *cuts, missing=True)
    keep = np.r_[0:200, 350:n]
    h, mh = gb.fit_binned(bins, yt, cuts, gb.GBDTParams(**kw), hole=(200, 150), return_margin=True)
    ref = gb.fit(torch.from_numpy(X[keep]), torch.from_numpy(y[keep]), gb.GBDTParams(**kw), cuts=cuts)
    assert _same_trees(h, ref) and np.array_equal(h.default_left, ref.default_left)
    assert gb.predict_margin(Xt, h).numpy().tobytes() == mh.numpy().tobytes()
    # eval rows given as floats with NaN, and the hole as the eval set with early stopping
    Xv, yv = Xt[:300].clone(), yt[:300].clone()
    e, rec = gb.fit(Xt, yt, gb.GBDTParams(**kw), cuts=cuts, eval_set=(Xv, yv))
    assert _same_trees(e, base)
    for t in (0, 4):
        want = R.eval_record(gb.predict_margin(Xv, e, n_trees=t + 1).numpy(), yv.numpy())
        assert np.array_equal(rec.records[t], want)
    s, ms, rs = gb.fit_binned(bins, yt, cuts, gb.GBDTParams(**{**kw, "n_estimators": 30, "learning_rate": 0.8}),
                              hole=(200, 150), eval_set="hole", early_stopping_rounds=2, return_margin=True)
    assert s.n_trees == rs.best_iteration + 1
    assert gb.predict_margin(Xt, s).numpy().tobytes() == ms.numpy().tobytes()
    want = R.eval_record(ms.numpy()[200:350], y[200:350])
    assert np.array_equal(rs.records[rs.best_iteration], want)


# ---- refusals ------------------------------------------------------------------------------------------------------
def test_refusals():
    from fraud_detection_amd.models.explainers import TreeExplainer, TreeKernelExplainer
    from fraud_detection_amd.models.gbdt_cv import DeviceGBDTCV

    with pytest.raises(ValueError, match="missing_policy"):
        gb.GBDTParams(missing_policy="median").validate()
    with pytest.raises(ValueError, match="missing_policy"):
        GBDTClassifier(missing_policy="zero", device="cpu").fit(*_plain()[:2])
    assert gb.GBDTParams().missing_policy == "last_bin" and gb.GBDTParams(missing_policy="learn").validate()
    m, X, _ = _learned()
    d = X.shape[1]
    bg = np.nan_to_num(X[:16], nan=0.0, posinf=1.0, neginf=-1.0)
    for cls in (TreeExplainer, TreeKernelExplainer):
        with pytest.raises(NotImplementedError, match="missing"):
            cls(m.ensemble, np.zeros(d), np.ones(d), bg, device="cpu")
    # an ensemble fitted under "learn" without any default-left node is an ordinary ensemble
    Xp, yp = _plain(200, 4)
    plain = GBDTClassifier(n_estimators=2, max_depth=2, missing_policy="learn", device="cpu").fit(Xp, yp)
    TreeExplainer(plain.ensemble, np.zeros(4), np.ones(4), Xp[:8], device="cpu")
    p = gb.GBDTParams(missing_policy="learn")
    with pytest.raises(NotImplementedError, match="missing_policy"):
        GBDTPipeline(params=p)
    with pytest.raises(NotImplementedError, match="missing_policy"):
        DeviceGBDTCV(params=p)
    GBDTPipeline(params=gb.GBDTParams())


def test_train_entry_point_points_to_the_policy():
    import inspect

    from fraud_detection_amd import train

    src = inspect.getsource(train)
    assert 'missing_policy="learn"' in src and "impute before training" in src


# ---- data parallel -------------------------------------------------------------------------------------------------
DP_KW = dict(n_estimators=4, max_depth=3, max_bin=32, min_child_weight=0.0, missing_policy="learn")


def _dp_data():
    X, y, _ = _messy(n=1201, seed=13, max_bin=32)
    return X, y


def _dp_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    from fraud_detection_amd.parallel.comm import Communicator

    comm = Communicator(backend="gloo")
    X, y = _dp_data()
    sh = slice(0, 601) if rank == 0 else slice(601, 1201)
    # no cuts given: the per-feature non-NaN counts come from the gathered sample
    ens = gb.fit(torch.from_numpy(X[sh].copy()), torch.from_numpy(y[sh].copy()), gb.GBDTParams(**DP_KW), comm=comm)
    np.savez(os.path.join(out_dir, f"m{rank}.npz"), feat=ens.feat, bin=ens.bin, leaf=ens.leaf, thr=ens.thr,
             dl=ens.default_left, cuts=ens.cuts)
    comm.close()


def test_dp_learn_equals_single_process(tmp_path):
    from test_distributed import _free_port

    mp.start_processes(_dp_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, start_method="spawn")
    X, y = _dp_data()
    ref = gb.fit(torch.from_numpy(X), torch.from_numpy(y), gb.GBDTParams(**DP_KW))
    assert ref.has_default_left
    for r in range(2):
        o = np.load(os.path.join(tmp_path, f"m{r}.npz"))
        assert np.array_equal(o["cuts"], ref.cuts)
        assert np.array_equal(o["feat"], ref.feat) and np.array_equal(o["bin"], ref.bin)
        assert np.array_equal(o["dl"], ref.default_left) and o["leaf"].tobytes() == ref.leaf.tobytes()
        assert o["thr"].tobytes() == ref.thr.tobytes()
