"""tree_perm.hip and the device scoring path against the numpy oracle, exactly.

Every case drives ops.perm_importance through TreePermutationImportance(ens, 0, 1) (so the raw rows
ARE the standardized rows) and compares margins as uint32 words with
ops/reference_gbdt.permuted_margins_reference -- predict_margin on explicitly permuted copies of the
rows -- and the scorers' ``raw`` as integers with the CPU path.  Shapes are the smallest that cross
the kernel's boundaries: R = TREE_PERM_ROWS rows per workgroup, C = TREE_PERM_CHUNK_TREES trees per
LDS chunk, K = TREE_PERM_COLS columns per workgroup."""
from __future__ import annotations

import functools
from dataclasses import replace

import numpy as np
import pytest
import torch

import _pd_cases as PC
import _perm_cases as QC
import _tree_cases as TC
from fraud_detection_amd.models.explainers import TreePermutationImportance
from fraud_detection_amd.ops import gbdt as gb
from fraud_detection_amd.ops import reference_gbdt as R
from fraud_detection_amd.ops.native import native
from fraud_detection_amd.ops.perm_importance import permutation_scores, permuted_margins

pytestmark = pytest.mark.gpu


def _expl(ens, dev):
    d = ens.n_features
    return TreePermutationImportance(ens, np.zeros(d), np.ones(d), device=str(dev))


def _check(dev, ens, Xs, features=None, n_repeats=2, seed=5, X=None):
    """Device margins of the rows Xs against the oracle; returns the device pair."""
    X = torch.from_numpy(Xs).to(dev) if X is None else X
    pm, base = permuted_margins(X, _expl(ens, dev), features, n_repeats, seed)
    want, wbase = R.permuted_margins_reference(Xs, ens, features, n_repeats, seed)
    assert PC.bits_equal(base, wbase)
    assert PC.bits_equal(pm, want)
    return pm, base


@functools.lru_cache(maxsize=None)
def _tiles():
    m = native()
    return int(m.TREE_PERM_ROWS), int(m.TREE_PERM_CHUNK_TREES), int(m.TREE_PERM_COLS)


def test_tile_constants(dev):
    rows, chunk, cols = _tiles()
    assert rows == 64 and chunk >= 2 and cols >= 2 and cols % 4 == 0


@pytest.mark.parametrize("n", ["1", "R-1", "R", "R+1", "3*R+5"])
def test_rows_around_the_workgroup(dev, n):
    n = int(eval(n, {"R": _tiles()[0]}))
    ens, Xs = PC.random_case(d=4, depth=3, T=5, n=n, seed=21, learn=True, nan_rows=True)
    _check(dev, ens, Xs)


@pytest.mark.parametrize("T", ["1", "2", "C-1", "C", "C+1", "2*C+1"])
def test_trees_around_the_lds_chunk(dev, T):
    T = int(eval(T, {"C": _tiles()[1]}))
    ens, Xs = PC.random_case(d=4, depth=3, T=T, n=70, seed=22, learn=True, nan_rows=True)
    _check(dev, ens, Xs)


@pytest.mark.parametrize("cols", ["K-2", "K-1", "K", "K+1", "3*K+2"])
def test_columns_around_the_column_tile(dev, cols):
    """F x n_repeats permuted columns out of d = 30 features, F the largest divisor of the count that
    is at most 30: with K = 64 that is 2 x 31, 21 x 3, 16 x 4, 13 x 5 and 2 x 97, so a wave's 16
    columns span several features and a tile boundary falls inside one feature's repeats.  The launch
    has one more column, the baseline, after them (K - 2: K - 1 columns in all)."""
    cols = int(eval(cols, {"K": _tiles()[2]}))
    F = max(f for f in range(1, 31) if cols % f == 0)
    reps = cols // F
    ens, Xs = PC.random_case(d=30, depth=4, T=6, n=70, seed=23, learn=True, nan_rows=True)
    pm, _ = _check(dev, ens, Xs, tuple(range(30 - F, 30)), reps)
    assert pm.shape[:2] == (F, reps)


@pytest.mark.parametrize("d", [1, 4, 30])
@pytest.mark.parametrize("depth", [1, 2, 3, 4, 5])
def test_every_depth_and_width(dev, depth, d):
    """Pass-through nodes, thresholds planted on row values, default_left and NaN in every column."""
    ens, Xs = PC.random_case(d=d, depth=depth, T=9, n=70, seed=100 * depth + d, learn=True, nan_rows=True)
    assert ens.has_default_left and np.isnan(Xs).any()
    _check(dev, ens, Xs, n_repeats=1 if d == 30 else 3)


def test_nan_rows_of_a_model_without_default_directions(dev):
    ens, Xs = PC.random_case(d=4, depth=4, T=9, n=70, seed=31, nan_rows=True)
    assert not ens.has_default_left
    _check(dev, ens, Xs)


def test_unused_feature_and_feature_of_every_node(dev):
    ens, Xs = PC.random_case(d=3, depth=3, T=9, n=70, seed=32)
    ens = TC.make_ensemble(3, 3, np.where(ens.feat >= 0, 1, -1), ens.thr, ens.leaf)
    pm, base = _check(dev, ens, Xs)
    assert PC.bits_equal(pm[0], np.stack([base, base])) and PC.bits_equal(pm[2], np.stack([base, base]))
    assert not PC.bits_equal(pm[1, 0], base)
    full = TC.make_ensemble(3, 3, np.ones_like(ens.feat), np.where(np.isinf(ens.thr), 0.25, ens.thr), ens.leaf)
    pm, _ = _check(dev, full, Xs)                                 # no pass-through node either
    donor = R.permutation_donors(70, 5, 1, 0)
    assert PC.bits_equal(pm[1, 0], PC.margin(Xs, full)[donor])    # only feature 1 matters: the donor's margin


def test_strided_rows(dev):
    ens, Xs = PC.random_case(d=4, depth=3, T=9, n=70, seed=35, learn=True, nan_rows=True)
    wide = torch.full((70, 7), float("nan"), device=dev)
    wide[:, :4] = torch.from_numpy(Xs).to(dev)
    view = wide[:, :4]
    assert view.stride(0) == 7
    _check(dev, ens, Xs, X=view)


def test_baseline_is_predict_margin_and_calls_repeat_bit_for_bit(dev):
    ens, Xs = PC.random_case(d=4, depth=5, T=40, n=197, seed=34, learn=True, nan_rows=True)
    pm, base = _check(dev, ens, Xs)
    Xd = torch.from_numpy(Xs).to(dev)
    assert PC.bits_equal(base, gb.predict_margin(Xd, ens).cpu().numpy())
    pm2, base2 = permuted_margins(Xd, _expl(ens, dev), None, 2, 5)
    assert PC.bits_equal(pm2, pm) and PC.bits_equal(base2, base)
    dp, db = permuted_margins(Xd, _expl(ens, dev), None, 2, 5, sync=False)
    assert dp.is_cuda and dp.dtype == torch.float32 and db.is_cuda and PC.bits_equal(dp.cpu().numpy(), pm)
    other, _ = permuted_margins(Xd, _expl(ens, dev), None, 2, 6)
    assert not PC.bits_equal(other, pm)


def test_explainer_standardizes_raw_rows(dev):
    from fraud_detection_amd.models.explainers import _standardize

    ens, Xs = PC.random_case(d=3, depth=3, T=5, n=70, seed=36)
    mean, scale = np.array([1.0, -2.0, 0.5]), np.array([2.0, 0.5, 4.0])
    X = (Xs.astype(np.float64) * scale + mean).astype(np.float32)
    expl = TreePermutationImportance(ens, mean, scale, device=str(dev))
    pm, base = permuted_margins(torch.from_numpy(X).to(dev), expl, None, 2, 1)
    want, wbase = R.permuted_margins_reference(_standardize(X, mean, scale), ens, None, 2, 1)
    assert PC.bits_equal(pm, want) and PC.bits_equal(base, wbase)


@functools.lru_cache(maxsize=None)
def _scoring_case():
    ens, Xs = PC.random_case(d=6, depth=4, T=12, n=1000, seed=37, learn=True, nan_rows=True)
    ens = replace(ens, feat=np.where(ens.feat == 4, -1, ens.feat).astype(np.int32))          # feature 4: unused
    y = QC.labels(Xs, ens, 38)
    return ens, Xs, y


@pytest.mark.parametrize("scoring", ["auc", "aucpr", "logloss"])
def test_scorers_equal_the_cpu_path(dev, scoring):
    ens, Xs, y = _scoring_case()
    raw, base_raw, P = permutation_scores(torch.from_numpy(Xs).to(dev), torch.from_numpy(y).to(dev), _expl(ens, dev),
                                          None, scoring, 3, 7)
    want, wbase, wP = permutation_scores(torch.from_numpy(Xs), torch.from_numpy(y), _expl(ens, "cpu"), None, scoring, 3, 7)
    assert raw.dtype == np.int64 and np.array_equal(raw, want) and base_raw == wbase and P == wP == int(y.sum())
    assert np.all(raw[4] == base_raw) and np.any(raw != base_raw)
    res = _expl(ens, dev).permutation_importance(Xs, y, scoring=scoring, n_repeats=3, seed=7)
    cpu = _expl(ens, "cpu").permutation_importance(Xs, y, scoring=scoring, n_repeats=3, seed=7)
    assert np.array_equal(res.raw, want) and np.array_equal(res.importances, cpu.importances)


@pytest.mark.parametrize("scoring", ["auc", "logloss"])
def test_column_groups_do_not_change_the_table(dev, scoring):
    ens, Xs, y = _scoring_case()
    Xd, yd, expl = torch.from_numpy(Xs).to(dev), torch.from_numpy(y).to(dev), _expl(ens, dev)
    one = permutation_scores(Xd, yd, expl, None, scoring, 3, 7)
    cols = 1 + 5 * 3                                              # the baseline and five used features
    small = 4 * len(y) * 5                                        # five columns per group: four groups
    assert -(-cols // 5) >= 3
    many = permutation_scores(Xd, yd, expl, None, scoring, 3, 7, max_bytes=small)
    each = permutation_scores(Xd, yd, expl, None, scoring, 3, 7, max_bytes=1)      # one column per group
    for got in (many, each):
        assert np.array_equal(got[0], one[0]) and got[1:] == one[1:]
    again = permutation_scores(Xd, yd, expl, None, scoring, 3, 7)
    assert np.array_equal(again[0], one[0]) and again[1:] == one[1:]


def test_an_empty_class_is_refused(dev):
    ens, Xs, y = _scoring_case()
    Xd, expl = torch.from_numpy(Xs).to(dev), _expl(ens, dev)
    for scoring in ("auc", "aucpr"):
        with pytest.raises(ValueError, match="both classes"):
            permutation_scores(Xd, torch.zeros(len(y), dtype=torch.uint8, device=dev), expl, (0,), scoring, 1, 0)
    with pytest.raises(ValueError):
        permutation_scores(Xd, torch.from_numpy(y[:-1]).to(dev), expl, (0,), "auc", 1, 0)


def test_classifier_on_device_equals_the_cpu_classifier(dev):
    import copy

    from fraud_detection_amd.models.gbdt import GBDTClassifier

    rng = np.random.default_rng(0)
    X = rng.normal(size=(500, 4)).astype(np.float32)
    y = (X[:, 0] - X[:, 2] + 0.3 * rng.normal(size=500) > 0).astype(np.uint8)
    m = GBDTClassifier(n_estimators=7, max_depth=3, device="auto").fit(torch.from_numpy(X).to(dev), torch.from_numpy(y).to(dev))
    cpu = copy.deepcopy(m)
    cpu.device = "cpu"
    for scoring in ("auc", "aucpr", "logloss"):
        a = m.permutation_importance(torch.from_numpy(X).to(dev), torch.from_numpy(y).to(dev), scoring=scoring, n_repeats=3)
        b = cpu.permutation_importance(X, y, scoring=scoring, n_repeats=3)
        assert np.array_equal(a.raw, b.raw) and a.baseline_raw == b.baseline_raw
        assert np.array_equal(a.importances, b.importances) and a.features == b.features
    head = m.permutation_importance(torch.from_numpy(X).to(dev), torch.from_numpy(y).to(dev), iteration_range=(0, 2))
    want, wbase = QC.oracle_raw(X, y, m.ensemble.head(2), (0, 1, 2, 3), 5, 0, "auc")
    assert np.array_equal(head.raw, want) and head.baseline_raw == wbase
