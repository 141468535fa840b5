"""tree_pd.hip on the device against the numpy oracle, bit for bit.

Every case drives ops.pdp.partial_dependence through TreePartialDependence(ens, 0, 1) (so the raw
rows ARE the standardized rows) and compares pd_q as integers and ICE as uint32 words with
ops/reference_gbdt.partial_dependence_reference -- predict_margin on modified copies of the rows.
Shapes are the smallest that cross the kernel's boundaries: R = TREE_PD_ROWS rows per workgroup,
C = TREE_PD_CHUNK_TREES trees per LDS chunk, TREE_PD_CELLS cells per workgroup."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import _pd_cases as PC
import _tree_cases as TC
from fraud_detection_amd.models.explainers import TreePartialDependence
from fraud_detection_amd.ops import reference_gbdt as R
from fraud_detection_amd.ops.native import native
from fraud_detection_amd.ops.pdp import partial_dependence

pytestmark = pytest.mark.gpu


def _expl(ens, dev):
    d = ens.n_features
    return TreePartialDependence(ens, np.zeros(d), np.ones(d), device=str(dev))


def _check(dev, ens, Xs, features, expl=None):
    """Device (pd_q, ice) of the rows Xs against the oracle; returns the device pair."""
    expl = expl if expl is not None else _expl(ens, dev)
    q, ice = partial_dependence(torch.from_numpy(Xs).to(dev), expl, features, ice=True)
    want_q, want_ice = R.partial_dependence_reference(Xs, ens, features)
    assert q.dtype == np.int64 and np.array_equal(q, want_q), features
    assert PC.bits_equal(ice, want_ice), features
    return q, ice


@functools.lru_cache(maxsize=None)
def _tiles():
    m = native()
    return int(m.TREE_PD_ROWS), int(m.TREE_PD_CHUNK_TREES), int(m.TREE_PD_CELLS)


def test_tile_constants(dev):
    rows, chunk, cells = _tiles()
    assert rows == 64 and chunk >= 2 and cells >= 2 and int(native().TREE_PD_MAX_CELLS) == R.PD_MAX_CELLS


@pytest.mark.parametrize("n", ["1", "R-1", "R", "R+1", "3*R+5"])
def test_rows_around_the_workgroup(dev, n):
    n = int(eval(n, {"R": _tiles()[0]}))
    ens, Xs = PC.random_case(d=4, depth=3, T=5, n=n, seed=21, learn=True, nan_rows=True)
    _check(dev, ens, Xs, 0)
    _check(dev, ens, Xs, (3, 1))


@pytest.mark.parametrize("T", ["1", "2", "C-1", "C", "C+1", "2*C+1"])
def test_trees_around_the_lds_chunk(dev, T):
    T = int(eval(T, {"C": _tiles()[1]}))
    ens, Xs = PC.random_case(d=4, depth=3, T=T, n=70, seed=22)
    _check(dev, ens, Xs, 2)


@pytest.mark.parametrize("cells", ["K-1", "K", "K+1", "3*K+2"])
def test_cells_around_the_cell_tile(dev, cells):
    cells = int(eval(cells, {"K": _tiles()[2]}))
    ens = PC.cap_ensemble(cells - 1, 3)
    Xs = np.random.default_rng(23).normal(size=(70, 3)).astype(np.float32)
    assert len(R.pd_cells(ens, 0)[0]) == cells
    _check(dev, ens, Xs, 0)


@pytest.mark.parametrize("d", [1, 4, 30])
@pytest.mark.parametrize("depth", [1, 2, 3, 4, 5])
def test_every_depth_and_width(dev, depth, d):
    """A learn model with NaN in every column: the missing cell, and NaN routed by default_left in
    the columns that are not overridden."""
    ens, Xs = PC.random_case(d=d, depth=depth, T=9, n=70, seed=100 * depth + d, learn=True, nan_rows=True)
    assert ens.has_default_left and np.isnan(Xs).any()
    q, ice = _check(dev, ens, Xs, 0)
    assert ice.shape[1] == len(R.pd_grid(ens, 0)) + 2
    if d > 1:
        _check(dev, ens, Xs, (d - 1, 0))


def test_nan_rows_of_a_model_without_default_directions(dev):
    ens, Xs = PC.random_case(d=4, depth=4, T=9, n=70, seed=31, nan_rows=True)
    assert not ens.has_default_left
    q, ice = _check(dev, ens, Xs, 1)
    assert ice.shape[1] == len(R.pd_grid(ens, 1)) + 1            # no missing cell


def test_unused_feature_and_feature_of_every_node(dev):
    ens, Xs = PC.random_case(d=3, depth=3, T=9, n=70, seed=32)
    ens = TC.make_ensemble(3, 3, np.where(ens.feat >= 0, 1, -1), ens.thr, ens.leaf)
    q, ice = _check(dev, ens, Xs, 2)                              # no tree uses it: one cell, the margin
    assert ice.shape == (70, 1) and PC.bits_equal(ice[:, 0], PC.margin(Xs, ens))
    q1, ice1 = _check(dev, ens, Xs, 1)                            # every split node is overridden
    assert np.all(ice1 == ice1[:1])                              # so the rows no longer matter
    qa, _ = _check(dev, ens, Xs, (1, 2))                          # pairs with the unused feature
    qb, _ = _check(dev, ens, Xs, (2, 1))
    assert np.array_equal(qa, q1) and np.array_equal(qb, q1)
    full = TC.make_ensemble(3, 3, np.ones_like(ens.feat), np.where(np.isinf(ens.thr), 0.25, ens.thr), ens.leaf)
    _check(dev, full, Xs, 1)                                      # no pass-through node either


def test_pair_at_the_cell_cap(dev):
    ens = PC.cap_ensemble(255, 255)
    Xs = np.random.default_rng(33).normal(size=(2, 3)).astype(np.float32)
    q, ice = _check(dev, ens, Xs, (0, 1))
    assert q.shape == (R.PD_MAX_CELLS,)
    with pytest.raises(ValueError, match="cells"):
        partial_dependence(torch.from_numpy(Xs).to(dev), _expl(PC.cap_ensemble(256, 255), dev), (0, 1))


def test_ice_is_optional_and_calls_repeat_bit_for_bit(dev):
    ens, Xs = PC.random_case(d=4, depth=5, T=40, n=197, seed=34, learn=True, nan_rows=True)
    expl = _expl(ens, dev)
    q, ice = _check(dev, ens, Xs, 0, expl)
    Xd = torch.from_numpy(Xs).to(dev)
    q0, none = partial_dependence(Xd, expl, 0)
    assert none is None and np.array_equal(q0, q)
    q2, ice2 = partial_dependence(Xd, expl, 0, ice=True)
    assert np.array_equal(q2, q) and PC.bits_equal(ice2, ice)
    dq, dice = partial_dependence(Xd, expl, 0, ice=True, sync=False)
    assert dq.is_cuda and dq.dtype == torch.int64 and dice.is_cuda and np.array_equal(dq.cpu().numpy(), q)
    qe, ie = partial_dependence(Xd[:0], expl, 0, ice=True)
    assert not qe.any() and ie.shape == (0, len(q))


def test_strided_rows(dev):
    ens, Xs = PC.random_case(d=4, depth=3, T=9, n=70, seed=35)
    wide = torch.full((70, 7), float("nan"), device=dev)
    wide[:, :4] = torch.from_numpy(Xs).to(dev)
    view = wide[:, :4]
    assert view.stride(0) == 7
    q, ice = partial_dependence(view, _expl(ens, dev), 3, ice=True)
    want_q, want_ice = R.partial_dependence_reference(Xs, ens, 3)
    assert np.array_equal(q, want_q) and PC.bits_equal(ice, want_ice)


def test_explainer_standardizes_raw_rows(dev):
    from fraud_detection_amd.models.explainers import _standardize

    ens, Xs = PC.random_case(d=3, depth=3, T=5, n=70, seed=36)
    mean, scale = np.array([1.0, -2.0, 0.5]), np.array([2.0, 0.5, 4.0])
    X = (Xs.astype(np.float64) * scale + mean).astype(np.float32)
    pd = TreePartialDependence(ens, mean, scale, device=str(dev)).partial_dependence(X, (0, 1), ice=True)
    want_q, want_ice = R.partial_dependence_reference(_standardize(X, mean, scale), ens, (0, 1))
    assert np.array_equal(pd.pd_q.ravel(), want_q) and PC.bits_equal(pd.ice.reshape(70, -1), want_ice)


def test_classifier_on_a_monotone_device_fit(dev):
    from fraud_detection_amd.models.gbdt import GBDTClassifier

    rng = np.random.default_rng(0)
    X = rng.normal(size=(700, 4)).astype(np.float32)
    y = (X[:, 0] - X[:, 2] + 0.5 * X[:, 1] * X[:, 3] + 0.3 * rng.normal(size=700) > 0).astype(np.uint8)
    m = GBDTClassifier(n_estimators=7, max_depth=3, monotone_constraints=(1, 0, -1, 0), device=str(dev)).fit(X, y)
    fx = m.predict_margin(X)
    for f, sign in ((0, 1), (2, -1), (1, 0)):
        pd = m.partial_dependence(X, f, kind="both")
        want_q, want_ice = R.partial_dependence_reference(X, m.ensemble, f)
        assert np.array_equal(pd.pd_q, want_q) and PC.bits_equal(pd.ice, want_ice)
        assert PC.bits_equal(pd.ice[np.arange(700), PC.own_cell(m.ensemble, f, X[:, f])], fx)
        if sign:
            assert pd.ice.shape[1] > 3
            assert np.all(sign * np.diff(pd.ice, axis=1) >= 0) and np.all(sign * np.diff(pd.pd_q) >= 0)
    head = m.partial_dependence(X, 0, kind="both", iteration_range=(0, 3))
    want_q, want_ice = R.partial_dependence_reference(X, m.ensemble.head(3), 0)
    assert np.array_equal(head.pd_q, want_q) and PC.bits_equal(head.ice, want_ice)
    assert m.partial_dependence(X, 0).ice is None
