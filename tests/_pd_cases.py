"""Shared cases of the partial-dependence tests (tests/test_partial_dependence*.py): hand-built and
random ensembles, the cell a value falls in, and plain loops over ``predict_margin``.  Numpy only."""
from __future__ import annotations

from dataclasses import replace

import numpy as np

import _tree_cases as TC
from fraud_detection_amd.ops import reference_gbdt as R

INF = np.inf


def hand_ensemble(default_left: bool = True):
    """Three depth-2 trees over d = 4 features.  Feature 0: thresholds 0.5 (twice, in two trees),
    -0.5 and 1.5; feature 1: 1.0; feature 2: 2.0 and a "missing rows only" node (thr -inf, bin -1,
    default_left); feature 3: unused; one pass-through node."""
    feat = [[0, 1, 0], [0, -1, 2], [2, 0, 0]]
    thr = [[0.5, 1.0, -0.5], [0.5, INF, 2.0], [-INF, 0.5, 1.5]]
    leaf = [[0.1, -0.2, 0.3, -0.4], [0.05, 0.07, -0.11, 0.13], [-0.3, 0.2, 0.25, -0.15]]
    ens = TC.make_ensemble(4, 2, feat, thr, leaf)
    binv = np.zeros((3, 3), np.int32)
    binv[2, 0] = -1
    dl = np.zeros((3, 3), np.uint8)
    if default_left:
        dl[2, 0] = 1
        dl[0, 2] = 1
    return replace(ens, bin=binv, default_left=dl if default_left else None)


def random_case(d: int, depth: int, T: int, n: int, seed: int, learn: bool = False, nan_rows: bool = False):
    """(ens, Xs [n, d]): a random ensemble with pass-through nodes and thresholds planted on row
    values; ``learn``: default_left on half of the split nodes; ``nan_rows``: 15 % NaN entries."""
    rng = np.random.default_rng(seed)
    Xs = rng.normal(size=(n, d)).astype(np.float32)
    ens = TC.random_ensemble(d, depth, T, seed + 1)
    ens = TC.plant_ties(ens, Xs, Xs, seed + 2)
    if learn:
        dl = ((rng.random(ens.feat.shape) < 0.5) & (ens.feat >= 0)).astype(np.uint8)
        ens = replace(ens, default_left=dl)
    if nan_rows:
        Xs[rng.random(Xs.shape) < 0.15] = np.nan
    return ens, Xs


def margin(Xs, ens):
    return R.predict_margin(Xs, ens.feat, ens.thr, ens.leaf, ens.depth, ens.base_margin,
                            ens.default_left if ens.has_default_left else None)


def loop_ice(Xs, ens, features):
    """float32 [n, C]: one plain predict_margin call per cell on a copy of Xs (pairs: ca * C_b + cb)."""
    fs = (features,) if np.isscalar(features) else tuple(features)
    reps = [R.pd_cells(ens, f)[0] for f in fs]
    cols = []
    for va in reps[0]:
        for vb in (reps[1] if len(fs) == 2 else [None]):
            Xm = np.array(Xs, np.float32, copy=True)
            Xm[:, fs[0]] = va
            if vb is not None:
                Xm[:, fs[1]] = vb
            cols.append(margin(Xm, ens))
    return np.stack(cols, 1)


def pd_q_of(ice):
    return np.rint(ice.astype(np.float64) * 2.0 ** 30).astype(np.int64).sum(0)


def own_cell(ens, f, x):
    """The cell of each value of x [n] (NaN: the missing cell, last)."""
    E = R.pd_grid(ens, f)
    c = np.searchsorted(E, x, side="right")          # x >= E[c - 1] and x < E[c]
    return np.where(np.isnan(x), len(E) + 1, c)


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def cap_ensemble(ka: int, kb: int):
    """Depth-5 trees over d = 3 whose nodes carry ka distinct thresholds on feature 0 and kb on
    feature 1 (the rest split on feature 2): (ka + 1) * (kb + 1) cells for the pair (0, 1)."""
    ni = 31
    T = -(-(ka + kb) // ni)
    feat = np.full(T * ni, 2, np.int32)
    thr = np.zeros(T * ni, np.float32)
    feat[:ka], feat[ka:ka + kb] = 0, 1
    thr[:ka] = np.linspace(-2, 2, ka)
    thr[ka:ka + kb] = np.linspace(-2, 2, kb)
    rng = np.random.default_rng(5)
    perm = rng.permutation(T * ni)                   # spread the two features over all trees and levels
    leaf = rng.normal(0, 0.3, (T, 32)).astype(np.float32)
    return TC.make_ensemble(3, 5, feat[perm].reshape(T, ni), thr[perm].reshape(T, ni), leaf)
