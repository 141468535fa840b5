"""Shared cases of the permutation-importance tests (tests/test_permutation_importance*.py): the
Feistel rounds as a plain loop, explicit permuted copies, labels with both classes.  Numpy only."""
from __future__ import annotations

import numpy as np

import _pd_cases as PC
from fraud_detection_amd.ops import reference_gbdt as R

M32 = 0xFFFFFFFF


def fmix32(x: int) -> int:
    x &= M32
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & M32
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & M32
    x ^= x >> 16
    return x


def loop_donors(n: int, seed: int, f: int, r: int) -> list:
    """permutation_donors written out element by element in Python integers."""
    c = 32 * r + f
    b = 2
    while (1 << b) < n:
        b += 1
    h = (b + 1) >> 1
    mask = (1 << h) - 1
    keys = [fmix32(seed ^ fmix32(0x9E3779B9 * (2 * c + 1) + k)) for k in range(4)]
    out = []
    for i in range(n):
        x = i
        while True:
            L, Rh = x >> h, x & mask
            for k in keys:
                L, Rh = Rh, L ^ (fmix32(Rh ^ k) & mask)
            x = (L << h) | Rh
            if x < n:
                break
        out.append(x)
    return out


def explicit_margins(Xs, ens, features, n_repeats: int, seed: int):
    """float32 [F, R, n]: PC.margin on a copy of Xs per column, the donors from the plain loop."""
    n = Xs.shape[0]
    out = np.empty((len(features), n_repeats, n), np.float32)
    for i, f in enumerate(features):
        for r in range(n_repeats):
            Xm = Xs.copy()
            Xm[:, f] = Xs[np.array(loop_donors(n, seed, f, r), np.int64), f]
            out[i, r] = PC.margin(Xm, ens)
    return out


def labels(Xs, ens, seed: int) -> np.ndarray:
    """uint8 [n] labels correlated with the margin, with at least one row of each class."""
    rng = np.random.default_rng(seed)
    m = PC.margin(Xs, ens).astype(np.float64)
    y = (m + rng.normal(0, 0.5 * (m.std() + 1e-3), len(m)) > np.median(m)).astype(np.uint8)
    P = int(y.sum())
    assert 0 < P < len(y), "the fixture needs both classes"
    return y


def oracle_raw(Xs, y, ens, features, n_repeats: int, seed: int, scoring: str):
    """(raw int64 [F, R], baseline_raw): the reference scorers on the oracle margins."""
    pm, base = R.permuted_margins_reference(Xs, ens, features, n_repeats, seed)
    score = {"auc": R.twice_pairs, "aucpr": R.ap_q, "logloss": lambda m, yy: int(R.eval_record(m, yy)[0])}[scoring]
    raw = np.array([[score(pm[i, r], y) for r in range(n_repeats)] for i in range(len(features))], np.int64)
    return raw.reshape(len(features), n_repeats), int(score(base, y))
