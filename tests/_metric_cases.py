"""Exact oracles and case builders for the metric (auc.hip), quantile-select (quantile.hip) and
stratified-split (split.hip) kernels.  Pure numpy and Python integers, no GPU imports:
test_metric_oracle.py validates them on the CPU against brute force, test_metric_kernels_gpu.py and
test_select_split_kernels_gpu.py hold the kernels to them.

Every oracle here is exact (integers or float32 bit patterns), so no test built on them carries a
tolerance.  NaN scores are outside the contract of the AUC / PR / histogram kernels: no builder of
scores emits one.
"""
from __future__ import annotations

import functools
import math

import numpy as np

from fraud_detection_amd.ops import reference as ref

TEST = 255                      # split.hip's code of a test row
DENORM = np.float32(1.4e-45)    # the smallest positive denormal, bits 0x00000001
BRUTE_MAX = 2048                # brute force is P x N: small inputs only


def f32_bits(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def bits_f32(b) -> np.ndarray:
    return np.ascontiguousarray(b, dtype=np.uint32).view(np.float32)


# ---- AUC ----------------------------------------------------------------------------------------
def brute_twice_pairs(s: np.ndarray, y: np.ndarray) -> int:
    """2 #{s_p > s_n} + #{s_p == s_n} over all P x N pairs, float32 compares (+-inf are ordinary
    scores, -0.0 == +0.0)."""
    s = np.asarray(s, dtype=np.float32).ravel()
    assert s.shape[0] <= BRUTE_MAX and not np.isnan(s).any()
    pos = np.asarray(y).ravel() != 0
    sp, sn = s[pos][:, None], s[~pos][None, :]
    return 2 * int(np.count_nonzero(sp > sn)) + int(np.count_nonzero(sp == sn))


def counts(y: np.ndarray) -> tuple[int, int]:
    pos = np.asarray(y).ravel() != 0
    return int(pos.sum()), int((~pos).sum())


def sorted_pairs(s: np.ndarray, y: np.ndarray):
    """(key uint32 [n], label uint8 [n]) of the rows sorted ascending by (order key, label != 0):
    what the stable LSD radix sort of auc.hip must leave."""
    packed = (ref.order_key(s).astype(np.uint64) << np.uint64(1)) | (np.asarray(y).ravel() != 0).astype(np.uint64)
    packed = np.sort(packed)
    return (packed >> np.uint64(1)).astype(np.uint32), (packed & np.uint64(1)).astype(np.uint8)


def hist_counts(s: np.ndarray, y: np.ndarray, bits: int) -> np.ndarray:
    """int64 [2, 2^bits]: (negative, positive) rows per bin, bin = order key >> (32 - bits)."""
    b = (ref.order_key(s) >> np.uint32(32 - bits)).astype(np.int64)
    pos = np.asarray(y).ravel() != 0
    nb = 1 << bits
    return np.stack([np.bincount(b[~pos], minlength=nb), np.bincount(b[pos], minlength=nb)]).astype(np.int64)


def hist_twice_pairs(h: np.ndarray) -> tuple[int, int, int]:
    """(sum_b P_b (2 N_<b + N_b), P, N) of a [2, nb] histogram, in Python integers."""
    neg, pos = np.asarray(h[0]).astype(np.uint64), np.asarray(h[1]).astype(np.uint64)
    before = np.cumsum(neg, dtype=np.uint64) - neg  # N < 2^63 in every case built here
    twice = 0
    for b in np.flatnonzero(pos):
        twice += int(pos[b]) * (2 * int(before[b]) + int(neg[b]))
    return twice, sum(int(v) for v in pos[pos != 0]), sum(int(v) for v in neg[neg != 0])


def special_values() -> np.ndarray:
    """float32 values where the kernels' compares, keys and radix digits can go wrong: +-inf, both
    zeros, +-smallest denormal, negatives (the inverted-key branch), the largest / smallest finite
    values, and neighbours of 1.0 and -1.0 whose keys differ from it in exactly one byte."""
    one, mone = 0x3F800000, 0xBF800000
    one_byte = [one ^ (v << (8 * byte)) for byte in range(4) for v in (1, 0x80 if byte < 3 else 0x04)]
    one_byte += [mone ^ (v << (8 * byte)) for byte in range(4) for v in (1, 0x80 if byte < 3 else 0x04)]
    vals = np.concatenate([
        np.array([np.inf, -np.inf, 0.0, -0.0, DENORM, -DENORM, 1.0, -1.0, -1.5, -0.25, 0.25,
                  np.finfo(np.float32).max, np.finfo(np.float32).min, np.finfo(np.float32).tiny], dtype=np.float32),
        bits_f32(np.array(one_byte, dtype=np.uint32))])
    assert not np.isnan(vals).any()
    return vals


@functools.lru_cache(maxsize=None)
def _special_scores(n: int, seed: int, rate: float):
    rng = np.random.default_rng([n, seed])
    sv = special_values()
    # every special value twice in each class, so ties inside and across the classes exist
    core_s = np.tile(sv, 4)
    core_y = np.repeat(np.array([0, 1, 0, 1], dtype=np.uint8), sv.shape[0])
    if n <= core_s.shape[0]:
        pick = rng.permutation(core_s.shape[0])[:n]
        s, y = core_s[pick], core_y[pick]
    else:
        k = n - core_s.shape[0]
        grid = (np.round(rng.normal(size=k) * 4) / 4).astype(np.float32)       # coarse grid of ties
        fine = rng.normal(size=k).astype(np.float32)
        kind = rng.random(k)
        fill = np.where(kind < 0.5, grid, np.where(kind < 0.8, fine, sv[rng.integers(0, sv.shape[0], k)]))
        s = np.concatenate([core_s, fill.astype(np.float32)])
        y = np.concatenate([core_y, (rng.random(k) < rate).astype(np.uint8)])
        p = rng.permutation(n)
        s, y = s[p], y[p]
    s = np.ascontiguousarray(s, dtype=np.float32)
    assert not np.isnan(s).any()
    s.setflags(write=False)
    y.setflags(write=False)
    return s, y


def special_scores(n: int, seed: int = 0, rate: float = 0.3):
    """(scores float32 [n], labels uint8 [n]): the special values, each repeated in both classes,
    mixed with a coarse grid of ties and plain normals.  Never a NaN.  Cached and read-only."""
    return _special_scores(int(n), int(seed), float(rate))


def finite_only(s: np.ndarray, y: np.ndarray):
    keep = np.isfinite(s)
    return s[keep], y[keep]


def inf_tie_case():
    """20 rows mixing repeated +inf and -inf across both classes (the tie groups np.diff splits:
    inf - inf is NaN)."""
    inf = np.inf
    s = np.array([inf, inf, inf, -inf, -inf, -inf, 0.5, 0.5, inf, -inf, 1.0, -1.0, inf, -inf, 0.5, inf, -inf, 2.0,
                  inf, -inf], dtype=np.float32)
    y = np.array([1, 0, 1, 0, 1, 0, 1, 0, 0, 1, 1, 0, 1, 0, 0, 1, 1, 0, 0, 1], dtype=np.uint8)
    return s, y


def heavy_ties(n: int, seed: int, rate: float = 0.3, levels: int = 37):
    """n scores on ``levels`` grid values (negatives, both zeros and +-inf among them): long tie
    segments that mix the classes."""
    rng = np.random.default_rng([n, seed, levels])
    grid = ((np.arange(levels) - levels // 2) / 4).astype(np.float32)
    grid[0], grid[-1] = -np.inf, np.inf
    s = grid[rng.integers(0, levels, n)]
    neg_zero = (s == 0) & (rng.random(n) < 0.5)
    s[neg_zero] = -0.0
    return s, (rng.random(n) < rate).astype(np.uint8)


def brute_pr_curve(s: np.ndarray, y: np.ndarray):
    """(thr, tp, fp) by a walk over the distinct float32 thresholds, descending: tp / fp = positives /
    negatives with score >= thr.  -0.0 and +0.0 are one threshold, reported as +0.0."""
    s = np.asarray(s, dtype=np.float32).ravel()
    pos = np.asarray(y).ravel() != 0
    thr = sorted({0.0 if v == 0 else float(v) for v in s}, reverse=True)
    tp = [int(np.count_nonzero(pos & (s >= np.float32(t)))) for t in thr]
    fp = [int(np.count_nonzero(~pos & (s >= np.float32(t)))) for t in thr]
    return np.array(thr, dtype=np.float32), np.array(tp, dtype=np.int64), np.array(fp, dtype=np.int64)


def brute_ap_q(tp, fp) -> int:
    """sum_g rint(dtp * (tp / (tp + fp)) * 2^30) with Python floats (IEEE double) and integers."""
    q, prev = 0, 0
    for t, f in zip((int(v) for v in tp), (int(v) for v in fp)):
        if t != prev:
            q += int(np.rint(float(t - prev) * (float(t) / float(t + f)) * 2.0 ** 30))
        prev = t
    return q


def bin_edge_scores(bits: int, nbins: int = 6):
    """Scores on the edges of several bins of a 2^bits histogram: for a bin b the largest key of b and
    the smallest of b + 1, over bins of negatives, of the zero crossing and of positives, plus +-inf,
    both zeros and +-denormals.  Keys of NaN patterns are left out."""
    sh = 32 - bits
    nb = 1 << bits
    # bins: around the key of -1.0, 0.0, 1.0 and the two ends of the finite range
    anchors = [int(ref.order_key(np.array([v], dtype=np.float32))[0]) >> sh for v in (-1.0, 0.0, 1.0, -3e38, 3e38)]
    keys = []
    for a in anchors:
        for b in range(max(a - nbins // 2, 0), min(a + nbins // 2, nb - 2) + 1):
            keys += [((b + 1) << sh) - 1, (b + 1) << sh, (b << sh) + ((1 << sh) >> 1)]
    vals = ref.order_key_inv(np.array(keys, dtype=np.uint32))
    vals = vals[~np.isnan(vals)]
    return np.concatenate([vals, special_values()]).astype(np.float32)


# ---- quantile select ------------------------------------------------------------------------------
def select_picks(sample: np.ndarray, max_bin: int, counts=None) -> np.ndarray:
    """float32 [max_bin, d]: per feature, np.sort(sample) at rank 0 and at ranks floor(t m_f / max_bin),
    t = 1 .. max_bin - 1, with m_f = clip(counts_f, 0, m) (m without counts).  NaN sorts last."""
    sample = np.asarray(sample, dtype=np.float32)
    m, d = sample.shape
    srt = np.sort(sample, axis=0)
    out = np.empty((max_bin, d), dtype=np.float32)
    for f in range(d):
        mf = m if counts is None else min(max(int(counts[f]), 0), m)
        ranks = [0] + [(t * mf) // max_bin for t in range(1, max_bin)]
        out[:, f] = srt[ranks, f]
    return out


SELECT_KINDS = ("low10", "mid11", "top_digit", "negatives", "constant", "signed_zeros", "denormals", "inf",
                "nan_some", "nan_all", "normal")


def select_feature(kind: str, m: int, rng) -> np.ndarray:
    """One float32 feature column of m rows.  The select takes the key's top 11 bits at level 0, the
    next 11 at level 1 and the last 10 at level 2; low10 / mid11 leave all the work to one level."""
    if kind == "low10":      # 1.0 + j 2^-23, j < 1024, with duplicates: only the low 10 key bits differ
        return bits_f32(np.uint32(0x3F800000) + rng.integers(0, 1024, m).astype(np.uint32))
    if kind == "mid11":      # only key bits 10 .. 20 differ
        return bits_f32(np.uint32(0x3F800000) + (rng.integers(0, 2048, m).astype(np.uint32) << np.uint32(10)))
    if kind == "top_digit":  # +-2^e: every value alone in its top-digit bucket
        e = rng.integers(-100, 101, m)
        return (np.where(rng.random(m) < 0.5, -1.0, 1.0) * np.exp2(e.astype(np.float64))).astype(np.float32)
    if kind == "negatives":
        return (-np.abs(rng.normal(size=m)) - 0.125).astype(np.float32)
    if kind == "constant":
        return np.full(m, 7.25, dtype=np.float32)
    if kind == "signed_zeros":
        return np.array([0.0, -0.0, -0.0, 0.0, 1.0, -1.0], dtype=np.float32)[rng.integers(0, 6, m)]
    if kind == "denormals":
        b = rng.integers(1, 1 << 20, m).astype(np.uint32)
        return bits_f32(np.where(rng.random(m) < 0.5, b | np.uint32(0x80000000), b))
    if kind == "inf":
        v = rng.normal(size=m).astype(np.float32)
        u = rng.random(m)
        v[u < 0.2] = np.inf
        v[u > 0.8] = -np.inf
        return v
    if kind in ("nan_some", "nan_all"):
        v = rng.normal(size=m).astype(np.float32)
        hit = np.ones(m, bool) if kind == "nan_all" else rng.random(m) < 0.3
        nan = bits_f32(np.where(rng.random(m) < 0.5, np.uint32(0x7FC00000), np.uint32(0xFFC00001)))
        f32_bits(v)[hit] = f32_bits(nan)[hit]  # through the bit patterns: both NaN signs survive
        return v
    if kind == "normal":
        return rng.normal(size=m).astype(np.float32)
    raise ValueError(kind)


def select_sample(m: int, d: int, offset: int = 0) -> tuple[np.ndarray, list]:
    """(sample float32 [m, d], the kind of every column): column j holds kind (j + offset) mod 11, so
    d = 32 holds every kind about three times and the d = 1 cases walk through them by ``offset``."""
    rng = np.random.default_rng([m, d, offset])
    kinds = [SELECT_KINDS[(j + offset) % len(SELECT_KINDS)] for j in range(d)]
    cols = [select_feature(k, m, rng) for k in kinds]
    # np.stack of float32 keeps every bit pattern (NaN payloads and signs included)
    return np.ascontiguousarray(np.stack(cols, axis=1), dtype=np.float32), kinds


def picks_mismatch(got: np.ndarray, exp: np.ndarray) -> str | None:
    """None when the raw picks meet the contract: equal to the oracle by value (NaN == NaN), every
    zero with its sign bit clear, every NaN where the oracle has one."""
    got = np.asarray(got, dtype=np.float32)
    if got.shape != exp.shape:
        return f"shape {got.shape} != {exp.shape}"
    if not np.array_equal(np.isnan(got), np.isnan(exp)):
        return f"NaN picks differ at {np.argwhere(np.isnan(got) != np.isnan(exp))[:4].tolist()}"
    if not np.array_equal(got, exp, equal_nan=True):
        bad = np.argwhere(~((got == exp) | (np.isnan(got) & np.isnan(exp))))
        t, f = bad[0]
        return f"{bad.shape[0]} picks differ, first at target {t} feature {f}: {got[t, f]!r} != {exp[t, f]!r}"
    if np.any(f32_bits(got)[got == 0] != 0):
        return "a zero pick carries a sign bit"
    return None


# ---- stratified split -----------------------------------------------------------------------------
def split_properties(codes: np.ndarray, y: np.ndarray, test_frac: float, k: int) -> list:
    """Violations (empty: none) of what the split must deliver, per class (class 1: label byte == 1,
    class 0: every other byte): the test count is min(floor(frac n_c + 0.5), n_c); the other rows
    carry fold codes < k whose sizes sum to the rest and differ by at most one, larger folds first;
    with k <= 1 the only fold code is 0."""
    codes = np.asarray(codes)
    y = np.asarray(y).ravel()
    bad = []
    if codes.dtype != np.uint8 or codes.shape != y.shape:
        return [f"codes {codes.dtype} {codes.shape}"]
    for cls, sel in ((0, y != 1), (1, y == 1)):
        c = codes[sel]
        n_c = int(c.shape[0])
        want_test = min(int(math.floor(test_frac * float(n_c) + 0.5)), n_c)
        n_test = int(np.count_nonzero(c == TEST))
        if n_test != want_test:
            bad.append(f"class {cls}: {n_test} test rows of {n_c}, want {want_test}")
        folds = c[c != TEST]
        rest = n_c - want_test
        if k <= 1:
            if np.any(folds != 0):
                bad.append(f"class {cls}: fold codes {np.unique(folds).tolist()} with k = {k}")
            continue
        if folds.shape[0] and int(folds.max()) >= k:
            bad.append(f"class {cls}: fold code {int(folds.max())} >= k = {k}")
            continue
        sizes = np.bincount(folds, minlength=k)
        q, r = divmod(rest, k)
        if sizes.tolist() != [q + 1] * r + [q] * (k - r):
            bad.append(f"class {cls}: fold sizes {sizes.tolist()}, want {r} x {q + 1} then {k - r} x {q}")
    return bad


def split_labels(n: int, n1: int, seed: int = 0, other_bytes: bool = False) -> np.ndarray:
    """uint8 [n] labels with exactly n1 ones at random rows; ``other_bytes``: a third of the other rows
    carry the bytes 2 and 255, which belong to class 0."""
    rng = np.random.default_rng([n, n1, seed])
    y = np.zeros(n, dtype=np.uint8)
    y[rng.permutation(n)[:n1]] = 1
    if other_bytes:
        u = rng.random(n)
        y[(y == 0) & (u < 0.17)] = 2
        y[(y == 0) & (u > 0.83)] = 255
    return y


def class_sizes(n: int, k: int) -> list:
    """Sizes of class 1 to try at n rows and k folds: empty, tiny, around k, everything, and 4, 5,
    2^j, 2^j + 1 (j = 8, 9), where the Feistel domain is two to four times the class."""
    want = {0, 1, 2, k - 1, k, k + 1, n, 4, 5, 256, 257, 512, 513}
    return sorted(v for v in want if 0 <= v <= n)
