"""The conditions that give the device k-NN tests (test_knn_kernels_gpu.py) their power, on the CPU.

The bf16x3 engines return the exact fp32 ranking only through a chain of proofs (knn.hip): the
approximate score hi.hi + hi.lo + lo.hi is within 2^-16 sum|q_f c_f| of the exact one, the margin
m = 2^-14 (||q|| tmax + 0.5 tmax^2) is at least 4x that, the running threshold never exceeds the exact
k-th best.  A device test pins those links only on inputs where breaking one changes the answer or a
checked intermediate.  These tests state that for the committed seeds, with an fp64 emulation
(_knn_cases.py) of the collect filter (bf16x3r, the auto engine) at its FINAL threshold: the
threshold is the k-th best lower bound approx - m, a candidate passes when approx + m reaches it.
Approximate scores are compared with each other only.  (The fixed-threshold rule of bf16x3t has its
own emulation: test_knn_twopass_oracle.py.)

Measured (k = 5, self-search).  err = max |approx3 - exact| / m, asserted <= 0.25; then the share of
queries whose re-ranked answer ``assert_valid_topk`` rejects when the filter is hi-only (both lo
halves lost), has lost the query's lo half, or uses m / 64:

  case          err     hi-only   no query lo   m / 64
  normal        0.065    2.1 %    0.1 %         0 %
  cluster3      0.061   65.0 %    0   %         0 %
  cluster30     0.079   29.7 %    0   %         0 %
  cluster3_far  0.101   93.0 %    0   %         0 %
  heavy         0.184    2.3 %    0   %         0 %
  near_origin   0.054    1.8 %    0.3 %         0 %
  lattice       0.151   60.5 %    0   %         0 %
  (with the intact filter: 0 % everywhere)

  * hi-only is caught by the ranking itself on the clusters, and a true neighbour is then left out by
    more than 2 tol (cluster3: 65 %).  ``normal`` shows it for 2.1 % of the queries -- 0.4 % of the
    returned entries, inside the 0.99 entry-match bar of the older continuous tests -- and a lost
    query lo for 0.1 %: ``normal`` alone is not a test.
  * A lost query lo half is not seen by the ranking (0 %): on cluster3_far the error lo_q . c is
    lo_q . b, the same for every candidate of a cluster b + P, plus lo_q . P_c, about
    2^-9 |q_f| |P_c| ~ 0.01 against m = 0.023, and a shift common to all scores moves the threshold
    with them.  The ABSOLUTE error of the best approximate scores sees it: with the query lo lost,
    96.7 % of cluster3_far's queries (100 % of cluster3's, 99.8 % of heavy's) have one of their 8
    best approximate scores off by more than m / 4 + tol.  The device tests hold the approximate
    scores they read back to that bound -- every two-pass group maximum within m / 4 of the intact
    emulation (test_knn_twopass_gpu.py) -- and check that every listed lower bound is one.
  * m / 64 is not seen by the ranking on the clusters either (0 %); it is caught on ``lattice``: its
    tight queries have >= 493 candidates inside the true margin (both list lanes overflow); with
    m / 64 only 31.5 on average (max 142) pass and 80 % of them stay within ONE lane's 64 entries --
    the device test's "the over-cap lanes are exactly the tight queries' lanes" fails.

Path coverage on ``lattice`` (nsplit = 1): the 501 tight queries (the 500 rows built tight and the
corner row that lent them its columns 4..29; the same set for k = 1, 5, 8) have >= 493 passing
candidates, >= 213 per list lane for certain; the spread queries 5.5 on average (max 9), and at most
63 per lane even under the lowest running threshold without compaction.  3.6 % of the lattice's
feature entries have lo != 0 (6.5 % of all prepped entries), 419 rows repeat an earlier one, and both
fp32 chain orders (columns 0..31; feature 16h + s at MFMA step s) reproduce the fp64 score bit for bit.

Checked against the device once, with deliberately broken builds that are not part of the tree, when
the suite still ran three more engines (since retired) and had 53 device tests: a split that zeroes
every lo half failed 40 of them, one that zeroes the queries' lo half 33, margins scaled by 1/64 14
-- in each case the engine tests on the cluster cases and the lattice, the fallback tests and the
proof-invariant tests among them."""
import numpy as np
import pytest

import _knn_cases as KC
from fraud_detection_amd.ops import reference as ref

K = 5


def _emulated(name, kind="approx3", scale=1.0):
    """(approx, margin, pass mask, re-ranked answer) of the self-search of one case under the collect
    filter (bf16x3r: threshold = k-th best LOWER BOUND)."""
    X = KC.case(name)
    s, _ = KC.oracle(name)
    mg = KC.margins(X, X) * scale
    a = KC.approx_scores(X, X, kind)
    p = KC.filter_pass(a, mg, K, 0) & np.isfinite(s)
    return a, mg, p, KC.filtered_topk(p, s, K)


def _lost_share(name, kind, scale=1.0):
    """Share of queries whose re-ranked answer ``assert_valid_topk`` rejects (a true neighbour left out
    beyond the tolerance)."""
    s, t = KC.oracle(name)
    return float(KC.outsider_violations(_emulated(name, kind, scale)[3], s, t).mean())


# ---- exactness on the lattice -----------------------------------------------------------------
def test_lattice_scores_are_exact_in_both_fp32_chain_orders():
    X = KC.case("lattice")
    s = KC.scores64(X, X)
    assert np.array_equal(s.astype(np.float32).astype(np.float64), s)
    Qp, Cp = KC.prep_rows(X, 1).astype(np.float64), KC.prep_rows(X, 0).astype(np.float64)
    assert np.array_equal(Cp[:, 30], -0.5 * np.sum(X[:, :30].astype(np.float64) ** 2, 1))
    orders = {"columns": list(range(32)), "mfma 16h+s": [16 * h + st for st in range(16) for h in range(2)]}
    for nm, order in orders.items():
        acc = np.zeros(s.shape, dtype=np.float32)
        for f in order:
            acc = (acc.astype(np.float64) + Qp[:, f][:, None] * Cp[:, f][None, :]).astype(np.float32)
        assert np.array_equal(acc.astype(np.float64), s), nm


def test_lattice_has_nonzero_lo_and_duplicates():
    X = KC.case("lattice")
    _, lo = KC.split_hi_lo(KC.prep_rows(X, 0))
    share = float((lo[:, :30] != 0).mean())
    assert 0.02 < share < 0.06, share  # measured 3.6 %
    assert len(np.unique(X[:, :30], axis=0)) < X.shape[0] - 100
    # bf16 is NOT exact here: the approximate score differs from the exact one
    a = KC.approx_scores(X, X)
    assert np.any(a != KC.scores64(X, X))


# ---- the error premise ------------------------------------------------------------------------
@pytest.mark.parametrize("name", KC.CASES)
def test_approx_error_is_within_a_quarter_of_the_margin(name):
    X = KC.case(name)
    ratio = np.abs(KC.approx_scores(X, X) - KC.scores64(X, X)) / KC.margins(X, X)
    assert ratio.max() <= 0.25, float(ratio.max())


@pytest.mark.parametrize("name", KC.CASES)
def test_intact_filter_loses_nothing(name):
    s, _ = KC.oracle(name)
    idx = _emulated(name)[3]
    assert np.array_equal(idx, ref.knn_topk(KC.case(name), KC.case(name), K, 0)[0])
    assert not np.isinf(np.take_along_axis(s, idx, 1)).any()


# ---- power under the emulated final-threshold filter -------------------------------------------
def test_hi_only_filter_is_caught_on_the_clusters():
    assert _lost_share("cluster3", "approx_hi_only") >= 0.25   # measured 65.0 %
    assert _lost_share("cluster30", "approx_hi_only") >= 0.10  # measured 29.7 %
    # "by more than 2 tol", stated directly: the kept k-th best is below the true one by over twice
    # the largest tolerance of the kept list
    s, t = KC.oracle("cluster3")
    idx = _emulated("cluster3", "approx_hi_only")[3]
    true = ref.knn_topk(KC.case("cluster3"), KC.case("cluster3"), K, 0)[0].astype(np.int64)
    gap = np.take_along_axis(s, true, 1).min(1) - np.take_along_axis(s, idx, 1).min(1)
    tmax = np.take_along_axis(t, idx, 1).max(1)
    assert np.mean(gap > 2 * tmax) >= 0.25, float(np.mean(gap > 2 * tmax))


def test_lost_query_lo_is_caught_on_cluster3_far():
    # the collect filter compares approximate scores with each other, and lo_q . b is common to every
    # candidate of a cluster b + P: its ranking does not see it (measured 0 %) ...
    assert _lost_share("cluster3_far", "approx_no_query_lo") < 0.01
    # ... the absolute error of the kept scores does, on at least 20 % of the queries
    assert _kept_error_share("cluster3_far", "approx_no_query_lo") >= 0.20   # measured 96.7 %
    assert _kept_error_share("cluster3", "approx_no_query_lo") >= 0.20       # measured 100 %
    assert _kept_error_share("heavy", "approx_no_query_lo") >= 0.20          # measured 99.8 %
    for name in ("cluster3_far", "cluster3", "heavy"):
        assert _kept_error_share(name, "approx3") == 0.0


def test_normal_alone_is_not_a_test():
    # under the auto engine's (collect) filter fewer than 1 % of the queries lose a neighbour to a
    # lost query lo half (measured 0.1 %), and a hi-only filter changes fewer than 1 % of the returned
    # ENTRIES (2.1 % of the queries, one entry each): inside a 0.99 entry-match bar
    assert _lost_share("normal", "approx_no_query_lo") < 0.01
    idx = _emulated("normal", "approx_hi_only")[3]
    true = ref.knn_topk(KC.case("normal"), KC.case("normal"), K, 0)[0]
    assert np.mean(idx != true) < 0.01


def _kept_error_share(name, kind):
    """Share of queries with one of their 8 best approximate scores off by more than margin / 4 + tol
    (the quarter margin the proof allows |approx - exact|; the device tests hold the approximate scores
    they read back, the two-pass group maxima, to it)."""
    X = KC.case(name)
    s, t = KC.oracle(name)
    a = np.where(np.isfinite(s), KC.approx_scores(X, X, kind), -np.inf)
    top = np.argsort(-a, axis=1, kind="stable")[:, :8]
    g = lambda M: np.take_along_axis(M, top, 1)
    return float(np.any(np.abs(g(a) - g(s)) > g(KC.margins(X, X)) / 4 + g(t), axis=1).mean())


# ---- path coverage on the lattice (nsplit = 1) ------------------------------------------------
def _lattice_paths(scale=1.0):
    """(the tight queries, the number of candidates that pass the final-threshold filter per query)"""
    return KC.lattice_tight(), _emulated("lattice", scale=scale)[2].sum(1)


def test_lattice_reaches_the_fallback_paths_for_tight_queries_only():
    tight, cnt = _lattice_paths()
    built = KC.lattice_built_tight()
    # the 500 rows built tight and the corner row that lent them its columns 4..29
    assert built.sum() == 500 and np.all(tight[built]) and tight.sum() == 501
    for k in (1, 8):
        assert np.array_equal(KC.lattice_tight(k), tight)
    assert cnt[tight].min() > 2 * 64, int(cnt[tight].min())           # measured 493
    assert cnt[~tight].mean() < 10 and cnt[~tight].max() < 64, (cnt[~tight].mean(), cnt[~tight].max())  # 5.5, 9
    # per list lane (a query's candidates are shared by two lanes, rows 4h .. 4h + 3 of every 8):
    # a tight query overflows BOTH 64-entry lanes whatever the approximate error is, every other
    # query fits both at the final threshold ...
    X = KC.case("lattice")
    s, _ = KC.oracle("lattice")
    sure, may = KC.sure_and_possible_pass(X, X, K, 0)
    half = KC.lane_half(X.shape[0])
    for h in (0, 1):
        assert sure[tight][:, half == h].sum(1).min() > 64    # measured 213 / 214
        assert may[~tight][:, half == h].sum(1).max() < 64    # measured 8 / 9
    # ... and under the RUNNING threshold too: with the threshold of tile t taken as low as the k-th
    # best of the tiles before it allows (s_k - 1.25 m) and every upper bound as high (s + 1.25 m),
    # no compaction, a lane of a spread query collects at most 63 entries
    m = KC.margins(X, X).max()
    run = np.zeros((X.shape[0], 2), dtype=np.int64)
    for lo in range(0, X.shape[0], 32):
        thr = -np.inf if lo == 0 else -np.partition(-s[:, :lo], K - 1, axis=1)[:, K - 1][:, None] - 1.25 * m
        p = s[:, lo:lo + 32] + 1.25 * m >= thr
        for h in (0, 1):
            run[:, h] += p[:, half[lo:lo + 32] == h].sum(1)
    assert run[~tight].max() <= 64, int(run[~tight].max())  # measured 63 (mean 27)


def test_margin_over_64_is_caught_on_the_lattice():
    tight, cnt = _lattice_paths(1.0 / 64)
    # most tight queries no longer overflow their two 64-entry lanes (measured mean 31.5, max 142)
    assert np.mean(cnt[tight] <= 64) >= 0.5, float(np.mean(cnt[tight] <= 64))
    # the ranking alone would not show it, here or on the far cluster (measured 0 %)
    assert _lost_share("cluster3_far", "approx3", 1.0 / 64) < 0.01


# ---- the checker itself -----------------------------------------------------------------------
@pytest.mark.parametrize("name", KC.CASES)
def test_checker_accepts_the_oracle_and_rejects_edits(name):
    X = KC.case(name)
    s, t = KC.oracle(name)
    idx, d2 = ref.knn_topk(X, X, K + 1, 0)
    idx, nxt = idx[:, :K].copy(), idx[:, K]
    score = np.take_along_axis(s, idx.astype(np.int64), 1).astype(np.float32)
    KC.assert_valid_topk(idx, score, X, X, K, 0, s=s, t=t)
    KC.assert_valid_topk(idx, None, X, X, K, 0)
    sl, tl = np.take_along_axis(s, idx.astype(np.int64), 1), np.take_along_axis(t, idx.astype(np.int64), 1)
    # swap two entries with well-separated scores
    sep = np.flatnonzero(sl[:, 0] - sl[:, K - 1] > 4 * (tl[:, 0] + tl[:, K - 1]))
    assert sep.size, "no query with separated first and last entries"
    bad = idx.copy()
    bad[sep[0], [0, K - 1]] = bad[sep[0], [K - 1, 0]]
    with pytest.raises(AssertionError):
        KC.assert_valid_topk(bad, None, X, X, K, 0, s=s, t=t)
    # the (k+1)-th in place of a neighbour, where the gap exceeds 2 tol
    rows = np.arange(X.shape[0])
    gap = sl[:, K - 1] - s[rows, nxt]
    far = np.flatnonzero(gap > 2.5 * np.maximum(tl[:, K - 1], t[rows, nxt]))
    assert far.size, "no query with a clear k-th / (k+1)-th gap"
    bad = idx.copy()
    bad[far[0], K - 1] = nxt[far[0]]
    with pytest.raises(AssertionError):
        KC.assert_valid_topk(bad, None, X, X, K, 0, s=s, t=t)
    # the self row
    bad = idx.copy()
    bad[3, 2] = 3
    with pytest.raises(AssertionError):
        KC.assert_valid_topk(bad, None, X, X, K, 0, s=s, t=t)
    # a repeated index, and a wrong device score
    bad = idx.copy()
    bad[5, 1] = bad[5, 0]
    with pytest.raises(AssertionError):
        KC.assert_valid_topk(bad, None, X, X, K, 0, s=s, t=t)
    off = score.copy()
    off[7, 0] += np.float32(4 * tl[7, 0]) + np.float32(1e-30)
    with pytest.raises(AssertionError):
        KC.assert_valid_topk(idx, off, X, X, K, 0, s=s, t=t)


def test_checker_rejects_duplicate_rows_out_of_index_order():
    X = KC.case("lattice")
    s, t = KC.oracle("lattice")
    idx = ref.knn_topk(X, X, K, 0)[0]
    prev = KC._prev_duplicate(X)
    # a query whose list holds a duplicate pair (equal rows, so adjacent entries)
    pair = np.argwhere(prev[idx[:, 1:].astype(np.int64)] == idx[:, :-1])
    assert len(pair)
    q, j = pair[0]
    bad = idx.copy()
    bad[q, [j, j + 1]] = bad[q, [j + 1, j]]
    with pytest.raises(AssertionError):
        KC.assert_valid_topk(bad, None, X, X, K, 0, s=s, t=t)
    # only the larger index of a pair returned: put the last entry's later duplicate in its place
    nxt = {int(p): i for i, p in enumerate(prev) if p >= 0}
    cand = [(qq, nxt[int(idx[qq, K - 1])]) for qq in range(X.shape[0])
            if int(idx[qq, K - 1]) in nxt and nxt[int(idx[qq, K - 1])] not in idx[qq] and nxt[int(idx[qq, K - 1])] != qq]
    assert cand
    q, c = cand[0]
    bad = idx.copy()
    bad[q, K - 1] = c
    with pytest.raises(AssertionError):
        KC.assert_valid_topk(bad, None, X, X, K, 0, s=s, t=t)
