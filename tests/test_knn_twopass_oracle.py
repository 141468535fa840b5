"""The two-pass k-NN rule (engine bf16x3t, knn.hip knn_groupmax / knn_threshold / knn_filter kernels)
emulated in numpy on the named cases of _knn_cases.py; no GPU.

Rule.  A query's candidates fall into the 32 groups c mod 32 (the accumulator register and wave half
that hold the candidate's score).  Pass 1 keeps every group's largest approximate score (self
excluded), v_K is the K-th largest of the 32 group maxima -- or, ``per_slice``, of the nsplit x 32
maxima kept apart per candidate slice -- and M the query's largest margin; T = v_K - M.  Pass 2
lists the candidates with approx + m >= T.  The K groups' best candidates are K distinct candidates
with exact >= approx - m >= T, so s_k >= T and every candidate with exact >= s_k is listed.

Two broken rules the checks must catch:
  ``no_margin``       T = v_K: exact scores lie on both sides of the approximate ones, so T > s_k for
                      about half the queries;
  ``all_candidates``  v_K = the K-th largest approximate score over ALL candidates.  That threshold is
                      valid too, but it is not what a pass that keeps one maximum per group can
                      compute: it equals the group rule's exactly when the K best candidates sit in K
                      different groups, which for K candidates at random positions has probability
                      p = prod_{i<K} (1 - i / 32) (0.724 for K = 5, 0.383 for K = 8).  On ``normal``
                      (1000 iid rows) the share of queries with T_group = T_all must lie within 4
                      binomial standard deviations of p; the broken rule gives 1.
"""
import functools

import numpy as np
import pytest

import _knn_cases as KC

LIST_CAP = 64  # knn.hip kListCap
KS = (1, 5, 8)
SLICES = (1, 3)


@functools.lru_cache(maxsize=None)
def _inputs(name):
    X = KC.case(name)
    a = KC.approx_scores(X, X)
    np.fill_diagonal(a, -np.inf)  # self_offset 0: the self candidate never enters a maximum or a list
    return a, KC.margins(X, X), KC.scores64(X, X, 0)


def _kth_largest(v, k):
    return -np.partition(-v, k - 1, axis=1)[:, k - 1]


def slice_of_tile(tiles, nsplit):
    """[tiles] the kernels' slice of every candidate tile: slice y owns tiles [tiles y / n, tiles (y + 1) / n)."""
    out = np.empty(tiles, dtype=np.int64)
    for y in range(nsplit):
        out[tiles * y // nsplit: tiles * (y + 1) // nsplit] = y
    return out


def two_pass(name, k, nsplit, per_slice=False, rule="group"):
    """T [mq], passed [mq, mc], the longest (slice, half) list per query [mq], for the given rule."""
    a, mg, s = _inputs(name)
    mq, mc = a.shape
    tiles = (mc + 31) // 32
    sl = slice_of_tile(tiles, nsplit)[np.arange(mc) // 32]
    cell = np.arange(mc) % 32 + (32 * sl if per_slice else 0)
    ncell = 32 * (nsplit if per_slice else 1)
    gm = np.full((mq, ncell), -np.inf)
    for g in range(ncell):
        cols = np.flatnonzero(cell == g)
        if cols.size:
            gm[:, g] = a[:, cols].max(axis=1)
    M = mg.max(axis=1)
    vk = _kth_largest(a, k) if rule == "all_candidates" else _kth_largest(gm, k)
    T = vk - (0.0 if rule == "no_margin" else M)
    passed = (a + mg) >= T[:, None]
    half = KC.lane_half(mc)
    longest = np.zeros(mq, dtype=np.int64)
    for y in range(nsplit):
        for h in (0, 1):
            longest = np.maximum(longest, passed[:, (sl == y) & (half == h)].sum(axis=1))
    return T, passed, longest


def distinct_groups_probability(k, groups=32):
    return float(np.prod([1.0 - i / groups for i in range(k)]))


def check(name, k, nsplit, per_slice=False, rule="group"):
    a, mg, s = _inputs(name)
    T, passed, longest = two_pass(name, k, nsplit, per_slice, rule)
    sk = _kth_largest(s, k)
    assert np.all(T <= sk), ("T above the exact k-th best", name, k, int(np.sum(T > sk)))
    lost = (s >= sk[:, None]) & ~passed
    assert not lost.any(), ("an exact contender is not listed", name, k, int(lost.sum()))
    over = longest > LIST_CAP
    if name == "lattice":
        assert np.array_equal(over, KC.lattice_tight(k)), ("overflowing queries", int(over.sum()))
    else:
        assert not over.any() and longest.max() <= LIST_CAP, (name, int(longest.max()))
    if name == "normal" and not per_slice:
        # the rule keeps ONE maximum per group (see the module docstring)
        T_all = _kth_largest(a, k) - mg.max(axis=1)
        assert np.all(T <= T_all)
        p, n = distinct_groups_probability(k), a.shape[0]
        share = float(np.mean(T == T_all))
        assert abs(share - p) <= 4.0 * np.sqrt(p * (1.0 - p) / n) + 1e-12, ("share of T_group = T_all", k, share, p)
    return passed.sum(axis=1), longest


@pytest.mark.parametrize("nsplit", SLICES)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", KC.CASES)
def test_two_pass_rule_lists_every_contender(name, k, nsplit):
    for per_slice in (False, True):
        n, longest = check(name, k, nsplit, per_slice)
        print(f"[twopass] {name} k={k} nsplit={nsplit} per_slice={per_slice}: listed per query "
              f"{n.mean():.2f} (max {n.max()}), longest lane list {longest.max()}")


def test_per_slice_groups_give_a_threshold_at_least_as_tight():
    for name in KC.CASES:
        T1 = two_pass(name, 5, 3)[0]
        T3 = two_pass(name, 5, 3, per_slice=True)[0]
        assert np.all(T3 >= T1)
    assert np.array_equal(two_pass("normal", 5, 1)[0], two_pass("normal", 5, 1, per_slice=True)[0])


@pytest.mark.parametrize("rule", ["no_margin", "all_candidates"])
def test_broken_rules_are_caught(rule):
    caught = []
    for name in KC.CASES:
        for k in KS:
            try:
                check(name, k, 1, rule=rule)
            except AssertionError:
                caught.append((name, k))
    assert caught, rule
    if rule == "no_margin":  # T = v_K lies above s_k wherever the approximate error is positive
        assert any(n == "normal" for n, _ in caught)
    else:  # k = 1: the two rules coincide (one candidate is always in one group)
        assert ("normal", 5) in caught and ("normal", 8) in caught and ("normal", 1) not in caught
