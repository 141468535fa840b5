"""The oracles of _metric_cases.py and the CPU paths of ops/metrics.py, ops/reference.py and
ops/split.py against brute force, on the special-value inputs (repeated +-inf in both classes, both
zeros, denormals, negatives, keys one byte apart).  Runs everywhere; the GPU files
test_metric_kernels_gpu.py and test_select_split_kernels_gpu.py then hold the kernels to the same
oracles."""
import numpy as np
import pytest
import torch

import _metric_cases as C
from fraud_detection_amd.ops import metrics as M
from fraud_detection_amd.ops import reference as ref
from fraud_detection_amd.ops import reference_gbdt as R
from fraud_detection_amd.ops import split as SP

SIZES = [(20, 0), (97, 1), (300, 2), (1000, 3), (2000, 4)]


def _cases():
    yield "inf_ties", C.inf_tie_case()
    for n, seed in SIZES:
        yield f"special-{n}", C.special_scores(n, seed)
    yield "heavy-1500", C.heavy_ties(1500, 5)


CASES = dict(_cases())


def test_special_scores_hold_what_they_promise():
    s, y = C.special_scores(1000, 3)
    assert s.dtype == np.float32 and y.dtype == np.uint8 and not np.isnan(s).any()
    pos = y != 0
    bits = C.f32_bits(s)
    for cls in (pos, ~pos):
        assert np.count_nonzero(np.isposinf(s[cls])) >= 2 and np.count_nonzero(np.isneginf(s[cls])) >= 2
        assert {0x00000000, 0x80000000, 0x00000001, 0x80000001} <= set(bits[cls].tolist())
        assert np.any(s[cls] < 0)
    one = int(ref.order_key(np.float32([1.0]))[0])
    keys = ref.order_key(s).astype(np.int64)
    for byte in range(4):  # a key that differs from 1.0's in this byte alone
        x = keys ^ one
        assert np.any((x != 0) & ((x & ~(0xFF << (8 * byte))) == 0)), byte


def test_order_key_is_the_float_order():
    s, _ = C.special_scores(300, 2)
    k = ref.order_key(s).astype(np.int64)
    assert np.array_equal(s[:, None] < s[None, :], k[:, None] < k[None, :])
    assert np.array_equal(s[:, None] == s[None, :], k[:, None] == k[None, :])
    back = ref.order_key_inv(ref.order_key(s))
    assert np.array_equal(back, s) and not np.any(C.f32_bits(back) == 0x80000000)


def test_inf_tie_reproduction():
    """Tied infinite scores form one tie group.  Tie bounds taken from np.diff made inf - inf = NaN a
    boundary between every two of them and ranked them as distinct: 106 on this input, where brute
    force over all pairs counts 102."""
    s, y = C.inf_tie_case()
    assert C.brute_twice_pairs(s, y) == 102 and C.counts(y) == (10, 10)
    assert R.twice_pairs(s, y) == 102
    assert ref.auc_twice_pairs(s, y) == 102
    assert ref.roc_auc(s, y) == 102 / 200  # rank sum and quotient are exact at this size
    assert M.auc_pair_counts(torch.from_numpy(s), torch.from_numpy(y)) == (102, 10, 10)


@pytest.mark.parametrize("name", list(CASES))
def test_auc_paths_equal_brute_force(name):
    s, y = CASES[name]
    P, N = C.counts(y)
    want = C.brute_twice_pairs(s, y)
    assert R.twice_pairs(s, y) == want
    assert ref.auc_twice_pairs(s, y) == want
    assert ref.auc_twice_pairs(s.astype(np.float64), y) == want
    assert M.auc_pair_counts(torch.from_numpy(np.array(s)), torch.from_numpy(np.array(y))) == (want, P, N)
    # at most 2000 rows: the rank sums stay far below 2^53, so the float names the integer exactly
    assert int(round(ref.roc_auc(s, y) * 2 * P * N)) == want
    assert int(round(ref.roc_auc(s.astype(np.float64), y) * 2 * P * N)) == want
    assert M.roc_auc(torch.from_numpy(np.array(s)), torch.from_numpy(np.array(y))) == want / (2.0 * P * N)


def test_auc_pair_counts_cpu_is_an_integer_sum():
    """The CPU path returns the integer itself (int64 sum of doubled ranks), not a rounded float:
    above brute-force sizes it equals the independent searchsorted count."""
    s, y = C.heavy_ties(200_003, 6)
    twice, P, N = M.auc_pair_counts(torch.from_numpy(s), torch.from_numpy(y))
    assert type(twice) is int and (twice, P, N) == (R.twice_pairs(s, y), *C.counts(y))
    s, y = C.special_scores(200_003, 7)
    assert M.auc_pair_counts(torch.from_numpy(np.array(s)), torch.from_numpy(np.array(y)))[0] == R.twice_pairs(s, y)


@pytest.mark.parametrize("name", list(CASES))
def test_auc_matches_sklearn_on_finite_scores(name):
    """sklearn rejects infinities, so it sees the finite rows only (brute force is the authority on
    the rest).  Its trapezoid sum is fp64 over at most n terms in [0, 1]: n 2^-52 bounds the gap."""
    from sklearn.metrics import roc_auc_score

    s, y = C.finite_only(*CASES[name])
    P, N = C.counts(y)
    if P == 0 or N == 0:
        pytest.fail("case lost a class with its infinities")
    assert abs(roc_auc_score(y != 0, s) - C.brute_twice_pairs(s, y) / (2.0 * P * N)) <= len(s) * 2.0 ** -52
    assert abs(roc_auc_score(y != 0, s) - ref.roc_auc(s, y)) <= 2 * len(s) * 2.0 ** -52


@pytest.mark.parametrize("name", list(CASES))
def test_pr_curve_and_ap_q_equal_threshold_walk(name):
    s, y = CASES[name]
    thr, tp, fp = C.brute_pr_curve(s, y)
    gthr, gtp, gfp = ref.pr_curve(s, y)
    assert np.array_equal(C.f32_bits(gthr), C.f32_bits(thr))  # bit patterns: +0.0 for the zeros, +-inf
    assert np.array_equal(gtp, tp) and np.array_equal(gfp, fp)
    P, N = C.counts(y)
    assert ref.average_precision_q(s, y) == (C.brute_ap_q(tp, fp), P, N)
    mthr, mtp, mfp = M.pr_curve(torch.from_numpy(np.array(s)), torch.from_numpy(np.array(y)))
    assert np.array_equal(C.f32_bits(mthr), C.f32_bits(thr)) and np.array_equal(mtp, tp) and np.array_equal(mfp, fp)


@pytest.mark.parametrize("bits", [8, 11, 16, 20])
def test_histogram_oracles_equal_brute_force_on_shifted_keys(bits):
    s = np.concatenate([C.bin_edge_scores(bits), C.special_scores(300, 2)[0]])
    y = (np.random.default_rng(bits).random(s.shape[0]) < 0.4).astype(np.uint8)
    h = C.hist_counts(s, y, bits)
    P, N = C.counts(y)
    assert h.shape == (2, 1 << bits) and int(h[1].sum()) == P and int(h[0].sum()) == N
    k = (ref.order_key(s) >> np.uint32(32 - bits)).astype(np.int64)
    pos = y != 0
    for b in np.unique(k):  # the counts, bin by bin
        assert h[1, b] == np.count_nonzero(pos & (k == b)) and h[0, b] == np.count_nonzero(~pos & (k == b))
    kp, kn = k[pos][:, None], k[~pos][None, :]
    want = 2 * int(np.count_nonzero(kp > kn)) + int(np.count_nonzero(kp == kn))
    assert C.hist_twice_pairs(h) == (want, P, N)
    hc = M.score_histogram(torch.from_numpy(s), torch.from_numpy(y), bits)
    assert np.array_equal(hc.numpy(), h)
    assert M.auc_from_histogram(hc) == (want, P, N)
    # an edge pair really straddles a bin boundary: consecutive keys, different bins
    key = np.unique(ref.order_key(s)).astype(np.int64)
    step = np.flatnonzero(np.diff(key) == 1)
    assert np.count_nonzero((key[step] >> (32 - bits)) != (key[step + 1] >> (32 - bits))) >= 6


def test_hist_twice_pairs_past_2_32():
    h = np.zeros((2, 256), dtype=np.int64)
    h[1, [3, 200, 255]] = [0xFFFFFFFF, 0xFFFFFFFF, 7]
    h[0, [0, 3, 199, 255]] = [5, 11, 0xFFFFFFFF, 2]
    want = 0xFFFFFFFF * (2 * 5 + 11) + 0xFFFFFFFF * 2 * (16 + 0xFFFFFFFF) + 7 * (2 * (16 + 0xFFFFFFFF) + 2)
    assert C.hist_twice_pairs(h) == (want, 2 * 0xFFFFFFFF + 7, 18 + 0xFFFFFFFF)


@pytest.mark.parametrize("m,d,max_bin", [(1, 1, 2), (3, 5, 37), (257, 32, 256), (300, 4, 255)])
def test_select_picks_equal_python_sorted(m, d, max_bin):
    sample, kinds = C.select_sample(m, d, offset=m % 11)
    cnt = [(-3, 0, 1, m - 1, m, m + 9)[f % 6] for f in range(d)]
    for counts in (None, cnt):
        got = C.select_picks(sample, max_bin, counts)
        for f in range(d):
            col = [float(v) for v in sample[:, f]]
            srt = sorted(v for v in col if v == v) + [v for v in col if v != v]  # NaN last, as np.sort
            mf = m if counts is None else min(max(counts[f], 0), m)
            exp = np.array([srt[0]] + [srt[(t * mf) // max_bin] for t in range(1, max_bin)], dtype=np.float32)
            assert np.array_equal(got[:, f], exp, equal_nan=True), (kinds[f], f)
    if d == 32:
        assert set(kinds) == set(C.SELECT_KINDS)


def test_picks_mismatch_sees_each_fault():
    exp = np.array([[0.0, np.nan], [1.0, 2.0]], dtype=np.float32)
    assert C.picks_mismatch(exp.copy(), exp) is None
    neg = exp.copy()
    neg[0, 0] = -0.0
    assert "sign" in C.picks_mismatch(neg, exp)
    assert C.picks_mismatch(np.where(np.isnan(exp), np.float32(3), exp), exp).startswith("NaN")
    off = exp.copy()
    off[1, 1] = np.nextafter(np.float32(2), np.float32(3))
    assert "differ" in C.picks_mismatch(off, exp)
    assert C.picks_mismatch(np.array([[-0.0]], np.float32), np.array([[0.0]], np.float32)) is not None
    assert C.picks_mismatch(np.array([[0.0]], np.float32), np.array([[-0.0]], np.float32)) is None


GRID_N = [1, 2, 3, 15, 16, 17, 31, 33, 255, 257]


@pytest.mark.parametrize("n", GRID_N)
def test_split_properties_hold_for_assign_numpy(n):
    seen = 0
    for n1 in sorted({0, 1, 2, 3, n // 2, n - 1, n} & set(range(n + 1))):
        y = C.split_labels(n, n1, other_bytes=n1 % 2 == 1)
        for frac in (0.0, 0.2, 0.5, 1.0):
            for k in (0, 1, 2, 5, 254):
                codes = SP.assign_numpy(y, frac, k, 42)
                assert C.split_properties(codes, y, frac, k) == [], (n, n1, frac, k)
                seen += 1
    assert seen >= 20 * 2


def test_split_properties_sees_each_fault():
    y = C.split_labels(257, 100)
    good = SP.assign_numpy(y, 0.2, 5, 42)
    assert C.split_properties(good, y, 0.2, 5) == []
    bad = good.copy()
    bad[np.flatnonzero((y == 1) & (good == C.TEST))[0]] = 0      # one test row fewer, fold 0 one larger
    assert len(C.split_properties(bad, y, 0.2, 5)) == 2
    bad = good.copy()
    i, j = np.flatnonzero((y == 0) & (good == 4))[:2]
    bad[[i, j]] = 0                                              # sizes now differ by more than one
    assert C.split_properties(bad, y, 0.2, 5) != []
    bad = good.copy()
    bad[np.flatnonzero(good == 1)[0]] = 7                        # a code >= k
    assert C.split_properties(bad, y, 0.2, 5) != []
    assert C.split_properties(good, y, 0.2, 1) != []             # k <= 1 admits only code 0
    swapped = good.copy()
    a, b = np.flatnonzero((y == 1) & (good == 0))[0], np.flatnonzero((y == 0) & (good == 4))[0]
    swapped[[a, b]] = swapped[[b, a]]                            # per class, not only overall
    assert C.split_properties(swapped, y, 0.2, 5) != []
