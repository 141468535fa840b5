"""Every kernel of auc.hip against the exact oracles of _metric_cases.py (validated on the CPU by
test_metric_oracle.py), path by path, at the smallest shapes that can break it, on MI355X.

Which test launches which kernel:

  auc_compact_kernel            test_auc_compact[*] (direct; 524 289: the second grid-stride sweep),
                                test_chunked_chain[*]
  sort_chunks_kernel            test_sort_chunks[64 / 1024 / 2048 / 16384] (direct), test_sort_chunks_guards,
                                test_chunked_chain[*]
  auc_count_kernel              test_auc_count_* (direct, on oracle-sorted chunks; ..._second_sweep:
                                2 097 160 rows), test_auc_count_guard, test_chunked_chain[*]
  confusion_kernel              test_confusion[1 / 257 / 2097160]
  radix_init_kernel             test_radix_sort[*] (1 048 577: its second sweep), test_radix_count_*
  radix_hist_kernel             test_radix_sort[*] (per-block ranges of 256, 512 and 768 rows)
  radix_rowscan_kernel          test_radix_sort[*]
  radix_scatter_kernel          test_radix_sort[*] (partial last sub-chunk at 257, 262 145, 524 289)
  auc_sorted_count_kernel       test_radix_sort[*], test_radix_count_second_sweep, test_radix_count_one_segment,
                                test_radix_count_lone_positive
  auc_sorted_finalize_kernel    the same tests (res = twice_pairs, P, N)
  auc_hist_kernel               test_auc_hist[8 / 11 / 16 / 20 / 24], test_auc_hist_guards
  auc_hist_reduce_kernel        test_auc_hist_reduce[256 / 2048 / 65536], test_auc_hist_reduce_past_2_32,
                                test_auc_hist_guards
  pr_tile_totals_kernel, pr_tile_scan_kernel, pr_emit_kernel, pr_ap_kernel, pr_finalize_kernel
                                test_pr_curve_special_values[*] (their sizes and tile edges:
                                test_pr_metrics_gpu.py)

Every comparison is integer or bit-pattern equality: there is no tolerance in this file.  No score is
a NaN (unsupported, nothing is pinned about it).  Every guard test relies on a host-side throw in
the launcher, before any launch: no kernel runs with arguments outside its contract.
"""
import numpy as np
import pytest
import torch

import _metric_cases as C
from fraud_detection_amd.ops import metrics as M
from fraud_detection_amd.ops import reference as ref
from fraud_detection_amd.ops import reference_gbdt as R
from fraud_detection_amd.ops.native import native, ptr, stream_of

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC0BEEF   # a NaN pattern no score carries: a kernel that reads or moves it shows
SWEEP2 = 2_097_153 + 7  # auc_count / confusion: 1024 blocks x 256 threads x 8 rows, + 1, + a ragged tail


def _dev(a, dev) -> torch.Tensor:
    return torch.from_numpy(np.array(a)).to(dev)


def _u32(t: torch.Tensor) -> np.ndarray:
    return t.view(torch.int32).cpu().numpy().view(np.uint32)


def _sentinel_buf(n: int, dev) -> torch.Tensor:
    return torch.full((n,), SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)


def _counter(v: int, dev) -> torch.Tensor:
    return torch.tensor([v], dtype=torch.int64, device=dev)


# ---- A. auc_compact_kernel ------------------------------------------------------------------------
def _label_cases(y: np.ndarray):
    n = y.shape[0]
    other = y.copy()
    hit = np.flatnonzero(y)
    other[hit[0::2]] = 2
    other[hit[1::2]] = 255
    last = np.zeros(n, dtype=np.uint8)
    last[-3:] = 1
    return {"mixed": y, "zeros": np.zeros(n, np.uint8), "ones": np.ones(n, np.uint8), "bytes_2_255": other,
            "last_three": last}


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 524_288, 524_289])
def test_auc_compact(dev, n):
    s, y0 = C.special_scores(n, 11)
    sd = _dev(s, dev)
    for name, y in _label_cases(np.array(y0)).items():
        P = int(np.count_nonzero(y))
        pos = _sentinel_buf(n + 8, dev)
        counter, yd = _counter(0, dev), _dev(y, dev)
        native().auc_compact(ptr(sd), ptr(yd), n, ptr(pos), ptr(counter), stream_of(sd))
        assert int(counter.item()) == P, (name, n)
        got = _u32(pos)
        # the order across waves is not defined: the multiset of bit patterns is
        assert np.array_equal(np.sort(got[:P]), np.sort(C.f32_bits(s[y != 0]))), (name, n)
        assert np.all(got[P:] == SENTINEL), (name, n)


# ---- B. sort_chunks_kernel ------------------------------------------------------------------------
def _sort_chunks(vals: np.ndarray, P: int, chunk: int, nchunks: int, dev) -> np.ndarray:
    pos = _sentinel_buf(P + 16, dev)
    pos[:P] = _dev(vals, dev)
    counter = _counter(P, dev)
    native().sort_chunks(ptr(pos), pos.shape[0], ptr(counter), chunk, nchunks, stream_of(pos))
    return _u32(pos)


@pytest.mark.parametrize("chunk", [64, 1024, 2048, 16384])
def test_sort_chunks(dev, chunk):
    """Below the 1024-thread block, equal to it, two elements per thread, the maximum.  The values hold
    duplicates, real +inf beside the +inf padding of a partial chunk, -inf, denormals and both zeros."""
    for P in (1, chunk - 1, chunk, chunk + 1, 2 * chunk + chunk // 2 + 1):
        vals = np.array(C.special_scores(P, chunk)[0])
        nchunks = (P + chunk - 1) // chunk + 1  # one more than needed: that block returns at lo >= P
        got = _sort_chunks(vals, P, chunk, nchunks, dev)
        assert np.all(got[P:] == SENTINEL), (chunk, P)
        for lo in range(0, P, chunk):
            sl = slice(lo, min(lo + chunk, P))
            # by value (bitonic is not stable: -0.0 / +0.0 may swap), and nothing lost or invented
            assert np.array_equal(got[sl].view(np.float32), np.sort(vals[sl])), (chunk, P, lo)
            assert np.array_equal(np.sort(got[sl]), np.sort(C.f32_bits(vals[sl]))), (chunk, P, lo)


def test_sort_chunks_guards(dev):
    """launch_sort_chunks checks chunk before anything else and returns on nchunks <= 0."""
    vals = np.array(C.special_scores(100, 1)[0])
    pos = _sentinel_buf(116, dev)
    pos[:100] = _dev(vals, dev)
    counter = _counter(100, dev)
    for chunk in (0, 48, 100, 32768):
        with pytest.raises(RuntimeError, match="power of two"):
            native().sort_chunks(ptr(pos), 116, ptr(counter), chunk, 1, stream_of(pos))
    native().sort_chunks(ptr(pos), 116, ptr(counter), 128, 0, stream_of(pos))
    assert np.array_equal(_u32(pos)[:100], C.f32_bits(vals)) and np.all(_u32(pos)[100:] == SENTINEL)


# ---- C. auc_count_kernel, on oracle-sorted chunks --------------------------------------------------
def _auc_count(s: np.ndarray, y: np.ndarray, chunk: int, extra_chunks: int, dev) -> int:
    positives = s[y != 0]
    P = positives.shape[0]
    for lo in range(0, P, chunk):
        positives[lo:lo + chunk] = np.sort(positives[lo:lo + chunk])
    pos = _sentinel_buf(P + 16, dev)
    pos[:P] = _dev(positives, dev)
    out = torch.zeros(1, dtype=torch.int64, device=dev)
    sd, yd, counter = _dev(s, dev), _dev(y, dev), _counter(P, dev)  # named: alive until the read-back
    native().auc_count(ptr(sd), ptr(yd), s.shape[0], ptr(pos), ptr(counter), chunk,
                       (P + chunk - 1) // chunk + extra_chunks, ptr(out), stream_of(sd))
    return int(out.item())


def _exact_positives(n: int, P: int, seed: int):
    """Special-value scores with exactly P positives, and negatives equal to +-inf and to the largest
    and the smallest positive."""
    s = np.array(C.special_scores(n, seed)[0])
    rng = np.random.default_rng([n, P, seed])
    y = np.zeros(n, dtype=np.uint8)
    y[rng.permutation(n)[:P]] = 1
    neg = np.flatnonzero(y == 0)
    s[neg[:4]] = [np.inf, -np.inf, s[y != 0].max(), s[y != 0].min()]
    return s, y


@pytest.mark.parametrize("extra", [0, 2])
def test_auc_count_three_small_chunks(dev, extra):
    """chunk = 64 with 150 positives: two full chunks and a partial one."""
    s, y = _exact_positives(1000, 150, 3)
    assert _auc_count(s, y, 64, extra, dev) == C.brute_twice_pairs(s, y)


def test_auc_count_two_full_size_chunks(dev):
    s, y = _exact_positives(30_011, 20_000, 4)
    assert _auc_count(s, y, 16384, 0, dev) == R.twice_pairs(s, y)


def test_auc_count_without_negatives(dev):
    s = np.array(C.special_scores(500, 5)[0])
    assert _auc_count(s, np.full(500, 7, dtype=np.uint8), 64, 1, dev) == 0


def test_auc_count_second_sweep(dev):
    s, y = C.heavy_ties(SWEEP2, 6, rate=0.001)
    assert _auc_count(s, y, 4096, 0, dev) == R.twice_pairs(s, y)


def test_auc_count_guard(dev):
    """The kernel's LDS array holds 16384 floats: the launcher refuses a larger or crooked chunk before
    any launch."""
    t = torch.zeros(64, dtype=torch.float32, device=dev)
    y = torch.zeros(64, dtype=torch.uint8, device=dev)
    out, counter = torch.zeros(1, dtype=torch.int64, device=dev), _counter(0, dev)
    for chunk in (0, 100, 32768):
        with pytest.raises(RuntimeError, match="power of two"):
            native().auc_count(ptr(t), ptr(y), 64, ptr(t), ptr(counter), chunk, 1, ptr(out), stream_of(t))
    assert int(out.item()) == 0


# ---- D. the chunked chain and the radix path on the same inputs ------------------------------------
CHAIN = {"inf_ties": C.inf_tie_case, "special-97": lambda: C.special_scores(97, 1),
         "special-1000": lambda: C.special_scores(1000, 3), "special-2000": lambda: C.special_scores(2000, 4),
         "heavy-1500": lambda: C.heavy_ties(1500, 5), "special-70001": lambda: C.special_scores(70_001, 8)}


@pytest.mark.parametrize("name", list(CHAIN))
def test_chunked_chain(dev, name):
    s, y = (np.array(a) for a in CHAIN[name]())
    P, N = C.counts(y)
    want = C.brute_twice_pairs(s, y) if s.shape[0] <= C.BRUTE_MAX else R.twice_pairs(s, y)
    sd, yd = _dev(s, dev), _dev(y, dev)
    assert M.auc_pair_counts(sd, yd) == (want, P, N)
    assert M.auc_pair_counts(torch.from_numpy(s), torch.from_numpy(y)) == (want, P, N)  # the CPU path
    auc, twice = M.auc_known_positives(sd, yd, P)
    assert int(twice.item()) == want
    _, res = M.auc_radix(sd, yd)
    assert tuple(int(v) for v in res.cpu()) == (want, P, N)


# ---- E. confusion_kernel --------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 257, SWEEP2])
def test_confusion(dev, n):
    s, y = C.heavy_ties(n, 7)  # a grid of k / 4 with +-inf and both zeros: every level heavily tied
    y = y.copy()
    y[(y != 0) & (np.arange(n) % 3 == 0)] = 2
    y[(y != 0) & (np.arange(n) % 3 == 1)] = 255
    sd, yd = _dev(s, dev), _dev(y, dev)
    pos = y != 0
    # 0.3: the binding narrows the threshold to float32, so the oracle compares with np.float32(0.3)
    # (0.25 < float32(0.3) < 0.5 on this grid either way; the narrowing is part of the contract)
    for thr in (0.25, np.inf, -np.inf, -0.0, 0.0, 0.3, -1.5):
        pred = s > np.float32(thr)  # strict: a score equal to the threshold is a negative call
        want = [np.count_nonzero(~pos & ~pred), np.count_nonzero(~pos & pred), np.count_nonzero(pos & ~pred),
                np.count_nonzero(pos & pred)]
        assert M.confusion_counts(sd, yd, thr).tolist() == want, (n, thr)


# ---- F. the radix sort, read out of the caller's workspace -----------------------------------------
def _radix(s: np.ndarray, y: np.ndarray, dev):
    """(sorted keys, sorted labels, res) of auc_radix.  radix_sort_pairs starts with the rows in
    regions [0] / [2] of auc_radix_layout and swaps the (in, out) pair after each of its five passes
    (label digit + four key bytes): an odd number of swaps, so the sorted keys sit in region [1] and
    the sorted labels in region [3]."""
    n = s.shape[0]
    m = native()
    off = [int(v) for v in m.auc_radix_layout(n)]
    ws = torch.zeros(int(m.auc_radix_workspace_bytes(n)), dtype=torch.uint8, device=dev)
    assert off[7] == ws.numel() and ws.data_ptr() % 256 == 0
    res = torch.empty(3, dtype=torch.int64, device=dev)
    auc = torch.empty((), dtype=torch.float64, device=dev)
    sd, yd = _dev(s, dev), _dev(y, dev)
    m.auc_radix(ptr(sd), ptr(yd), n, ptr(ws), ptr(res), ptr(auc), stream_of(sd))
    keys = ws[off[1]:off[1] + 4 * n].cpu().numpy().view(np.uint32)
    labs = ws[off[3]:off[3] + n].cpu().numpy()
    return keys, labs, tuple(int(v) for v in res.cpu())


def _radix_inputs(n: int):
    rng = np.random.default_rng(n)
    y = (rng.random(n) < 0.4).astype(np.uint8)
    y[y != 0] = rng.choice(np.array([1, 2, 255], dtype=np.uint8), int(np.count_nonzero(y)))
    one = np.uint32(0x3F800000)
    yield "identical", np.full(n, 1.5, dtype=np.float32), y
    yield "byte0", C.bits_f32(one | rng.integers(0, 256, n).astype(np.uint32)), y
    # byte 3 = sign and the upper seven exponent bits: finite for every value of the byte
    yield "byte3", C.bits_f32(rng.integers(0, 256, n).astype(np.uint32) << np.uint32(24)), y
    yield "digits256", C.bits_f32(one | (rng.permutation(n).astype(np.uint32) % np.uint32(256)) << np.uint32(8)), y
    s, ys = C.special_scores(n, 9)
    yield "special", np.array(s), np.array(ys)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 262_144, 262_145, 524_288, 524_289, 1_048_577])
def test_radix_sort(dev, n):
    for name, s, y in _radix_inputs(n):
        assert not np.isnan(s).any()
        keys, labs, res = _radix(s, y, dev)
        wk, wl = C.sorted_pairs(s, y)
        assert np.array_equal(keys, wk), (name, n)
        assert np.array_equal(labs, wl), (name, n)
        P, N = C.counts(y)
        assert res == (R.twice_pairs(s, y) if P and N else 0, P, N), (name, n)


def test_radix_count_second_sweep(dev):
    """auc_sorted_count_kernel past one sweep of its grid, with mixed tie segments far longer than a
    block's rows."""
    s, y = C.heavy_ties(SWEEP2, 10)
    keys, labs, res = _radix(s, y, dev)
    wk, wl = C.sorted_pairs(s, y)
    assert np.array_equal(keys, wk) and np.array_equal(labs, wl)
    assert res == (R.twice_pairs(s, y), *C.counts(y))


@pytest.mark.parametrize("ends", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_radix_count_one_segment(dev, ends):
    """One tie segment over sorted rows 1 .. n - 2 with a lone row of either class on each side."""
    n = 5003
    rng = np.random.default_rng(n)
    s = np.zeros(n, dtype=np.float32)
    s[rng.random(n) < 0.5] = -0.0
    y = (rng.random(n) < 0.3).astype(np.uint8)
    s[17], s[4000] = -2.0, 3.0
    y[17], y[4000] = ends
    _, _, res = _radix(s, y, dev)
    assert res == (R.twice_pairs(s, y), *C.counts(y))
    small = slice(0, 1500)  # the same shape under brute force
    s2, y2 = s[small].copy(), y[small].copy()
    s2[1000], y2[1000] = 3.0, ends[1]
    assert _radix(s2, y2, dev)[2] == (C.brute_twice_pairs(s2, y2), *C.counts(y2))


@pytest.mark.parametrize("top", [False, True])
def test_radix_count_lone_positive(dev, top):
    n = 1025
    s = np.random.default_rng(n).permutation(n).astype(np.float32) - 500
    y = np.zeros(n, dtype=np.uint8)
    y[np.argmax(s) if top else np.argmin(s)] = 1
    keys, labs, res = _radix(s, y, dev)
    assert int(np.flatnonzero(labs)[0]) == (n - 1 if top else 0)
    assert res == (2 * (n - 1) if top else 0, 1, n - 1)


# ---- G. auc_hist_kernel ---------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [8, 11, 16, 20, 24])
def test_auc_hist(dev, bits):
    """Scores on both sides of bin edges (the largest key of bin b, the smallest of b + 1), +-inf, both
    zeros and denormals.  bits = 24 is the launcher's maximum: 128 MiB of counters."""
    s = np.concatenate([C.bin_edge_scores(bits), np.array(C.special_scores(5000, bits)[0])])
    y = np.random.default_rng(bits).choice(np.array([0, 0, 1, 2, 255], dtype=np.uint8), s.shape[0])
    h = M.score_histogram(_dev(s, dev), _dev(y, dev), bits)
    assert tuple(h.shape) == (2, 1 << bits)
    assert np.array_equal(h.cpu().numpy().astype(np.int64), C.hist_counts(s, y, bits))
    if bits < 24:  # the reduce kernel on a scored histogram as well
        assert M.auc_from_histogram(h) == C.hist_twice_pairs(C.hist_counts(s, y, bits))


def test_auc_hist_guards(dev):
    """Both launchers check bits before any launch."""
    t = torch.zeros(64, dtype=torch.float32, device=dev)
    y = torch.zeros(64, dtype=torch.uint8, device=dev)
    h = torch.zeros(2 << 8, dtype=torch.int32, device=dev)
    out = torch.zeros(3, dtype=torch.int64, device=dev)
    for bits in (7, 25):
        with pytest.raises(RuntimeError, match=r"\[8, 24\]"):
            native().auc_hist(ptr(t), ptr(y), 64, bits, ptr(h), stream_of(t))
        with pytest.raises(RuntimeError, match=r"\[8, 24\]"):
            native().auc_hist_reduce(ptr(h), bits, ptr(out), stream_of(h))
    assert int(h.sum().item()) == 0 and out.cpu().tolist() == [0, 0, 0]


# ---- H. auc_hist_reduce_kernel on synthetic histograms ---------------------------------------------
def _reduce(h: np.ndarray, dev):
    nb = h.shape[1]
    hd = torch.from_numpy(np.ascontiguousarray(h, dtype=np.uint32).view(np.int32).reshape(-1)).to(dev)
    out = torch.zeros(3, dtype=torch.int64, device=dev)
    native().auc_hist_reduce(ptr(hd), nb.bit_length() - 1, ptr(out), stream_of(hd))
    return tuple(int(v) & 0xFFFFFFFFFFFFFFFF for v in out.cpu().tolist())


@pytest.mark.parametrize("nb", [256, 2048, 65536])
def test_auc_hist_reduce(dev, nb):
    """One block of 1024 threads, ceil(nb / 1024) consecutive bins each: with nb = 256 threads 256 .. 1023
    own no bin."""
    per = (nb + 1023) // 1024
    rng = np.random.default_rng(nb)
    cases = {}
    for name, bins in (("first", [0]), ("last", [nb - 1]), ("first_and_last", [0, nb - 1])):
        h = np.zeros((2, nb), dtype=np.uint32)
        h[0, bins], h[1, bins] = 5, 3
        cases[name] = h
    for t in (1, 64, 65, min(512, nb // per - 1)):  # either side of a thread's range; 64: a wave boundary
        b = t * per
        for neg_bin, pos_bin in ((b - 1, b), (b, b - 1), (b - 1, b - 1), (b, b)):
            h = np.zeros((2, nb), dtype=np.uint32)
            h[0, neg_bin], h[1, pos_bin] = 7, 11
            h[0, 0], h[1, nb - 1] = 2, 1
            cases[f"edge{t}-{neg_bin}-{pos_bin}"] = h
    cases["dense"] = rng.integers(0, 1000, (2, nb)).astype(np.uint32)
    sparse = np.zeros((2, nb), dtype=np.uint32)
    sparse[rng.integers(0, 2, 40), rng.integers(0, nb, 40)] = rng.integers(1, 1 << 20, 40)  # 2 P N stays far below 2^63
    cases["sparse_large"] = sparse
    for name, h in cases.items():
        assert _reduce(h, dev) == C.hist_twice_pairs(h), (nb, name)


def test_auc_hist_reduce_past_2_32(dev):
    """P above 2^32 (what merging the histograms of many ranks gives) with 2 P N below 2^63."""
    nb = 2048
    h = np.zeros((2, nb), dtype=np.uint32)
    h[1, [1, 63, 64, 1000, 2047]] = [0xFFFFFFFF, 0xFFFFFFF0, 0xFFFFFFFF, 0xEEEEEEEE, 0xFFFFFFFF]
    h[0, [0, 1, 64, 999, 2046]] = [4_000_000, 5_000_000, 6_000_000, 7_000_000, 8_000_000]
    want = C.hist_twice_pairs(h)
    assert want[1] > 1 << 32 and 2 * want[1] * want[2] < 1 << 63
    assert _reduce(h, dev) == want


# ---- I. the precision-recall kernels on the special values -----------------------------------------
@pytest.mark.parametrize("name", ["inf_ties", "special-1000", "heavy-1500"])
def test_pr_curve_special_values(dev, name):
    s, y = (np.array(a) for a in CHAIN[name]())
    thr, tp, fp = C.brute_pr_curve(s, y)
    gthr, gtp, gfp = M.pr_curve(_dev(s, dev), _dev(y, dev))
    assert np.array_equal(C.f32_bits(gthr), C.f32_bits(thr))
    assert np.array_equal(gtp, tp) and np.array_equal(gfp, fp)
    _, res = M.average_precision_device(_dev(s, dev), _dev(y, dev))
    assert tuple(int(v) for v in res.cpu()) == (C.brute_ap_q(tp, fp), *C.counts(y), thr.shape[0])
    assert ref.average_precision_q(s, y)[0] == C.brute_ap_q(tp, fp)
