"""missing_policy="learn" on the device: every kernel that learned about the missing slot, alone
against the oracle (ops/reference_gbdt.py) on crafted state, then whole fits against the CPU path.
Integer or bitwise comparisons throughout."""
import json
import os

import numpy as np
import pytest
import torch

import _gbdt_state as S
import test_gbdt_kernels_gpu as K
from fraud_detection_amd.ops import gbdt as gb
from fraud_detection_amd.ops import reference_gbdt as R
from fraud_detection_amd.ops.native import native, ptr, stream_of

pytestmark = pytest.mark.gpu

NEG_NAN = K.NEG_NAN
GINV, HINV = K.GINV, K.HINV
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "gbdt_last_bin_nonfinite.json")


# ---- gbdt_bin<MISS> --------------------------------------------------------------------------------
def _bin_case(rng, n, d):
    """K._bin_case with 255 / 1 / 2 real bins: cut-edge values, +-inf, NaN of both signs, denormals."""
    X, cuts, nbins = K._bin_case(rng, n, d)
    for f in np.flatnonzero(nbins == 256):  # 255 real bins: drop the largest finite cut
        cuts[f, 254] = np.inf
    return X, cuts, np.minimum(nbins, 255).astype(np.int32)


@pytest.mark.parametrize("layout", ["tail_of_nan_buffer", "view_of_32", "offset_one_float"])
@pytest.mark.parametrize("d", [1, 3, 4, 8, 29, 30])
def test_bin_kernel_missing_slot(dev, d, layout):
    rng = np.random.default_rng(d)
    seen = set()
    for n in (1, 31, 32, 33, 8191):
        X, cuts, nbins = _bin_case(rng, n, d)
        seen |= set(nbins.tolist())
        Xh = torch.from_numpy(X)
        if layout == "tail_of_nan_buffer":
            buf = torch.full(((n + 4) * d,), float("nan"), dtype=torch.float32, device=dev)
            Xd = buf[4 * d:].view(n, d)
        elif layout == "view_of_32":
            buf = torch.full((n, 32), float("nan"), dtype=torch.float32, device=dev)
            Xd = buf[:, :d]
        else:
            buf = torch.full((n * d + 1,), float("nan"), dtype=torch.float32, device=dev)
            Xd = buf[1:].view(n, d)
            assert Xd.data_ptr() % 16 == 4
        Xd.copy_(Xh)
        got = gb.bin_rows(Xd, cuts, nbins, missing=True).cpu().numpy()
        ref = R.bin_rows(X, cuts, nbins, missing=True)
        assert np.array_equal(got, ref), (n, np.argwhere(got != ref)[:5])
        assert not got[:, d:].any()
        nan = np.isnan(X)
        assert np.all(got[:, :d][nan] == 255) and np.all(got[:, :d][~nan] < nbins[None, :].repeat(n, 0)[~nan])
        if n == 8191:
            bits = X.view(np.uint32)
            assert (nan & (bits >> 31 == 1)).any() and (nan & (bits >> 31 == 0)).any()
            # the flag off: the rows bin as they always did
            assert np.array_equal(gb.bin_rows(Xd, cuts, nbins).cpu().numpy(), R.bin_rows(X, cuts, nbins))
    assert seen == ({1, 2, 255} if d >= 3 else {255})


# ---- quantile_select with per-feature counts ---------------------------------------------------------
@pytest.mark.parametrize("max_bin", [37, 255])
@pytest.mark.parametrize("shape", [(5000, 3), (70000, 17)])
def test_quantile_select_counts(dev, shape, max_bin):
    n, d = shape
    rng = np.random.default_rng(n + max_bin)
    X = rng.normal(size=(n, d)).astype(np.float32)
    X[:, 0] = np.round(X[:, 0] * 4) / 4 + 0.0     # few distinct values: duplicate picks (no -0.0: the select returns +0.0)
    for f in range(d):
        frac = (0.0, 0.3, 1.0)[f % 3]
        m = rng.random(n) < frac if frac < 1.0 else np.ones(n, bool)
        X[m, f] = np.where(rng.random(int(m.sum())) < 0.5, np.float32(np.nan), NEG_NAN)
    Xd = torch.from_numpy(X).to(dev)
    cuts, nbins = gb.quantile_cuts(Xd, max_bin, missing=True)
    rc, rn = R.quantile_cuts(X, max_bin, missing=True)
    assert np.array_equal(nbins, rn) and cuts.tobytes() == rc.tobytes()
    assert nbins[2] == 1 and nbins.max() <= 255 and nbins[1] > 2
    # a strided sample, and the counts argument left out: the old select
    sc, sn = gb.quantile_cuts(Xd, max_bin, sample_rows=n // 3, missing=True)
    stride = max(1, n // (n // 3))
    rc, rn = R.quantile_cuts(X[::stride][:n // 3], max_bin, missing=True)
    assert np.array_equal(sn, rn) and sc.tobytes() == rc.tobytes()
    oc, on = gb.quantile_cuts(Xd, max_bin)
    rc, rn = R.quantile_cuts(X, max_bin)
    assert np.array_equal(on, rn) and oc.tobytes() == rc.tobytes()


# ---- gbdt_split<MISS> ----------------------------------------------------------------------------------
def _hist_missing(rng, d, nbins, Gq, Hq, gmax, p_missing=0.7):
    """S.hist_with_totals with part of every feature's totals moved into slot 255."""
    H = np.zeros((S.MAX_FEAT, 256, 2), np.int64)
    for f in range(d):
        hm = int(rng.integers(0, Hq + 1)) if rng.random() < p_missing else 0
        gm = int(rng.integers(-gmax, gmax + 1)) if hm or rng.random() < 0.2 else 0
        if hm and rng.random() < 0.3:  # a slot that outweighs every bin: present | missing often wins
            gm *= 16
        H[f] = S.hist_with_totals(rng, 1, nbins[f:f + 1], Gq - gm, Hq - hm, gmax)[0]
        H[f, 255] = (gm, hm)
    return H


def _level_hists(rng, level, d, nbins, hmax, gmax):
    """K._level_hists with missing slots: one sibling of a pair written, the other parent - sibling."""
    ni = (2 << level) - 1
    h0, nn = S.heap_first(level), 1 << level
    hist = np.zeros((ni, S.MAX_FEAT, 256, 2), np.int64)
    gcnt = np.zeros(2 * ni + 1, np.int64)
    gcnt[h0:h0 + nn] = rng.integers(0, 1000, nn)
    tot = lambda: (int(rng.integers(-gmax, gmax)), int(rng.integers(1, hmax)))  # noqa: E731
    if level == 0:
        hist[0] = _hist_missing(rng, d, nbins, *tot(), gmax)
        return hist, gcnt
    for k in range(0, nn, 2):
        if k % 4 == 0:
            gcnt[h0 + k + 1] = gcnt[h0 + k]
        a, b = _hist_missing(rng, d, nbins, *tot(), gmax), _hist_missing(rng, d, nbins, *tot(), gmax)
        built = S.built_mask(level, gcnt[h0:h0 + nn])
        hist[h0 + k + (0 if built[k] else 1)] = a
        hist[(h0 + k - 1) >> 1] = a + b
    return hist, gcnt


def _split_oracle(hist, gcnt, level, d, nbins, cuts, lam, mcw, gamma, fmask=None):
    """S.split_level_oracle under missing=True; `words` are the device's split words."""
    h0, nn = S.heap_first(level), 1 << level
    built = S.built_mask(level, gcnt[h0:h0 + nn])
    hist = hist.copy()
    feat, binv = np.full(nn, -1, np.int32), np.full(nn, 255, np.int32)
    dl = np.zeros(nn, np.uint8)
    thr, gain = np.full(nn, np.inf, np.float32), np.zeros(nn)
    sums = {}
    for k in range(nn):
        node = h0 + k
        if not built[k]:
            hist[node, :d] = hist[(node - 1) >> 1, :d] - hist[h0 + (k ^ 1), :d]
        g_, f, b, GLq, HLq, Gq, Hq, dleft = R.best_split(hist[node, :d], np.asarray(nbins), GINV, HINV, lam, mcw,
                                                         None if fmask is None else int(fmask[node]), True)
        if node == 0:
            sums[0] = (Gq, Hq)
        if R.accepts_split(g_, gamma):
            feat[k], binv[k], dl[k], gain[k] = f, b, dleft, g_
            thr[k] = cuts[f, b] if b >= 0 else -np.inf
            sums[2 * node + 1], sums[2 * node + 2] = (GLq, HLq), (Gq - GLq, Hq - HLq)
        else:
            sums[2 * node + 1], sums[2 * node + 2] = (Gq, Hq), (0, 0)
    return hist, feat, gb.encode_bin_words(binv, dl), thr, gain, sums, binv, dl


def _run_split(hist, gcnt, level, d, nbins, cuts, lam, mcw, gamma, dev, fmask=None):
    m = native()
    ni = hist.shape[0]
    h0, nn = S.heap_first(level), 1 << level
    hd, gd = S.to_dev(hist.reshape(-1), dev), S.to_dev(np.asarray(gcnt, np.int64), dev)
    nt, ct = S.to_dev(np.asarray(nbins, np.int32), dev), S.to_dev(np.asarray(cuts[:d], np.float32), dev)
    feat = torch.full((ni,), -7, dtype=torch.int32, device=dev)
    binv = torch.full((ni,), -7, dtype=torch.int32, device=dev)
    thr = torch.full((ni,), -7.0, dtype=torch.float32, device=dev)
    gain = torch.full((ni,), -7.0, dtype=torch.float64, device=dev)
    ng = torch.full((2 * ni + 1,), S.POISON, dtype=torch.int64, device=dev)
    nh = torch.full((2 * ni + 1,), S.POISON, dtype=torch.int64, device=dev)
    fm = S.to_dev(np.asarray(fmask, np.uint32).view(np.int32), dev) if fmask is not None else None
    m.gbdt_split(ptr(hd), ptr(gd), level, d, ptr(nt), ptr(ct), GINV, HINV, float(lam), float(mcw), float(gamma),
                 ptr(feat), ptr(binv), ptr(thr), ptr(gain), ptr(ng), ptr(nh), stream_of(hd),
                 0 if fm is None else ptr(fm), True)
    torch.cuda.synchronize()
    sl = slice(h0, h0 + nn)
    return (hd.cpu().numpy().reshape(hist.shape), feat[sl].cpu().numpy(), binv[sl].cpu().numpy(),
            thr[sl].cpu().numpy(), gain[sl].cpu().numpy(), ng.cpu().numpy(), nh.cpu().numpy())


def _split_both(dev, hist, gcnt, level, d, nbins, cuts, lam, mcw, gamma, fmask=None):
    ref = _split_oracle(hist, gcnt, level, d, nbins, cuts, lam, mcw, gamma, fmask)
    got = _run_split(hist, gcnt, level, d, nbins, cuts, lam, mcw, gamma, dev, fmask)
    S.assert_split_equal(got, ref[:6], level)
    return ref


SPLIT_NBINS = (1, 2, 3, 4, 5, 254, 255)  # 4 | 5: a lane boundary; 255: the last real bin shares lane 63 with the slot


@pytest.mark.parametrize("masked", [False, True], ids=["all_features", "fmask"])
@pytest.mark.parametrize("level", [0, 1, 2, 3, 4, 5, 6])
def test_split_missing_random_histograms(dev, level, masked):
    rng = np.random.default_rng(50 + level)
    kinds = set()
    for d in (5, 7, 30):  # 5: small features only, where the present | missing candidate often wins
        nb = np.array([SPLIT_NBINS[(f + level) % (5 if d == 5 else 7)] for f in range(d)], np.int32)
        cuts = K._cuts(rng, d)
        ni = (2 << level) - 1
        fmask = None
        if masked:
            fmask = rng.integers(1, 1 << d, ni).astype(np.uint32)
            fmask[rng.random(ni) < 0.1] = 0            # no feature allowed: no split
            fmask[rng.random(ni) < 0.2] &= ~np.uint32(1)  # feature 0 masked: it still gives the totals
        for lam, mcw in ((0.0, 0.0), (1.0, 1.0), (10.0, 0.0)):
            hist, gcnt = _level_hists(rng, level, d, nb, 1 << 30, 1 << 24)
            ref = _split_both(dev, hist, gcnt, level, d, nb, cuts, lam, mcw, 0.0, fmask)
            if level:  # the derived nodes' slot 255 came out of the subtraction
                h0, nn = S.heap_first(level), 1 << level
                derived = ~S.built_mask(level, gcnt[h0:h0 + nn])
                assert derived.sum() == nn // 2 and np.any(ref[0][h0:h0 + nn][derived][:, :d, 255] != 0)
            for f, b, dl in zip(ref[1], ref[6], ref[7]):
                if f >= 0:
                    kinds.add("present|missing" if b < 0 else ("left" if dl else "right"))
    if level >= 3:
        assert kinds == {"present|missing", "left", "right"}, kinds


def test_split_missing_tie_levels(dev):
    """Feature, then bin with -1 lowest, then default_left 0: each decides one crafted node."""
    rng = np.random.default_rng(6)
    gc = np.zeros(3, np.int64)
    for d in (17, 30):  # equal features (a wave's second feature ties with its first): the lowest
        nb = np.full(d, 64, np.int32)
        hist = np.zeros((1, S.MAX_FEAT, 256, 2), np.int64)
        hist[0, :d] = _hist_missing(rng, 1, nb[:1], 12345, 1 << 22, 1 << 18, p_missing=1.0)[0]
        ref = _split_both(dev, hist, gc, 0, d, nb, K._cuts(rng, d), 1.0, 1.0, 0.0)
        assert ref[1][0] == 0
    for d in (1, 2, 18):
        nb = np.full(d, 9, np.int32)
        cuts = K._cuts(rng, d)
        # bins 0 .. 3 empty, all present mass in bin 4, mirrored mass in the slot: b = -1 and
        # (b = 0 .. 3, default left) have the same left side -- the lowest b, -1, wins
        hist = np.zeros((1, S.MAX_FEAT, 256, 2), np.int64)
        hist[0, :d, 4], hist[0, :d, 255] = (4 << 14, 2 << 16), (-(4 << 14), 2 << 16)
        if d > 1:  # the earlier features gain nothing: everything in one bin
            hist[0, :d - 1, 4], hist[0, :d - 1, 255] = (0, 4 << 16), (0, 0)
        ref = _split_both(dev, hist, gc, 0, d, nb, cuts, 1.0, 1.0, 0.0)
        assert (ref[1][0], ref[6][0], ref[7][0]) == (d - 1, -1, 1) and np.isneginf(ref[3][0]) and ref[4][0] > 1e-6
        # no missing rows: both directions of a bin gain the same -- default_left 0; equal gains in
        # bins 0 .. 7 -- the lowest
        hist = np.zeros((1, S.MAX_FEAT, 256, 2), np.int64)
        hist[0, :d, 0], hist[0, :d, 8] = (4 << 14, 2 << 16), (-(4 << 14), 2 << 16)
        if d > 1:
            hist[0, :d - 1, 0], hist[0, :d - 1, 8] = (0, 4 << 16), (0, 0)
        ref = _split_both(dev, hist, gc, 0, d, nb, cuts, 1.0, 1.0, 0.0)
        assert (ref[1][0], ref[6][0], ref[7][0]) == (d - 1, 0, 0) and ref[2][0] == 0
        # the slot's rows belong on the left of bin 2: (2, default left) beats (2, missing right)
        hist = np.zeros((1, S.MAX_FEAT, 256, 2), np.int64)
        hist[0, :d, 1], hist[0, :d, 5], hist[0, :d, 255] = (3 << 14, 1 << 16), (-(6 << 14), 2 << 16), (3 << 14, 1 << 16)
        if d > 1:
            hist[0, :d - 1] = 0
            hist[0, :d - 1, 4] = (0, 4 << 16)
        ref = _split_both(dev, hist, gc, 0, d, nb, cuts, 1.0, 1.0, 0.0)
        assert (ref[1][0], ref[6][0], ref[7][0]) == (d - 1, 1, 1) and ref[2][0] == (0x200 | 2)


def test_split_missing_child_weight_and_gamma(dev):
    """min_child_weight on the missing-only side, gamma at the best gain, lambda = 0 with an empty slot."""
    rng = np.random.default_rng(8)
    nb = np.array([3], np.int32)
    cuts = K._cuts(rng, 1)
    gc = np.zeros(3, np.int64)
    hs = int(1 / HINV)
    hist = np.zeros((1, S.MAX_FEAT, 256, 2), np.int64)
    hist[0, 0, 0], hist[0, 0, 2], hist[0, 0, 255] = (1 << 10, 5 * hs), (1 << 9, 5 * hs), (-(1 << 16), hs)
    ref = _split_both(dev, hist, gc, 0, 1, nb, cuts, 1.0, 1.0, 0.0)   # Hm = mcw exactly: allowed
    assert (ref[6][0], ref[7][0]) == (-1, 1)
    hist[0, 0, 255, 1] -= 1
    ref2 = _split_both(dev, hist, gc, 0, 1, nb, cuts, 1.0, 1.0, 0.0)  # one quantum below: b = -1 is out
    assert ref2[6][0] != -1
    g = float(ref2[4][0])
    assert _split_both(dev, hist, gc, 0, 1, nb, cuts, 1.0, 1.0, g)[1][0] == 0
    assert _split_both(dev, hist, gc, 0, 1, nb, cuts, 1.0, 1.0, np.nextafter(g, np.inf))[1][0] == -1
    hist[0, 0, 255] = 0
    for mcw in (0.0, 1.0):
        _split_both(dev, hist, gc, 0, 1, nb, cuts, 0.0, mcw, 0.0)


# ---- partition, margin walk, eval walk ------------------------------------------------------------------
WALK_NBINS = np.array([255, 2, 1, 16, 255, 3, 100, 2, 255], np.int32)


def _missing_state(rng, level, sizes, hole, seed, depth):
    st = S.level_state(level, sizes, d=9, hole=hole, seed=seed, nbins=WALK_NBINS, depth=depth)
    miss = rng.random((st.n_table, 9)) < 0.2
    miss[:, 4] = False  # one feature without missing rows
    st.bins[:, :9][miss] = 255
    return st


def _mixed_tree(rng, ni, nbins, bins=None):
    """Old words, default-left words, b = -1 and pass-through nodes."""
    d = len(nbins)
    feat = rng.integers(0, d, ni).astype(np.int32)
    binv = np.array([rng.integers(0, max(1, int(nbins[f]) - 1)) for f in feat], np.int32)
    if bins is not None:  # split bins from the data: bin == split bin occurs and goes left
        binv = np.array([min(int(bins[rng.integers(0, bins.shape[0]), f]), max(0, int(nbins[f]) - 2)) for f in feat],
                        np.int32)
    dl = (rng.random(ni) < 0.5).astype(np.uint8)
    kind = rng.random(ni)
    binv[kind < 0.2], dl[kind < 0.2] = -1, 1
    feat[kind > 0.85], binv[kind > 0.85], dl[kind > 0.85] = -1, 255, 0
    if ni > 3:
        feat[0], feat[1], binv[1], dl[1] = abs(int(feat[0])), -1, 255, 0
        binv[2], dl[2] = -1, 1
        feat[2] = max(int(feat[2]), 0)
        feat[3], binv[3], dl[3] = 0, 253, 1  # every present byte left, the slot left too: nothing goes right
    return feat, binv, dl


def _partition_oracle(st, feat, binv, dl):
    """S.partition_level with the direction rule."""
    h0, nn = S.heap_first(st.level), 1 << st.level
    ridx_out, nid_out = np.empty_like(st.ridx), np.empty_like(st.nid)
    flag = np.zeros(st.n_fit, np.uint8)
    seg, gcnt = st.seg.copy(), st.gcnt.copy()
    node_r = np.zeros(st.nheap, np.int64)
    for k in range(nn):
        node = h0 + k
        s, c = (int(v) for v in st.seg[node])
        rows = st.ridx[s:s + c]
        f = int(feat[node])
        right = R.bins_go_right(st.bins[rows, max(f, 0)], int(binv[node]), int(dl[node])) if f >= 0 else np.zeros(c, bool)
        flag[s:s + c] = right
        nl, nr = int((~right).sum()), int(right.sum())
        ridx_out[s:s + nl], ridx_out[s + nl:s + c] = rows[~right], rows[right]
        nid_out[s:s + nl], nid_out[s + nl:s + c] = 2 * node + 1, 2 * node + 2
        seg[2 * node + 1], seg[2 * node + 2] = (s, nl), (s + nl, nr)
        gcnt[2 * node + 1], gcnt[2 * node + 2] = nl, nr
        node_r[node] = nr
    return ridx_out, nid_out, flag, seg, node_r, gcnt


@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 20001])
@pytest.mark.parametrize("level", [0, 2, 5])
def test_partition_direction_words(dev, level, n):
    rng = np.random.default_rng(2000 * level + n)
    holes = [None] + ([(n // 2, 333), (0, 5), (n, 9)] if level == 0 else [])
    for hole in holes:
        st = _missing_state(rng, level, K._part_sizes(rng, level, n, "mixed"), hole, n, level + 1)
        feat, binv, dl = _mixed_tree(rng, (2 << level) - 1, WALK_NBINS)
        if level == 0:
            feat[0], binv[0], dl[0] = 0, (-1, 100, 7, 200)[len(holes) - 1 if hole is None else holes.index(hole) - 1], 1
        ref = _partition_oracle(st, feat, binv, dl)
        got = S.run_partition(st, feat, gb.encode_bin_words(binv, dl), dev)
        for name, g, r in zip(K.PART_NAMES, got, ref):
            assert np.array_equal(g, r), (name, hole)
        if n > 1000:
            old = S.partition_level(st, feat, binv)  # the walk ignoring the direction differs
            assert not np.array_equal(old[2], ref[2])


@pytest.mark.parametrize("nkey", list(K.MARGIN_ROWS))
@pytest.mark.parametrize("depth", [1, 5, 7])
def test_margin_and_eval_walk_direction_words(dev, depth, nkey):
    m = native()
    n_fit = K.MARGIN_ROWS[nkey](K._blocks())
    rng = np.random.default_rng(depth * 20000 + n_fit)
    spw = 3.0
    gs, hs = R.grad_scales(spw)
    d, ni, nl = 9, (1 << depth) - 1, 1 << depth
    for hole in ((0, 0), (n_fit // 2, 300)):
        st = _missing_state(rng, 0, [n_fit], hole, n_fit + depth, 1)
        N = st.n_table
        feat, binv, dl = _mixed_tree(rng, ni, WALK_NBINS, st.bins)
        leaf = rng.normal(scale=0.3, size=nl).astype(np.float32)
        words = gb.encode_bin_words(binv, dl)
        m0 = rng.normal(scale=2.0, size=N).astype(np.float32)
        y = (rng.random(N) < 0.3).astype(np.uint8)
        walk = R.predict_margin_bins(st.bins, feat[None], binv[None], leaf[None], depth, 0.0, dl[None])
        exp = (m0 + walk).astype(np.float32)
        if N > 1000 and depth > 1:
            blind = R.predict_margin_bins(st.bins, feat[None], binv[None], leaf[None], depth, 0.0)
            assert not np.array_equal(blind, walk)
        bt, ldt = S.transpose_bins(st.bins, d)
        binsT = S.to_dev(bt, dev)
        fd, wd, ld, yd = S.to_dev(feat, dev), S.to_dev(words, dev), S.to_dev(leaf, dev), S.to_dev(y, dev)
        margin = S.to_dev(m0, dev)
        gh = torch.full((N, 2), -1, dtype=torch.int16, device=dev)
        m.gbdt_margin(ptr(binsT), ldt, N, ptr(fd), ptr(wd), ptr(ld), depth, ptr(margin), ptr(yd), spw, gs, hs, ptr(gh),
                      stream_of(binsT))
        assert np.array_equal(margin.cpu().numpy().view(np.uint32), exp.view(np.uint32)), hole
        gh_g = torch.empty((N, 2), dtype=torch.int16, device=dev)  # the gradients of the new margin
        m.gbdt_grad(ptr(margin), ptr(yd), N, spw, gs, hs, ptr(gh_g), stream_of(binsT))
        assert torch.equal(gh, gh_g)
        # the sampled and weighted walks share goes_right
        w = rng.random(N).astype(np.float32)
        for name, extra in (("gbdt_margin_weighted", (S.to_dev(w, dev),)), ("gbdt_margin_sampled", None)):
            mg = S.to_dev(m0, dev)
            gh2 = torch.empty((N, 2), dtype=torch.int16, device=dev)
            if extra is not None:
                m.gbdt_margin_weighted(ptr(binsT), ldt, N, ptr(fd), ptr(wd), ptr(ld), depth, ptr(mg), ptr(yd),
                                       ptr(extra[0]), spw, gs, hs, ptr(gh2), stream_of(binsT))
            else:
                m.gbdt_margin_sampled(ptr(binsT), ldt, N, ptr(fd), ptr(wd), ptr(ld), depth, ptr(mg), ptr(yd), spw, gs,
                                      hs, ptr(gh2), 5, 1, 0, R.sample_threshold(0.5), stream_of(binsT))
            assert torch.equal(mg, margin), (name, hole)
        # the eval walk: margins and the exact record
        for wts in (None, w):
            me = S.to_dev(m0, dev)
            rec = torch.zeros(4, dtype=torch.int64, device=dev)
            if wts is None:
                m.gbdt_eval_walk(ptr(binsT), ldt, N, ptr(fd), ptr(wd), ptr(ld), depth, ptr(me), ptr(yd), ptr(rec),
                                 stream_of(binsT))
                want = R.eval_record(exp, y)
            else:
                ws = R.eval_weight_scale(float(w.max()))
                wt = S.to_dev(w, dev)
                m.gbdt_eval_walk_weighted(ptr(binsT), ldt, N, ptr(fd), ptr(wd), ptr(ld), depth, ptr(me), ptr(yd),
                                          ptr(wt), ws, ptr(rec), stream_of(binsT))
                want = R.eval_record_weighted(exp, y, w, ws)
            assert torch.equal(me, margin), hole
            got = rec.cpu().numpy()
            assert np.array_equal(got[1:], want[1:]) and abs(int(got[0]) - int(want[0])) <= N, (got, want)  # loss: libm


# ---- gbdt_predict with default_left ----------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257])
@pytest.mark.parametrize("depth", [1, 4, 7])
def test_predict_kernel_default_left(dev, depth, n):
    rng = np.random.default_rng(depth * 3000 + n)
    d = 7
    ni, nl = (1 << depth) - 1, 1 << depth
    c = 12288 // (2 * ni + nl)  # the LDS chunk: the footprint of a tree is unchanged
    T = c + 1
    X = rng.normal(size=(n, d)).astype(np.float32)
    X[:, 1] = np.round(X[:, 1] * 2) / 2
    special = np.array([np.nan, NEG_NAN, np.inf, -np.inf, -0.0, 0.0], np.float32)
    mask = rng.random((n, d)) < 0.3
    X[mask] = special[rng.integers(0, len(special), int(mask.sum()))]
    feat = rng.integers(-1, d, (T, ni)).astype(np.int32)
    thr = X[rng.integers(0, n, (T, ni)), np.maximum(feat, 0)].astype(np.float32)
    thr[np.isnan(thr)] = 0.25
    thr[rng.random((T, ni)) < 0.1] = 0.0
    dl = ((rng.random((T, ni)) < 0.5) & (feat >= 0)).astype(np.uint8)
    only_missing = (rng.random((T, ni)) < 0.2) & (feat >= 0)
    thr[only_missing], dl[only_missing] = -np.inf, 1
    thr[feat < 0] = np.inf
    if ni > 1:
        feat[:, 0], thr[:, 0], dl[:, 0] = 0, -np.inf, 1
    leaf = rng.normal(scale=0.05, size=(T, nl)).astype(np.float32)
    ens = gb.TreeEnsemble(depth=depth, feat=feat, bin=np.zeros_like(feat), thr=thr, gain=np.zeros((T, ni)), leaf=leaf,
                          cuts=np.full((d, 256), np.inf, np.float32), nbins=np.ones(d, np.int32), base_score=0.3,
                          default_left=dl)
    buf = torch.zeros((n, 37), dtype=torch.float32, device=dev)
    buf[:, 3:3 + d] = torch.from_numpy(X).to(dev)
    Xs, Xc = buf[:, 3:3 + d], torch.from_numpy(X).to(dev)
    dens = gb.DeviceEnsemble(ens, dev)
    assert dens.dleft is not None
    differs = False
    for k in (0, 1, c - 1, c, c + 1):
        ref = R.predict_margin(X, feat[:k], thr[:k], leaf[:k], depth, ens.base_margin, dl[:k])
        differs |= not np.array_equal(ref, R.predict_margin(X, feat[:k], thr[:k], leaf[:k], depth, ens.base_margin))
        for Xd in (Xc, Xs):
            got = gb.predict_margin(Xd, ens, dens, n_trees=k).cpu().numpy()
            assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (k, Xd.stride())
    assert differs or n == 1
    # an all-zero default_left is the null pointer: the walk the kernel always did
    ens0 = gb.TreeEnsemble(**{**ens.__dict__, "default_left": np.zeros_like(dl)})
    assert gb.DeviceEnsemble(ens0, dev).dleft is None
    ref = R.predict_margin(X, feat, thr, leaf, depth, ens.base_margin)
    assert np.array_equal(gb.predict_margin(Xc, ens0).cpu().numpy().view(np.uint32), ref.view(np.uint32))


# ---- whole fits: the device against the CPU path -----------------------------------------------------------
def _fit_data(n, d, frac, seed):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, d)).astype(np.float32)
    if d > 1:
        X[:, 1] = np.round(X[:, 1] * 3) / 3 + 0.0  # no -0.0: the device's select returns +0.0 for it
    sig = np.zeros(n, bool)
    if frac:
        for f in range(0, d, 2):
            mk = rng.random(n) < frac
            X[mk, f] = np.where(rng.random(int(mk.sum())) < 0.5, np.float32(np.nan), NEG_NAN)
        sig = np.isnan(X[:, 0])
    logit = 1.2 * np.nan_to_num(X[:, 0]) - 1.5 * (np.nan_to_num(X[:, min(1, d - 1)]) > 0.3) - 1.0 - 3.0 * sig
    y = (rng.random(n) < 1 / (1 + np.exp(-logit))).astype(np.uint8)
    if d >= 6:
        X[:, d - 1] = np.nan  # one all-NaN column
    if n <= 50:
        y[0], y[1] = 0, 1
    return X, y


def _assert_same_fit(a, b):
    for k in ("feat", "bin", "thr", "gain", "leaf"):
        x, y = getattr(a, k), getattr(b, k)
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), k
    assert np.array_equal(a.default_left, b.default_left)


@pytest.mark.parametrize("max_bin", [2, 37, 256])
@pytest.mark.parametrize("depth", [1, 5, 7])
@pytest.mark.parametrize("d", [1, 6, 30])
@pytest.mark.parametrize("n", [3, 50, 4000])
def test_fit_device_equals_cpu(dev, n, d, depth, max_bin):
    for frac in (0.0, 0.1):
        X, y = _fit_data(n, d, frac, n + d + depth)
        p = gb.GBDTParams(n_estimators=2, max_depth=depth, max_bin=max_bin, scale_pos_weight=3.0, min_child_weight=0.0,
                          missing_policy="learn")
        ref, rm = gb.fit(torch.from_numpy(X), torch.from_numpy(y), p, return_margin=True)
        ens, m = gb.fit(torch.from_numpy(X).to(dev), torch.from_numpy(y).to(dev), p, return_margin=True)
        assert np.array_equal(ens.cuts, ref.cuts) and np.array_equal(ens.nbins, ref.nbins) and ens.nbins.max() <= 255
        _assert_same_fit(ens, ref)
        assert np.array_equal(m.cpu().numpy().view(np.uint32), rm.numpy().view(np.uint32))
        got = gb.predict_margin(torch.from_numpy(X).to(dev), ens)
        assert torch.equal(got, m)
        if frac and n == 4000 and depth > 1 and max_bin > 2:
            assert ens.has_default_left
        if not frac and d < 6:
            assert not ens.has_default_left


def _big(dev):
    X, y = _fit_data(6000, 6, 0.1, 77)
    return X, y, torch.from_numpy(X).to(dev), torch.from_numpy(y).to(dev)


KW = dict(n_estimators=6, max_depth=5, max_bin=37, min_child_weight=0.0, missing_policy="learn")


@pytest.mark.parametrize("what", ["sampling", "weights", "eval_float_rows", "eval_hole_early_stop", "graph", "fuse_env",
                                  "resume"])
def test_fit_composes_on_device(dev, monkeypatch, tmp_path, what):
    X, y, Xd, yd = _big(dev)
    Xt, yt = torch.from_numpy(X), torch.from_numpy(y)
    n = len(X)
    if what == "sampling":
        p = gb.GBDTParams(**KW, subsample=0.6, colsample_bynode=0.6, seed=5)
        ref, rm = gb.fit(Xt, yt, p, return_margin=True)
        ens, m = gb.fit(Xd, yd, p, return_margin=True)
    elif what == "weights":
        w = np.where(y != 0, 2.5, 0.75).astype(np.float32)
        w[::7] = 0.0
        p = gb.GBDTParams(**KW)
        ref, rm = gb.fit(Xt, yt, p, return_margin=True, sample_weight=torch.from_numpy(w))
        ens, m = gb.fit(Xd, yd, p, return_margin=True, sample_weight=torch.from_numpy(w).to(dev))
    elif what == "eval_float_rows":
        p = gb.GBDTParams(**KW)
        Xv, yv = Xt[:1500].clone(), yt[:1500].clone()
        assert torch.isnan(Xv).any()
        ref, rm, rrec = gb.fit(Xt, yt, p, return_margin=True, eval_set=(Xv, yv), eval_metric=("error", "logloss"))
        ens, m, rec = gb.fit(Xd, yd, p, return_margin=True, eval_set=(Xv.to(dev), yv.to(dev)),
                             eval_metric=("error", "logloss"))
        assert np.array_equal(rec.records[:, 1:], rrec.records[:, 1:])
        assert np.all(np.abs(rec.records[:, 0] - rrec.records[:, 0]) <= 1500)  # libm in the loss
    elif what == "eval_hole_early_stop":
        p = gb.GBDTParams(**{**KW, "n_estimators": 40, "learning_rate": 0.9})
        cuts = gb.quantile_cuts(Xt, 37, missing=True)
        kw = dict(hole=(1000, 1200), eval_set="hole", eval_metric="error", early_stopping_rounds=2, return_margin=True)
        ref, rm, rrec = gb.fit_binned(gb.bin_rows(Xt, *cuts, missing=True), yt, cuts, p, **kw)
        ens, m, rec = gb.fit_binned(gb.bin_rows(Xd, *cuts, missing=True), yd, cuts, p, **kw)
        assert rec.stopped and rec.best_iteration == rrec.best_iteration and ens.n_trees < 40
        assert np.array_equal(rec.records[:, 1:], rrec.records[:, 1:])
    elif what == "graph":
        p = gb.GBDTParams(**KW)
        ref, rm = gb.fit(Xt, yt, p, return_margin=True)
        ens, m = gb.fit(Xd, yd, p, return_margin=True, use_graph=True)
    elif what == "fuse_env":
        p = gb.GBDTParams(**KW)
        ref, rm = gb.fit(Xt, yt, p, return_margin=True)
        monkeypatch.setenv("FDX_GBDT_FUSE_MARGIN", "1")  # falls back: the fused pass knows no directions
        ens, m = gb.fit(Xd, yd, p, return_margin=True)
    else:
        from fraud_detection_amd.utils.checkpoint import CheckpointManager

        p = gb.GBDTParams(**KW)
        cuts = gb.quantile_cuts(Xt, 37, missing=True)
        ref, rm = gb.fit(Xt, yt, p, cuts=cuts, return_margin=True)
        mgr = CheckpointManager(str(tmp_path), prefix="g")
        gb.fit(Xd, yd, gb.GBDTParams(**{**KW, "n_estimators": 4}), cuts=cuts, checkpoint=mgr, checkpoint_every=2)
        ens, m = gb.fit(Xd, yd, p, cuts=cuts, checkpoint=mgr, checkpoint_every=2, return_margin=True)
        cpu = gb.fit(Xt, yt, p, cuts=cuts, checkpoint=mgr, checkpoint_every=2)  # a device checkpoint resumes on the CPU
        _assert_same_fit(cpu, ref)
    assert ens.has_default_left
    _assert_same_fit(ens, ref)
    assert np.array_equal(m.cpu().numpy().view(np.uint32), rm.numpy().view(np.uint32))
    assert torch.equal(gb.predict_margin(Xd, ens), m)
    assert n == m.shape[0]


# ---- the old path is what it was ---------------------------------------------------------------------------
def test_last_bin_fits_unchanged(dev):
    """"last_bin" fits on the non-finite data of the parameter sweep: to_dict() as recorded (on the
    CPU path) before missing_policy existed -- on the CPU path and on the device."""
    with open(GOLDEN) as f:
        golden = json.load(f)
    X, y, depth, spw, max_bins = K._sweep_data("nonfinite")
    assert len(golden) == len(K.REG) * len(max_bins)
    Xd, yd = torch.from_numpy(X).to(dev), torch.from_numpy(y).to(dev)
    for g in golden:
        lam, mcw, gamma = (float(v) for v in g["reg"])
        p = gb.GBDTParams(n_estimators=1, max_depth=depth, scale_pos_weight=spw, reg_lambda=lam, min_child_weight=mcw,
                          gamma=gamma, max_bin=g["max_bin"])
        cuts = R.quantile_cuts(X, g["max_bin"])
        for Xa, ya in ((torch.from_numpy(X), torch.from_numpy(y)), (Xd, yd)):
            got = json.loads(json.dumps(gb.fit(Xa, ya, p, cuts=cuts).to_dict()))
            assert got == g["model"], (g["reg"], g["max_bin"], Xa.device)
