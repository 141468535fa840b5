"""GBDT monotone constraints on the device: gbdt_split_kernel<MISS, MONO> and gbdt_leaf with bounds
against the numpy oracle (every output exact, gains and bounds bitwise), then whole fits -- device
trees equal to the oracle's bit for bit and exactly monotone margins -- alone and composed with
learned missing directions, sampling, weights, early stopping, the CV job and the pipeline.  The
two-rank fit runs on the CPU path (test_gbdt_monotone.test_dp_equals_single_process): the device
GBDT tests have no two-rank pattern, and the constrained scan sees only all-reduced histograms."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import _gbdt_state as S
import test_gbdt_kernels_gpu as K
import test_gbdt_missing_gpu as M
import test_gbdt_monotone as C
from fraud_detection_amd.ops import gbdt as gb
from fraud_detection_amd.ops import reference_gbdt as R
from fraud_detection_amd.ops.native import native, ptr, stream_of

pytestmark = pytest.mark.gpu

GINV, HINV = K.GINV, K.HINV
SENT = 7.25  # what a bounds entry holds before a block stores into it
INF = np.inf


def masks_of(cons):
    return (sum(1 << f for f, c in enumerate(cons) if c > 0), sum(1 << f for f, c in enumerate(cons) if c < 0))


# ---- gbdt_split<MISS, MONO> -------------------------------------------------------------------------
def split_oracle(hist, gcnt, level, d, nbins, cuts, lam, mcw, gamma, cons, lo, hi, fmask=None, missing=False):
    """The level's decisions under the nodes' bounds lo / hi [2^level]: derived nodes first become
    parent - sibling, then best_split(mono=...) + the split rule + mono_children.  Returns (hist
    after, feat, device bin words, thr, gain, {heap id: (ng, nh)}, {heap id: (lo, hi)})."""
    h0, nn = S.heap_first(level), 1 << level
    built = S.built_mask(level, gcnt[h0:h0 + nn])
    hist = hist.copy()
    feat, binv, dl = np.full(nn, -1, np.int32), np.full(nn, 255, np.int32), np.zeros(nn, np.uint8)
    thr, gain = np.full(nn, np.inf, np.float32), np.zeros(nn)
    sums, bounds = {}, {}
    for k in range(nn):
        node = h0 + k
        if not built[k]:
            hist[node, :d] = hist[(node - 1) >> 1, :d] - hist[h0 + (k ^ 1), :d]
        mono = None if cons is None else (np.asarray(cons), lo[k], hi[k])
        out = R.best_split(hist[node, :d], np.asarray(nbins), GINV, HINV, lam, mcw,
                           None if fmask is None else int(fmask[node]), missing, mono)
        g_, f, b, GLq, HLq, Gq, Hq = out[:7]
        if node == 0:
            sums[0] = (Gq, Hq)
            if cons is not None:
                bounds[0] = (-INF, INF)
        split = R.accepts_split(g_, gamma)
        if split:
            feat[k], binv[k], gain[k] = f, b, g_
            dl[k] = out[7] if missing else 0
            thr[k] = cuts[f, b] if b >= 0 else -np.inf
            sums[2 * node + 1], sums[2 * node + 2] = (GLq, HLq), (Gq - GLq, Hq - HLq)
        else:
            sums[2 * node + 1], sums[2 * node + 2] = (Gq, Hq), (0, 0)
        if cons is not None:
            ll, lh, rl, rh = R.mono_children(int(cons[f]) if split else 0, lo[k], hi[k], GLq, HLq, Gq, Hq, GINV, HINV,
                                             lam, mcw)
            bounds[2 * node + 1], bounds[2 * node + 2] = (ll, lh), (rl, rh)
    words = gb.encode_bin_words(binv, dl) if missing else binv
    return hist, feat, words, thr, gain, sums, bounds


def run_split(dev, hist, gcnt, level, d, nbins, cuts, lam, mcw, gamma, cons, lo, hi, fmask=None, missing=False):
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
    b_lo, b_hi = np.full(2 * ni + 1, SENT), np.full(2 * ni + 1, SENT)
    if level:  # a level-0 block must not read its bounds: they stay the sentinel
        b_lo[h0:h0 + nn], b_hi[h0:h0 + nn] = lo, hi
    blo, bhi = S.to_dev(b_lo, dev), S.to_dev(b_hi, dev)
    fm = S.to_dev(np.asarray(fmask, np.uint32).view(np.int32), dev) if fmask is not None else None
    inc, dec = masks_of(cons) if cons is not None else (0, 0)
    m.gbdt_split(ptr(hd), ptr(gd), level, d, ptr(nt), ptr(ct), GINV, HINV, float(lam), float(mcw), float(gamma),
                 ptr(feat), ptr(binv), ptr(thr), ptr(gain), ptr(ng), ptr(nh), stream_of(hd),
                 0 if fm is None else ptr(fm), missing, inc, dec, ptr(blo), ptr(bhi))
    torch.cuda.synchronize()
    sl = slice(h0, h0 + nn)
    return ((hd.cpu().numpy().reshape(hist.shape), feat[sl].cpu().numpy(), binv[sl].cpu().numpy(),
             thr[sl].cpu().numpy(), gain[sl].cpu().numpy(), ng.cpu().numpy(), nh.cpu().numpy()),
            blo.cpu().numpy(), bhi.cpu().numpy(), b_lo, b_hi)


def split_both(dev, hist, gcnt, level, d, nbins, cuts, lam, mcw, gamma, cons, lo, hi, fmask=None, missing=False):
    """Every output of the kernel against the oracle, exactly; the bounds bitwise, and no bounds
    entry written but node 0's (level 0) and the children's."""
    ref = split_oracle(hist, gcnt, level, d, nbins, cuts, lam, mcw, gamma, cons, lo, hi, fmask, missing)
    got, blo, bhi, lo0, hi0 = run_split(dev, hist, gcnt, level, d, nbins, cuts, lam, mcw, gamma, cons, lo, hi, fmask,
                                        missing)
    S.assert_split_equal(got, ref[:6], level)
    want_lo, want_hi = lo0.copy(), hi0.copy()
    for node, (a, b) in ref[6].items():
        want_lo[node], want_hi[node] = a, b
    assert blo.tobytes() == want_lo.tobytes(), (blo, want_lo)
    assert bhi.tobytes() == want_hi.tobytes(), (bhi, want_hi)
    return ref


def node_weight(hist, level, k, gcnt, d, lam):
    """The unconstrained weight -G / (H + lam) of node k of the level (derived nodes subtracted)."""
    h0, nn = S.heap_first(level), 1 << level
    node = h0 + k
    H = hist[node, 0]
    if not S.built_mask(level, gcnt[h0:h0 + nn])[k]:
        H = hist[(node - 1) >> 1, 0] - hist[h0 + (k ^ 1), 0]
    G, Hs = float(H[:, 0].sum()) * GINV, float(H[:, 1].sum()) * HINV
    return -G / (Hs + lam) if Hs + lam > 0 else 0.0


BOUND_STATES = ("inf", "lo_above", "hi_below", "tight", "around")


def bounds_for(state, w0):
    """A node's [lo, hi] by state, relative to its unconstrained weight w0: lo_above / hi_below
    exclude w0 (the node's own weight clamps), tight leaves one value, around is two-sided."""
    s = max(abs(w0), 1e-3)
    return {"inf": (-INF, INF), "lo_above": (w0 + 0.3 * s, INF), "hi_below": (-INF, w0 - 0.3 * s),
            "tight": (w0 + 0.1 * s, w0 + 0.1 * s), "around": (w0 - 0.4 * s, w0 + 0.4 * s)}[state]


def cons_for(kind, d, rng):
    return {"plus": np.ones(d, np.int64), "minus": -np.ones(d, np.int64),
            "mixed": rng.integers(-1, 2, d), "empty": None}[kind]


SPLIT_NBINS = (2, 3, 255, 256)


@pytest.mark.parametrize("kind", ["plus", "minus", "mixed", "empty"])
@pytest.mark.parametrize("d", [1, 5, 30])
@pytest.mark.parametrize("level", [0, 1, 2])
def test_split_random_histograms(dev, level, d, kind):
    """Built and derived nodes, every bounds state on some node, fmask rows, min_child_weight 0 / 1,
    reg_lambda 0 (empty sides: hist_with_totals leaves empty bins at 255 / 256 bins)."""
    rng = np.random.default_rng(100 * level + d)
    nn = 1 << level
    nb = np.array([SPLIT_NBINS[(f + level) % 4] for f in range(d)], np.int32)
    cuts = K._cuts(rng, d)
    seen, n_split, n_clamped = set(), 0, 0
    for rep, (lam, mcw) in enumerate(((0.0, 0.0), (1.0, 1.0), (10.0, 0.0), (1.0, 0.0))):
        cons = cons_for(kind, d, rng)
        if cons is not None and not cons.any():
            cons[0] = 1
        hist, gcnt = K._level_hists(rng, level, d, nb, 1 << 30, 1 << 24)
        states = [BOUND_STATES[(k + rep) % 5] if level else "inf" for k in range(nn)]
        bl = [bounds_for(s, node_weight(hist, level, k, gcnt, d, lam)) for k, s in enumerate(states)]
        lo, hi = np.array([b[0] for b in bl]), np.array([b[1] for b in bl])
        fmask = None
        if rep == 3:
            fmask = rng.integers(1, 1 << d, hist.shape[0]).astype(np.uint32)
            fmask[rng.random(hist.shape[0]) < 0.2] &= ~np.uint32(1)  # feature 0 masked: it still gives the totals
        ref = split_both(dev, hist, gcnt, level, d, nb, cuts, lam, mcw, 0.0, cons, lo, hi, fmask)
        if cons is None:
            assert ref[6] == {}
            continue
        free = split_oracle(hist, gcnt, level, d, nb, cuts, lam, mcw, 0.0, None, lo, hi, fmask)
        n_clamped += int(np.any(free[1] != ref[1]) or np.any(free[2] != ref[2]))
        n_split += int((ref[1] >= 0).sum())
        for k, s in enumerate(states):
            seen.add(s)
            if s == "tight":  # every weight is the one value: no candidate can gain
                assert ref[1][k] == -1
                assert ref[6][2 * (S.heap_first(level) + k) + 1] == (lo[k], hi[k])
    if kind != "empty":
        assert n_split > 0
        assert level == 0 or (seen == set(BOUND_STATES) if level == 2 else len(seen) >= 2)


@pytest.mark.parametrize("level", [0, 1, 2])
def test_split_missing_instantiation(dev, level):
    """gbdt_split_kernel<true, true>: mass in slot 255, the constraint tested on the candidate's own
    sides whichever one the missing rows join."""
    rng = np.random.default_rng(40 + level)
    nn = 1 << level
    kinds = set()
    for d in (5, 30):
        nb = np.array([M.SPLIT_NBINS[(f + level) % 7] for f in range(d)], np.int32)
        cuts = K._cuts(rng, d)
        for rep, (lam, mcw) in enumerate(((0.0, 0.0), (1.0, 1.0), (10.0, 0.0))):
            cons = cons_for(("plus", "minus", "mixed")[rep], d, rng)
            cons[0] = cons[0] or 1
            hist, gcnt = M._level_hists(rng, level, d, nb, 1 << 30, 1 << 24)
            states = [BOUND_STATES[(k + rep) % 5] if level else "inf" for k in range(nn)]
            bl = [bounds_for(s, node_weight(hist, level, k, gcnt, d, lam)) for k, s in enumerate(states)]
            lo, hi = np.array([b[0] for b in bl]), np.array([b[1] for b in bl])
            fmask = rng.integers(1, 1 << d, hist.shape[0]).astype(np.uint32) if rep == 2 else None
            ref = split_both(dev, hist, gcnt, level, d, nb, cuts, lam, mcw, 0.0, cons, lo, hi, fmask, missing=True)
            b, dl = gb.decode_bin_words(ref[2])
            for f, bb, dd in zip(ref[1], b, dl):
                if f >= 0:
                    kinds.add("present|missing" if bb < 0 else ("left" if dd else "right"))
    assert len(kinds) >= 2, kinds


def test_split_ties_and_sign(dev):
    """Identical feature columns: the lowest feature; equal gains at several bins: the lowest bin; and
    the same histogram under the opposite sign has no candidate at all."""
    rng = np.random.default_rng(6)
    gc = np.zeros(3, np.int64)
    lo, hi = np.array([-INF]), np.array([INF])
    for d in (2, 17, 30):
        nb = np.full(d, 9, np.int32)
        cuts = K._cuts(rng, d)
        hist = np.zeros((1, S.MAX_FEAT, 256, 2), np.int64)
        hist[0, :d, 0], hist[0, :d, 8] = (4 << 14, 2 << 16), (-(4 << 14), 2 << 16)  # wl < 0 < wr, bins 0 .. 7 tie
        up = split_both(dev, hist, gc, 0, d, nb, cuts, 1.0, 1.0, 0.0, np.ones(d, np.int64), lo, hi)
        assert (up[1][0], up[2][0]) == (0, 0) and up[4][0] > 1e-6
        ll, lh = up[6][1]
        assert ll == -INF and lh == up[6][2][0] == 0.0 and up[6][2][1] == INF  # mid of -w and +w
        down = split_both(dev, hist, gc, 0, d, nb, cuts, 1.0, 1.0, 0.0, -np.ones(d, np.int64), lo, hi)
        assert down[1][0] == -1 and down[6][1] == down[6][2] == (-INF, INF)
        # only the last feature may rise: it wins although every other one gains the same
        last = -np.ones(d, np.int64)
        last[d - 1] = 0
        assert split_both(dev, hist, gc, 0, d, nb, cuts, 1.0, 1.0, 0.0, last, lo, hi)[1][0] == d - 1
        # a random feature copied into every column, on a node with two-sided bounds (level 1)
        nb2 = np.full(d, 256, np.int32)
        hist, gcnt = K._level_hists(rng, 1, 1, nb2[:1], 1 << 30, 1 << 24)
        hist[:, 1:d] = hist[:, :1]
        w = [node_weight(hist, 1, k, gcnt, d, 1.0) for k in range(2)]
        bl = [bounds_for("around", w[0]), bounds_for("hi_below", w[1])]
        ref = split_both(dev, hist, gcnt, 1, d, nb2, K._cuts(rng, d), 1.0, 0.0, 0.0, np.ones(d, np.int64),
                         np.array([b[0] for b in bl]), np.array([b[1] for b in bl]))
        assert np.all(ref[1] <= 0)


def test_split_child_weight_gamma_and_empty_side(dev):
    rng = np.random.default_rng(8)
    nb = np.array([3], np.int32)
    cuts = K._cuts(rng, 1)
    gc = np.zeros(3, np.int64)
    hs = int(1 / HINV)
    lo, hi = np.array([-INF]), np.array([INF])
    up = np.ones(1, np.int64)
    hist = np.zeros((1, S.MAX_FEAT, 256, 2), np.int64)
    hist[0, 0, 0], hist[0, 0, 1], hist[0, 0, 2] = (1 << 16, hs), (1 << 9, 5 * hs), (-(1 << 10), 5 * hs)
    ref = split_both(dev, hist, gc, 0, 1, nb, cuts, 1.0, 1.0, 0.0, up, lo, hi)  # HL = mcw exactly: allowed
    assert (ref[1][0], ref[2][0]) == (0, 0)
    hist[0, 0, 0, 1] -= 1
    ref2 = split_both(dev, hist, gc, 0, 1, nb, cuts, 1.0, 1.0, 0.0, up, lo, hi)  # one quantum below: bin 0 is out
    assert (ref2[1][0], ref2[2][0]) == (0, 1)
    g = float(ref2[4][0])
    assert split_both(dev, hist, gc, 0, 1, nb, cuts, 1.0, 1.0, g, up, lo, hi)[1][0] == 0
    assert split_both(dev, hist, gc, 0, 1, nb, cuts, 1.0, 1.0, np.nextafter(g, np.inf), up, lo, hi)[1][0] == -1
    # reg_lambda = 0 with an empty left side (H = 0: weight 0 by the zero rule, term 0), under bounds
    # that clamp the zero up: level 1, lo > 0
    hist = np.zeros((3, S.MAX_FEAT, 256, 2), np.int64)
    hist[1, 0, 1], hist[1, 0, 2] = (-(1 << 14), 3 * hs), (-(3 << 14), 2 * hs)
    hist[0] = hist[1]
    gcnt = np.zeros(7, np.int64)
    gcnt[1], gcnt[2] = 1, 5  # node 1 built, node 2 derived and empty
    for mcw in (0.0, 1.0):
        for cons in (up, -up):
            split_both(dev, hist, gcnt, 1, 1, nb, cuts, 0.0, mcw, 0.0, cons, np.array([0.05, -INF]),
                       np.array([INF, INF]))


# ---- gbdt_leaf with bounds -------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [1, 3, 7])
def test_leaf_kernel_bounds(dev, depth):
    rng = np.random.default_rng(depth)
    m = native()
    nl, ni = 1 << depth, (1 << depth) - 1
    hs = int(1 / HINV)
    ng = rng.integers(-(1 << 24), 1 << 24, 2 * nl - 1)
    nh = rng.integers(0, 1 << 22, 2 * nl - 1)
    lo, hi = np.full(2 * nl - 1, -INF), np.full(2 * nl - 1, INF)
    w = np.array([-(float(g) * GINV) / (float(h) * HINV + 1.0) for g, h in zip(ng, nh)])
    state = rng.integers(0, 4, 2 * nl - 1)
    lo[state == 1] = w[state == 1] + 0.01   # clamped up
    hi[state == 2] = w[state == 2] - 0.01   # clamped at hi
    lo[state == 3], hi[state == 3] = w[state == 3] - 0.5, w[state == 3] + 0.5  # inside: untouched
    nh[ni] = hs - 1                          # H < min_child_weight under lo > 0: the zero is clamped up
    lo[ni], hi[ni] = 0.125, INF
    if nl > 1:
        ng[ni + 1], nh[ni + 1] = -(1 << 20), 4 * hs  # a large positive weight clamped at hi
        lo[ni + 1], hi[ni + 1] = -INF, 0.5
    want = R.leaf_values(ng, nh, depth, GINV, HINV, 1.0, 1.0, 0.3, lo, hi)
    assert want[0] == np.float32(0.3 * 0.125) and (nl == 1 or want[1] == np.float32(0.3 * 0.5))
    leaf = torch.full((nl,), -7.0, dtype=torch.float32, device=dev)
    ngd, nhd, lod, hid = (S.to_dev(a, dev) for a in (ng.astype(np.int64), nh.astype(np.int64), lo, hi))
    m.gbdt_leaf(ptr(ngd), ptr(nhd), depth, GINV, HINV, 1.0, 1.0, 0.3, ptr(leaf), stream_of(leaf), ptr(lod), ptr(hid))
    torch.cuda.synchronize()
    assert leaf.cpu().numpy().tobytes() == want.tobytes()
    plain = R.leaf_values(ng, nh, depth, GINV, HINV, 1.0, 1.0, 0.3)
    assert plain.tobytes() != want.tobytes()
    for tail in ((), (0, 0)):  # null pointers: the leaf kernel as it always was
        m.gbdt_leaf(ptr(ngd), ptr(nhd), depth, GINV, HINV, 1.0, 1.0, 0.3, ptr(leaf), stream_of(leaf), *tail)
        torch.cuda.synchronize()
        assert leaf.cpu().numpy().tobytes() == plain.tobytes()


def test_launcher_refusals(dev):
    m = native()
    z = torch.zeros(4096, dtype=torch.int64, device=dev)
    f = torch.zeros(64, dtype=torch.float64, device=dev)

    def split(d, inc, dec, lo, hi):
        m.gbdt_split(ptr(z), ptr(z), 0, d, ptr(z), ptr(z), 1.0, 1.0, 1.0, 1.0, 0.0, ptr(z), ptr(z), ptr(z), ptr(z), ptr(z),
                     ptr(z), stream_of(z), 0, False, inc, dec, lo, hi)

    for args, msg in (((4, 3, 2, ptr(f), ptr(f)), "overlap"), ((4, 16, 0, ptr(f), ptr(f)), "at or above d"),
                      ((4, 1, 2, 0, 0), "both bounds"), ((4, 1, 0, ptr(f), 0), "both bounds")):
        with pytest.raises(RuntimeError, match=msg):
            split(*args)
    with pytest.raises(RuntimeError, match="both arrays or neither"):
        m.gbdt_leaf(ptr(z), ptr(z), 2, 1.0, 1.0, 1.0, 1.0, 0.1, ptr(f), stream_of(z), ptr(f), 0)


# ---- whole fits ------------------------------------------------------------------------------------
CONS, FIT_KW = C.CONS, C.FIT_KW


def dev_predict(ens, dev):
    return lambda rows: gb.predict_margin(torch.from_numpy(np.ascontiguousarray(rows)).to(dev), ens).cpu().numpy()


def assert_monotone(ens, X, dev, cons=CONS):
    v = C.violations(dev_predict(ens, dev), X, ens.cuts, ens.nbins, cons)
    assert all(n == 0 for n, _ in v.values()), v


@pytest.fixture(scope="module")
def cpu_fits():
    X, y = C.fixture_data()
    Xt, yt = torch.from_numpy(X), torch.from_numpy(y)
    return X, y, gb.fit(Xt, yt, gb.GBDTParams(**FIT_KW)), gb.fit(Xt, yt, gb.GBDTParams(monotone_constraints=CONS, **FIT_KW))


def test_fit_equals_oracle_and_is_monotone(dev, cpu_fits):
    X, y, free_c, mono_c = cpu_fits
    Xd, yd = torch.from_numpy(X).to(dev), torch.from_numpy(y).to(dev)
    mono = gb.fit(Xd, yd, gb.GBDTParams(monotone_constraints=CONS, **FIT_KW))
    assert C.same_trees(mono, mono_c)
    assert mono.params["monotone_constraints"] == list(CONS)
    assert_monotone(mono, X, dev)
    free = gb.fit(Xd, yd, gb.GBDTParams(**FIT_KW))
    assert C.same_trees(free, free_c) and not C.same_trees(free, mono)
    v = C.violations(dev_predict(free, dev), X, free.cuts, free.nbins, CONS)
    assert v[0][0] > 0 and v[1][0] > 0, v
    for form in ((0, 0, 0, 0), "(0,0,0,0)"):  # all zero: the default fit bit for bit
        zero = gb.fit(Xd, yd, gb.GBDTParams(monotone_constraints=form, **FIT_KW))
        assert C.same_trees(zero, free) and zero.to_dict() == free.to_dict()
    graph = gb.fit(Xd, yd, gb.GBDTParams(monotone_constraints=CONS, **FIT_KW), use_graph=True)
    assert C.same_trees(graph, mono)  # the recorded round replays the static bounds pointers


@pytest.mark.parametrize("depth,max_bin,cons", [(1, 2, (-1, 1, 1, -1)), (5, 256, (1, -1, 0, 0)), (7, 37, (-1, -1, 1, 1))])
def test_fit_shapes_equal_oracle(dev, depth, max_bin, cons):
    X, y = C.fixture_data()
    p = gb.GBDTParams(n_estimators=4, max_depth=depth, max_bin=max_bin, learning_rate=0.5, min_child_weight=0.0,
                      monotone_constraints=cons)
    ref = gb.fit(torch.from_numpy(X), torch.from_numpy(y), p)
    got = gb.fit(torch.from_numpy(X).to(dev), torch.from_numpy(y).to(dev), p)
    assert C.same_trees(got, ref)
    assert_monotone(got, X, dev, cons)


def nan_data():
    X, y = C.fixture_data()
    rng = np.random.default_rng(11)
    Xn = X.copy()
    Xn[rng.random(600) < 0.1, 0] = np.nan
    Xn[rng.random(600) < 0.1, 2] = np.nan
    return X, Xn, y, rng.uniform(0.25, 2.0, 600).astype(np.float32)


@pytest.mark.parametrize("what", ["learn", "sampling", "weights", "all"])
def test_fit_composes_on_device(dev, what):
    X, Xn, y, w = nan_data()
    kw, fit_kw, rows = dict(FIT_KW), {}, X
    if what in ("learn", "all"):
        kw["missing_policy"], rows = "learn", Xn
    if what in ("sampling", "all"):
        kw.update(subsample=0.8, colsample_bynode=0.5, seed=3)
    for cons in (CONS, (0, 0, 0, 0), None):
        p = gb.GBDTParams(monotone_constraints=cons, **kw)
        wk = lambda d: {"sample_weight": torch.from_numpy(w).to(d)} if what in ("weights", "all") else {}  # noqa: E731
        ref = gb.fit(torch.from_numpy(rows), torch.from_numpy(y), p, **wk("cpu"))
        got = gb.fit(torch.from_numpy(rows).to(dev), torch.from_numpy(y).to(dev), p, **wk(dev))
        assert C.same_trees(got, ref)
        if kw.get("missing_policy") == "learn":
            assert np.array_equal(got.default_left, ref.default_left)
        if cons == CONS:
            mono = got
            assert_monotone(got, X, dev)  # over non-NaN values of the swept feature
        elif cons is None:
            assert C.same_trees(got, zero) and not C.same_trees(got, mono)
        else:
            zero = got


def test_early_stopping_keeps_monotone_trees(dev):
    X, y = C.fixture_data()
    Xd, yd = torch.from_numpy(X).to(dev), torch.from_numpy(y).to(dev)
    p = gb.GBDTParams(monotone_constraints=CONS, **{**FIT_KW, "n_estimators": 40, "learning_rate": 0.8})
    ens, rec = gb.fit(Xd[:450], yd[:450], p, eval_set=(Xd[450:], yd[450:]), early_stopping_rounds=3)
    ref, rec_c = gb.fit(torch.from_numpy(X[:450]), torch.from_numpy(y[:450]), p,
                        eval_set=(torch.from_numpy(X[450:]), torch.from_numpy(y[450:])), early_stopping_rounds=3)
    assert rec.stopped and ens.n_trees == rec.best_iteration + 1 < 40
    assert rec.best_iteration == rec_c.best_iteration and C.same_trees(ens, ref)
    assert_monotone(ens, X, dev)


def test_cv_job_and_pipeline_take_constraints(dev):
    from fraud_detection_amd.data.synthetic import separable
    from fraud_detection_amd.models.gbdt import GBDTPipeline
    from fraud_detection_amd.models.gbdt_cv import DeviceGBDTCV
    from fraud_detection_amd.models.pipeline import TrainConfig

    X, y = separable(6000, fraud_rate=0.05, seed=21, device=dev, n_features=8)
    # the data's own directions on features 1 .. 3 (they keep their splits), the opposite one on 4
    cons = (0, -1, 1, -1, -1, 0, 0, 0)
    p = gb.GBDTParams(n_estimators=6, max_depth=3, max_bin=32, learning_rate=0.5,
                      monotone_constraints={1: -1, 2: 1, 3: -1, 4: -1})
    free = gb.GBDTParams(n_estimators=6, max_depth=3, max_bin=32, learning_rate=0.5)
    cv = DeviceGBDTCV(TrainConfig(), p, n_folds=3).run(X, y)
    pipe = GBDTPipeline(TrainConfig(), p).fit(X, y)
    for res in (cv.final, pipe):
        ens = res.ensemble
        assert ens.params["monotone_constraints"] == list(cons)
        Xs = res.standardize(X[:64]).contiguous().cpu().numpy()  # a positive scale: the same constraint
        assert_monotone(ens, Xs, dev, cons)
        assert sum(int((ens.feat == f).sum()) for f in (1, 2, 3)) > 0
    assert len(cv.fold_aucs) == 3
    assert not C.same_trees(GBDTPipeline(TrainConfig(), free).fit(X, y).ensemble, pipe.ensemble)
