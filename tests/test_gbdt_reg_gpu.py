"""GBDT reg_alpha / max_delta_step on the device: every gbdt_split_kernel instantiation that carries a
RegArgs (MISS x MONO x INTER, with and without an fmask row) and gbdt_leaf with the two values against
the numpy oracle -- every output exact, gains and bounds bitwise -- then whole fits: device trees
equal to the oracle's bit for bit, alone and composed with sampling, weights, learned missing
directions, monotone and interaction constraints, early stopping and the captured graph, and the two
estimator-level properties.  The two-rank fit runs on the CPU path
(test_gbdt_reg.test_dp_equals_single_process): the scan sees only all-reduced histograms."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import _gbdt_state as S
import test_gbdt_interaction as IC
import test_gbdt_kernels_gpu as K
import test_gbdt_missing_gpu as M
import test_gbdt_monotone_gpu as G
import test_gbdt_reg as C
from fraud_detection_amd.models.gbdt import GBDTClassifier
from fraud_detection_amd.ops import gbdt as gb
from fraud_detection_amd.ops import reference_gbdt as R
from fraud_detection_amd.ops.native import native, ptr, stream_of

pytestmark = pytest.mark.gpu

GINV, HINV = K.GINV, K.HINV  # powers of two: an integer sum times GINV is exact
INF = np.inf
PATH_SENT = 0x5A5A5A5A
KINDS = ("alpha", "mds", "both")


# ---- gbdt_split with the RegArgs tail ---------------------------------------------------------------------
def split_oracle(hist, gcnt, level, d, nbins, cuts, lam, mcw, gamma, reg, cons=None, lo=None, hi=None, elig=None,
                 missing=False):
    """The level's decisions: derived nodes first become parent - sibling, then best_split(mono=, reg=)
    + the split rule + mono_children(reg=).  ``elig``: uint32 [heap] eligible-feature words (fmask and
    interaction already combined) or None.  Returns (hist after, feat, device bin words, thr, gain,
    {heap id: (ng, nh)}, {heap id: (lo, hi)})."""
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
                           None if elig is None else int(elig[node]), missing, mono, reg)
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
                                             lam, mcw, reg)
            bounds[2 * node + 1], bounds[2 * node + 2] = (ll, lh), (rl, rh)
    words = gb.encode_bin_words(binv, dl) if missing else binv
    return hist, feat, words, thr, gain, sums, bounds


def run_split(dev, hist, gcnt, level, d, nbins, cuts, lam, mcw, gamma, reg, cons=None, lo=None, hi=None, fmask=None,
              missing=False, masks=None, path=None):
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
    mono, bounds = (0, 0, 0, 0), None
    if cons is not None:
        b_lo, b_hi = np.full(2 * ni + 1, G.SENT), np.full(2 * ni + 1, G.SENT)
        if level:  # a level-0 block must not read its bounds
            b_lo[h0:h0 + nn], b_hi[h0:h0 + nn] = lo, hi
        blo, bhi = S.to_dev(b_lo, dev), S.to_dev(b_hi, dev)
        mono = (*G.masks_of(cons), ptr(blo), ptr(bhi))
    inter, p0 = ([], 0), None
    if masks is not None:
        p0 = np.full(2 * ni + 1, PATH_SENT, np.int32)
        if level:
            p0[h0:h0 + nn] = path
        pd = S.to_dev(p0, dev)
        inter = ([int(g) for g in masks], ptr(pd))
    m.gbdt_split(ptr(hd), ptr(gd), level, d, ptr(nt), ptr(ct), GINV, HINV, float(lam), float(mcw), float(gamma),
                 ptr(feat), ptr(binv), ptr(thr), ptr(gain), ptr(ng), ptr(nh), stream_of(hd),
                 0 if fm is None else ptr(fm), missing, *mono, *inter, reg_alpha=reg[0], max_delta_step=reg[1])
    torch.cuda.synchronize()
    sl = slice(h0, h0 + nn)
    got = (hd.cpu().numpy().reshape(hist.shape), feat[sl].cpu().numpy(), binv[sl].cpu().numpy(), thr[sl].cpu().numpy(),
           gain[sl].cpu().numpy(), ng.cpu().numpy(), nh.cpu().numpy())
    if cons is not None:
        bounds = (blo.cpu().numpy(), bhi.cpu().numpy(), b_lo, b_hi)
    return got, bounds, (None if masks is None else (pd.cpu().numpy(), p0))


def split_both(dev, hist, gcnt, level, d, nbins, cuts, lam, mcw, gamma, reg, cons=None, lo=None, hi=None, fmask=None,
               missing=False, masks=None, path=None):
    """Every output of the kernel against the oracle, exactly: feat, bin words, thr, gain bitwise, ng /
    nh (nothing else written), the histogram after derivation, the bounds of a monotone launch bitwise
    and the path words of a launch with interaction groups."""
    h0, nn = S.heap_first(level), 1 << level
    elig = fmask
    if masks is not None:
        elig = eligible_words(level, d, masks, path, fmask)
    ref = split_oracle(hist, gcnt, level, d, nbins, cuts, lam, mcw, gamma, reg, cons, lo, hi, elig, missing)
    got, bounds, paths = run_split(dev, hist, gcnt, level, d, nbins, cuts, lam, mcw, gamma, reg, cons, lo, hi, fmask,
                                   missing, masks, path)
    S.assert_split_equal(got, ref[:6], level)
    if cons is not None:
        blo, bhi, lo0, hi0 = bounds
        for node, (a, b) in ref[6].items():
            lo0[node], hi0[node] = a, b
        assert blo.tobytes() == lo0.tobytes() and bhi.tobytes() == hi0.tobytes()
    if masks is not None:
        pth, want = paths
        want = want.copy()
        if level == 0:
            want[0] = 0
        for k in range(nn):
            node = h0 + k
            below = (int(path[k]) if level else 0) | ((1 << int(ref[1][k])) if ref[1][k] >= 0 else 0)
            want[2 * node + 1] = want[2 * node + 2] = below
        assert np.array_equal(pth, want)
    return ref


def eligible_words(level, d, masks, path, fmask):
    """uint32 [heap]: fmask & interaction_allowed(path) of every node of the level (level 0: path 0)."""
    h0, nn = S.heap_first(level), 1 << level
    out = np.zeros((2 << level) - 1, np.uint32)
    for k in range(nn):
        fm = (1 << d) - 1 if fmask is None else int(fmask[h0 + k])
        out[h0 + k] = fm & R.interaction_allowed(int(path[k]) if level else 0, masks, d)
    return out


def node_hist(hist, gcnt, level, k, d):
    """int64 [d, 256, 2] of node k of the level (a derived node: parent - sibling)."""
    h0, nn = S.heap_first(level), 1 << level
    node = h0 + k
    if S.built_mask(level, gcnt[h0:h0 + nn])[k]:
        return hist[node, :d]
    return hist[(node - 1) >> 1, :d] - hist[h0 + (k ^ 1), :d]


def candidate_sides(H, nbins, mcw, missing=False):
    """The fp64 (G, H) of both sides of every candidate the scan evaluates on a node's histogram H
    [d, 256, 2]: b < nbins - 1 and both sides' H >= mcw (with ``missing`` the two placements of slot
    255 and the b = -1 candidate).  Returns (GL, HL, GR, HR) as flat arrays."""
    cg, chs = np.cumsum(H[:, :, 0], 1), np.cumsum(H[:, :, 1], 1)
    Gq, Hq = cg[:, -1:], chs[:, -1:]
    b = np.arange(256)[None, :]
    ok = b < (np.asarray(nbins)[:, None] - 1)
    GLq, HLq = [cg], [chs]
    oks = [ok]
    if missing:
        gm, hm = H[:, 255:256, 0], H[:, 255:256, 1]
        GLq += [cg + gm, np.broadcast_to(gm, cg.shape)[:, :1]]
        HLq += [chs + hm, np.broadcast_to(hm, chs.shape)[:, :1]]
        oks += [ok, np.ones((H.shape[0], 1), bool)]
    out = [[], [], [], []]
    for gl, hl, o in zip(GLq, HLq, oks):
        GL, HL = gl.astype(np.float64) * GINV, hl.astype(np.float64) * HINV
        GR, HR = (Gq - gl).astype(np.float64) * GINV, (Hq - hl).astype(np.float64) * HINV
        v = o & (HL >= mcw) & (HR >= mcw)
        for acc, a in zip(out, (GL, HL, GR, HR)):
            acc.append(a[v])
    return tuple(np.concatenate(a) for a in out)


def reg_from_hist(hist, gcnt, level, d, nbins, lam, mcw, kind, missing=False, k=0):
    """(alpha, m) built from node k's own candidates, exact: alpha = the median |G| over the candidates'
    sides (an integer sum times GINV), m = the median |w| over the sides' non-zero weights under that
    alpha (one candidate's own weight).  Returns (reg, stats) with stats counting the sides inside
    [-alpha, alpha], exactly at alpha, the weights exactly at m and above m by sign."""
    GL, HL, GR, HR = candidate_sides(node_hist(hist, gcnt, level, k, d), nbins, mcw, missing)
    Gs, Hs = np.concatenate([GL, GR]), np.concatenate([HL, HR])
    alpha = 0.0
    if kind in ("alpha", "both") and Gs.size:
        alpha = float(np.sort(np.abs(Gs))[Gs.size // 2])
    w = R._mono_weight_v(Gs, Hs, lam, mcw, -INF, INF, (alpha, 0.0)) if Gs.size else np.zeros(0)
    m_ = 0.0
    if kind in ("mds", "both") and np.any(w != 0.0):
        nz = np.sort(np.abs(w[w != 0.0]))
        m_ = float(nz[nz.size // 2])
    stats = {"inside": int((np.abs(Gs) < alpha).sum()), "at_alpha": int((np.abs(Gs) == alpha).sum()) if alpha else 0,
             "at_m": int((np.abs(w) == m_).sum()) if m_ else 0, "above_pos": int((w > m_).sum()) if m_ else 0,
             "above_neg": int((w < -m_).sum()) if m_ else 0}
    return (alpha, m_), stats


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("d", [1, 5, 30])
@pytest.mark.parametrize("level", [0, 1, 2])
def test_split_random_histograms(dev, level, d, kind):
    """gbdt_split_kernel<false, false, RegArgs>: built and derived nodes, 2 / 3 / 255 / 256 bins,
    reg_lambda 0 and 1, min_child_weight 0 and 1, alpha and m taken from the first node's candidates."""
    rng = np.random.default_rng(100 * level + d)
    nb = np.array([G.SPLIT_NBINS[(f + level) % 4] for f in range(d)], np.int32)
    cuts = K._cuts(rng, d)
    n_split = n_changed = 0
    for lam, mcw in ((0.0, 0.0), (1.0, 1.0), (1.0, 0.0), (0.0, 1.0)):
        hist, gcnt = K._level_hists(rng, level, d, nb, 1 << 30, 1 << 24)
        reg, _ = reg_from_hist(hist, gcnt, level, d, nb, lam, mcw, kind, k=(1 << level) - 1)
        if reg == (0.0, 0.0):  # a 2-bin single feature whose only candidate is invalid: nothing to build from
            reg = {"alpha": (0.5, 0.0), "mds": (0.0, 0.01), "both": (0.5, 0.01)}[kind]
        ref = split_both(dev, hist, gcnt, level, d, nb, cuts, lam, mcw, 0.0, reg)
        free = S.split_level_oracle(hist, gcnt, level, d, nb, cuts, GINV, HINV, lam, mcw, 0.0)
        n_split += int((ref[1] >= 0).sum())
        n_changed += int(ref[4].tobytes() != free[4].tobytes())
        if level:
            h0, nn = S.heap_first(level), 1 << level
            assert (~S.built_mask(level, gcnt[h0:h0 + nn])).sum() == nn // 2
    assert n_changed > 0
    if d > 1:
        assert n_split > 0


@pytest.mark.parametrize("mono", [False, True], ids=["free", "mono"])
@pytest.mark.parametrize("missing", [False, True], ids=["plain", "missing"])
@pytest.mark.parametrize("kind", KINDS)
def test_split_parameter_combinations(dev, kind, missing, mono):
    """All eight instantiations with a RegArgs, each with and without an fmask row: alpha alone, m
    alone, both; bounds in every state of test_gbdt_monotone_gpu.BOUND_STATES on some node."""
    level = 2
    nn, h0 = 1 << level, S.heap_first(level)
    seen = set()
    n_split = 0
    for d in (5, 30):
        rng = np.random.default_rng(10 * d + missing + 2 * mono)
        nb = (np.array([M.SPLIT_NBINS[(f + level) % 7] for f in range(d)], np.int32) if missing
              else np.array([G.SPLIT_NBINS[(f + level) % 4] for f in range(d)], np.int32))
        cuts = K._cuts(rng, d)
        groups = IC.random_groups(rng, d, 3)
        for rep, (masked, inter) in enumerate(((False, False), (True, False), (False, True), (True, True))):
            lam, mcw = ((0.0, 0.0), (1.0, 1.0), (10.0, 0.0), (1.0, 0.0))[rep]
            hist, gcnt = (M if missing else K)._level_hists(rng, level, d, nb, 1 << 30, 1 << 24)
            reg, _ = reg_from_hist(hist, gcnt, level, d, nb, lam, mcw, kind, missing, k=rep)
            assert reg != (0.0, 0.0)
            fmask = rng.integers(1, 1 << d, hist.shape[0]).astype(np.uint32) if masked else None
            masks = path = None
            if inter:
                masks = IC.masks_of(groups)
                path = np.array([0, 1 << (d - 1), 1 << 1, (1 << (d - 1)) | 1][:nn], np.int32)
            cons = lo = hi = None
            if mono:
                cons = rng.integers(-1, 2, d)
                cons[0] = cons[0] or 1
                states = [G.BOUND_STATES[(k + rep + d) % 5] for k in range(nn)]
                seen |= set(states)
                bl = [G.bounds_for(s, G.node_weight(hist, level, k, gcnt, d, lam)) for k, s in enumerate(states)]
                lo, hi = np.array([b[0] for b in bl]), np.array([b[1] for b in bl])
            ref = split_both(dev, hist, gcnt, level, d, nb, cuts, lam, mcw, 0.0, reg, cons, lo, hi, fmask, missing,
                             masks, path)
            n_split += int((ref[1] >= 0).sum())
    assert n_split > 0
    assert not mono or seen == set(G.BOUND_STATES)


@pytest.mark.parametrize("missing", [False, True], ids=["plain", "missing"])
@pytest.mark.parametrize("level", [0, 1])
def test_split_alpha_and_m_built_from_the_histogram(dev, level, missing):
    """alpha is one candidate side's |G| and m one candidate side's |w|, both exact: the oracle says
    that some side lies strictly inside [-alpha, alpha], one exactly at alpha, one weight exactly at
    m, and weights of both signs above m -- and the kernel agrees with it bit for bit on all of them."""
    rng = np.random.default_rng(7 + level)
    d = 5
    nb = np.array([255, 64, 16, 3, 200], np.int32)
    cuts = K._cuts(rng, d)
    for lam, mcw in ((1.0, 1.0), (0.0, 0.0)):
        hist, gcnt = (M if missing else K)._level_hists(rng, level, d, nb, 1 << 30, 1 << 24)
        reg, st = reg_from_hist(hist, gcnt, level, d, nb, lam, mcw, "both", missing)
        assert st["inside"] > 0 and st["at_alpha"] > 0 and st["at_m"] > 0, st
        assert st["above_pos"] > 0 and st["above_neg"] > 0, st
        both = split_both(dev, hist, gcnt, level, d, nb, cuts, lam, mcw, 0.0, reg, missing=missing)
        a_only = split_both(dev, hist, gcnt, level, d, nb, cuts, lam, mcw, 0.0, (reg[0], 0.0), missing=missing)
        m_only = split_both(dev, hist, gcnt, level, d, nb, cuts, lam, mcw, 0.0, (0.0, reg[1]), missing=missing)
        assert len({both[4].tobytes(), a_only[4].tobytes(), m_only[4].tobytes()}) == 3
        # under bounds too: the cap first, the clamp after it (lo above m on node 0)
        cons = np.array([1, -1, 0, 1, -1])
        nn = 1 << level
        lo = np.full(nn, -INF)
        hi = np.full(nn, INF)
        if level:
            lo[0], hi[1] = 1.5 * reg[1], -0.5 * reg[1]
        split_both(dev, hist, gcnt, level, d, nb, cuts, lam, mcw, 0.0, reg, cons, lo, hi, missing=missing)


def test_split_zero_values_launch_the_old_kernels(dev):
    """reg_alpha = max_delta_step = 0 by keyword: the results of the call without them, bit for bit,
    with and without the monotone tail."""
    rng = np.random.default_rng(5)
    d, level = 5, 1
    nb = np.full(d, 64, np.int32)
    cuts = K._cuts(rng, d)
    hist, gcnt = K._level_hists(rng, level, d, nb, 1 << 30, 1 << 24)
    want = S.split_level_oracle(hist, gcnt, level, d, nb, cuts, GINV, HINV, 1.0, 1.0, 0.0)
    got, _, _ = run_split(dev, hist, gcnt, level, d, nb, cuts, 1.0, 1.0, 0.0, (0.0, 0.0))
    S.assert_split_equal(got, want, level)
    cons, lo, hi = np.array([1, -1, 0, 0, 1]), np.array([-0.01, -INF]), np.array([INF, 0.02])
    ref = G.split_oracle(hist, gcnt, level, d, nb, cuts, 1.0, 1.0, 0.0, cons, lo, hi)
    got, _, _ = run_split(dev, hist, gcnt, level, d, nb, cuts, 1.0, 1.0, 0.0, (0.0, 0.0), cons, lo, hi)
    S.assert_split_equal(got, ref[:6], level)


# ---- gbdt_leaf with the two values -----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("depth", [1, 3, 7])
def test_leaf_kernel(dev, depth, kind):
    rng = np.random.default_rng(depth)
    m = native()
    nl, ni = 1 << depth, (1 << depth) - 1
    hs = int(1 / HINV)
    ng = rng.integers(-(1 << 24), 1 << 24, 2 * nl - 1)
    nh = rng.integers(hs, 1 << 22, 2 * nl - 1)
    alpha = float(abs(int(ng[ni + nl // 2]))) * GINV if kind != "mds" else 0.0  # one leaf's |G| exactly
    nh[ni] = hs - 1  # H < min_child_weight: 0 before the clamp
    w0 = np.array([R.mono_weight(float(g) * GINV, float(h) * HINV, 1.0, 1.0, -INF, INF, (alpha, 0.0)) for g, h in zip(ng, nh)])
    nz = np.sort(np.abs(w0[ni:][w0[ni:] != 0.0]))
    m_ = 0.0
    if kind != "alpha":  # one leaf's |w| exactly (half of it where there is only one); no weight left: any value
        m_ = 0.125 if not nz.size else float(nz[(nz.size - 1) // 2]) if nz.size > 1 else float(nz[0]) / 2.0
    reg = (alpha, m_)
    lo, hi = np.full(2 * nl - 1, -INF), np.full(2 * nl - 1, INF)
    state = rng.integers(0, 4, 2 * nl - 1)
    lo[state == 1] = w0[state == 1] + 0.01
    hi[state == 2] = w0[state == 2] - 0.01
    lo[state == 3], hi[state == 3] = w0[state == 3] - 0.5, w0[state == 3] + 0.5
    lo[ni], hi[ni] = (2.0 * m_ if m_ else 0.125), INF  # the zero is lifted to lo, above the cap
    ngd, nhd, lod, hid = (S.to_dev(a, dev) for a in (ng.astype(np.int64), nh.astype(np.int64), lo, hi))
    leaf = torch.full((nl,), -7.0, dtype=torch.float32, device=dev)
    plain = R.leaf_values(ng, nh, depth, GINV, HINV, 1.0, 1.0, 0.3)
    seen = []
    for bounds in (False, True):
        want = R.leaf_values(ng, nh, depth, GINV, HINV, 1.0, 1.0, 0.3, lo if bounds else None, hi if bounds else None, reg)
        m.gbdt_leaf(ptr(ngd), ptr(nhd), depth, GINV, HINV, 1.0, 1.0, 0.3, ptr(leaf), stream_of(leaf),
                    *((ptr(lod), ptr(hid)) if bounds else ()), reg_alpha=reg[0], max_delta_step=reg[1])
        torch.cuda.synchronize()
        assert leaf.cpu().numpy().tobytes() == want.tobytes()
        assert want.tobytes() != plain.tobytes()
        seen.append(want)
        if bounds:
            assert want[0] == np.float32(0.3 * lo[ni])
        else:
            assert want[0] == 0.0
            if m_:
                assert np.all(np.abs(want) <= np.float32(0.3 * m_))
                assert np.any(np.abs(want) == np.float32(0.3 * m_)) == bool(np.any(np.abs(w0[ni:]) >= m_))
            if alpha:
                assert want[nl // 2] == 0.0
    assert seen[0].tobytes() != seen[1].tobytes()
    # zeros by keyword: the leaf kernel as it always was
    m.gbdt_leaf(ptr(ngd), ptr(nhd), depth, GINV, HINV, 1.0, 1.0, 0.3, ptr(leaf), stream_of(leaf), reg_alpha=0.0,
                max_delta_step=0.0)
    torch.cuda.synchronize()
    assert leaf.cpu().numpy().tobytes() == plain.tobytes()


def test_launcher_refusals(dev):
    """Negative and NaN values raise before any launch: every output buffer keeps its fill."""
    m = native()
    z = torch.zeros(4096, dtype=torch.int64, device=dev)
    out = torch.full((64,), -7.0, dtype=torch.float64, device=dev)
    leaf = torch.full((8,), -7.0, dtype=torch.float32, device=dev)
    for kw, msg in (({"reg_alpha": -1.0}, "reg_alpha must be finite"), ({"reg_alpha": float("nan")}, "reg_alpha must be finite"),
                    ({"max_delta_step": -0.5}, "max_delta_step must be finite"),
                    ({"max_delta_step": float("nan")}, "max_delta_step must be finite"),
                    ({"reg_alpha": 1.0, "max_delta_step": float("inf")}, "max_delta_step must be finite")):
        with pytest.raises(RuntimeError, match=msg):
            m.gbdt_split(ptr(z), ptr(z), 0, 4, ptr(z), ptr(z), 1.0, 1.0, 1.0, 1.0, 0.0, ptr(z), ptr(z), ptr(z), ptr(out),
                         ptr(z), ptr(z), stream_of(z), **kw)
        with pytest.raises(RuntimeError, match=msg):
            m.gbdt_leaf(ptr(z), ptr(z), 3, 1.0, 1.0, 1.0, 1.0, 0.1, ptr(leaf), stream_of(z), **kw)
    torch.cuda.synchronize()
    assert torch.all(out == -7.0) and torch.all(leaf == -7.0) and torch.all(z == 0)


# ---- whole fits ------------------------------------------------------------------------------------------------
FIT_KW, REG_KW = C.FIT_KW, C.REG_KW


@pytest.fixture(scope="module")
def data(dev):
    X, y = C.fixture_data()
    rng = np.random.default_rng(11)
    Xn = X.copy()
    Xn[rng.random(C.N) < 0.1, 0] = np.nan
    Xn[rng.random(C.N) < 0.1, 2] = np.nan
    return X, Xn, y, rng.uniform(0.25, 2.0, C.N).astype(np.float32)


def both_fits(dev, rows, y, p, w=None, **kw):
    wk = lambda d: {} if w is None else {"sample_weight": torch.from_numpy(w).to(d)}  # noqa: E731
    mv = lambda t, d: tuple(torch.from_numpy(a).to(d) for a in t)  # noqa: E731
    ev = lambda d: {k: (mv(v, d) if k == "eval_set" else v) for k, v in kw.items()}  # noqa: E731
    ref = gb.fit(torch.from_numpy(rows), torch.from_numpy(y), p, **wk("cpu"), **ev("cpu"))
    got = gb.fit(torch.from_numpy(rows).to(dev), torch.from_numpy(y).to(dev), p, **wk(dev), **ev(dev))
    return got, ref


@pytest.mark.parametrize("kind", KINDS)
def test_fit_equals_oracle(dev, data, kind):
    X, _, y, _ = data
    reg = {"alpha": dict(reg_alpha=1.5), "mds": dict(max_delta_step=0.4), "both": REG_KW}[kind]
    p = gb.GBDTParams(**FIT_KW, **reg)
    got, ref = both_fits(dev, X, y, p)
    assert C.same_trees(got, ref) and (got.feat >= 0).any()
    assert got.params == ref.params and set(reg) <= set(got.params)
    plain, plain_c = both_fits(dev, X, y, gb.GBDTParams(**FIT_KW))
    assert C.same_trees(plain, plain_c) and not C.same_trees(plain, got)
    zero = gb.fit(torch.from_numpy(X).to(dev), torch.from_numpy(y).to(dev),
                  gb.GBDTParams(**FIT_KW, reg_alpha=0.0, max_delta_step=0.0))
    assert zero.to_dict() == plain.to_dict()


@pytest.mark.parametrize("what", ["sampling", "weights", "learn", "monotone", "interaction", "all"])
def test_fit_composes_on_device(dev, data, what):
    X, Xn, y, w = data
    kw, rows, wt = dict(FIT_KW, max_depth=4, n_estimators=5), X, None
    if what in ("sampling", "all"):
        kw.update(subsample=0.8, colsample_bynode=0.5, seed=3)
    if what in ("weights", "all"):
        wt = w
    if what in ("learn", "all"):
        kw["missing_policy"], rows = "learn", Xn
    if what in ("monotone", "all"):
        kw["monotone_constraints"] = (1, -1, 0, 0, 0, 0)
    if what in ("interaction", "all"):
        kw["interaction_constraints"] = [[0, 1], [2, 3, 4]]
    got, ref = both_fits(dev, rows, y, gb.GBDTParams(**kw, **REG_KW), wt)
    assert C.same_trees(got, ref) and (got.feat >= 0).any()
    if kw.get("missing_policy") == "learn":
        assert np.array_equal(got.default_left, ref.default_left)
    assert np.all(np.abs(got.leaf) <= np.float32(0.3 * 0.4))
    free, free_c = both_fits(dev, rows, y, gb.GBDTParams(**kw), wt)
    assert C.same_trees(free, free_c) and not C.same_trees(free, got)


def test_early_stopping_on_an_eval_set(dev, data):
    X, _, y, _ = data
    p = gb.GBDTParams(**{**FIT_KW, "n_estimators": 40, "learning_rate": 0.8}, reg_alpha=0.5, max_delta_step=2.0)
    (ens, rec), (ref, rec_c) = both_fits(dev, X[:1500], y[:1500], p, eval_set=(X[1500:], y[1500:]), early_stopping_rounds=3)
    assert rec.stopped and ens.n_trees == rec.best_iteration + 1 < 40
    assert rec.best_iteration == rec_c.best_iteration and C.same_trees(ens, ref)


@pytest.mark.parametrize("mono", [False, True], ids=["free", "mono"])
def test_graph_path_replays_the_values(dev, data, mono):
    X, _, y, _ = data
    extra = {"monotone_constraints": (1, -1, 0, 0, 0, 0)} if mono else {}
    p = gb.GBDTParams(**{**FIT_KW, "n_estimators": 6}, **REG_KW, **extra)
    Xd, yd = torch.from_numpy(X).to(dev), torch.from_numpy(y).to(dev)
    eager = gb.fit(Xd, yd, p)
    graph = gb.fit(Xd, yd, p, use_graph=True)
    assert C.same_trees(graph, eager)
    assert C.same_trees(eager, gb.fit(torch.from_numpy(X), torch.from_numpy(y), p))


@pytest.mark.parametrize("spw", [1.0, 13.0])
def test_large_alpha_leaves_every_tree_empty(dev, data, spw):
    X, _, y, _ = data
    alpha = 2.0 * C.N * max(spw, 1.0)
    clf = GBDTClassifier(device="cuda", scale_pos_weight=spw, base_score=0.3, reg_alpha=alpha, **FIT_KW).fit(X, y)
    ens = clf.ensemble
    assert np.all(ens.feat == -1) and np.all(ens.gain == 0.0) and np.all(ens.leaf == 0.0)
    assert np.all(np.asarray(clf.predict_margin(X)) == np.float32(np.log(0.3 / 0.7)))


def test_leaf_bound_on_device(dev, data):
    X, _, y, _ = data
    for m_, eta in ((1e-3, 0.3), (0.05, 1.0)):
        clf = GBDTClassifier(device="cuda", max_delta_step=m_, **{**FIT_KW, "learning_rate": eta}).fit(X, y)
        ens = clf.ensemble
        bound = np.float32(eta * m_)
        assert np.all(np.abs(ens.leaf) <= bound)
        assert all(np.any(np.abs(ens.leaf[t]) == bound) for t in range(ens.n_trees))  # the cap is at work in every tree
        p = gb.GBDTParams(**{**FIT_KW, "learning_rate": eta}, max_delta_step=m_)
        assert sum(1 for _ in C.replay(X, y, ens, p)) == 4  # the oracle's trees, round by round
