"""Numpy oracle of the K11 GBDT kernels (csrc/kernels/gbdt.hip), also the CPU execution path.

Same algorithm, same fixed-point quantisation, same fp64 operation order in the split gain,
same tie rules, so a device fit given the same quantised gradients builds bit-identical trees:

* cuts: per feature, sample quantiles at i*m//B (i = 1..B-1) of the sorted sample, deduplicated,
  values <= the sample minimum dropped, +inf appended (bin(x) = #cuts <= x, bins [0, nb-1]);
* split "bins <= b go left" <=> x < cuts[b]; gain = (GL^2/(HL+l) + GR^2/(HR+l)) - G^2/(H+l),
  valid when HL, HR >= min_child_weight; argmax over (feature, bin), ties -> lowest feature,
  then lowest bin; split iff gain > 1e-6 and not gain < gamma (xgboost kRtEps / pruner);
* complete heap trees of depth D; a non-split node passes every row to its left child;
* leaf = float32(eta * (-G/(H+l))) (0 when H < min_child_weight or H <= 0);
* a gain term G^2/(H+l) whose denominator H+l is <= 0 counts as 0 -- the node's own term and both
  child terms alike.  Only reg_lambda = 0 reaches it (an empty side, or rows whose quantised
  Hessian is 0): the term would be 0/0 or G^2/0, and a NaN or +inf gain decides nothing.  Where
  every denominator is positive -- every fit with reg_lambda > 0 -- no bit changes.  xgboost's
  CalcGain zeroes the term on H <= 0 whatever lambda is; that would change finite gains at
  min_child_weight = 0 (an empty child contributes 0^2/l = 0 either way, but a child with H = 0,
  G != 0 contributes G^2/l here), so it is deliberately not adopted.

Missing values (``missing=True``, GBDTParams.missing_policy = "learn"; default off, and off means
every function here is what it was):

* cuts: per feature over the sample's non-NaN values only, ranks floor(t m_f / B) with m_f the
  feature's non-NaN count and B = min(max_bin, 255); m_f = 0 gives nbins = 1, every cut +inf;
  nbins <= 255 counts real bins only;
* binning: a NaN of either sign goes to byte 255 (MISSING_BIN) for every feature, every other value
  (+-inf included) as before;
* split scan: with (Gm, Hm) the sums of slot 255, a feature's candidates in tie order are b = -1
  with default left (left = the missing rows only; stored bin -1, thr -inf, default_left 1), then
  for b = 0 .. nbins - 2 "missing right" (GL = prefix(b), default_left 0) and "missing left"
  (GL = prefix(b) + Gm, default_left 1).  Same gain formula and validity tests; ties go to the
  lowest feature, then the lowest b, then default_left 0 -- so NaN-free data gives default_left 0;
* direction: fp32 rows go right iff isnan(x) ? !default_left : !(x < thr); binned rows iff
  (v == 255) ? !default_left : v > bin.  x < -inf is false for every non-NaN x, so the b = -1
  split sends exactly the missing rows left in both walks.

Monotone constraints (``mono=(cons, lo, hi)`` / ``monotone=cons``; default off, and off means every
function here is what it was): cons[f] in {-1, 0, +1}, every heap node carries weight bounds
[lo, hi], the root (-inf, +inf) -- xgboost's TreeEvaluator in fp64:

* weight w(G, H) = clamp(H < mcw or H <= 0 ? 0 : -G / (H + l), lo, hi), the clamp after the zero rule
  and written w < lo ? lo : (w > hi ? hi : w);
* term(G, H, w) = -(2 G w + (H + l) w w) where H + l > 0, else 0 (unclamped it is G^2 / (H + l));
* a candidate's gain is (term(L, wl) + term(R, wr)) - term(node, w(node)), wl / wr the children's
  weights under the NODE's bounds; on a feature with c > 0 it needs wl <= wr, with c < 0 wl >= wr, on
  top of the unchanged validity tests.  Same tie order, same acceptance rule;
* children inherit [lo, hi]; with mid = (wl + wr) / 2 of the winning candidate, c > 0 sets
  hi[left] = lo[right] = mid and c < 0 sets lo[left] = hi[right] = mid; a pass-through node hands its
  bounds to both children;
* leaf = float32(eta * w(G, H)) under the leaf node's bounds.
With ``missing`` the missing rows count in whichever side the candidate puts them.

Interaction constraints (``interaction=`` group masks; default off, and off means every function
here is what it was): a list of groups, each a set of feature indices in [0, d) given as a bit mask;
groups may overlap and a feature may be in none -- xgboost's FeatureInteractionConstraintHost
(Reset / SplitImpl / Query) as a pure function of the path:

* a heap node's ``path`` is the set of split features of its proper ancestors that did split; a
  pass-through ancestor adds nothing and hands its path unchanged to both children;
* path empty (the root, or only pass-through ancestors): every one of the d features is allowed;
* otherwise allowed = path | union of the groups g with path a subset of g (interaction_allowed): a
  feature in no group may only be followed by itself, a feature in two groups opens both until a
  later split narrows the path to one of them;
* only eligibility changes: the node's candidates are those of ``fmask & allowed`` (the column
  sample is drawn first, then filtered; nothing left means no split) -- gain arithmetic, validity
  tests, tie order and the acceptance rule are untouched, and best_split is what it was.

L1 regularisation and max_delta_step (``reg=(alpha, max_delta_step)``; default None, and None means
every function here is what it was): a = reg_alpha >= 0, m = max_delta_step >= 0 (0: off), [lo, hi]
the node's monotone bounds ((-inf, +inf) when nothing is constrained).  Everything fp64, evaluated
as written:

* soft threshold T(G) = G > a ? G - a : (G < -a ? G + a : 0.0);
* weight w = (H < mcw or H <= 0) ? 0 : -T(G) / (H + l); then, if m > 0 and fabs(w) > m,
  w = copysign(m, w); last the monotone clamp w < lo ? lo : (w > hi ? hi : w) -- xgboost's order,
  CalcWeight first, the evaluator's bounds after it;
* term(G, H, w) = -(2 G w + (H + l) w w + 2 a fabs(w)) where H + l > 0, else 0: twice the reduction of
  the regularised objective G w + (H + l) w^2 / 2 + a |w| at w; where nothing clamps it is
  T(G)^2 / (H + l);
* gain = (term(L, wl) + term(R, wr)) - term(node, w(node)), all three weights under the node's own
  bounds.  With ``reg`` and no monotone constraint the scan takes this weight / term form with the
  bounds -inf / +inf.  Validity tests, tie order, acceptance rule, the learned missing side, feature
  masks, the monotone sign test and mid = (wl + wr) / 2 and the interaction paths are unchanged; wl,
  wr and mid use the weight above;
* leaf = float32(eta * w(G, H)) under the leaf node's bounds;
* against xgboost: with only one of the two set and no monotone constraint these gains equal
  xgboost's CalcGain in exact arithmetic (ThresholdL1(G)^2 / (H + l), resp. CalcGainGivenWeight).
  With both set xgboost's CalcGain ADDS a |w| to the term, and under monotone constraints its
  evaluator drops the a part of the term; here one formula, the objective's own, holds everywhere.
  Not adopted either: a in the quantile cuts, any per-objective default of max_delta_step.

xgboost itself is not installed in this image, so parity with xgboost is "unpinned"; the
semantics above follow xgboost's hist updater (train_model.py:69-80 uses XGBClassifier).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

MAX_BIN = 256
ROW_BYTES = 32
MISSING_BIN = 255  # the byte of a NaN under missing=True (real bins are then 0 .. 254)


def quantile_cuts(sample: np.ndarray, max_bin: int = MAX_BIN, missing: bool = False):
    """sample: [m, d] float32.  Returns (cuts [d, 256] float32 padded with +inf, nbins [d] int32).
    ``missing``: the quantiles of every feature over its non-NaN values only (module docstring)."""
    sample = np.asarray(sample, dtype=np.float32)
    m, d = sample.shape
    if max_bin < 2 or max_bin > MAX_BIN:
        raise ValueError("max_bin must be in [2, 256]")
    cuts = np.full((d, MAX_BIN), np.inf, dtype=np.float32)
    nbins = np.zeros(d, dtype=np.int32)
    if missing:
        B = min(max_bin, MAX_BIN - 1)
        srt = np.sort(sample, axis=0)  # NaN last, whatever its sign
        mf = (sample == sample).sum(0).astype(np.int64)
        idx = (np.arange(1, B, dtype=np.int64)[:, None] * mf[None, :]) // B  # < mf wherever mf > 0
        picks = np.take_along_axis(srt, idx, 0) if m else np.full((B - 1, d), np.nan, np.float32)
        return cuts_from_sorted_picks(picks, srt[0] if m else np.full(d, np.nan, np.float32), B, True)
    if m == 0:
        nbins[:] = 1
        return cuts, nbins
    idx = (np.arange(1, max_bin, dtype=np.int64) * m) // max_bin
    srt = np.sort(sample, axis=0)
    return cuts_from_sorted_picks(srt[idx], srt[0], max_bin)


def cuts_from_sorted_picks(picks: np.ndarray, vmin: np.ndarray, max_bin: int = MAX_BIN, missing: bool = False):
    """picks [max_bin-1, d]: sample values at the quantile positions; vmin [d]: sample minimum.
    ``missing``: picks and minimum were taken over the non-NaN values (max_bin <= 255); a NaN
    minimum means the feature has none (NaN sorts last): nbins = 1, every cut +inf."""
    picks = np.asarray(picks, dtype=np.float32)
    d = picks.shape[1]
    cuts = np.full((d, MAX_BIN), np.inf, dtype=np.float32)
    nbins = np.zeros(d, dtype=np.int32)
    if missing and max_bin > MAX_BIN - 1:
        raise ValueError("missing: at most 255 real bins")
    for f in range(d):
        if missing and vmin[f] != vmin[f]:
            nbins[f] = 1
            continue
        c = np.unique(picks[:, f])
        c = c[c > vmin[f]][: max_bin - 1]
        cuts[f, : len(c)] = c
        nbins[f] = len(c) + 1  # + the +inf cut
    return cuts, nbins


def bin_rows(X: np.ndarray, cuts: np.ndarray, nbins: np.ndarray, missing: bool = False) -> np.ndarray:
    """``missing``: a NaN goes to byte MISSING_BIN instead of the feature's last bin."""
    X = np.asarray(X, dtype=np.float32)
    n, d = X.shape
    out = np.zeros((n, ROW_BYTES), dtype=np.uint8)
    for f in range(d):
        nb = int(nbins[f])
        out[:, f] = np.searchsorted(cuts[f, :nb], X[:, f], side="right").clip(0, nb - 1)
        if missing:
            out[np.isnan(X[:, f]), f] = MISSING_BIN
    return out


GRAD_BITS = 14  # |g_q|, h_q <= 2^14: the device packs (h, g) of a row into one 64-bit LDS atomic


def grad_scales(scale_pos_weight: float, wmax: float = 1.0):
    """Power-of-two fixed-point scales with |g * gscale| <= 2^14 and h * hscale <= 2^14
    (h = p (1 - p) w <= w / 4): 2^16 rows of packed (h << 32) + g sum exactly in 64 bits.
    ``wmax``: the largest per-row sample weight of the fit (all ranks); the largest effective
    weight is W = max(scale_pos_weight, 1) * wmax.  With wmax = 1 (no weights, or all ones) the
    scales are what they always were."""
    W = max(float(scale_pos_weight), 1.0) * float(wmax)
    gscale = float(2.0 ** np.floor(np.log2((2.0 ** GRAD_BITS) / W)))
    return gscale, 4.0 * gscale


def effective_weights(y: np.ndarray, spw: float, weight=None) -> np.ndarray:
    """fp64 [n]: w_eff = (double)w_i * (y_i ? (double)(float)spw : 1.0), w_i float32 (None: 1)."""
    pos = np.asarray(y) != 0
    w = np.where(pos, float(np.float32(spw)), 1.0)
    if weight is not None:
        w = np.asarray(weight, dtype=np.float32).astype(np.float64) * w
    return w


def gradients(margin: np.ndarray, y: np.ndarray, spw: float, gscale: float, hscale: float, weight=None) -> np.ndarray:
    """int32 [n, 2] quantised (g, h) of the logistic loss (fp64 arithmetic on fp32 margins).
    ``weight``: float32 [n] per-row sample weights, one more exact factor in front of the
    quantisation: g = (p - y) w_eff, h = max(p (1 - p), 1e-16) w_eff (effective_weights)."""
    m = np.asarray(margin, dtype=np.float32).astype(np.float64)
    p = 1.0 / (1.0 + np.exp(-m))
    pos = np.asarray(y) != 0
    w = effective_weights(y, spw, weight)
    g = (p - pos.astype(np.float64)) * w
    h = np.maximum(p * (1.0 - p), 1e-16) * w
    return np.stack([np.rint(g * gscale), np.rint(h * hscale)], 1).astype(np.int32)


WEIGHT_MIN_QUANTA = 16.0  # a row with w_eff * gscale below this has < 16 quanta of gradient at full scale


def weight_stats(weight: np.ndarray, y=None, spw: float = 1.0):
    """(wmax, smallest positive w_eff or +inf, count of NaN / infinite / negative entries) of
    float32 weights -- what a fit validates and scales by (gbdt.hip gbdt_weight_stats_kernel)."""
    w = np.asarray(weight, dtype=np.float32)
    bad = ~(w >= 0) | np.isinf(w)
    ok = w[~bad]
    wmax = float(ok.max()) if ok.size else 0.0
    eff = effective_weights(y, spw, w)[~bad] if y is not None else ok.astype(np.float64)
    eff = eff[ok > 0]
    return wmax, (float(eff.min()) if eff.size else float("inf")), int(bad.sum())


def _hist(bins: np.ndarray, q: np.ndarray, node: np.ndarray, nn: int, d: int) -> np.ndarray:
    """int64 [nn, d, 256, 2] exact histograms (float64 bincount of integers in < 2^53 chunks)."""
    out = np.zeros((nn, d, MAX_BIN, 2), dtype=np.int64)
    n = bins.shape[0]
    step = max(1, int(2 ** 52 // (2 ** 31 + 1)) // 2)
    keys_f = (np.arange(d, dtype=np.int64) * MAX_BIN)[None, :]
    for lo in range(0, n, step):
        hi = min(n, lo + step)
        k = (node[lo:hi, None].astype(np.int64) * (d * MAX_BIN) + keys_f + bins[lo:hi, :d]).ravel()
        for c in range(2):
            w = np.repeat(q[lo:hi, c].astype(np.float64), d)
            out[..., c] += np.bincount(k, weights=w, minlength=nn * d * MAX_BIN).astype(np.int64).reshape(nn, d, MAX_BIN)
    return out


@dataclass
class TreeArrays:
    feat: np.ndarray   # [ni] int32, -1 = pass-through
    bin: np.ndarray    # [ni] int32
    thr: np.ndarray    # [ni] float32 (+inf when not split)
    gain: np.ndarray   # [ni] float64
    leaf: np.ndarray   # [nl] float32
    default_left: np.ndarray | None = None  # [ni] uint8 (build_tree with missing=True), else None


def best_split(H: np.ndarray, nbins: np.ndarray, ginv: float, hinv: float, lam: float, mcw: float,
               fmask: int | None = None, missing: bool = False, mono=None, reg=None):
    """H: int64 [d, 256, 2] of one node.  Returns (gain, feature, bin, GLq, HLq, Gq, Hq).
    ``fmask``: bit f set = feature f may be picked (None: all).  The node totals come from feature
    0's sums whether or not feature 0 is allowed; with no valid allowed split the gain is -inf.
    ``missing``: slot 255 holds the missing rows' sums and the scan learns their side (module
    docstring); the return value gains default_left as its eighth element and bin may be -1.
    ``mono``: (cons [d] in {-1, 0, 1}, lo, hi) -- the node's weight bounds and the features' signs
    (module docstring); None is the unconstrained scan, untouched.
    ``reg``: (alpha, max_delta_step) -- the weight / term form of the gain under L1 regularisation
    and the weight cap (module docstring), with bounds -inf / +inf where ``mono`` is None."""
    if missing:
        return _best_split_missing(H, nbins, ginv, hinv, lam, mcw, fmask, mono, reg)
    d = H.shape[0]
    cg = np.cumsum(H[:, :, 0], axis=1)
    chs = np.cumsum(H[:, :, 1], axis=1)
    Gq, Hq = int(cg[0, -1]), int(chs[0, -1])
    G, Hs = float(Gq) * ginv, float(Hq) * hinv
    root = G * G / (Hs + lam) if Hs + lam > 0.0 else 0.0
    GL = cg.astype(np.float64) * ginv
    HL = chs.astype(np.float64) * hinv
    GR = (Gq - cg).astype(np.float64) * ginv
    HR = (Hq - chs).astype(np.float64) * hinv
    dl, dr = HL + lam, HR + lam
    with np.errstate(all="ignore"):  # a term with a denominator <= 0 counts as 0 (module docstring)
        gain = (np.where(dl > 0.0, GL * GL / dl, 0.0) + np.where(dr > 0.0, GR * GR / dr, 0.0)) - root
    b = np.arange(MAX_BIN)[None, :]
    valid = (b < (nbins[:d, None] - 1)) & (HL >= mcw) & (HR >= mcw)
    if mono is not None or reg is not None:
        gain, ok = _mono_gain(GL, HL, GR, HR, G, Hs, lam, mcw, mono, reg)
        valid &= ok
    if fmask is not None:
        valid &= ((int(fmask) >> np.arange(d)) & 1).astype(bool)[:, None]
    gain = np.where(valid, gain, -np.inf)
    flat = int(np.argmax(gain))
    f, bb = divmod(flat, MAX_BIN)
    return float(gain[f, bb]), f, bb, int(cg[f, bb]), int(chs[f, bb]), Gq, Hq


def soft_threshold(G: float, alpha: float) -> float:
    """T(G) = G > alpha ? G - alpha : (G < -alpha ? G + alpha : 0.0)."""
    return G - alpha if G > alpha else (G + alpha if G < -alpha else 0.0)


def mono_weight(G: float, H: float, lam: float, mcw: float, lo: float, hi: float, reg=None) -> float:
    """clamp(H < mcw or H <= 0 ? 0 : -G / (H + lam), lo, hi) on Python floats (IEEE fp64).
    ``reg`` = (alpha, m): -T(G) / (H + lam) instead, capped to copysign(m, w) where m > 0 and
    fabs(w) > m, before the clamp."""
    if reg is None:
        w = 0.0 if (H < mcw or H <= 0.0) else -G / (H + lam)
        return lo if w < lo else (hi if w > hi else w)
    alpha, m = float(reg[0]), float(reg[1])
    w = 0.0 if (H < mcw or H <= 0.0) else -soft_threshold(G, alpha) / (H + lam)
    if m > 0.0 and abs(w) > m:
        w = float(np.copysign(m, w))
    return lo if w < lo else (hi if w > hi else w)


def mono_term(G: float, H: float, lam: float, w: float, reg=None) -> float:
    dn = H + lam
    if reg is None:
        return -(2.0 * G * w + dn * w * w) if dn > 0.0 else 0.0
    return -(2.0 * G * w + dn * w * w + 2.0 * float(reg[0]) * abs(w)) if dn > 0.0 else 0.0


def _mono_weight_v(G, H, lam, mcw, lo, hi, reg=None):
    with np.errstate(all="ignore"):
        if reg is None:
            w = np.where((H < mcw) | (H <= 0.0), 0.0, -G / (H + lam))
        else:
            alpha, m = float(reg[0]), float(reg[1])
            T = np.where(G > alpha, G - alpha, np.where(G < -alpha, G + alpha, 0.0))
            w = np.where((H < mcw) | (H <= 0.0), 0.0, -T / (H + lam))
            if m > 0.0:
                w = np.where(np.abs(w) > m, np.copysign(m, w), w)
    return np.where(w < lo, lo, np.where(w > hi, hi, w))


def _mono_term_v(G, H, lam, w, reg=None):
    dn = H + lam
    with np.errstate(all="ignore"):
        if reg is None:
            return np.where(dn > 0.0, -(2.0 * G * w + dn * w * w), 0.0)
        return np.where(dn > 0.0, -(2.0 * G * w + dn * w * w + 2.0 * float(reg[0]) * np.abs(w)), 0.0)


def _mono_gain(GL, HL, GR, HR, G, Hs, lam, mcw, mono, reg=None):
    """(gain table, sign test) of candidates with fp64 side sums [d, K] under mono = (cons, lo, hi);
    the expression order is gbdt.hip's (gbdt_split_kernel<MISS, true>).  ``mono`` None (with ``reg``):
    no signs, bounds -inf / +inf."""
    if mono is None:
        mono = (np.zeros(GL.shape[0], np.int64), -np.inf, np.inf)
    cons, lo, hi = mono
    lo, hi = float(lo), float(hi)
    root = mono_term(G, Hs, lam, mono_weight(G, Hs, lam, mcw, lo, hi, reg), reg)
    wl = _mono_weight_v(GL, HL, lam, mcw, lo, hi, reg)
    wr = _mono_weight_v(GR, HR, lam, mcw, lo, hi, reg)
    gain = (_mono_term_v(GL, HL, lam, wl, reg) + _mono_term_v(GR, HR, lam, wr, reg)) - root
    c = np.asarray(cons, np.int64)[: GL.shape[0], None]
    return gain, np.where(c > 0, wl <= wr, np.where(c < 0, wl >= wr, True))


def mono_children(c: int, lo: float, hi: float, GLq: int, HLq: int, Gq: int, Hq: int, ginv: float, hinv: float,
                  lam: float, mcw: float, reg=None):
    """(lo_left, hi_left, lo_right, hi_right) below a split on a feature of sign c whose left child
    has the sums (GLq, HLq): the weights are recomputed from the integers as the candidate's were."""
    lo, hi = float(lo), float(hi)
    if c == 0:
        return lo, hi, lo, hi
    wl = mono_weight(float(GLq) * ginv, float(HLq) * hinv, lam, mcw, lo, hi, reg)
    wr = mono_weight(float(Gq - GLq) * ginv, float(Hq - HLq) * hinv, lam, mcw, lo, hi, reg)
    mid = (wl + wr) / 2.0
    return (lo, mid, mid, hi) if c > 0 else (mid, hi, lo, mid)


def _best_split_missing(H, nbins, ginv, hinv, lam, mcw, fmask, mono=None, reg=None):
    """best_split with a learned side for slot 255.  Candidate (b, dl) sits at column 2 (b + 1) + dl
    of a [d, 512] gain table -- the tie order -- so one argmax picks the lowest feature, then the
    lowest b (-1 first), then default_left 0.  Column 0 (b = -1, nothing left) is no candidate."""
    d = H.shape[0]
    cg = np.cumsum(H[:, :, 0], axis=1)
    chs = np.cumsum(H[:, :, 1], axis=1)
    Gq, Hq = int(cg[0, -1]), int(chs[0, -1])
    G, Hs = float(Gq) * ginv, float(Hq) * hinv
    root = G * G / (Hs + lam) if Hs + lam > 0.0 else 0.0
    gm, hm = H[:, MISSING_BIN, 0], H[:, MISSING_BIN, 1]
    GLq = np.zeros((d, 2 * MAX_BIN), np.int64)
    HLq = np.zeros((d, 2 * MAX_BIN), np.int64)
    GLq[:, 1], HLq[:, 1] = gm, hm                                   # b = -1, default left
    GLq[:, 2::2], HLq[:, 2::2] = cg[:, :-1], chs[:, :-1]            # b = 0 .. 254, missing right
    GLq[:, 3::2], HLq[:, 3::2] = cg[:, :-1] + gm[:, None], chs[:, :-1] + hm[:, None]  # missing left
    GL = GLq.astype(np.float64) * ginv
    HL = HLq.astype(np.float64) * hinv
    GR = (Gq - GLq).astype(np.float64) * ginv
    HR = (Hq - HLq).astype(np.float64) * hinv
    dl, dr = HL + lam, HR + lam
    with np.errstate(all="ignore"):
        gain = (np.where(dl > 0.0, GL * GL / dl, 0.0) + np.where(dr > 0.0, GR * GR / dr, 0.0)) - root
    b = (np.arange(2 * MAX_BIN) >> 1)[None, :] - 1
    valid = (b < (nbins[:d, None] - 1)) & (HL >= mcw) & (HR >= mcw)
    valid[:, 0] = False
    if mono is not None or reg is not None:
        gain, ok = _mono_gain(GL, HL, GR, HR, G, Hs, lam, mcw, mono, reg)
        valid &= ok
    if fmask is not None:
        valid &= ((int(fmask) >> np.arange(d)) & 1).astype(bool)[:, None]
    gain = np.where(valid, gain, -np.inf)
    flat = int(np.argmax(gain))
    f, k = divmod(flat, 2 * MAX_BIN)
    return float(gain[f, k]), f, (k >> 1) - 1, int(GLq[f, k]), int(HLq[f, k]), Gq, Hq, k & 1


def bins_go_right(v: np.ndarray, b, default_left) -> np.ndarray:
    """The direction rule on bin bytes v: (v == 255) ? !default_left : v > b.  With default_left 0
    it is v > b for every byte (b <= 254 wherever 255 is the missing slot)."""
    v = np.asarray(v).astype(np.int64)
    return np.where((v == MISSING_BIN) & (np.asarray(default_left) != 0), False, v > b)


def interaction_allowed(path_mask: int, groups, d: int) -> int:
    """Allowed-feature bits of a node whose ancestors split on the features of ``path_mask``, under
    the interaction groups ``groups`` (bit masks) of a d-feature fit: all d features for an empty
    path, else the path's own features and every group that contains the whole path."""
    path_mask = int(path_mask)
    if path_mask == 0:
        return (1 << d) - 1
    allowed = path_mask
    for g in groups:
        if path_mask & ~int(g) == 0:
            allowed |= int(g)
    return allowed


def build_tree(bins: np.ndarray, q: np.ndarray, cuts: np.ndarray, nbins: np.ndarray, depth: int, lam: float,
               mcw: float, gamma: float, eta: float, gscale: float, hscale: float, comm=None, fmasks=None,
               missing: bool = False, monotone=None, interaction=None, reg=None):
    """Grow one depth-`depth` heap tree.  Returns (TreeArrays, leaf index per row [n]).
    ``fmasks``: uint32 [2^depth - 1] allowed-feature bits per heap node (feature_masks), or None.
    ``missing``: byte 255 of ``bins`` is the missing slot; TreeArrays.default_left is filled.
    ``monotone``: [d] signs in {-1, 0, 1} (None: unconstrained); every node gets weight bounds.
    ``interaction``: group masks (None: unconstrained); every node gets its ancestors' feature set
    and only fmask & interaction_allowed(path) may be picked.
    ``reg``: (alpha, max_delta_step) of the weights, gains and leaves (None: neither)."""
    n = bins.shape[0]
    d = int(len(nbins))
    ginv, hinv = 1.0 / gscale, 1.0 / hscale
    ni, nl = (1 << depth) - 1, 1 << depth
    feat = np.full(ni, -1, np.int32)
    binv = np.full(ni, 255, np.int32)
    thr = np.full(ni, np.inf, np.float32)
    gain = np.zeros(ni, np.float64)
    dleft = np.zeros(ni, np.uint8)
    ng = np.zeros(2 * nl - 1, np.int64)
    nh = np.zeros(2 * nl - 1, np.int64)
    blo = bhi = None
    if monotone is not None:
        monotone = np.asarray(monotone, np.int64)
        blo, bhi = np.full(2 * nl - 1, -np.inf), np.full(2 * nl - 1, np.inf)
    path = None if interaction is None else np.zeros(2 * nl - 1, np.int64)
    node = np.zeros(n, np.int64)  # index within the level
    for level in range(depth):
        nn = 1 << level
        Hl = _hist(bins, q, node, nn, d)
        if comm is not None and comm.world_size > 1:
            import torch

            Hl = comm.all_reduce(torch.from_numpy(Hl)).numpy()
        h0 = nn - 1
        right = np.zeros(n, bool)
        for k in range(nn):
            hid = h0 + k
            fm = None if fmasks is None else int(fmasks[hid])
            if interaction is not None:
                fm = ((1 << d) - 1 if fm is None else fm) & interaction_allowed(path[hid], interaction, d)
            mono = None if monotone is None else (monotone, blo[hid], bhi[hid])
            if missing:
                g_, f, b, GLq, HLq, Gq, Hq, dl = best_split(Hl[k], nbins, ginv, hinv, lam, mcw, fm, True, mono, reg)
            else:
                (g_, f, b, GLq, HLq, Gq, Hq), dl = best_split(Hl[k], nbins, ginv, hinv, lam, mcw, fm, mono=mono,
                                                                   reg=reg), 0
            if hid == 0:
                ng[0], nh[0] = Gq, Hq
            split = accepts_split(g_, gamma)
            lc, rc = 2 * hid + 1, 2 * hid + 2
            if split:
                feat[hid], binv[hid], thr[hid], gain[hid] = f, b, (cuts[f, b] if b >= 0 else -np.inf), g_
                dleft[hid] = dl
                ng[lc], nh[lc], ng[rc], nh[rc] = GLq, HLq, Gq - GLq, Hq - HLq
                sel = node == k
                right |= sel & (bins_go_right(bins[:, f], b, dl) if missing else (bins[:, f] > b))
            else:
                ng[lc], nh[lc], ng[rc], nh[rc] = Gq, Hq, 0, 0
            if monotone is not None:
                blo[lc], bhi[lc], blo[rc], bhi[rc] = mono_children(
                    int(monotone[f]) if split else 0, blo[hid], bhi[hid], GLq, HLq, Gq, Hq, ginv, hinv, lam, mcw, reg)
            if interaction is not None:
                path[lc] = path[rc] = path[hid] | ((1 << f) if split else 0)
        node = 2 * node + right.astype(np.int64)
    return TreeArrays(feat, binv, thr, gain, leaf_values(ng, nh, depth, ginv, hinv, lam, mcw, eta, blo, bhi, reg),
                      dleft if missing else None), node


def accepts_split(gain: float, gamma: float) -> bool:
    """The split rule on a node's best gain: gain > 1e-6 and not gain < gamma."""
    return bool(np.isfinite(gain) and gain > 1e-6 and not (gain < gamma))


def leaf_values(ng: np.ndarray, nh: np.ndarray, depth: int, ginv: float, hinv: float, lam: float, mcw: float,
                eta: float, lo=None, hi=None, reg=None) -> np.ndarray:
    """float32 [2^depth] leaf values from the heap's int64 node sums ng / nh (leaves at 2^depth - 1 ..).
    ``lo`` / ``hi``: [heap] weight bounds of a monotone fit (the weight is clamped into them).
    ``reg``: (alpha, max_delta_step) -- the weight is mono_weight(..., reg)'s (module docstring)."""
    ni, nl = (1 << depth) - 1, 1 << depth
    leaf = np.zeros(nl, np.float32)
    for i in range(nl):
        G, H = float(ng[ni + i]) * ginv, float(nh[ni + i]) * hinv
        if reg is not None:
            w = mono_weight(G, H, lam, mcw, -np.inf if lo is None else float(lo[ni + i]),
                            np.inf if hi is None else float(hi[ni + i]), reg)
        else:
            w = 0.0 if (H < mcw or H <= 0.0) else -G / (H + lam)
            if lo is not None:
                w = float(lo[ni + i]) if w < lo[ni + i] else (float(hi[ni + i]) if w > hi[ni + i] else w)
        leaf[i] = np.float32(eta * w)
    return leaf


# ---- stochastic boosting: stateless Philox draws ----------------------------------------------------
# Every draw is a pure function of (seed, round, global row | feature): repeated fits, data-parallel
# shards, checkpoint resumes and folds around a row hole all see the same bits.  The tags separate
# the four streams (counter word c3); gbdt.hip mirrors TAG_ROW.
TAG_ROW = 0x47425201
TAG_TREE = 0x47425402
TAG_LEVEL = 0x47424C03
TAG_NODE = 0x47424E04


def sample_threshold(subsample: float) -> int:
    """floor(subsample * 2^32) in fp64: a row is in the sample iff its 32-bit word is below it."""
    return int(np.floor(float(subsample) * 4294967296.0))


def row_sample_mask(seed: int, t: int, rows, subsample: float) -> np.ndarray:
    """bool [len(rows)]: which GLOBAL row ids (int64) are in round t's sample.  Row r takes word
    r & 3 of philox4x32_10(lo32(r >> 2), hi32(r >> 2), t, TAG_ROW, lo32(seed), hi32(seed)), so one
    call serves 4 consecutive rows."""
    from .reference import philox4x32_10

    rows = np.asarray(rows, dtype=np.int64)
    grp = (rows >> 2).astype(np.uint64)
    seed = int(seed)
    w = philox4x32_10((grp & np.uint64(0xFFFFFFFF)).astype(np.uint32), (grp >> np.uint64(32)).astype(np.uint32),
                      np.full(rows.shape, int(t) & 0xFFFFFFFF, np.uint32), np.full(rows.shape, TAG_ROW, np.uint32),
                      seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    word = np.choose(rows & 3, w) if rows.size else np.zeros(0, np.uint32)
    return word.astype(np.uint64) < np.uint64(sample_threshold(subsample))


def _colsample_stage(cand: list, frac: float, keys: np.ndarray) -> list:
    """The max(1, int(frac * len(cand))) features of `cand` with the smallest (key, feature)."""
    if frac == 1.0:
        return cand
    k = max(1, int(frac * len(cand)))
    return sorted(sorted(cand, key=lambda f: (int(keys[f]), f))[:k])


def feature_masks(seed: int, t: int, d: int, depth: int, bytree: float = 1.0, bylevel: float = 1.0,
                  bynode: float = 1.0) -> np.ndarray:
    """uint32 [2^depth - 1]: the allowed-feature bits of every heap node of round t's tree.  Three
    nested stages as in xgboost (node within level within tree); a stage with fraction c over the
    candidates C keeps the max(1, int(c * len(C))) features with the smallest (key, f),
    key = philox4x32_10(f, idx, t, TAG, lo32(seed), hi32(seed)).x with (idx, TAG) = (0, TAG_TREE),
    (level, TAG_LEVEL), (heap id, TAG_NODE).  A stage at 1.0 passes its set through without a draw."""
    from .reference import philox4x32_10

    seed = int(seed)
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    ni = (1 << depth) - 1

    def keys(idx, tag):  # [len(idx), d] uint32
        idx = np.asarray(idx, np.uint32)
        shape = (idx.shape[0], d)
        f = np.broadcast_to(np.arange(d, dtype=np.uint32)[None, :], shape)
        return philox4x32_10(f, np.broadcast_to(idx[:, None], shape), np.full(shape, int(t) & 0xFFFFFFFF, np.uint32),
                             np.full(shape, tag, np.uint32), k0, k1)[0]

    tree = _colsample_stage(list(range(d)), bytree, keys([0], TAG_TREE)[0] if bytree != 1.0 else None)
    lkeys = keys(np.arange(depth), TAG_LEVEL) if bylevel != 1.0 else None
    nkeys = keys(np.arange(ni), TAG_NODE) if bynode != 1.0 else None
    out = np.zeros(ni, np.uint32)
    for level in range(depth):
        lset = _colsample_stage(tree, bylevel, None if lkeys is None else lkeys[level])
        for hid in range((1 << level) - 1, (2 << level) - 1):
            nset = _colsample_stage(lset, bynode, None if nkeys is None else nkeys[hid])
            out[hid] = sum(1 << f for f in nset)
    return out


def feature_mask_table(seed: int, rounds: int, d: int, depth: int, bytree: float = 1.0, bylevel: float = 1.0,
                       bynode: float = 1.0) -> np.ndarray:
    """uint32 [rounds, 2^depth - 1]: feature_masks of rounds 0 .. rounds - 1, what a fit draws once
    (and uploads once).  The same draws taken for all rounds at a time: a stage is one Philox call
    over [round, index, feature] and one sort of (key << 5 | feature) with the non-candidates pushed
    to the end -- the candidate count of a stage is the same in every round and node."""
    from .reference import philox4x32_10

    seed = int(seed)
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    ni = (1 << depth) - 1
    fbits = np.uint32(1) << np.arange(d, dtype=np.uint32)
    if rounds == 0:
        return np.zeros((0, ni), np.uint32)

    def stage(cand, frac, idx, tag):  # cand: bool [rounds, len(idx) or 1, d]
        cand = np.broadcast_to(cand, (rounds, len(idx), d))
        if frac == 1.0:
            return cand
        k = max(1, int(frac * int(cand[0, 0].sum())))
        shape = cand.shape
        f = np.broadcast_to(np.arange(d, dtype=np.uint32), shape)
        key = philox4x32_10(f, np.broadcast_to(np.asarray(idx, np.uint32)[None, :, None], shape),
                            np.broadcast_to(np.arange(rounds, dtype=np.uint32)[:, None, None], shape),
                            np.full(shape, tag, np.uint32), k0, k1)[0]
        comp = np.where(cand, (key.astype(np.uint64) << np.uint64(5)) | f.astype(np.uint64), np.uint64(2 ** 64 - 1))
        out = np.zeros(shape, bool)
        np.put_along_axis(out, np.argsort(comp, axis=-1, kind="stable")[..., :k], True, axis=-1)
        return out

    tree = stage(np.ones((rounds, 1, d), bool), bytree, [0], TAG_TREE)
    level = stage(tree, bylevel, np.arange(depth), TAG_LEVEL)
    node_level = np.floor(np.log2(np.arange(ni) + 1)).astype(np.int64)  # heap id -> level
    node = stage(level[:, node_level, :], bynode, np.arange(ni), TAG_NODE)
    # C-contiguous whatever layout the indexing above left: row t is what round t's split launches read
    return np.ascontiguousarray((node * fbits).sum(-1, dtype=np.uint32))


LOSS_CAP = 36.841361487904734  # -ln(1e-16): xgboost clamps p to [eps, 1 - eps], eps = 1e-16
LOSS_SCALE = float(2 ** 30)    # fixed point of a row's log-loss
EVAL_MAX_ROWS = 1 << 27        # 36.85 * 2^30 * 2^27 < 2^63: the int64 loss sum cannot overflow


def eval_record(margin: np.ndarray, y: np.ndarray) -> np.ndarray:
    """int64 [4] = (loss_q, n_err, n_pos, n_rows) of fp32 margins against 0/1 labels -- the oracle
    of gbdt.hip's gbdt_eval_kernel.  loss_q = sum rint(loss * 2^30) with, per row in fp64,
    loss = min(softplus(y ? -m : m), -ln(1e-16)), softplus(z) = max(z, 0) + log1p(exp(-|z|));
    a row is an error when (m > 0) != (y != 0).  All four are exact integers, so records of
    disjoint row sets add."""
    m = np.asarray(margin, dtype=np.float32).astype(np.float64).ravel()
    pos = np.asarray(y).ravel() != 0
    if m.shape[0] > EVAL_MAX_ROWS:
        raise ValueError("at most 2^27 eval rows")
    z = np.where(pos, -m, m)
    with np.errstate(over="ignore"):
        sp = np.maximum(z, 0.0) + np.log1p(np.exp(-np.abs(z)))
    q = np.rint(np.fmin(sp, LOSS_CAP) * LOSS_SCALE).astype(np.int64)
    return np.array([q.sum(), np.count_nonzero((m > 0.0) != pos), np.count_nonzero(pos), m.shape[0]], dtype=np.int64)


EVAL_WEIGHT_BITS = 16   # u = w * wscale <= 2^16
EVAL_WEIGHT_SCALE = float(2 ** 14)  # 2^16 * 2^14 = LOSS_SCALE: unit weights give the unweighted loss terms


def eval_weight_scale(wmax: float) -> float:
    """wscale = 2^floor(log2(2^16 / wmax)) for the largest eval weight (all ranks), wmax > 0."""
    return float(2.0 ** np.floor(np.log2((2.0 ** EVAL_WEIGHT_BITS) / float(wmax))))


def eval_weight_q(w: np.ndarray, wscale: float) -> np.ndarray:
    """int64 [m]: rint(u * 2^14), u = w * wscale (exact: a power of two times an fp32) -- a row's
    term of the weight sum wsum_q and of the weighted error sum."""
    u = np.asarray(w, dtype=np.float32).astype(np.float64).ravel() * float(wscale)
    return np.rint(u * EVAL_WEIGHT_SCALE).astype(np.int64)


def eval_record_weighted(margin: np.ndarray, y: np.ndarray, w: np.ndarray, wscale: float) -> np.ndarray:
    """int64 [4] = (loss_q, err_q, n_pos, n_rows) with per-row weights (xgboost's
    sample_weight_eval_set) -- the oracle of gbdt.hip's weighted gbdt_eval_kernel.  With
    u = w * wscale <= 2^16: loss_q = sum rint(min(softplus, cap) * u * 2^14) and err_q = sum over
    the error rows of rint(u * 2^14); n_pos and n_rows are counts as in eval_record.  The metrics
    divide by wsum_q = eval_weight_q(w, wscale).sum(): logloss = loss_q / wsum_q, error = err_q /
    wsum_q.  All weights equal to the largest one (u = 2^16) give eval_record's loss_q."""
    m = np.asarray(margin, dtype=np.float32).astype(np.float64).ravel()
    pos = np.asarray(y).ravel() != 0
    if m.shape[0] > EVAL_MAX_ROWS:
        raise ValueError("at most 2^27 eval rows")
    u = np.asarray(w, dtype=np.float32).astype(np.float64).ravel() * float(wscale)
    z = np.where(pos, -m, m)
    with np.errstate(over="ignore"):
        sp = np.maximum(z, 0.0) + np.log1p(np.exp(-np.abs(z)))
    q = np.rint(np.fmin(sp, LOSS_CAP) * u * EVAL_WEIGHT_SCALE).astype(np.int64)
    eq = np.rint(u * EVAL_WEIGHT_SCALE).astype(np.int64)
    return np.array([q.sum(), eq[(m > 0.0) != pos].sum(), np.count_nonzero(pos), m.shape[0]], dtype=np.int64)


def twice_pairs(margin: np.ndarray, y: np.ndarray) -> int:
    """2 #{s_p > s_n} + #{s_p == s_n} over (positive, negative) pairs: AUC = twice_pairs / (2 P N)."""
    s = np.asarray(margin, dtype=np.float32).ravel()
    pos = np.asarray(y).ravel() != 0
    neg = np.sort(s[~pos])
    sp = s[pos]
    return int(np.searchsorted(neg, sp, side="left").sum() + np.searchsorted(neg, sp, side="right").sum())


def ap_q(margin: np.ndarray, y: np.ndarray) -> int:
    """The average precision of fp32 margins as an exact integer: sum over tie groups (descending)
    of rint(dtp * precision * 2^30); AP = ap_q / 2^30 / P (ops/reference.py average_precision_q)."""
    from .reference import average_precision_q

    return average_precision_q(np.asarray(margin, dtype=np.float32).ravel(), np.asarray(y).ravel())[0]


def predict_margin(X: np.ndarray, feat: np.ndarray, thr: np.ndarray, leaf: np.ndarray, depth: int,
                   base_margin: float = 0.0, default_left: np.ndarray | None = None) -> np.ndarray:
    """X [n, d] float32; feat/thr [T, ni]; leaf [T, nl].  float32 margins (sum in tree order).
    ``default_left`` [T, ni] (None: all zero): a NaN goes left at a node where it is set."""
    X = np.asarray(X, dtype=np.float32)
    n = X.shape[0]
    out = np.full(n, np.float32(base_margin), dtype=np.float32)
    rows = np.arange(n)
    for t in range(feat.shape[0]):
        node = np.zeros(n, np.int64)
        for _ in range(depth):
            f = feat[t][node]
            xv = X[rows, np.maximum(f, 0)]
            right = (f >= 0) & ~(xv < thr[t][node])
            if default_left is not None:
                right &= ~(np.isnan(xv) & (default_left[t][node] != 0))
            node = 2 * node + 1 + right
        out = (out + leaf[t][node - ((1 << depth) - 1)]).astype(np.float32)
    return out


def predict_margin_bins(bins: np.ndarray, feat: np.ndarray, binv: np.ndarray, leaf: np.ndarray, depth: int,
                        base_margin: float = 0.0, default_left: np.ndarray | None = None) -> np.ndarray:
    """The device margin walk (gbdt.hip gbdt_margin_kernel) on binned rows: a row goes right at a
    node when its bin of the node's feature exceeds the split bin.  float32, summed in tree order.
    ``default_left`` [T, ni] (None: all zero): byte 255 goes left at a node where it is set."""
    bins = np.asarray(bins)
    n = bins.shape[0]
    out = np.full(n, np.float32(base_margin), dtype=np.float32)
    rows = np.arange(n)
    for t in range(feat.shape[0]):
        node = np.zeros(n, np.int64)
        for _ in range(depth):
            f = feat[t][node]
            bv = bins[rows, np.maximum(f, 0)].astype(np.int64)
            right = (f >= 0) & (bv > binv[t][node])
            if default_left is not None:
                right &= ~((bv == MISSING_BIN) & (default_left[t][node] != 0))
            node = 2 * node + 1 + right
        out = (out + leaf[t][node - ((1 << depth) - 1)]).astype(np.float32)
    return out


COVER_SCALE = float(2 ** 30)  # fixed point of a row's hessian in node covers
COVER_KINDS = ("hessian", "count")


def node_cover(X: np.ndarray, feat: np.ndarray, thr: np.ndarray, leaf: np.ndarray, depth: int,
               base_margin: float = 0.0, default_left: np.ndarray | None = None, kind: str = "hessian") -> np.ndarray:
    """int64 [T, 2^(depth+1)] node covers by 1-based heap node (index 0 unused and 0) over the fp32
    rows X [n, d]: the oracle of csrc/kernels/treecover.hip.

    kind "count": rows that reach the node.  kind "hessian" (xgboost's sum_hess): the sum over those
    rows of h_q = llrint(p (1 - p) 2^30), p = sigmoid((double)m), m the fp32 margin of the row before
    tree t (float(base_margin) plus the leaves of trees 0 .. t-1 added in tree order in fp32:
    predict_margin(..., n_trees = t)).  Routing is predict_margin's.  Leaves are accumulated and an
    internal node is the exact integer sum of its children."""
    if kind not in COVER_KINDS:
        raise ValueError(f"cover kind must be one of {COVER_KINDS}, not {kind!r}")
    X = np.asarray(X, dtype=np.float32)
    n = X.shape[0]
    T = feat.shape[0]
    ni, nl = (1 << depth) - 1, 1 << depth
    out = np.zeros((T, 2 * nl), np.int64)
    rows = np.arange(n)
    margin = np.full(n, np.float32(base_margin), dtype=np.float32)
    for t in range(T):
        node = np.zeros(n, np.int64)
        for _ in range(depth):
            f = feat[t][node]
            xv = X[rows, np.maximum(f, 0)]
            right = (f >= 0) & ~(xv < thr[t][node])
            if default_left is not None:
                right &= ~(np.isnan(xv) & (default_left[t][node] != 0))
            node = 2 * node + 1 + right
        lf = node - ni
        if kind == "count":
            w = np.ones(n, np.int64)
        else:
            p = 1.0 / (1.0 + np.exp(-margin.astype(np.float64)))
            w = np.rint(p * (1.0 - p) * COVER_SCALE).astype(np.int64)
        np.add.at(out[t], nl + lf, w)
        margin = (margin + leaf[t][lf]).astype(np.float32)
        for k in range(nl - 1, 0, -1):
            out[t, k] = out[t, 2 * k] + out[t, 2 * k + 1]
    return out


# ---- partial dependence / ICE of the margin ---------------------------------------------------------
# The model is piecewise constant, so the complete curve of feature f has one value per CELL: the
# intervals between the ensemble's distinct thresholds on f (models/explainers.py
# TreePartialDependence has the definitions; csrc/kernels/tree_pd.hip is the device form).
PD_SCALE = float(2 ** 30)  # fixed point of a row's margin in the partial-dependence sums
PD_MAX_CELLS = 65536


def pd_grid(ens, f: int) -> np.ndarray:
    """E_f, float32 ascending: the distinct thresholds of the nodes that split on feature f, -inf (a
    "missing rows only" split, bin -1) dropped.  K_f = len(E_f) edges make K_f + 1 value cells."""
    f = int(f)
    if not 0 <= f < ens.n_features:
        raise ValueError(f"feature {f} out of range [0, {ens.n_features})")
    thr = np.asarray(ens.thr, np.float32)[np.asarray(ens.feat) == f]
    return np.unique(thr[thr != -np.inf])


def pd_cells(ens, f: int):
    """(representatives float32 [C], has_missing): cell 0 is -inf (below every edge), cell c >= 1 the
    edge E_f[c - 1] (standing for [E_f[c-1], E_f[c])), and where the model has learned default
    directions one last cell NaN, "missing"."""
    reps = np.concatenate([np.array([-np.inf], np.float32), pd_grid(ens, f)])
    if ens.has_default_left:
        reps = np.concatenate([reps, np.array([np.nan], np.float32)])
    return reps, bool(ens.has_default_left)


def pd_features(ens, features) -> tuple:
    """``features`` (an int or a pair of distinct ints) as a checked tuple."""
    fs = (int(features),) if np.isscalar(features) else tuple(int(v) for v in features)
    if len(fs) not in (1, 2):
        raise ValueError("partial dependence takes one feature or a pair")
    for f in fs:
        if not 0 <= f < ens.n_features:
            raise ValueError(f"feature {f} out of range [0, {ens.n_features})")
    if len(fs) == 2 and fs[0] == fs[1]:
        raise ValueError("the two features of a pair must differ")
    return fs


def pd_check(ens, features, n: int):
    """(features tuple, per-feature representatives, has_missing) after the family's limits, the cell
    cap and the int64 guard: with Mb = |base_margin| + sum_t max |leaf_t| a sum of n rows stays below
    2^63 when n (Mb + 1) 2^30 < 2^63."""
    if not 1 <= ens.depth <= 5:
        raise ValueError("partial dependence supports depth 1..5 (the reference trains max_depth=5)")
    if not 1 <= ens.n_trees <= 2048:
        raise ValueError("partial dependence supports 1..2048 trees")
    if ens.n_features > 30:
        raise ValueError(f"tree explainers support at most 30 features, the model has {ens.n_features}")
    fs = pd_features(ens, features)
    cells = [pd_cells(ens, f) for f in fs]
    total = int(np.prod([len(r) for r, _ in cells]))
    if total > PD_MAX_CELLS:
        raise ValueError(f"{total} cells: at most {PD_MAX_CELLS} (shorten the model with iteration_range or take "
                         "one feature)")
    leaf = np.abs(np.asarray(ens.leaf, np.float64))
    if not np.all(np.isfinite(leaf)):
        raise ValueError("partial dependence needs finite leaf values")
    mb = abs(float(ens.base_margin)) + float(leaf.max(1).sum())
    if float(n) * (mb + 1.0) * PD_SCALE >= 2.0 ** 63:
        raise ValueError(f"{n} rows of margins up to {mb:.3g} would overflow the int64 sums")
    return fs, [r for r, _ in cells], bool(ens.has_default_left)


def partial_dependence_reference(Xs: np.ndarray, ens, features, ice: bool = True):
    """The oracle: ICE and brute partial dependence of the margin on STANDARDIZED rows Xs [n, d] by
    predict_margin on copies of Xs whose column f holds the cell's representative (NaN for the missing
    cell).  Returns (pd_q int64 [C], ice float32 [n, C] or None); a pair's cells are flattened as
    ca * C_b + cb; pd_q[c] = sum_i rint((double)ice[i, c] * 2^30)."""
    Xs = np.asarray(Xs, np.float32)
    if Xs.ndim != 2 or Xs.shape[1] != ens.n_features:
        raise ValueError(f"model has {ens.n_features} features, X has shape {Xs.shape}")
    fs, reps, _ = pd_check(ens, features, Xs.shape[0])
    dl = ens.default_left if ens.has_default_left else None
    n, d = Xs.shape
    pair = len(fs) == 2
    cb = len(reps[1]) if pair else 1
    va = np.repeat(reps[0], cb)                       # the flattened cell's value of the first feature
    vb = np.tile(reps[1], len(reps[0])) if pair else None
    C = len(va)
    out = np.empty((n, C), np.float32)
    step = max(1, (1 << 20) // max(n, 1))             # cells per predict_margin call: <= 2^20 rows at a time
    for c0 in range(0, C, step):
        c1 = min(C, c0 + step)
        Xm = np.repeat(Xs[None], c1 - c0, 0)          # [cells, n, d]
        Xm[:, :, fs[0]] = va[c0:c1, None]
        if pair:
            Xm[:, :, fs[1]] = vb[c0:c1, None]
        m = predict_margin(Xm.reshape(-1, d), ens.feat, ens.thr, ens.leaf, ens.depth, ens.base_margin, dl)
        out[:, c0:c1] = m.reshape(c1 - c0, n).T
    pd_q = np.rint(out.astype(np.float64) * PD_SCALE).astype(np.int64).sum(0)
    return pd_q, (out if ice else None)


# ---- permutation feature importance -----------------------------------------------------------------
# Column (feature f, repeat r) gives row i the value of feature f of row donors[i] and leaves the
# rest of the row as observed (models/explainers.py TreePermutationImportance has the definitions;
# csrc/kernels/feistel_perm.h and tree_perm.hip are the device form).
def _fmix32(x):
    x = np.asarray(x, dtype=np.uint32).copy()
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x85EBCA6B)
    x ^= x >> np.uint32(13)
    x *= np.uint32(0xC2B2AE35)
    x ^= x >> np.uint32(16)
    return x


def permutation_donors(n: int, seed: int, f: int, r: int) -> np.ndarray:
    """int64 [n]: the permutation of the rows that column (feature f, repeat r) reads feature f
    through.  A keyed Feistel bijection with cycle walking (the construction of ops/split's class
    permutation on the domain [0, n)): 4 rounds over half-words of h = (b + 1) >> 1 bits, 2^b >= n and
    b >= 2, fmix32 as the round function, applied again while the value is >= n; keys
    key[k] = fmix32(seed ^ fmix32(0x9E3779B9 (2 c + 1) + k)) with the column id c = 32 r + f.  So
    repeat r of feature f is the same permutation whatever else is asked for.  ``seed`` is an integer
    in [0, 2^32)."""
    n, seed, f, r = int(n), int(seed), int(f), int(r)
    if n < 0:
        raise ValueError("negative row count")
    if not 0 <= seed < 2 ** 32:
        raise ValueError("seed must be an integer in [0, 2^32)")
    if not 0 <= f < 32 or r < 0:
        raise ValueError("column (f, r) needs 0 <= f < 32 and r >= 0")
    c = 32 * r + f
    b = 2
    while b < 64 and (1 << b) < n:
        b += 1
    h = (b + 1) >> 1
    mask = np.uint64((1 << h) - 1)
    with np.errstate(over="ignore"):
        keys = [int(_fmix32(np.uint32(seed) ^ _fmix32(np.uint32((0x9E3779B9 * (2 * c + 1) + k) & 0xFFFFFFFF))))
                for k in range(4)]
        x = np.arange(n, dtype=np.uint64)
        todo = np.ones(n, bool)
        while todo.any():
            xs = x[todo]
            L, Rh = xs >> np.uint64(h), xs & mask
            for kv in keys:
                g = _fmix32((Rh ^ np.uint64(kv)).astype(np.uint32)).astype(np.uint64) & mask
                L, Rh = Rh, L ^ g
            xs = (L << np.uint64(h)) | Rh
            x[todo] = xs
            todo[todo] = xs >= np.uint64(n)
    return x.astype(np.int64)


def perm_check(ens, features, n_repeats: int, seed: int) -> tuple:
    """The checked feature tuple of a permutation-importance call (None: every feature) after the
    family's limits: depth 1..5, 1..2048 trees, at most 30 features."""
    if not 1 <= ens.depth <= 5:
        raise ValueError("permutation importance supports depth 1..5 (the reference trains max_depth=5)")
    if not 1 <= ens.n_trees <= 2048:
        raise ValueError("permutation importance supports 1..2048 trees")
    d = ens.n_features
    if d > 30:
        raise ValueError(f"tree explainers support at most 30 features, the model has {d}")
    if int(n_repeats) < 1:
        raise ValueError("n_repeats must be at least 1")
    if not 0 <= int(seed) < 2 ** 32:
        raise ValueError("seed must be an integer in [0, 2^32)")
    fs = tuple(range(d)) if features is None else tuple(int(v) for v in np.atleast_1d(np.asarray(features)))
    for f in fs:
        if not 0 <= f < d:
            raise ValueError(f"feature {f} out of range [0, {d})")
    if len(set(fs)) != len(fs):
        raise ValueError("a feature is listed twice")
    if len(fs) < 1:
        raise ValueError("no feature to permute")
    return fs


def permuted_margins_reference(Xs: np.ndarray, ens, features, n_repeats: int, seed: int):
    """The oracle: (float32 [F, R, n], float32 [n]) -- predict_margin on explicit copies of the
    STANDARDIZED rows Xs [n, d] whose column f is Xs[permutation_donors(n, seed, f, r), f], and
    predict_margin of Xs itself (the baseline)."""
    Xs = np.asarray(Xs, np.float32)
    if Xs.ndim != 2 or Xs.shape[1] != ens.n_features:
        raise ValueError(f"model has {ens.n_features} features, X has shape {Xs.shape}")
    fs = perm_check(ens, features, n_repeats, seed)
    dl = ens.default_left if ens.has_default_left else None
    n = Xs.shape[0]
    out = np.empty((len(fs), int(n_repeats), n), np.float32)
    for i, f in enumerate(fs):
        for r in range(int(n_repeats)):
            Xm = Xs.copy()
            Xm[:, f] = Xs[permutation_donors(n, seed, f, r), f]
            out[i, r] = predict_margin(Xm, ens.feat, ens.thr, ens.leaf, ens.depth, ens.base_margin, dl)
    return out, predict_margin(Xs, ens.feat, ens.thr, ens.leaf, ens.depth, ens.base_margin, dl)
