"""GBDT interaction constraints on the device: all eight gbdt_split_kernel instantiations (fmask x
MISS x MONO, each with the interaction tail) against the numpy oracle, every output exact and the
path words checked entry by entry; then whole fits -- device trees equal to the oracle's bit for bit
and every path inside a group -- alone and composed with column and row sampling, learned missing
directions, monotone constraints, weights, early stopping, the row hole, the captured graph, the CV
job and the pipeline.  The two-rank fit runs on the CPU path
(test_gbdt_interaction.test_dp_equals_single_process): the constrained scan sees only all-reduced
histograms.  The composed fits, early stopping, the row hole and the checkpoint resume all run at
the whole-fit shapes (30 features, depth 7), not at the CPU file's small fixture."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import _gbdt_state as S
import test_gbdt_interaction as C
import test_gbdt_kernels_gpu as K
import test_gbdt_missing_gpu as M
import test_gbdt_monotone_gpu as G
from fraud_detection_amd.ops import gbdt as gb
from fraud_detection_amd.ops import reference_gbdt as R
from fraud_detection_amd.ops.native import native, ptr, stream_of

pytestmark = pytest.mark.gpu

GINV, HINV = K.GINV, K.HINV
SENT = 0x5A5A5A5A  # what a path word holds before a block stores into it (as a path it would restrict)
INF = np.inf


# ---- gbdt_split with the interaction tail ------------------------------------------------------------
def eligible_words(level, d, masks, path, fmask):
    """uint32 [heap]: fmask & interaction_allowed(path) of every node of the level (level 0: path 0)."""
    h0, nn = S.heap_first(level), 1 << level
    out = np.zeros((2 << level) - 1, np.uint32)
    for k in range(nn):
        fm = (1 << d) - 1 if fmask is None else int(fmask[h0 + k])
        out[h0 + k] = fm & R.interaction_allowed(int(path[k]) if level else 0, masks, d)
    return out


def run_split(dev, hist, gcnt, level, d, nbins, cuts, lam, mcw, gamma, masks, path, fmask, missing, cons, lo, hi):
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
    p0 = np.full(2 * ni + 1, SENT, np.int32)
    if level:  # a level-0 block must not read its path word: it stays the sentinel
        p0[h0:h0 + nn] = path
    pd = S.to_dev(p0, dev)
    fm = S.to_dev(np.asarray(fmask, np.uint32).view(np.int32), dev) if fmask is not None else None
    mono = ()
    if cons is not None:
        b_lo, b_hi = np.full(2 * ni + 1, G.SENT), np.full(2 * ni + 1, G.SENT)
        if level:
            b_lo[h0:h0 + nn], b_hi[h0:h0 + nn] = lo, hi
        blo, bhi = S.to_dev(b_lo, dev), S.to_dev(b_hi, dev)
        mono = (*G.masks_of(cons), ptr(blo), ptr(bhi))
    else:
        mono = (0, 0, 0, 0)
    m.gbdt_split(ptr(hd), ptr(gd), level, d, ptr(nt), ptr(ct), GINV, HINV, float(lam), float(mcw), float(gamma),
                 ptr(feat), ptr(binv), ptr(thr), ptr(gain), ptr(ng), ptr(nh), stream_of(hd),
                 0 if fm is None else ptr(fm), missing, *mono, [int(g) for g in masks], ptr(pd))
    torch.cuda.synchronize()
    sl = slice(h0, h0 + nn)
    got = (hd.cpu().numpy().reshape(hist.shape), feat[sl].cpu().numpy(), binv[sl].cpu().numpy(), thr[sl].cpu().numpy(),
           gain[sl].cpu().numpy(), ng.cpu().numpy(), nh.cpu().numpy())
    bounds = (blo.cpu().numpy(), bhi.cpu().numpy(), b_lo, b_hi) if cons is not None else None
    return got, pd.cpu().numpy(), p0, bounds


def split_both(dev, hist, gcnt, level, d, nbins, cuts, lam, mcw, gamma, masks, path, fmask=None, missing=False,
               cons=None, lo=None, hi=None):
    """Every output of the kernel against the oracle, exactly: feat, bin words, thr, gain bitwise, the
    children's sums, the histogram after derivation, the bounds of a monotone launch, and the path
    words -- none written but node 0's (level 0) and the children's."""
    h0, nn = S.heap_first(level), 1 << level
    elig = eligible_words(level, d, masks, path, fmask)
    ref = G.split_oracle(hist, gcnt, level, d, nbins, cuts, lam, mcw, gamma, cons, lo, hi, elig, missing)
    got, pth, p0, bounds = run_split(dev, hist, gcnt, level, d, nbins, cuts, lam, mcw, gamma, masks, path, fmask,
                                     missing, cons, lo, hi)
    S.assert_split_equal(got, ref[:6], level)
    want = p0.copy()
    if level == 0:
        want[0] = 0
    for k in range(nn):
        node = h0 + k
        below = (int(path[k]) if level else 0) | ((1 << int(ref[1][k])) if ref[1][k] >= 0 else 0)
        want[2 * node + 1] = want[2 * node + 2] = below
    assert np.array_equal(pth, want), (pth, want)
    if cons is not None:
        blo, bhi, lo0, hi0 = bounds
        for node, (a, b) in ref[6].items():
            lo0[node], hi0[node] = a, b
        assert blo.tobytes() == lo0.tobytes() and bhi.tobytes() == hi0.tobytes()
    return ref, elig


def incoming_paths(rng, level, d, groups):
    """One path word per node of the level, cycling: empty, one listed feature, one unlisted feature,
    two features of one group, two features no group holds together.  Returns (words, kinds)."""
    nn = 1 << level
    listed = sorted({f for g in groups for f in g})
    unlisted = [f for f in range(d) if f not in listed]
    multi = [g for g in groups if len(g) >= 2]
    sets = [set(g) for g in groups]
    apart = [(a, b) for a in range(d) for b in range(a + 1, d) if not any({a, b} <= s for s in sets)]
    words, kinds = np.zeros(nn, np.int32), []
    for k in range(nn):
        kind = ("empty", "listed", "unlisted", "inside", "apart")[(k + level) % 5] if level else "empty"
        if kind == "listed":
            w = 1 << int(rng.choice(listed))
        elif kind == "unlisted" and unlisted:
            w = 1 << int(rng.choice(unlisted))
        elif kind == "inside" and multi:
            g = multi[int(rng.integers(len(multi)))]
            w = sum(1 << int(f) for f in rng.choice(g, size=2, replace=False))
        elif kind == "apart" and apart:
            a, b = apart[int(rng.integers(len(apart)))]
            w = (1 << a) | (1 << b)
        else:
            kind, w = "empty", 0
        words[k] = w
        kinds.append(kind)
    return words, kinds


@pytest.mark.parametrize("n_groups", [1, 2, 32])
@pytest.mark.parametrize("d", [1, 5, 30])
@pytest.mark.parametrize("level", [0, 1, 3, 6])
def test_split_all_instantiations(dev, level, d, n_groups):
    """Random int64 histograms with built and derived nodes, random incoming paths of every kind, with
    and without fmask, MISS and MONO; under fmask some nodes get a sample that misses the allowed set
    entirely: no split, and the children inherit the path."""
    rng = np.random.default_rng(1000 * level + 10 * d + n_groups)
    nn, h0 = 1 << level, S.heap_first(level)
    groups = C.random_groups(rng, d, n_groups)
    masks = C.masks_of(groups)
    cuts = K._cuts(rng, d)
    seen, n_split, n_narrow, n_empty = set(), 0, 0, 0
    for missing in (False, True):
        nb = (np.array([M.SPLIT_NBINS[(f + level) % 7] for f in range(d)], np.int32) if missing
              else np.array([G.SPLIT_NBINS[(f + level) % 4] for f in range(d)], np.int32))
        hist, gcnt = (M if missing else K)._level_hists(rng, level, d, nb, 1 << 30, 1 << 24)
        for masked in (False, True):
            for mono in (False, True):
                lam, mcw = ((0.0, 0.0), (1.0, 1.0), (10.0, 0.0), (1.0, 0.0))[2 * masked + mono]
                path, kinds = incoming_paths(rng, level, d, groups)
                seen |= set(kinds)
                fmask = None
                if masked:
                    fmask = rng.integers(1, 1 << d, hist.shape[0]).astype(np.uint32)
                    for k in range(level and nn):  # every third restricted node: a sample outside the allowed set
                        al = R.interaction_allowed(int(path[k]), masks, d)
                        if k % 3 == 0 and path[k] and al != (1 << d) - 1:
                            fmask[h0 + k] = ((1 << d) - 1) & ~al
                cons = lo = hi = None
                if mono:
                    cons = rng.integers(-1, 2, d)
                    cons[0] = cons[0] or 1
                    states = ["around" if (level and k % 2) else "inf" for k in range(nn)]
                    bl = [G.bounds_for(s, G.node_weight(hist, level, k, gcnt, d, lam)) for k, s in enumerate(states)]
                    lo, hi = np.array([b[0] for b in bl]), np.array([b[1] for b in bl])
                ref, elig = split_both(dev, hist, gcnt, level, d, nb, cuts, lam, mcw, 0.0, masks, path, fmask, missing,
                                       cons, lo, hi)
                n_split += int((ref[1] >= 0).sum())
                n_narrow += int(sum(int(elig[h0 + k]) != (1 << d) - 1 for k in range(nn)))
                for k in range(nn):
                    if elig[h0 + k] == 0:
                        n_empty += 1
                        assert ref[1][k] == -1
                    elif ref[1][k] >= 0:
                        assert (int(elig[h0 + k]) >> int(ref[1][k])) & 1
    assert n_split > 0
    if level and d > 1:
        assert n_narrow > 0
        assert len(seen) >= (2 if level == 1 else 4), seen
    if level >= 3 and d == 30:
        assert n_empty > 0


def test_split_level0_ignores_path_word_and_root_allows_all(dev):
    """The root has no path: every feature competes whatever path[0] holds, also a feature in no group."""
    rng = np.random.default_rng(3)
    d, nb = 5, np.full(5, 16, np.int32)
    cuts = K._cuts(rng, d)
    hist, gcnt = K._level_hists(rng, 0, d, nb, 1 << 30, 1 << 24)
    free = S.split_level_oracle(hist, gcnt, 0, d, nb, cuts, GINV, HINV, 1.0, 1.0, 0.0)
    for groups in ([(0,)], [(1, 2)], [(0, 1), (2, 3)]):
        ref, _ = split_both(dev, hist, gcnt, 0, d, nb, cuts, 1.0, 1.0, 0.0, C.masks_of(groups), np.zeros(1, np.int32))
        assert ref[1][0] == free[1][0] >= 0 and ref[4][0] == free[4][0]


def test_split_named_paths(dev):
    """One histogram under chosen paths: a feature in two groups opens both, a later split narrows, a
    path inside no group or on an unlisted feature leaves the path itself."""
    rng = np.random.default_rng(9)
    d, level = 6, 3
    nb = np.full(d, 32, np.int32)
    cuts = K._cuts(rng, d)
    groups = [(0, 1, 2), (2, 3)]
    masks = C.masks_of(groups)
    hist, gcnt = K._level_hists(rng, level, d, nb, 1 << 30, 1 << 24)
    path = np.array([0, 1 << 2, (1 << 2) | (1 << 3), (1 << 0) | (1 << 2), (1 << 0) | (1 << 3), 1 << 5, 1 << 4, 1 << 1], np.int32)
    want = [0b111111, 0b001111, 0b001100, 0b000111, 0b001001, 0b100000, 0b010000, 0b000111]
    ref, elig = split_both(dev, hist, gcnt, level, d, nb, cuts, 1.0, 0.0, 0.0, masks, path)
    assert [int(e) for e in elig[7:15]] == want
    assert all(f >= 0 and (w >> f) & 1 for f, w in zip(ref[1], want))
    free = S.split_level_oracle(hist, gcnt, level, d, nb, cuts, GINV, HINV, 1.0, 0.0, 0.0)
    assert np.any(free[1] != ref[1])


@pytest.mark.parametrize("missing", [False, True], ids=["plain", "missing"])
def test_split_pass_through_hands_path_unchanged(dev, missing):
    """Every node has a best candidate and gamma rejects it: both children get the node's path as it
    came, the candidate's feature is not added."""
    rng = np.random.default_rng(12)
    d, level = 5, 3
    groups = [(0, 1, 2), (2, 3)]
    nb = np.full(d, 16, np.int32)
    cuts = K._cuts(rng, d)
    hist, gcnt = (M if missing else K)._level_hists(rng, level, d, nb, 1 << 30, 1 << 24)
    path, _ = incoming_paths(rng, level, d, groups)
    taken, _ = split_both(dev, hist, gcnt, level, d, nb, cuts, 1.0, 0.0, 0.0, C.masks_of(groups), path, missing=missing)
    assert np.all(taken[1] >= 0)  # there are candidates
    ref, _ = split_both(dev, hist, gcnt, level, d, nb, cuts, 1.0, 0.0, 1e30, C.masks_of(groups), path, missing=missing)
    assert np.all(ref[1] == -1)


def test_launcher_refusals(dev):
    """The binding's host guards raise before anything is launched: the outputs keep their fill."""
    m = native()
    z = torch.zeros(4096, dtype=torch.int64, device=dev)
    out = torch.full((64,), -7, dtype=torch.int32, device=dev)
    pth = torch.full((64,), SENT, dtype=torch.int32, device=dev)

    def split(d, groups, path):
        m.gbdt_split(ptr(z), ptr(z), 0, d, ptr(z), ptr(z), 1.0, 1.0, 1.0, 1.0, 0.0, ptr(out), ptr(out), ptr(z), ptr(z),
                     ptr(z), ptr(z), stream_of(z), 0, False, 0, 0, 0, 0, groups, path)

    for args, msg in (((4, [1] * 33, ptr(pth)), "at most 32"), ((4, [3, 16], ptr(pth)), "at or above d"),
                      ((30, [1 << 30], ptr(pth)), "at or above d"), ((4, [3, 0], ptr(pth)), "empty interaction group"),
                      ((4, [3], 0), "need the path array"), ((4, [], ptr(pth)), "needs interaction groups")):
        with pytest.raises(RuntimeError, match=msg):
            split(*args)
    with pytest.raises(RuntimeError, match="need the path array"):
        m.gbdt_split(ptr(z), ptr(z), 0, 4, ptr(z), ptr(z), 1.0, 1.0, 1.0, 1.0, 0.0, ptr(out), ptr(out), ptr(z), ptr(z),
                     ptr(z), ptr(z), stream_of(z), inter_groups=[3])
    torch.cuda.synchronize()
    assert bool((out == -7).all()) and bool((pth == SENT).all()) and bool((z == 0).all())


# ---- whole fits ------------------------------------------------------------------------------------
GROUPS = C.GROUPS
GROUPS30 = ((0, 1, 29), (2, 3), (2, 5, 6, 7), (4, 10, 11), (12, 13, 14, 15, 16))
FIT = dict(n_estimators=6, max_bin=32, learning_rate=0.4)
SHAPES = {"d6_depth3": (2000, 6, 3, GROUPS), "d6_depth7": (2500, 6, 7, GROUPS), "d30_depth3": (3000, 30, 3, GROUPS30),
          "d30_depth7": (4000, 30, 7, GROUPS30)}


def fit_pair(dev, X, y, p, **kw):
    """(device fit, CPU oracle fit) of the same call; tensors in ``kw`` move with the rows."""
    on = lambda d: {k: (v.to(d) if isinstance(v, torch.Tensor) else                      # noqa: E731
                        tuple(t.to(d) for t in v) if isinstance(v, tuple) and isinstance(v[0], torch.Tensor) else v)
                    for k, v in kw.items()}
    Xt, yt = torch.from_numpy(X), torch.from_numpy(y)
    return gb.fit(Xt.to(dev), yt.to(dev), p, **on(dev)), gb.fit(Xt, yt, p, **on("cpu"))


@pytest.mark.parametrize("shape", list(SHAPES))
def test_fit_equals_oracle_and_keeps_paths_inside_groups(dev, shape):
    n, d, depth, groups = SHAPES[shape]
    X, y = C.fixture_data(n, d, seed=7)
    p = gb.GBDTParams(max_depth=depth, interaction_constraints=groups, **FIT)
    got, ref = fit_pair(dev, X, y, p)
    assert C.same_trees(got, ref)
    assert got.params["interaction_constraints"] == [list(g) for g in groups]
    assert C.path_violations(got, groups) == 0 and C.n_mixed_paths(got) > 0
    free, free_ref = fit_pair(dev, X, y, gb.GBDTParams(max_depth=depth, **FIT))
    assert C.same_trees(free, free_ref) and not C.same_trees(free, got)
    assert C.path_violations(free, groups) > 0  # the data can show a failure
    Xd, yd = torch.from_numpy(X).to(dev), torch.from_numpy(y).to(dev)
    assert C.same_trees(gb.fit(Xd, yd, p), got)  # two fits are bitwise equal
    graph = gb.fit(Xd, yd, p, use_graph=True)
    assert C.same_trees(graph, got)  # the recorded round replays the group words and the static path pointer
    if shape == "d6_depth3":
        for form in ([], [[]]):  # no group: the default fit bit for bit
            zero = gb.fit(Xd, yd, gb.GBDTParams(max_depth=depth, interaction_constraints=form, **FIT))
            assert C.same_trees(zero, free) and zero.to_dict() == free.to_dict()


COMPOSED_SHAPES = ("d6_depth7", "d30_depth3", "d30_depth7")


def shape_data(shape):
    """(rows, rows with NaN in features 0 and 2, labels, weights, depth, groups, monotone signs) of a
    SHAPES entry; the signs follow the label's own direction on features 0 and 2."""
    n, d, depth, groups = SHAPES[shape]
    X, y = C.fixture_data(n, d, seed=7)
    rng = np.random.default_rng(11)
    Xn = X.copy()
    Xn[rng.random(n) < 0.1, 0] = np.nan
    Xn[rng.random(n) < 0.1, 2] = np.nan
    w = rng.uniform(0.25, 2.0, n).astype(np.float32)
    return X, Xn, y, w, depth, groups, (1, 0, 1) + (0,) * (d - 3)


@pytest.mark.parametrize("shape", ["d6_depth7", "d30_depth7"])
def test_classifier_on_device(dev, shape):
    from fraud_detection_amd.models.gbdt import GBDTClassifier

    X, _, y, _, depth, groups, _ = shape_data(shape)
    kw = dict(max_depth=depth, **FIT)
    Xd, yd = torch.from_numpy(X).to(dev), torch.from_numpy(y).to(dev)
    assert C.path_violations(GBDTClassifier(**kw).fit(Xd, yd).ensemble, groups) > 0
    clf = GBDTClassifier(interaction_constraints=str([list(g) for g in groups]), **kw).fit(Xd, yd)
    assert C.path_violations(clf.ensemble, groups) == 0 and C.n_mixed_paths(clf.ensemble) > 0


@pytest.mark.parametrize("shape", COMPOSED_SHAPES)
@pytest.mark.parametrize("what", list(C.COMPOSE))
def test_fit_composes_on_device(dev, what, shape):
    """Every composition at the whole-fit shapes: 30 features, depth 7 (levels 0 .. 6 of the
    MISS / MONO / fmask instantiations with the interaction tail), against the oracle bit for bit."""
    X, Xn, y, w, depth, groups, signs = shape_data(shape)
    kw = {**FIT, "max_depth": depth, **C.COMPOSE[what]}
    if "monotone_constraints" in kw:
        kw["monotone_constraints"] = signs
    rows = Xn if kw.get("missing_policy") == "learn" else X
    fit_kw = {"sample_weight": torch.from_numpy(w)} if what in ("weights", "all") else {}
    got, ref = fit_pair(dev, rows, y, gb.GBDTParams(interaction_constraints=groups, **kw), **fit_kw)
    assert C.same_trees(got, ref)
    if kw.get("missing_policy") == "learn":
        assert np.array_equal(got.default_left, ref.default_left)
    assert C.path_violations(got, groups) == 0 and C.n_mixed_paths(got) > 0
    free, free_ref = fit_pair(dev, rows, y, gb.GBDTParams(**kw), **fit_kw)
    assert C.same_trees(free, free_ref) and not C.same_trees(free, got)
    assert C.path_violations(free, groups) > 0
    if what == "bynode":
        assert C.empty_eligible_nodes(got, groups, kw["seed"], kw["colsample_bynode"]) > 0
    if "monotone_constraints" in kw:
        v = G.C.violations(G.dev_predict(got, dev), X, got.cuts, got.nbins, signs)
        assert all(n == 0 for n, _ in v.values()), v


@pytest.mark.parametrize("shape", COMPOSED_SHAPES)
def test_early_stopping_and_row_hole_on_device(dev, shape):
    X, _, y, _, depth, groups, _ = shape_data(shape)
    n, cut = len(y), 3 * len(y) // 4
    Xt, yt = torch.from_numpy(X), torch.from_numpy(y)
    p = gb.GBDTParams(interaction_constraints=groups, max_depth=depth, max_bin=32, n_estimators=40, learning_rate=0.8)
    (ens, rec), (ref, rec_c) = fit_pair(dev, X[:cut], y[:cut], p, eval_set=(Xt[cut:], yt[cut:]), early_stopping_rounds=3)
    assert rec.stopped and ens.n_trees == rec.best_iteration + 1 < 40
    assert rec.best_iteration == rec_c.best_iteration and C.same_trees(ens, ref)
    assert C.path_violations(ens, groups) == 0
    q = gb.GBDTParams(interaction_constraints=groups, max_depth=depth, **FIT)
    cuts = gb.quantile_cuts(Xt, 32)
    bins = gb.bin_rows(Xt, cuts[0], cuts[1])
    hole_at = (n // 5, n // 4)  # a fold's block: rows [n/5, n/5 + n/4) are left out
    hole = gb.fit_binned(bins.to(dev), yt.to(dev), cuts, q, hole=hole_at)
    assert C.same_trees(hole, gb.fit_binned(bins, yt, cuts, q, hole=hole_at))
    keep = np.r_[0:hole_at[0], hole_at[0] + hole_at[1]:n]
    assert C.same_trees(hole, gb.fit_binned(bins[keep].contiguous().to(dev), yt[keep].contiguous().to(dev), cuts, q))
    assert C.path_violations(hole, groups) == 0 and C.n_mixed_paths(hole) > 0


@pytest.mark.parametrize("shape", COMPOSED_SHAPES)
def test_checkpoint_resume_on_device(dev, shape, tmp_path):
    """A constrained device fit interrupted after 4 of 6 rounds and resumed equals the uninterrupted
    device fit and the oracle bit for bit, margins included; the device checkpoint also resumes on
    the CPU path, and an unconstrained fit does not pick it up (the groups are in the signature)."""
    from fraud_detection_amd.utils.checkpoint import CheckpointManager

    X, _, y, _, depth, groups, _ = shape_data(shape)
    Xt, yt = torch.from_numpy(X), torch.from_numpy(y)
    Xd, yd = Xt.to(dev), yt.to(dev)
    kw = dict(max_depth=depth, interaction_constraints=groups, **FIT)
    p = gb.GBDTParams(**kw)
    cuts = gb.quantile_cuts(Xt, 32)
    ref, rm = gb.fit(Xt, yt, p, cuts=cuts, return_margin=True)
    whole, wm = gb.fit(Xd, yd, p, cuts=cuts, return_margin=True)
    mgr = CheckpointManager(str(tmp_path), prefix="g")
    gb.fit(Xd, yd, gb.GBDTParams(**{**kw, "n_estimators": 4}), cuts=cuts, checkpoint=mgr, checkpoint_every=2)
    saved = []
    save = mgr.save
    mgr.save = lambda step, *a, **k: (saved.append(step), save(step, *a, **k))[1]
    ens, m = gb.fit(Xd, yd, p, cuts=cuts, checkpoint=mgr, checkpoint_every=2, return_margin=True)
    assert saved == [6]  # rounds 1 .. 4 came from the checkpoint
    assert C.same_trees(ens, whole) and C.same_trees(ens, ref)
    assert torch.equal(m, wm) and np.array_equal(m.cpu().numpy().view(np.uint32), rm.numpy().view(np.uint32))
    assert C.path_violations(ens, groups) == 0 and C.n_mixed_paths(ens) > 0
    mgr.save = save
    assert C.same_trees(gb.fit(Xt, yt, p, cuts=cuts, checkpoint=mgr, checkpoint_every=2), ref)
    free = gb.GBDTParams(**{**kw, "interaction_constraints": None})
    other = gb.fit(Xd, yd, free, cuts=cuts, checkpoint=mgr, checkpoint_every=6)
    assert C.same_trees(other, gb.fit(Xd, yd, free, cuts=cuts)) and not C.same_trees(other, ens)


def test_cv_job_and_pipeline_take_constraints(dev):
    from fraud_detection_amd.data.synthetic import separable
    from fraud_detection_amd.models.gbdt import GBDTPipeline
    from fraud_detection_amd.models.gbdt_cv import DeviceGBDTCV
    from fraud_detection_amd.models.pipeline import TrainConfig

    X, y = separable(6000, fraud_rate=0.05, seed=21, device=dev, n_features=8)
    groups = ((1, 2), (3, 4), (0, 5))
    kw = dict(n_estimators=6, max_depth=3, max_bin=32, learning_rate=0.5)
    p = gb.GBDTParams(interaction_constraints="[[2, 1], [3, 4], [5, 0]]", **kw)
    cv = DeviceGBDTCV(TrainConfig(), p, n_folds=3).run(X, y)
    pipe = GBDTPipeline(TrainConfig(), p).fit(X, y)
    for res in (cv.final, pipe):
        ens = res.ensemble
        assert ens.params["interaction_constraints"] == [list(g) for g in groups]
        assert C.path_violations(ens, groups) == 0 and C.n_mixed_paths(ens) > 0
    assert len(cv.fold_aucs) == 3
    free = GBDTPipeline(TrainConfig(), gb.GBDTParams(**kw)).fit(X, y).ensemble
    assert C.path_violations(free, groups) > 0 and not C.same_trees(free, pipe.ensemble)
