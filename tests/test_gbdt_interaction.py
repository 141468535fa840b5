"""GBDT interaction constraints (xgboost's interaction_constraints), CPU side: the allowed-set
function against an independent set-based form of the incremental rule, the numpy oracle
(ops/reference_gbdt.py) against a row-level brute force, the structural property of whole fits, the
parameter forms, serialisation, checkpoints and the train entry point's option."""
from __future__ import annotations

import json
import os
import pickle

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from fraud_detection_amd.models.gbdt import GBDTClassifier
from fraud_detection_amd.ops import gbdt as gb
from fraud_detection_amd.ops import reference_gbdt as R

TREE_KEYS = ("feat", "bin", "thr", "gain", "leaf")
GROUPS = ((0, 1), (2, 3))  # features 4 and 5 are in no group
FIT_KW = dict(n_estimators=12, max_depth=3, max_bin=16, learning_rate=0.3)


def same_trees(a, b, keys=TREE_KEYS):
    return all(getattr(a, k).tobytes() == getattr(b, k).tobytes() for k in keys)


def masks_of(groups):
    return [sum(1 << f for f in g) for g in groups]


def fixture_data(n=600, d=6, seed=5):
    """The label depends on the product of features 0 and 2 -- different groups of GROUPS -- on both
    features alone and on the unlisted feature 4, so an unconstrained tree splits on 0 and on 2 along
    one path."""
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, d)).astype(np.float32)
    z = 1.5 * X[:, 0] + 1.5 * X[:, 2] + 2.0 * X[:, 0] * X[:, 2] + 0.8 * X[:, 4] - 0.5 * X[:, 1]
    y = (rng.random(n) < 1.0 / (1.0 + np.exp(-z))).astype(np.uint8)
    return X, y


# ---- the rule, as sets --------------------------------------------------------------------------------
def allowed_set(path: set, groups, d: int) -> set:
    """allowed = path | union of the groups that contain the whole path; every feature for no path."""
    if not path:
        return set(range(d))
    out = set(path)
    for g in groups:
        if path <= set(g):
            out |= set(g)
    return out


def path_violations(ens, groups) -> int:
    """Split nodes with a non-empty ancestor set P whose feature is outside P | union{g : P <= g}."""
    d = len(ens.nbins)
    bad = 0
    for feat in np.asarray(ens.feat):
        paths = {0: set()}
        for node in range(len(feat)):
            P = paths[node]
            f = int(feat[node])
            if f >= 0 and P and f not in allowed_set(P, groups, d):
                bad += 1
            paths[2 * node + 1] = paths[2 * node + 2] = (P | {f}) if f >= 0 else P
    return bad


def n_mixed_paths(ens) -> int:
    """Split nodes below at least one split ancestor (the nodes the property speaks about)."""
    n = 0
    for feat in np.asarray(ens.feat):
        below = {0: False}
        for node in range(len(feat)):
            n += int(below[node] and feat[node] >= 0)
            below[2 * node + 1] = below[2 * node + 2] = below[node] or feat[node] >= 0
    return n


class _Incremental:
    """xgboost's host constraint as it is kept per node: Reset gives the root every feature; a split
    of node p on feature f gives both children p's path plus f, plus every group that contains f and
    the whole of p's path.  Sets of ints only."""

    def __init__(self, groups, d):
        self.groups = [set(g) for g in groups]
        self.path = {0: set()}
        self.allowed = {0: set(range(d))}

    def split(self, node, f):
        path = self.path[node] | {f}
        allowed = set(path)
        for g in self.groups:
            if f in g and self.path[node] <= g:
                allowed |= g
        for c in (2 * node + 1, 2 * node + 2):
            self.path[c], self.allowed[c] = set(path), set(allowed)

    def pass_through(self, node):
        for c in (2 * node + 1, 2 * node + 2):
            self.path[c], self.allowed[c] = set(self.path[node]), set(self.allowed[node])


def random_groups(rng, d, n_groups):
    """Overlapping groups over [0, d) that leave some feature unlisted where d allows it and name
    feature d - 1 at least once."""
    pool = list(range(d)) if d < 3 else [f for f in range(d) if f != 1]  # feature 1 stays unlisted
    groups = []
    for _ in range(n_groups):
        k = int(rng.integers(1, max(2, min(len(pool), 6) + 1)))
        groups.append(tuple(sorted(rng.choice(pool, size=min(k, len(pool)), replace=False).tolist())))
    groups[0] = tuple(sorted(set(groups[0]) | {d - 1}))
    return groups


@pytest.mark.parametrize("n_groups", [1, 2, 32])
@pytest.mark.parametrize("d", [1, 5, 30])
def test_allowed_equals_incremental_sets(d, n_groups):
    rng = np.random.default_rng(1000 * d + n_groups)
    narrowed = opened = 0
    for rep in range(40):
        groups = random_groups(rng, d, n_groups)
        masks = masks_of(groups)
        inc = _Incremental(groups, d)
        assert R.interaction_allowed(0, masks, d) == (1 << d) - 1
        node = 0
        for depth in range(6):
            # the next split feature: mostly an allowed one (a real tree), sometimes any (the function
            # is defined for every path), sometimes none (a pass-through)
            r = rng.random()
            if r < 0.15:
                inc.pass_through(node)
            else:
                pick = sorted(inc.allowed[node]) if r < 0.8 else list(range(d))
                inc.split(node, int(rng.choice(pick)))
            node = 2 * node + 1 + int(rng.integers(0, 2))
            path = inc.path[node]
            got = R.interaction_allowed(sum(1 << f for f in path), masks, d)
            want = inc.allowed[node] if path else set(range(d))
            assert got == sum(1 << f for f in want), (groups, path, got, want)
            assert want == allowed_set(path, groups, d)
            narrowed += int(bool(path) and want != set(range(d)))
            opened += int(want > path)
    assert narrowed > 0 or d == 1
    assert opened > 0 or d == 1


def test_allowed_named_cases():
    g = masks_of([(0, 1, 2), (2, 3), (29,)])
    A = lambda *p: R.interaction_allowed(sum(1 << f for f in p), g, 30)  # noqa: E731
    assert A() == (1 << 30) - 1                      # the root: every feature
    assert A(2) == 0b1111                            # in two groups: both open
    assert A(2, 3) == 0b1100                         # narrowed to one of them
    assert A(0, 2) == 0b0111
    assert A(0, 3) == 0b1001                         # inside no group: the path itself only
    assert A(5) == 1 << 5                            # an unlisted feature is followed by itself only
    assert A(29) == 1 << 29
    assert R.interaction_allowed(0b11, [0b11], 2) == 0b11  # one group of everything allows everything
    assert R.interaction_allowed(0b01, [], 2) == 0b01


# ---- parameter forms --------------------------------------------------------------------------------------
def test_forms_normalise():
    want = ((0, 2), (1, 3, 4))
    for form in (want, [[0, 2], [1, 3, 4]], [[2, 0], (4, 1, 3)], "[[0, 2], [1, 3, 4]]", " [[2,0],[4,3,1]] ",
                 [np.array([0, 2]), np.array([1, 3, 4], np.int32)], np.array([[0, 2], [1, 3]]).tolist() + [[1, 3, 4]],
                 [[0, 2], [], [1, 3, 4], [2, 0]]):
        got = gb.normalize_interaction(form)
        if len(got) == 3:
            assert got == ((0, 2), (1, 3), (1, 3, 4)), form
        else:
            assert got == want, form
        assert gb.GBDTParams(interaction_constraints=form).validate().interaction_constraints == got
    for empty in (None, [], (), [[]], [[], ()], "[]", "[[]]"):
        assert gb.normalize_interaction(empty) is None, empty
        assert gb.GBDTParams(interaction_constraints=empty).validate().interaction_masks(4) is None
    p = gb.GBDTParams(interaction_constraints="[[0, 2], [1, 3, 4], [29]]").validate()
    assert p.interaction_masks(30) == [0b101, 0b11010, 1 << 29]
    assert GBDTClassifier(interaction_constraints=[[3, 1], [0]]).get_params()["interaction_constraints"] == ((1, 3), (0,))


@pytest.mark.parametrize("bad", [[[0, 1.0]], [[0, True]], [[-1, 2]], [[0, 1, 0]], "[[0, 1", "[[0, x]]", "[[0, 1.5]]",
                                 "[[0, true]]", "[[1, 1]]", 7, [0, 1], "[0, 1]", {0: [1]}, [["a"]], [[None]], "0,1;2"],
                         ids=lambda b: repr(b).replace(" ", ""))
def test_bad_values_raise(bad):
    with pytest.raises(ValueError, match="interaction_constraints"):
        gb.normalize_interaction(bad)
    with pytest.raises(ValueError, match="interaction_constraints"):
        gb.GBDTParams(interaction_constraints=bad).validate()
    with pytest.raises(ValueError, match="interaction_constraints"):
        GBDTClassifier(interaction_constraints=bad)


def test_out_of_range_and_too_many_groups_raise():
    X, y = fixture_data()
    for bad in ([[0, 6]], [[0, 1], [30]], "[[5, 6]]"):
        with pytest.raises(ValueError, match="out of range"):
            gb.fit(torch.from_numpy(X), torch.from_numpy(y), gb.GBDTParams(interaction_constraints=bad, **FIT_KW))
        with pytest.raises(ValueError, match="out of range"):
            GBDTClassifier(interaction_constraints=bad, device="cpu", **FIT_KW).fit(X, y)
    pairs = [(a, b) for a in range(9) for b in range(a + 1, 9)]
    assert gb.GBDTParams(interaction_constraints=pairs[:32]).validate().interaction_masks(9) == masks_of(pairs[:32])
    with pytest.raises(ValueError, match="at most 32"):
        gb.GBDTParams(interaction_constraints=pairs[:33]).validate().interaction_masks(9)
    # 33 listed, 32 distinct and non-empty: fine
    assert len(gb.GBDTParams(interaction_constraints=pairs[:32] + [[]] + [pairs[0]]).validate().interaction_masks(9)) == 32


# ---- the oracle against a brute force over the rows ---------------------------------------------------
def _brute_tree(bins, q, nbins, depth, lam, mcw, gamma, eta, ginv, hinv, groups, fmasks, missing):
    """No histograms, no cumsum and no bit masks: per node the eligible features as a set (the path's
    own and every group that holds the whole path, all of them for an empty path; then the column
    sample), per eligible feature and cut (and direction) the sums over the node's rows and the
    documented gain on Python floats.  Candidates are tried in tie order and replaced only by a
    strictly larger gain."""
    n, d = bins.shape[0], len(nbins)
    ni = (1 << depth) - 1
    feat, binv, dleft, gain = np.full(ni, -1), np.full(ni, 255), np.zeros(ni, np.uint8), np.zeros(ni)
    sums, rows_of, paths = {}, {0: np.arange(n)}, {0: frozenset()}
    g, h = q[:, 0].astype(np.int64), q[:, 1].astype(np.int64)
    empty_nodes = 0

    def term(Gq, Hq):
        G, H = float(Gq) * ginv, float(Hq) * hinv
        return G * G / (H + lam) if H + lam > 0.0 else 0.0

    for node in range(ni):
        rows = rows_of[node]
        Gq, Hq = int(g[rows].sum()), int(h[rows].sum())
        if node == 0:
            sums[0] = (Gq, Hq)
        eligible = allowed_set(set(paths[node]), groups, d)
        if fmasks is not None:
            eligible = {f for f in eligible if (int(fmasks[node]) >> f) & 1}
        empty_nodes += int(not eligible)
        root = term(Gq, Hq)
        best = (-np.inf, None)
        for f in range(d):
            if f not in eligible:
                continue
            v = bins[rows, f].astype(np.int64)
            miss = (v == 255) if missing else np.zeros(len(rows), bool)
            cands = [(-1, 1, miss)] if missing else []
            for b in range(int(nbins[f]) - 1):
                cands.append((b, 0, (v <= b) & ~miss))
                if missing:
                    cands.append((b, 1, (v <= b) | miss))
            for b, dl, left in cands:
                GLq, HLq = int(g[rows][left].sum()), int(h[rows][left].sum())
                if not (float(HLq) * hinv >= mcw and float(Hq - HLq) * hinv >= mcw):
                    continue
                gn = (term(GLq, HLq) + term(Gq - GLq, Hq - HLq)) - root
                if gn > best[0]:
                    best = (gn, (f, b, dl, left, GLq, HLq))
        lc, rc = 2 * node + 1, 2 * node + 2
        if best[1] is not None and best[0] > 1e-6 and not best[0] < gamma:
            f, b, dl, left, GLq, HLq = best[1]
            feat[node], binv[node], dleft[node], gain[node] = f, b, dl, best[0]
            rows_of[lc], rows_of[rc] = rows[left], rows[~left]
            sums[lc], sums[rc] = (GLq, HLq), (Gq - GLq, Hq - HLq)
            paths[lc] = paths[rc] = paths[node] | {f}
        else:
            rows_of[lc], rows_of[rc] = rows, rows[:0]
            sums[lc], sums[rc] = (Gq, Hq), (0, 0)
            paths[lc] = paths[rc] = paths[node]
    leaf = np.zeros(1 << depth, np.float32)
    where = np.zeros(n, np.int64)
    for i in range(1 << depth):
        G, H = float(sums[ni + i][0]) * ginv, float(sums[ni + i][1]) * hinv
        leaf[i] = np.float32(eta * (0.0 if (H < mcw or H <= 0.0) else -G / (H + lam)))
        where[rows_of[ni + i]] = i
    return feat, binv, dleft, gain, leaf, where, empty_nodes


BRUTE_GROUPS = {"two": ((0, 1), (2, 3)), "overlap": ((0, 1, 2), (2, 3)), "single": ((1, 3),), "all": ((0, 1, 2, 3, 4),),
                "chain": ((0, 1), (1, 2), (2, 3), (3, 4))}


@pytest.mark.parametrize("missing", [False, True], ids=["plain", "missing"])
@pytest.mark.parametrize("reg", [(0.0, 0.0, 0.0), (1.0, 1.0, 0.0), (1.0, 0.0, 0.5)], ids=lambda r: "l%g_w%g_g%g" % r)
@pytest.mark.parametrize("colsample", [False, True], ids=["allcols", "bynode"])
@pytest.mark.parametrize("groups", list(BRUTE_GROUPS))
def test_build_tree_matches_row_brute_force(groups, colsample, reg, missing):
    lam, mcw, gamma = reg
    name, groups = groups, BRUTE_GROUPS[groups]
    changed = splits = empties = 0
    for seed in (0, 1, 2):
        rng = np.random.default_rng(seed)
        n, d, depth = 90, 5, 4
        X = rng.integers(-3, 4, size=(n, d)).astype(np.float32)  # few distinct values: ties between candidates
        if missing:
            X[rng.random(n) < 0.3, 0] = np.nan
            X[rng.random(n) < 0.1, 2] = np.nan
        cuts, nbins = R.quantile_cuts(X, 6, missing=missing)
        bins = R.bin_rows(X, cuts, nbins, missing=missing)
        gs, hs = R.grad_scales(1.0)
        q = np.stack([rng.integers(-(1 << 14), (1 << 14) + 1, n), rng.integers(0, (1 << 14) + 1, n)], 1).astype(np.int32)
        q[rng.random(n) < 0.2, 1] = 0
        fmasks = R.feature_masks(7, seed, d, depth, bynode=0.4) if colsample else None
        tr, node = R.build_tree(bins, q, cuts, nbins, depth, lam, mcw, gamma, 0.3, gs, hs, fmasks=fmasks, missing=missing,
                                interaction=masks_of(groups))
        feat, binv, dleft, gain, leaf, where, empty = _brute_tree(bins[:, :d], q, nbins, depth, lam, mcw, gamma, 0.3,
                                                                  1 / gs, 1 / hs, groups, fmasks, missing)
        assert np.array_equal(tr.feat, feat) and np.array_equal(tr.bin, binv), (tr.feat, feat, tr.bin, binv)
        if missing:
            assert np.array_equal(tr.default_left, dleft)
        assert tr.gain.tobytes() == gain.tobytes()
        assert tr.leaf.tobytes() == leaf.tobytes()
        assert np.array_equal(node, where)
        free, _ = R.build_tree(bins, q, cuts, nbins, depth, lam, mcw, gamma, 0.3, gs, hs, fmasks=fmasks, missing=missing)
        changed += int(not same_trees(tr, free, ("feat", "bin", "leaf")))
        splits += int((tr.feat >= 0).sum())
        empties += empty
    assert splits > 0
    assert (changed > 0) == (name != "all")  # one group of everything is the unconstrained tree
    if colsample and name in ("two", "single", "chain"):
        assert empties > 0  # the drawn sample and the allowed set do not meet somewhere: no split there


# ---- whole fits --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fits():
    X, y = fixture_data()
    Xt, yt = torch.from_numpy(X), torch.from_numpy(y)
    free = gb.fit(Xt, yt, gb.GBDTParams(**FIT_KW))
    inter = gb.fit(Xt, yt, gb.GBDTParams(interaction_constraints=GROUPS, **FIT_KW))
    return X, y, free, inter


def test_unconstrained_fit_violates(fits):
    """The data can show a failure: without constraints features of different groups share a path."""
    _, _, free, _ = fits
    assert path_violations(free, GROUPS) > 0
    assert "interaction_constraints" not in free.params


def test_constrained_fit_keeps_paths_inside_groups(fits):
    _, _, free, inter = fits
    assert path_violations(free, GROUPS) > 0  # otherwise the next line shows nothing
    assert path_violations(inter, GROUPS) == 0
    assert n_mixed_paths(inter) > 0 and not same_trees(inter, free)
    assert inter.params["interaction_constraints"] == [list(g) for g in GROUPS]
    # every feature the label depends on is still split on, the unlisted one included
    assert all(int((inter.feat == f).sum()) > 0 for f in (0, 2, 4))


def test_classifier_takes_the_constraints():
    """Fails where the estimator drops the argument: the fit is then the unconstrained one, which
    violates the property.  Uses the estimator alone, nothing of the ops layer's new interface."""
    X, y = fixture_data()
    assert path_violations(GBDTClassifier(device="cpu", **FIT_KW).fit(X, y).ensemble, GROUPS) > 0
    clf = GBDTClassifier(interaction_constraints=[list(g) for g in GROUPS], device="cpu", **FIT_KW).fit(X, y)
    assert path_violations(clf.ensemble, GROUPS) == 0
    assert n_mixed_paths(clf.ensemble) > 0


def test_classifier_equals_the_ops_fit(fits):
    X, y, _, inter = fits
    clf = GBDTClassifier(interaction_constraints=[list(g) for g in GROUPS], device="cpu", **FIT_KW).fit(X, y)
    assert clf.get_params()["interaction_constraints"] == GROUPS
    assert same_trees(clf.ensemble, inter)


def test_empty_forms_equal_default_bit_for_bit(fits):
    X, y, free, inter = fits
    Xt, yt = torch.from_numpy(X), torch.from_numpy(y)
    for form in (None, [], [[]], "[]"):
        zero = gb.fit(Xt, yt, gb.GBDTParams(interaction_constraints=form, **FIT_KW))
        assert same_trees(zero, free)
        assert json.dumps(zero.to_dict(), sort_keys=True) == json.dumps(free.to_dict(), sort_keys=True)
    every = gb.fit(Xt, yt, gb.GBDTParams(interaction_constraints=[list(range(6))], **FIT_KW))
    assert same_trees(every, free) and every.params["interaction_constraints"] == [list(range(6))]
    for form in ("[[0, 1], [2, 3]]", [[1, 0], [3, 2], [0, 1]]):
        assert same_trees(gb.fit(Xt, yt, gb.GBDTParams(interaction_constraints=form, **FIT_KW)), inter)


def test_json_and_pickle_round_trip(tmp_path, fits):
    X, y, free, inter = fits
    clf = GBDTClassifier(interaction_constraints="[[0, 1], [2, 3]]", device="cpu", **FIT_KW).fit(X, y)
    want = clf.predict_margin(X)
    path = str(tmp_path / "m.json")
    clf.save_model(path)
    with open(path) as f:
        o = json.load(f)
    assert o["params"]["interaction_constraints"] == [[0, 1], [2, 3]]
    assert set(o) == set(free.to_dict()) | {"feature_names"}  # a constrained tree is an ordinary tree: no new field
    back = GBDTClassifier.load_model(path, device="cpu")
    assert back.get_params()["interaction_constraints"] == GROUPS
    assert same_trees(back.ensemble, inter) and np.array_equal(back.predict_margin(X), want)
    again = pickle.loads(pickle.dumps(clf))
    assert again.get_params()["interaction_constraints"] == GROUPS
    assert np.array_equal(again.predict_margin(X), want)
    assert same_trees(again.fit(X, y).ensemble, inter)  # the unpickled estimator refits constrained
    # an unconstrained model serialises as it always did
    plain = GBDTClassifier(device="cpu", **FIT_KW).fit(X, y)
    assert "interaction_constraints" not in plain.ensemble.to_dict()["params"]
    assert plain.get_params()["interaction_constraints"] is None
    plain.save_model(path)
    free_path = str(tmp_path / "f.json")
    GBDTClassifier(interaction_constraints=[[]], device="cpu", **FIT_KW).fit(X, y).save_model(free_path)
    with open(path, "rb") as a, open(free_path, "rb") as b:
        assert a.read() == b.read()


# ---- checkpoints -----------------------------------------------------------------------------------------
class _Recorder:
    """A checkpoint manager's interface that records the signatures a fit asks for."""

    def __init__(self):
        self.sigs = []

    def latest(self, sig):
        self.sigs.append(sig)
        return None

    def save(self, step, tensors, meta):
        self.sigs.append(meta["signature"])


def test_checkpoint_signature_unchanged_when_unconstrained():
    """A checkpoint written before the field existed names no such parameter: it still resumes."""
    from fraud_detection_amd.utils.checkpoint import config_signature

    X, y = fixture_data()
    Xt, yt = torch.from_numpy(X), torch.from_numpy(y)
    kw = dict(n_estimators=2, max_depth=2, max_bin=8)
    cuts = gb.quantile_cuts(Xt, 8)

    def sig_of(**extra):
        rec = _Recorder()
        gb.fit(Xt, yt, gb.GBDTParams(**kw, **extra), cuts=cuts, checkpoint=rec, checkpoint_every=2)
        assert len(set(rec.sigs)) == 1
        return rec.sigs[0]

    p = gb.GBDTParams(**kw)
    old = {k: v for k, v in p.__dict__.items()
           if k not in ("n_estimators", "monotone_constraints", "interaction_constraints")
           and not (k in p.SAMPLING_DEFAULTS and v == p.SAMPLING_DEFAULTS[k])}
    want = config_signature(params=old, spw=1.0, cuts=cuts[0], nbins=cuts[1], n=600, d=6)
    assert sig_of() == want
    assert sig_of(interaction_constraints=[]) == want == sig_of(interaction_constraints=[[]])
    inter = sig_of(interaction_constraints=GROUPS)
    assert inter != want
    assert sig_of(interaction_constraints="[[1, 0], [3, 2]]") == inter
    assert sig_of(interaction_constraints=[[0, 1], [2, 3, 4]]) != inter


def test_checkpoint_resume_equals_uninterrupted(tmp_path):
    from fraud_detection_amd.utils.checkpoint import CheckpointManager

    X, y = fixture_data()
    Xt, yt = torch.from_numpy(X), torch.from_numpy(y)
    kw = dict(max_depth=3, max_bin=16, learning_rate=0.3, interaction_constraints=GROUPS)
    full = gb.fit(Xt, yt, gb.GBDTParams(n_estimators=6, **kw))
    mgr = CheckpointManager(str(tmp_path), prefix="g")
    gb.fit(Xt, yt, gb.GBDTParams(n_estimators=3, **kw), checkpoint=mgr, checkpoint_every=3)
    saved = []
    save = mgr.save
    mgr.save = lambda step, *a, **k: (saved.append(step), save(step, *a, **k))[1]
    res = gb.fit(Xt, yt, gb.GBDTParams(n_estimators=6, **kw), checkpoint=mgr, checkpoint_every=1)
    assert saved == [4, 5, 6]
    assert same_trees(res, full) and path_violations(res, GROUPS) == 0
    # the groups are part of the signature: an unconstrained fit does not pick these rounds up
    free_kw = {**kw, "interaction_constraints": None}
    other = gb.fit(Xt, yt, gb.GBDTParams(n_estimators=6, **free_kw), checkpoint=mgr, checkpoint_every=6)
    assert same_trees(other, gb.fit(Xt, yt, gb.GBDTParams(n_estimators=6, **free_kw)))
    assert not same_trees(other, full)


# ---- composition on the CPU path ---------------------------------------------------------------------------
def nan_data():
    X, y = fixture_data()
    rng = np.random.default_rng(11)
    Xn = X.copy()
    Xn[rng.random(600) < 0.1, 0] = np.nan
    Xn[rng.random(600) < 0.1, 2] = np.nan
    return X, Xn, y, rng.uniform(0.25, 2.0, 600).astype(np.float32)


COMPOSE = {"bynode": dict(colsample_bynode=0.34, seed=3), "learn": dict(missing_policy="learn"),
           "monotone": dict(monotone_constraints=(1, 0, 1, 0, 0, 0)), "subsample": dict(subsample=0.7, seed=9),
           "weights": {}, "all": dict(colsample_bynode=0.5, subsample=0.8, seed=3, missing_policy="learn",
                                      monotone_constraints=(1, 0, 1, 0, 0, 0))}


def empty_eligible_nodes(ens, groups, seed, bynode) -> int:
    """Heap nodes of a colsample_bynode fit whose drawn features all lie outside the allowed set."""
    d, D = len(ens.nbins), ens.depth
    n = 0
    for t, feat in enumerate(np.asarray(ens.feat)):
        fm = R.feature_masks(seed, t, d, D, bynode=bynode)
        paths = {0: set()}
        for node in range(len(feat)):
            ok = {f for f in allowed_set(paths[node], groups, d) if (int(fm[node]) >> f) & 1}
            if not ok:
                n += 1
                assert feat[node] == -1
            elif feat[node] >= 0:
                assert int(feat[node]) in ok
            paths[2 * node + 1] = paths[2 * node + 2] = paths[node] | ({int(feat[node])} if feat[node] >= 0 else set())
    return n


@pytest.mark.parametrize("what", list(COMPOSE))
def test_composes_on_the_cpu_path(what):
    X, Xn, y, w = nan_data()
    kw = {**FIT_KW, **COMPOSE[what]}
    rows = Xn if kw.get("missing_policy") == "learn" else X
    fit_kw = {"sample_weight": torch.from_numpy(w)} if what in ("weights", "all") else {}
    Xt, yt = torch.from_numpy(rows), torch.from_numpy(y)
    free = gb.fit(Xt, yt, gb.GBDTParams(**kw), **fit_kw)
    inter = gb.fit(Xt, yt, gb.GBDTParams(interaction_constraints=GROUPS, **kw), **fit_kw)
    assert path_violations(inter, GROUPS) == 0 and n_mixed_paths(inter) > 0
    assert path_violations(free, GROUPS) > 0 and not same_trees(free, inter)
    if "colsample_bynode" in kw:
        n_empty = empty_eligible_nodes(inter, GROUPS, kw["seed"], kw["colsample_bynode"])
        assert what != "bynode" or n_empty > 0
    if "monotone_constraints" in kw:
        from test_gbdt_monotone import ens_predict, violations

        v = violations(ens_predict(inter), X, inter.cuts, inter.nbins, kw["monotone_constraints"])
        assert all(n == 0 for n, _ in v.values()), v


def test_composes_with_early_stopping_and_row_hole():
    X, Xn, y, w = nan_data()
    Xt, yt = torch.from_numpy(X), torch.from_numpy(y)
    p = gb.GBDTParams(interaction_constraints=GROUPS, **{**FIT_KW, "n_estimators": 40, "learning_rate": 0.8})
    ens, rec = gb.fit(Xt[:450], yt[:450], p, eval_set=(Xt[450:], yt[450:]), early_stopping_rounds=3)
    assert rec.stopped and ens.n_trees == rec.best_iteration + 1 < 40
    assert path_violations(ens, GROUPS) == 0
    full = gb.fit(Xt[:450], yt[:450], p)
    assert all(getattr(ens, k).tobytes() == getattr(full, k)[: ens.n_trees].tobytes() for k in TREE_KEYS)
    # a fold around a row hole = the fit on the kept rows
    q = gb.GBDTParams(interaction_constraints=GROUPS, **FIT_KW)
    cuts = gb.quantile_cuts(Xt, 16)
    bins = gb.bin_rows(Xt, cuts[0], cuts[1])
    hole = gb.fit_binned(bins, yt, cuts, q, hole=(100, 150))
    keep = np.r_[0:100, 250:600]
    assert same_trees(hole, gb.fit_binned(bins[keep].contiguous(), yt[keep].contiguous(), cuts, q))
    assert path_violations(hole, GROUPS) == 0 and n_mixed_paths(hole) > 0


# ---- data parallelism ------------------------------------------------------------------------------------
DP_KW = dict(n_estimators=4, max_depth=3, max_bin=16, learning_rate=0.3, interaction_constraints=GROUPS)


def _dp_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    from fraud_detection_amd.parallel.comm import Communicator

    comm = Communicator(backend="gloo")
    X, y = fixture_data()
    sh = slice(0, 301) if rank == 0 else slice(301, 600)
    ens = gb.fit(torch.from_numpy(X[sh].copy()), torch.from_numpy(y[sh].copy()), gb.GBDTParams(**DP_KW), comm=comm)
    np.savez(os.path.join(out_dir, f"m{rank}.npz"), **{k: getattr(ens, k) for k in TREE_KEYS}, cuts=ens.cuts)
    comm.close()


def test_dp_equals_single_process(tmp_path):
    """The histograms are all-reduced before the scan: every rank walks the same paths."""
    from test_distributed import _free_port

    mp.start_processes(_dp_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, start_method="spawn")
    X, y = fixture_data()
    ref = gb.fit(torch.from_numpy(X), torch.from_numpy(y), gb.GBDTParams(**DP_KW))
    assert not same_trees(ref, gb.fit(torch.from_numpy(X), torch.from_numpy(y),
                                      gb.GBDTParams(**{**DP_KW, "interaction_constraints": None})))
    for r in range(2):
        o = np.load(os.path.join(tmp_path, f"m{r}.npz"))
        assert np.array_equal(o["cuts"], ref.cuts)
        assert all(o[k].tobytes() == getattr(ref, k).tobytes() for k in TREE_KEYS)


# ---- the train entry point -------------------------------------------------------------------------------
def test_train_entry_point_resolves_names():
    from fraud_detection_amd.train import parse_gbdt_interaction

    cols = ["Time", "V1", "V14", "Amount"]
    assert parse_gbdt_interaction("Amount,Time;V14,V1", cols) == [[3, 0], [2, 1]]
    assert parse_gbdt_interaction(" Amount , Time ; V14 ", cols) == [[3, 0], [2]]
    assert parse_gbdt_interaction("Amount,Time;Amount,V14", cols) == [[3, 0], [3, 2]]  # groups may overlap
    assert parse_gbdt_interaction(None, cols) is None and parse_gbdt_interaction("  ", cols) is None
    for bad in ("Amonut,Time", "Amount,Amount", "Amount,;V1", "Amount;;V1", ";"):
        with pytest.raises(ValueError, match="gbdt-interaction"):
            parse_gbdt_interaction(bad, cols)


def test_train_entry_point_takes_constraints(tmp_path, monkeypatch):
    from fraud_detection_amd import train
    from fraud_detection_amd.config import Settings
    from fraud_detection_amd.data.synthetic import reference_frame
    import fraud_detection_amd.models.gbdt as mg

    df = reference_frame(3000, seed=5)
    csv = tmp_path / "cc.csv"
    df.to_csv(csv, index=False)
    monkeypatch.setenv("DATA_CSV", str(csv))
    monkeypatch.setenv("MLFLOW_TRACKING_URI", str(tmp_path / "mlruns"))
    monkeypatch.setenv("MLFLOW_AUC_THRESHOLD", "0.0")
    orig = gb.GBDTParams
    monkeypatch.setattr(mg.gb, "GBDTParams", lambda **kw: orig(**{"n_estimators": 5, "max_depth": 3, "max_bin": 16, **kw}))
    run = lambda **kw: train.run(Settings.load(), cv_folds=2, model_dir=str(tmp_path / "models"), verbose=False, **kw)  # noqa: E731
    with pytest.raises(ValueError, match="gbdt-interaction"):
        run(model_type="gbdt", gbdt_interaction="Amonut,Time")
    with pytest.raises(ValueError, match="needs --model gbdt"):
        run(model_type="logistic", gbdt_interaction="Amount,Time")
    out = run(model_type="gbdt", gbdt_interaction="Amount,Time;V14,V17,V12")
    assert out["gbdt_interaction"] == [["Time", "Amount"], ["V12", "V14", "V17"]]
    clf = GBDTClassifier.load_model(str(tmp_path / "models" / "xgb_model.json"), device="cpu")
    names = [c for c in df.columns if c != "Class"]
    groups = [sorted(names.index(c) for c in g) for g in (("Amount", "Time"), ("V14", "V17", "V12"))]
    assert clf.ensemble.params["interaction_constraints"] == groups
    assert path_violations(clf.ensemble, groups) == 0 and n_mixed_paths(clf.ensemble) > 0


def test_cli_flag_needs_the_gbdt_model(monkeypatch, tmp_path):
    """``train --gbdt-interaction`` without ``--model gbdt`` is an error, not a silently ignored flag."""
    from fraud_detection_amd import train
    from fraud_detection_amd.data.synthetic import reference_frame

    csv = tmp_path / "cc.csv"
    reference_frame(400, seed=1).to_csv(csv, index=False)
    monkeypatch.setenv("DATA_CSV", str(csv))
    monkeypatch.setenv("MLFLOW_TRACKING_URI", str(tmp_path / "mlruns"))
    with pytest.raises(ValueError, match="--gbdt-interaction needs --model gbdt"):
        train.main(["--model", "logistic", "--model-dir", str(tmp_path / "m"), "--gbdt-interaction", "Amount,Time"])
