"""Stochastic boosting on the GPU (gbdt.hip: gbdt_grad_kernel<SAMPLE>, gbdt_margin_kernel<GRAD, SAMPLE>,
the masked gbdt_split_kernel) against the numpy oracle's draws (ops/reference_gbdt.py).

The draws are integer functions, so which rows and features are in a sample is exact; the only
tolerance is test_gbdt_gpu.py's for the fp64 sigmoid of an in-sample row."""
import numpy as np
import pytest
import torch

import _gbdt_state as S
from fraud_detection_amd.ops import gbdt as gb
from fraud_detection_amd.ops import reference_gbdt as R
from fraud_detection_amd.ops.native import native, ptr, stream_of

pytestmark = pytest.mark.gpu

TREE_ARRAYS = ("feat", "bin", "thr", "gain", "leaf")
N_ROWS = 10_007  # odd, 40 blocks of 256 minus a ragged tail
SUB = 0.37
SEED = (0x9E37 << 32) | 0x1234567  # both key words in use
OFFSETS = [0, 3, (1 << 34) - 6]    # aligned; lane quads off the Philox groups; group ids across 2^32


def _data(n, d, seed=0, dev="cuda"):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, d)).astype(np.float32)
    X[:, 1] = np.round(X[:, 1] * 3) / 3
    logit = 1.2 * X[:, 0] - 1.5 * (X[:, 1] > 0.3) + X[:, 2] * X[:, 3] - 3.0
    y = (rng.random(n) < 1 / (1 + np.exp(-logit))).astype(np.uint8)
    return torch.from_numpy(X).to(dev), torch.from_numpy(y).to(dev), X, y


_rows = {}


def _row_case():
    """Margins, labels and (for the walk) bins + a crafted depth-3 tree, shared by the kernel tests."""
    if not _rows:
        rng = np.random.default_rng(1)
        d = 6
        nb = np.array([256, 2, 256, 5, 1, 64], np.int32)
        bins = S.random_bins(rng, N_ROWS, d, nb)
        feat = np.array([0, -1, 2, 5, 3, 0, 1], np.int32)
        binv = np.array([int(bins[17, 0]), 255, int(bins[5, 2]), 31, 2, 254, 0], np.int32)
        _rows.update(margin=rng.normal(scale=3.0, size=N_ROWS).astype(np.float32),
                     y=(rng.random(N_ROWS) < 0.3).astype(np.uint8), d=d, bins=bins, feat=feat, binv=binv,
                     leaf=rng.normal(scale=0.3, size=8).astype(np.float32))
    return _rows


def _check_sampled_gh(gh: np.ndarray, margin, y, spw, t, off):
    """Out-of-sample rows exactly 0; in-sample rows within test_grad_kernel_matches_oracle's bound."""
    gs, hs = R.grad_scales(spw)
    mask = R.row_sample_mask(SEED, t, off + np.arange(len(margin), dtype=np.int64), SUB)
    ref = R.gradients(margin, y, spw, gs, hs)
    ref[~mask] = 0
    assert 0.3 < mask.mean() < 0.44  # 0.37 +- 5 sigma at 10^4 rows is +-0.025
    assert (gh[~mask] == 0).all()
    assert (ref[mask] != 0).any(axis=1).mean() > 0.9  # the in-sample rows do carry gradients
    diff = np.abs(gh.astype(np.int64) - ref)
    assert diff.max() <= 1 and (diff > 0).mean() < 1e-3


@pytest.mark.parametrize("t", [0, 7])
@pytest.mark.parametrize("off", OFFSETS)
def test_sampled_grad_kernel(dev, off, t):
    c = _row_case()
    spw = 37.5
    gs, hs = R.grad_scales(spw)
    md, yd = S.to_dev(c["margin"], dev), S.to_dev(c["y"], dev)
    gh = torch.full((N_ROWS + 8, 2), -1, dtype=torch.int16, device=dev)
    native().gbdt_grad_sampled(ptr(md), ptr(yd), N_ROWS, spw, gs, hs, ptr(gh), SEED, t, off,
                               R.sample_threshold(SUB), stream_of(md))
    got = gh.cpu().numpy()
    assert (got[N_ROWS:] == -1).all()  # nothing past row n
    _check_sampled_gh(got[:N_ROWS], c["margin"], c["y"], spw, t, off)


@pytest.mark.parametrize("t", [1, 7])
@pytest.mark.parametrize("off", OFFSETS)
def test_sampled_margin_kernel(dev, off, t):
    m = native()
    c = _row_case()
    spw, depth, d = 3.0, 3, c["d"]
    gs, hs = R.grad_scales(spw)
    bt, ldt = S.transpose_bins(c["bins"], d)
    binsT, yd = S.to_dev(bt, dev), S.to_dev(c["y"], dev)
    fd, bd, ld = S.to_dev(c["feat"], dev), S.to_dev(c["binv"], dev), S.to_dev(c["leaf"], dev)
    plain = S.to_dev(c["margin"], dev)
    gh_plain = torch.empty((N_ROWS, 2), dtype=torch.int16, device=dev)
    m.gbdt_margin(ptr(binsT), ldt, N_ROWS, ptr(fd), ptr(bd), ptr(ld), depth, ptr(plain), ptr(yd), spw, gs, hs,
                  ptr(gh_plain), stream_of(binsT))
    samp = S.to_dev(c["margin"], dev)
    gh = torch.full((N_ROWS + 8, 2), -1, dtype=torch.int16, device=dev)
    m.gbdt_margin_sampled(ptr(binsT), ldt, N_ROWS, ptr(fd), ptr(bd), ptr(ld), depth, ptr(samp), ptr(yd), spw, gs, hs,
                          ptr(gh), SEED, t, off, R.sample_threshold(SUB), stream_of(binsT))
    # every row takes the tree's leaf, in the sample or not
    assert torch.equal(samp, plain)
    walk = R.predict_margin_bins(c["bins"], c["feat"][None], c["binv"][None], c["leaf"][None], depth, 0.0)
    new_margin = (c["margin"] + walk).astype(np.float32)
    assert np.array_equal(samp.cpu().numpy().view(np.uint32), new_margin.view(np.uint32))
    got = gh.cpu().numpy()
    assert (got[N_ROWS:] == -1).all()
    _check_sampled_gh(got[:N_ROWS], new_margin, c["y"], spw, t, off)
    # an in-sample row's word is the unsampled kernel's, bit for bit (same device function)
    mask = R.row_sample_mask(SEED, t, off + np.arange(N_ROWS, dtype=np.int64), SUB)
    assert np.array_equal(got[:N_ROWS][mask], gh_plain.cpu().numpy()[mask])


def test_sampled_launchers_reject_bad_arguments(dev):
    c = _row_case()
    md, yd = S.to_dev(c["margin"], dev), S.to_dev(c["y"], dev)
    gh = torch.empty((N_ROWS, 2), dtype=torch.int16, device=dev)
    for rnd, off in ((-1, 0), (1 << 32, 0), (0, -1)):
        with pytest.raises(RuntimeError):
            native().gbdt_grad_sampled(ptr(md), ptr(yd), N_ROWS, 1.0, 1.0, 1.0, ptr(gh), 0, rnd, off, 1, stream_of(md))


# ---- masked split -----------------------------------------------------------------------------------
GS, HS = R.grad_scales(1.0)
GINV, HINV = 1.0 / GS, 1.0 / HS


def split_level_oracle(hist, gcnt, level, d, nbins, cuts, lam, mcw, gamma, fmask):
    """_gbdt_state.split_level_oracle with a per-heap-node feature mask: a derived node's histogram
    is stored for EVERY feature, the totals are feature 0's, only the candidates are masked."""
    h0, nn = S.heap_first(level), 1 << level
    built = S.built_mask(level, gcnt[h0:h0 + nn])
    hist = hist.copy()
    feat = np.full(nn, -1, np.int32)
    binv = np.full(nn, 255, np.int32)
    thr = np.full(nn, np.inf, np.float32)
    gain = np.zeros(nn, np.float64)
    sums = {}
    for k in range(nn):
        node = h0 + k
        if not built[k]:
            hist[node, :d] = hist[(node - 1) >> 1, :d] - hist[h0 + (k ^ 1), :d]
        g_, f, b, GLq, HLq, Gq, Hq = R.best_split(hist[node, :d], np.asarray(nbins), GINV, HINV, lam, mcw,
                                                  fmask=int(fmask[node]))
        if node == 0:
            sums[0] = (Gq, Hq)
        if R.accepts_split(g_, gamma):
            feat[k], binv[k], thr[k], gain[k] = f, b, cuts[f, b], g_
            sums[2 * node + 1], sums[2 * node + 2] = (GLq, HLq), (Gq - GLq, Hq - HLq)
        else:
            sums[2 * node + 1], sums[2 * node + 2] = (Gq, Hq), (0, 0)
    return hist, feat, binv, thr, gain, sums


def run_split(hist, gcnt, level, d, nbins, cuts, lam, mcw, gamma, fmask, dev):
    """_gbdt_state.run_split with the mask argument (None: the argument left out)."""
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
    extra = () if fmask is None else (ptr(S.to_dev(np.asarray(fmask, np.uint32).view(np.int32), dev)),)
    m.gbdt_split(ptr(hd), ptr(gd), level, d, ptr(nt), ptr(ct), GINV, HINV, float(lam), float(mcw), float(gamma),
                 ptr(feat), ptr(binv), ptr(thr), ptr(gain), ptr(ng), ptr(nh), stream_of(hd), *extra)
    torch.cuda.synchronize()
    sl = slice(h0, h0 + nn)
    return (hd.cpu().numpy().reshape(hist.shape), feat[sl].cpu().numpy(), binv[sl].cpu().numpy(),
            thr[sl].cpu().numpy(), gain[sl].cpu().numpy(), ng.cpu().numpy(), nh.cpu().numpy())


def _level_hists(rng, level, d, nbins):
    """A level's histogram tensor: of every sibling pair one node is written (built), the other
    exists only as parent - sibling (test_gbdt_kernels_gpu._level_hists)."""
    ni = (2 << level) - 1
    h0, nn = S.heap_first(level), 1 << level
    hist = np.zeros((ni, S.MAX_FEAT, 256, 2), np.int64)
    gcnt = np.zeros(2 * ni + 1, np.int64)
    gcnt[h0:h0 + nn] = rng.integers(0, 1000, nn)
    tot = lambda: (int(rng.integers(-(1 << 24), 1 << 24)), int(rng.integers(1, 1 << 30)))  # noqa: E731
    if level == 0:
        hist[0] = S.hist_with_totals(rng, d, nbins, *tot(), 1 << 24)
        return hist, gcnt
    for k in range(0, nn, 2):
        a = S.hist_with_totals(rng, d, nbins, *tot(), 1 << 24)
        b = S.hist_with_totals(rng, d, nbins, *tot(), 1 << 24)
        built = S.built_mask(level, gcnt[h0:h0 + nn])
        hist[h0 + k + (0 if built[k] else 1)] = a
        hist[(h0 + k - 1) >> 1] = a + b
    return hist, gcnt


@pytest.mark.parametrize("d", [30, 5])
@pytest.mark.parametrize("level", [0, 2])
def test_masked_split(dev, level, d):
    rng = np.random.default_rng(10 * level + d)
    nb = np.array([(256, 1, 2, 77, 256)[f % 5] for f in range(d)], np.int32)
    cuts = np.sort(rng.normal(size=(d, 256)).astype(np.float32), axis=1)
    cuts[:, 255] = np.inf
    hist, gcnt = _level_hists(rng, level, d, nb)
    ni = hist.shape[0]
    h0, nn = S.heap_first(level), 1 << level
    everything = (1 << d) - 1
    lam, mcw, gamma = 1.0, 1.0, 0.0
    free = split_level_oracle(hist, gcnt, level, d, nb, cuts, lam, mcw, gamma, np.full(ni, everything, np.uint32))
    assert all(np.array_equal(a, b) for a, b in zip(free[:5], S.split_level_oracle(
        hist, gcnt, level, d, nb, cuts, GINV, HINV, lam, mcw, gamma)[:5]))
    assert (free[1] >= 0).all()  # every node of the level splits when it may use any feature
    if level:
        assert (~S.built_mask(level, gcnt[h0:h0 + nn])).sum() == nn // 2  # derived nodes in the level
    # a null mask and an all-ones mask are the unmasked kernel
    S.assert_split_equal(run_split(hist, gcnt, level, d, nb, cuts, lam, mcw, gamma, None, dev), free, level)
    no_winner = np.full(ni, everything, np.uint32)
    no_winner[h0:h0 + nn] &= ~(np.uint32(1) << free[1].astype(np.uint32))
    masks = {"all": np.full(ni, everything, np.uint32),
             "one feature": np.full(ni, 1 << (d - 1), np.uint32),
             "feature 0 excluded": np.full(ni, everything & ~1, np.uint32),
             "constant features only": np.full(ni, sum(1 << f for f in range(d) if nb[f] == 1), np.uint32),
             "winner excluded": no_winner,
             "random per node": rng.integers(1, everything + 1, ni).astype(np.uint32)}
    for name, fm in masks.items():
        ref = split_level_oracle(hist, gcnt, level, d, nb, cuts, lam, mcw, gamma, fm)
        got = run_split(hist, gcnt, level, d, nb, cuts, lam, mcw, gamma, fm, dev)
        S.assert_split_equal(got, ref, level)  # incl. the stored derived histograms of masked features
        for k in range(nn):
            assert ref[1][k] < 0 or (int(fm[h0 + k]) >> int(ref[1][k])) & 1, name
        if name == "one feature":
            assert set(ref[1].tolist()) <= {-1, d - 1}
        if name == "constant features only":
            assert (ref[1] == -1).all()  # no valid allowed split: the node does not split
        if name == "winner excluded":
            assert (ref[1] != free[1]).all() and (ref[4] <= free[4]).all()
        if name == "feature 0 excluded":
            assert (ref[1] != 0).all()
            for node in range(h0, h0 + nn):  # totals still feature 0's sums
                assert ref[5][2 * node + 1][0] + ref[5][2 * node + 2][0] == int(ref[0][node, 0, :, 0].sum())


# ---- whole fits -------------------------------------------------------------------------------------
ALL_HALF = dict(subsample=0.5, colsample_bytree=0.5, colsample_bylevel=0.5, colsample_bynode=0.5, seed=SEED)


def _assert_same_fit(a, b):
    for k in TREE_ARRAYS:
        assert np.array_equal(getattr(a, k), getattr(b, k)), k


@pytest.mark.parametrize("n,d,depth", [(5_000, 7, 3), (777, 4, 6), (60_000, 30, 5)])
def test_first_sampled_tree_exact(dev, n, d, depth):
    """Round 0 (margin 0: exactly representable gradients): same rows, same features, same tree."""
    Xd, yd, X, y = _data(n, d, seed=n)
    p = gb.GBDTParams(n_estimators=1, max_depth=depth, scale_pos_weight=3.0, **ALL_HALF)
    cuts = R.quantile_cuts(X, 256)
    ens, margin = gb.fit(Xd, yd, p, cuts=cuts, return_margin=True)
    ref, rmargin = gb.fit(torch.from_numpy(X), torch.from_numpy(y), p, cuts=cuts, return_margin=True)
    _assert_same_fit(ens, ref)
    assert np.array_equal(margin.cpu().numpy(), rmargin.numpy())
    assert (ref.feat >= 0).any()
    plain = gb.fit(torch.from_numpy(X), torch.from_numpy(y),
                   gb.GBDTParams(n_estimators=1, max_depth=depth, scale_pos_weight=3.0), cuts=cuts)
    assert not np.array_equal(plain.leaf, ref.leaf)  # the sample does change the tree


def test_first_sampled_tree_exact_around_a_hole(dev):
    """A row keeps its table index: the rows behind the hole draw as rows 1777 .., on both paths."""
    Xd, yd, X, y = _data(5_000, 7, seed=5_000)
    p = gb.GBDTParams(n_estimators=1, max_depth=3, scale_pos_weight=3.0, **ALL_HALF)
    cuts = R.quantile_cuts(X, 256)
    bins_h = torch.from_numpy(R.bin_rows(X, *cuts))
    hole = (1000, 777)
    ens, margin = gb.fit_binned(bins_h.to(dev), yd, cuts, p, return_margin=True, hole=hole)
    ref, rmargin = gb.fit_binned(bins_h, torch.from_numpy(y), cuts, p, return_margin=True, hole=hole)
    _assert_same_fit(ens, ref)
    assert np.array_equal(margin.cpu().numpy(), rmargin.numpy())
    keep = np.r_[0:1000, 1777:5000]
    packed = gb.fit_binned(bins_h[keep], torch.from_numpy(y[keep]), cuts, p)  # the same rows, renumbered
    assert not np.array_equal(packed.leaf, ref.leaf)


def test_sampled_boosting_matches_oracle(dev):
    """test_boosting_matches_oracle's data and its two bounds, with half the rows and half the features."""
    Xd, yd, X, y = _data(80_000, 12, seed=5)
    p = gb.GBDTParams(n_estimators=12, max_depth=5, scale_pos_weight=5.0, subsample=0.5, colsample_bytree=0.5, seed=SEED)
    cuts = R.quantile_cuts(X, 256)
    ens, margin = gb.fit(Xd, yd, p, cuts=cuts, return_margin=True)
    ref, rmargin = gb.fit(torch.from_numpy(X), torch.from_numpy(y), p, cuts=cuts, return_margin=True)
    same = np.all(ens.feat == ref.feat, axis=1) & np.all(ens.bin == ref.bin, axis=1)
    print(f"identical trees {same.mean():.3f}, max |margin diff| {np.abs(margin.cpu().numpy() - rmargin.numpy()).max():.3e}")
    assert same.mean() >= 0.9
    np.testing.assert_allclose(margin.cpu().numpy(), rmargin.numpy(), atol=2e-3)


@pytest.mark.parametrize("fracs", [(0.5, 1.0, 1.0), (1.0, 0.5, 1.0), (0.8, 0.5, 0.3)])
def test_every_round_splits_inside_its_own_masks(dev, fracs):
    """Twenty rounds at 30 features (two features per scanning wave): round t's launches read row t
    of the uploaded table, every node its own word -- checked against the per-round definition."""
    Xd, yd, X, y = _data(20_000, 30, seed=17)
    T, depth = 20, 5
    p = gb.GBDTParams(n_estimators=T, max_depth=depth, colsample_bytree=fracs[0], colsample_bylevel=fracs[1],
                      colsample_bynode=fracs[2], seed=SEED)
    ens = gb.fit(Xd, yd, p, cuts=R.quantile_cuts(X, 256))
    for t in range(T):
        fm = R.feature_masks(SEED, t, 30, depth, *fracs)
        for node, f in enumerate(ens.feat[t]):
            assert f < 0 or (int(fm[node]) >> int(f)) & 1, (t, node, int(f))
    assert (ens.feat >= 0).sum() > 10 * T
    used = {int(f) for f in ens.feat.ravel() if f >= 0}
    assert len(used) > int(30 * fracs[0] * fracs[1] * fracs[2])  # the draws do move from round to round


def test_sampled_fits_repeat_and_defaults_change_nothing(dev, monkeypatch):
    Xd, yd, X, y = _data(50_000, 30, seed=14)
    cuts = R.quantile_cuts(X, 256)
    kw = dict(n_estimators=6, max_depth=5)
    p = gb.GBDTParams(subsample=0.5, colsample_bynode=0.5, seed=3, **kw)
    a, ma = gb.fit(Xd, yd, p, cuts=cuts, return_margin=True)
    b, mb = gb.fit(Xd, yd, p, cuts=cuts, return_margin=True)
    _assert_same_fit(a, b)
    assert torch.equal(ma, mb)
    # every fraction at 1.0: the seed is dead and the fit is the default fit
    base, mbase = gb.fit(Xd, yd, gb.GBDTParams(**kw), cuts=cuts, return_margin=True)
    seeded, mseed = gb.fit(Xd, yd, gb.GBDTParams(seed=9, **kw), cuts=cuts, return_margin=True)
    _assert_same_fit(base, seeded)
    assert torch.equal(mbase, mseed)
    assert not np.array_equal(a.leaf, base.leaf)
    # the opt-in paths fall back to the eager, unfused round under sampling
    g, mg = gb.fit(Xd, yd, p, cuts=cuts, return_margin=True, use_graph=True)
    _assert_same_fit(a, g)
    assert torch.equal(ma, mg)
    monkeypatch.setenv("FDX_GBDT_GRAPH", "1")
    g, mg = gb.fit(Xd, yd, p, cuts=cuts, return_margin=True)
    _assert_same_fit(a, g)
    assert torch.equal(ma, mg)
    monkeypatch.delenv("FDX_GBDT_GRAPH")
    monkeypatch.setenv("FDX_GBDT_FUSE_MARGIN", "1")
    f, mf = gb.fit(Xd, yd, p, cuts=cuts, return_margin=True)
    _assert_same_fit(a, f)
    assert torch.equal(ma, mf)


def test_sampled_resume_bit_identical(dev, tmp_path):
    from fraud_detection_amd.utils.checkpoint import CheckpointManager

    Xd, yd, X, y = _data(30_000, 10, seed=13)
    kw = dict(max_depth=4, subsample=0.5, colsample_bynode=0.5, seed=8)
    cuts = R.quantile_cuts(X, 256)
    full = gb.fit(Xd, yd, gb.GBDTParams(n_estimators=6, **kw), cuts=cuts)
    mgr = CheckpointManager(str(tmp_path), prefix="g")
    gb.fit(Xd, yd, gb.GBDTParams(n_estimators=3, **kw), cuts=cuts, checkpoint=mgr, checkpoint_every=3)
    res = gb.fit(Xd, yd, gb.GBDTParams(n_estimators=6, **kw), cuts=cuts, checkpoint=mgr, checkpoint_every=3)
    _assert_same_fit(res, full)


def test_sampled_early_stopping(dev):
    """Evaluation sees the full eval rows whatever the training sample is: round 0's exact record
    equals the CPU fit's, and the ensemble keeps best_iteration + 1 trees."""
    Xd, yd, X, y = _data(20_000, 8, seed=21)
    Xv, yv, Xvh, yvh = _data(4_000, 8, seed=22)
    cuts = R.quantile_cuts(X, 256)
    p = gb.GBDTParams(n_estimators=12, max_depth=4, learning_rate=0.5, subsample=0.5, seed=2)
    ens, rec = gb.fit(Xd, yd, p, cuts=cuts, eval_set=(Xv, yv), early_stopping_rounds=3)
    ref, rrec = gb.fit(torch.from_numpy(X), torch.from_numpy(y), p, cuts=cuts,
                       eval_set=(torch.from_numpy(Xvh), torch.from_numpy(yvh)), early_stopping_rounds=3)
    assert np.array_equal(rec.records[0], rrec.records[0])
    assert rec.records[0, 3] == 4_000
    assert ens.n_trees == rec.best_iteration + 1 and ref.n_trees == rrec.best_iteration + 1
    assert np.array_equal(ens.feat[0], ref.feat[0]) and np.array_equal(ens.leaf[0], ref.leaf[0])
