"""The two-pass k-NN engine bf16x3t on the MI355X: knn_groupmax_kernel (pass 1) -> knn_threshold_kernel
-> knn_filter_kernel (pass 2) -> the re-rank of bf16x3r, each stage against the fp64 emulation of
tests/_knn_cases.py, then end to end on every named case, the variants and small shapes of
test_knn_kernels_gpu.py, and against fp32 / bf16x3r on the pipeline's own minority rows.
The rule and why a broken one is caught: tests/test_knn_twopass_oracle.py.

Tolerance of the stage checks: a quarter of the candidate's margin m (the proof's own requirement on
|approx - exact|, four times the bf16x3 error bound); the device's approximate score differs from the
fp64 emulation of the same three bf16 products only by its fp32 accumulation, far inside that.

Measured on the MI355X (test_filter_lists_hold_exactly_what_passes prints it): heavy lists 6.42
candidates per query, cluster3_far 7.61 (7.78 for queries 7..207); the longest lane list is 13 entries
(cluster3_far, one slice) against the cap of 64."""
import functools

import numpy as np
import pytest
import torch

import _knn_cases as KC
from test_knn_kernels_gpu import VARIANTS, _assert_lattice_exact, _check, _search
from fraud_detection_amd.data.synthetic import separable
from fraud_detection_amd.models.pipeline import DevicePipeline, TrainConfig
from fraud_detection_amd.ops import knn as K
from fraud_detection_amd.ops import scaler as S
from fraud_detection_amd.ops.native import native

pytestmark = pytest.mark.gpu

ENGINE = "bf16x3t"
NEG = -1.0e37  # at or below: no real candidate (the kernel's -3e38 start value or a padding row's score)
STAGE_CASES = ("normal", "heavy", "cluster3_far")
# (query range, self_offset): the fused self-search, and a range whose self candidates straddle two tiles
RANGES = (((0, None), 0), ((7, 207), 7))


def _slice_of_tile(tiles, nsplit):
    out = np.empty(tiles, dtype=np.int64)
    for y in range(nsplit):
        out[tiles * y // nsplit: tiles * (y + 1) // nsplit] = y
    return out


@functools.lru_cache(maxsize=None)
def _emulated(name, lo, hi, self_offset):
    """(approx [mq, mc] with the self column at -inf, margins [mq, mc]) of queries case[lo:hi]; fp64."""
    X = KC.case(name)
    Q = X[lo:hi]
    a = KC.approx_scores(Q, X)
    r = np.arange(Q.shape[0])
    a[r, self_offset + r] = -np.inf
    return a, KC.margins(Q, X)


def _stages(dev, name, k, nsplit, qrange, self_offset):
    lo, hi = qrange
    ops = _search(dev, name, ENGINE, k=k, self_offset=self_offset, lo=lo, hi=hi, nsplit=nsplit)[3]
    out = {n: ops[n].cpu().numpy() for n in ("gmax", "thr", "lists", "counts")}
    out["tmax"] = ops["tmax"].cpu().numpy()
    return out


def _lane_tables(qb):
    """query [qb, 64], half [64] and the group c mod 32 of (register r, lane) [16, 64]."""
    lane = np.arange(64)
    q = np.arange(qb)[:, None] * 32 + (lane & 31)[None, :]
    h = lane >> 5
    r = np.arange(16)[:, None]
    return q, h, 4 * h[None, :] + (r & 3) + 8 * (r >> 2)


@pytest.mark.parametrize("qrange,self_offset", RANGES)
@pytest.mark.parametrize("nsplit", [1, 3])
@pytest.mark.parametrize("name", STAGE_CASES)
def test_group_maxima_and_threshold(dev, name, nsplit, qrange, self_offset):
    k = 5
    a, mg = _emulated(name, qrange[0], qrange[1], self_offset)
    mq, mc = a.shape
    st = _stages(dev, name, k, nsplit, qrange, self_offset)
    gmax = st["gmax"].astype(np.float64)              # [slice][block][17][lane]
    qb = gmax.shape[1]
    q, h, grp = _lane_tables(qb)
    live = q < mq                                      # [qb, 64]
    sl = _slice_of_tile((mc + 31) // 32, nsplit)[np.arange(mc) // 32]
    qs = np.where(live, q, 0)
    for y in range(nsplit):
        for r in range(16):
            lo_b = np.full((qb, 64), -np.inf)          # max of approx -/+ m / 4 over the group's candidates
            hi_b = np.full((qb, 64), -np.inf)
            for hh in (0, 1):
                g = int(grp[r, 32 * hh])
                cols = np.flatnonzero((np.arange(mc) % 32 == g) & (sl == y))
                if cols.size == 0:
                    continue
                aa, mm = a[:, cols], mg[:, cols]
                lane_sel = h == hh
                lo_b[:, lane_sel] = (aa - mm / 4).max(axis=1)[qs[:, lane_sel]]
                hi_b[:, lane_sel] = (aa + mm / 4).max(axis=1)[qs[:, lane_sel]]
            dev_v = gmax[y, :, r, :]
            real = live & np.isfinite(hi_b)
            assert np.all(dev_v[real] >= lo_b[real]) and np.all(dev_v[real] <= hi_b[real]), (y, r)
            assert np.all(dev_v[live & ~real] <= NEG)  # self only, or no candidate at all
        # row 16: the largest margin of the slice's tiles
        if np.any(sl == y):
            want = mg[:, sl == y].max(axis=1)[qs]
            assert np.all(np.abs(gmax[y, :, 16, :][live] - want[live]) <= 1e-5 * want[live] + 1e-30)
    # T = the K-th largest of the 32 group maxima (elementwise max over slices) - the largest margin,
    # recomputed in fp32 from the device's own maxima: bit for bit
    g32 = st["gmax"][:, :, :16, :].max(axis=0)        # [block][16][lane]
    pair = np.concatenate([g32[:, :, :32], g32[:, :, 32:]], axis=1)  # [block][32 groups][j]
    vk = -np.partition(-pair, k - 1, axis=1)[:, k - 1, :]            # [block][j]
    M = st["gmax"][:, :, 16, :32].max(axis=0)
    T_want = (vk - M).astype(np.float32).reshape(-1)
    T_dev, M_dev = st["thr"][0], st["thr"][1]
    assert np.array_equal(T_dev[:mq], T_want[:mq]) and np.all(np.isposinf(T_dev[mq:]))
    assert np.array_equal(M_dev[:mq], M.reshape(-1)[:mq])
    # ... and within a quarter margin of the emulated rule's
    gm = np.stack([a[:, np.arange(mc) % 32 == g].max(axis=1) for g in range(32)], axis=1)
    T_emu = -np.partition(-gm, k - 1, axis=1)[:, k - 1] - mg.max(axis=1)
    assert np.all(np.abs(T_dev[:mq] - T_emu) <= mg.max(axis=1) / 4 + 1e-5 * mg.max(axis=1))
    s = KC.scores64(KC.case(name)[qrange[0]:qrange[1]], KC.case(name), self_offset)
    assert np.all(T_dev[:mq] <= -np.partition(-s, k - 1, axis=1)[:, k - 1])


@pytest.mark.parametrize("qrange,self_offset", RANGES)
@pytest.mark.parametrize("nsplit", [1, 3])
@pytest.mark.parametrize("name", STAGE_CASES)
def test_filter_lists_hold_exactly_what_passes(dev, name, nsplit, qrange, self_offset):
    k, cap = 5, int(native().KNN3R_LIST_CAP)
    a, mg = _emulated(name, qrange[0], qrange[1], self_offset)
    mq, mc = a.shape
    st = _stages(dev, name, k, nsplit, qrange, self_offset)
    T_dev, M_dev = st["thr"][0].astype(np.float64), st["thr"][1]
    cnt = st["counts"]                                  # [3][slice][block][lane]
    n = cnt[0]
    qb = n.shape[1]
    q, h, _ = _lane_tables(qb)
    live_lane = q < mq
    # threshold plane = T, margin plane = M, on every lane of every slice; padding queries list nothing
    for y in range(nsplit):
        assert np.array_equal(cnt[1][y].view(np.float32)[live_lane], st["thr"][0][q[live_lane]])
        assert np.array_equal(cnt[2][y].view(np.float32)[live_lane], M_dev[q[live_lane]])
        assert np.all(np.isposinf(cnt[1][y].view(np.float32)[~live_lane])) and not n[y][~live_lane].any()
    assert n.max() <= cap                               # no overflow on these cases
    L = st["lists"]                                     # [slice][block][entry][lane][2]
    lb, ci = L[..., 0].view(np.float32).astype(np.float64), L[..., 1].astype(np.int64)
    ent = np.arange(cap)[None, None, :, None] < n[:, :, None, :]
    qq = np.broadcast_to(q[None, :, None, :], ent.shape)[ent]
    yy = np.broadcast_to(np.arange(nsplit)[:, None, None, None], ent.shape)[ent]
    hh = np.broadcast_to(h[None, None, None, :], ent.shape)[ent]
    cl, lbl = ci[ent], lb[ent]
    assert qq.max() < mq and cl.min() >= 0 and cl.max() < mc and not np.any(cl == self_offset + qq)
    sl = _slice_of_tile((mc + 31) // 32, nsplit)[np.arange(mc) // 32]
    assert np.array_equal(sl[cl], yy) and np.array_equal(KC.lane_half(mc)[cl], hh)  # the lane's own candidates
    listed = np.zeros((mq, mc), dtype=bool)
    listed[qq, cl] = True
    assert int(listed.sum()) == cl.size == int(n.sum())  # nothing listed twice
    # the stored lower bound is approx - m
    assert np.all(np.abs(lbl - (a[qq, cl] - mg[qq, cl])) <= mg[qq, cl] / 4)
    # every candidate that passes for certain is listed, none that cannot pass is
    sure = (a + 0.75 * mg) >= T_dev[:mq, None]
    possible = (a + 1.25 * mg) >= T_dev[:mq, None]
    assert np.all(listed[sure]), int(np.sum(sure & ~listed))
    assert not np.any(listed[~possible]), int(np.sum(listed & ~possible))
    print(f"\n[knn] {ENGINE} {name} nsplit={nsplit} q={qrange}: listed per query {listed.sum() / mq:.2f}, "
          f"longest lane list {int(n.max())}")


# ---- end to end -------------------------------------------------------------------------------
def _same_as_collect(dev, name, idx, score, **kw):
    """bf16x3r runs the same re-rank on lists that hold every contender: bit-identical results."""
    ri, rs, _, _ = _search(dev, name, "bf16x3r", **kw)
    assert np.array_equal(idx, ri) and np.array_equal(score.view(np.uint32), rs.view(np.uint32))


@pytest.mark.parametrize("name", KC.CASES)
def test_every_case(dev, name):
    idx, score, d2, _ = _search(dev, name, ENGINE)
    _check(name, idx, score, d2, 5)
    _same_as_collect(dev, name, idx, score)
    if name == "lattice":
        _assert_lattice_exact(idx, score, 5)


@pytest.mark.parametrize("k,self_offset,qrange,nsplit", VARIANTS)
@pytest.mark.parametrize("name", ["cluster3", "cluster3_far", "near_origin", "lattice"])
def test_k_self_offset_and_slices(dev, name, k, self_offset, qrange, nsplit):
    lo, hi = qrange
    idx, score, d2, _ = _search(dev, name, ENGINE, k=k, self_offset=self_offset, lo=lo, hi=hi, nsplit=nsplit)
    _check(name, idx, score, d2, k, self_offset, lo, hi)
    _same_as_collect(dev, name, idx, score, k=k, self_offset=self_offset, lo=lo, hi=hi, nsplit=nsplit)
    if name == "lattice":
        _assert_lattice_exact(idx, score, k, self_offset, lo, hi)


@pytest.mark.parametrize("rows,qhi,nsplit", [(6, None, None), (32, None, None), (33, None, None), (300, 1, None),
                                             (300, None, None), (40, None, 3), (300, None, 16), (45, None, 2)])
def test_small_shapes_and_more_slices_than_tiles(dev, rows, qhi, nsplit):
    for name in ("near_origin", "normal"):
        idx, score, d2, _ = _search(dev, name, ENGINE, hi=qhi, nsplit=nsplit, rows=rows)
        _check(name, idx, score, d2, 5, 0, 0, qhi, rows=rows)
        _same_as_collect(dev, name, idx, score, hi=qhi, nsplit=nsplit, rows=rows)


@pytest.mark.parametrize("nsplit", [1, 3])
def test_lattice_sends_exactly_the_tight_queries_to_the_scan(dev, nsplit):
    tight = KC.lattice_tight()
    dg = {}
    idx, score, d2, _ = _search(dev, "lattice", ENGINE, nsplit=nsplit, diag=dg)
    assert dg["nsplit"] == nsplit and dg["exact_scans"] == int(tight.sum())
    assert np.array_equal(dg["scanned"].cpu().numpy(), tight)
    _check("lattice", idx, score, d2, 5)
    _assert_lattice_exact(idx, score, 5)


# ---- the pipeline's rows ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def fit_data(dev):
    return separable(400_000, seed=1000, device=dev)


def test_agrees_with_fp32_and_collect_on_the_minority_rows(dev, fit_data):
    X, y = fit_data
    n = X.shape[0]
    out = torch.empty((n, 32), device=dev, dtype=torch.bfloat16)
    # plain path: standardized minority rows through the index-list chain
    st0 = S.scaler_fit_cast(X, y, out)
    xmin = S.scale_cast(X, st0, labels=y, out_dtype="f32", idx=S.compact_indices(y, 1))
    assert xmin.shape[0] == 680
    plain = {e: K.knn_topk(xmin, xmin, k=5, self_offset=0, engine=e) for e in ("fp32", "bf16x3r", ENGINE)}
    assert torch.equal(plain[ENGINE], plain["fp32"]) and torch.equal(plain[ENGINE], plain["bf16x3r"])
    # fused path: raw rows from the scaler pass, standardized by the prep launch
    fused = {}
    for e in ("fp32", "bf16x3r", ENGINE):
        mino = S.minority_rows_async(y, 1)
        st1 = S.scaler_fit_cast(X, y, out, minority=mino, defer_finalize=True)
        raw = mino.rows()
        fused[e] = K.knn_topk(raw, raw, k=5, self_offset=0, raw_stats=st1, engine=e)
    assert torch.equal(fused[ENGINE], fused["fp32"]) and torch.equal(fused[ENGINE], fused["bf16x3r"])
    assert torch.equal(fused[ENGINE], plain[ENGINE])


def _fit(X, y):
    pipe = DevicePipeline(TrainConfig(solver="sgd", storage="bf16"))
    res = pipe.fit(X, y)
    pipe.settle()
    st = res.scaler
    return (np.array(res.w, copy=True),
            [getattr(st, f).cpu().numpy() for f in ("mean64", "var64", "scale64", "mean32", "inv32", "aff")],
            (res.n_rows, res.n_train_rows, res.n_minority, res.n_synthetic))


def test_one_pipeline_fit_is_bitwise_the_collect_engines(dev, fit_data, monkeypatch):
    X, y = fit_data
    used = []
    real = K.knn_engine  # FDX_KNN is read at every call
    monkeypatch.setattr(K, "knn_engine", lambda *a, **kw: (used.append(real(*a, **kw)), used[-1])[1])
    fits = {}
    for e in ("bf16x3r", ENGINE):
        monkeypatch.setenv("FDX_KNN", e)
        fits[e] = _fit(X, y)
        assert used and set(used) == {e}
        used.clear()
    a, b = fits[ENGINE], fits["bf16x3r"]
    assert a[2] == b[2] and a[2][2] == 680 and a[2][3] > 0
    assert np.array_equal(a[0].view(np.uint8), b[0].view(np.uint8))
    for u, v in zip(a[1], b[1]):
        assert np.array_equal(u.view(np.uint8), v.view(np.uint8))
