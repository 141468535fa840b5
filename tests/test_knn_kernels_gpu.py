"""Every k-NN kernel of csrc/kernels/knn.hip against fp64 oracles on near-tie inputs (MI355X).

prep (all three roles, the fused split included) -> split (row and fragment order, tmax) -> the
engines fp32 / bf16x3r through ``assert_valid_topk`` (bf16x3t is pinned to bf16x3r bit for bit on
every case by tests/test_knn_twopass_gpu.py) -> the fallback (list overflow -> exact scan) -> the
proof's invariants on the device's own MFMA results -> shapes of one tile, one query and more slices
than tiles.
Cases, oracle, tolerance and the filter emulation: tests/_knn_cases.py; why these cases would catch a
broken filter: tests/test_knn_oracle.py."""
import functools

import numpy as np
import pytest
import torch

import _knn_cases as KC
from fraud_detection_amd.ops import knn as K
from fraud_detection_amd.ops import reference as ref
from fraud_detection_amd.ops.native import native, ptr, stream_of

pytestmark = pytest.mark.gpu

# fp32: one 32x32x2 MFMA chain, feature 16h + s at step s; bf16x3r: one re-score chain, columns 0..31 in order
ENGINES = ("fp32", "bf16x3r")


def _pad32(n):
    return max(32, (n + 31) // 32 * 32)


@functools.lru_cache(maxsize=None)
def _dev_rows(name, dev):
    return torch.tensor(KC.case(name), device=dev)


def _search(dev, name, engine, k=5, self_offset=0, lo=0, hi=None, nsplit=None, diag=None, rows=None):
    """One knn_topk call of queries case[lo:hi] (the very tensor when the range is whole: the fused
    self-search prep) against the first ``rows`` rows of the case; (idx, device scores, d2, operands)."""
    C = _dev_rows(name, dev)
    if rows is not None:
        C = C[:rows].contiguous()
    Q = C if lo == 0 and hi is None else C[lo:hi]
    ops = {}
    idx, d2 = K.knn_topk(Q, C, k=k, self_offset=self_offset, want_dist=True, nsplit=nsplit, engine=engine,
                         _operands=ops, _diag=diag)
    return idx.cpu().numpy(), ops["score"].cpu().numpy(), d2.cpu().numpy(), ops


def _check(name, idx, score, d2, k, self_offset=0, lo=0, hi=None, rows=None):
    X = KC.case(name)
    if rows is None:
        s, t = KC.oracle(name, self_offset, lo, hi)
        C = X
    else:
        C = X[:rows]
        s, t = KC.scores64(C[lo:hi], C, self_offset), KC.tolerance(C[lo:hi], C)
    Q = C[lo:hi]
    KC.assert_valid_topk(idx, score, Q, C, k, self_offset, s=s, t=t)
    # the returned squared distance is fp32(||q||^2 - 2 score) of the device's own score, in fp64
    qn = np.sum(Q[:, :30].astype(np.float64) ** 2, axis=1, keepdims=True)
    want = qn - 2.0 * score.astype(np.float64)
    assert np.all(np.abs(d2 - want) <= 2.0 ** -23 * np.abs(want) + 1e-12 * qn)
    return s, t


# ---- 1. prep ----------------------------------------------------------------------------------
def _prep(dev, X, role, m_pad, fused=False):
    """knn_prep on the device; numpy outputs (out, outq or None, Chl, Qhl, tmax or None)."""
    m = native()
    Xd = torch.tensor(X, device=dev)
    out = torch.full((m_pad, 32), float("nan"), device=dev)
    outq = torch.full((m_pad, 32), float("nan"), device=dev) if role == 2 else None
    hl = (None, None, None)
    if fused:
        hl = (torch.zeros((m_pad, 64), device=dev, dtype=torch.bfloat16),
              torch.zeros((m_pad, 64), device=dev, dtype=torch.bfloat16),
              torch.full((m_pad // 32,), float("nan"), device=dev))
    m.knn_prep(ptr(Xd), X.shape[0], m_pad, role, ptr(out), stream_of(Xd), ptr(outq), 0, 0, *(ptr(h) for h in hl))
    torch.cuda.synchronize()
    n = lambda a: None if a is None else (a.view(torch.int16) if a.dtype == torch.bfloat16 else a).cpu().numpy()
    return n(out), n(outq), n(hl[0]), n(hl[1]), n(hl[2])


def _assert_prepped(out, X, role):
    m, m_pad = X.shape[0], out.shape[0]
    assert np.array_equal(out[:m, :30].view(np.uint32), X[:, :30].view(np.uint32))
    assert not np.any(out[:, 31])
    if role == 1:
        assert np.all(out[:m, 30] == 1.0) and not np.any(out[m:])
        return
    h = 0.5 * np.sum(X[:, :30].astype(np.float64) ** 2, axis=1)
    assert np.all(np.abs(out[:m, 30].astype(np.float64) + h) <= 30 * 2.0 ** -24 * h)
    assert not np.any(out[m:, :30]) and np.all(out[m:, 30] == np.float32(KC.PAD_NORM))


@pytest.mark.parametrize("m", [1, 31, 32, 33, 255, 257])
def test_prep_rows_all_roles(dev, m):
    for name in ("normal", "near_origin"):
        X = KC.case(name)[:m]
        m_pad = _pad32(m)
        c, q, *_ = _prep(dev, X, 2, m_pad)
        _assert_prepped(c, X, 0)
        _assert_prepped(q, X, 1)
        c0, *_ = _prep(dev, X, 0, m_pad)
        q1, *_ = _prep(dev, X, 1, m_pad + 96)  # a pad beyond the next multiple of 32: all padding rows
        assert np.array_equal(c0.view(np.uint32), c.view(np.uint32))
        _assert_prepped(q1, X, 1)
        assert np.array_equal(q1[:m_pad].view(np.uint32), q.view(np.uint32))
        cf, qf, *_ = _prep(dev, X, 2, m_pad, fused=True)  # the fused launch writes the same fp32 operands
        assert np.array_equal(cf.view(np.uint32), c.view(np.uint32)) and np.array_equal(qf.view(np.uint32), q.view(np.uint32))


# ---- 2. split ---------------------------------------------------------------------------------
def _bf16_bits(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16).view(torch.int16).numpy()


def _expected_hl(Xp):
    """[m_pad, 64] int16, row order: bf16_rne(x) of columns 0..31, then bf16_rne(x - hi)."""
    hi = ref.bf16_round(Xp)
    return np.concatenate([_bf16_bits(Xp), _bf16_bits(Xp - hi)], axis=1)


def _from_fragment_order(raw):
    """knn_split_kernel role 2: tile r / 32 is [u 0..3][lane 64] 16-byte pieces, lane (half hh, row j)
    of load u holding chunk 2u + hh of row j (chunks 0..3 = hi columns 8v .. 8v + 7, 4..7 = lo)."""
    tiles = raw.shape[0] // 32
    a = raw.reshape(tiles, 4, 2, 32, 8)                      # [tile][u][hh][j][8 bf16]
    return a.transpose(0, 3, 1, 2, 4).reshape(tiles * 32, 64)  # [tile * 32 + j][(2u + hh) * 8 ..]


def _assert_tmax(tmax, Cp, X):
    m = X.shape[0]
    n = np.zeros(Cp.shape[0])
    n[:m] = np.sqrt(np.sum(X[:, :30].astype(np.float64) ** 2, axis=1))
    n = n.reshape(-1, 32).max(axis=1)
    assert np.all(tmax.astype(np.float64) >= n)
    assert np.all(tmax.astype(np.float64) <= n * 1.0001 * (1 + 2.0 ** -20))
    assert tmax[-1] == 0.0 and n[-1] == 0.0  # the all-padding tile


@pytest.mark.parametrize("name", ["normal", "heavy", "lattice"])
def test_split_hi_lo_fragment_order_and_tmax(dev, name):
    m_ = native()
    X = KC.case(name)
    m_pad = _pad32(X.shape[0]) + 32  # one all-padding tile
    Cp, Qp, chl_f, qhl_f, tmax_f = _prep(dev, X, 2, m_pad, fused=True)
    want_c, want_q = _expected_hl(Cp), _expected_hl(Qp)
    if name == "lattice":
        assert np.any(want_c[: X.shape[0], 32:62]) and np.any(want_q[: X.shape[0], 32:62])  # lo != 0
    # the fused prep's split: candidates in fragment order, queries in row order
    assert np.array_equal(_from_fragment_order(chl_f), want_c)
    assert np.array_equal(qhl_f, want_q)
    _assert_tmax(tmax_f, Cp, X)
    # the split kernel on the same prepped rows
    Cd, Qd = torch.from_numpy(Cp).to(dev), torch.from_numpy(Qp).to(dev)
    for role, src, want in ((0, Cd, want_c), (2, Cd, want_c), (1, Qd, want_q)):
        hl = torch.zeros((m_pad, 64), device=dev, dtype=torch.bfloat16)
        tm = torch.full((m_pad // 32,), float("nan"), device=dev)
        m_.knn_split(ptr(src), m_pad, role, ptr(hl), ptr(tm) if role != 1 else 0, stream_of(src))
        got = hl.view(torch.int16).cpu().numpy()
        assert np.array_equal(_from_fragment_order(got) if role == 2 else got, want), role
        if role != 1:
            assert np.array_equal(tm.cpu().numpy(), tmax_f)
            _assert_tmax(tm.cpu().numpy(), Cp, X)


# ---- 3. engines -------------------------------------------------------------------------------
def _assert_groups(res, lattice):
    """bit identity of (idx, score) across the engines on the lattice, where every product and sum is exact
    in fp32 whatever the summation chain.  Off it the engines' chains differ, and each engine is held to
    the fp64 oracle by ``_check`` alone."""
    if not lattice:
        return
    for e in ENGINES[1:]:
        assert np.array_equal(res[e][0], res[ENGINES[0]][0]), (ENGINES[0], e, "idx")
        assert np.array_equal(res[e][1].view(np.uint32), res[ENGINES[0]][1].view(np.uint32)), (ENGINES[0], e, "score")


def _assert_lattice_exact(idx, score, k, self_offset=0, lo=0, hi=None):
    X = KC.case("lattice")
    want = ref.knn_topk(X[lo:hi], X, k, self_offset)[0]
    s, _ = KC.oracle("lattice", self_offset, lo, hi)
    assert np.array_equal(idx, want)
    assert np.array_equal(score, np.take_along_axis(s, want.astype(np.int64), 1).astype(np.float32))


@pytest.mark.parametrize("name", KC.CASES)
def test_engines_on_every_case(dev, name):
    res = {}
    for e in ENGINES:
        idx, score, d2, _ = _search(dev, name, e)
        _check(name, idx, score, d2, 5)
        res[e] = (idx, score)
    _assert_groups(res, name == "lattice")
    if name == "lattice":
        _assert_lattice_exact(*res["fp32"], 5)


# (k, self_offset, query range, nsplit): every engine sees k in {1, 8}, self_offset in {-1, 7} with a
# strict sub-range of the candidates as queries, and nsplit in {1, 3}
VARIANTS = [(1, 0, (0, None), 1), (8, -1, (10, 150), 3), (8, 7, (7, 207), 1), (1, -1, (40, 41), 3)]


@pytest.mark.parametrize("k,self_offset,qrange,nsplit", VARIANTS)
@pytest.mark.parametrize("name", ["cluster3", "cluster3_far", "near_origin", "lattice"])
def test_engines_k_self_offset_and_slices(dev, name, k, self_offset, qrange, nsplit):
    lo, hi = qrange
    res = {}
    for e in ENGINES:
        idx, score, d2, _ = _search(dev, name, e, k=k, self_offset=self_offset, lo=lo, hi=hi, nsplit=nsplit)
        _check(name, idx, score, d2, k, self_offset, lo, hi)
        res[e] = (idx, score)
    _assert_groups(res, name == "lattice")
    if name == "lattice":
        _assert_lattice_exact(*res["fp32"], k, self_offset, lo, hi)


# ---- 4. the fallback on the lattice --------------------------------------------------------------
def test_collect_overflow_sends_exactly_the_tight_queries_to_the_scan(dev):
    X, tight = KC.case("lattice"), KC.lattice_tight()
    mq = X.shape[0]
    dg = {}
    idx, score, d2, _ = _search(dev, "lattice", "bf16x3r", nsplit=1, diag=dg)
    cap = dg["list_cap"]
    over = (dg["counts"].cpu().numpy()[0] > cap)            # [query block][lane = j + 32 h]
    assert 0 < dg["over_cap"] < over.size and dg["over_cap"] == int(over.sum())
    per_query = over.reshape(-1, 2, 32).transpose(0, 2, 1).reshape(-1, 2)  # [query][h]
    assert not per_query[mq:].any()                         # padding queries append nothing
    assert np.array_equal(per_query[:mq, 0], tight) and np.array_equal(per_query[:mq, 1], tight)
    _check("lattice", idx, score, d2, 5)
    _assert_lattice_exact(idx, score, 5)


# ---- 5. the proof's invariants on the device's own MFMA results ----------------------------------
def _operands(dev, name):
    """Prepped rows, hi/lo operands (candidates in fragment order) and tmax of a case's self-search."""
    ops = _search(dev, name, "bf16x3r")[3]
    return ops["Qp"], ops["Qhl"], ops["Cp"], ops["Chl"], ops["tmax"]


@pytest.mark.parametrize("nsplit", [1, 3])
@pytest.mark.parametrize("name", ["cluster3", "cluster3_far", "heavy"])
def test_collect_lists_hold_lower_bounds_and_every_contender(dev, name, nsplit):
    m_ = native()
    X = KC.case(name)
    s, t = KC.oracle(name)
    mq = mc = X.shape[0]
    k, cap = 5, int(m_.KNN3R_LIST_CAP)
    Qp, Qhl, Cp, Chl, tmax = _operands(dev, name)
    mq_pad, mc_pad = Qp.shape[0], Cp.shape[0]
    qb = mq_pad // 32
    nb = nsplit * qb * 64
    lists = torch.full((nb * cap * 2,), -1, device=dev, dtype=torch.int32)
    counts = torch.full((3 * nb,), -1, device=dev, dtype=torch.int32)
    idx = torch.empty((mq, k), device=dev, dtype=torch.int32)
    score = torch.empty((mq, k), device=dev, dtype=torch.float32)
    m_.knn_topk3r(ptr(Qp), ptr(Qhl), mq_pad, mq, ptr(Cp), ptr(Chl), ptr(tmax), mc_pad, mc, 0, k, ptr(idx),
                  ptr(score), ptr(lists), ptr(counts), nsplit, stream_of(Qp))
    KC.assert_valid_topk(idx.cpu().numpy(), score.cpu().numpy(), X, X, k, 0, s=s, t=t)
    cnt = counts.cpu().numpy().reshape(3, nsplit, qb, 64)
    n, thr = cnt[0], cnt[1].view(np.float32)
    L = lists.cpu().numpy().reshape(nsplit, qb, cap, 64, 2)
    lb, ci = L[..., 0].view(np.float32), L[..., 1]
    # query of [slice][block][entry][lane]: block * 32 + (lane & 31)
    q = (np.arange(qb)[:, None, None] * 32 + (np.arange(64) & 31)[None, None, :]) + np.zeros((nsplit, 1, cap, 1), dtype=np.int64)
    live = (np.arange(cap)[None, None, :, None] < np.minimum(n, cap)[:, :, None, :]) & (q < mq)
    assert not n[:, (np.arange(qb)[:, None] * 32 + (np.arange(64) & 31)[None, :]) >= mq].any()
    ql, cl, lbl = q[live], ci[live].astype(np.int64), lb[live].astype(np.float64)
    assert cl.min() >= 0 and cl.max() < mc and not np.any(cl == ql)
    # a listed lower bound really is one
    assert np.all(lbl <= s[ql, cl] + t[ql, cl]), float(np.max(lbl - s[ql, cl] - t[ql, cl]))
    # each lane's final threshold is at most the k-th best exact score (k candidates have s + t >= lb >= thr)
    kth_hi = -np.partition(-(s + t), k - 1, axis=1)[:, k - 1]
    lane_q = np.arange(qb)[:, None] * 32 + (np.arange(64) & 31)[None, :]
    okq = lane_q < mq
    for y in range(nsplit):
        assert np.all(thr[y][okq].astype(np.float64) <= kth_hi[lane_q[okq]])
    # every candidate that could be in the answer is on a list of its query (no lane over the cap here)
    listed = np.zeros((mq, mc), dtype=bool)
    listed[ql, cl] = True
    over = np.zeros(mq, dtype=bool)
    ov = n > cap
    for y in range(nsplit):
        over[lane_q[okq & ov[y]]] = True
    sk = -np.partition(-s, k - 1, axis=1)[:, k - 1]
    must = (s >= sk[:, None] - t) & ~over[:, None]
    assert np.all(listed[must]), int(np.sum(must & ~listed))


# ---- 6. small shapes --------------------------------------------------------------------------
@pytest.mark.parametrize("rows,qhi,nsplit", [(6, None, None), (32, None, None), (33, None, None), (300, 1, None),
                                             (40, None, 3), (300, None, 16)])
def test_small_shapes_and_more_slices_than_tiles(dev, rows, qhi, nsplit):
    # one tile, one tile and a row, a single query; then slices that own no tile at all (their lists
    # stay empty and the seeded slices of the collect kernel get no seed): the merged answer
    for name in ("near_origin", "normal"):
        for e in ENGINES:
            idx, score, d2, _ = _search(dev, name, e, hi=qhi, nsplit=nsplit, rows=rows)
            _check(name, idx, score, d2, 5, 0, 0, qhi, rows=rows)
