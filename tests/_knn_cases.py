"""Shared inputs and oracles of the k-NN oracle tests (test_knn_oracle.py, test_knn_kernels_gpu.py).
numpy only: seeded cases of 32-column padded rows, the fp64 score matrix with its derived fp32
tolerance, a checker that accepts every top-k an fp32 engine may legitimately return, and an fp64
emulation of the bf16x3 filter (hi/lo split, approximate score, margin, final-threshold filter).

Tolerance.  score(q, c) = q.c - 0.5 ||c||^2.  With S = |q|.|c| + 0.5 ||c||^2 (the sum of the absolute
terms): the prep's 30-fmaf norm chain is off by at most 30 ulp of 0.5 ||c||^2 and a 31- or 32-term
fp32 score chain by at most 32 ulp of S in ANY summation order, so tol = 64 * 2^-24 * S covers the
32x32x2 MFMA chain (feature 16h + s at step s) and the column-order re-score alike.  Derived, not
tuned."""
import functools

import numpy as np

from fraud_detection_amd.ops import reference as ref

D = 30
K_MARGIN_SCALE = 2.0 ** -14  # knn.hip kMarginScale
NORM_SLACK = 1.0001          # knn.hip: tmax and ||q|| are inflated by this factor
PAD_NORM = -3.0e38           # column 30 of a padding candidate row


# ---- scores, tolerance, the checker -----------------------------------------------------------
def scores64(Q, C, self_offset=-1):
    """ref.knn_topk's fp64 score matrix [mq, mc]; the self column of every query is -inf."""
    q = np.asarray(Q, dtype=np.float64)[:, :D]
    c = np.asarray(C, dtype=np.float64)[:, :D]
    s = q @ c.T - 0.5 * np.sum(c * c, axis=1)[None, :]
    if self_offset >= 0:
        r = np.arange(q.shape[0])
        s[r, self_offset + r] = -np.inf
    return s


def tolerance(Q, C):
    """tol = 64 * 2^-24 * (|Q| |C|^T + 0.5 ||c||^2), [mq, mc] (see the module docstring)."""
    q = np.abs(np.asarray(Q, dtype=np.float64)[:, :D])
    c = np.asarray(C, dtype=np.float64)[:, :D]
    return 64.0 * 2.0 ** -24 * (q @ np.abs(c).T + 0.5 * np.sum(c * c, axis=1)[None, :])


def _prev_duplicate(C):
    """prev[c] = the largest index below c whose 30 features are bitwise those of row c, or -1."""
    f = np.ascontiguousarray(np.asarray(C, dtype=np.float32)[:, :D]).view(np.uint32)
    _, inv = np.unique(f, axis=0, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    prev = np.full(f.shape[0], -1, dtype=np.int64)
    last = {}
    for i, g in enumerate(inv.tolist()):
        prev[i] = last.get(g, -1)
        last[g] = i
    return prev


def outsider_violations(idx, s, t):
    """[mq] bool: some candidate outside the returned list beats it beyond the tolerance,
    s(c) > min_{i in L}(s(i) + t(i)) + t(c).  ``s`` carries -inf on the self column."""
    idx = np.asarray(idx, dtype=np.int64)
    floor = np.min(np.take_along_axis(s, idx, 1) + np.take_along_axis(t, idx, 1), axis=1)
    out = s - t
    np.put_along_axis(out, idx, -np.inf, 1)
    return np.max(out, axis=1) > floor


def assert_valid_topk(idx, score, Q, C, k, self_offset=-1, s=None, t=None):
    """Every query's list is a top-k some fp32 engine could return: see the checks below.  ``score``
    (or None) holds the device's scores q.c - 0.5||c||^2; ``s`` / ``t`` may pass in precomputed
    ``scores64`` / ``tolerance``."""
    idx = np.asarray(idx).astype(np.int64)
    mq, mc = np.asarray(Q).shape[0], np.asarray(C).shape[0]
    assert idx.shape == (mq, k), idx.shape
    s = scores64(Q, C, self_offset) if s is None else s
    t = tolerance(Q, C) if t is None else t
    rows = np.arange(mq)
    # distinct, in range, never the self row
    assert idx.min() >= 0 and idx.max() < mc, ("index range", int(idx.min()), int(idx.max()))
    srt = np.sort(idx, axis=1)
    assert np.all(srt[:, 1:] != srt[:, :-1]), ("repeated index", np.flatnonzero(np.any(srt[:, 1:] == srt[:, :-1], 1))[:5])
    if self_offset >= 0:
        assert not np.any(idx == (self_offset + rows)[:, None]), "self row returned"
    sl, tl = np.take_along_axis(s, idx, 1), np.take_along_axis(t, idx, 1)
    # no outsider beats the list
    bad = outsider_violations(idx, s, t)
    assert not bad.any(), ("a better candidate was left out", int(bad.sum()), np.flatnonzero(bad)[:5])
    # consecutive entries in order within t
    gap = sl[:, 1:] - sl[:, :-1]
    ok = gap <= tl[:, 1:] + tl[:, :-1]
    assert ok.all(), ("order", np.argwhere(~ok)[:5])
    # bitwise-duplicate candidate rows: smaller index first, and never the larger one alone
    prev = _prev_duplicate(C)
    p = prev[idx]
    if self_offset >= 0:
        is_self = p == (self_offset + rows)[:, None]
        p = np.where(is_self, prev[np.where(p >= 0, p, 0)], p)
    need = p >= 0
    if need.any():
        hit = idx[:, :, None] == p[:, None, :]            # [q, position, entry]
        pos = np.where(hit.any(1), hit.argmax(1), k)      # position of each entry's duplicate, k = absent
        ok = ~need | (pos < np.arange(k)[None, :])
        assert ok.all(), ("duplicate rows out of index order", np.argwhere(~ok)[:5])
    if score is not None:
        sd = np.asarray(score)
        assert sd.shape == (mq, k) and sd.dtype == np.float32
        err = np.abs(sd.astype(np.float64) - sl)
        assert np.all(err <= tl), ("score", float(np.max(err / tl)))
        # bit-equal device scores: the smaller index first
        for a in range(k):
            for b in range(a + 1, k):
                eq = sd[:, a] == sd[:, b]
                assert np.all(idx[eq, a] < idx[eq, b]), ("tie order", a, b, np.flatnonzero(eq & (idx[:, a] >= idx[:, b]))[:5])


# ---- the kernels' operand prep and bf16x3 filter, emulated ------------------------------------
def _f32_chain(terms):
    """fp32 fmaf chain over the last axis of fp64 ``terms`` (each an exact product): acc = float32(acc + term)."""
    acc = np.zeros(terms.shape[:-1], dtype=np.float32)
    for i in range(terms.shape[-1]):
        acc = (acc.astype(np.float64) + terms[..., i]).astype(np.float32)
    return acc


def prep_rows(X, role):
    """knn_prep_kernel's output for unpadded rows: features copied, column 31 zero, column 30 =
    1 (role 1, queries) or -0.5 * the fp32 fmaf-chain norm (role 0, candidates)."""
    X = np.asarray(X, dtype=np.float32)
    out = np.zeros((X.shape[0], 32), dtype=np.float32)
    out[:, :D] = X[:, :D]
    if role == 1:
        out[:, 30] = 1.0
    else:
        x = X[:, :D].astype(np.float64)
        out[:, 30] = np.float32(-0.5) * _f32_chain(x * x)
    return out


def split_hi_lo(Xp):
    """x = hi + lo: hi = bf16(x), lo = bf16(x - hi), both as fp32 arrays."""
    Xp = np.asarray(Xp, dtype=np.float32)
    hi = ref.bf16_round(Xp)
    lo = ref.bf16_round(Xp - hi)
    return hi, lo


def approx_scores(Q, C, kind="approx3"):
    """fp64 emulation of the filter's score over prepped rows: ``approx3`` = hi.hi + hi.lo + lo.hi,
    ``approx_no_query_lo`` = hi.hi + q_hi.c_lo (the query's lo half lost), ``approx_hi_only`` = hi.hi."""
    qh, ql = (a.astype(np.float64) for a in split_hi_lo(prep_rows(Q, 1)))
    ch, cl = (a.astype(np.float64) for a in split_hi_lo(prep_rows(C, 0)))
    a = qh @ ch.T
    if kind in ("approx3", "approx_no_query_lo"):
        a = a + qh @ cl.T
    if kind == "approx3":
        a = a + ql @ ch.T
    elif kind not in ("approx_no_query_lo", "approx_hi_only"):
        raise ValueError(kind)
    return a


def tile_tmax(C):
    """[ceil(mc / 32)] fp64: the kernel's per-32-row bound 1.0001 * max ||c|| (padding rows: norm 0)."""
    c = np.asarray(C, dtype=np.float64)[:, :D]
    n = np.sqrt(np.sum(c * c, axis=1))
    nt = (len(n) + 31) // 32
    n = np.r_[n, np.zeros(nt * 32 - len(n))].reshape(nt, 32)
    return NORM_SLACK * n.max(axis=1)


def margins(Q, C, scale=K_MARGIN_SCALE):
    """[mq, mc] fp64: m = scale * (1.0001 ||q|| * tmax_t + 0.5 tmax_t^2) of the candidate's tile t."""
    q = np.asarray(Q, dtype=np.float64)[:, :D]
    qn = NORM_SLACK * np.sqrt(np.sum(q * q, axis=1))
    tm = np.repeat(tile_tmax(C), 32)[: np.asarray(C).shape[0]]
    return scale * (qn[:, None] * tm[None, :] + 0.5 * tm[None, :] ** 2)


def filter_pass(approx, margin, k, self_offset=-1):
    """[mq, mc] bool: the collect kernel's filter at its FINAL threshold (one slice): thr = the k-th
    best lower bound approx - m, a candidate passes when its upper bound approx + m reaches it."""
    a = np.array(approx, dtype=np.float64)
    if self_offset >= 0:
        r = np.arange(a.shape[0])
        a[r, self_offset + r] = -np.inf
    lb = a - margin
    thr = -np.partition(-lb, k - 1, axis=1)[:, k - 1]
    return (a + margin) >= thr[:, None]


def filtered_topk(passed, s, k):
    """What the exact re-rank returns from the candidates that passed: their fp64 top-k (ties ->
    smaller index).  ``s`` carries -inf on the self column."""
    sc = np.where(passed, s, -np.inf)
    order = np.lexsort((np.broadcast_to(np.arange(s.shape[1]), s.shape), -sc), axis=1)
    return order[:, :k]


# ---- named cases ------------------------------------------------------------------------------
def _rows(F):
    """32-column padded fp32 rows: features, then intercept 1 and label 1 (both ignored by the search)."""
    X = np.ones((F.shape[0], 32), dtype=np.float32)
    X[:, :D] = F.astype(np.float32)
    return X


def _cluster(rng, m, base_norm, cols, sigma):
    b = rng.normal(size=D)
    b *= base_norm / np.linalg.norm(b)
    P = np.zeros((m, D))
    P[:, cols] = rng.normal(0.0, sigma, size=(m, len(cols)))
    return b[None, :] + P


def _lattice(rng):
    """Exact fp32 arithmetic with lo != 0 and near-ties far inside the margin: 1000 spread rows
    (columns 4..29 in {-2, -1.75, .., 2}, columns 0..3 = 16 + j / 16, j in [-16, 16]) and, at random
    positions, 500 tight rows sharing one spread row's columns 4..29 with columns 0..3 =
    16 + {-1, 0, 1} / 16 (81 distinct rows: duplicates by construction).  16 + j / 16 needs 9
    significant bits for odd j > 0, one more than bf16 holds; every product and partial sum of a score
    fits fp32 exactly.  Returns (features [1500, 30], the tight rows' mask)."""
    n_spread, n_tight = 1000, 500
    m = n_spread + n_tight
    grid = np.arange(-2.0, 2.0 + 1e-9, 0.25)
    F = np.empty((m, D))
    tight = np.zeros(m, dtype=bool)
    tight[rng.permutation(m)[:n_tight]] = True
    sp = np.flatnonzero(~tight)
    F[sp, 4:] = rng.choice(grid, size=(n_spread, D - 4))
    F[sp, :4] = 16.0 + rng.integers(-16, 17, size=(n_spread, 4)) / 16.0
    # the row that lends the tight group its columns 4..29 sits at a corner of the lattice, far from
    # every other spread row: the group is then never among a spread query's running best, so only
    # the tight queries themselves fill their lists with it (a group at a typical distance overflowed
    # the lists of ~5 % of the spread queries while their running threshold was still low)
    F[sp[0], 4:] = rng.choice([-2.0, 2.0], size=D - 4)
    ti = np.flatnonzero(tight)
    F[ti, 4:] = F[sp[0], 4:][None, :]
    F[ti, :4] = 16.0 + rng.integers(-1, 2, size=(n_tight, 4)) / 16.0
    return F, tight


CASES = ("normal", "cluster3", "cluster30", "cluster3_far", "heavy", "near_origin", "lattice")


@functools.lru_cache(maxsize=None)
def case(name: str) -> np.ndarray:
    """The case's [m, 32] fp32 rows (read-only; fixed seed)."""
    if name == "normal":
        F = np.random.default_rng(11).normal(size=(1000, D))
    elif name == "cluster3":
        rng = np.random.default_rng(12)
        F = _cluster(rng, 300, 4.0, rng.permutation(D)[:3], 0.5)
    elif name == "cluster30":
        F = _cluster(np.random.default_rng(13), 300, 8.0, np.arange(D), 0.5)
    elif name == "cluster3_far":
        rng = np.random.default_rng(14)
        F = _cluster(rng, 300, 16.0, rng.permutation(D)[:3], 1.0)
    elif name == "heavy":
        F = np.array(case("normal")[:, :D], dtype=np.float64)
        F[:, 7] *= np.exp(1.5 * np.random.default_rng(15).normal(size=F.shape[0]))
    elif name == "near_origin":
        F = 0.05 * np.random.default_rng(16).normal(size=(333, D))
    elif name == "lattice":
        F = _lattice(np.random.default_rng(17))[0]
    else:
        raise KeyError(name)
    X = _rows(F)
    X.setflags(write=False)
    return X


def lattice_built_tight() -> np.ndarray:
    """[m] bool: the 500 rows BUILT tight (within 2^-3 of each other in columns 0..3, equal elsewhere)."""
    return _lattice(np.random.default_rng(17))[1]


def sure_and_possible_pass(Q, C, k, self_offset=-1):
    """([mq, mc] bool, [mq, mc] bool): the candidates that pass the filter at its final threshold
    whatever the approximate error within margin / 4 is, s >= s_k - 1.5 m, and those that can pass at
    all, s >= s_k - 2.5 m.  (lb = approx - m and |approx - s| <= m / 4 put the final threshold, the
    k-th best lb, in [s_k - 1.25 m, s_k - 0.75 m] where m is uniform; the upper bound approx + m is
    in [s + 0.75 m, s + 1.25 m].)"""
    s, m = scores64(Q, C, self_offset), margins(Q, C)
    sk = -np.partition(-s, k - 1, axis=1)[:, k - 1][:, None]
    return s >= sk - 1.5 * m, s >= sk - 2.5 * m


def lane_half(mc: int) -> np.ndarray:
    """[mc] the half h of the wave whose lanes score candidate row c: rows 4h .. 4h + 3 of every 8."""
    return (np.arange(mc) % 8) // 4


@functools.lru_cache(maxsize=None)
def lattice_tight(k: int = 5) -> np.ndarray:
    """[m] bool: the lattice rows that search the tight group AS QUERIES: more than 2 x 64 candidates
    pass their filter for certain (``sure_and_possible_pass``).  For k = 1, 5 and 8 alike these are the
    500 rows built tight and the corner row that lent them its columns 4..29 (test_knn_oracle.py)."""
    X = case("lattice")
    t = sure_and_possible_pass(X, X, k, 0)[0].sum(axis=1) > 128
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def oracle(name: str, self_offset: int = 0, lo: int = 0, hi: int | None = None):
    """(scores64, tolerance) of queries case[lo:hi] against the whole case; read-only, computed once."""
    X = case(name)
    Q = X[lo:hi]
    s, t = scores64(Q, X, self_offset), tolerance(Q, X)
    s.setflags(write=False)
    t.setflags(write=False)
    return s, t
