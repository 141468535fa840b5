"""Inputs and oracles of the streaming-kernel tests (test_stream_oracle.py, test_stream_kernels_gpu.py):
scaler.hip (partial sums, reduce, finalize, scale_cast, the fused stats+cast pass, the fp8 prescale,
the small scan and the per-tile count) and predict.hip (predict, predict+SHAP, gather-logit).

numpy only.  Nothing here calls ops/reference.py: the scaler sums are exact rationals of the float32
inputs, bf16 is rounded by integer arithmetic on the fp32 bits, e4m3 by an exact fp64 quantiser, and
the predict oracles are plain fp64 products of the decoded stored rows.
"""
import functools
from fractions import Fraction

import numpy as np

NCOLS, BIAS_COL, LABEL_COL = 32, 30, 31
ROWS = (1, 7, 8, 9, 63, 64, 65, 127, 128, 129, 1000)
DIMS = (1, 2, 3, 5, 7, 28, 29, 30)
PREDICT_ROWS = ROWS + (15, 16, 17, 255, 256, 257)
# One case past the first grid sweep of every streaming kernel.  The scaler, cast and predict_shap
# grids are capped at 2048 blocks (common.h stream_grid's max_blocks; capped_grid's cap is the
# resident blocks, at most 8 blocks per CU x 256 CUs = 2048) and a block covers at most 128 rows per
# sweep (one 128-row tile; the strided kernels 4 waves x 4 groups x 8 rows): 2048 x 128 = 262 144.
# predict_bf16 / predict_fp8 cover 4 waves x 64 rows = 256 rows per block: 2048 x 256 = 524 288.
SWEEP_ROWS = 262_144 + 137
PREDICT_SWEEP_ROWS = 524_288 + 65
U24, U53 = 2.0 ** -24, 2.0 ** -53
FP8_SCALE = 4.0  # a power of two: v / FP8_SCALE * FP8_SCALE is exact


# ---- the raw table -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _master_table(nmax: int) -> np.ndarray:
    """[nmax, 30] float32, column j of kind j % 7:
    0 ~1e5 +- 1 (the Time column), 1 the constant float32(0.1) (non-dyadic), 2 log-uniform over
    1e-3 .. 1e4, 3 +-0.0, 4 two values one float32 ulp apart at 1e6, 5 the constant 1e7,
    6 N(2.5, 1)."""
    rng = np.random.default_rng(77)
    X = np.empty((nmax, 30), dtype=np.float32)
    for j in range(30):
        k = j % 7
        if k == 0:
            X[:, j] = (1e5 + rng.uniform(-1.0, 1.0, nmax)).astype(np.float32)
        elif k == 1:
            X[:, j] = np.float32(0.1)
        elif k == 2:
            X[:, j] = (10.0 ** rng.uniform(-3.0, 4.0, nmax)).astype(np.float32)
        elif k == 3:
            X[:, j] = np.where(rng.random(nmax) < 0.5, np.float32(0.0), np.float32(-0.0))
        elif k == 4:
            lo = np.float32(1e6)
            X[:, j] = np.where(rng.random(nmax) < 0.5, lo, np.nextafter(lo, np.float32(2e6)))
        elif k == 5:
            X[:, j] = np.float32(1e7)
        else:
            X[:, j] = rng.normal(2.5, 1.0, nmax).astype(np.float32)
    X.setflags(write=False)
    return X


def table(n: int, d: int) -> np.ndarray:
    """The first n rows and d columns of the table (every n <= 1000 is a prefix of one table)."""
    return _master_table(1000 if n <= 1000 else n)[:n, :d]


CONST_KINDS = (1, 5)  # column kinds whose value is one constant


def explicit_pivot(d: int) -> np.ndarray:
    """A pivot row unequal to every row of the table, of each column's own magnitude."""
    per_kind = [1e5 + 2.5, 0.1 + 2.0 ** -10, 100.0, 0.25, 1e6 - 1.0, 1e7 - 3.0, 2.0]
    return np.array([per_kind[j % 7] for j in range(d)], dtype=np.float32)


def labels_case(n: int, rate: float = 0.3, seed: int = 5) -> np.ndarray:
    return (np.random.default_rng(seed).random(max(n, 1))[:n] < rate).astype(np.uint8)


# ---- exact scaler sums -------------------------------------------------------------------------
def _col_moments(col: np.ndarray):
    """(sum x, sum x^2) of a float32 column as exact Fractions.  x = k 2^e with |k| < 2^24: per
    exponent the integers k and k^2 (< 2^48, summed in two 24-bit halves) add exactly in int64."""
    col = np.asarray(col, dtype=np.float32)
    assert np.all(np.isfinite(col))
    m, e = np.frexp(col.astype(np.float64))
    k = np.ldexp(m, 24).astype(np.int64)
    assert np.array_equal(np.ldexp(k.astype(np.float64), e - 24), col.astype(np.float64))
    s1, s2 = Fraction(0), Fraction(0)
    for ev in np.unique(e[k != 0]):
        kk = k[(e == ev) & (k != 0)]
        sq = kk * kk
        unit = Fraction(2) ** (int(ev) - 24)
        s1 += int(kk.sum()) * unit
        s2 += ((int((sq >> 24).sum()) << 24) + int((sq & 0xFFFFFF).sum())) * unit * unit
    return s1, s2


class ExactSums:
    """Exact shifted sums of X [n, d] about ``pivot`` and the exact statistics they define.

    s1, s2: sum (x - p), sum (x - p)^2 rounded to fp64 once.  b1, b2: what any fp64 summation order
    may differ by, (n + 64) 2^-53 sum |x - p| (resp. of the squares): n - 1 additions plus a reduce
    tree of at most 64 levels, each one rounding of a partial sum bounded by the absolute sum."""

    def __init__(self, X: np.ndarray, pivot: np.ndarray | None = None):
        X = np.asarray(X, dtype=np.float32)
        n, d = X.shape
        self.n, self.d = n, d
        self.pivot = np.asarray(X[0] if pivot is None else pivot, dtype=np.float32)[:d].copy()
        F1, F2, M, V = [], [], [], []
        for j in range(d):
            p = Fraction(float(self.pivot[j]))
            t1, t2 = _col_moments(X[:, j])
            F1.append(t1 - n * p)
            F2.append(t2 - 2 * p * t1 + n * p * p)
            mean = t1 / n
            M.append(mean)
            V.append(t2 / n - mean * mean)
        self.F1, self.F2 = F1, F2
        self.s1 = np.array([float(f) for f in F1])
        self.s2 = np.array([float(f) for f in F2])
        D = np.abs(X.astype(np.float64) - self.pivot.astype(np.float64)[None, :])
        self.b1 = (n + 64) * U53 * D.sum(0)
        self.b2 = (n + 64) * U53 * self.s2
        self.mean = np.array([float(f) for f in M])
        self.var = np.array([float(f) for f in V])
        self.var_exact_zero = np.array([f == 0 for f in V])
        # the finalize's own arithmetic on top of sums within b1 / b2: var = s2 / n - m^2, m = s1 / n
        m = np.abs(self.s1) / n
        self.mean_bound = 4.0 * 2.0 ** -52 * np.maximum(np.abs(self.mean), np.abs(self.pivot.astype(np.float64)))
        self.var_bound = (self.b2 + 2.0 * m * self.b1) / n + (self.b1 / n) ** 2 + 8.0 * U53 * (self.s2 / n + m * m)
        # sklearn's near-constant rule (scaler_finalize.h): scale = 1 where var <= ub
        eps = 2.0 ** -52
        self.ub = n * eps * self.var + (n * self.mean * eps) ** 2


@functools.lru_cache(maxsize=None)
def exact_case(n: int, d: int, explicit: bool) -> ExactSums:
    """The exact sums of table(n, d) about row 0 or about explicit_pivot(d); shared, never modified."""
    return ExactSums(table(n, d), explicit_pivot(d) if explicit else None)


def stats_dict(st) -> dict:
    """The arrays of an ops.scaler.ScalerStats on the host."""
    g = {k: getattr(st, k).cpu().numpy() for k in ("mean64", "var64", "scale64", "mean32", "inv32")}
    g["aff"] = None if st.aff is None else st.aff.cpu().numpy()
    return g


def check_sums(sums: np.ndarray, ex: ExactSums) -> None:
    """[64] shifted sums against the exact ones; slots past d are zero (slot 31 may carry a count)."""
    d = ex.d
    sums = np.asarray(sums, dtype=np.float64)
    assert np.all(np.isfinite(sums)), "a poisoned padding value leaked into the sums"
    e1, e2 = np.abs(sums[:d] - ex.s1), np.abs(sums[32:32 + d] - ex.s2)
    assert np.all(e1 <= ex.b1), ("first moment", e1, ex.b1)
    assert np.all(e2 <= ex.b2), ("second moment", e2, ex.b2)
    assert not np.any(sums[d:31]) and not np.any(sums[32 + d:])


def check_stats(got: dict, ex: ExactSums, default_pivot: bool, colscale: np.ndarray | None = None) -> None:
    """mean64 / var64 / scale64 / mean32 / inv32 (and aff) [32] against the exact statistics.

    mean: 4 x 2^-52 max(|mean|, |pivot|) (the rounding of pivot + m and of m).  var: ExactSums.var_bound.
    scale: sqrt(var) to the same relative bound halved, where the exact variance clears the
    near-constant threshold ub by more than var_bound; exactly 1 where it is exactly 0; not
    determined in between (the decision then depends on rounding noise).  mean32, inv32 and aff
    are functions of the fp64 outputs and are checked bitwise against them."""
    d = ex.d
    mean, var, scale = (np.asarray(got[k], dtype=np.float64) for k in ("mean64", "var64", "scale64"))
    assert np.all(np.abs(mean[:d] - ex.mean) <= ex.mean_bound), ("mean", mean[:d] - ex.mean, ex.mean_bound)
    assert np.all(np.abs(var[:d] - ex.var) <= ex.var_bound), ("var", var[:d] - ex.var, ex.var_bound)
    assert np.all(var[:d] >= 0.0)
    for j in range(d):
        if ex.var_exact_zero[j] and default_pivot:
            # every x equals the pivot: all shifted terms are exactly zero
            assert var[j] == 0.0 and scale[j] == 1.0 and mean[j] == float(ex.pivot[j]), (j, mean[j], var[j], scale[j])
        elif ex.var[j] - ex.var_bound[j] > 2.0 * ex.ub[j] and ex.var_bound[j] < 0.25 * ex.var[j]:
            rel = ex.var_bound[j] / ex.var[j] + 4.0 * U53  # d sqrt(v) / sqrt(v) = dv / 2v, doubled; sqrt rounding
            assert abs(scale[j] - np.sqrt(ex.var[j])) <= rel * np.sqrt(ex.var[j]), (j, scale[j], np.sqrt(ex.var[j]))
        else:
            assert scale[j] == 1.0 or scale[j] == np.sqrt(var[j]), (j, scale[j], var[j])
    assert not np.any(mean[d:]) and not np.any(var[d:]) and np.all(scale[d:] == 1.0)
    m32, i32 = np.asarray(got["mean32"]), np.asarray(got["inv32"])
    assert m32.dtype == np.float32 and i32.dtype == np.float32
    assert np.array_equal(m32, mean.astype(np.float32))
    exp_inv = np.zeros(32, dtype=np.float32)
    exp_inv[:d] = (1.0 / scale[:d]).astype(np.float32)
    assert np.array_equal(i32, exp_inv)
    if got.get("aff") is not None:
        aff = np.asarray(got["aff"], dtype=np.float64)
        k = np.ones(32)
        if colscale is not None:
            k[:d] = np.asarray(colscale, dtype=np.float32)[:d].astype(np.float64)
        # aff[c] = m k with m = s1 / n: the sum bound over n, one division and one product rounding
        m = ex.s1 / ex.n
        tol = (ex.b1 / ex.n + 4.0 * U53 * np.abs(m)) * k[:d]
        assert np.all(np.abs(aff[:d] - m * k[:d]) <= tol), ("aff c", aff[:d] - m * k[:d], tol)
        assert np.array_equal(aff[32:32 + d], 1.0 / scale[:d] / k[:d])
        assert not np.any(aff[d:32]) and np.all(aff[32 + d:] == 1.0)


# ---- bf16 --------------------------------------------------------------------------------------
def bf16_bits(x: np.ndarray) -> np.ndarray:
    """uint16 bf16 of float32 values, round to nearest even on the fp32 bits; NaN stays NaN."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = (b + np.uint64(0x7FFF) + ((b >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)
    nan = (b & np.uint64(0x7FFFFFFF)) > np.uint64(0x7F800000)
    r = np.where(nan, (b >> np.uint64(16)) | np.uint64(0x40), r)
    return r.astype(np.uint16)


def bf16_values(bits: np.ndarray) -> np.ndarray:
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def bf16_equal(got_bits: np.ndarray, exp_bits: np.ndarray) -> bool:
    """Bitwise, except that any NaN matches any NaN (the payload is not specified)."""
    g, e = np.asarray(got_bits, dtype=np.uint16), np.asarray(exp_bits, dtype=np.uint16)
    gn, en = np.isnan(bf16_values(g)), np.isnan(bf16_values(e))
    return bool(np.array_equal(gn, en) and np.array_equal(g[~gn], e[~en]))


def bf16_ties() -> np.ndarray:
    """float32 values with low half 0x8000 (exact bf16 ties): odd and even upper halves, both
    signs, from the smallest normal exponent to the largest finite one (whose top tie rounds to inf)."""
    uppers = []
    for ex in (0x01, 0x70, 0x7E, 0x7F, 0x80, 0x85, 0x8A, 0x96, 0xFE):  # the 8-bit exponent field
        for mant in (0x00, 0x01, 0x02, 0x7E, 0x7F):
            uppers.append((ex << 7) | mant)
    up = np.array(uppers, dtype=np.uint32)
    up = np.concatenate([up, up | np.uint32(0x8000)])
    v = ((up << np.uint32(16)) | np.uint32(0x8000)).view(np.float32)
    return v[np.isfinite(v)]


def bf16_sweep() -> np.ndarray:
    """Every tie pattern (all 65536 upper halves with low half 0x8000) and its two fp32 neighbours."""
    up = np.arange(65536, dtype=np.uint32) << np.uint32(16)
    return np.concatenate([up | np.uint32(0x7FFF), up | np.uint32(0x8000), up | np.uint32(0x8001), up]).view(np.float32)


# ---- fp8 e4m3 (OCP, satfinite) -----------------------------------------------------------------
def fp8_decode(codes: np.ndarray) -> np.ndarray:
    """fp64 values of e4m3 codes (0x7f / 0xff: NaN)."""
    b = np.asarray(codes, dtype=np.uint8).astype(np.int64)
    e, m = (b >> 3) & 15, b & 7
    v = np.where(e == 0, m * 2.0 ** -9, (8 + m) * np.exp2((e - 10).astype(np.float64)))
    v = np.where((e == 15) & (m == 7), np.nan, v)
    return np.where(b & 0x80, -v, v)


def fp8_encode(x: np.ndarray) -> np.ndarray:
    """uint8 e4m3 codes of float32 values, RNE + satfinite, vectorised: |x| is quantised in fp64 to
    its binade's step 2^(e-3) (e >= -6: the subnormals share the smallest normal binade's step) with
    rint, which rounds ties to even; the code is then (e + 7) << 3 plus q - 8, carries included."""
    x = np.asarray(x, dtype=np.float32)
    a = np.abs(x).astype(np.float64)
    fin = np.isfinite(a)
    _, ex = np.frexp(np.where(fin, a, 1.0))
    e = np.where(a == 0.0, -6, np.maximum(ex - 1, -6))  # frexp(0) has exponent 0
    q = np.rint(np.ldexp(np.where(fin, a, 1.0), 3 - e)).astype(np.int64)
    code = ((e + 7).astype(np.int64) << 3) + q - 8
    code = np.where((a >= 2.0 ** 10) | ~fin, 0x7E, np.minimum(code, 0x7E))  # satfinite (also keeps `code` small)
    code = np.where(np.isnan(x), 0x7F, code)
    return (code | (np.signbit(x).astype(np.int64) << 7)).astype(np.uint8)


def fp8_nearest(x: np.ndarray) -> np.ndarray:
    """The definition, by search: the code of the nearest finite e4m3 magnitude (127 of them per
    sign; 253 distinct values with +-0 merged), ties to the even code, the sign bit kept (so +-0 stay
    apart), everything past the largest finite value saturating to it."""
    x = np.asarray(x, dtype=np.float32)
    mags = fp8_decode(np.arange(0x7F, dtype=np.uint8))  # ascending
    a = np.abs(x).astype(np.float64).reshape(-1)
    a = np.where(np.isfinite(a), np.minimum(a, 1e6), 1e6)
    hi = np.clip(np.searchsorted(mags, a, side="left"), 1, 0x7E)
    lo = hi - 1
    dl, dh = a - mags[lo], mags[hi] - a  # exact: float32 inputs, 4-bit grid values
    pick = np.where(dl < dh, lo, np.where(dh < dl, hi, np.where(lo % 2 == 0, lo, hi)))
    code = np.where(np.isnan(x.reshape(-1)), 0x7F, pick)
    return (code | (np.signbit(x.reshape(-1)).astype(np.int64) << 7)).astype(np.uint8).reshape(x.shape)


def fp8_midpoints() -> np.ndarray:
    """Every midpoint between adjacent finite e4m3 magnitudes with its two float32 neighbours, both
    signs (all exactly representable in float32)."""
    mags = fp8_decode(np.arange(0x7F, dtype=np.uint8))
    mid = ((mags[:-1] + mags[1:]) / 2.0).astype(np.float32)
    assert np.array_equal(mid.astype(np.float64), (mags[:-1] + mags[1:]) / 2.0)
    inf = np.float32(np.inf)
    v = np.concatenate([mid, np.nextafter(mid, inf), np.nextafter(mid, -inf)])
    return np.concatenate([v, -v])


def fp8_edges() -> np.ndarray:
    """The midpoint sweep plus |v| at 2^-10, 2^-9, 2^-6, 448, 463.9, 464, 1e6, and -0.0 / +0.0."""
    e = np.array([2.0 ** -10, 2.0 ** -9, 2.0 ** -6, 448.0, 463.9, 464.0, 1e6], dtype=np.float32)
    return np.concatenate([fp8_midpoints(), e, -e, np.array([-0.0, 0.0], dtype=np.float32)])


def fp8_is_tie(x: np.ndarray) -> np.ndarray:
    """True where a float32 lies exactly half-way between two adjacent finite e4m3 values."""
    a = np.abs(np.asarray(x, dtype=np.float32)).astype(np.float64)
    _, ex = np.frexp(np.where(a > 0, a, 1.0))
    t = np.ldexp(np.minimum(a, 1024.0), 3 - np.maximum(ex - 1, -6))
    return (a < 464.0) & (t - np.floor(t) == 0.5)


# ---- scale_cast / fused cast -------------------------------------------------------------------
def cast_table(n: int, d: int, fp8_scale: float = FP8_SCALE) -> np.ndarray:
    """The raw table with the rounding edges injected: every third cell (row-major) cycles through
    the bf16 ties and the e4m3 edge set divided by fp8_scale, so that under identity statistics the
    output bits are the edges' own roundings."""
    X = np.array(table(n, d), dtype=np.float32)
    ties = bf16_ties()
    if n > 1000:  # room for every tie pattern, subnormals included
        ties = bf16_sweep()[65536:131072]
        ties = ties[np.isfinite(ties)]
    edges = np.concatenate([ties, fp8_edges() / np.float32(fp8_scale)]).astype(np.float32)
    flat = X.reshape(-1)
    cells = np.arange(0, flat.shape[0], 3)
    flat[cells] = edges[(cells // 3 + 11 * n + d) % edges.shape[0]]
    return X


def store(vals: np.ndarray, kind: str) -> np.ndarray:
    """float32 row values -> stored elements: float32, bf16 bits (uint16) or e4m3 codes (uint8)."""
    if kind == "f32":
        return np.asarray(vals, dtype=np.float32)
    return bf16_bits(vals) if kind == "bf16" else fp8_encode(vals)


def cast_oracle(X, mean32, inv32, labels, bias_value, kind, fp8_scale=FP8_SCALE, idx=None) -> np.ndarray:
    """scale_cast's padded rows: (x - mean) * inv in float32 (two rounded operations, as the kernel:
    a subtraction feeding a product is not contractible), zeros in d..29, the bias, the label of the
    SOURCE row; fp8 multiplies the features by fp8_scale in float32 before encoding."""
    X = np.asarray(X, dtype=np.float32)
    src = np.arange(X.shape[0]) if idx is None else np.asarray(idx, dtype=np.int64)
    d = X.shape[1]
    out = np.zeros((src.shape[0], NCOLS), dtype=np.float32)
    with np.errstate(over="ignore"):  # the largest bf16 tie times fp8_scale overflows, as on the device
        out[:, :d] = (X[src] - np.asarray(mean32, np.float32)[None, :d]) * np.asarray(inv32, np.float32)[None, :d]
        if kind == "fp8":
            out[:, :d] *= np.float32(fp8_scale)
    out[:, BIAS_COL] = np.float32(bias_value)
    if labels is not None:
        out[:, LABEL_COL] = np.asarray(labels)[src].astype(np.float32)
    return store(out, kind)


def fused_values(X, pivot, labels, bias_value, kind, ks=None) -> np.ndarray:
    """The float32 row values the fused pass rounds (see fused_oracle), in source-row order."""
    X = np.asarray(X, dtype=np.float32)
    n, d = X.shape
    o = np.zeros((n, NCOLS), dtype=np.float32)
    o[:, :d] = X - np.asarray(pivot, np.float32)[None, :d]
    if kind == "fp8":
        o[:, :d] *= np.asarray(ks, dtype=np.float32)[None, :d]
    o[:, BIAS_COL] = np.float32(bias_value)
    if labels is not None:
        o[:, LABEL_COL] = np.asarray(labels).astype(np.float32)
    return o


def fused_oracle(X, pivot, labels, bias_value, kind, ks=None, out_idx=None) -> np.ndarray:
    """scaler_fit_cast's rows: bf16 of x - pivot, or e4m3 of (x - p) * ks in float32 with
    ks = colscale * fp8_scale formed in float32 first (the kernel's operation order); row i lands in
    out[out_idx[i]]."""
    st = store(fused_values(X, pivot, labels, bias_value, kind, ks), kind)
    if out_idx is None:
        return st
    out = np.empty_like(st)
    out[np.asarray(out_idx, dtype=np.int64)] = st
    return out


def gather_idx(n_out: int, n_src: int, seed: int = 3) -> np.ndarray:
    """int64 [n_out] source rows: out of order, with repeats, including n_src - 1 and leaving
    some source rows unused (those are poisoned)."""
    rng = np.random.default_rng(seed + n_out)
    pool = np.arange(0, n_src, 2)  # odd rows stay unused (except the last)
    idx = rng.choice(pool, size=n_out, replace=True)
    idx[0] = n_src - 1
    if n_out > 2:
        idx[-1] = idx[1]
    return idx.astype(np.int64)


def sample_moments(X: np.ndarray, sample_rows: int):
    """(stride, ns, mean [d], 1/std [d]) of the fp8 prescale: rows 0, stride, ... in fp64, population
    std, k = 1 on a constant column."""
    n = X.shape[0]
    stride = max(1, n // max(1, sample_rows))
    ns = min(sample_rows, (n - 1) // stride + 1)
    smp = np.asarray(X[::stride][:ns], dtype=np.float64)
    dd = smp - smp[0][None, :]
    mu = smp[0] + dd.mean(0)
    var = (dd * dd).mean(0) - dd.mean(0) ** 2
    const = np.all(smp == smp[0][None, :], axis=0)
    k = np.where(const, 1.0, 1.0 / np.sqrt(np.where(const, 1.0, var)))
    return stride, ns, mu, k


# ---- predict -----------------------------------------------------------------------------------
SMALL_W_COL = 3  # the column whose weight is 1e-4


def predict_weights(d: int = 30) -> np.ndarray:
    """[32] weights exact in fp32: N(0, 0.3) features with one weight of 1e-4, intercept -1.5 and a
    NON-ZERO label slot, which the kernels must ignore."""
    w = np.zeros(32)
    w[:d] = np.random.default_rng(8).normal(0, 0.3, d)
    w[min(SMALL_W_COL, d - 1)] = 1e-4
    w[BIAS_COL], w[LABEL_COL] = -1.5, 7.0
    return w.astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def _predict_master(kind: str):
    """(stored rows, decoded model-space fp64 rows) of PREDICT_SWEEP_ROWS rows: features N(0, 1.5),
    column 30 = 1, random labels in column 31."""
    n = PREDICT_SWEEP_ROWS
    rng = np.random.default_rng(31 if kind == "bf16" else 32)
    r = (rng.standard_normal((n, 32), dtype=np.float32) * np.float32(1.5))
    r[:, BIAS_COL] = 1.0
    r[:, LABEL_COL] = (rng.random(n) < 0.3).astype(np.float32)
    if kind == "bf16":
        rows = bf16_bits(r)
        R = bf16_values(rows).astype(np.float64)
    else:
        r[:, :30] *= np.float32(FP8_SCALE)
        rows = fp8_encode(r)
        R = fp8_decode(rows)
        R[:, :30] /= FP8_SCALE
    rows.setflags(write=False)
    R.setflags(write=False)
    return rows, R


def predict_rows_case(n: int, kind: str):
    rows, R = _predict_master(kind)
    return rows[:n], R[:n]


def predict_oracle(R: np.ndarray, w: np.ndarray):
    """(z, bound): the fp64 logit over columns 0..30 (the label column never counts) and what an
    fp32 evaluation may differ by: 40 x 2^-24 sum_j |w_j x_j| -- gamma_32 of a 32-term fma chain in
    any order, plus the butterfly's additions."""
    w = np.asarray(w, dtype=np.float64).copy()
    w[LABEL_COL] = 0.0
    T = np.asarray(R, dtype=np.float64) * w[None, :]
    return T.sum(1), 40.0 * U24 * np.abs(T).sum(1)


def sigmoid64(z):
    z = np.asarray(z, dtype=np.float64)
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-z))


def check_prob(p: np.ndarray, z: np.ndarray) -> None:
    """Probabilities against the fp64 sigmoid of the kernel's OWN float32 logit.  |z| <= 80:
    relative (|z| + 4) 2^-23 -- the exp2 argument z log2(e) is rounded to fp32 (relative 2^-24 of an
    exponent, i.e. |z| 2^-24 of the result), then v_exp_f32, the add and v_rcp_f32 at one ulp each;
    the sum doubled.  Beyond (and at +-inf) the result saturates: exactly 0 or 1, never NaN."""
    p = np.asarray(p, dtype=np.float64)
    z = np.asarray(z, dtype=np.float64)
    assert not np.any(np.isnan(p))
    mid = np.abs(z) <= 80.0
    s = sigmoid64(z[mid])
    assert np.all(np.abs(p[mid] - s) <= (np.abs(z[mid]) + 4.0) * 2.0 ** -23 * s), \
        float(np.max(np.abs(p[mid] - s) / ((np.abs(z[mid]) + 4.0) * 2.0 ** -23 * s)))
    far = np.abs(z) >= 200.0
    assert np.array_equal(p[far], (z[far] > 0).astype(np.float64))
    rest = ~mid & ~far
    assert np.all((p[rest] >= 0.0) & (p[rest] <= 1.0))


def shap_case(n: int, ld: int, dd: int, seed: int = 0):
    """Raw rows [n, ld] float32: N(1, 2) in columns < dd, NaN poison from dd on."""
    rng = np.random.default_rng(900 + seed)
    X = np.full((n, ld), np.nan, dtype=np.float32)
    X[:, :dd] = rng.normal(1.0, 2.0, (n, dd)).astype(np.float32)
    return X


def shap_params(seed: int = 1):
    """(a [32], c [32], bias): fp32-exact folded weights (one of 1e-4), background and intercept."""
    rng = np.random.default_rng(seed)
    a = rng.normal(0, 0.4, 32)
    a[SMALL_W_COL] = 1e-4
    c = rng.normal(0.5, 1.0, 32)
    return (a.astype(np.float32).astype(np.float64), c.astype(np.float32).astype(np.float64),
            float(np.float32(-0.75)))


def shap_oracle(X: np.ndarray, a, c, bias: float, dz: int, dphi: int):
    """(z, z_bound, phi, phi_bound) in fp64 from rows X (already decoded).  Logit as predict_oracle
    over dz terms and the bias; phi_j = a_j (x_j - c_j) within 4 x 2^-24 |a_j| (|x_j| + |c_j|): the
    rounding of the difference and of the product, doubled."""
    X = np.asarray(X, dtype=np.float64)
    a, c = np.asarray(a, dtype=np.float64), np.asarray(c, dtype=np.float64)
    T = X[:, :dz] * a[None, :dz]
    z = T.sum(1) + bias
    zb = 40.0 * U24 * (np.abs(T).sum(1) + abs(bias))
    phi = a[None, :dphi] * (X[:, :dphi] - c[None, :dphi])
    pb = 4.0 * U24 * np.abs(a[None, :dphi]) * (np.abs(X[:, :dphi]) + np.abs(c[None, :dphi]))
    return z, zb, phi, pb


def gather_logit_oracle(X: np.ndarray, idx: np.ndarray, w: np.ndarray, mean: np.ndarray, scale: np.ndarray, d: int):
    """(z, bound) of predict_gather_logit: the fp64 fold a = w / scale, bias = w_30 - sum a mean over
    the gathered rows; the predict bound plus the float32 rounding of a and of the bias
    (2^-24 of every product and of the bias, on top of the 40 x 2^-24 chain bound)."""
    a = np.asarray(w, dtype=np.float64)[:d] / np.asarray(scale, dtype=np.float64)[:d]
    bias = float(w[BIAS_COL] - np.sum(a * np.asarray(mean, dtype=np.float64)[:d]))
    T = np.asarray(X, dtype=np.float64)[np.asarray(idx)][:, :d] * a[None, :]
    z = T.sum(1) + bias
    return z, 41.0 * U24 * (np.abs(T).sum(1) + abs(bias))
