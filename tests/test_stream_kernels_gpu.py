"""Every kernel path of scaler.hip and predict.hip (the persistent serving kernel apart) against the
exact oracles of _stream_cases.py, at the smallest shapes that can break it, on MI355X.

Which test launches which kernel (the intended launcher branch is re-derived from ld and the base
address in every test, so a silent fall-through to another kernel fails it):

  scaler_partial_tiled_kernel                 test_scaler_partial_sums[tiled-*], ..._second_sweep[tiled]
  scaler_partial_kernel<4> / <2> / <1>        test_scaler_partial_sums[vec4 / vec2 / vec1, vec1_off -*],
                                              test_scaler_partial_second_sweep[vec4 / vec2 / vec1]
  scaler_reduce_kernel (one and two levels)   test_scaler_reduce_dyadic, every scaler_partial / fit test
  scaler_finalize_kernel                      test_scaler_fit[*], test_scaler_fit_nan_column, test_scaler_fit_cast[*]
  scale_cast_tiled_kernel<0 / 1 / 2>          test_scale_cast[tiled-bf16 / f32 / fp8-plain], ..._second_sweep[tiled-*]
  scale_cast_kernel<VEC, OUT> (all nine)      test_scale_cast[vec4 / vec2 / vec1 / vec1_off - kind - plain / gather],
                                              test_scale_cast_second_sweep[vec4 / vec2 / vec1 - kind]
  scaler_stats_cast_kernel<0, FP8, IDX, MIN>  test_scaler_fit_cast[bf16 / fp8 - plain / scatter / minority - d],
                                              test_scaler_fit_cast_second_sweep[*] (minority_overflow: past the
                                              row buffer's capacity), test_scaler_fit_cast_refuses_strided_rows
  sample_partial_kernel, sample_finalize_kernel   test_fp8_prescale[*] (and every fp8 test_scaler_fit_cast)
  fp8_hw_check_kernel (v_cvt_pk_fp8_f32)      test_fp8_hardware_encode_midpoint_sweep
  exclusive_scan_small_kernel                 test_exclusive_scan_small, test_compact_count_tiles
  compact_count_tiles_kernel                  test_compact_count_tiles, test_scaler_fit_cast[*-minority-*]
  predict_kernel<4> / <2>                     test_predict_rows[bf16 / fp8], test_predict_rows_second_sweep,
                                              test_predict_saturation
  predict_shap_kernel<0,1> <1,4> <1,2> <1,1>  test_predict_shap[bf16 / vec4_* / vec2_d30 / vec1_*-...],
                                              test_predict_shap_second_sweep[*]
  predict_shap_kernel<1,2,double> <1,1,double>    test_predict_h2h[30 / 31]
  predict_gather_logit_kernel                 test_predict_gather_logit[*]

Every tolerance is zero (bitwise) or carries its derivation where it is defined in _stream_cases.py.
"""
import functools

import numpy as np
import pytest
import torch

import _stream_cases as C
from fraud_detection_amd.ops import predict as P
from fraud_detection_amd.ops import scaler as S
from fraud_detection_amd.ops.native import native, ptr, stream_of

pytestmark = pytest.mark.gpu

# layout -> (row stride in floats, 0: ld = d; base offset in floats)
LAYOUTS = {"tiled": (0, 0), "vec4": (32, 0), "vec2": (34, 0), "vec1": (33, 0), "vec1_off": (0, 1)}
INTENDED = {"tiled": "tiled", "vec4": "vec4", "vec2": "vec2", "vec1": "vec1", "vec1_off": "vec1"}


def _view(X: np.ndarray, layout: str, dev, poison_rows=None) -> torch.Tensor:
    """X [n, d] on the device as the [:, :d] view of an [n, ld] buffer at a base offset; the padding
    columns, the offset slot and the rows ``poison_rows`` hold NaN."""
    n, d = X.shape
    ld, off = LAYOUTS[layout]
    ld = ld or d
    buf = np.full(n * ld + off + 3, np.nan, dtype=np.float32)
    v = buf[off:off + n * ld].reshape(n, ld)
    v[:, :d] = X
    if poison_rows is not None:
        v[poison_rows] = np.nan
    t = torch.from_numpy(buf).to(dev)
    assert t.data_ptr() % 256 == 0
    return t[off:off + n * ld].view(n, ld)[:, :d]


def _path(X: torch.Tensor, gather: bool = False) -> str:
    """The branch launch_scaler_partial / launch_scale_cast take for this view (scaler.hip vec_for)."""
    ld, d, a = X.stride(0), X.shape[1], X.data_ptr()
    if not gather and ld == d and d <= 30 and a % 16 == 0:
        return "tiled"
    if ld % 4 == 0 and a % 16 == 0:
        return "vec4"
    if ld % 2 == 0 and a % 8 == 0:
        return "vec2"
    return "vec1"


def _dev(a: np.ndarray, dev) -> torch.Tensor:
    return torch.from_numpy(np.array(a)).to(dev)


def _bits(t: torch.Tensor) -> np.ndarray:
    """Stored elements of a row buffer on the host: float32, bf16 bits (uint16) or e4m3 codes."""
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    return t.cpu().numpy()


_STORAGE = {"f32": (torch.float32, np.uint32, 0x7FC01234), "bf16": (torch.bfloat16, np.uint16, 0x7FC1),
            "fp8": (torch.uint8, np.uint8, 0xFF)}
_INT_OF = {np.uint32: np.int32, np.uint16: np.int16, np.uint8: np.uint8}


def _framed_out(n: int, kind: str, dev):
    """(whole buffer, its rows 1 .. n): the output rows with one NaN canary row before and after."""
    tdt, ndt, pat = _STORAGE[kind]
    raw = np.full((n + 2, 32), pat, dtype=ndt).view(_INT_OF[ndt])
    whole = torch.from_numpy(raw).to(dev).view(tdt)
    return whole, whole[1:n + 1]


def _canaries_intact(whole: torch.Tensor, kind: str) -> bool:
    _, ndt, pat = _STORAGE[kind]
    w = whole.view({"f32": torch.int32, "bf16": torch.int16, "fp8": torch.uint8}[kind]).cpu().numpy().view(ndt)
    return bool(np.all(w[0] == pat) and np.all(w[-1] == pat))


def _rows_equal(got: np.ndarray, exp: np.ndarray, kind: str) -> bool:
    if kind == "bf16":
        return C.bf16_equal(got, exp)
    if kind == "f32":
        return bool(np.array_equal(got.view(np.uint32), exp.view(np.uint32)))
    return bool(np.array_equal(got, exp))


# ---- A. scaler_partial + scaler_reduce ---------------------------------------------------------
@pytest.mark.parametrize("d", C.DIMS)
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_scaler_partial_sums(dev, layout, d):
    for explicit in (False, True):
        for n in C.ROWS:
            ex = C.exact_case(n, d, explicit)
            X = _view(C.table(n, d), layout, dev)
            assert _path(X) == INTENDED[layout], (n, d, X.stride(0), X.data_ptr() % 16)
            sums = S.scaler_partial_sums(X, _dev(ex.pivot, dev)).cpu().numpy()
            C.check_sums(sums, ex)


@functools.lru_cache(maxsize=None)
def _sweep_exact() -> C.ExactSums:
    return C.ExactSums(C.table(C.SWEEP_ROWS, 30), C.explicit_pivot(30))


@pytest.mark.parametrize("layout", ["tiled", "vec4", "vec2", "vec1"])
def test_scaler_partial_second_sweep(dev, layout):
    ex = _sweep_exact()
    X = _view(C.table(C.SWEEP_ROWS, 30), layout, dev)
    assert _path(X) == INTENDED[layout]
    C.check_sums(S.scaler_partial_sums(X, _dev(ex.pivot, dev)).cpu().numpy(), ex)


@pytest.mark.parametrize("nblocks", [1, 127, 128, 129, 2048])
def test_scaler_reduce_dyadic(dev, nblocks):
    """Dyadic partials (integers / 8 below 2^20): every partial sum is exact in fp64, so the fixed
    tree gives the exact total bitwise whatever its shape (one level up to 128 blocks, then two)."""
    m = native()
    rng = np.random.default_rng(nblocks)
    part = rng.integers(-2 ** 20, 2 ** 20, (nblocks, 64)).astype(np.float64) / 8.0
    scratch = m.scaler_reduce_scratch_rows(nblocks)
    assert scratch == (0 if nblocks <= 128 else (nblocks + 127) // 128)
    buf = torch.full(((nblocks + scratch) * 64,), float("nan"), dtype=torch.float64, device=dev)
    buf[: nblocks * 64] = _dev(part.reshape(-1), dev)
    sums = torch.full((64,), float("nan"), dtype=torch.float64, device=dev)
    m.scaler_reduce(ptr(buf), nblocks, ptr(sums), stream_of(buf))
    assert np.array_equal(sums.cpu().numpy(), part.sum(0))
    assert np.array_equal(buf[: nblocks * 64].cpu().numpy(), part.reshape(-1))  # the inputs stay


# ---- B. finalize -------------------------------------------------------------------------------
@pytest.mark.parametrize("d", C.DIMS)
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_scaler_fit(dev, layout, d):
    for explicit in (False, True):
        for n in C.ROWS:  # n = 1 included: every column is constant, exactly
            ex = C.exact_case(n, d, explicit)
            X = _view(C.table(n, d), layout, dev)
            assert _path(X) == INTENDED[layout]
            st = S.scaler_fit(X, pivot=_dev(ex.pivot, dev) if explicit else None)
            C.check_stats(C.stats_dict(st), ex, default_pivot=not explicit)
            assert st.n == float(n)


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_scaler_fit_nan_column(dev, layout):
    """A NaN in one column makes that column's statistics NaN and leaves every other column's bits."""
    X = np.array(C.table(129, 7))
    base = C.stats_dict(S.scaler_fit(_view(X, layout, dev)))
    X[77, 2] = np.nan
    got = C.stats_dict(S.scaler_fit(_view(X, layout, dev)))
    keep = np.arange(32) != 2
    for k in ("mean64", "var64", "scale64", "mean32", "inv32"):
        assert np.isnan(got[k][2]), k
        assert np.array_equal(got[k][keep], base[k][keep]), k


# ---- C. scale_cast -----------------------------------------------------------------------------
def _cast_stats(d: int, ident: bool, dev):
    if ident:
        return S.stats_from_numpy(np.zeros(d), np.ones(d), device=dev)
    return S.stats_from_numpy(C.explicit_pivot(d).astype(np.float64), 0.75 + 0.03125 * np.arange(d), device=dev)


def _check_scale_cast(dev, X, layout, kind, st, labels, bias, idx, intended):
    """One launch: X [n_src, d] (cast table), idx None or the gathered source rows."""
    n_src, d = X.shape
    n_out = n_src if idx is None else idx.shape[0]
    unused = None
    if idx is not None:
        unused = np.ones(n_src, dtype=bool)
        unused[idx] = False
    Xd = _view(X, layout, dev, poison_rows=unused)
    assert _path(Xd, gather=idx is not None) == intended, (n_src, d, layout)
    yd = None
    if labels is not None:
        y = labels.copy()
        if unused is not None:
            y[unused] = 200  # a label read from the OUTPUT row's position would show
        yd = _dev(y, dev)
    whole, out = _framed_out(n_out, kind, dev)
    kw = {} if bias is None else {"bias_value": bias}
    r = S.scale_cast(Xd, st, labels=yd, out_dtype=kind, out=out, idx=None if idx is None else _dev(idx, dev),
                     fp8_scale=C.FP8_SCALE, **kw)
    assert r.data_ptr() == out.data_ptr()
    exp = C.cast_oracle(X, st.mean32.cpu().numpy(), st.inv32.cpu().numpy(), labels, 1.0 if bias is None else bias,
                        kind, C.FP8_SCALE, idx)
    got = _bits(out)
    assert _rows_equal(got, exp, kind), (n_src, d, layout, kind, np.argwhere(got != exp)[:4])
    zero = C.store(np.zeros(1, dtype=np.float32), kind)[0]
    assert np.all(got[:, d:30] == zero)  # +0 in every unused feature column
    assert _canaries_intact(whole, kind)


@pytest.mark.parametrize("form", ["plain", "gather"])
@pytest.mark.parametrize("kind", ["bf16", "f32", "fp8"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_scale_cast(dev, layout, kind, form):
    """Bitwise over the whole table: f32 exactly, bf16 by the integer RNE, fp8 by the vectorised
    encoder including the sign of zero (these kernels use the software encoder).  Identity statistics
    on the table with the rounding edges injected, so the output bits are the edges' own roundings;
    real statistics too at three row counts.  A gather never takes the tiled kernel."""
    if layout == "tiled" and form == "gather":
        layouts = {28: "vec4", 30: "vec2", 2: "vec2"}  # contiguous rows under idx: vec_for(ld = d)
    for d in C.DIMS:
        intended = INTENDED[layout]
        if layout == "tiled" and form == "gather":
            intended = layouts.get(d, "vec1")
        for n in C.ROWS:
            n_src = n + 5 if form == "gather" else n
            idx = C.gather_idx(n, n_src) if form == "gather" else None
            labels = None if n in (8, 64, 128) else C.labels_case(n_src)
            bias = None if n == 1000 else -2.5
            _check_scale_cast(dev, C.cast_table(n_src, d), layout, kind, _cast_stats(d, True, dev), labels, bias, idx,
                              intended)
            if n in (9, 129, 1000):
                _check_scale_cast(dev, np.array(C.table(n_src, d)), layout, kind, _cast_stats(d, False, dev), labels,
                                  bias, idx, intended)


@functools.lru_cache(maxsize=None)
def _sweep_cast_oracle(kind: str) -> np.ndarray:
    X = C.cast_table(C.SWEEP_ROWS, 30)
    return C.cast_oracle(X, np.zeros(30, np.float32), np.ones(30, np.float32), C.labels_case(C.SWEEP_ROWS), -2.5, kind)


@pytest.mark.parametrize("kind", ["bf16", "f32", "fp8"])
@pytest.mark.parametrize("layout", ["tiled", "vec4", "vec2", "vec1"])
def test_scale_cast_second_sweep(dev, layout, kind):
    """Past 2048 blocks x 128 rows; the table cycles through every bf16 tie pattern (subnormals too)."""
    n = C.SWEEP_ROWS
    Xd = _view(C.cast_table(n, 30), layout, dev)
    assert _path(Xd) == INTENDED[layout]
    whole, out = _framed_out(n, kind, dev)
    S.scale_cast(Xd, _cast_stats(30, True, dev), labels=_dev(C.labels_case(n), dev), out_dtype=kind, out=out,
                 bias_value=-2.5, fp8_scale=C.FP8_SCALE)
    assert _rows_equal(_bits(out), _sweep_cast_oracle(kind), kind)
    assert _canaries_intact(whole, kind)


# ---- D. scaler_fit_cast (fused) and the fp8 prescale -------------------------------------------
@functools.lru_cache(maxsize=4)
def _exact_about(n: int, d: int, pivot_bytes: bytes) -> C.ExactSums:
    """Exact sums of table(n, d) about a pivot given as bytes (one evaluation per distinct pivot)."""
    return C.ExactSums(C.table(n, d), np.frombuffer(pivot_bytes, dtype=np.float32))


def _check_fit_cast(dev, n: int, d: int, kind: str, form: str, rate: float = 0.3):
    X = np.array(C.table(n, d))
    y = C.labels_case(n, rate=rate)
    Xd, yd = _dev(X, dev), _dev(y, dev)
    pivot, k = X[0], None
    if kind == "fp8":  # the prescale the pass will compute again (fixed-order kernels: the same bits)
        pv, kv = S.fp8_fused_prescale(Xd)
        pivot, k = pv.cpu().numpy(), kv.cpu().numpy()
    dest = np.random.default_rng(n).permutation(n).astype(np.int64) if form == "scatter" else None
    mo = S.minority_rows_async(yd, 1) if form == "minority" else None
    whole, out = _framed_out(n, kind, dev)
    st = S.scaler_fit_cast(Xd, yd, out, bias_value=-2.5, fp8_scale=C.FP8_SCALE,
                           out_idx=None if dest is None else _dev(dest, dev), minority=mo)
    ks = None if k is None else (k * np.float32(C.FP8_SCALE)).astype(np.float32)
    exp = C.fused_oracle(X, pivot, y, -2.5, kind, ks, dest)
    got = _bits(out)
    if kind == "bf16":
        assert C.bf16_equal(got, exp), (n, d, form)
    else:
        # the hardware conversion may encode -0 / tiny negatives as +0: decoded values must agree.
        # Ties (none in these tables, by construction) are pinned by the hardware sweep test instead.
        assert not np.any(C.fp8_is_tie(C.fused_values(X, pivot, y, -2.5, kind, ks)))
        assert np.array_equal(C.fp8_decode(got), C.fp8_decode(exp)), (n, d, form)
    assert _canaries_intact(whole, kind)
    C.check_stats(C.stats_dict(st), _exact_about(n, d, np.asarray(pivot, dtype=np.float32).tobytes()), default_pivot=True,
                  colscale=k)
    if mo is not None:
        hit = np.flatnonzero(y == 1)
        assert mo.count() == hit.shape[0]
        e = np.zeros((hit.shape[0], 32), dtype=np.float32)
        e[:, :d] = X[hit]
        e[:, 30], e[:, 31] = -2.5, 1.0
        rows = mo.rows()
        if hit.shape[0] > mo.cap:  # overflow: the rows past the capacity are dropped and the caller is told
            assert rows is None
            rows, e = mo.xraw[:mo.cap], e[:mo.cap]
        assert np.array_equal(rows.cpu().numpy().view(np.uint32), e.view(np.uint32))


@pytest.mark.parametrize("d", C.DIMS)
@pytest.mark.parametrize("form", ["plain", "scatter", "minority"])
@pytest.mark.parametrize("kind", ["bf16", "fp8"])
def test_scaler_fit_cast(dev, kind, form, d):
    """Rows: bf16 bitwise rne(x - pivot); fp8 decoded values equal to the RNE oracle's of
    (x - p) k fp8_scale evaluated in float32 in the kernel's order.  Statistics as scaler_fit's.
    The prescale pivot equals the value on a constant column, so those stay exact for fp8 too."""
    for n in C.ROWS:
        _check_fit_cast(dev, n, d, kind, form)


@pytest.mark.parametrize("form", ["plain", "scatter", "minority", "minority_overflow"])
@pytest.mark.parametrize("kind", ["bf16", "fp8"])
def test_scaler_fit_cast_second_sweep(dev, kind, form):
    """Past 2048 x 128 rows.  Minority rows at a rate of 1 % fit the buffer (n / 64 rows); at 30 % they
    overflow it: the first ``cap`` are kept, the rest dropped, the cast rows and statistics unchanged."""
    if form.startswith("minority"):
        _check_fit_cast(dev, C.SWEEP_ROWS, 30, kind, "minority", rate=0.3 if form == "minority_overflow" else 0.01)
    else:
        _check_fit_cast(dev, C.SWEEP_ROWS, 30, kind, form)


def test_scaler_fit_cast_refuses_strided_rows(dev):
    """The fused pass has only the tiled form: a padded or offset view is an error, not a fall-back."""
    for layout in ("vec4", "vec1_off"):
        X = _view(np.array(C.table(9, 30)), layout, dev)
        out = torch.empty((9, 32), dtype=torch.bfloat16, device=dev)
        with pytest.raises(ValueError):
            S.scaler_fit_cast(X, None, out)


def test_fp8_hardware_encode_midpoint_sweep(dev):
    """v_cvt_pk_fp8_f32 behind the +-448 clamp (common.h f32x4_to_fp8) on every midpoint between
    adjacent finite e4m3 values, its two float32 neighbours and the edge values: round to nearest
    even, saturating; only the sign of a zero result may differ from the software encoder."""
    vals = C.fp8_edges()
    vals = np.concatenate([vals, np.zeros((-vals.shape[0]) % 4, dtype=np.float32)])
    vt = _dev(vals, dev)
    dec = torch.empty(256, dtype=torch.float32, device=dev)
    enc = torch.empty(vals.shape[0], dtype=torch.uint8, device=dev)
    native().fp8_hw_check(ptr(dec), ptr(vt), vals.shape[0], ptr(enc), stream_of(vt))
    hw, sw = enc.cpu().numpy(), C.fp8_encode(vals)
    bad = C.fp8_decode(hw) != C.fp8_decode(sw)
    assert not np.any(bad), list(zip(vals[bad][:8], hw[bad][:8], sw[bad][:8]))
    nz = C.fp8_decode(sw) != 0
    assert np.array_equal(hw[nz], sw[nz])
    d_hw, d_sw = dec.cpu().numpy().astype(np.float64), C.fp8_decode(np.arange(256, dtype=np.uint8))
    fin = ~np.isnan(d_sw)
    assert np.array_equal(d_hw[fin], d_sw[fin]) and np.all(np.isnan(d_hw[~fin]))
    assert np.array_equal(np.signbit(d_hw[fin]), np.signbit(d_sw[fin]))


@pytest.mark.parametrize("d", [1, 7, 30])
def test_fp8_prescale(dev, d):
    """mean and population 1/std of rows 0, stride, ... against fp64, relative 1e-6: the float32
    rounding of the outputs (6e-8) with margin.  A constant column gives k = 1 exactly."""
    m = native()
    nb = m.fp8_prescale_blocks()
    for n in (1, 9, 1000, 70_001):
        X = np.array(C.table(n, d))
        Xd = _dev(X, dev)
        for sr in (1, 8, 65_536):
            stride, ns, emu, ek = C.sample_moments(X, sr)
            ws = torch.full(((nb + m.scaler_reduce_scratch_rows(nb)) * 64 + 64,), float("nan"), device=dev,
                            dtype=torch.float64)
            out = torch.full((2 * d + 2,), float("nan"), device=dev, dtype=torch.float32)
            m.fp8_prescale(ptr(Xd), n, d, ns, stride, ptr(ws), ptr(ws[-64:]), ptr(out), ptr(out[d:]), stream_of(Xd))
            o = out.cpu().numpy()
            mu, k = o[:d].astype(np.float64), o[d:2 * d].astype(np.float64)
            assert np.all(np.isnan(o[2 * d:]))
            assert np.all(np.abs(mu - emu) <= 1e-6 * np.abs(emu)), (n, sr, mu, emu)
            assert np.all(np.abs(k - ek) <= 1e-6 * np.abs(ek)), (n, sr, k, ek)
            const = np.all(X[::stride][:ns] == X[0][None, :], axis=0)
            assert np.all(k[const] == 1.0) and np.array_equal(mu[const], X[0][const].astype(np.float64))
    with pytest.raises(RuntimeError):
        m.fp8_prescale(ptr(Xd), 10, d, 6, 2, ptr(ws), ptr(ws[-64:]), ptr(out), ptr(out[d:]), stream_of(Xd))


# ---- E. small scan and per-tile count ----------------------------------------------------------
def test_exclusive_scan_small(dev):
    m = native()
    for n in (1, 3, 4, 5, 255, 256, 257, 1023, 4095, 4096):
        rng = np.random.default_rng(n)
        a = rng.integers(0, 2 ** 20, n).astype(np.int64)
        a[rng.integers(0, n, max(1, n // 7))] += np.int64(2 ** 33) + np.int64(2 ** 40)
        buf = torch.full((n + 4,), -7, dtype=torch.int64, device=dev)
        buf[:n] = _dev(a, dev)
        tot = torch.full((2,), -7, dtype=torch.int64, device=dev)
        m.exclusive_scan_small(ptr(buf), n, ptr(tot), stream_of(buf), 0)
        got = buf.cpu().numpy()
        inc = np.cumsum(a)
        assert np.array_equal(got[:n], inc - a), n
        assert np.all(got[n:] == -7) and list(tot.cpu().numpy()) == [int(inc[-1]), -7]


@pytest.mark.parametrize("target", [0, 1])
def test_compact_count_tiles(dev, target):
    """tinfo = (minority rows of the block's earlier tiles | rows of this tile << 16) and the 128-bit
    match mask of every 128-row tile, decoded and compared with the labels; the scanned block offsets
    and the total.  n at the 128-row tile edge and the 256-tile block edge."""
    for n in (1, 127, 128, 129, 32_767, 32_768, 32_769):
        y = C.labels_case(n, rate=0.3, seed=n)
        mo = S.minority_rows_async(_dev(y, dev), target)
        pend = mo.pending
        hit = y == target
        assert pend.count() == int(hit.sum())
        nt = (n + 127) // 128
        tinfo = pend.tinfo.cpu().numpy()[:nt].view(np.uint32)
        words = pend.tmask.cpu().numpy().view(np.uint32).reshape(nt, 4)
        bits = ((words[:, :, None] >> np.arange(32, dtype=np.uint32)[None, None, :]) & 1).reshape(nt, 128).astype(bool)
        padded = np.zeros(nt * 128, dtype=bool)
        padded[:n] = hit
        per_tile = padded.reshape(nt, 128)
        assert np.array_equal(bits, per_tile)
        cnt = per_tile.sum(1)
        assert np.array_equal(tinfo >> 16, cnt)
        blk = np.arange(nt) // 256
        before = np.cumsum(cnt) - cnt
        first = np.r_[0, np.cumsum(np.bincount(blk, weights=cnt).astype(np.int64))][blk]
        assert np.array_equal(tinfo & 0xFFFF, before - first)
        offs = pend.counts.cpu().numpy()
        assert offs.shape[0] == (nt + 255) // 256 == native().compact_count_tiles_blocks(n)
        assert np.array_equal(offs, np.r_[0, np.cumsum(np.bincount(blk, weights=cnt).astype(np.int64))][:-1])


# ---- F. predict_bf16 / predict_fp8 -------------------------------------------------------------
def _rows_dev(rows: np.ndarray, kind: str, dev) -> torch.Tensor:
    if kind == "bf16":
        return torch.from_numpy(np.array(rows).view(np.int16)).to(dev).view(torch.bfloat16)
    return _dev(rows, dev)


def _check_predict(dev, rows_dev, R, w):
    p, z = P.predict_rows(rows_dev, torch.from_numpy(w), want_logit=True, fp8_scale=C.FP8_SCALE)
    p, z = p.cpu().numpy(), z.cpu().numpy()
    ze, zb = C.predict_oracle(R, w)
    err = np.abs(z.astype(np.float64) - ze)
    assert np.all(err <= zb), (R.shape[0], float(np.max(err / zb)))
    C.check_prob(p, z)
    p_only = P.predict_rows(rows_dev, torch.from_numpy(w), fp8_scale=C.FP8_SCALE).cpu().numpy()
    assert np.array_equal(p_only.view(np.uint32), p.view(np.uint32))  # the logit output is optional


@pytest.mark.parametrize("kind", ["bf16", "fp8"])
def test_predict_rows(dev, kind):
    """Logit within 40 x 2^-24 sum |w_j x_j| of the fp64 dot of the decoded rows (the label slot's
    weight of 7 ignored, a weight of 1e-4 not); probabilities as C.check_prob."""
    w = C.predict_weights()
    rows, R = C.predict_rows_case(1000, kind)
    rd = _rows_dev(rows, kind, dev)
    for n in sorted(C.PREDICT_ROWS):
        _check_predict(dev, rd[:n], R[:n], w)


@pytest.mark.parametrize("kind", ["bf16", "fp8"])
def test_predict_rows_second_sweep(dev, kind):
    rows, R = C.predict_rows_case(C.PREDICT_SWEEP_ROWS, kind)
    _check_predict(dev, _rows_dev(rows, kind, dev), R, C.predict_weights())


@pytest.mark.parametrize("kind", ["bf16", "fp8"])
def test_predict_saturation(dev, kind):
    """Logits of +-80, +-200 and +-inf (bf16: an infinite feature; fp8: 448 x 3e38 overflows in
    fp32): the probability is exactly 0 or 1 beyond +-200 and never NaN."""
    m = native()
    vals = np.array([80.0, -80.0, 200.0, -200.0, np.inf, -np.inf, 0.0, 1.0] * 3, dtype=np.float32)
    n = vals.shape[0]
    r = np.zeros((n, 32), dtype=np.float32)
    r[:, 31] = 1.0  # the label, under a weight of 7: ignored
    w = np.zeros(32, dtype=np.float32)
    w[31] = 7.0
    if kind == "bf16":
        r[:, 5] = vals
        w[5] = 1.0
        rows = C.bf16_bits(r)
    else:  # kernel-space weights (predict_fp8 reads the stored values as they are)
        w[5], w[6], w[7] = 1.5625, 3e38, 1.0  # 128 x 1.5625 = 200; 448 x 3e38 = inf in fp32
        big, inf = np.abs(vals) == 200.0, np.isinf(vals)
        r[big, 5] = np.copysign(128.0, vals[big])
        r[inf, 6] = np.copysign(448.0, vals[inf])
        r[~big & ~inf, 7] = vals[~big & ~inf]
        rows = C.fp8_encode(r)
        assert np.array_equal(C.fp8_decode(rows), r.astype(np.float64))  # every entry is an e4m3 value
    rd = _rows_dev(rows, kind, dev)
    wd = _dev(w, dev)
    prob = torch.empty(n, device=dev, dtype=torch.float32)
    logit = torch.empty(n, device=dev, dtype=torch.float32)
    getattr(m, "predict_" + kind)(ptr(rd), n, ptr(wd), ptr(prob), ptr(logit), stream_of(rd))
    z, p = logit.cpu().numpy().astype(np.float64), prob.cpu().numpy()
    assert np.array_equal(z, vals.astype(np.float64))  # one non-zero product per row: exact
    C.check_prob(p, z)
    assert np.array_equal(p[np.isinf(z)], (z[np.isinf(z)] > 0).astype(np.float32))


# ---- G. predict_shap ---------------------------------------------------------------------------
PAIRS = [(30, 30), (30, 0), (30, 7), (29, 29), (28, 28), (7, 7)]
# raw forms: (ld or 0 for ld = width, width, base offset, intended instantiation)
RAW_FORMS = {"vec4_ld32": (32, 30, 0, 4), "vec4_d28": (0, 28, 0, 4), "vec2_d30": (0, 30, 0, 2),
             "vec1_ld33": (33, 30, 0, 1), "vec1_off": (0, 30, 1, 1)}
SENTINEL = 12345.0


def _shap_vec(ld: int, a: int) -> int:
    """launch_predict_shap's choice for raw rows."""
    return 4 if (ld % 4 == 0 and a % 16 == 0) else 2 if (ld % 2 == 0 and a % 8 == 0) else 1


def _shap_launch(dev, Xd, in_kind, n, ld, dz, dphi, a, c, bias, ld_phi):
    av, cv = _dev(a.astype(np.float32), dev), _dev(c.astype(np.float32), dev)
    prob = torch.full((n + 1,), float("nan"), device=dev, dtype=torch.float32)
    logit = torch.full((n + 1,), float("nan"), device=dev, dtype=torch.float32)
    phi = torch.full((n + 1, ld_phi), SENTINEL, device=dev, dtype=torch.float32) if ld_phi else None
    native().predict_shap(ptr(Xd), in_kind, n, ld, dz, dphi, ptr(av), ptr(cv), float(bias), ptr(prob), ptr(logit),
                          ptr(phi), ld_phi, stream_of(Xd))
    p, z = prob.cpu().numpy(), logit.cpu().numpy()
    assert np.isnan(p[n]) and np.isnan(z[n])
    return p[:n], z[:n], None if phi is None else phi.cpu().numpy()


def _check_shap(Xv, a, c, bias, dz, dphi, p, z, phi, n):
    ze, zb, pe, pb = C.shap_oracle(Xv, a, c, bias, dz, dphi)
    err = np.abs(z.astype(np.float64) - ze)
    assert np.all(err <= zb), (n, dz, float(np.max(err / zb)))
    C.check_prob(p, z)
    if phi is not None:
        assert np.all(phi[n] == SENTINEL) and np.all(phi[:n, dphi:] == SENTINEL)  # nothing past dphi, or past n
        assert np.all(np.abs(phi[:n, :dphi].astype(np.float64) - pe) <= pb), (n, dz, dphi)


def _shap_params():
    return [(f, dz, dphi, lp) for f in ["bf16"] + list(RAW_FORMS) for dz, dphi in PAIRS for lp in ("dphi", 32, 31)
            if f == "bf16" or max(dz, dphi) <= RAW_FORMS[f][1]]


@pytest.mark.parametrize("form,dz,dphi,ldphi", _shap_params())
def test_predict_shap(dev, form, dz, dphi, ldphi):
    """ld_phi = dphi / 32 / 31 reaches the float2 (even) or scalar, the float4 and the scalar phi
    stores; columns from max(dz, dphi) on are NaN in the input and must not be read; the phi buffer's
    columns from dphi on keep their sentinel.  bf16 rows score all 31 columns (dz = 31: the intercept
    is a[30] times the stored 1)."""
    a, c, bias = C.shap_params()
    ld_phi = dphi if ldphi == "dphi" else ldphi
    for n in C.ROWS:
        if form == "bf16":
            rows, R = C.predict_rows_case(n, "bf16")
            cc = c.copy()
            cc[30] = 1.0
            p, z, phi = _shap_launch(dev, _rows_dev(rows, "bf16", dev), 0, n, 32, 31, dphi, a, cc, 0.0, ld_phi)
            _check_shap(R, a, cc, 0.0, 31, dphi, p, z, phi, n)
            continue
        ld, width, off, vec = RAW_FORMS[form]
        ld = ld or width
        X = C.shap_case(n, ld, max(dz, dphi), seed=n)
        buf = np.full(n * ld + off + 3, np.nan, dtype=np.float32)
        buf[off:off + n * ld] = X.reshape(-1)
        Xd = _dev(buf, dev)[off:]
        assert _shap_vec(ld, Xd.data_ptr()) == vec
        p, z, phi = _shap_launch(dev, Xd, 1, n, ld, dz, dphi, a, c, bias, ld_phi)
        _check_shap(X, a, c, bias, dz, dphi, p, z, phi, n)


@pytest.mark.parametrize("form", ["bf16", "vec4_ld32", "vec2_d30", "vec1_ld33"])
def test_predict_shap_second_sweep(dev, form):
    a, c, bias = C.shap_params()
    n = C.SWEEP_ROWS
    if form == "bf16":
        rows, R = C.predict_rows_case(n, "bf16")
        cc = c.copy()
        cc[30] = 1.0
        p, z, phi = _shap_launch(dev, _rows_dev(rows, "bf16", dev), 0, n, 32, 31, 30, a, cc, 0.0, 30)
        _check_shap(R, a, cc, 0.0, 31, 30, p, z, phi, n)
        return
    ld, width, off, vec = RAW_FORMS[form]
    ld = ld or width
    X = C.shap_case(n, ld, 30, seed=1)
    Xd = _dev(X.reshape(-1), dev)
    assert _shap_vec(ld, Xd.data_ptr()) == vec
    p, z, phi = _shap_launch(dev, Xd, 1, n, ld, 30, 30, a, c, bias, 32)
    _check_shap(X, a, c, bias, 30, 30, p, z, phi, n)


@pytest.mark.parametrize("ld", [30, 31])
def test_predict_h2h(dev, ld):
    """The double instantiations (even ld: <1,2,double>, odd: <1,1,double>) through the host-to-host
    path in three chunks (2056 rows, the minimum chunk of 1024): the fp64 outputs are the float32
    kernel's results widened, bitwise, and sit within the oracle's bounds."""
    m = native()
    n, d = 2049 + 7, 30
    a, c, bias = C.shap_params()
    X = C.shap_case(n, ld, d, seed=ld)  # ld = 31: column 30 is NaN and must not be read
    av = _dev(a.astype(np.float32), dev)
    p64, z64 = np.full(n, np.nan), np.full(n, np.nan)
    x_dev = torch.empty((n, ld), dtype=torch.float32, device=dev)
    o_dev = torch.empty((2, n), dtype=torch.float64, device=dev)
    streams = [torch.cuda.Stream(device=dev) for _ in range(3)]
    torch.cuda.synchronize()
    m.predict_h2h(X.ctypes.data, n, ld, d, ptr(av), float(bias), p64.ctypes.data, z64.ctypes.data, ptr(x_dev),
                  ptr(o_dev[0]), ptr(o_dev[1]), 1, *(s.cuda_stream for s in streams))
    torch.cuda.synchronize()
    assert _shap_vec(ld, x_dev.data_ptr()) == (2 if ld % 2 == 0 else 1)
    p32, z32, _ = _shap_launch(dev, _dev(X.reshape(-1), dev), 1, n, ld, d, 0, a, c, bias, 0)
    assert np.array_equal(z64, z32.astype(np.float64)) and np.array_equal(p64, p32.astype(np.float64))
    _check_shap(X, a, c, bias, d, 0, p64, z64, None, n)


# ---- H. predict_gather_logit -------------------------------------------------------------------
@pytest.mark.parametrize("d", [2, 8, 30])
def test_predict_gather_logit(dev, d):
    """Logits of gathered raw rows under fp64 w / mean / scale folded on the device; unused table
    rows are NaN; scale = 1 on the constant column."""
    m = native()
    rng = np.random.default_rng(d)
    w = np.r_[rng.normal(0, 0.5, 30), -1.25, 0.0]
    w[min(C.SMALL_W_COL, d - 1)] = 1e-4
    for n in C.ROWS:
        n_src = n + 5
        X = np.array(C.table(n_src, d))
        st = S.scaler_fit(torch.from_numpy(X))
        mean, scale = st.mean64.numpy(), st.scale64.numpy()
        if d > 1:
            assert scale[1] == 1.0  # the constant column
        idx = C.gather_idx(n, n_src)
        unused = np.ones(n_src, dtype=bool)
        unused[idx] = False
        Xp = X.copy()
        Xp[unused] = np.nan
        Xd, idxd = _dev(Xp, dev), _dev(idx, dev)
        wd, md, sd = _dev(w, dev), _dev(mean, dev), _dev(scale, dev)
        z = torch.full((n + 1,), float("nan"), device=dev, dtype=torch.float32)
        m.predict_gather_logit(ptr(Xd), ptr(idxd), n, d, ptr(wd), ptr(md), ptr(sd), ptr(z), stream_of(Xd))
        got = z.cpu().numpy()
        ze, zb = C.gather_logit_oracle(X, idx, w, mean, scale, d)
        assert np.isnan(got[n])
        err = np.abs(got[:n].astype(np.float64) - ze)
        assert np.all(err <= zb), (n, d, float(np.max(err / zb)))
    for bad in (d + 1 if d % 2 == 0 else d, 34):
        with pytest.raises(ValueError):
            m.predict_gather_logit(ptr(Xd), ptr(idxd), 1, bad, ptr(wd), ptr(md), ptr(sd), ptr(z), stream_of(Xd))
