"""The oracles of _stream_cases.py checked against independent definitions, and the CPU branches of
ops/scaler.py and ops/predict.py (what GPU tests elsewhere compare against) run through the same
cases and bounds as the device kernels in test_stream_kernels_gpu.py.  No GPU needed."""
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

import _stream_cases as C
from fraud_detection_amd.ops import predict as P
from fraud_detection_amd.ops import reference as ref
from fraud_detection_amd.ops import scaler as S

CPU_ROWS = (1, 9, 129, 1000)
CPU_DIMS = (1, 3, 7, 30)


def _bf16_tensor_bits(t: torch.Tensor) -> np.ndarray:
    return t.view(torch.int16).numpy().view(np.uint16)


# ---- the oracles themselves ----------------------------------------------------------------------
def test_col_moments_are_exact():
    rng = np.random.default_rng(0)
    col = np.concatenate([rng.normal(0, 1, 200), 10.0 ** rng.uniform(-30, 30, 200), [0.0, -0.0, 1e-45, 3e38],
                          -(10.0 ** rng.uniform(-5, 5, 100))]).astype(np.float32)
    s1, s2 = C._col_moments(col)
    f = [Fraction(float(v)) for v in col]
    assert s1 == sum(f) and s2 == sum(v * v for v in f)


def test_exact_sums_match_fsum_where_differences_are_exact():
    X = C.table(1000, 30)
    for pivot in (None, C.explicit_pivot(30)):
        ex = C.ExactSums(X, pivot)
        D = X.astype(np.float64) - ex.pivot.astype(np.float64)[None, :]
        for j in range(30):  # the table's differences are exact in fp64 (one magnitude per column)
            assert Fraction(float(D[0, j])) == Fraction(float(X[0, j])) - Fraction(float(ex.pivot[j]))
            assert ex.s1[j] == math.fsum(D[:, j])
            assert abs(ex.s2[j] - math.fsum(D[:, j] * D[:, j])) <= 1000 * C.U53 * ex.s2[j]  # the squares round
        assert ex.mean.shape == (30,) and np.all(ex.var >= 0)
    assert not np.any(X == C.explicit_pivot(30)[None, :])


def test_table_columns():
    X = C.table(1000, 30)
    assert np.all(np.abs(X[:, 0] - 1e5) <= 1.01) and np.all(X[:, 1] == np.float32(0.1)) and np.all(X[:, 5] == 1e7)
    assert X[:, 2].min() < 2e-3 and X[:, 2].max() > 5e3
    assert np.all(X[:, 3] == 0) and 0 < np.signbit(X[:, 3]).sum() < 1000
    u = np.unique(X[:, 4])
    assert u.shape == (2,) and u[1] == np.nextafter(u[0], np.float32(np.inf)) and u[0] == np.float32(1e6)
    assert np.array_equal(C.table(129, 7), X[:129, :7])
    ex = C.ExactSums(X)
    assert [j for j in range(30) if ex.var_exact_zero[j]] == [j for j in range(30) if j % 7 in (1, 3, 5)]


def test_bf16_integer_rne_matches_torch_on_every_tie():
    v = C.bf16_sweep()
    got = C.bf16_bits(v)
    exp = _bf16_tensor_bits(torch.from_numpy(v).to(torch.bfloat16))
    assert C.bf16_equal(got, exp)
    nan = np.isnan(v)
    assert np.all(np.isnan(C.bf16_values(got[nan]))) and not np.any(np.isnan(C.bf16_values(got[~nan])))
    t = C.bf16_ties()
    assert np.all((t.view(np.uint32) & 0xFFFF) == 0x8000)
    assert np.all((C.bf16_bits(t) & 1) == 0) or np.all(np.isinf(C.bf16_values(C.bf16_bits(t))[(C.bf16_bits(t) & 1) == 1]))
    up = t.view(np.uint32) >> 16
    assert np.any(up & 1) and np.any(~up & 1) and np.any(t < 0) and np.any(t > 0)


def _fp8_probe() -> np.ndarray:
    rng = np.random.default_rng(1)
    return np.concatenate([C.fp8_edges(), rng.normal(0, 3, 4000).astype(np.float32),
                           rng.uniform(-500, 500, 2000).astype(np.float32),
                           (10.0 ** rng.uniform(-5, 3, 2000)).astype(np.float32),
                           np.array([np.inf, -np.inf, np.nan, 1e-30, -1e-30], dtype=np.float32)])


def test_fp8_vector_encoder_matches_scalar_encoder():
    v = _fp8_probe()
    assert np.array_equal(C.fp8_encode(v), ref.fp8_encode(v))
    codes = np.arange(256, dtype=np.uint8)
    a, b = C.fp8_decode(codes), ref.fp8_decode(codes).astype(np.float64)
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])
    assert np.array_equal(np.signbit(a), np.signbit(b))


def test_fp8_vector_encoder_is_nearest_even_satfinite():
    v = _fp8_probe()
    enc = C.fp8_encode(v)
    assert np.array_equal(enc, C.fp8_nearest(v))
    mid = C.fp8_midpoints()
    n = mid.shape[0] // 6
    assert n == 126 and np.all(C.fp8_is_tie(mid[:n])) and not np.any(C.fp8_is_tie(mid[n:3 * n]))
    assert np.all((C.fp8_encode(mid[:n]) & 1) == 0)  # ties land on even codes
    # the sign of zero is kept; the round trip of every finite code is the identity
    assert C.fp8_encode(np.float32(-0.0)) == 0x80 and C.fp8_encode(np.float32(0.0)) == 0x00
    codes = np.array([c for c in range(256) if c & 0x7F != 0x7F], dtype=np.uint8)
    assert codes.shape[0] == 254
    assert np.array_equal(C.fp8_encode(C.fp8_decode(codes).astype(np.float32)), codes)
    edge = np.array([2.0 ** -10, 2.0 ** -9, 2.0 ** -6, 448.0, 463.9, 464.0, 1e6], dtype=np.float32)
    assert list(C.fp8_encode(edge)) == [0x00, 0x01, 0x08, 0x7E, 0x7E, 0x7E, 0x7E]
    assert list(C.fp8_encode(-edge)) == [0x80, 0x81, 0x88, 0xFE, 0xFE, 0xFE, 0xFE]


def test_cast_table_holds_the_edges_and_fused_inputs_hold_no_fp8_tie():
    X = C.cast_table(1000, 30)
    lo = X.view(np.uint32) & 0xFFFF
    assert (lo == 0x8000).sum() > 1000
    with np.errstate(over="ignore"):
        assert C.fp8_is_tie(X * np.float32(C.FP8_SCALE)).sum() >= 126
    assert np.any(np.signbit(X) & (X == 0))
    idx = C.gather_idx(500, 1000)
    assert idx[0] == 999 and len(np.unique(idx)) < 500 and np.any(np.diff(idx) < 0)


# ---- CPU branches: scaler ------------------------------------------------------------------------
_stats_dict = C.stats_dict


@pytest.mark.parametrize("d", CPU_DIMS)
@pytest.mark.parametrize("explicit", [False, True])
def test_cpu_scaler_sums_and_fit(d, explicit):
    for n in CPU_ROWS:
        X = C.table(n, d)
        pivot = C.explicit_pivot(d) if explicit else None
        ex = C.ExactSums(X, pivot)
        Xt = torch.from_numpy(np.array(X))
        pt = torch.from_numpy(ex.pivot.copy())
        C.check_sums(S.scaler_partial_sums(Xt, pt).numpy(), ex)
        st = S.scaler_fit(Xt, pivot=None if pivot is None else pt)
        C.check_stats(_stats_dict(st), ex, default_pivot=not explicit)


def test_cpu_scaler_nan_column_stays_in_its_column():
    X = np.array(C.table(129, 7))
    base = _stats_dict(S.scaler_fit(torch.from_numpy(X.copy())))
    X[77, 2] = np.nan
    got = _stats_dict(S.scaler_fit(torch.from_numpy(X)))
    keep = np.arange(32) != 2
    for k in ("mean64", "var64", "scale64", "mean32", "inv32"):
        assert np.isnan(got[k][2]), k
        assert np.array_equal(got[k][keep], base[k][keep]), k


@pytest.mark.parametrize("kind", ["f32", "bf16", "fp8"])
@pytest.mark.parametrize("use_idx", [False, True])
def test_cpu_scale_cast(kind, use_idx):
    for d in CPU_DIMS:
        for n in CPU_ROWS:
            n_src = n + 5 if use_idx else n
            X = C.cast_table(n_src, d)
            y = C.labels_case(n_src)
            idx = C.gather_idx(n, n_src) if use_idx else None
            for ident in (True, False):
                if ident:
                    st = S.stats_from_numpy(np.zeros(d), np.ones(d))
                else:
                    X = np.array(C.table(n_src, d))
                    st = S.scaler_fit(torch.from_numpy(X))
                with np.errstate(over="ignore"):  # the largest bf16 tie times fp8_scale
                    out = S.scale_cast(torch.from_numpy(X), st, labels=torch.from_numpy(y), out_dtype=kind,
                                       idx=None if idx is None else torch.from_numpy(idx), bias_value=-2.5,
                                       fp8_scale=C.FP8_SCALE)
                exp = C.cast_oracle(X, st.mean32.numpy(), st.inv32.numpy(), y, -2.5, kind, C.FP8_SCALE, idx)
                got = _bf16_tensor_bits(out) if kind == "bf16" else out.numpy()
                if kind == "bf16":
                    assert C.bf16_equal(got, exp), (n, d, ident)
                else:
                    assert np.array_equal(got.view(np.uint32) if kind == "f32" else got,
                                          exp.view(np.uint32) if kind == "f32" else exp), (n, d, ident)


@pytest.mark.parametrize("kind", ["bf16", "fp8"])
@pytest.mark.parametrize("scatter", [False, True])
def test_cpu_scaler_fit_cast(kind, scatter):
    for d in CPU_DIMS:
        for n in CPU_ROWS:
            X = np.array(C.table(n, d))
            y = C.labels_case(n)
            Xt, yt = torch.from_numpy(X), torch.from_numpy(y)
            dest = np.random.default_rng(n).permutation(n).astype(np.int64) if scatter else None
            out = torch.zeros((n, 32), dtype=torch.bfloat16 if kind == "bf16" else torch.uint8)
            pivot, k = (None, None)
            if kind == "fp8":
                pivot, k = S.fp8_fused_prescale(Xt)
            st = S.scaler_fit_cast(Xt, yt, out, bias_value=-2.5, fp8_scale=C.FP8_SCALE,
                                   out_idx=None if dest is None else torch.from_numpy(dest))
            piv = X[0] if pivot is None else pivot.numpy()
            ks = None if k is None else (k.numpy() * np.float32(C.FP8_SCALE)).astype(np.float32)
            exp = C.fused_oracle(X, piv, y, -2.5, kind, ks, dest)
            if kind == "bf16":
                assert C.bf16_equal(_bf16_tensor_bits(out), exp), (n, d)
            else:
                assert np.array_equal(out.numpy(), exp), (n, d)
            C.check_stats(_stats_dict(st), C.ExactSums(X, piv), default_pivot=kind == "bf16",
                          colscale=None if k is None else k.numpy())


def test_cpu_sample_moments():
    for n in (1, 9, 1000, 70_001):
        X = torch.from_numpy(np.array(C.table(n, 30)))
        for sr in (1, 8, 65_536):
            mu, k = S._sample_moments(X, sr)
            _, _, emu, ek = C.sample_moments(X.numpy(), sr)
            # float32 output rounding (6e-8) with margin
            assert np.all(np.abs(mu.numpy() - emu) <= 1e-6 * np.abs(emu)), (n, sr)
            assert np.all(np.abs(k.numpy() - ek) <= 1e-6 * np.abs(ek)), (n, sr)


def test_cpu_compact_indices():
    for n in (1, 127, 128, 129, 32_769):
        y = C.labels_case(n, rate=0.1)
        for target in (0, 1):
            got = S.compact_indices(torch.from_numpy(y), target).numpy()
            assert np.array_equal(got, np.flatnonzero(y == target))


# ---- CPU branches: predict -----------------------------------------------------------------------
def _rows_tensor(rows: np.ndarray, kind: str) -> torch.Tensor:
    if kind == "bf16":
        return torch.from_numpy(np.array(rows).view(np.int16)).view(torch.bfloat16)
    return torch.from_numpy(np.array(rows))


@pytest.mark.parametrize("kind", ["bf16", "fp8"])
def test_cpu_predict_rows(kind):
    w = C.predict_weights()
    for n in (1, 17, 257, 1000):
        rows, R = C.predict_rows_case(n, kind)
        p, z = P.predict_rows(_rows_tensor(rows, kind), torch.from_numpy(w), want_logit=True, fp8_scale=C.FP8_SCALE)
        ze, zb = C.predict_oracle(R, w)
        assert np.all(np.abs(z.numpy() - ze) <= zb)
        C.check_prob(p.numpy(), z.numpy())


def test_predict_bound_notices_a_dropped_column_and_a_counted_label():
    w = C.predict_weights()
    _, R = C.predict_rows_case(1000, "bf16")
    ze, zb = C.predict_oracle(R, w)
    dropped = ze - R[:, C.SMALL_W_COL] * w[C.SMALL_W_COL]
    assert np.mean(np.abs(dropped - ze) > zb) > 0.5  # most rows: the weight-1e-4 column is above the bound
    labelled = ze + R[:, 31] * w[31]
    assert np.all((np.abs(labelled - ze) > zb) == (R[:, 31] != 0))


def test_check_prob_saturation_and_bound():
    z = np.array([-np.inf, -200.0, -80.0, -3.0, 0.0, 3.0, 80.0, 200.0, np.inf])
    p = C.sigmoid64(z).astype(np.float32)
    C.check_prob(p, z)
    with pytest.raises(AssertionError):
        C.check_prob(p * np.float32(1.0 + 2e-5), z)


@pytest.mark.parametrize("dz,dphi", [(30, 30), (30, 0), (30, 7), (29, 29), (28, 28), (7, 7)])
def test_cpu_predict_shap_raw(dz, dphi):
    a, c, bias = C.shap_params()
    X = C.shap_case(129, dz, dz)
    p, phi, z = P.predict_shap_raw(torch.from_numpy(X), torch.from_numpy(a), torch.from_numpy(c), bias, dphi=dphi,
                                   want_logit=True)
    ze, zb, pe, pb = C.shap_oracle(X, a, c, bias, dz, dphi)
    assert np.all(np.abs(z.numpy() - ze) <= zb) and phi.shape == (129, dphi)
    assert np.all(np.abs(phi.numpy() - pe) <= pb)
    C.check_prob(p.numpy(), z.numpy())


def test_cpu_predict_shap_rows():
    a, c, _ = C.shap_params()
    rows, R = C.predict_rows_case(257, "bf16")
    for dphi in (30, 7, 29):
        p, phi, z = P.predict_shap_rows(_rows_tensor(rows, "bf16"), torch.from_numpy(a), torch.from_numpy(c), dphi=dphi,
                                        want_logit=True)
        cc = c.copy()
        cc[30] = 1.0
        ze, zb, pe, pb = C.shap_oracle(R, a, cc, 0.0, 31, dphi)
        assert np.all(np.abs(z.numpy() - ze) <= zb)
        assert np.all(np.abs(phi.numpy() - pe) <= pb)
        C.check_prob(p.numpy(), z.numpy())
