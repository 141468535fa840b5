"""Fused minority chain (TrainConfig.fuse_minority): the scaler pass writes the raw minority rows it
holds in LDS and one k-NN prep launch finalizes the scaler, standardizes them and writes the k-NN
operands.  The oracle everywhere is the index-list chain run in the same process --
compact_indices + scale_cast(out_dtype="f32", idx=...) + the plain knn_prep -- and every
comparison is bitwise."""
import numpy as np
import pytest
import torch

from fraud_detection_amd.data.synthetic import separable
from fraud_detection_amd.models.pipeline import DevicePipeline, TrainConfig
from fraud_detection_amd.ops import knn as K
from fraud_detection_amd.ops import scaler as S
from fraud_detection_amd.ops.native import native

pytestmark = pytest.mark.gpu

STAT_FIELDS = ("mean64", "var64", "scale64", "mean32", "inv32", "aff")


def _rows(n, d, seed, dev):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn((n, d), generator=g) * 3.0 + torch.arange(d, dtype=torch.float32)
    return X.to(dev).contiguous()


def _labels(n, pattern, seed, dev):
    g = torch.Generator().manual_seed(seed + 1)
    y = torch.zeros(n, dtype=torch.uint8)
    if pattern == "random":  # ~30 % minority: several per tile
        y = (torch.rand(n, generator=g) < 0.3).to(torch.uint8)
    elif pattern == "sparse":  # ~1 %: most tiles empty
        y = (torch.rand(n, generator=g) < 0.01).to(torch.uint8)
    elif pattern == "ends":
        y[0] = 1
        y[n - 1] = 1
    elif pattern == "tile":  # one whole 128-row tile of the pass, nothing else
        y[128:256] = 1
    elif pattern == "one":
        y[:] = 1
    else:
        assert pattern == "none"
    return y.to(dev)


def _out(n, storage, dev):
    return torch.empty((n, 32), device=dev, dtype=torch.bfloat16 if storage == "bf16" else torch.uint8)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int16)


def _assert_stats_equal(a, b):
    for f in STAT_FIELDS:
        assert torch.equal(getattr(a, f), getattr(b, f)), f


def _check_pass(n, d, pattern, storage, dev, seed=0):
    X, y = _rows(n, d, seed, dev), _labels(n, pattern, seed, dev)
    out0 = _out(n, storage, dev)
    st0 = S.scaler_fit_cast(X, y, out0)
    idx = S.compact_indices(y, 1)
    mino = S.minority_rows_async(y, 1)
    mino.xraw.fill_(-7.0)
    out1 = _out(n, storage, dev)
    st1 = S.scaler_fit_cast(X, y, out1, minority=mino)
    total = mino.pending.total  # the scan's device total (released once the count is read)
    cnt = mino.count()
    assert cnt == int(total.item()) == idx.numel() == int((y == 1).sum().item())
    raw = mino.rows()
    assert raw is not None and raw.shape == (cnt, 32)
    assert torch.equal(raw[:, :d], X[idx])  # the right rows, in stable order
    assert torch.all(raw[:, d:30] == 0) and torch.all(raw[:, 30] == 1) and torch.all(raw[:, 31] == 1)
    assert torch.all(mino.xraw[cnt:] == -7.0)  # nothing past the count
    # the training rows and the statistics are those of a pass without the minority output
    assert torch.equal(out1.view(torch.uint8), out0.view(torch.uint8))
    _assert_stats_equal(st1, st0)


@pytest.mark.parametrize("n", [1, 127, 128, 129, 1000])
def test_pass_emits_minority_rows(dev, n):
    _check_pass(n, 30, "random", "bf16", dev, seed=n)


@pytest.mark.parametrize("n,pattern", [(1, "one"), (1000, "ends"), (1000, "none"), (1000, "tile")])
def test_pass_label_patterns(dev, n, pattern):
    _check_pass(n, 30, pattern, "bf16", dev, seed=5)


@pytest.mark.parametrize("d", [7, 29, 30])
def test_pass_feature_counts(dev, d):
    _check_pass(1000, d, "random", "bf16", dev, seed=d)


def test_pass_spans_count_blocks(dev):
    # 70 001 rows = 547 tiles: three count blocks of 256 tiles, so block offset and in-block prefix both matter
    assert native().compact_count_tiles_blocks(70_001) == 3
    _check_pass(70_001, 30, "sparse", "bf16", dev, seed=11)


def test_pass_second_tile_per_block(dev):
    # more rows than grid x 128, so blocks of the occupancy-derived grid take a second tile
    grid = S._stats_cast_grid(native(), dev, False, True)
    n = max(300_001, grid * 128 + 4097)
    assert (n + 127) // 128 > grid
    _check_pass(n, 30, "sparse", "bf16", dev, seed=13)


@pytest.mark.parametrize("n,pattern", [(1000, "random"), (70_001, "sparse")])
def test_pass_fp8(dev, n, pattern):
    _check_pass(n, 30, pattern, "fp8", dev, seed=17)


def test_capacity_overflow_drops_rows_past_cap(dev):
    n, d, cap = 1000, 30, 37
    X, y = _rows(n, d, 3, dev), _labels(n, "random", 3, dev)
    idx = S.compact_indices(y, 1)
    assert idx.numel() > cap
    buf = torch.full((idx.numel() + 8, 32), -7.0, device=dev)
    mino = S.minority_rows_async(y, 1, cap=cap, xraw=buf)
    out = _out(n, "bf16", dev)
    S.scaler_fit_cast(X, y, out, minority=mino)
    assert mino.count() == idx.numel()  # the host still sees the whole count
    assert mino.rows() is None
    assert torch.equal(buf[:cap, :d], X[idx[:cap]])
    assert torch.all(buf[cap:] == -7.0)  # rows at and beyond cap untouched


def _minority_problem(m, d, dev, seed):
    """Raw rows with exactly m minority rows among 3 m + 5."""
    n = 3 * m + 5
    X = _rows(n, d, seed, dev)
    y = torch.zeros(n, dtype=torch.uint8)
    y[torch.randperm(n, generator=torch.Generator().manual_seed(seed))[:m]] = 1
    return X, y.to(dev)


def _check_prep(m, d, engine, fold, dev):
    X, y = _minority_problem(m, d, dev, seed=100 + m + d)
    n = X.shape[0]
    k = min(5, m - 1)
    # oracle: finalize + index list + gather + the plain prep
    st0 = S.scaler_fit_cast(X, y, _out(n, "bf16", dev))
    xmin = S.scale_cast(X, st0, labels=y, out_dtype="f32", idx=S.compact_indices(y, 1))
    assert xmin.shape[0] == m
    par0 = torch.empty((m, 32), dtype=torch.bfloat16, device=dev)
    ops0 = {}
    nbr0 = K.knn_topk(xmin, xmin, k=k, self_offset=0, parents=par0, parents_affine=st0.aff, engine=engine,
                      _operands=ops0)
    # fused: raw rows from the pass, one prep launch
    mino = S.minority_rows_async(y, 1)
    st1 = S.scaler_fit_cast(X, y, _out(n, "bf16", dev), minority=mino, defer_finalize=True)
    assert st1.pending is not None
    if not fold:  # the prep reads a finalize launch's outputs instead
        st1.finalize()
    raw = mino.rows()
    par1 = torch.empty((m, 32), dtype=torch.bfloat16, device=dev)
    ops1 = {}
    nbr1 = K.knn_topk(raw, raw, k=k, self_offset=0, parents=par1, raw_stats=st1, engine=engine, _operands=ops1)
    assert st1.pending is None
    assert sorted(ops0) == sorted(ops1) and ("Chl" in ops0) == (engine != "fp32")
    for name in ops0:
        a, b = ops1[name], ops0[name]
        if name == "lists":  # bf16x3t's [slice][block][entry][lane]: a lane writes its first counts[0] entries only
            assert torch.equal(ops1["counts"], ops0["counts"])
            live = torch.arange(a.shape[2], device=dev)[None, None, :, None] < ops0["counts"][0][:, :, None, :]
            a, b = a[live], b[live]
        assert torch.equal(_bits(a), _bits(b)), name
    assert torch.equal(_bits(par1), _bits(par0))
    assert torch.equal(nbr1, nbr0)
    _assert_stats_equal(st1, st0)


@pytest.mark.parametrize("d", [7, 30])
@pytest.mark.parametrize("m", [2, 31, 32, 33, 1000])
@pytest.mark.parametrize("engine", ["fp32", "bf16x3r"])
def test_fused_prep_matches_chain(dev, engine, m, d):
    _check_prep(m, d, engine, True, dev)


@pytest.mark.parametrize("engine,m,d,fold", [("bf16x3t", 1000, 30, True), ("bf16x3t", 33, 7, True),
                                             ("bf16x3r", 33, 30, False), ("fp32", 1000, 7, False)])
def test_fused_prep_other_forms(dev, engine, m, d, fold):
    _check_prep(m, d, engine, fold, dev)


def _fit(X, y, fuse, solver, storage):
    pipe = DevicePipeline(TrainConfig(solver=solver, storage=storage, fuse_minority=fuse, max_iter=20))
    res = pipe.fit(X, y)
    pipe.settle()
    st = res.scaler
    return (np.array(res.w, copy=True), [getattr(st, f).cpu().numpy() for f in STAT_FIELDS],
            (res.n_rows, res.n_train_rows, res.n_minority, res.n_synthetic))


def _assert_fits_equal(a, b):
    assert np.array_equal(a[0], b[0])
    for u, v in zip(a[1], b[1]):
        assert np.array_equal(u, v)
    assert a[2] == b[2]


@pytest.fixture(scope="module")
def fit_data(dev):
    return separable(40_000, fraud_rate=0.005, seed=21, device=dev)


@pytest.mark.parametrize("storage", ["bf16", "fp8"])
@pytest.mark.parametrize("solver", ["sgd", "newton"])
def test_whole_fit_equal_with_switch_on_and_off(dev, fit_data, monkeypatch, solver, storage):
    X, y = fit_data
    off = _fit(X, y, False, solver, storage)
    # with the switch on the index-list chain must not run at all
    used = []
    real = S.compact_indices_async
    monkeypatch.setattr(S, "compact_indices_async", lambda *a, **kw: (used.append(1), real(*a, **kw))[1])
    on = _fit(X, y, True, solver, storage)
    assert not used
    assert on[2][2] > 1 and on[2][3] > 0  # minority rows and SMOTE samples: the k-NN ran
    _assert_fits_equal(on, off)


def test_pipeline_falls_back_on_overflow(dev, fit_data, monkeypatch):
    X, y = fit_data
    off = _fit(X, y, False, "sgd", "bf16")
    monkeypatch.setattr(S, "minority_capacity", lambda n: 16)  # far below the ~200 minority rows
    used = []
    real = S.compact_indices_async
    monkeypatch.setattr(S, "compact_indices_async", lambda *a, **kw: (used.append(1), real(*a, **kw))[1])
    on = _fit(X, y, True, "sgd", "bf16")
    assert used  # the index-list chain served this fit
    _assert_fits_equal(on, off)
