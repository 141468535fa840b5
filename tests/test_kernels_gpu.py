"""Numerics of every HIP kernel against its CPU oracle (ops/reference.py / sklearn), on MI355X."""
import numpy as np
import pytest
import torch

import _smote_cases as SC
from fraud_detection_amd.data.synthetic import separable
from fraud_detection_amd.ops import knn as K
from fraud_detection_amd.ops import logreg as L
from fraud_detection_amd.ops import metrics as M
from fraud_detection_amd.ops import predict as P
from fraud_detection_amd.ops import reference as ref
from fraud_detection_amd.ops import scaler as S

pytestmark = pytest.mark.gpu


def _data(n, seed=0, rate=0.01):
    X, y = separable(n, fraud_rate=rate, seed=seed)
    return X, y


@pytest.mark.parametrize("n,d", [(1, 30), (37, 30), (100_003, 30), (4096, 7), (2048, 29)])
def test_scaler_stats_match_sklearn(dev, n, d):
    from sklearn.preprocessing import StandardScaler

    X, _ = _data(max(n, 2), seed=n)
    X = X[:n, :d].contiguous()
    X[:, min(2, d - 1)] = 3.25  # constant column -> scale 1
    st = S.scaler_fit(X.to(dev))
    sk = StandardScaler().fit(X.numpy().astype(np.float64))
    mean, var, scale = st.numpy()
    np.testing.assert_allclose(mean, sk.mean_, rtol=1e-12, atol=1e-9)
    np.testing.assert_allclose(var, sk.var_, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(scale, sk.scale_, rtol=1e-9, atol=1e-9)


def test_scaler_odd_row_stride(dev):
    X, _ = _data(5000, seed=9)
    big = torch.zeros((5000, 33))
    big[:, :30] = X
    Xs = big[:, :30]  # ld = 33, odd: scalar-load kernel variant
    st = S.scaler_fit(Xs.to(dev))
    st_ref = S.scaler_fit(Xs.contiguous())
    np.testing.assert_allclose(st.numpy()[0], st_ref.numpy()[0], rtol=1e-12)


@pytest.mark.parametrize("kind", ["bf16", "f32", "fp8"])
def test_scale_cast_matches_oracle(dev, kind):
    X, y = _data(10_007, seed=3)
    st = S.scaler_fit(X)
    out_cpu = S.scale_cast(X, st, labels=y, out_dtype=kind) if kind != "fp8" else None
    out_gpu = S.scale_cast(X.to(dev), st.to(dev), labels=y.to(dev), out_dtype=kind).cpu()
    if kind == "fp8":
        exp = S.scale_cast(X[:512], st, labels=y[:512], out_dtype="fp8")
        assert torch.equal(out_gpu[:512], exp)
    else:
        assert torch.equal(out_gpu, out_cpu)
    r = ref.rows_to_f32(out_gpu).numpy()
    assert np.all(r[:, 30] == 1.0)
    assert np.array_equal(r[:, 31], y.numpy().astype(np.float32))


def test_scale_cast_gather(dev):
    X, y = _data(20_000, seed=4)
    st = S.scaler_fit(X)
    idx = S.compact_indices(y.to(dev), 1)
    assert torch.equal(idx.cpu(), torch.nonzero(y == 1).reshape(-1))
    g = S.scale_cast(X.to(dev), st.to(dev), labels=y.to(dev), out_dtype="f32", idx=idx).cpu()
    e = S.scale_cast(X, st, labels=y, out_dtype="f32", idx=idx.cpu())
    assert torch.equal(g, e)


def test_predict_bf16_and_fp8(dev):
    X, y = _data(50_001, seed=5)
    st = S.scaler_fit(X)
    w = torch.from_numpy(np.r_[np.random.default_rng(0).normal(0, 0.5, 30), -3.0, 7.0])  # w[31] ignored
    rows = S.scale_cast(X, st, labels=y, out_dtype="bf16")
    p_ref, z_ref = P.predict_rows(rows, w, want_logit=True)
    p, z = P.predict_rows(rows.to(dev), w, want_logit=True)
    np.testing.assert_allclose(z.cpu().numpy(), z_ref.numpy(), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(p.cpu().numpy(), p_ref.numpy(), rtol=1e-5, atol=1e-6)
    rows8 = S.scale_cast(X.to(dev), st.to(dev), labels=y.to(dev), out_dtype="fp8")
    p8, z8 = P.predict_rows(rows8, w, want_logit=True)
    z8_ref = ref.predict_rows(ref.rows_to_f32(rows8.cpu()).numpy(), w.numpy())[1]
    np.testing.assert_allclose(z8.cpu().numpy(), z8_ref, rtol=1e-5, atol=1e-4)


def test_predict_rows_with_device_weights_never_synchronises(dev):
    """resident fp32 device weights (label slot nonzero: the kernel ignores it) go
    straight to the kernel -- no D2H read-back, no host synchronisation per call."""
    X, y = _data(20_000, seed=6)
    st = S.scaler_fit(X)
    rows = S.scale_cast(X, st, labels=y, out_dtype="bf16").to(dev)
    w = torch.from_numpy(np.r_[np.random.default_rng(1).normal(0, 0.5, 30), -3.0, 5.0]).float().to(dev)
    p_ref = P.predict_rows(rows.cpu(), w.cpu())
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        p = P.predict_rows(rows, w)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    np.testing.assert_allclose(p.cpu().numpy(), p_ref.numpy(), rtol=1e-5, atol=1e-6)


def test_predict_shap_raw(dev):
    X, _ = _data(30_011, seed=6)
    st = S.scaler_fit(X)
    w = np.r_[np.random.default_rng(1).normal(0, 1, 30), -4.2, 0.0]
    mean, _, scale = st.numpy()
    bg = np.random.default_rng(2).normal(0, 0.1, 30)
    a, c, b = P.fold_scaler(w, mean, scale, bg)
    at, ct = torch.from_numpy(a), torch.from_numpy(c)
    p, phi, z = P.predict_shap_raw(X.to(dev), at.to(dev), ct.to(dev), b, want_logit=True)
    Xs = (X.double().numpy() - mean) / scale
    z_ref = Xs @ w[:30] + w[30]
    phi_ref = w[:30] * (Xs - bg)
    np.testing.assert_allclose(z.cpu().numpy(), z_ref, rtol=2e-5, atol=2e-4)
    np.testing.assert_allclose(phi.cpu().numpy(), phi_ref, rtol=2e-4, atol=2e-4)
    # additivity: sum(phi) = z - z(background)
    z_bg = bg @ w[:30] + w[30]
    np.testing.assert_allclose(phi.cpu().double().numpy().sum(1), z.cpu().numpy() - z_bg, atol=5e-3)


def test_predict_shap_rows_bf16(dev):
    X, y = _data(9_999, seed=8)
    st = S.scaler_fit(X)
    rows = S.scale_cast(X, st, labels=y, out_dtype="bf16")
    w = torch.from_numpy(np.r_[np.random.default_rng(3).normal(0, 1, 30), -2.0, 0.0])
    bg = torch.zeros(32)
    p_ref, phi_ref = P.predict_shap_rows(rows, w, bg)
    p, phi = P.predict_shap_rows(rows.to(dev), w, bg)
    np.testing.assert_allclose(p.cpu().numpy(), p_ref.numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(phi.cpu().numpy(), phi_ref.numpy(), rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("kind", ["bf16", "fp8"])
def test_logreg_pass(dev, kind):
    X, y = _data(70_000, seed=10, rate=0.05)
    st = S.scaler_fit(X)
    rows = S.scale_cast(X.to(dev), st.to(dev), labels=y.to(dev), out_dtype=kind)
    w = torch.from_numpy(np.r_[np.random.default_rng(4).normal(0, 0.3, 30), -2.5, 0.0])
    g, loss, ws, H = L.logreg_pass(rows, w, class_w=(1.0, 3.0))
    g_r, loss_r, ws_r, H_r = ref.logreg_pass(ref.rows_to_f32(rows.cpu()).numpy(), w.numpy(), (1.0, 3.0))
    np.testing.assert_allclose(g, g_r, rtol=1e-4, atol=1e-2)
    assert abs(loss - loss_r) / loss_r < 1e-5
    assert ws == pytest.approx(ws_r)
    rel = np.linalg.norm(H - H_r) / np.linalg.norm(H_r)
    assert rel < 5e-3, rel  # bf16-rounded sqrt(D) X operands, fp32 MFMA accumulation
    np.testing.assert_allclose(H, H.T, atol=1e-6 * np.abs(H).max())


def test_newton_gpu_matches_cpu_and_sklearn(dev):
    from sklearn.linear_model import LogisticRegression

    X, y = _data(60_000, seed=11, rate=0.03)
    st = S.scaler_fit(X)
    rows = S.scale_cast(X, st, labels=y, out_dtype="bf16")
    # tol 1e-7: the device gradient is accumulated in fp32 per block (noise floor ~1e-8)
    fit_g = L.newton_fit(rows.to(dev), C=1.0, tol=1e-7, max_iter=30)
    fit_c = L.newton_fit(rows, C=1.0, tol=1e-7, max_iter=30)
    assert fit_g.converged and fit_c.converged
    np.testing.assert_allclose(fit_g.w[:31], fit_c.w[:31], rtol=1e-5, atol=1e-5)
    R = ref.rows_to_f32(rows).double().numpy()
    sk = LogisticRegression(C=1.0, tol=1e-10, max_iter=2000).fit(R[:, :30], R[:, 31])
    np.testing.assert_allclose(fit_g.w[:30], sk.coef_[0], atol=1e-4)
    assert fit_g.w[30] == pytest.approx(sk.intercept_[0], abs=1e-4)


def test_newton_subsampled_hessian_same_solution(dev):
    X, y = _data(200_000, seed=21, rate=0.02)
    st = S.scaler_fit(X.to(dev))
    rows = S.scale_cast(X.to(dev), st, labels=y.to(dev))
    full = L.newton_fit(rows, tol=1e-7, max_iter=30, hess_stride=1)
    sub = L.newton_fit(rows, tol=1e-7, max_iter=30, hess_stride=4)
    assert full.converged and sub.converged
    np.testing.assert_allclose(sub.w[:31], full.w[:31], atol=2e-5)


def test_newton_progressive_same_solution(dev):
    X, y = _data(300_000, seed=22, rate=0.02)
    st = S.scaler_fit(X.to(dev))
    rows = S.scale_cast(X.to(dev), st, labels=y.to(dev))
    base = L.newton_fit(rows, tol=1e-6, max_iter=30, progressive=[])
    prog = L.newton_fit(rows, tol=1e-6, max_iter=30, progressive=[(8, 2), (2, 2)])
    assert base.converged and prog.converged
    np.testing.assert_allclose(prog.w[:31], base.w[:31], atol=1e-4)


@pytest.mark.parametrize("d,fi", [(20, True), (30, False), (12, False)])
def test_newton_generic_shapes(dev, d, fi):
    """The generic (runtime-m) Newton update kernel, beside the m = 31 specialisation."""
    X, y = _data(50_000, seed=30 + d, rate=0.05)
    X = X[:, :d].contiguous()
    st = S.scaler_fit(X)
    rows = S.scale_cast(X, st, labels=y)
    fit_g = L.newton_fit(rows.to(dev), d=d, fit_intercept=fi, tol=1e-7, max_iter=30)
    fit_c = L.newton_fit(rows, d=d, fit_intercept=fi, tol=1e-7, max_iter=30)
    assert fit_g.converged and fit_c.converged
    np.testing.assert_allclose(fit_g.w[:31], fit_c.w[:31], rtol=1e-5, atol=1e-5)
    if not fi:
        assert fit_g.w[30] == 0.0


def test_newton_lazy_hessian_same_solution(dev):
    X, y = _data(200_000, seed=23, rate=0.02)
    st = S.scaler_fit(X.to(dev))
    rows = S.scale_cast(X.to(dev), st, labels=y.to(dev))
    base = L.newton_fit(rows, tol=1e-7, max_iter=40, hess_refresh=0, progressive=[])
    lazy = L.newton_fit(rows, tol=1e-7, max_iter=40, hess_refresh=3, progressive=[(4, 2)])
    assert base.converged and lazy.converged
    np.testing.assert_allclose(lazy.w[:31], base.w[:31], atol=2e-5)


def test_sgd_device_resume_bit_identical(dev, tmp_path):
    from fraud_detection_amd.utils.checkpoint import CheckpointManager

    X, y = _data(30_000, seed=24, rate=0.05)
    st = S.scaler_fit(X.to(dev))
    rows = S.scale_cast(X.to(dev), st, labels=y.to(dev))
    kw = dict(epochs=3, batches=6)
    full = L.sgd_fit(rows, **kw)
    mgr = CheckpointManager(str(tmp_path), prefix="sgd")
    L.sgd_fit(rows, **kw, checkpoint=mgr, checkpoint_every=3, max_steps=9)  # "crash" mid-epoch 2
    res = L.sgd_fit(rows, **kw, checkpoint=mgr, checkpoint_every=3)
    assert np.array_equal(res.w, full.w) and res.n_iter == full.n_iter == 18


def test_newton_deterministic(dev):
    X, y = _data(40_000, seed=12, rate=0.05)
    st = S.scaler_fit(X.to(dev))
    rows = S.scale_cast(X.to(dev), st, labels=y.to(dev))
    a = L.newton_fit(rows, max_iter=15).w
    b = L.newton_fit(rows, max_iter=15).w
    assert np.array_equal(a, b)


@pytest.mark.parametrize("kind", ["bf16", "fp8", "virtual"])
def test_newton_fused_iteration_matches_unfused(dev, kind, monkeypatch):
    """FDX_NEWTON_FUSE: the pass's last blocks reduce the partials and run the Newton update in the
    same launch (logreg.hip newton_fused_tail).  Same fit as pass + logreg_reduce + newton_update
    up to the fp64 summation order (group sums instead of 64 row-groups): same iteration count and
    convergence, weights within 1e-6.  The fused fit is bitwise reproducible run to run."""
    X, y = _data(300_000, seed=27, rate=0.03)
    st = S.scaler_fit(X.to(dev))
    rows = S.scale_cast(X.to(dev), st, labels=y.to(dev), out_dtype="fp8" if kind == "fp8" else "bf16")
    kw = dict(tol=1e-6, max_iter=30, progressive=[(8, 2), (2, 1)], hess_refresh=2)
    if kind == "virtual":  # SMOTE samples of the positives, generated inside every pass
        pos = rows[rows[:, 31].float() > 0].contiguous()
        g = torch.Generator().manual_seed(5)
        nbr = torch.randint(0, pos.shape[0], (pos.shape[0], 5), generator=g, dtype=torch.int32).to(dev)
        kw["virtual"] = L.VirtualSmote(pos, nbr, 100_000, seed=3, counter_base=1)
    fits = {}
    for fuse in ("0", "1", "1"):  # FDX_NEWTON_FUSE: 0 unfused, 1 fused
        monkeypatch.setenv("FDX_NEWTON_FUSE", fuse)
        fits.setdefault(fuse, []).append(L.newton_fit(rows, workspace=L.LRWorkspace(dev), **kw).as_fit_info())
    a, b, b2 = fits["0"][0], fits["1"][0], fits["1"][1]
    assert a.converged and b.converged and a.n_iter == b.n_iter
    np.testing.assert_allclose(b.w, a.w, atol=1e-6)
    assert np.array_equal(b.w, b2.w)


@pytest.mark.parametrize("pred", [1, 2, 6])
def test_newton_deferred_check_same_fit(dev, pred):
    """newton_fit(full_iters=k): k full-data iterations enqueued with no host wait, convergence
    verified later.  A short prediction (1) is finished by verify(), a long one (6) runs no-op
    iterations: every case is bit-identical to the host-checked fit, iteration count included."""
    X, y = _data(300_000, seed=25, rate=0.02)
    st = S.scaler_fit(X.to(dev))
    rows = S.scale_cast(X.to(dev), st, labels=y.to(dev))
    sched = [(8, 2), (2, 1)]
    ref_fit = L.newton_fit(rows, tol=1e-6, max_iter=30, progressive=sched).as_fit_info()
    f = L.newton_fit(rows, tol=1e-6, max_iter=30, progressive=sched, workspace=L.LRWorkspace(dev), full_iters=pred)
    assert f.deferred
    got = f.as_fit_info()
    assert not f.deferred and got.converged and ref_fit.converged
    assert got.n_iter == ref_fit.n_iter and f.full_phase_iters == ref_fit.n_iter - 3
    assert np.array_equal(got.w, ref_fit.w)


def test_pipeline_deferred_check_matches_checked(dev):
    """Pipeline fits with deferred checks (two alternating buffers, predicted iteration count)
    return the same models as host-checked fits, fit after fit."""
    from fraud_detection_amd.models.pipeline import DevicePipeline, TrainConfig

    X, y = _data(400_000, seed=26, rate=0.01)
    X, y = X.to(dev), y.to(dev)
    on = DevicePipeline(TrainConfig(seed=3))
    off = DevicePipeline(TrainConfig(seed=3, deferred_check=False))
    res_on = [on.fit(X, y) for _ in range(4)]  # fit 3+ run with a prediction learned from fit 1
    res_off = [off.fit(X, y) for _ in range(2)]
    assert on._full_pred is not None
    for r in res_on:
        assert r.fit.n_iter == res_off[0].fit.n_iter
        assert np.array_equal(r.w, res_off[0].w)
    assert on._bufs[0] is not None and on._bufs[1] is not None and off._bufs[1] is None




@pytest.mark.parametrize("mq,k", [(33, 5), (400, 5), (1000, 3), (2500, 8)])
def test_knn_topk_exact(dev, mq, k):
    rng = np.random.default_rng(mq)
    C = np.zeros((mq + 17, 32), np.float32)
    C[:, :30] = rng.normal(size=(mq + 17, 30))
    C[:, 30] = 1.0
    Ct = torch.from_numpy(C)
    off = 5
    Q = Ct[off: off + mq].contiguous()
    idx, d2 = K.knn_topk(Q.to(dev), Ct.to(dev), k=k, self_offset=off, want_dist=True)
    idx_r, d2_r = ref.knn_topk(Q.numpy(), C, k, off)
    idx = idx.cpu().numpy()
    match = (idx == idx_r).all(1)
    # allow disagreement only where the reference distances are within fp32 rounding
    for r in np.flatnonzero(~match):
        gap = np.abs(np.sort(d2_r[r]) - np.sort(d2.cpu().numpy()[r].astype(np.float64)))
        assert gap.max() < 1e-3, (r, idx[r], idx_r[r])
    assert match.mean() > 0.99
    assert not np.any(idx == (np.arange(mq)[:, None] + off))  # self excluded


@pytest.mark.parametrize("engine", ["bf16x3r", "bf16x3t"])
@pytest.mark.parametrize("mq,k,scale", [(400, 5, 1.0), (2500, 8, 1.0), (3000, 5, 40.0)])
def test_knn_engine_exact(dev, mq, k, scale, engine):
    """The bf16x3 filter engines return the exact fp32 ranking: same lists as the oracle (up to
    fp32 rounding of near-equal distances), self excluded, including large-magnitude features."""
    rng = np.random.default_rng(mq + 1)
    C = np.zeros((mq + 17, 32), np.float32)
    C[:, :30] = rng.normal(size=(mq + 17, 30)) * scale
    Ct = torch.from_numpy(C)
    off = 5
    Q = Ct[off: off + mq].contiguous()
    idx, d2 = K.knn_topk(Q.to(dev), Ct.to(dev), k=k, self_offset=off, want_dist=True, engine=engine)
    idx_r, d2_r = ref.knn_topk(Q.numpy(), C, k, off)
    idx = idx.cpu().numpy()
    match = (idx == idx_r).all(1)
    for r in np.flatnonzero(~match):
        gap = np.abs(np.sort(d2_r[r]) - np.sort(d2.cpu().numpy()[r].astype(np.float64)))
        assert gap.max() < 1e-3 * scale * scale, (r, idx[r], idx_r[r])
    assert match.mean() > 0.99
    assert not np.any(idx == (np.arange(mq)[:, None] + off))


def test_knn_engines_agree_with_ties_and_auto_selection(dev):
    """The engines give identical lists and scores on a coarse grid with exact ties and duplicate
    rows, and agree on a 70k-row candidate set."""
    rng = np.random.default_rng(11)
    C = np.zeros((3001, 32), np.float32)
    C[:, :30] = np.round(rng.normal(size=(3001, 30)) * 4) / 4
    C[1500:1600] = C[100:200]
    Ct = torch.from_numpy(C).to(dev)
    Q = Ct[:1000].contiguous()
    a, sa = K.knn_topk(Q, Ct, k=5, self_offset=0, want_dist=True, engine="fp32")
    b, sb = K.knn_topk(Q, Ct, k=5, self_offset=0, want_dist=True, engine="bf16x3r", nsplit=1)
    assert torch.equal(a, b)
    assert torch.allclose(sa, sb, rtol=0, atol=1e-4)
    # more slices, and the two-pass collect: the same exact re-score chain, so bit-identical to it
    for eng, ns in (("bf16x3r", 2), ("bf16x3r", 5), ("bf16x3t", None)):
        r, sr = K.knn_topk(Q, Ct, k=5, self_offset=0, want_dist=True, engine=eng, nsplit=ns)
        assert torch.equal(a, r) and torch.equal(sb, sr), (eng, ns)
    assert K.knn_engine(10, 4_000) == "fp32" and K.knn_engine(10, 13_600) == "bf16x3r"  # ops/knn.py
    # a larger candidate set: 256 queries, every engine
    Cb = torch.from_numpy(rng.normal(size=(70_000, 32)).astype(np.float32)).to(dev)
    Qb = Cb[:256].contiguous()
    ia = K.knn_topk(Qb, Cb, k=5, self_offset=0, engine="fp32")
    for eng in ("bf16x3r", "bf16x3t"):
        ib = K.knn_topk(Qb, Cb, k=5, self_offset=0, engine=eng)
        assert (ia == ib).all(1).float().mean().item() > 0.99


def test_knn_bf16x3r_lists_stay_bounded_on_heavy_tailed_rows(dev):
    """The config-5 shard's minority set (17k standardized rows with the heavy-tailed Amount
    column): the collect pass compacts full lists instead of overflowing (no brute-force scan),
    and the lists equal the fp32 engine's."""
    from fraud_detection_amd.data.synthetic import separable

    X, y = separable(200_000, fraud_rate=0.085, seed=31, device=dev)
    xm = X[y == 1][:17_000]
    xm = (xm - X.mean(0)) / X.std(0)
    C = torch.zeros((xm.shape[0], 32), device=dev)
    C[:, :30] = xm
    C[:, 30] = 1.0
    C = C.contiguous()
    a = K.knn_topk(C, C, k=5, self_offset=0, engine="fp32")
    dg = {}
    b = K.knn_topk(C, C, k=5, self_offset=0, engine="bf16x3r", _diag=dg)
    assert dg["over_cap"] == 0, dg
    assert (a == b).all(1).float().mean().item() > 0.999


def test_knn_collect_list_overflow_falls_back_to_exact_scan(dev):
    """All-equal candidates pass every tile's filter, so the per-lane lists overflow: the re-rank
    kernel's exact scan must still return the k smallest indices (self excluded)."""
    C = torch.ones((3000, 32), dtype=torch.float32, device=dev)
    C[:, 30:] = 0.0
    Q = C[:100].contiguous()
    for ns in (None, 1):
        idx = K.knn_topk(Q, C, k=5, self_offset=0, engine="bf16x3r", nsplit=ns).cpu().numpy()
        for q in range(100):
            want = [c for c in range(7) if c != q][:5]
            assert list(idx[q]) == want, (q, idx[q])


@pytest.mark.parametrize("nsplit", [2, 3, 7, 40])
def test_knn_split_search_identical(dev, nsplit):
    """Candidate slices + merge must reproduce the single-slice lists exactly (incl. tie order)."""
    rng = np.random.default_rng(7)
    C = np.zeros((3001, 32), np.float32)
    C[:, :30] = np.round(rng.normal(size=(3001, 30)) * 4) / 4  # coarse grid -> many exact ties
    C[1500:1600] = C[100:200]                                  # duplicate rows across slices
    Ct = torch.from_numpy(C).to(dev)
    Q = Ct[:1000].contiguous()
    a, sa = K.knn_topk(Q, Ct, k=5, self_offset=0, want_dist=True, nsplit=1)
    b, sb = K.knn_topk(Q, Ct, k=5, self_offset=0, want_dist=True, nsplit=nsplit)
    assert torch.equal(a, b) and torch.equal(sa, sb)


def test_smote_generate_matches_oracle(dev):
    rng = np.random.default_rng(0)
    m = 300
    C = np.zeros((m, 32), np.float32)
    C[:, :30] = rng.normal(size=(m, 30))
    C[:, 30] = 1.0
    C[:, 31] = 1.0
    Ct = torch.from_numpy(C)
    nbr = K.knn_topk(Ct, Ct, k=5, self_offset=0)
    n_new = 50_000
    out = torch.empty((n_new, 32), dtype=torch.bfloat16, device=dev)
    K.smote_generate(Ct.to(dev), nbr.to(dev), 0, n_new, out, seed=42, counter_base=3)
    exp = ref.smote_generate(C, nbr.numpy(), 0, n_new, 42, 3)
    np.testing.assert_allclose(out.float().cpu().numpy(), exp, rtol=1e-2, atol=1e-2)
    assert np.all(out[:, 31].float().cpu().numpy() == 1.0)
    # the single-rounded oracle (_smote_cases.py): the stored bf16 bits of every element
    bits = SC.generate_oracle(C, nbr.numpy(), 0, SC.sample_ids(n_new), "bf16", seed=42, counter_base=3)
    assert np.array_equal(out.view(torch.int16).cpu().numpy().view(np.uint16), bits)


@pytest.mark.parametrize("link,tol", [("logit_model", 2e-4), ("identity", 2e-5), ("logit", 2e-4)])
def test_kernelshap_matches_oracle(dev, link, tol):
    from fraud_detection_amd.models.explainers import KernelExplainer, kernelshap_reference

    rng = np.random.default_rng(5)
    a = np.r_[rng.normal(0, 0.5, 30), 0, 0]
    B = rng.normal(size=(100, 30)).astype(np.float32)
    X = rng.normal(size=(64, 30)).astype(np.float32)
    ke = KernelExplainer(a, -3.0, B, link=link, device=str(dev))
    phi, fx, f0 = ke.explain(X)
    phi_r, fx_r, f0_r = kernelshap_reference(X, a, -3.0, B, ke.Z, ke.A, ke.zM, link)
    np.testing.assert_allclose(phi, phi_r, atol=tol, rtol=1e-3)
    np.testing.assert_allclose(phi.sum(1), fx - f0, atol=1e-4)          # efficiency
    if link == "logit_model":                                          # == LinearSHAP exactly
        np.testing.assert_allclose(phi, a[None, :30] * (X - B.mean(0)), atol=tol)


@pytest.mark.parametrize("n,rate,quant", [(1000, 0.1, None), (300_000, 0.002, None), (200_000, 0.3, 0.05),
                                          (50_000, 0.5, 1.0)])
def test_auc_exact(dev, n, rate, quant):
    from sklearn.metrics import roc_auc_score

    rng = np.random.default_rng(n)
    y = (rng.random(n) < rate).astype(np.uint8)
    s = (rng.normal(size=n) + y * 1.5).astype(np.float32)
    if quant:
        s = (np.round(s / quant) * quant).astype(np.float32)  # heavy ties
    auc = M.roc_auc(torch.from_numpy(s).to(dev), torch.from_numpy(y).to(dev))
    assert auc == pytest.approx(roc_auc_score(y, s), abs=1e-12)
    cm = M.confusion_counts(torch.from_numpy(s).to(dev), torch.from_numpy(y).to(dev), 0.3)
    assert np.array_equal(cm, ref.confusion(s, y, 0.3))


@pytest.mark.parametrize("n", [1, 15, 16, 17, 4095, 100_003, 2_000_001])
@pytest.mark.parametrize("offset", [0, 3])
def test_compact_indices_exact(dev, n, offset):
    """Vectorised (16-byte aligned) and scalar (offset view) compaction == torch.nonzero."""
    g = torch.Generator().manual_seed(n)
    lab = (torch.rand(n + offset, generator=g) < 0.3).to(torch.uint8).to(dev)
    view = lab[offset:]
    for target in (0, 1):
        got = S.compact_indices(view, target)
        ref_idx = torch.nonzero(view == target).reshape(-1)
        assert torch.equal(got, ref_idx)


@pytest.mark.parametrize("n", [17, 2_000_001])
def test_compact_indices_side_stream(dev, n):
    """Count/scan on a side stream behind a ready event, index write on the compute stream (the
    pipeline's placement beside the fused scaler pass) == torch.nonzero.  The compute stream frees
    scratch of the count's size classes while kernels that still write it are queued (as the
    scaler pass's partial sums are): the side stream must not be handed those blocks."""
    g = torch.Generator().manual_seed(n)
    src = (torch.rand(n, generator=g) < 0.3).to(torch.uint8).to(dev)
    lab = torch.empty_like(src)
    big = torch.randn(4096, 4096, device=dev)
    side = torch.cuda.Stream(dev)
    lab.copy_(src)  # labels produced on the compute stream
    ready = torch.cuda.Event()
    ready.record()  # the side stream need not wait for what follows
    nb = max(1, min(512, (n + 255) // 256))
    tmp_counts = torch.empty(nb, dtype=torch.int64, device=dev)
    tmp_total = torch.empty(1, dtype=torch.int64, device=dev)
    _ = big @ big
    tmp_counts.fill_(-7)  # queued behind the matmul
    tmp_total.fill_(-7)
    del tmp_counts, tmp_total  # freed to the compute stream's pool with writes still queued
    pend = S.compact_indices_async(lab, 1, side=side, ready=ready)
    junk = [torch.full((1,), -7, dtype=torch.int64, device=dev) for _ in range(64)]
    got = pend.result()
    assert torch.equal(got, torch.nonzero(src == 1).reshape(-1))
    del junk


@pytest.mark.parametrize("n,rate", [(2_000_000, 0.002), (300_001, 0.3)])
def test_auc_hist_matches_oracle_and_exact(dev, n, rate):
    g = torch.Generator().manual_seed(n)
    y = (torch.rand(n, generator=g) < rate).to(torch.uint8)
    s = (torch.randn(n, generator=g) + 1.7 * y.float()).contiguous()
    s[:1000] = torch.round(s[:1000] * 4) / 4  # some exact ties
    hg = M.score_histogram(s.to(dev), y.to(dev))
    hc = M.score_histogram(s, y)
    assert torch.equal(hg.cpu(), hc)
    assert M.auc_from_histogram(hg) == M.auc_from_histogram(hc)
    exact = M.roc_auc(s.to(dev), y.to(dev))
    assert abs(M.roc_auc_hist(s.to(dev), y.to(dev)) - exact) < 2e-4


@pytest.mark.parametrize("n,rate,k,seed", [(1, 0.5, 5, 42), (1037, 0.02, 5, 42), (2_000_003, 0.0017, 5, 42),
                                           (300_000, 0.3, 10, 9), (65_536, 0.01, 0, 42)])
def test_strat_assign_matches_oracle(n, rate, k, seed):
    from fraud_detection_amd.ops import split as SP

    y = (np.random.default_rng(n).random(n) < rate).astype(np.uint8)
    got = SP.assign(torch.from_numpy(y).cuda(), 0.2, k, seed).cpu().numpy()
    assert np.array_equal(got, SP.assign_numpy(y, 0.2, k, seed))


@pytest.mark.parametrize("n,d", [(1, 30), (1037, 30), (600_011, 30), (4096, 7)])
def test_scaler_fit_cast_fused(dev, n, d):
    """Fused K1+K2: same statistics as scaler_fit (to fp64 summation order), rows = bf16(x - pivot)."""
    X, y = _data(max(n, 2), seed=n)
    X = X[:n, :d].contiguous()
    y = y[:n].contiguous()
    Xd, yd = X.to(dev), y.to(dev)
    out = torch.empty((n, 32), dtype=torch.bfloat16, device=dev)
    st = S.scaler_fit_cast(Xd, yd, out)
    ref_st = S.scaler_fit(Xd)
    for a, b in zip(st.numpy(), ref_st.numpy()):
        np.testing.assert_allclose(a, b, rtol=1e-12, atol=1e-12)
    exp = torch.empty((n, 32), dtype=torch.bfloat16)
    st_cpu = S.scaler_fit_cast(X, y, exp)
    assert torch.equal(out.cpu(), exp)
    np.testing.assert_allclose(st.aff.cpu().numpy(), st_cpu.aff.numpy(), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("storage,d", [("bf16", 30), ("fp8", 30), ("bf16", 7)])
def test_scaler_fit_cast_scatter_form(dev, storage, d):
    """out_idx: row i of X lands in out[out_idx[i]] (the CV table), statistics of the in-order pass."""
    n = 300_007
    X, y = _data(n, seed=31 + d)
    X = X[:, :d].contiguous()
    Xd, yd = X.to(dev), y.to(dev)
    dest = torch.randperm(n, generator=torch.Generator().manual_seed(3)).to(dev)
    dt = torch.bfloat16 if storage == "bf16" else torch.uint8
    plain = torch.empty((n, 32), dtype=dt, device=dev)
    st0 = S.scaler_fit_cast(Xd, yd, plain, fp8_scale=4.0)
    scat = torch.empty((n, 32), dtype=dt, device=dev)
    st1 = S.scaler_fit_cast(Xd, yd, scat, fp8_scale=4.0, out_idx=dest)
    exp = torch.empty_like(plain)
    exp[dest] = plain
    assert torch.equal(scat, exp)
    for a, b in zip(st0.numpy(), st1.numpy()):
        assert np.array_equal(a, b)
    if storage == "bf16":  # the host oracle's scatter too
        cpu = torch.empty((n, 32), dtype=torch.bfloat16)
        S.scaler_fit_cast(X, y, cpu, out_idx=dest.cpu())
        assert torch.equal(cpu, scat.cpu())


def test_smote_affine_output_matches_oracle(dev):
    X, y = _data(200_000, seed=23, rate=0.02)
    sh = torch.empty((X.shape[0], 32), dtype=torch.bfloat16)
    st = S.scaler_fit_cast(X, y, sh)
    idx = torch.nonzero(y == 1).reshape(-1)
    xmin = S.scale_cast(X[idx].contiguous(), st, labels=y[idx].contiguous(), out_dtype="f32")
    nbr = K.knn_topk(xmin, xmin, 5, 0)
    out_cpu = torch.empty((50_000, 32), dtype=torch.bfloat16)
    K.smote_generate(xmin, nbr, 0, 50_000, out_cpu, seed=7, affine=st.aff)
    out_gpu = torch.empty((50_000, 32), dtype=torch.bfloat16, device=dev)
    K.smote_generate(xmin.to(dev), nbr.to(dev), 0, 50_000, out_gpu, seed=7, affine=st.aff.to(dev))
    # the kernel interpolates with one fma, the oracle with mul+add: rare 1-ulp bf16 flips
    g, c = out_gpu.float().cpu(), out_cpu.float()
    assert torch.all((g - c).abs() <= 2.0 ** -7 * c.abs() + 1e-6)
    assert (g != c).float().mean().item() < 1e-3
    # the single-rounded oracle (_smote_cases.py) applies the affine map as the kernel does: bit for bit
    bits = SC.generate_oracle(xmin.numpy(), nbr.numpy(), 0, SC.sample_ids(50_000), "bf16", aff=st.aff.numpy(), seed=7,
                              counter_base=0)
    assert np.array_equal(out_gpu.view(torch.int16).cpu().numpy().view(np.uint16), bits)


def test_newton_affine_matches_cpu(dev):
    X, y = _data(300_000, seed=21)
    sh = torch.empty((X.shape[0], 32), dtype=torch.bfloat16)
    st = S.scaler_fit_cast(X, y, sh)
    f_cpu = L.newton_fit(sh, tol=1e-8, affine=st.aff, w0=np.r_[np.full(30, 0.1), 0.0, 0.0])
    f_gpu = L.newton_fit(sh.to(dev), tol=1e-8, affine=st.aff.to(dev), w0=np.r_[np.full(30, 0.1), 0.0, 0.0],
                         progressive=[])
    assert f_gpu.converged
    np.testing.assert_allclose(f_gpu.w, f_cpu.w, rtol=0, atol=2e-4)


def test_pipeline_fold_scaler_same_model(dev):
    from fraud_detection_amd.models.pipeline import DevicePipeline, TrainConfig, evaluate

    X, y = separable(3_000_000, seed=41, device=dev)
    Xt, yt = separable(500_000, seed=42, device=dev)
    res = {}
    for fold in (True, False):
        r = DevicePipeline(TrainConfig(fold_scaler=fold, tol=1e-6)).fit(X, y)
        res[fold] = (r, evaluate(r, Xt, yt))
    (ra, ea), (rb, eb) = res[True], res[False]
    assert ra.fit.converged and rb.fit.converged
    assert ra.n_train_rows == rb.n_train_rows
    assert np.allclose(ra.w, rb.w, rtol=0, atol=5e-3)
    assert abs(ea["auc"] - eb["auc"]) < 2e-4 and ea["auc"] > 0.95


def test_fp8_hardware_conversions(dev):
    """gfx950 v_cvt_pk_f32_fp8 / v_cvt_pk_fp8_f32 against the software OCP e4m3 codec."""
    from fraud_detection_amd.ops.native import native, ptr, stream_of

    dec = torch.empty(256, dtype=torch.float32, device=dev)
    rng = np.random.default_rng(0)
    vals = np.concatenate([rng.normal(0, 3, 40_000), rng.uniform(-500, 500, 20_000),
                           rng.normal(0, 0.01, 20_000), [0.0, -0.0, 448.0, -448.0, 464.0, 1e6, 2.0 ** -10]])
    vals = vals[: len(vals) // 4 * 4].astype(np.float32)
    vt = torch.from_numpy(vals).to(dev)
    enc = torch.empty(len(vals), dtype=torch.uint8, device=dev)
    native().fp8_hw_check(ptr(dec), ptr(vt), len(vals), ptr(enc), stream_of(vt))
    codes = np.arange(256, dtype=np.uint8)
    sw = ref.fp8_decode(codes)
    hw = dec.cpu().numpy()
    finite = np.isfinite(sw)
    assert np.array_equal(hw[finite], sw[finite])
    assert np.all(np.isnan(hw[~finite]))
    e_sw = ref.fp8_encode(vals)
    e_hw = enc.cpu().numpy()
    # identical codes, except that -0.0 / tiny negatives may encode as +0 vs -0
    diff = e_hw != e_sw
    assert np.all(ref.fp8_decode(e_hw[diff]) == ref.fp8_decode(e_sw[diff])), vals[diff][:10]


@pytest.mark.gpu
def test_compaction_slots_survive_many_in_flight(dev):
    """more pending compactions than pinned slots; each keeps its own count."""
    g = torch.Generator().manual_seed(3)
    labs = [(torch.rand(50_000 + 977 * i, generator=g) < 0.01 * (i + 1)).to(torch.uint8) for i in range(12)]
    pend = [S.compact_indices_async(l.to(dev), 1) for l in labs]
    for l, p in zip(labs, pend):
        exp = torch.nonzero(l == 1).reshape(-1)
        assert torch.equal(p.result().cpu(), exp)


@pytest.mark.gpu
def test_sgd_fused_scaler_matches_unfused(dev):
    """The SGD solver on the fused scaler pass (pivot-shifted rows + affine-mapped updates) gives
    the unfused pipeline's model (standardized rows)."""
    from fraud_detection_amd.data.synthetic import separable
    from fraud_detection_amd.models.pipeline import DevicePipeline, TrainConfig, evaluate

    X, y = separable(400_000, fraud_rate=0.01, seed=13, device=dev)
    Xt, yt = separable(100_000, fraud_rate=0.01, seed=14, device=dev)
    r_f = DevicePipeline(TrainConfig(solver="sgd", seed=42)).fit(X, y)
    r_u = DevicePipeline(TrainConfig(solver="sgd", seed=42, fold_scaler=False)).fit(X, y)
    assert np.allclose(r_f.fit.w[:31], r_u.fit.w[:31], rtol=0, atol=5e-3)
    assert abs(evaluate(r_f, Xt, yt)["auc"] - evaluate(r_u, Xt, yt)["auc"]) < 1e-3


def test_stream_of_follows_current_stream(dev):
    """ops.native.stream_of (raw handle query) == torch's current stream, inside and outside a
    stream context: every launcher enqueues where torch would."""
    from fraud_detection_amd.ops.native import stream_of

    t = torch.empty(1, device=dev)
    assert stream_of(t) == torch.cuda.current_stream(dev).cuda_stream
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        assert stream_of(t) == side.cuda_stream
    assert stream_of(t) == torch.cuda.current_stream(dev).cuda_stream
