"""Every kernel on the Newton path of logreg.hip against a plain fp64 oracle, at the smallest
shapes where it can still go wrong: the bf16 / fp8 passes (row-count edges on small grids, the CV
hole, tile subsets and the sub-sampled Hessian with its weight in red[34], value edges),
logreg_reduce_kernel (bitwise on dyadic partials), newton_update_kernel against NewtonStateRef on
the same reduced vector and state (every branch), the fused tail against the unfused launches, and
logreg_init / logreg_fold.  Oracles: ops/reference.py; cases and tolerances: tests/_logreg_cases.py.

Tolerances (none tuned to the kernels): red[33] / red[34] exact; loss 1e-5 relative; gradient 1e-5
of its own absolute-term sum + 1e-7; H 5e-3 relative Frobenius and symmetric to 1e-6 max|H|;
Newton step 16 m 2^-46 cond(A) |step|_inf."""
import numpy as np
import pytest
import torch

import _logreg_cases as LC
from fraud_detection_amd.ops import logreg as L
from fraud_detection_amd.ops import reference as ref
from fraud_detection_amd.ops.native import native, ptr, stream_of

pytestmark = pytest.mark.gpu

CW = (1.0, 3.0)
KINDS = ["bf16", "fp8"]


def _pass_case(dev, n, kind, nblocks, class_w=CW, hessian=True, hess_stride=1, sub=1, hole=None, w=None):
    """Run one device pass and its oracle: (red, exp, R the pass's logical rows, w)."""
    rows, R = LC.rows_case(n, kind)
    w = LC.weights_case() if w is None else w
    red = L.logreg_pass(rows.to(dev), torch.from_numpy(w), class_w, hessian, LC.FP8_SCALE, hess_stride=hess_stride,
                        sub=sub, hole=hole, nblocks=nblocks, full=True)
    if hole is not None:
        R = np.delete(R, slice(hole[0], hole[0] + hole[1]), axis=0)
    m = native()
    nb = nblocks or m.logreg_pass_blocks(0 if kind == "bf16" else 1)
    exp = ref.logreg_pass_tiles(R, w, class_w, hess_stride, sub, 0, 4 * nb, hessian)
    return red, exp, R, w


# ---- A. row-count edges on a small grid ------------------------------------------------------
def _edge_rows(nblocks):
    gw = 4 * nblocks
    return [1, 63, 64, 65, 64 * gw - 1, 64 * gw, 64 * gw + 1, 3 * 64 * gw + 17]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("hessian", [True, False])
@pytest.mark.parametrize("nblocks,n", [(nb, n) for nb in (1, 3) for n in _edge_rows(nb)])
def test_pass_row_count_edges(dev, nblocks, n, hessian, kind):
    red, exp, R, w = _pass_case(dev, n, kind, nblocks, hessian=hessian)
    LC.assert_pass_matches(red, R, w, CW, exp, hessian)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("hessian", [True, False])
def test_pass_default_grid_mostly_idle(dev, hessian, kind):
    red, exp, R, w = _pass_case(dev, 1000, kind, None, hessian=hessian)
    LC.assert_pass_matches(red, R, w, CW, exp, hessian)


# ---- B. the hole -----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("hole", [(0, 91), (37, 91), (64, 64), (909, 91), (500, 0)])
def test_pass_steps_over_the_hole(dev, hole, kind):
    """The rows inside the hole are NaN with label 1: any contribution from them shows."""
    rows, R = LC.rows_case(1000, kind)
    rows = rows.clone()
    at, ln = hole
    if kind == "bf16":
        rows[at:at + ln] = float("nan")
        rows[at:at + ln, 31] = 1.0
    else:
        rows[at:at + ln] = 0x7F  # e4m3 NaN
        rows[at:at + ln, 31] = int(ref.fp8_encode(np.array([1.0], dtype=np.float32))[0])
    w = LC.weights_case()
    red = L.logreg_pass(rows.to(dev), torch.from_numpy(w), CW, True, LC.FP8_SCALE, hole=hole, nblocks=1, full=True)
    Rh = np.delete(R, slice(at, at + ln), axis=0)
    exp = ref.logreg_pass_tiles(Rh, w, CW, 1, 1, 0, 4)
    assert np.all(np.isfinite(red))
    LC.assert_pass_matches(red, Rh, w, CW, exp)


# ---- C. tile subsets and the sub-sampled Hessian ---------------------------------------------
SUBSETS = [(1, 2), (1, 3), (1, 8), (2, 1), (3, 2), (4, 16), (16, 16)]


def _subset_rows(nblocks, sub, hs):
    return 64 * 4 * nblocks * sub * 2 * hs + 29  # every wave's Hessian phase wraps twice


@pytest.mark.parametrize("nblocks", [1, 3])
@pytest.mark.parametrize("sub,hs", SUBSETS)
def test_pass_tile_subsets_bf16(dev, sub, hs, nblocks):
    red, exp, R, w = _pass_case(dev, _subset_rows(nblocks, sub, hs), "bf16", nblocks, hess_stride=hs, sub=sub)
    visited = (np.arange(R.shape[0]) // 64) % sub == 0
    LC.assert_pass_matches(red, R[visited], w, CW, exp)


@pytest.mark.parametrize("nblocks,sub,hs", [(1, 3, 2), (3, 1, 8)])
def test_pass_tile_subsets_fp8(dev, nblocks, sub, hs):
    red, exp, R, w = _pass_case(dev, _subset_rows(nblocks, sub, hs), "fp8", nblocks, hess_stride=hs, sub=sub)
    visited = (np.arange(R.shape[0]) // 64) % sub == 0
    LC.assert_pass_matches(red, R[visited], w, CW, exp)


# ---- D. value edges --------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_pass_saturated_logits(dev, kind):
    """Weights scaled until z spans beyond +-200 on both labels: the loss still is logaddexp (the
    clamp at |z| = 80 only bounds exp), g and H stay finite."""
    rows, R = LC.rows_case(257, kind)
    w = (LC.weights_case() * 40.0).astype(np.float32).astype(np.float64)
    z = R[:, :31] @ w[:31]
    for lab in (0, 1):
        zl = z[R[:, 31] == lab]
        assert zl.min() < -200 and zl.max() > 200
    red = L.logreg_pass(rows.to(dev), torch.from_numpy(w), CW, True, LC.FP8_SCALE, nblocks=1, full=True)
    exp = ref.logreg_pass_tiles(R, w, CW, 1, 1, 0, 4)
    assert np.all(np.isfinite(red))
    assert red[33] == exp[33] and red[34] == exp[34]
    assert abs(red[32] - exp[32]) / exp[32] < 1e-5, (red[32], exp[32])


@pytest.mark.parametrize("kind", KINDS)
def test_pass_zero_weights(dev, kind):
    red, exp, R, w = _pass_case(dev, 257, kind, 1, w=np.zeros(32))
    assert abs(red[32] - red[33] * np.log(2.0)) <= 1e-5 * red[33] * np.log(2.0)
    LC.assert_pass_matches(red, R, w, CW, exp)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("class_w", [(1.0, 0.0), (0.0, 1.0), (1.0, 3.0)])
def test_pass_class_weights(dev, class_w, kind):
    red, exp, R, w = _pass_case(dev, 257, kind, 1, class_w=class_w)
    LC.assert_pass_matches(red, R, w, class_w, exp)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("label", [0.0, 1.0])
def test_pass_single_class(dev, label, kind):
    rows, R = LC.rows_case(257, kind)
    rows, R = rows.clone(), R.copy()
    one = torch.tensor(label, dtype=torch.bfloat16) if kind == "bf16" else int(
        ref.fp8_encode(np.array([label], dtype=np.float32))[0])
    rows[:, 31] = one
    R[:, 31] = label
    w = LC.weights_case()
    red = L.logreg_pass(rows.to(dev), torch.from_numpy(w), CW, True, LC.FP8_SCALE, nblocks=1, full=True)
    exp = ref.logreg_pass_tiles(R, w, CW, 1, 1, 0, 4)
    LC.assert_pass_matches(red, R, w, CW, exp)


# ---- E. logreg_reduce_kernel -----------------------------------------------------------------
SENTINEL = -12345.678


@pytest.mark.parametrize("nblocks", [1, 63, 64, 65, 767, 768, 769, 1024])
def test_reduce_is_exact_on_dyadic_partials(dev, nblocks):
    """Small integers x 2^-8: every fp64 summation order is exact, so out[:ncols] is the column sum
    bitwise; out[ncols:] keeps what it held (a gradient pass keeps red[34..]); done: untouched."""
    m = native()
    rng = np.random.default_rng(nblocks)
    part = (rng.integers(-64, 65, (nblocks, L.PART_STRIDE)) / 256.0).astype(np.float32)
    sums = part.astype(np.float64).sum(0)
    pd = torch.from_numpy(part).to(dev)
    done = torch.zeros(1, dtype=torch.int32, device=dev)
    s = stream_of(pd)
    for ncols in (34, 36, L.PART_STRIDE):
        out = torch.full((L.PART_STRIDE,), SENTINEL, dtype=torch.float64, device=dev)
        m.logreg_reduce(ptr(pd), nblocks, ncols, ptr(out), ptr(done), s)
        got = out.cpu().numpy()
        np.testing.assert_array_equal(got[:ncols], sums[:ncols])
        assert np.all(got[ncols:] == SENTINEL)
        m.logreg_reduce(ptr(pd), nblocks, ncols, ptr(out), 0, s)  # no done flag: the same sums
        np.testing.assert_array_equal(out.cpu().numpy(), got)
    done.fill_(1)
    out = torch.full((L.PART_STRIDE,), SENTINEL, dtype=torch.float64, device=dev)
    m.logreg_reduce(ptr(pd), nblocks, L.PART_STRIDE, ptr(out), ptr(done), s)
    assert np.all(out.cpu().numpy() == SENTINEL)


# ---- F. newton_update against NewtonStateRef -------------------------------------------------
def _w_case(d, fi):
    """Active weights random, inactive coordinates hold sentinels that must survive."""
    w = np.random.default_rng(40 + d).normal(0, 0.2, 32)
    w[d:30] = 0.125
    w[30] = 0.3 if fi else -0.625
    w[31] = 0.0
    return w


def _check_update(dev, st, red, d=30, C=1.0, tol=1e-9, max_iter=25, fi=True, phase_start=False, affine=None):
    """One kernel launch and one mirror update from the same red and state; returns the mirror."""
    before = LC.state_vector(st)
    w_before = st.w.copy()
    w32_0 = np.full(32, 7.5, dtype=np.float32)
    got, w32, done = L.newton_update_once(red, before, d, C, tol, max_iter, fi, phase_start, affine, 0, w32_0, dev)
    took_step = st.n_accepted
    st.update(red, d, C, tol, max_iter, fi, phase_start, affine)
    took_step = st.n_accepted - took_step
    exp = LC.state_vector(st)
    for slot in (L.S_ITER, L.S_BACKTRACKS, L.S_NACC, L.S_CONV):
        assert got[slot] == exp[slot], (slot, got[slot], exp[slot])
    assert done == int(st.done)
    assert got[L.S_OBJ] == pytest.approx(exp[L.S_OBJ], rel=1e-13)
    assert got[L.S_GMAX] == pytest.approx(exp[L.S_GMAX], rel=1e-13)
    if np.isfinite(exp[L.S_OBJPREV]):
        assert got[L.S_OBJPREV] == pytest.approx(exp[L.S_OBJPREV], rel=1e-13)
    else:
        assert got[L.S_OBJPREV] == exp[L.S_OBJPREV]
    gs, gw, gp = got[L.S_STEP:L.S_STEP + 32], got[L.S_W:L.S_W + 32], got[L.S_WPREV:L.S_WPREV + 32]
    if took_step:
        bound = LC.step_bound(red, w_before, d, C, fi, affine, st.step)
        assert np.max(np.abs(gs - st.step)) <= bound, (np.max(np.abs(gs - st.step)), bound)
        assert np.max(np.abs(gw - st.w)) <= bound + 2.0 ** -52 * np.max(np.abs(st.w))
        np.testing.assert_array_equal(gp, w_before)
    else:  # backtrack (exact halving), converged or no-op: the same fp64 operations
        np.testing.assert_array_equal(gs, st.step)
        np.testing.assert_array_equal(gw, st.w)
        np.testing.assert_array_equal(gp, st.w_prev)
    idx = list(range(d)) + ([30] if fi else [])
    off = np.setdiff1d(np.arange(32), idx)
    np.testing.assert_array_equal(gw[off], w_before[off])  # inactive coordinates: untouched
    np.testing.assert_array_equal(gs[off], exp[L.S_STEP:L.S_STEP + 32][off])
    np.testing.assert_array_equal(got[L.S_VEL:L.S_VEL + 32], 0.0)
    np.testing.assert_array_equal(got[135:], 0.0)
    # the fp32 weights the next pass reads
    if affine is None:
        e32 = gw.astype(np.float32)
        e32[31] = 0.0
        assert np.array_equal(w32.view(np.uint32), e32.view(np.uint32))
    else:
        f = ref.fold_weights(gw, affine).astype(np.float32)
        ulp = np.spacing(np.abs(f))
        assert np.all(np.abs(w32 - f) <= ulp), np.max(np.abs(w32 - f) / ulp)
        assert w32[31] == 0.0
    return st


@pytest.mark.parametrize("d,fi", [(30, True), (30, False), (20, True), (12, False), (1, True)])
def test_update_takes_a_step(dev, d, fi):
    red = LC.synth_red(LC.RED_SEED)
    st = _check_update(dev, LC.make_state(_w_case(d, fi)), red, d=d, fi=fi)
    assert (st.iter, st.n_accepted, st.backtracks, st.done) == (1, 1, 0, False)
    # a second step from a mid-fit state with a better objective behind it
    _, _, _, obj, gmax = ref.newton_system(red, st.w, d, 1.0, fi)
    st.obj_prev = obj * 1.01
    assert gmax > 1e-9 * 1.01
    st = _check_update(dev, st, red, d=d, fi=fi)
    assert (st.iter, st.n_accepted) == (2, 2)


def _mid_fit(d=30, fi=True, worse=True, it=3, backtracks=2):
    """A mid-fit state whose objective is 1 % above (or below) the last accepted one."""
    red = LC.synth_red(LC.RED_SEED)
    w = _w_case(d, fi)
    step = np.zeros(32)
    step[:d] = np.random.default_rng(41).normal(0, 0.1, d)
    st = LC.make_state(w, step, it=it, backtracks=backtracks, n_accepted=3)
    _, _, _, obj, gmax = ref.newton_system(red, st.w, d, 1.0, fi)
    st.obj_prev = obj / 1.01 if worse else obj * 1.01
    return red, st, gmax


def test_update_backtracks(dev):
    red, st, _ = _mid_fit()
    st = _check_update(dev, st, red)
    assert (st.iter, st.backtracks, st.n_accepted) == (4, 3, 3)


def test_update_phase_start_suppresses_the_backtrack(dev):
    red, st, _ = _mid_fit()
    st = _check_update(dev, st, red, phase_start=True)
    assert (st.iter, st.backtracks, st.n_accepted) == (4, 0, 4)


@pytest.mark.parametrize("backtracks,accepted", [(39, 3), (40, 4)])
def test_update_backtrack_cap(dev, backtracks, accepted):
    red, st, _ = _mid_fit(it=50, backtracks=backtracks)
    st = _check_update(dev, st, red, max_iter=100)
    assert st.n_accepted == accepted and st.backtracks == (40 if accepted == 3 else 0)


def test_update_converges(dev):
    red, st, gmax = _mid_fit(worse=False)
    st = _check_update(dev, st, red, tol=1.01 * gmax)
    assert st.converged and st.done and st.n_accepted == 3
    red, st, gmax = _mid_fit(worse=False)
    st = _check_update(dev, st, red, tol=gmax / 1.01)  # 1 % short of tol: a step instead
    assert not st.done and st.n_accepted == 4


def test_update_stops_at_max_iter(dev):
    red, st, gmax = _mid_fit(worse=False, it=24)
    st = _check_update(dev, st, red, max_iter=25)
    assert st.done and not st.converged and st.iter == 25
    red, st, gmax = _mid_fit(worse=True, it=24)  # a backtrack on the last iteration ends the fit too
    st = _check_update(dev, st, red, max_iter=25)
    assert st.done and not st.converged and st.backtracks == 3


@pytest.mark.parametrize("affine", [False, True])
def test_update_done_is_a_no_op(dev, affine):
    red, st, _ = _mid_fit()
    before = LC.state_vector(st)
    w32_0 = np.arange(32, dtype=np.float32) + 0.5
    aff = LC.affine_case(LC.AFFINE_SEED) if affine else None
    got, w32, done = L.newton_update_once(red, before, 30, 1.0, 1e-9, 25, True, False, aff, 1, w32_0, dev)
    assert done == 1
    assert np.array_equal(got.view(np.uint64), before.view(np.uint64))
    assert np.array_equal(w32.view(np.uint32), w32_0.view(np.uint32))


@pytest.mark.parametrize("d,fi", [(30, True), (20, True)])
def test_update_rescales_the_hessian_by_its_weight(dev, d, fi):
    """red[34] = red[33] / 4: H counts four times -- the step of 4 H at equal weights."""
    red = LC.synth_red(LC.RED_SEED, 64.0, 16.0)
    st = _check_update(dev, LC.make_state(_w_case(d, fi)), red, d=d, fi=fi)
    scaled = LC.synth_red(LC.RED_SEED)
    scaled[64:] *= 4.0
    twin = LC.make_state(_w_case(d, fi))
    twin.update(scaled, d, 1.0, 1e-9, 25, fi)
    np.testing.assert_allclose(st.step, twin.step, rtol=1e-12)


@pytest.mark.parametrize("S,SH", [(64.0, 0.0), (0.0, 0.0), (0.0, 16.0)])
def test_update_weight_fallbacks(dev, S, SH):
    st = _check_update(dev, LC.make_state(_w_case(30, True)), LC.synth_red(LC.RED_SEED, S, SH))
    assert st.n_accepted == 1


@pytest.mark.parametrize("d,fi", [(30, True), (20, True), (12, False)])
def test_update_affine(dev, d, fi):
    aff = LC.affine_case(LC.AFFINE_SEED, d)
    red = LC.synth_red(LC.RED_SEED)
    st = _check_update(dev, LC.make_state(_w_case(d, fi)), red, d=d, fi=fi, affine=aff)
    assert st.n_accepted == 1
    red, st, _ = _mid_fit(d, fi)  # the affine map does not move the objective: still a backtrack
    st = _check_update(dev, st, red, d=d, fi=fi, affine=aff)
    assert st.backtracks == 3


# ---- G. the fused tail -----------------------------------------------------------------------
def _fused_rows(nblocks):
    return min(64 * 4 * nblocks + 5, 20_000)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("nblocks", [1, 15, 16, 17, 33, None])
def test_fused_tail_matches_unfused(dev, nblocks, kind, monkeypatch):
    """One Hessian iteration, then one gradient-only iteration, fused (newton_fused_tail: group
    sums of 16 blocks) against pass + logreg_reduce + newton_update from the same rows and start."""
    m = native()
    nb = nblocks or m.logreg_pass_blocks(0 if kind == "bf16" else 1)
    rows, R = LC.rows_case(_fused_rows(nb), kind)
    rows = rows.to(dev)
    w0 = LC.weights_case(seed=9, scale=0.1)
    tickets = (int(m.NEWTON_FUSE_WORDS) - 128 * 576)  # 8-byte words ahead of the group sums
    assert tickets == 65
    out = {}
    for fuse in ("0", "1"):
        monkeypatch.setenv("FDX_NEWTON_FUSE", fuse)
        ws = L.LRWorkspace(dev, nblocks)
        ws.reset(w0, CW)
        snaps = []
        for hessian in (1, 0):
            held = ws.red.cpu().numpy().copy()
            L.newton_iteration(rows, ws, hessian, fp8_scale=LC.FP8_SCALE)
            part = ws.partial[:nb * L.PART_STRIDE].cpu().double().numpy().reshape(nb, L.PART_STRIDE)
            snaps.append((ws.red.cpu().numpy().copy(), ws.state.cpu().numpy().copy(), np.abs(part).sum(0), held))
        assert int(ws.done.cpu()[0]) == 0
        assert not np.any(ws.newton_fuse[:tickets].cpu().numpy())
        out[fuse] = snaps
    for it, hessian in enumerate((1, 0)):
        red_u, st_u, abs_u, _ = out["0"][it]
        red_f, st_f, _, held_f = out["1"][it]
        # the slots the pass wrote (35..63 are unused: no block stores them)
        cols = np.r_[0:35, 64:L.PART_STRIDE] if hessian else np.r_[0:L.GRAD_SLOTS]
        assert np.all(np.abs(red_f[cols] - red_u[cols]) <= 1e-12 * abs_u[cols])
        H = red_f[64:].reshape(32, 32)
        assert np.array_equal(H, H.T)
        if not hessian:  # a gradient pass keeps the held Hessian and its weight
            assert np.array_equal(red_f[34:].view(np.uint64), held_f[34:].view(np.uint64))
            assert np.array_equal(red_u[34:].view(np.uint64), out["0"][it][3][34:].view(np.uint64))
        for slot in (L.S_ITER, L.S_BACKTRACKS, L.S_NACC, L.S_CONV):
            assert st_f[slot] == st_u[slot]
        assert st_f[L.S_OBJ] == pytest.approx(st_u[L.S_OBJ], rel=1e-13)
        assert st_f[L.S_GMAX] == pytest.approx(st_u[L.S_GMAX], rel=1e-12)
        if st_u[L.S_NACC] > (out["0"][it - 1][1][L.S_NACC] if it else 0):
            w_at = st_u[L.S_WPREV:L.S_WPREV + 32]
            bound = LC.step_bound(red_u, w_at, 30, 1.0, True, None, st_u[L.S_STEP:L.S_STEP + 32])
            assert np.max(np.abs(st_f[L.S_STEP:L.S_STEP + 32] - st_u[L.S_STEP:L.S_STEP + 32])) <= bound
            assert np.max(np.abs(st_f[L.S_W:L.S_W + 32] - st_u[L.S_W:L.S_W + 32])) <= bound + 2.0 ** -52
        else:
            np.testing.assert_array_equal(st_f[:128], st_u[:128])
    # the first iteration took a Newton step on the whole data in both forms
    assert out["0"][0][1][L.S_NACC] == 1 and out["0"][0][0][34] == out["0"][0][0][33]


# ---- H. logreg_init / logreg_fold ------------------------------------------------------------
def _check_init(ws, w_exp, class_w, aff=None):
    st = ws.state.cpu().numpy()
    np.testing.assert_array_equal(st[L.S_W:L.S_W + 32], w_exp)
    np.testing.assert_array_equal(st[L.S_WPREV:L.S_WPREV + 32], w_exp)
    assert st[L.S_OBJPREV] == np.inf
    rest = np.delete(st, np.r_[0:64, L.S_OBJPREV])
    assert not np.any(rest)
    assert int(ws.done.cpu()[0]) == 0
    np.testing.assert_array_equal(ws.class_w.cpu().numpy(), np.asarray(class_w, dtype=np.float32))
    w32 = ws.w32.cpu().numpy()
    if aff is None:
        e32 = w_exp.astype(np.float32)
        e32[31] = 0.0
        assert np.array_equal(w32.view(np.uint32), e32.view(np.uint32))
    else:
        f = ref.fold_weights(w_exp, aff).astype(np.float32)
        assert np.all(np.abs(w32 - f) <= np.spacing(np.abs(f)))
        assert w32[31] == 0.0


@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("source", ["w0", "w0_dev"])
def test_init_writes_the_whole_blob(dev, source, affine):
    ws = L.LRWorkspace(dev, 1)
    ws.state.fill_(3.25)  # a previous fit's leftovers
    ws.w32.fill_(3.25)
    ws.done.fill_(1)
    w0 = np.r_[np.random.default_rng(50).normal(0, 0.3, 30), -0.75, 0.0]
    aff = LC.affine_case(LC.AFFINE_SEED) if affine else None
    aff_dev = torch.from_numpy(aff).to(dev) if affine else None
    if source == "w0":
        ws.reset(w0, (0.5, 2.0), ptr(aff_dev) if affine else 0)
    else:  # another fit's device state: weights first, the label slot ignored
        other = torch.zeros(L.STATE_SIZE, dtype=torch.float64, device=dev)
        other[:32] = torch.from_numpy(w0)
        other[31] = 9.0
        other[32:] = 4.5
        ws.reset(np.full(32, -1.0), (0.5, 2.0), ptr(aff_dev) if affine else 0, ptr(other))
    _check_init(ws, w0, (0.5, 2.0), aff)


def test_fold_kernel(dev):
    ws = L.LRWorkspace(dev, 1)
    w = np.r_[np.random.default_rng(51).normal(0, 0.3, 30), 0.4, 0.0]
    ws.reset(w, CW)
    aff = LC.affine_case(LC.AFFINE_SEED)
    aff_dev = torch.from_numpy(aff).to(dev)
    native().logreg_fold(ptr(ws.state), ptr(aff_dev), ptr(ws.w32), stream_of(ws.state))
    w32 = ws.w32.cpu().numpy()
    f = ref.fold_weights(w, aff).astype(np.float32)
    assert np.all(np.abs(w32 - f) <= np.spacing(np.abs(f)))
    assert w32[31] == 0.0
    np.testing.assert_array_equal(ws.state.cpu().numpy()[:32], w)
