"""The fp64 oracles the logistic-regression kernel tests stand on (ops/reference.py
logreg_pass_tiles, NewtonStateRef with phase_start / affine; tests/_logreg_cases.py): they agree
with the plain pass, their tile subsets partition the rows, the affine map is the change of
variables it claims to be, and the mirror takes the update kernel's documented decisions."""
import numpy as np
import pytest
import torch

import _logreg_cases as LC
from fraud_detection_amd.ops import logreg as L
from fraud_detection_amd.ops import reference as ref

CW = (1.0, 3.0)


def _rows(n):
    return LC.rows_case(n, "bf16")[1]


def test_tiles_default_is_the_plain_pass():
    R, w = _rows(1000), LC.weights_case()
    for gw in (4, 12, 4096):
        red = ref.logreg_pass_tiles(R, w, CW, 1, 1, 0, gw)
        exp = ref.pack_reduced(*ref.logreg_pass(R, w, CW))
        exp[34] = exp[33]  # pack_reduced leaves the Hessian weight out: every row feeds H here
        np.testing.assert_array_equal(red, exp)
    grad_only = ref.logreg_pass_tiles(R, w, CW, 1, 1, 0, 4, hessian=False)
    assert grad_only[34] == 0 and not np.any(grad_only[64:])
    np.testing.assert_array_equal(grad_only[:34], red[:34])


@pytest.mark.parametrize("sub", [2, 3, 16])
def test_sub_phases_partition_the_pass(sub):
    R, w = _rows(64 * 37 + 11), LC.weights_case()
    full = ref.logreg_pass_tiles(R, w, CW, 1, 1, 0, 12)
    parts = [ref.logreg_pass_tiles(R, w, CW, 1, sub, ph, 12) for ph in range(sub)]
    tot = np.sum(parts, axis=0)
    assert tot[33] == full[33] and tot[34] == full[33]
    np.testing.assert_allclose(tot[:33], full[:33], rtol=1e-12, atol=1e-12 * np.abs(full[:33]).max())
    np.testing.assert_allclose(tot[64:], full[64:], rtol=1e-12, atol=1e-12 * np.abs(full[64:]).max())
    # phase ph holds exactly the tiles t with t mod sub == ph
    t = np.arange(R.shape[0]) // 64
    for ph in range(sub):
        s = np.where(R[t % sub == ph, 31] > 0.5, CW[1], CW[0]).sum()
        assert parts[ph][33] == s


@pytest.mark.parametrize("hs,gw,sub", [(2, 4, 1), (3, 4, 1), (8, 12, 1), (2, 12, 3), (16, 4, 4)])
def test_hessian_phases_partition_each_waves_tiles(hs, gw, sub):
    """Over the hess_stride possible wave phases every tile of a wave feeds H exactly once: the
    feeding sets of waves w, w + 1, ..., w + hs - 1 (mod hs) at one tile index i are disjoint and
    cover it.  Checked through the weights first (all-zero rows of weight 1: red[33] / red[34] count
    rows), then on real rows against the Hessian of exactly the feeding tiles."""
    ntiles = gw * sub * (2 * hs + 1) + 3
    R = np.zeros((64 * ntiles, 32))
    w = np.zeros(32)
    red = ref.logreg_pass_tiles(R, w, (1.0, 1.0), hs, sub, 0, gw)
    t = np.arange(ntiles)
    visited = t[t % sub == 0]
    j = visited // sub
    wave, i = j % gw, j // gw
    assert red[33] == 64 * len(visited)
    feeds = (wave % hs + i) % hs == 0
    assert red[34] == hs * 64 * feeds.sum()
    # per wave: tile i feeds iff i == -wave (mod hs); the hs shifts of that rule partition the tiles
    for wv in range(gw):
        mine = i[wave == wv]
        got = np.zeros(len(mine), dtype=int)
        for shift in range(hs):
            got += ((wv + shift) % hs + mine) % hs == 0
        assert np.all(got == 1)
    # and the oracle's H is hs x the Hessian of exactly those tiles
    Rr, wr = _rows(64 * ntiles), LC.weights_case()
    red = ref.logreg_pass_tiles(Rr, wr, CW, hs, sub, 0, gw)
    keep = np.repeat(np.isin(t, visited[feeds]), 64)
    _, _, wh, H = ref.logreg_pass(Rr[keep], wr, CW)
    assert red[34] == hs * wh
    np.testing.assert_array_equal(red[64:], hs * H.reshape(-1))


def test_hole_is_deleting_the_block():
    rows, R = LC.rows_case(1000, "bf16")
    w = LC.weights_case()
    Rh = np.delete(R, slice(37, 37 + 91), axis=0)
    got = L.logreg_pass(rows, torch.from_numpy(w), CW, hole=(37, 91), nblocks=1, full=True)
    np.testing.assert_array_equal(got, ref.logreg_pass_tiles(Rh, w, CW, 1, 1, 0, 4))
    plain = L.logreg_pass(rows, torch.from_numpy(w), CW)
    np.testing.assert_array_equal(plain[0], ref.logreg_pass(R, w, CW)[0])  # the unchanged default path


def test_grad_abs_bounds_the_gradient():
    R, w = _rows(500), LC.weights_case()
    g = ref.logreg_pass(R, w, CW)[0]
    assert np.all(np.abs(g) <= ref.logreg_grad_abs(R, w, CW) * (1 + 1e-12))
    assert ref.logreg_grad_abs(R, w, CW)[31] == 0.0


@pytest.mark.parametrize("d,fi", [(30, True), (20, True), (12, False)])
def test_affine_map_is_the_change_of_variables(d, fi):
    """red over shifted rows S with folded weights, updated with affine == red over standardized
    rows Z = (S - c) inv with no affine: same new state to 1e-12 relative."""
    rng = np.random.default_rng(7 + d)
    n = 400
    aff = LC.affine_case(3, d)
    c, inv = aff[:32], aff[32:]
    S = rng.normal(0, 1.5, (n, 32))
    S[:, d:30] = 0.0
    S[:, 30] = 1.0
    S[:, 31] = rng.random(n) < 0.3
    Z = (S - c) * inv
    Z[:, 30], Z[:, 31] = 1.0, S[:, 31]
    w = np.zeros(32)
    w[:d] = rng.normal(0, 0.3, d)
    w[30] = -0.5 if fi else 0.0
    v = ref.fold_weights(w, aff)
    np.testing.assert_allclose(S[:, :31] @ v[:31], Z[:, :31] @ w[:31], rtol=1e-12, atol=1e-12)
    red_s = ref.pack_reduced(*ref.logreg_pass(S, v, CW))
    red_z = ref.pack_reduced(*ref.logreg_pass(Z, w, CW))
    a, b = LC.make_state(w), LC.make_state(w)
    a.update(red_s, d, 1.0, 1e-9, 25, fi, affine=aff)
    b.update(red_z, d, 1.0, 1e-9, 25, fi)
    assert a.n_accepted == b.n_accepted == 1
    sa, sb = LC.state_vector(a), LC.state_vector(b)
    np.testing.assert_allclose(sa, sb, rtol=1e-12, atol=1e-12 * np.abs(sb[:96]).max())


def test_mirror_defaults_keep_the_cpu_fit():
    """phase_start / affine default off: the CPU Newton fit is the fit of the plain recurrence."""
    rows = LC.rows_case(3000, "bf16")[0]
    fit = L.newton_fit(rows, tol=1e-9, max_iter=30)
    R = ref.rows_to_f32(rows).double().numpy()
    st = ref.NewtonStateRef(np.zeros(32))
    while not st.done:
        st.update(ref.pack_reduced(*ref.logreg_pass(R, st.w, (1.0, 1.0))), 30, 1.0, 1e-9, 30, True, False, None)
    assert fit.converged and st.converged and fit.n_iter == st.iter
    np.testing.assert_array_equal(fit.w, st.w)
    g = ref.logreg_pass(R, st.w, (1.0, 1.0))[0] / R.shape[0]
    g[:30] += st.w[:30] / R.shape[0]
    assert np.abs(g[:31]).max() <= 1e-9


def _decision_case():
    red = LC.synth_red(11)
    w = np.r_[np.random.default_rng(12).normal(0, 0.2, 30), 0.3, 0.0]
    step = np.r_[np.random.default_rng(13).normal(0, 0.1, 31), 0.0]
    _, _, _, obj, gmax = ref.newton_system(red, w, 30, 1.0, True)
    return red, w, step, obj, gmax


def test_mirror_backtracks_on_a_worse_objective():
    red, w, step, obj, gmax = _decision_case()
    st = LC.make_state(w, step, it=3, obj_prev=obj / 1.01, backtracks=2, n_accepted=3)
    wp = st.w_prev.copy()
    st.update(red, 30, 1.0, 1e-9, 25)
    assert (st.iter, st.backtracks, st.n_accepted, st.done) == (4, 3, 3, False)
    np.testing.assert_array_equal(st.step, 0.5 * step)
    np.testing.assert_array_equal(st.w, wp + 0.5 * step)
    assert st.obj == obj and st.gmax == 0.5 and st.obj_prev == obj / 1.01


def test_mirror_phase_start_forgets_the_previous_phase():
    red, w, step, obj, gmax = _decision_case()
    st = LC.make_state(w, step, it=3, obj_prev=obj / 1.01, backtracks=2, n_accepted=3)
    w_at = st.w.copy()
    st.update(red, 30, 1.0, 1e-9, 25, phase_start=True)
    assert (st.iter, st.backtracks, st.n_accepted, st.done) == (4, 0, 4, False)
    assert st.obj_prev == obj and st.gmax == gmax
    np.testing.assert_array_equal(st.w_prev, w_at)
    # the first iteration of a fit never backtracks either
    st = LC.make_state(w, step, it=0, obj_prev=obj / 1.01)
    st.update(red, 30, 1.0, 1e-9, 25)
    assert st.n_accepted == 1 and st.backtracks == 0


def test_mirror_backtrack_cap():
    red, w, step, obj, gmax = _decision_case()
    st = LC.make_state(w, step, it=50, obj_prev=obj / 1.01, backtracks=39, n_accepted=3)
    st.update(red, 30, 1.0, 1e-9, 100)
    assert st.backtracks == 40 and st.n_accepted == 3
    st = LC.make_state(w, step, it=50, obj_prev=obj / 1.01, backtracks=40, n_accepted=3)
    st.update(red, 30, 1.0, 1e-9, 100)
    assert st.backtracks == 0 and st.n_accepted == 4  # capped: the step is taken
    st = LC.make_state(w, step, it=50, obj_prev=obj / 1.01, backtracks=40, n_accepted=3)
    st.update(red, 30, 1.0, 2 * gmax, 100)
    assert st.converged and st.done and st.backtracks == 40  # capped and within tol: converged


def test_mirror_convergence_and_max_iter():
    red, w, step, obj, gmax = _decision_case()
    st = LC.make_state(w, step, it=3, obj_prev=obj * 1.01)
    st.update(red, 30, 1.0, 1.01 * gmax, 25)
    assert st.converged and st.done and st.iter == 4 and st.n_accepted == 0
    st = LC.make_state(w, step, it=24, obj_prev=obj * 1.01)
    st.update(red, 30, 1.0, gmax / 1.01, 25)
    assert st.done and not st.converged and st.iter == 25 and st.n_accepted == 1
    before = LC.state_vector(st)
    st.update(red, 30, 1.0, 1e-9, 25)  # done: a no-op
    np.testing.assert_array_equal(LC.state_vector(st), before)


def test_mirror_rescales_a_subsampled_hessian():
    """H over a quarter of the weight (red[34] = red[33] / 4) counts four times; red[34] = 0 and
    red[33] = 0 fall back to 1."""
    w = np.r_[np.random.default_rng(12).normal(0, 0.2, 30), 0.3, 0.0]
    base = LC.synth_red(11)
    quarter = base.copy()
    quarter[34] = 0.25 * base[33]
    scaled = base.copy()
    scaled[64:] *= 4.0
    a, b = LC.make_state(w), LC.make_state(w)
    a.update(quarter, 30, 1.0, 1e-9, 25)
    b.update(scaled, 30, 1.0, 1e-9, 25)
    np.testing.assert_allclose(a.step, b.step, rtol=1e-13)
    nosh = base.copy()
    nosh[34] = 0.0
    c, e = LC.make_state(w), LC.make_state(w)
    c.update(nosh, 30, 1.0, 1e-9, 25)
    e.update(base, 30, 1.0, 1e-9, 25)
    np.testing.assert_array_equal(c.step, e.step)
    nos = base.copy()
    nos[33] = nos[34] = 0.0
    one = base.copy()
    one[33] = one[34] = 1.0
    c, e = LC.make_state(w), LC.make_state(w)
    c.update(nos, 30, 1.0, 1e-9, 25)
    e.update(one, 30, 1.0, 1e-9, 25)
    np.testing.assert_array_equal(c.step, e.step)


def test_synth_red_is_well_conditioned():
    """The seeds the device tests commit to: cond(A) <= 1e3 on every active block they use."""
    for d, fi in [(30, True), (30, False), (20, True), (12, False), (1, True)]:
        for S, SH in [(64.0, None), (64.0, 16.0), (64.0, 0.0), (0.0, 0.0)]:
            for aff in (None, LC.affine_case(LC.AFFINE_SEED, d)):
                _, A, _, _, _ = ref.newton_system(LC.synth_red(LC.RED_SEED, S, SH), np.zeros(32), d, 1.0, fi, aff)
                assert np.linalg.cond(A) <= 1e3, (d, fi, S, SH, aff is not None)
