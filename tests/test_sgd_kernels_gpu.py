"""Every kernel on the SGD path of logreg.hip against a plain fp64 oracle, at the smallest shapes
where it can still go wrong: the FUSE passes' fixed-point sums (A: row-count, replica, idle-block,
hole, poison and value edges, housekeeping of the accumulators), sgd_step_kernel's reduction (B:
bitwise on integer partials), sgd_update / sgd_update_fixed against SgdStateRef on the same sums and
state (C: every branch, both affine branches), the fused per-step launch against its parts (D:
bitwise) and the persistent launch on 1- and 2-block grids against the per-step launches (E:
bitwise).  Oracles: ops/reference.py sgd_pass_sums / sgd_sums_abs / SgdStateRef; cases and the
derivation of the bounds: tests/_sgd_cases.py.  sgd_recover_kernel is reached only by
test_sgd_gpu.py's recovery test: nothing here forces a barrier timeout.

Bounds (none tuned to the kernels): weight sums exact; loss and curvature 1e-5 relative, gradient
1e-5 of its absolute-term sum + 1e-7, each plus half a fixed-point unit per working wave and the
per-sample integer roundings of the virtual samples (_sgd_cases.pass_bounds); update kernels
2^-46 of each slot's absolute-term sum (SgdStateRef.mag), integer slots exact."""
import functools
import itertools

import numpy as np
import pytest
import torch

import _logreg_cases as LC
import _sgd_cases as SC
from fraud_detection_amd.ops import logreg as L
from fraud_detection_amd.ops import reference as ref
from fraud_detection_amd.ops.native import native, ptr

pytestmark = pytest.mark.gpu

CW = SC.CW
KINDS = ["bf16", "fp8"]
ARGS = dict(C=0.7, c=0.5, momentum=0.55, nb=3, tol=-1.0)  # of the update tests


@functools.lru_cache(maxsize=None)
def _dev_rows(n, kind, dev):
    return LC.rows_case(n, kind)[0].to(dev)


def _affine(on, d=30):
    return LC.affine_case(LC.AFFINE_SEED, d) if on else None


def _finite(q):
    """int64 sums that came from finite values (a NaN or an overflow converts to an extreme)."""
    return int(q.min()) > -2 ** 62 and int(q.max()) < 2 ** 62


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


# ---- A. the FUSE passes' sums against ref.sgd_pass_sums --------------------------------------
def _check_pass(dev, ws, n, kind, n_new, affine, blocks, rsub, phase, w=None, class_w=CW, hole=None, rows=None,
                check=True):
    """One sgd_pass_sums launch on ``ws`` and its oracle: (int64 sums, oracle, bound).  The
    accumulators and the ticket must be back at zero after every launch."""
    m = native()
    R = LC.rows_case(n, kind)[1]
    rows = _dev_rows(n, kind, dev) if rows is None else rows
    w = LC.weights_case() if w is None else w
    v, vt, pair = SC.virtual_case(n_new, dev) if n_new else (None, None, None)
    q = L.sgd_pass_sums_once(rows, w, rsub, phase, blocks, class_w, affine, v, hole, 0, LC.FP8_SCALE, ws)
    assert not np.any(ws.sgd_acc.cpu().numpy()), "accumulators / ticket not left zero"
    if hole is not None:
        R = np.delete(R, slice(hole[0], hole[0] + hole[1]), axis=0)
    exp = ref.sgd_pass_sums(R, w, class_w, rsub, phase, vt, affine)
    ab = ref.sgd_sums_abs(R, w, class_w, rsub, phase, vt)
    ns, npk, pair_max = 0, 0, None
    if n_new:
        mine = (vt[1] // ref.PICK_TILE) % rsub == phase
        ns = int(mine.sum())
        npk = int(np.unique(vt[1][mine]).size)  # picks of the phase that hold samples
        pair_max = pair[mine].max(0) if ns else np.zeros(32)
    W = SC.active_waves(R.shape[0], 4 * blocks, rsub, phase, SC.N_PICKS if n_new else 0)
    bound = SC.pass_bounds(ab, W, affine, ns, pair_max, float(m.SGD_SYN_Q), float(m.SGD_SYN_QL), npk)
    if check:
        got = q.astype(np.float64) / SC.FIX
        assert q[34] == 0
        assert got[33] == exp[33], (got[33], exp[33])
        err = np.abs(got - exp)
        assert np.all(err <= bound), (n, blocks, rsub, phase, int(np.argmax(err / np.maximum(bound, 1e-300))),
                                      float(np.max(err / np.maximum(bound, 1e-300))))
    return q, exp, bound


def _edge_rows(blocks, rsub):
    g = 64 * 4 * blocks * rsub
    return [1, 63, 64, 65, g - 1, g, g + 1, 3 * g + 17]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n_new", [0, 1, 900])
@pytest.mark.parametrize("affine", [False, True])
def test_pass_sums_row_count_edges(dev, affine, n_new, kind):
    ws = L.LRWorkspace(dev, 1)
    aff = _affine(affine)
    for blocks, rsub in itertools.product((1, 3), (1, 3)):
        for n in _edge_rows(blocks, rsub):
            for phase in range(rsub):
                q, _, _ = _check_pass(dev, ws, n, kind, n_new, aff, blocks, rsub, phase)
                if not n_new and phase * 64 >= n:  # a phase without a stored row: exactly zero
                    assert not np.any(q)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n_new", [0, 900])
def test_pass_sums_replica_and_idle_block_edges(dev, n_new, kind):
    """Grids around the accumulator replica count (block b adds into replica b mod R) and far beyond
    the row tiles (5000 rows are 79 tiles: most waves of 65 blocks are idle, the blocks from 20 on
    add nothing), then with a row tile for every wave of the largest grid, so that the blocks behind
    the first R -- the ones that wrap around to replica 0 -- carry sums."""
    R = int(native().SGD_REPLICAS)
    ws = L.LRWorkspace(dev, 1)
    for blocks in (R - 1, R, R + 1, 2 * R + 1):
        for rsub, phase in ((1, 0), (2, 1)):
            for aff in (None, _affine(True)):
                _check_pass(dev, ws, 5000, kind, n_new, aff, blocks, rsub, phase)
    n_busy = 64 * 4 * (2 * R + 1) + 17
    for blocks in (R, R + 1, 2 * R + 1):
        assert SC.active_waves(n_busy, 4 * blocks, 1, 0) == 4 * blocks
        _check_pass(dev, ws, n_busy, kind, n_new, None, blocks, 1, 0)


def _nan_rows(rows, kind, sl):
    """Rows ``sl`` NaN with label 1: any contribution from them shows."""
    if kind == "bf16":
        rows[sl] = float("nan")
        rows[sl, 31] = 1.0
    else:
        rows[sl] = 0x7F  # e4m3 NaN
        rows[sl, 31] = int(ref.fp8_encode(np.array([1.0], dtype=np.float32))[0])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n_new", [0, 900])
@pytest.mark.parametrize("hole", [(0, 91), (37, 91), (64, 64), (909, 91), (500, 0)])
def test_pass_sums_steps_over_the_hole(dev, hole, n_new, kind):
    """The hole's rows are NaN with label 1; so are 256 rows behind the table's end, which a virtual
    pass (row_end = stored rows + samples) must never read as stored rows."""
    n, (at, ln) = 1000, hole
    big = torch.zeros(n + 256, 32, dtype=LC.rows_case(1, kind)[0].dtype)
    big[:n] = LC.rows_case(n, kind)[0]
    _nan_rows(big, kind, slice(at, at + ln))
    _nan_rows(big, kind, slice(n, n + 256))
    rows = big.to(dev)[:n]
    ws = L.LRWorkspace(dev, 1)
    for blocks, rsub, phase, aff in ((1, 1, 0, None), (3, 3, 1, _affine(True))):
        q, _, _ = _check_pass(dev, ws, n, kind, n_new, aff, blocks, rsub, phase, hole=hole, rows=rows)
        assert _finite(q)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n_new", [0, 900])
def test_pass_sums_reads_only_its_phase(dev, n_new, kind):
    """Stored rows of the other phases are NaN: the sums are finite and the oracle's."""
    n, rsub = 3000, 3
    ws = L.LRWorkspace(dev, 1)
    tile = torch.arange(n) // 64
    for phase in range(rsub):
        rows = LC.rows_case(n, kind)[0].clone()
        _nan_rows(rows, kind, tile % rsub != phase)
        for blocks in (1, 3):
            _check_pass(dev, ws, n, kind, n_new, None, blocks, rsub, phase, rows=rows.to(dev))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n_new", [0, 900])
def test_pass_sums_value_edges(dev, n_new, kind):
    ws = L.LRWorkspace(dev, 1)
    n = 1000
    # w = 0: p = 1/2 everywhere
    q, exp, _ = _check_pass(dev, ws, n, kind, n_new, None, 1, 1, 0, w=np.zeros(32))
    assert abs(exp[35] - 0.25 * exp[33]) <= 1e-12 * exp[33]
    # |z| beyond the +-80 clamp on both labels: finite sums, the loss within its bound (the clamp only
    # bounds exp: the loss still is logaddexp), curvature >= 0
    w = (LC.weights_case() * 40.0).astype(np.float32).astype(np.float64)
    R = LC.rows_case(n, kind)[1]
    z = R[:, :31] @ w[:31]
    assert z.min() < -200 and z.max() > 200
    q, exp, bound = _check_pass(dev, ws, n, kind, n_new, None, 1, 1, 0, w=w, check=False)
    got = q / SC.FIX
    assert _finite(q) and q[34] == 0 and got[33] == exp[33]
    assert abs(got[32] - exp[32]) <= bound[32], (got[32], exp[32], bound[32])
    assert q[35] >= 0
    # class weights (1, 0) and (0, 1): slot 33 counts each class (positives: with the phase's samples)
    _, vt, _ = SC.virtual_case(n_new) if n_new else (None, None, None)
    for rsub, phase in ((1, 0), (3, 2)):
        y = R[(np.arange(n) // 64) % rsub == phase, 31]
        ns = int(np.sum((vt[1] // ref.PICK_TILE) % rsub == phase)) if n_new else 0
        qn, _, _ = _check_pass(dev, ws, n, kind, n_new, None, 3, rsub, phase, class_w=(1.0, 0.0))
        qp, _, _ = _check_pass(dev, ws, n, kind, n_new, None, 3, rsub, phase, class_w=(0.0, 1.0))
        assert qn[33] == int(np.sum(y == 0)) * 2 ** 20 and qp[33] == (int(np.sum(y == 1)) + ns) * 2 ** 20
        assert qn[33] > 0 and qp[33] > 0


@pytest.mark.parametrize("kind", KINDS)
def test_virtual_loss_below_the_clamp_newton_pass(dev, kind):
    """The Newton passes share the virtual samples' terms with the SGD passes: a sample whose logit
    lies below -80 must count its whole loss s softplus(-z) there too, as a stored row does, not the
    80 s its fixed-point term is clamped to."""
    rows, R = LC.rows_case(257, kind)
    w = (LC.weights_case() * 40.0).astype(np.float32).astype(np.float64)
    v, vt, _ = SC.virtual_case(900, dev)
    zs = vt[0][:, :31] @ w[:31]
    assert np.sum(zs < -100) >= 10
    red = L.logreg_pass(rows.to(dev), torch.from_numpy(w), CW, True, LC.FP8_SCALE, virtual=v, nblocks=1, full=True)
    _, loss, wsum, _ = ref.logreg_pass(np.concatenate([R, vt[0]]), w, CW, False)
    assert red[33] == wsum
    # 1e-5 relative (the pass bound) + half a 1 / kSynQL unit per sample and one more per pick (the
    # cut-off part is rounded once per pick: _sgd_cases.pass_bounds)
    assert abs(red[32] - loss) <= 1e-5 * loss + (900 + SC.N_PICKS) * 0.5 / float(native().SGD_SYN_QL), (red[32], loss)


@pytest.mark.parametrize("kind", KINDS)
def test_virtual_sums_do_not_depend_on_the_bucket_order(dev, kind):
    """The order of a pick's lambdas inside its bucket is whatever the fill's atomics made it, and
    it decides which lane of the pick gets which sample.  Every sum must be a function of the
    pick's sample set only: each bucket reversed, and rotated by one, gives the same bits -- at
    ordinary weights and with samples below the logit clamp, in the SGD and the Newton pass."""
    import dataclasses

    rows, _ = LC.rows_case(257, kind)
    rows = rows.to(dev)
    v = SC.virtual_case(900, dev)[0].prepare()
    lam, off, cnt = (t.cpu().numpy() for t in (v.lam, v.off, v.cnt))
    assert cnt.max() >= 9  # more samples than lanes in some pick
    variants = []
    for change in (lambda s: s[::-1], lambda s: np.roll(s, 1)):
        l2 = lam.copy()
        for o, c in zip(off, cnt):
            l2[o:o + c] = change(lam[o:o + c])
        assert not np.array_equal(l2, lam)
        variants.append(dataclasses.replace(v, lam=torch.from_numpy(l2).to(dev)))
    ws = L.LRWorkspace(dev, 1)
    # 14 to 20: a few samples just below the clamp, where a pick's loss is small enough for one
    # fixed-point unit of its sum to survive the pick's fp32 conversion
    # Positive weight 1/4 on three blocks: a pick's loss then fits fp32 to the last fixed-point unit
    # and most waves hold one pick tile and no stored row, so a unit is not rounded away downstream.
    for scale, cw, blocks in itertools.product((1.0, 14.0, 16.0, 20.0, 40.0), (CW, (1.0, 0.25)), (1, 3)):
        w = (LC.weights_case() * scale).astype(np.float32).astype(np.float64)
        q = L.sgd_pass_sums_once(rows, w, 1, 0, blocks, cw, None, v, None, 0, LC.FP8_SCALE, ws).copy()
        red = L.logreg_pass(rows, torch.from_numpy(w), cw, True, LC.FP8_SCALE, virtual=v, nblocks=blocks, full=True)
        for v2 in variants:
            q2 = L.sgd_pass_sums_once(rows, w, 1, 0, blocks, cw, None, v2, None, 0, LC.FP8_SCALE, ws)
            assert np.array_equal(q, q2), np.flatnonzero(q != q2)
            red2 = L.logreg_pass(rows, torch.from_numpy(w), cw, True, LC.FP8_SCALE, virtual=v2, nblocks=blocks,
                                 full=True)
            assert np.array_equal(_bits(red), _bits(red2)), np.flatnonzero(red != red2)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n_new", [0, 900])
def test_pass_sums_housekeeping(dev, n_new, kind):
    ws = L.LRWorkspace(dev, 1)
    aff = _affine(True)
    q1, _, _ = _check_pass(dev, ws, 5000, kind, n_new, aff, 3, 2, 1)
    q2, _, _ = _check_pass(dev, ws, 5000, kind, n_new, aff, 3, 2, 1)
    assert np.array_equal(q1, q2) and q1[34] == 0
    # done = 1: sums, accumulators and ticket untouched
    v = SC.virtual_case(n_new, dev)[0] if n_new else None
    ws.sgd_sums.fill_(-77)
    ws.sgd_acc.fill_(5)
    got = L.sgd_pass_sums_once(_dev_rows(5000, kind, dev), LC.weights_case(), 2, 1, 3, CW, aff, v, None, 1,
                               LC.FP8_SCALE, ws)
    assert np.all(got == -77) and np.all(ws.sgd_acc.cpu().numpy() == 5)
    assert int(ws.done.cpu()[0]) == 1


# ---- B. sgd_step_kernel's reduction ----------------------------------------------------------
def _step_blocks():
    m = native()
    G, Lo = int(m.SGD_GROUPS), int(m.SGD_LOADS)
    return [1, G - 1, G, G + 1, G * Lo - 1, G * Lo, G * Lo + 1, 1024]


@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("epoch_end", [0, 1])
@pytest.mark.parametrize("case", range(8))
def test_step_kernel_reduces_exactly(dev, case, epoch_end, affine):
    """Integer partials (|v| <= 2^10: every fp64 summation order is exact).  The columns behind the
    36 slots are NaN: they do not matter.  Column 34 is NaN too: whether or not the kernel loads it,
    a NaN in slot 34 does not reach the state (sgd_apply never consumes that slot, so a read of the
    column itself cannot be observed here).  The state and weights are bitwise those of
    sgd_update_kernel fed the column sums (the 1008-thread block runs the same sgd_apply as the
    64-thread one)."""
    nblocks = _step_blocks()[case]
    rng = np.random.default_rng(100 + nblocks)
    part = np.full((nblocks, L.PART_STRIDE), np.nan, dtype=np.float32)
    part[:, :32] = rng.integers(-1024, 1025, (nblocks, 32))
    part[:, 32] = rng.integers(0, 1025, nblocks)
    part[:, 33] = rng.integers(1, 1025, nblocks)
    part[:, 35] = rng.integers(1, 257, nblocks)
    sums = np.zeros(36)
    sums[np.r_[0:34, 35]] = part[:, np.r_[0:34, 35]].astype(np.float64).sum(0)
    st0 = SC.state_vector(SC.mid_fit_state(), fill=SC.SENTINEL)
    w32_0 = np.full(32, 7.5, dtype=np.float32)
    kw = dict(d=30, avg=1, epoch_end=epoch_end, affine=_affine(affine), w32=w32_0, device=dev, **ARGS)
    a = L.sgd_step_once(part, nblocks, st0, **kw)
    b = L.sgd_update_once("red", sums, st0, **kw)
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1])) and a[2] == b[2]
    assert a[0][L.S_ITER] == st0[L.S_ITER] + 1 and a[0][L.S_EPW] == (0.0 if epoch_end else st0[L.S_EPW] + sums[33])
    done = L.sgd_step_once(part, nblocks, st0, done=1, **kw)
    assert np.array_equal(_bits(done[0]), _bits(st0)) and np.array_equal(_bits(done[1]), _bits(w32_0)) and done[2] == 1


# ---- C. the update kernels against SgdStateRef -----------------------------------------------
def _check_update(dev, kind, st, sums, d=30, fi=True, avg=0, epoch_end=0, affine=None, tol=-1.0, C=0.7, c=0.5,
                  momentum=0.55, nb=3):
    """One kernel launch and one mirror step from the same sums and state; returns the mirror, with
    the largest |dev - ref| / (2^-46 mag) of this launch in its ``ratio`` (for the record).
    ``kind`` "red": sgd_update_kernel on the fp64 sums (mapped by the kernel under an affine);
    "fixed": sgd_update_fixed_kernel on rint(sums 2^20) (mapped already)."""
    before = SC.state_vector(st, fill=SC.SENTINEL)
    w32_0 = np.full(32, 7.5, dtype=np.float32)
    if kind == "fixed":
        q = np.rint(np.asarray(sums) * SC.FIX).astype(np.int64)
        fed, sums = q, q.astype(np.float64) / SC.FIX
    else:
        fed = sums
    got, w32, done = L.sgd_update_once(kind, fed, before, d, C, c, momentum, fi, nb, avg, epoch_end, tol, affine, 0,
                                       w32_0, dev)
    st.step(sums[:32], sums[32], sums[33], sums[35], d, C, c, momentum, nb, avg, epoch_end, tol, fi, affine=affine,
            mapped=kind == "fixed")
    exp, mag = SC.state_vector(st, fill=SC.SENTINEL), SC.mag_vector(st)
    for slot in SC.EXACT:
        assert got[slot] == exp[slot], (slot, got[slot], exp[slot])
    assert done == int(st.done)
    err = np.abs(got[SC.OWNED] - exp[SC.OWNED])
    bound = 2.0 ** -46 * mag[SC.OWNED]
    assert np.all(err <= bound), (SC.OWNED[np.argmax(err - bound)], float(np.max(err - bound)))
    nz = bound > 0
    st.ratio = float(np.max(err[nz] / bound[nz])) if np.any(nz) else 0.0
    rest = np.setdiff1d(np.arange(L.STATE_SIZE), SC.OWNED)
    assert np.array_equal(_bits(got[rest]), _bits(before[rest])), "a slot the step does not own changed"
    gw = got[L.S_W:L.S_W + 32]
    if affine is None:
        e32 = gw.astype(np.float32)
        e32[31] = 0.0
        assert np.array_equal(_bits(w32), _bits(e32))
    else:
        f = ref.fold_weights(gw, affine).astype(np.float32)
        ulp = np.spacing(np.abs(f))
        assert np.all(np.abs(w32 - f) <= ulp), np.max(np.abs(w32 - f) / ulp)
        assert w32[31] == 0.0
    return st


@pytest.mark.parametrize("kind", ["red", "fixed"])
@pytest.mark.parametrize("d,fi", [(d, fi) for d in (30, 20, 12) for fi in (0, 1)])
@pytest.mark.parametrize("affine", [False, True])
def test_update_follows_the_mirror(dev, affine, d, fi, kind):
    sums = SC.synth_sums()
    ratios = []
    for avg, epoch_end in itertools.product((0, 1), (0, 1)):
        st = _check_update(dev, kind, SC.mid_fit_state(d, bool(fi)), sums, d, bool(fi), avg, epoch_end,
                           _affine(affine, d))
        assert st.iter == 6 and st.n_avg == (0 if epoch_end else 2 + avg) and not st.done
        ratios.append(st.ratio)
    print("max |dev - ref| / (2^-46 mag):", max(ratios))


@pytest.mark.parametrize("kind", ["red", "fixed"])
@pytest.mark.parametrize("affine", [False, True])
def test_update_branches(dev, affine, kind):
    aff = _affine(affine)
    mk = SC.mid_fit_state
    st = _check_update(dev, kind, mk(), SC.synth_sums(S=0.0), affine=aff)            # S = 0 counts as 1
    assert st.ep_w == 128.0 and st.dbar == 1e-3
    st = _check_update(dev, kind, mk(), SC.synth_sums(dsum=2.0 ** -12), affine=aff)  # the dbar floor
    assert st.dbar == 1e-3 and st.lr == 500.0
    st = _check_update(dev, kind, mk(n_avg=0), SC.synth_sums(), epoch_end=1, affine=aff)  # no average taken
    assert st.n_avg == 0 and np.isfinite(st.obj)
    st = _check_update(dev, kind, mk(), SC.synth_sums(), avg=1, epoch_end=1, affine=aff, tol=1e9)  # tol reached
    assert st.done and st.converged
    zero = ref.SgdStateRef(np.zeros(32))  # epoch gradient exactly 0 and still no convergence under tol = -1
    flat = SC.synth_sums()
    flat[:32] = 0.0
    st = _check_update(dev, kind, zero, flat, epoch_end=1, affine=aff, tol=-1.0)
    assert st.gmax == 0.0 and not st.done


@pytest.mark.parametrize("kind", ["red", "fixed"])
@pytest.mark.parametrize("affine", [False, True])
def test_update_done_is_a_no_op(dev, affine, kind):
    before = SC.state_vector(SC.mid_fit_state(), fill=SC.SENTINEL)
    w32_0 = np.arange(32, dtype=np.float32) + 0.5
    sums = SC.synth_sums() if kind == "red" else np.rint(SC.synth_sums() * SC.FIX).astype(np.int64)
    got, w32, done = L.sgd_update_once(kind, sums, before, avg=1, epoch_end=1, affine=_affine(affine), done=1,
                                       w32=w32_0, device=dev, **ARGS)
    assert done == 1 and np.array_equal(_bits(got), _bits(before)) and np.array_equal(_bits(w32), _bits(w32_0))


@pytest.mark.parametrize("epoch_end", [0, 1])
def test_update_fixed_is_update_on_scaled_sums(dev, epoch_end):
    """Without an affine map the two kernels differ only in how the sums arrive: bitwise the same."""
    q = np.rint(SC.synth_sums() * SC.FIX).astype(np.int64)
    before = SC.state_vector(SC.mid_fit_state(), fill=SC.SENTINEL)
    kw = dict(avg=1, epoch_end=epoch_end, device=dev, **ARGS)
    a = L.sgd_update_once("fixed", q, before, **kw)
    b = L.sgd_update_once("red", q.astype(np.float64) / SC.FIX, before, **kw)
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1])) and a[2] == b[2]


@pytest.mark.parametrize("kind", KINDS)
def test_update_on_device_pass_sums(dev, kind):
    """Sums of part A (1000 rows + 900 samples) through both update kernels: the mapped sums through
    sgd_update_fixed, the raw ones (2^-20 units -> fp64) through sgd_update with the affine."""
    ws = L.LRWorkspace(dev, 1)
    aff = _affine(True)
    mapped, _, _ = _check_pass(dev, ws, 1000, kind, 900, aff, 3, 2, 1)
    raw, _, _ = _check_pass(dev, ws, 1000, kind, 900, None, 3, 2, 1)
    ratios = []
    for avg, epoch_end in ((0, 0), (1, 1)):
        for kind_u, sums in (("fixed", mapped), ("red", raw)):
            st = _check_update(dev, kind_u, SC.mid_fit_state(), sums / SC.FIX, avg=avg, epoch_end=epoch_end, affine=aff,
                               nb=2)
            ratios.append(st.ratio)
    print("max |dev - ref| / (2^-46 mag):", max(ratios))


# ---- D. the fused step is its parts ----------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n_new", [0, 900])
@pytest.mark.parametrize("affine", [False, True])
def test_fused_step_is_pass_sums_then_update_fixed(dev, affine, n_new, kind):
    """Six steps over two epochs of three minibatches, one fused launch each: the state after a step
    is bitwise sgd_update_fixed applied to the state before it, fed sgd_pass_sums at the weights the
    step read -- no tolerance accumulates."""
    n, blocks, nbs, lrs, C, mom, tol = 5000, 3, [3, 3], [0.2, 0.3], 0.7, 0.55, 1e-3
    rows = _dev_rows(n, kind, dev)
    v = SC.virtual_case(n_new, dev)[0] if n_new else None
    aff = _affine(affine)
    aff_dev = torch.from_numpy(aff).to(dev) if affine else None
    ws, ws_pass = L.LRWorkspace(dev), L.LRWorkspace(dev, 1)
    ws.reset(LC.weights_case(seed=9, scale=0.1), CW, ptr(aff_dev) if affine else 0)
    for i in range(6):
        st0, w32_0, done0 = ws.state.cpu().numpy().copy(), ws.w32.cpu().numpy().copy(), int(ws.done.cpu()[0])
        assert done0 == 0
        L.sgd_run_steps(rows, ws, i, i + 1, blocks, nbs, lrs, C=C, momentum=mom, tol=tol, avg_from=1, affine=aff_dev,
                        virtual=v, fp8_scale=LC.FP8_SCALE)
        ep, pos = divmod(i, 3)
        q = L.sgd_pass_sums_once(rows, w32_0, 3, pos, blocks, CW, aff, v, None, 0, LC.FP8_SCALE, ws_pass)
        est, ew32, edone = L.sgd_update_once("fixed", q, st0, 30, C, lrs[ep], mom, True, 3, int(ep >= 1), int(pos == 2),
                                             tol, aff, 0, w32_0, dev)
        got = ws.state.cpu().numpy()
        assert np.array_equal(_bits(got), _bits(est)), (i, np.flatnonzero(_bits(got) != _bits(est)))
        assert np.array_equal(_bits(ws.w32.cpu().numpy()), _bits(ew32)) and int(ws.done.cpu()[0]) == edone
        assert got[L.S_ITER] == i + 1
        assert not np.any(ws.sgd_acc.cpu().numpy())
    assert got[L.S_NAVG] == 0 and np.isfinite(got[L.S_OBJ]) and got[L.S_GMAX] > 0


# ---- E. the persistent launch on small grids -------------------------------------------------
FIT_LR = 0.2  # step scalar of the small fits: the library default is tuned for millions of rows and
              # diverges on a few hundred (the fp64 mirror then amplifies a 1e-7 change of w0 to 5e-3)


def _fit_rows(n, kind, dev):
    return _dev_rows(n, kind, dev), dict(fp8_scale=LC.FP8_SCALE, class_w=CW, lr=FIT_LR)


def _same_fit(a, b):
    assert np.array_equal(_bits(a.w), _bits(b.w)), np.abs(a.w - b.w).max()
    assert a.n_iter == b.n_iter and a.objective == b.objective and a.grad_max == b.grad_max
    assert a.converged == b.converged and not a.recovered and not b.recovered


def _both(rows, **kw):
    a = L.sgd_fit(rows, persistent=True, **kw).as_fit_info()
    b = L.sgd_fit(rows, persistent=False, **kw).as_fit_info()
    _same_fit(a, b)
    return a


# n_stored, batches, pass blocks, persistent blocks, schedule
SHAPES = {
    "700: 4 of 8 waves idle": (700, 3, 1, 1, dict(epochs=3, subsample=None, avg_from=1)),
    "6161: 12 of 16 waves": (6161, 2, 3, 2, dict(epochs=4, subsample=None, avg_from=1)),
    "37: phase 1 holds picks only": (37, 2, 1, 1, dict(epochs=4, subsample=None, avg_from=1)),
    "2053: sub-sampled epoch": (2053, 2, 1, 1, dict(epochs=3, epoch_batches=(2, 2, 2), subsample=(2, 1, 1),
                                                    avg_from=1)),
}


# every shape with and without virtual samples; the 37-row one is about the picks: virtual only
SHAPE_CASES = [(s, nn) for s in SHAPES for nn in (0, 900) if nn or SHAPES[s][0] != 37]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape,n_new", SHAPE_CASES)
def test_persistent_small_grids_are_the_per_step_launches(dev, shape, n_new, kind):
    n, batches, pass_blocks, persist_blocks, sched = SHAPES[shape]
    m = native()
    ws = L.LRWorkspace(dev)
    blocks = ref.sgd_grid_blocks(n, batches, ws.sgd_blocks)
    assert blocks == pass_blocks and m.sgd_persist_blocks(blocks) == persist_blocks > 0
    waves = persist_blocks * int(m.SGD_PERSIST_WAVES)
    assert 4 * blocks <= waves and (n != 700 or waves - 4 * blocks == 4) and (n != 6161 or (4 * blocks, waves) == (12, 16))
    if "epoch_batches" in sched:  # the sub-sampled epoch survives on this shard
        subs = L._effective_subs(sched["subsample"], n, SC.N_PICKS if n_new else 0, sched["epoch_batches"], blocks)
        assert subs == [2, 1, 1]
    rows, kw = _fit_rows(n, kind, dev)
    v = SC.virtual_case(n_new, dev)[0] if n_new else None
    fit = _both(rows, virtual=v, batches=batches, tol=-1.0, **sched, **kw)
    assert fit.n_iter == batches * sched["epochs"] and np.all(np.isfinite(fit.w)) and np.any(fit.w[:30] != 0)


@pytest.mark.parametrize("kind", KINDS)
def test_persistent_small_grid_with_hole_and_affine(dev, kind):
    n, (at, ln) = 6161, (100, 91)
    rows, kw = _fit_rows(n + ln, kind, dev)
    aff = torch.from_numpy(_affine(True)).to(dev)
    v = SC.virtual_case(900, dev)[0]
    fit = _both(rows, virtual=v, batches=2, epochs=4, subsample=None, avg_from=1, tol=-1.0, affine=aff, hole=(at, ln),
                **kw)
    assert fit.n_iter == 8


def test_persistent_accumulator_sets_rotate_twice(dev):
    """Nine steps on the one-block grid: each of the three accumulator sets is used three times."""
    rows, kw = _fit_rows(700, "bf16", dev)
    fit = _both(rows, virtual=SC.virtual_case(900, dev)[0], batches=3, epochs=3, subsample=None, avg_from=0, tol=-1.0,
                **kw)
    assert fit.n_iter == 9 >= 7


@pytest.mark.parametrize("kind", KINDS)
def test_persistent_leaves_through_convergence(dev, kind):
    """tol = 1: the fit converges at the first epoch end and the persistent loop leaves through its
    done flag; both paths stop counting there."""
    rows, kw = _fit_rows(700, kind, dev)
    fit = _both(rows, virtual=SC.virtual_case(900, dev)[0], batches=3, epochs=3, subsample=None, tol=1.0, **kw)
    assert fit.converged and fit.n_iter == 3 and fit.grad_max <= 1.0


def test_persistent_split_launches_and_checkpoint_resume(dev, tmp_path):
    from fraud_detection_amd.utils.checkpoint import CheckpointManager

    rows, kw = _fit_rows(3000, "bf16", dev)
    kw.update(virtual=SC.virtual_case(900, dev)[0], batches=2, epochs=4, subsample=None, avg_from=1, tol=-1.0)
    full = _both(rows, **kw)
    assert full.n_iter == 8
    part = _both(rows, max_steps=5, **kw)  # the schedule cut after five steps
    assert part.n_iter == 5 and not np.array_equal(part.w, full.w)
    mgr = CheckpointManager(str(tmp_path / "c"), keep=3)
    L.sgd_fit(rows, persistent=True, checkpoint=mgr, checkpoint_every=2, max_steps=5, **kw)  # one launch per step
    res = L.sgd_fit(rows, persistent=True, checkpoint=mgr, checkpoint_every=2, **kw).as_fit_info()
    _same_fit(res, full)


def test_persistent_serpentine_follows_the_cpu_mirror(dev):
    """Odd epochs visit the minibatches in reverse (persistent launch only): compared with the fp64
    CPU mirror of the same order.  No derived bound: the serpentine fit is allowed 4x the distance
    of the plain-order fit of the same case from the same mirror -- the same arithmetic in another
    visiting order."""
    rows_h = LC.rows_case(700, "bf16")[0]
    kw = dict(batches=3, epochs=3, subsample=None, avg_from=1, tol=-1.0, class_w=CW, lr=FIT_LR)
    dist = {}
    for serp in (False, True):
        g = L.sgd_fit(rows_h.to(dev), virtual=SC.virtual_case(900, dev)[0], persistent=True, serpentine=serp,
                      **kw).as_fit_info()
        c = L.sgd_fit(rows_h, virtual=SC.virtual_case(900)[0], serpentine=serp, **kw)
        assert g.n_iter == c.n_iter == 9
        dist[serp] = float(np.max(np.abs(g.w[:31] - c.w[:31])))
    print("max|w_dev - w_cpu|: plain", dist[False], "serpentine", dist[True])
    assert dist[False] > 0
    # measured on an MI355X: plain 2.74e-8, serpentine 2.92e-8 (fp32 pass sums against fp64 ones)
    assert dist[True] <= 4 * dist[False], dist
