"""Shared case builders of the logistic-regression oracle tests (test_logreg_oracle.py,
test_logreg_kernels_gpu.py): seeded rows in both storage formats, synthesized reduced vectors for
the Newton update, and the state-vector <-> NewtonStateRef mapping."""
import functools

import numpy as np
import torch

from fraud_detection_amd.ops import logreg as L
from fraud_detection_amd.ops import reference as ref

FP8_SCALE = 4.0
RED_SEED, AFFINE_SEED = 21, 5  # synth_red / affine_case seeds of the device update tests
FP8_MASTER_ROWS = 20_000   # fp8 cases are prefixes of one encoded table (the encoder is a Python loop)
BF16_MASTER_ROWS = 400_000


def _master_f32(n: int, seed: int) -> torch.Tensor:
    """features ~ N(0, 1.5), column 30 = 1, labels (column 31) at rate 0.3."""
    g = torch.Generator().manual_seed(seed)
    r = torch.randn(n, 32, generator=g) * 1.5
    r[:, 30] = 1.0
    r[:, 31] = (torch.rand(n, generator=g) < 0.3).float()
    return r


@functools.lru_cache(maxsize=None)
def _master(kind: str):
    """(stored rows, decoded fp64 rows) of the whole table of one storage format; never modified."""
    if kind == "bf16":
        rows = _master_f32(BF16_MASTER_ROWS, 101).to(torch.bfloat16)
    else:
        r = _master_f32(FP8_MASTER_ROWS, 102).to(torch.bfloat16).float().numpy().copy()
        r[:, :30] *= FP8_SCALE
        rows = torch.from_numpy(ref.fp8_encode(r))
    R = ref.rows_to_f32(rows, FP8_SCALE).double().numpy()
    R.setflags(write=False)
    return rows, R


def rows_case(n: int, kind: str):
    """(stored rows [n, 32] on the host, their exact fp64 values): the first n rows of the table."""
    rows, R = _master(kind)
    if n > rows.shape[0]:
        raise ValueError(f"{kind} table holds {rows.shape[0]} rows")
    return rows[:n], R[:n]


def weights_case(seed: int = 4, scale: float = 0.3) -> np.ndarray:
    """[32] fp64 weights that are exact in fp32 (the device pass reads fp32 weights): N(0, scale)
    features, intercept -1, label slot 0."""
    w = np.r_[np.random.default_rng(seed).normal(0, scale, 30), -1.0, 0.0]
    return w.astype(np.float32).astype(np.float64)


def assert_pass_matches(red, R, w, class_w, exp, hessian=True):
    """The tolerances of one device pass against its fp64 oracle vector ``exp``.

    red[33], red[34]: exact (dyadic class weights, sums < 2^24).  Loss: relative 1e-5 (a sum of
    positive terms).  Gradient: 1e-5 of its own absolute-term sum + 1e-7.  H: 5e-3 relative in the
    Frobenius norm (bf16 MFMA operands), symmetric to 1e-6 max|H|; exactly zero from a gradient pass."""
    assert red[33] == exp[33] and red[34] == exp[34], (red[33:35], exp[33:35])
    if exp[32] > 0:
        assert abs(red[32] - exp[32]) / exp[32] < 1e-5, (red[32], exp[32])
    else:
        assert red[32] == 0.0
    gabs = ref.logreg_grad_abs(R, w, class_w)
    err = np.abs(red[:32] - exp[:32])
    bound = 1e-5 * gabs + 1e-7
    assert np.all(err <= bound), ("gradient", float(np.max(err / bound)))
    H, He = red[64:].reshape(32, 32), exp[64:].reshape(32, 32)
    if not hessian or not np.any(He):
        assert not np.any(H)
        return
    rel = np.linalg.norm(H - He) / np.linalg.norm(He)
    assert rel < 5e-3, ("hessian", rel)
    assert np.all(np.abs(H - H.T) <= 1e-6 * np.abs(H).max())


# ---- Newton update ---------------------------------------------------------------------------
def state_vector(st: ref.NewtonStateRef) -> np.ndarray:
    """The device state [256] of a mirror state (ops/logreg.py S_* offsets)."""
    s = np.zeros(L.STATE_SIZE)
    s[L.S_W:L.S_W + 32] = st.w
    s[L.S_WPREV:L.S_WPREV + 32] = st.w_prev
    s[L.S_STEP:L.S_STEP + 32] = st.step
    s[L.S_VEL:L.S_VEL + 32] = st.vel
    s[L.S_OBJPREV], s[L.S_ITER], s[L.S_BACKTRACKS] = st.obj_prev, st.iter, st.backtracks
    s[L.S_GMAX], s[L.S_OBJ], s[L.S_NACC], s[L.S_CONV] = st.gmax, st.obj, st.n_accepted, float(st.converged)
    return s


def make_state(w, step=None, it=0, obj_prev=np.inf, backtracks=0, n_accepted=0) -> ref.NewtonStateRef:
    """A consistent mid-fit mirror state: w = w_prev + step."""
    st = ref.NewtonStateRef(np.zeros(32))
    st.step = np.zeros(32) if step is None else np.asarray(step, dtype=np.float64).copy()
    st.w_prev = np.asarray(w, dtype=np.float64) - st.step
    st.w = st.w_prev + st.step
    st.iter, st.obj_prev, st.backtracks, st.n_accepted = it, obj_prev, backtracks, n_accepted
    st.gmax, st.obj = 0.5, 0.75  # leftovers of an earlier iteration: overwritten or kept, never inf
    return st


def synth_red(seed: int, S: float = 64.0, SH: float | None = None) -> np.ndarray:
    """A reduced vector made on the host: H = A^T A + I from a seeded A [128, 32] (symmetric, positive
    definite, condition ~1e1), a gradient of the same scale, loss = 0.6 S, weight S, and slot 34 =
    ``SH`` (default S: H taken over the same rows as g)."""
    rng = np.random.default_rng(seed)
    A = rng.normal(0, 1, (128, 32))
    H = A.T @ A + np.eye(32)
    H = 0.5 * (H + H.T)
    red = np.zeros(L.PART_STRIDE)
    red[:32] = rng.normal(0, 0.25 * S, 32)
    red[32] = 0.6 * S
    red[33] = S
    red[34] = S if SH is None else SH
    red[64:] = H.reshape(-1)
    return red


def affine_case(seed: int, d: int = 30) -> np.ndarray:
    """[64] c | inv: random pivots c ~ N(0, 0.5) on the d feature columns (0 elsewhere), inv in
    [0.5, 2] there (1 elsewhere).  (Pivots of unit scale push cond of the mapped synth_red matrix
    past 1e3: the map couples every feature with the intercept.)"""
    rng = np.random.default_rng(seed)
    a = np.zeros(64)
    a[32:] = 1.0
    a[:d] = rng.normal(0, 0.5, d)
    a[32:32 + d] = rng.uniform(0.5, 2.0, d)
    return a


def step_bound(red, w, d, C, fit_intercept, affine, ref_step) -> float:
    """|step - mirror step|_inf allowed: 16 m 2^-46 cond(A) |mirror step|_inf.  The device's
    reciprocal square root is refined to ~46 bits; A is the mirror's own matrix."""
    idx, A, _, _, _ = ref.newton_system(red, w, d, C, fit_intercept, affine)
    cond = float(np.linalg.cond(A))
    assert cond <= 1e3, cond
    return 16.0 * len(idx) * 2.0 ** -46 * cond * float(np.max(np.abs(ref_step)))
