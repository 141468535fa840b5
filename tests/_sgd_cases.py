"""Shared cases and bounds of the SGD oracle tests (test_sgd_oracle.py, test_sgd_kernels_gpu.py):
the state-vector <-> SgdStateRef mapping, mid-fit states, synthesized sums, the virtual-SMOTE case,
and the derived bounds of one device pass.  Rows, weights and the affine map come from
_logreg_cases (rows_case, weights_case, affine_case)."""
import functools

import numpy as np
import torch

from fraud_detection_amd.ops import logreg as L
from fraud_detection_amd.ops import reference as ref

CW = (1.0, 3.0)
FIX = 2.0 ** 20          # logreg.hip kFixScale: the fixed point of the fused passes' sums
SENTINEL = -12345.678    # slots a step does not own hold it and must keep it
# virtual-SMOTE case (tests/test_sgd_gpu._case at its smallest): 40 parents, 30 query rows, k = 5
V_PARENTS, V_MQ, V_K, V_SEED = 40, 30, 5, 17
N_PICKS = V_MQ * V_K


# ---- state vector ----------------------------------------------------------------------------
OWNED = np.r_[L.S_W:L.S_W + 32, L.S_VEL:L.S_VEL + 32, L.S_AVG:L.S_AVG + 32, L.S_EPG:L.S_EPG + 32, L.S_EPLOSS,
              L.S_EPW, L.S_NAVG, L.S_DBAR, L.S_LR, L.S_ITER, L.S_GMAX, L.S_OBJ, L.S_CONV]
EXACT = (L.S_ITER, L.S_NAVG, L.S_CONV)  # integer-valued slots


def state_vector(st: ref.SgdStateRef, fill: float = 0.0) -> np.ndarray:
    """The device state [256] of a mirror state (ops/logreg.py S_* offsets); the slots sgd_apply
    does not own (w_prev, step, the Newton scalars, the tail) hold ``fill``."""
    s = np.full(L.STATE_SIZE, float(fill))
    s[L.S_W:L.S_W + 32], s[L.S_VEL:L.S_VEL + 32] = st.w, st.v
    s[L.S_AVG:L.S_AVG + 32], s[L.S_EPG:L.S_EPG + 32] = st.avg, st.ep_g
    s[L.S_EPLOSS], s[L.S_EPW], s[L.S_NAVG], s[L.S_ITER] = st.ep_loss, st.ep_w, st.n_avg, st.iter
    s[L.S_DBAR], s[L.S_LR] = st.dbar, st.lr
    s[L.S_GMAX], s[L.S_OBJ], s[L.S_CONV] = st.gmax, st.obj, float(st.converged)
    return s


def from_state_vector(s: np.ndarray) -> ref.SgdStateRef:
    s = np.asarray(s, dtype=np.float64)
    st = ref.SgdStateRef(s[L.S_W:L.S_W + 32])
    st.v, st.avg, st.ep_g = (s[o:o + 32].copy() for o in (L.S_VEL, L.S_AVG, L.S_EPG))
    st.ep_loss, st.ep_w, st.n_avg, st.iter = float(s[L.S_EPLOSS]), float(s[L.S_EPW]), int(s[L.S_NAVG]), int(s[L.S_ITER])
    st.dbar, st.lr = float(s[L.S_DBAR]), float(s[L.S_LR])
    st.gmax, st.obj, st.converged = float(s[L.S_GMAX]), float(s[L.S_OBJ]), bool(s[L.S_CONV] > 0)
    st.done = st.converged
    return st


def mag_vector(st: ref.SgdStateRef) -> np.ndarray:
    """SgdStateRef.mag of the last step laid out as the state vector (0 where the mirror defines no
    magnitude: those slots are compared exactly)."""
    m = np.zeros(L.STATE_SIZE)
    g = st.mag
    m[L.S_W:L.S_W + 32], m[L.S_VEL:L.S_VEL + 32] = g["w"], g["v"]
    m[L.S_AVG:L.S_AVG + 32], m[L.S_EPG:L.S_EPG + 32] = g["avg"], g["ep_g"]
    m[L.S_EPLOSS], m[L.S_EPW], m[L.S_DBAR], m[L.S_LR] = g["ep_loss"], g["ep_w"], g["dbar"], g["lr"]
    m[L.S_GMAX], m[L.S_OBJ] = g.get("gmax", 0.0), g.get("obj", 0.0)
    return m


def mid_fit_state(d: int = 30, fit_intercept: bool = True, n_avg: int = 2, seed: int = 60) -> ref.SgdStateRef:
    """A state in the middle of an epoch: non-zero velocity, Polyak sum over ``n_avg`` steps, epoch
    sums of two minibatches of weight 64, iter 5; inactive coordinates hold values that must follow
    the kernel's rule for them (velocity decays, no gradient)."""
    rng = np.random.default_rng(seed + d)
    w = rng.normal(0, 0.2, 32)
    w[d:30] = 0.125
    w[30] = 0.3 if fit_intercept else -0.625
    w[31] = 0.0
    st = ref.SgdStateRef(w)
    st.v = rng.normal(0, 0.02, 32)
    st.v[31] = 0.0
    st.avg = n_avg * w + rng.normal(0, 0.05, 32) if n_avg else np.zeros(32)
    st.n_avg = n_avg
    st.ep_g = rng.normal(0, 8.0, 32)
    st.ep_g[31] = 0.0
    st.ep_loss, st.ep_w, st.iter = 0.55 * 128.0, 128.0, 5
    st.gmax, st.obj = 0.5, 0.75  # an earlier epoch's: kept until the next epoch end
    st.dbar, st.lr = 0.2, 2.5
    return st


def synth_sums(seed: int = 21, S: float = 64.0, dsum: float | None = None) -> np.ndarray:
    """[36] fp64 sums of a minibatch of weight ``S`` made on the host, exact in 2^-20 fixed point:
    gradient ~ N(0, S / 4), loss 0.6 S, curvature ``dsum`` (default 0.15 S)."""
    rng = np.random.default_rng(seed)
    s = np.zeros(36)
    s[:31] = rng.normal(0, 0.25 * max(S, 1.0), 31)
    s[32], s[33], s[35] = 0.6 * S, S, 0.15 * S if dsum is None else dsum
    return np.rint(s * FIX) / FIX


# ---- virtual samples -------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _virtual_host(n_new: int):
    g = torch.Generator().manual_seed(V_SEED)
    par = torch.randn(V_PARENTS, 32, generator=g) + 0.7
    par[:, 30] = 1.0
    par[:, 31] = 1.0
    nbr = torch.stack([torch.randperm(V_PARENTS, generator=g)[:V_K] for _ in range(V_MQ)]).to(torch.int32)
    par = par.to(torch.bfloat16)
    v = L.VirtualSmote(par, nbr, n_new, seed=V_SEED, counter_base=1)
    samples = v.rows_f32().double().numpy()
    pick, _ = ref.smote_pick_draws(V_MQ, V_K, n_new, V_SEED, 1, 0)
    pick = pick.astype(np.int64)
    P = par.float().double().numpy()
    pair = np.abs(P[pick // V_K]) + np.abs(P[nbr.numpy().astype(np.int64).reshape(-1)[pick]])  # |xa| + |xb| per sample
    pair[:, 31] = 0.0
    for a in (samples, pick, pair):
        a.setflags(write=False)
    return par, nbr, samples, pick, pair


@functools.lru_cache(maxsize=None)
def _virtual_dev(n_new: int, dev: str):
    par, nbr, *_ = _virtual_host(n_new)
    return L.VirtualSmote(par.to(dev), nbr.to(dev), n_new, seed=V_SEED, counter_base=1)


def virtual_case(n_new: int, dev=None):
    """(VirtualSmote on ``dev`` (None: on the host), oracle tuple (samples fp64, picks, n_picks),
    |xa| + |xb| of every sample's two parent rows [n_new, 32])."""
    par, nbr, samples, pick, pair = _virtual_host(n_new)
    v = (_virtual_dev(n_new, str(dev)) if dev is not None
         else L.VirtualSmote(par, nbr, n_new, seed=V_SEED, counter_base=1))
    return v, (samples, pick, N_PICKS), pair


# ---- the bounds of one device pass -----------------------------------------------------------
def active_waves(n_stored: int, gw: int, rsub: int, phase: int, n_picks: int = 0) -> int:
    """W: waves of a grid of ``gw`` that visit at least one stored tile or pick tile of the phase.
    Wave w's first stored tile is w rsub + phase (rows from 64 times that), its first pick tile the
    same index among the ceil(n_picks / PICK_TILE) pick tiles."""
    first = np.arange(gw, dtype=np.int64) * rsub + phase
    ptiles = -(-int(n_picks) // ref.PICK_TILE)
    return int(np.sum((first * ref.ROW_TILE < n_stored) | (first < ptiles)))


def pass_bounds(sums_abs: np.ndarray, W: int, affine=None, n_samples: int = 0, pair_max=None, syn_q: float = 0.0,
                syn_ql: float = 0.0, n_picks: int = 0) -> np.ndarray:
    """[36] allowed |device sums 2^-20 - ref.sgd_pass_sums| of one FUSE pass; none tuned to the kernel.

    The pass accumulates in fp32 and is held to the Newton pass's bound (_logreg_cases
    assert_pass_matches): gradient slot t within 1e-5 of its absolute-term sum (``sums_abs``, from
    ref.sgd_sums_abs) + 1e-7; loss and curvature 1e-5 relative (their terms are not negative); the
    weight exact (dyadic class weights, sums < 2^24).  Every virtual sample's terms are rounded to
    integers one by one (logreg.hip pick_compute): r and r lam in units of 1 / kSynQ, so gradient
    slot t moves by up to 0.5 / kSynQ (|xa_t| + |xb_t|) per sample (``pair_max``: that sum's
    maximum over the phase's samples); the loss term in units of 1 / kSynQL and the curvature term
    in units of 1 / kSynQ, half a unit per sample each.  A pick with samples below the logit clamp
    adds the part of their loss the clamp cut off as one more term, rounded once per pick: half a
    1 / kSynQL unit for each of the phase's ``n_picks`` picks.  With ``affine`` the device maps each wave's
    gradient, rz_t = inv_t (g_t - c_t g_bias): the bound b maps to |inv_t| (b_t + |c_t| b_bias).
    Last, every wave's mapped sum is rounded to 2^-20 fixed point on its own: half a unit, 2^-21,
    for each of the W waves with anything to add (every slot but the exact weight)."""
    b = np.zeros(36)
    b[:32] = 1e-5 * sums_abs[:32] + 1e-7
    b[32], b[35] = 1e-5 * sums_abs[32], 1e-5 * sums_abs[35]
    if n_samples:
        b[:32] += n_samples * 0.5 / syn_q * np.asarray(pair_max)
        b[32] += (n_samples + n_picks) * 0.5 / syn_ql
        b[35] += n_samples * 0.5 / syn_q
    if affine is not None:
        a = np.asarray(affine, dtype=np.float64)
        b[:32] = np.abs(a[32:]) * (b[:32] + np.abs(a[:32]) * b[ref.BIAS_COL])
    fx = W * 2.0 ** -21
    b[:33] += fx
    b[35] += fx
    b[31] = 0.0  # the label column carries no gradient
    return b
