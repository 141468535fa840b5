"""Cases, exact oracles, derived error bounds and a numpy emulation (with mutants) of the two
linear KernelSHAP kernels, kernelshap_linear_kernel and kernelshap_paired_kernel
(csrc/kernels/kernelshap.hip).

Plain numpy (torch only for its round-to-nearest-even bf16 cast), no GPU.  The oracle has two
stages, so that a device error can be told from the error the kernel is specified to have:

  exact      brute-force Shapley values over all 2^d subsets (d <= 11; uses neither the design Z
             nor the WLS operator A), kernelshap_reference for sampled designs (d >= 12);
  operands   the same quantities evaluated in fp64 from the kernel's specified operands: the
             hi + lo bf16 halves of u = fl(fl(fl(a32 x) - W) us), the fp32 c_b, fp32 A and A z_M.
             |operands - exact| <= operand_bound,  |device - operands| <= device_bound.

``emulate`` re-runs both kernels in numpy in their own precision and summation order; MUTANTS are
defects planted into that emulation.  test_kernelshap_oracle.py shows on the CPU that the faithful
emulation stays inside device_bound on every run of ``all_runs()`` and that each mutant leaves it on a
named case; test_kernelshap_kernels_gpu.py runs the same list on the device."""
from __future__ import annotations

import dataclasses
import functools
import math

import numpy as np
import torch

from _tree_cases import U, assert_within  # noqa: F401  (assert_within is re-exported)
from fraud_detection_amd.models import explainers as EX
from fraud_detection_amd.ops.kernelshap import complement_pairs

UB = 2.0 ** -8           # unit roundoff of bf16 (8 significant bits)
# Accuracy of v_exp_f32, v_rcp_f32 and v_log_f32 in units of fp32 ulp (2^-23).  Source: the AMD
# Instinct CDNA3 / CDNA4 ISA reference guides, VOP1 opcode table: "V_EXP_F32 ... 1ULP accuracy",
# "V_LOG_F32 ... 1ULP accuracy", "V_RCP_F32 ... 1ULP accuracy".
HW_ULPS = 1.0
HWU = HW_ULPS * 2.0      # the same in units of U = 2^-24
F32 = np.float32
LOG2E32 = F32(1.4426950408889634)
PAIR_SHIFT = 40.0        # kernelshap.hip kPairShift
NULL_ACC = 70.0          # kernelshap.hip kNullAcc
# link_pair / form_y clamp the mean probability of the "logit" link to [1e-12f, 1.0f - 1e-7f]
CLAMP_DEVICE = (float(F32(1e-12)), float(F32(1.0) - F32(1e-7)))
CLAMP_HOST = (1e-12, 1.0 - 1e-12)       # models/explainers._link
LINKS = ("identity", "logit", "logit_model")
MUTANTS = ("no_lo", "pair_drop", "null_counted", "ngl_short", "tau_no_c", "off2_no_s0", "no_az")


def _bf16(v):
    return torch.from_numpy(np.ascontiguousarray(v, F32)).to(torch.bfloat16).to(torch.float32).numpy()


def _logit(p):
    return np.log(p / (1.0 - p))


def _sig2(acc):
    """1 / (1 + 2^acc) in fp64 (the kernel's accumulator is -log2(e) logit)."""
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp2(acc))


# ---------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True, eq=False)
class Case:
    name: str
    a: np.ndarray        # fp64 [32]
    bias: float
    B: np.ndarray        # fp32 [n_bg, d]
    X: np.ndarray        # fp32 [E, d]
    clamp: tuple = CLAMP_DEVICE
    clamped: bool = False  # the logit link's clamp is meant to bind in this case

    @property
    def d(self):
        return self.B.shape[1]

    @property
    def n_bg(self):
        return self.B.shape[0]

    def parts(self):
        return self.a, self.bias, self.B, self.X

    def design(self):
        return EX.cached_design(self.d)

    def explainer(self, link, device="cpu"):
        return EX.KernelExplainer(self.a, self.bias, self.B, link=link, device=device)


def random_case(d: int, n_bg: int, E: int, seed: int, scale: float = 0.5) -> Case:
    """N(0, 1) rows, N(0, scale) weights: moderate logits."""
    rng = np.random.default_rng(seed)
    a = np.zeros(32)
    a[:d] = rng.normal(0, scale, d)
    B = rng.normal(size=(n_bg, d)).astype(F32)
    X = rng.normal(size=(E, d)).astype(F32)
    return Case(f"random d={d} n_bg={n_bg} E={E}", a, float(rng.normal(0, 0.5)), B, X)


def coalition_logits(case: Case) -> np.ndarray:
    """fp64 L_b(z_s) [E, n_bg, S] over the case's design."""
    Z = case.design()[0].astype(np.float64)
    a = case.a[: case.d]
    X, B = case.X.astype(np.float64), case.B.astype(np.float64)
    c = B @ a + case.bias
    return np.einsum("ebk,sk->ebs", a * (X[:, None, :] - B[None, :, :]), Z) + c[None, :, None]


REGIMES = ("moderate", "pair_overflow", "exp_overflow", "tb_low", "high")


def regime_case(regime: str, feature: int = 0, d: int = 8, n_bg: int = 11, E: int = 3) -> Case:
    """Background row 0 holds B[0, feature] = v, weight a[feature] = 1, so L_0(z) ~ v for every
    coalition without ``feature`` and ~ x[feature] with it; all other rows stay moderate.  Row 0
    shares its 4-row pair group (rows 0..3) with moderate rows.  v per regime:

      moderate       0     every |L| < 10
      pair_overflow  -60   L_0 < -44 beside a logit in [-10, 10]: the unshifted pair product
                           overflowed here and dropped the partner (the bug that shipped)
      exp_overflow   -150  L_0 < -116: exp2 itself overflows, the tile takes the NaN fallback
      tb_low         -50   T_0 = logit(x) + c_0 < -44
      high           +80   L_0 > 60

    ``feature`` chooses which coalitions carry the extreme row: with the enumerated design's pairing
    (small subsets are bases) feature 0 and feature d - 1 put it on different base / complement
    columns; ``regime_stats`` counts both sides and ``assert_regime`` demands both."""
    v = {"moderate": 0.0, "pair_overflow": -60.0, "exp_overflow": -150.0, "tb_low": -50.0, "high": 80.0}[regime]
    rng = np.random.default_rng(1000 + REGIMES.index(regime) * 10 + feature)
    a = np.zeros(32)
    a[:d] = rng.normal(0, 0.5, d)
    a[feature] = 1.0
    B = rng.normal(size=(n_bg, d)).astype(F32)
    X = rng.normal(size=(E, d)).astype(F32)
    B[0, feature] = v
    case = Case(f"regime {regime} feature={feature}", a, 0.25, B, X)
    assert_regime(case, regime)
    return case


def regime_stats(case: Case) -> dict:
    L = coalition_logits(case)                                      # [E, nb, S]
    Z = case.design()[0]
    base, comp = complement_pairs(Z)
    a = case.a[: case.d]
    T = (case.X.astype(np.float64) @ a + case.bias)[:, None] + (case.B.astype(np.float64) @ a + case.bias)[None, :]
    nb = case.n_bg
    grp = np.arange(nb) // 4
    mod = (np.abs(L) <= 10.0)
    low = L < -44.0
    beside = np.zeros_like(low)
    for g in np.unique(grp):                                        # a moderate row in the same 4-row group
        rows = grp == g
        beside[:, rows, :] = low[:, rows, :] & (mod[:, rows, :].sum(1, keepdims=True) > 0)
    side = np.zeros(Z.shape[0], bool)
    side[base] = True
    return {
        "max_abs": float(np.abs(L).max()),
        "low_beside_moderate": int(beside.sum()),
        "below_116_base": int((L[:, :, side] < -116.5).sum()),
        "below_116_comp": int((L[:, :, ~side] < -116.5).sum()),
        "below_44_base": int(low[:, :, side].sum()),
        "below_44_comp": int(low[:, :, ~side].sum()),
        "tb_below_44": int((T < -44.0).sum()),
        "above_60_base": int((L[:, :, side] > 60.0).sum()),
        "above_60_comp": int((L[:, :, ~side] > 60.0).sum()),
    }


def assert_regime(case: Case, regime: str) -> dict:
    """The case reaches the regime it is named after (fp64), on base and on complement columns."""
    st = regime_stats(case)
    if regime == "moderate":
        assert st["max_abs"] < 10.0, st
    elif regime == "pair_overflow":
        assert st["low_beside_moderate"] > 0 and st["below_44_base"] > 0 and st["below_44_comp"] > 0, st
        assert st["below_116_base"] + st["below_116_comp"] == 0, st
    elif regime == "exp_overflow":
        assert st["below_116_base"] > 0 and st["below_116_comp"] > 0 and st["low_beside_moderate"] > 0, st
    elif regime == "tb_low":
        assert st["tb_below_44"] > 0, st
    elif regime == "high":
        assert st["above_60_base"] > 0 and st["above_60_comp"] > 0, st
    else:
        raise ValueError(regime)
    return st


def clamp_case(which: str, d: int = 8, n_bg: int = 9, E: int = 3) -> Case:
    """The two cases that pin the "logit" link's clamps.  Feature 0 alone lifts every background
    row's logit by ``jump``, the rest of the model is small, so a coalition's mean probability is
    either within 1e-9 of 1 (clamped on the device to logit 15.9) or moderate.

      "wide_fx"   jump 36: |logit(x)| > 28, beyond the old host clip of fx at 27.6
      "near_one"  jump 30: logit(x) < 28 and coalition probabilities within 1e-7 of 1"""
    jump = {"wide_fx": 36.0, "near_one": 30.0}[which]
    rng = np.random.default_rng({"wide_fx": 71, "near_one": 72}[which])
    a = np.zeros(32)
    a[:d] = rng.normal(0, 0.3, d)
    a[0] = 1.0
    B = rng.normal(0, 0.5, size=(n_bg, d)).astype(F32)
    X = rng.normal(0, 0.5, size=(E, d)).astype(F32)
    B[:, 0] = rng.normal(0, 0.2, n_bg).astype(F32)
    X[:, 0] = F32(jump)
    case = Case(f"clamp {which}", a, -4.0, B, X, clamped=True)
    lx = case.X.astype(np.float64) @ a[:d] + case.bias
    p = _sig2(-coalition_logits(case) / math.log(2.0)).mean(1)
    assert (np.abs(lx).min() > 28.0) if which == "wide_fx" else (np.abs(lx).max() < 28.0), lx
    assert np.any(1.0 - p < 1e-7), "no coalition within 1e-7 of 1"
    # away from the clamp's edge: clearly clamped or clearly not (no value the bound cannot decide)
    assert np.all((1.0 - p < 1e-9) | (1.0 - p > 1e-4)), "a coalition sits on the clamp's edge"
    return case


def assert_unclamped(case: Case):
    """Every logit-link probability of the case (coalitions, f0) lies in [1e-6, 1 - 1e-6]: no clamp
    of either implementation binds."""
    p = _sig2(-coalition_logits(case) / math.log(2.0)).mean(1)
    c = case.B.astype(np.float64) @ case.a[: case.d] + case.bias
    p0 = float((1.0 / (1.0 + np.exp(-c))).mean())
    assert p.min() >= 1e-6 and p.max() <= 1 - 1e-6 and 1e-6 <= p0 <= 1 - 1e-6, (case.name, p.min(), p.max(), p0)


# ---------------------------------------------------------------------------------------------
# oracle 1: exact
# ---------------------------------------------------------------------------------------------
def closed_form(X, B, a, bias):
    """logit_model: phi_i = a_i (x_i - mean_b B_bi), fx = a . x + bias, f0 = mean_b (a . B_b + bias)."""
    X, B = np.asarray(X, np.float64), np.asarray(B, np.float64)
    a = np.asarray(a, np.float64)[: X.shape[1]]
    return a[None, :] * (X - B.mean(0)[None, :]), X @ a + bias, float((B @ a + bias).mean())


def brute_force_shapley(X, B, a, bias, link: str, clamp=CLAMP_DEVICE):
    """(phi [E, d], fx [E], f0) in fp64: Shapley values of v(S) = link(mean_b f(x_S, B_b,~S)) by the
    subset-weight formula phi_i = sum_{S without i} |S|! (d - |S| - 1)! / d! (v(S + i) - v(S)) over all
    2^d subsets.  Uses neither the coalition design nor the WLS operator.  ``clamp`` = (lo, hi)
    bounds the mean probability under the "logit" link (the device: CLAMP_DEVICE); the full
    coalition's value is the model's logit itself, unclamped, as shap's link of the model output."""
    X, B = np.asarray(X, np.float64), np.asarray(B, np.float64)
    E, d = X.shape
    if d > 11:
        raise ValueError("brute force enumerates 2^d subsets: d <= 11")
    a = np.asarray(a, np.float64)[:d]
    m = np.arange(1 << d)
    masks = (m[:, None] >> np.arange(d)[None, :] & 1).astype(np.float64)     # [2^d, d]
    size = masks.sum(1).astype(int)
    w = np.array([math.factorial(s) * math.factorial(d - s - 1) / math.factorial(d) for s in range(d)] + [0.0])
    c = B @ a + bias
    lx = X @ a + bias
    phi = np.zeros((E, d))
    fx = np.empty(E)
    f0 = 0.0
    for e in range(E):
        L = masks @ (a[:, None] * (X[e][:, None] - B.T)) + c[None, :]            # [2^d, nb]
        if link == "logit_model":
            v = L.mean(1)
        else:
            with np.errstate(over="ignore"):
                v = (1.0 / (1.0 + np.exp(-L))).mean(1)
            if link == "logit":
                v = _logit(np.clip(v, clamp[0], clamp[1]))
                v[-1] = lx[e]
        fx[e], f0 = v[-1], float(v[0])
        for i in range(d):
            without = m[(m >> i & 1) == 0]
            phi[e, i] = np.sum(w[size[without]] * (v[without | (1 << i)] - v[without]))
    return phi, fx, f0


def exact(case: Case, link: str):
    """The exact oracle of a case: brute force (d <= 11), kernelshap_reference (sampled designs)."""
    if case.d <= 11:
        return brute_force_shapley(case.X, case.B, case.a, case.bias, link, case.clamp)
    if link == "logit":
        assert not case.clamped
        assert_unclamped(case)          # kernelshap_reference clips at CLAMP_HOST: it must not bind
    Z, _, A, zM = case.design()
    return EX.kernelshap_reference(case.X, case.a, case.bias, case.B, Z, A, zM, link)


# ---------------------------------------------------------------------------------------------
# oracle at the kernel's operands
# ---------------------------------------------------------------------------------------------
def operands(case: Case, logits: bool) -> dict:
    """The kernel's operands, reproduced bit for bit on the host.

    a32, W [n_bg, 32], cb [n_bg]   what ops/kernelshap._device_design uploads
    xs [E, 32]                     fl(a32 x) (columns >= d: 0)
    hi, lo [E, n_bg, 32] fp32      the bf16 halves of u = fl(fl(xs - W) us), us = 1 (logits) or
                                   fl(-log2 e); column 31 = the intercept fl(cb us); column 30 = -40
                                   (sigmoid links: the exp2 shift) or 0
    op = hi + lo in fp64           what the MFMA multiplies
    T [E, n_bg] fp64               T_b = sum of the feature columns + 2 x the intercept column of op:
                                   the paired kernel's complement identity L_b(1 - z) = T_b - L_b(z)"""
    d, nb = case.d, case.n_bg
    a32 = np.zeros(32, F32)
    a32[:d] = case.a[:d]
    xs = np.zeros((case.X.shape[0], 32), F32)
    xs[:, :d] = a32[None, :d] * case.X.astype(F32)
    cb = (case.B.astype(np.float64) @ case.a[:d] + case.bias).astype(F32)
    W = np.zeros((nb, 32), F32)
    W[:, :d] = case.B.astype(F32) * a32[None, :d]
    W[:, 31] = -cb
    us = F32(1.0) if logits else -LOG2E32
    u = ((xs[:, None, :] - W[None, :, :]) * us).astype(F32)
    if not logits:
        u[:, :, 30] = -PAIR_SHIFT
    hi = _bf16(u)
    lo = _bf16(u - hi)
    op = hi.astype(np.float64) + lo.astype(np.float64)
    T = op[:, :, :30].sum(2) + 2.0 * op[:, :, 31]
    return {"a32": a32, "W": W, "cb": cb, "xs": xs, "us": us, "u": u, "hi": hi, "lo": lo, "op": op, "T": T,
            "bias32": F32(case.bias)}


def _A32(case):
    _, _, A, zM = case.design()
    return A.astype(F32).astype(np.float64), (A @ zM).astype(F32).astype(np.float64)


def _finish64(v, f0l, fxl, A, Az):
    y = v - f0l
    delta = fxl - f0l
    phi = np.empty((v.shape[0], A.shape[0] + 1))
    phi[:, :-1] = y @ A.T - np.outer(delta, Az)
    phi[:, -1] = delta - phi[:, :-1].sum(1)
    return phi, delta


def oracle_at_operands(case: Case, link: str, ops: dict | None = None) -> dict:
    """fp64 evaluation of coalition values, link, projection and last feature from ``operands``
    (and the fp32 A, A z_M, bias the kernel receives): what a kernel with exact arithmetic returns.
    In exact arithmetic T_b - L_b(z) is L_b(1 - z) from the same halves, so both kernels share it."""
    logits = link == "logit_model"
    ops = ops or operands(case, logits)
    Z = case.design()[0].astype(np.float64)
    d = case.d
    A, Az = _A32(case)
    acc = np.einsum("ebk,sk->ebs", ops["op"][:, :, :d], Z) + ops["op"][:, :, 31][:, :, None]   # unshifted
    cb = ops["cb"].astype(np.float64)
    lx = ops["xs"].astype(np.float64).sum(1) + float(ops["bias32"])
    if logits:
        p, p0 = acc.mean(1), float(cb.mean())
        v, f0l, fxl = p, p0, lx
    else:
        p, p0 = _sig2(acc).mean(1), float((1.0 / (1.0 + np.exp(-cb))).mean())
        if link == "logit":
            v, f0l, fxl = _logit(np.clip(p, *case.clamp)), float(_logit(np.clip(p0, *case.clamp))), lx
        else:
            v, f0l, fxl = p, p0, 1.0 / (1.0 + np.exp(-lx))
    phi, delta = _finish64(v, f0l, fxl, A, Az)
    return {"phi": phi, "fx": fxl, "f0": f0l, "delta": delta, "acc": acc, "p": p, "p0": p0, "v": v, "lx": lx}


# ---------------------------------------------------------------------------------------------
# bounds
# ---------------------------------------------------------------------------------------------
def _link_sup(p, ep, link, clamp):
    """sup |link(p') - link(p)| over |p' - p| <= ep: the link is monotone, so at an end point.  With
    the clamp inside, a probability clearly beyond it costs nothing and one near it what it must
    (condition number 1 / (p (1 - p)))."""
    if link != "logit":
        return ep
    g = lambda q: _logit(np.clip(q, clamp[0], clamp[1]))  # noqa: E731
    return np.maximum(np.abs(g(p + ep) - g(p)), np.abs(g(p - ep) - g(p)))


def _sig_sup(acc, eacc):
    s = _sig2(acc)
    return np.maximum(np.abs(_sig2(acc + eacc) - s), np.abs(_sig2(acc - eacc) - s))


def _project_bound(v, ev, f0l, ef0, fxl, efx, A, Az, k_y, k_dot, k_az, k_phi, k_last):
    """Propagate errors ev [E, S] of the link-space coalition values, ef0, efx [E] through
    y = v - f0l, acc_i = sum_s A_is y_s, phi_i = acc_i - Az_i delta, phi_last = delta - sum phi_i.
    f0l's error is common to all y_s, so it enters acc_i through |sum_s A_is|, not sum_s |A_is|.
    k_* count the roundings (units of U) of each step: k_y on |y| and on |delta| (the subtractions),
    k_dot on W_i = sum_s |A_is y_s|, k_az on |Az_i delta|, k_phi on |phi_i|, k_last on
    |delta| + sum |phi_i|.  -> {"phi" [E, d], "fx", "f0", "delta"}."""
    y = v - f0l
    delta = fxl - f0l
    aA = np.abs(A)
    ey = ev + k_y * U * np.abs(y)
    W = np.abs(y) @ aA.T
    ed = efx + ef0 + k_y * U * np.abs(delta)
    phi, _ = _finish64(v, f0l, fxl, A, Az)
    b = np.empty_like(phi)
    # f0l is ONE number subtracted from every v_s: its error reaches acc_i as (sum_s A_is) ef0
    b[:, :-1] = (ey @ aA.T + np.abs(A.sum(1))[None, :] * ef0 + k_dot * U * W + np.abs(Az)[None, :] * ed[:, None]
                 + k_az * U * np.abs(np.outer(delta, Az)) + k_phi * U * np.abs(phi[:, :-1]))
    b[:, -1] = b[:, :-1].sum(1) + ed + k_last * U * (np.abs(delta) + np.abs(phi[:, :-1]).sum(1))
    return {"phi": b, "fx": efx, "f0": ef0, "delta": ed}


def operand_bound(case: Case, link: str) -> dict:
    """|oracle_at_operands - exact| for phi [E, d], fx [E], f0, delta [E].

    One coalition logit is L_b(z) = sum_k z_k a_k (x_k - B_bk) + c_b.  The operand that stands for
    a_k (x_k - B_bk) is hi + lo of fl(fl(fl(a32 x) - fl(a32 B)) us):
      a32 = fl(a)                     relative u on both products
      fl(a32 x), fl(a32 B)            u each                       -> 2 u (|a x| + |a B|) so far
      the subtraction                 u |a x - a B| <= u (|a x| + |a B|)
      us = fl(-log2 e), the product   2 u |u_k|   (the oracle divides by the exact log2 e)
      the split                       |u - hi - lo| <= 2^-8 2^-8 |u| = 2^-16 |u|
    so |error_k| <= (5 u + 2^-16) (|a x_k| + |a B_bk|) =: r m_bk, and the intercept column carries
    fl(c_b) (u), the product (2 u) and the split: (3 u + 2^-16) |c_b|.  The logit error
    eL_bs = r sum_k z_sk m_bk + (3 u + 2^-16) |c_b| goes through the sigmoid as the exact
    sup |sigma(L +- eL) - sigma(L)| (sigma' <= 1/4), the mean over b keeps the mean of the errors.
    f0 sees only fl(c_b): u |c_b| through the sigmoid.  logit(x) sees a32, the product and
    fl(bias): 2 u sum |a x| + u |bias|.  The link: sup over the interval (``_link_sup``).  The
    projection multiplies by fl(A) and fl(A z_M): u on sum_s |A_is y_s| and on |Az_i delta|.  First
    order in the roundings; the interval sups carry the higher orders of the nonlinear steps."""
    logits = link == "logit_model"
    d = case.d
    Zd, _, A, zM = case.design()
    Z = Zd.astype(np.float64)
    a = case.a[:d]
    X, B = case.X.astype(np.float64), case.B.astype(np.float64)
    c = B @ a + case.bias
    mag = np.abs(a * X)[:, None, :] + np.abs(a * B)[None, :, :]              # [E, nb, d]
    eL = (5 * U + UB * UB) * np.einsum("ebk,sk->ebs", mag, Z) + ((3 * U + UB * UB) * np.abs(c))[None, :, None]
    L = coalition_logits(case)
    lx = X @ a + case.bias
    elx = 2 * U * np.abs(a * X).sum(1) + U * abs(case.bias)
    ln2 = math.log(2.0)
    if logits:
        v, ev = L.mean(1), eL.mean(1)
        f0l, ef0 = float(c.mean()), float(U * np.abs(c).mean())
        fxl, efx = lx, elx
    else:
        p, ep = _sig2(-L / ln2).mean(1), _sig_sup(-L / ln2, eL / ln2).mean(1)
        p0 = float(_sig2(-c / ln2).mean())
        ep0 = float(_sig_sup(-c / ln2, U * np.abs(c) / ln2).mean())
        if link == "logit":
            v, ev = _logit(np.clip(p, *case.clamp)), _link_sup(p, ep, link, case.clamp)
            f0l, ef0 = float(_logit(np.clip(p0, *case.clamp))), float(_link_sup(p0, ep0, link, case.clamp))
            fxl, efx = lx, elx
        else:
            v, ev, f0l, ef0 = p, ep, p0, ep0
            fxl, efx = _sig2(-lx / ln2), _sig_sup(-lx / ln2, elx / ln2)
    return _project_bound(v, ev, f0l, ef0, fxl, efx, A, A @ zM, k_y=0, k_dot=1, k_az=1, k_phi=0, k_last=0)


def launch_shape(n_bg: int, n_tiles: int, parts: int) -> dict:
    """The launchers' own formulas: ntb, ngl, null rows evaluated, per part its tile range, the
    tiles run whole (nfull) and the remainder count."""
    ntb = (n_bg + 31) >> 5
    ngl = (n_bg - 32 * (ntb - 1) + 7) >> 3
    st = [(p * n_tiles) // parts for p in range(parts + 1)]
    sizes = [st[p + 1] - st[p] for p in range(parts)]
    return {"ntb": ntb, "ngl": ngl, "nulls": 32 * (ntb - 1) + 8 * ngl - n_bg, "st": st,
            "nfull": [s // 4 * 4 for s in sizes], "rem": [s % 4 for s in sizes]}


def seg_chain(ns: int) -> int:
    """Longest chain of fused multiply-adds into one accumulator of seg_dot over ns coalitions: a
    thread owns ns / 32 float4 steps; rounds of 8 steps spread over 4 accumulators (2 each, into
    a4[0] too), the remaining < 8 steps all go to a4[0]; 4 fused multiply-adds per step."""
    n8 = ns // 32
    return 4 * (2 * (n8 // 8) + n8 % 8)


def n_tiles_of(case: Case, paired: bool) -> int:
    Z = case.design()[0]
    if paired:
        return (len(complement_pairs(Z)[0]) + 31) // 32
    return (Z.shape[0] + 31) // 32


def device_bound(case: Case, link: str, paired: bool, parts: int, ops: dict | None = None,
                 rcp_pow2_exact: bool = False) -> dict:
    """|device - oracle_at_operands| for phi [E, d], fx [E], f0, delta [E], from the kernels' own
    arithmetic.  u = 2^-24, h = HW_ULPS 2^-23 (hardware exp2 / rcp / log), all magnitudes exact.

    accumulator    acc_bs = sum_k op_bk z_sk through 4 MFMAs with fp32 accumulation.  Products with
                   z in {0, 1} are exact; only a nonzero addend can round, and coalition s has
                   n_s = 2 (|z_s| + 1) + 1 <= 64 of them (hi and lo of each member and of the
                   intercept, the shift).  Each rounding is relative to a partial sum, which in any
                   order lies between minus the sum of the negative addends and the sum of the
                   positive ones: P_bs = max of the two (sigmoid links: the 40 of the shift is a
                   negative addend, which is why the accumulator's magnitude is 40 + log2(e) |L|
                   and not |L|):  e_acc = n_s u P_bs.
    paired         tau_b: d + 2 nonzero addends (hi + lo is exact in fp32) summed in sequence with
                   partial sums <= PT_b = sum_k |op_bk| + 2 |op_b31|, then -80: e_T = (d + 2) u PT_b
                   + u (|T_b| + 80); the complement's exponent tau - acc adds the base's e_acc and
                   u |tau - acc|.
    sigmoid        sigma = 2^-40 / (2^-40 + exp2(acc)).  The NaN fallback forms acc + 40 first:
                   u |acc + 40| more on the exponent (charged always).  The exponent error goes
                   through the sigmoid as an exact sup over the interval.  Relative to sigma:
                   exp2 (h), + 2^-40 (u), and per pair the product (u), rcp (h), d0 + d1 (u):
                   (2 h + 3 u); the per-element form (h + u + h) is smaller.
    sum over b     4 fused adds per tile, x + y, the tiles (<= 4), the half-wave exchange; the
                   fallback adds 16 in sequence instead: <= 16 + 4 + 1 = 21 u relative to the sum
                   of nonnegative terms; the paired kernel subtracts null_half (1 u, null rows are
                   part of the sum); times fl(1 / n_bg): 2 u.  Null rows of the unpaired kernel
                   each leave 2^-70.
                   logits link: the same counts relative to sum_b |acc_b| (signed terms); the paired
                   complement is sumT - sb: 8 u sum |T_b| (2 per lane + 6 butterfly levels) + u |f|.
    f0             fast_sigmoid(c_b) = rcp(1 + exp2(fl(-c_b log2 e))): the argument's rounding and
                   fl(log2 e) move the exponent by 2 u |c_b| log2 e, then h, u, h as above;
                   6 butterfly levels + 3 wave sums + 2 for 1 / n_bg: 11 u.
    fx             logit(x) = butterfly sum of fl(a32 x) (6 levels) + bias: 6 u sum |a x| + u |lx|;
                   identity link: fast_sigmoid as for f0.
    link "logit"   the probability's error through ``_link_sup`` (condition number 1 / (p (1 - p))
                   with the clamp inside), then 1 - p (u), the division (u, correctly rounded),
                   v_log_f32 (h relative to max(|log2 r|, 1): its result is exponent + log2 of the
                   mantissa, each good to an ulp of its own magnitude), times fl(ln 2) (2 u |v|).
    projection     y_s = v_s - f0l (u |y|); seg_dot's longest fused chain (``seg_chain`` of the
                   largest part; the paired kernel runs two segments and adds them: + 1), its 4
                   accumulators joined (2), group_sum<8> (3), the parts in order (parts - 1), all
                   relative to W_i = sum_s |A_is y_s|.
    finish         delta = fxl - f0l (u); Az_i delta (u) subtracted (u |phi_i|); the last feature
                   delta - (d - 1 sequential additions): d u (|delta| + sum |phi_i|).
    First order in u; the nonlinear steps use interval sups, which are exact.

    ``rcp_pow2_exact`` (the clamp cases only).  A coalition whose every row is saturated (shifted
    exponent below -66, error included) has d = fl(2^-40 + exp2(acc)) = 2^-40 in every row whatever
    exp2's last bit: pair sums 2^-39, products 2^-80, and IF v_rcp_f32 returns 2^80 for 2^-80 --
    true of a correctly rounded reciprocal, more than the ISA's "1 ULP" promises -- every sigma is
    1.0f, their sum a small integer (the paired kernel's null rows: exact halves), and only
    fl(1 / n_bg) and its product round: p = 1 +- u >= 1 - 2^-24, above the clamp 1 - 2^-23.  Without
    the assumption the derived relative error of p (h alone is 2^-23) reaches across the clamp and
    the bound there is the clamp's whole condition number; the clamp tests assert both."""
    logits = link == "logit_model"
    ops = ops or operands(case, logits)
    ref = oracle_at_operands(case, link, ops)
    d, nb = case.d, case.n_bg
    Zd = case.design()[0]
    Z = Zd.astype(np.float64)
    S = Z.shape[0]
    A, Az = _A32(case)
    aop = np.abs(ops["op"])
    shift = 0.0 if logits else PAIR_SHIFT
    n_s = 2.0 * (Z.sum(1) + 1.0) + 1.0                                        # [S]
    # whatever the order, a partial sum lies between -(sum of the negative addends) and the sum of
    # the positive ones (the shift is a negative addend)
    opd = ops["op"]
    pos = np.einsum("ebk,sk->ebs", np.maximum(opd[:, :, :d], 0.0), Z) + np.maximum(opd[:, :, 31], 0.0)[:, :, None]
    neg = np.einsum("ebk,sk->ebs", np.maximum(-opd[:, :, :d], 0.0), Z) + np.maximum(-opd[:, :, 31], 0.0)[:, :, None] + shift
    P = np.maximum(pos, neg)
    eacc = n_s[None, None, :] * U * P
    acc = ref["acc"]                                                          # unshifted exponent
    nt = n_tiles_of(case, paired)
    shp = launch_shape(nb, nt, parts)
    if paired:
        base, comp = complement_pairs(Zd)
        is_comp = np.zeros(S, bool)
        src = np.arange(S)
        has = comp >= 0
        is_comp[comp[has]] = True
        src[comp[has]] = base[has]
        PT = aop[:, :, :30].sum(2) + 2.0 * aop[:, :, 31]
        T = ops["T"]
        eT = (d + 2) * U * PT + U * (np.abs(T) + 2 * shift)
        # complement columns: exponent tau - acc(base): the base's accumulator error, tau's, the subtraction
        ecomp = eacc[:, :, src] + eT[:, :, None] + U * np.abs(acc - shift)
        eacc = np.where(is_comp[None, None, :], ecomp, eacc)
    if logits:
        sum_abs = np.abs(acc).sum(1)
        if paired:   # a complement is sumT - sb: the base's sum with its roundings, sumT's, the subtraction
            sum_abs = sum_abs[:, src]
        ev = eacc.mean(1) + (21 + 2) * U * sum_abs / nb
        if paired:
            ev = ev + np.where(is_comp[None, :], 8 * U * np.abs(ops["T"]).sum(1)[:, None] / nb + U * np.abs(ref["p"]), 0.0)
        v = ref["p"]
        cb = np.abs(ops["cb"].astype(np.float64))
        ef0 = float(11 * U * cb.mean())
        efx = 6 * U * np.abs(ops["xs"].astype(np.float64)).sum(1) + U * np.abs(ref["lx"])
    else:
        sig = _sig2(acc)
        erow = _sig_sup(acc, eacc + U * np.abs(acc)) + (2 * HWU + 3) * U * sig
        nulls = shp["nulls"]
        rel = (21 + 2 + (1 if paired else 0)) * U
        ep = erow.mean(1) + rel * (ref["p"] + (0.5 * nulls / nb if paired else 0.0))
        if not paired:
            ep = ep + nulls * 2.0 ** -70 / nb
        if rcp_pow2_exact:
            sat = ((acc - shift) + (eacc + U * np.abs(acc)) < -66.0).all(1)       # [E, S]
            ep = np.where(sat, U * ref["p"] + (0.0 if paired else nulls * 2.0 ** -70 / nb), ep)

        def fast_sigmoid_err(c):  # c: logits (fp64), -> error of fast_sigmoid(fl32 c) against sigma(c)
            ex = -c / math.log(2.0)
            return _sig_sup(ex, 2 * U * np.abs(ex)) + (2 * HWU + 1) * U * _sig2(ex)

        cb = ops["cb"].astype(np.float64)
        ep0 = float(fast_sigmoid_err(cb).mean() + 11 * U * ref["p0"])
        elx = 6 * U * np.abs(ops["xs"].astype(np.float64)).sum(1) + U * np.abs(ref["lx"])
        if link == "logit":
            def log_err(p, e):
                q = np.clip(p, *case.clamp)
                r = q / (1.0 - q)
                return (_link_sup(p, e, link, case.clamp) + 2 * U
                        + HWU * U * np.maximum(np.abs(np.log2(r)), 1.0) * math.log(2.0) + 2 * U * np.abs(np.log(r)))
            v, ev = ref["v"], log_err(ref["p"], ep)
            ef0 = float(log_err(ref["p0"], ep0))
            efx = elx
        else:
            v, ev, ef0 = ref["p"], ep, ep0
            ex = -ref["lx"] / math.log(2.0)
            efx = _sig_sup(ex, elx / math.log(2.0) + 2 * U * np.abs(ex)) + (2 * HWU + 1) * U * _sig2(ex)
    ns_max = 32 * max(b - a_ for a_, b in zip(shp["st"][:-1], shp["st"][1:]))
    k_dot = seg_chain(ns_max) + (1 if paired else 0) + 2 + 3 + (parts - 1)
    return _project_bound(v, ev, ref["f0"], ef0, ref["fx"], efx, A, Az, k_y=1, k_dot=k_dot, k_az=1, k_phi=1, k_last=d)


def efficiency_bound(phi, fx, f0, d):
    """|sum_i phi_i - (fx - f0)| of the device's own outputs: phi_last = fl(delta - s), s the
    sequential fp32 sum of the other d - 1, delta = fl(fx - f0): d roundings of partial sums no
    larger than |delta| + sum |phi_i|."""
    phi = np.asarray(phi, np.float64)
    return d * U * (np.abs(np.asarray(fx, np.float64) - f0) + np.abs(phi).sum(1))


# ---------------------------------------------------------------------------------------------
# emulation of both kernels in their own precision, and its mutants
# ---------------------------------------------------------------------------------------------
def _f(v):
    return np.asarray(v, F32)


def _fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


def _butterfly(v, width):
    """Sum over the last axis (length ``width``, a power of two) the way xor-shuffles do."""
    v = _f(v)
    while width > 1:
        width //= 2
        v = v[..., :width] + v[..., width:2 * width]
    return v[..., 0]


def _fast_sigmoid32(z):
    with np.errstate(over="ignore"):
        return F32(1.0) / (F32(1.0) + np.exp2(_f(-_f(z)) * LOG2E32))


def _seg_dot(Ai, ys):
    """seg_dot for the 8 lanes of every feature: Ai [d - 1, ns], ys [E, ns] -> [E, d - 1, 8].  Lane
    ``part`` owns the float4 steps part, part + 8, ...; rounds of 8 steps go to accumulators
    0, 1, 2, 3, 0, 1, 2, 3, what is left to accumulator 0."""
    E, ns = ys.shape
    n8 = ns // 32
    Aq = Ai.reshape(Ai.shape[0], n8, 8, 4)
    Yq = ys.reshape(E, n8, 8, 4)
    a4 = [np.zeros((E, Ai.shape[0], 8), F32) for _ in range(4)]

    def step(acc, st):
        for c in (3, 2, 1, 0):
            acc = _fma(Aq[None, :, st, :, c], Yq[:, None, st, :, c], acc)
        return acc

    rounds = n8 // 8
    for r in range(rounds):
        for uu in range(8):
            a4[uu & 3] = step(a4[uu & 3], 8 * r + uu)
    for st in range(8 * rounds, n8):
        a4[0] = step(a4[0], st)
    return (a4[0] + a4[1]) + (a4[2] + a4[3])


def emulate(case: Case, link: str, paired: bool, parts: int, mutant: str | None = None) -> dict:
    """Both kernels in numpy with the kernels' precision: fp32 operands and hi / lo halves, one fp32
    rounding per MFMA of the chain, the shifted pair reciprocal with its NaN fallback, the tile /
    half-wave / remainder-tile summation orders, tau from the halves, null_half, the paired A layout
    with off2, the part split, seg_dot's accumulator order and the sequential last feature.
    exp2 / log / reciprocal are numpy's fp32 ones (within an ulp of the hardware's).
    ``mutant``: one of MUTANTS.  -> {"phi" [E, d], "fx" [E], "f0", "delta" [E]}."""
    if mutant is not None and mutant not in MUTANTS:
        raise ValueError(mutant)
    logits = link == "logit_model"
    ops = operands(case, logits)
    d, nb = case.d, case.n_bg
    E = case.X.shape[0]
    Zd, _, A64, zM = case.design()
    S = Zd.shape[0]
    nt = n_tiles_of(case, paired)
    shp = launch_shape(nb, nt, parts)
    ntb, ngl = shp["ntb"], shp["ngl"]
    ngl_eval = ngl - 1 if mutant == "ngl_short" else ngl
    nrow = 32 * ntb
    kOne = F32(2.0 ** -40)
    # operand halves, null rows appended
    hi = np.zeros((E, nrow, 32), F32)
    lo = np.zeros((E, nrow, 32), F32)
    hi[:, :nb], lo[:, :nb] = ops["hi"], ops["lo"]
    if not logits:
        hi[:, nb:, 30] = -PAIR_SHIFT
        if not paired and mutant != "null_counted":
            hi[:, nb:, 31] = NULL_ACC
    if mutant == "no_lo":
        lo[:] = 0.0
    # coalition columns
    if paired:
        base, comp = complement_pairs(Zd)
        Ppad = 32 * nt
        Zc = np.zeros((Ppad, 32))
        Zc[: len(base), :d] = Zd[base]
        Ap = np.zeros((d - 1, 2 * Ppad), F32)
        Ap[:, : len(base)] = A64[:, base]
        has = comp >= 0
        Ap[:, Ppad + np.nonzero(has)[0]] = A64[:, comp[has]]
        ncol = Ppad
    else:
        ncol = 32 * nt
        Zc = np.zeros((ncol, 32))
        Zc[:S, :d] = Zd
        Ap = np.zeros((d - 1, ncol), F32)
        Ap[:, :S] = A64
    Zc[:, 30] = 1.0
    Zc[:, 31] = 1.0
    acc = np.zeros((E, nrow, ncol), F32)
    for h_, k0 in ((hi, 0), (lo, 0), (hi, 16), (lo, 16)):   # 4 MFMAs, fp32 accumulator
        acc = (acc.astype(np.float64) + np.einsum("ebk,sk->ebs", h_[:, :, k0:k0 + 16].astype(np.float64),
                                                   Zc[:, k0:k0 + 16])).astype(F32)
    accr = acc.reshape(E, ntb, 4, 2, 4, ncol)                # [e, tile, group j, half h, row k, col]
    inv_nb = F32(1.0) / F32(nb)
    old = np.seterr(over="ignore", invalid="ignore")
    try:
        if paired:
            # tau from the halves, in the kernel's column order (skipping the shift column)
            tsum = np.zeros((E, nrow), F32)
            for k in range(32):
                if k != 30:
                    tsum = tsum + (hi[:, :, k] + lo[:, :, k])
            c31 = hi[:, :, 31] + lo[:, :, 31]
            tau = tsum if mutant == "tau_no_c" else tsum + c31
            tau = np.where(np.arange(nrow)[None, :] < nb, tau, F32(0.0)).astype(F32)
            tau = tau - F32(0.0 if logits else 2.0 * PAIR_SHIFT)
            taur = tau.reshape(E, ntb, 4, 2, 4)
            null_half = F32(0.0 if mutant == "null_counted" else 0.5 * (32 * (ntb - 1) + 8 * ngl - nb))
            per_tile = []                                    # per background tile: ([E, 2, col] base, comp)
            for t in range(ntb):
                ng = 4 if t < ntb - 1 else ngl_eval
                if logits:
                    ts = np.zeros((E, 2, ncol), F32)
                    for j in range(ng):
                        for k in range(4):
                            ts = ts + accr[:, t, j, :, k]
                    per_tile.append((ts, np.zeros_like(ts)))
                    continue
                tb = [np.zeros((E, 2, ncol), F32) for _ in range(2)]
                tc = [np.zeros((E, 2, ncol), F32) for _ in range(2)]
                fb = np.zeros((E, 2, ncol), F32)
                fc = np.zeros((E, 2, ncol), F32)
                for j in range(ng):
                    a_ = accr[:, t, j]                                        # [E, 2, 4, col]
                    tv = taur[:, t, j][..., None]                             # [E, 2, 4, 1]
                    db = np.exp2(a_) + kOne
                    dc = np.exp2(_f(tv - a_)) + kOne
                    for q, (k0, k1) in enumerate(((0, 1), (2, 3))):
                        for dd, tt in ((db, tb), (dc, tc)):
                            term = _f(dd[:, :, k0] + dd[:, :, k1]).astype(np.float64) * (F32(1.0) / _f(dd[:, :, k0] * dd[:, :, k1]))
                            if mutant == "pair_drop":
                                term = np.where(np.isnan(term), 0.0, term)
                            tt[q] = (term + tt[q]).astype(F32)
                    for k in range(4):
                        fb = fb + F32(1.0) / (F32(1.0) + np.exp2(_f(a_[:, :, k] + F32(PAIR_SHIFT))))
                        fc = fc + F32(1.0) / (F32(1.0) + np.exp2(_f(_f(tv[:, :, k] - a_[:, :, k]) + F32(PAIR_SHIFT))))
                ox, oy = (tb[0] + tb[1]) * kOne, (tc[0] + tc[1]) * kOne
                nan = np.isnan(ox + oy)
                per_tile.append((np.where(nan, fb, ox), np.where(nan, fc, oy)))
            # whole tiles: per half over the background tiles, then the halves; remainder tiles: the
            # halves per background tile, then the tiles in order
            whole = [np.zeros((E, 2, ncol), F32), np.zeros((E, 2, ncol), F32)]
            for t in range(ntb):
                whole = [whole[i] + per_tile[t][i] for i in range(2)]
            whole = [w[:, 0] + w[:, 1] for w in whole]
            remd = [per_tile[0][i][:, 0] + per_tile[0][i][:, 1] for i in range(2)]
            for t in range(1, ntb):
                remd = [remd[i] + (per_tile[t][i][:, 0] + per_tile[t][i][:, 1]) for i in range(2)]
            is_rem = np.zeros(ncol, bool)
            for p in range(parts):
                is_rem[32 * (shp["st"][p] + shp["nfull"][p]): 32 * shp["st"][p + 1]] = True
            sb = np.where(is_rem[None, :], remd[0], whole[0])
            sc = np.where(is_rem[None, :], remd[1], whole[1])
            if logits:
                bq = np.arange(128)
                Tq = np.zeros((E, 128), F32)
                Tq[:, ((bq & ~3) | ((bq & 1) << 1) | ((bq >> 1) & 1))[:nrow]] = tau      # MFMA row order
                Tq = Tq.reshape(E, 2, 64)
                sumT = _butterfly(Tq[:, 0] + Tq[:, 1], 64)
                fbv, fcv = sb, sumT[:, None] - sb
            else:
                fbv, fcv = sb - null_half, sc - null_half
            f = np.concatenate([fbv * inv_nb, fcv * inv_nb], 1)               # [E, 2 Ppad], the kernel's ys layout
        else:
            fs = np.zeros((E, 2, ncol), F32)
            for t in range(ntb):
                ng = 4 if t < ntb - 1 else ngl_eval
                if logits:
                    ts = np.zeros((E, 2, ncol), F32)
                    for j in range(ng):
                        for k in range(4):
                            ts = ts + accr[:, t, j, :, k]
                    fs = fs + ts
                    continue
                tx = np.zeros((E, 2, ncol), F32)
                ty = np.zeros((E, 2, ncol), F32)
                fb = np.zeros((E, 2, ncol), F32)
                for j in range(ng):
                    a_ = accr[:, t, j]
                    dd = np.exp2(a_) + kOne
                    tms = []
                    for k0, k1 in ((0, 1), (2, 3)):
                        term = _f(dd[:, :, k0] + dd[:, :, k1]).astype(np.float64) * (F32(1.0) / _f(dd[:, :, k0] * dd[:, :, k1]))
                        if mutant == "pair_drop":
                            term = np.where(np.isnan(term), 0.0, term)
                        tms.append(term)
                    tx, ty = (tms[0] + tx).astype(F32), (tms[1] + ty).astype(F32)
                    for k in range(4):
                        fb = fb + F32(1.0) / (F32(1.0) + np.exp2(_f(a_[:, :, k] + F32(PAIR_SHIFT))))
                ts = (tx + ty) * kOne
                fs = fs + np.where(np.isnan(ts), fb, ts)
            f = (fs[:, 0] + fs[:, 1]) * inv_nb                                # [E, S_pad]
        # f0, fx
        cb = ops["cb"]
        z0 = np.zeros(256, F32)
        z0[:nb] = cb if logits else _fast_sigmoid32(cb)
        red = _butterfly(z0.reshape(4, 64), 64)
        f0m = (((red[0] + red[1]) + red[2]) + red[3]) * inv_nb
        xs64 = np.concatenate([ops["xs"], np.zeros((E, 32), F32)], 1)
        lx = _butterfly(xs64, 64) + ops["bias32"]
        if link == "logit_model":
            f0l, fxl = f0m, lx
        elif link == "logit":
            p0 = np.minimum(np.maximum(f0m, F32(1e-12)), F32(1.0) - F32(1e-7))
            f0l, fxl = _f(np.log(_f(p0 / (F32(1.0) - p0)))), lx
        else:
            f0l, fxl = f0m, _fast_sigmoid32(lx)
        if link == "logit":
            q = np.minimum(np.maximum(f, F32(1e-12)), F32(1.0) - F32(1e-7))
            f = _f(np.log(_f(q / (F32(1.0) - q))))
        ys = _f(f - f0l)
        if not paired:
            ys[:, S:] = 0.0
        # projection per part, parts summed in order
        ph = None
        for p in range(parts):
            s0, s1 = 32 * shp["st"][p], 32 * shp["st"][p + 1]
            if paired:
                o2 = ncol if (mutant == "off2_no_s0" and p > 0) else ncol + s0
                part = _seg_dot(Ap[:, s0:s1], ys[:, s0:s1]) + _seg_dot(Ap[:, o2:o2 + s1 - s0], ys[:, ncol + s0:ncol + s1])
            else:
                part = _seg_dot(Ap[:, s0:s1], ys[:, s0:s1])
            part = _butterfly(part[..., [0, 4, 2, 6, 1, 5, 3, 7]], 8)         # xor 1, then 2, then 4
            ph = part if ph is None else ph + part
        delta = _f(fxl - f0l)
        Az32 = (A64 @ zM).astype(F32)
        if mutant != "no_az":
            ph = ph - Az32[None, :] * delta[:, None]
        tot = np.zeros(E, F32)
        for k in range(d - 1):
            tot = tot + ph[:, k]
        phi = np.concatenate([ph, (delta - tot)[:, None]], 1)
    finally:
        np.seterr(**old)
    return {"phi": phi.astype(np.float64), "fx": np.asarray(fxl, np.float64), "f0": float(f0l),
            "delta": delta.astype(np.float64)}


# ---------------------------------------------------------------------------------------------
# the GPU case list
# ---------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Run:
    group: str
    key: tuple           # builder arguments of the case (``case_of``)
    link: str
    paired: bool
    parts: int

    @property
    def id(self):
        return f"{'-'.join(str(k) for k in self.key)}-{self.link}-{'paired' if self.paired else 'unpaired'}-p{self.parts}"


@functools.lru_cache(maxsize=None)
def case_of(key: tuple) -> Case:
    kind = key[0]
    if kind == "random":
        return random_case(*key[1:])
    if kind == "regime":
        return regime_case(*key[1:])
    if kind == "clamp":
        return clamp_case(*key[1:])
    raise ValueError(key)


def instantiation_n_bg():
    """[(ntb, ngl, n_bg)]: 32 (ntb - 1) + 8 (ngl - 1) + r with r cycling through 1, 5, 8 (7, 3 and 0
    null rows in the last group); n_bg = 1 and n_bg = 128 are the two corners."""
    out = []
    for ntb in range(1, 5):
        for ngl in range(1, 5):
            r = 1 if (ntb, ngl) == (1, 1) else 8 if (ntb, ngl) == (4, 4) else (1, 5, 8)[(ntb + ngl) % 3]
            out.append((ntb, ngl, 32 * (ntb - 1) + 8 * (ngl - 1) + r))
    return out


PARTS_NBG = {1: 21, 2: 40, 3: 70, 4: 100}      # one n_bg per NTB for the part / remainder sweep


@functools.lru_cache(maxsize=None)
def gpu_runs() -> tuple:
    runs = []
    # every (NTB, NGL) x LOGITS x kernel at d = 8 (127 pairs -> Ppad = 128, S_pad = 256)
    for ntb, ngl, nbg in instantiation_n_bg():
        for link in LINKS:
            for paired in (False, True):
                runs.append(Run("instantiations", ("random", 8, nbg, 3, 100 + nbg), link, paired, 1))
    # parts 1..8 and the four remainder counts at every NTB (paired); the unpaired kernel takes the same sweep
    for ntb, nbg in PARTS_NBG.items():
        for dd, plist in ((8, (2, 3, 4)), (9, (3, 5, 8))):
            for parts in plist:
                for paired in (False, True):
                    link = LINKS[(parts + ntb) % 3]
                    runs.append(Run("parts", ("random", dd, nbg, 1, 200 + dd), link, paired, parts))
    for parts, link in ((1, "identity"), (6, "logit"), (7, "logit_model"), (8, "identity")):
        for paired in (False, True):
            runs.append(Run("parts", ("random", 11, 37, 1, 211), link, paired, parts))
    # small widths: d = 2 (two coalitions, Ppad = 32), d = 3
    for dd in (2, 3):
        for link in LINKS:
            for paired in (False, True):
                runs.append(Run("widths", ("random", dd, 5, 3, 300 + dd), link, paired, 1))
    # sampled designs
    for dd, nbgs in ((12, (8,)), (17, (33,)), (29, (64,)), (30, (100, 128))):
        for nbg in nbgs:
            for i, link in enumerate(LINKS):
                for paired in (False, True):
                    parts = (1, 4, 8)[(i + dd) % 3] if dd == 30 else (1, 2, 5)[(i + dd) % 3]
                    runs.append(Run("sampled", ("random", dd, nbg, 1, 400 + dd), link, paired, parts))
    return tuple(runs)


def regime_runs() -> tuple:
    runs = []
    for regime in REGIMES:
        for feature in (0, 7):
            for link in (("identity", "logit") if regime != "moderate" else LINKS):
                for paired in (False, True):
                    runs.append(Run("regimes", ("regime", regime, feature), link, paired, 1 if feature == 0 else 2))
    return tuple(runs)


def clamp_runs() -> tuple:
    return tuple(Run("clamp", ("clamp", which), "logit", paired, 1) for which in ("wide_fx", "near_one")
                 for paired in (False, True))


def all_runs() -> tuple:
    return gpu_runs() + regime_runs() + clamp_runs()


def coverage(runs) -> dict:
    """What a run list reaches, by the launchers' own formulas."""
    inst = {False: set(), True: set()}
    rem_at = {n: set() for n in range(1, 5)}
    parts, nulls = set(), set()
    for r in runs:
        case = case_of(r.key)
        shp = launch_shape(case.n_bg, n_tiles_of(case, r.paired), r.parts)
        inst[r.paired].add((shp["ntb"], shp["ngl"], r.link == "logit_model"))
        parts.add(r.parts)
        nulls.add(shp["nulls"])
        if r.paired:
            rem_at[shp["ntb"]].update(shp["rem"])
    return {"unpaired": inst[False], "paired": inst[True], "rem_at": rem_at, "parts": parts, "nulls": nulls}


# named witnesses: the run on which each mutant leaves device_bound (chosen on the CPU)
MUTANT_WITNESS = {
    "no_lo": ("regime-tb_low-0-identity-unpaired-p1", "regime-tb_low-0-identity-paired-p1"),
    "pair_drop": ("regime-exp_overflow-0-identity-unpaired-p1", "regime-exp_overflow-0-identity-paired-p1"),
    "null_counted": ("random-8-9-3-109-logit-unpaired-p1", "random-8-9-3-109-logit-paired-p1"),
    "ngl_short": ("random-8-9-3-109-logit-unpaired-p1", "random-8-9-3-109-logit-paired-p1"),
    "tau_no_c": ("random-2-5-3-302-logit_model-paired-p1",),
    "off2_no_s0": ("random-9-70-1-209-logit_model-paired-p8",),
    "no_az": ("random-3-5-3-303-logit_model-unpaired-p1", "random-3-5-3-303-logit_model-paired-p1"),
}


@functools.lru_cache(maxsize=None)
def oracles(key: tuple, link: str) -> dict:
    """Both oracles and the operand bound of one (case, link), computed once and shared (read only):
    {"exact": {"phi", "fx", "f0", "delta"}, "at": oracle_at_operands, "ob": operand_bound, "ops"}."""
    case = case_of(key)
    if link == "logit" and not case.clamped:
        assert_unclamped(case)
    phi, fx, f0 = exact(case, link)
    ops = operands(case, link == "logit_model")
    return {"exact": {"phi": phi, "fx": np.asarray(fx, np.float64), "f0": float(f0), "delta": np.asarray(fx) - f0},
            "at": oracle_at_operands(case, link, ops), "ob": operand_bound(case, link), "ops": ops}


@functools.lru_cache(maxsize=None)
def bound_of(run: Run, rcp_pow2_exact: bool = False) -> dict:
    return device_bound(case_of(run.key), run.link, run.paired, run.parts, oracles(run.key, run.link)["ops"],
                        rcp_pow2_exact)


def assert_outputs_within(got: dict, want: dict, bound: dict, what: str, extra: dict | None = None) -> float:
    """phi, fx, f0 and delta of ``got`` against ``want`` within ``bound`` (+ ``extra``); -> the largest ratio."""
    worst = 0.0
    for k in ("phi", "fx", "f0", "delta"):
        b = np.asarray(bound[k], np.float64) + (np.asarray(extra[k], np.float64) if extra else 0.0)
        worst = max(worst, assert_within(got[k], want[k], b, f"{what} {k}"))
    return worst
