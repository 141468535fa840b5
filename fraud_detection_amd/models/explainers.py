"""Explainers: LinearSHAP (K6) and KernelSHAP with the coalition-masked MFMA GEMM (K7).

Reference: shap.LinearExplainer in explain_model.py:24-27 / api/worker.py:53-75 and the
``coef_ * x`` attribution of xai_tasks.py:103-110 (BASELINE.json
config 4).  shap is not installed here; the algorithms are implemented directly:

LinearSHAP (interventional, independent features): phi_i = w_i (x_i - E_bg[x_i]) in the model's
standardized input space; logit(x) = E[logit] + sum(phi).

KernelSHAP (Lundberg & Lee 2017, shap.KernelExplainer semantics without L1 feature selection):
  * coalition design Z (S x M, S = 2M + 2048 by default): subset sizes enumerated completely from
    the outside in (size 1 and M-1, then 2 and M-2, ...) while the remaining sample budget covers
    them, the rest drawn in complement pairs with Shapley-kernel weights; duplicates merge weights;
  * f(z) = mean_b link(model(z * x + (1 - z) * B_b)) over the background rows B;
  * efficiency-constrained weighted least squares: eliminating the last feature,
        phi_{<M} = A (y - z_M * delta),  phi_M = delta - sum(phi_{<M}),
        A = (X^T W X)^-1 X^T W,  X = Z[:, :M-1] - Z[:, M-1],  y = f(z) - f0,  delta = f(x) - f0,
    so A is solved ONCE per design (fp64, host) and every explanation is two GEMMs.
For the logistic model the coalition logits are linear in z:
    logit(z, b) = sum_i z_i u_bi + c_b,   u_b = a * (x - B_b),   c_b = a . B_b + bias,
i.e. one (n_bg x M) x (M x S) GEMM per explanation: on MI355X bf16 MFMA with Z exact in bf16
and u split into hi + lo bf16 (fp32-grade products), sigmoid/mean epilogue fused, then A y.
Identity link on logits (``link="logit_model"``) makes KernelSHAP exactly equal LinearSHAP, which
is the exact oracle the tests use.

Model-agnostic paths (shap.KernelExplainer takes any model; reference train_model.py:95-113 ships an
XGBoost model):
  * ``TreeKernelExplainer`` -- the GBDT family: every masked row z * x + (1 - z) * B_b is walked
    through the ensemble inside the kernel (kernelshap_tree_kernel), never materialised;
  * ``TreeExplainer`` -- interventional TreeSHAP of the GBDT margin: exact, no coalition sampling
    (treeshap.hip), orders of magnitude less work than KernelSHAP on trees;
  * ``TreePathExplainer`` -- path-dependent TreeSHAP of the GBDT margin from the node covers stored
    in the model (treeshap_path.hip): exact, no background, NaN follows the learned default
    direction -- xgboost's pred_contribs; and the SHAP interaction values of the same game
    (treeshap_interact.hip) -- pred_interactions, shap_interaction_values;
  * ``TreePartialDependence`` -- the global counterpart: partial dependence and ICE curves of the
    GBDT margin over the complete threshold grid of one feature or a pair (tree_pd.hip), brute
    (exact integer means over the rows) or by recursion over the stored node covers;
  * ``FunctionKernelExplainer`` -- any callable on device tensors (e.g. a torch model): masked rows
    are built in chunks on the device, the model is called on them, and the shared WLS operator
    projects the coalition values.
The KernelSHAP paths share one cached coalition design per (M, nsamples, seed).
"""
from __future__ import annotations

import functools
import itertools
import math
import time
from dataclasses import dataclass

import numpy as np
import torch

from ..ops import predict as P


# ------------------------------------------------------------------------------------------
# coalition design + WLS operator
# ------------------------------------------------------------------------------------------
def coalition_design(M: int, nsamples: int | None = None, seed: int = 0):
    """Return (Z [S, M] uint8, w [S] float64) following shap's KernelExplainer sampling scheme."""
    nsamples = nsamples or 2 * M + 2048
    max_samples = 2 ** 30 if M > 30 else 2 ** M - 2
    nsamples = min(nsamples, max_samples)
    rng = np.random.default_rng(seed)
    num_sizes = int(math.ceil((M - 1) / 2.0))
    num_paired = int(math.floor((M - 1) / 2.0))
    wv = np.array([(M - 1.0) / (i * (M - i)) for i in range(1, num_sizes + 1)])
    wv[:num_paired] *= 2
    wv /= wv.sum()
    rows, weights = [], []
    left = nsamples
    full_sizes = 0
    rem = wv.copy()
    for size in range(1, num_sizes + 1):
        nsub = math.comb(M, size) * (2 if size <= num_paired else 1)
        if left * rem[size - 1] / nsub >= 1.0 - 1e-8:
            full_sizes += 1
            left -= nsub
            if rem[size - 1] < 1.0:
                rem /= 1.0 - rem[size - 1]
            w = wv[size - 1] / math.comb(M, size)
            if size <= num_paired:
                w /= 2.0
            for inds in itertools.combinations(range(M), size):
                z = np.zeros(M, np.uint8)
                z[list(inds)] = 1
                rows.append(z)
                weights.append(w)
                if size <= num_paired:
                    rows.append(1 - z)
                    weights.append(w)
        else:
            break
    nfixed = len(rows)
    if full_sizes != num_sizes and left > 0:
        rem_w = wv[full_sizes:].copy()
        rem_w /= rem_w.sum()
        seen = {}
        drawn = 0
        budget = left
        while drawn < budget:
            size = rng.choice(len(rem_w), p=rem_w) + full_sizes + 1
            z = np.zeros(M, np.uint8)
            z[rng.permutation(M)[:size]] = 1
            key = z.tobytes()
            if key in seen:
                weights[seen[key]] += 1.0
            else:
                seen[key] = len(rows)
                rows.append(z)
                weights.append(1.0)
            drawn += 1
            if drawn < budget and size <= num_paired:
                zc = 1 - z
                kc = zc.tobytes()
                if kc in seen:
                    weights[seen[kc]] += 1.0
                else:
                    seen[kc] = len(rows)
                    rows.append(zc)
                    weights.append(1.0)
                drawn += 1
        # the sampled part shares the remaining weight mass
        wsum = sum(weights[nfixed:])
        if wsum > 0:
            scale = float(wv[full_sizes:].sum()) / wsum
            for i in range(nfixed, len(weights)):
                weights[i] *= scale
    return np.asarray(rows, np.uint8), np.asarray(weights, np.float64)


@functools.lru_cache(maxsize=16)
def cached_design(M: int, nsamples: int | None = None, seed: int = 0):
    """(Z, w, A, zM) for a design, solved once per process (read-only arrays)."""
    Z, w = coalition_design(M, nsamples, seed)
    A, zM = wls_operator(Z, w)
    for v in (Z, w, A, zM):
        v.setflags(write=False)
    return Z, w, A, zM


def wls_operator(Z: np.ndarray, w: np.ndarray):
    """(A [M-1, S], zlast [S]) of the efficiency-constrained WLS (last feature eliminated)."""
    Zf = Z.astype(np.float64)
    zM = Zf[:, -1]
    Xm = Zf[:, :-1] - zM[:, None]
    XtW = Xm.T * w[None, :]
    G = XtW @ Xm
    A = np.linalg.solve(G + 1e-12 * np.eye(G.shape[0]), XtW)
    return A, zM


def _link(v, link, eps: float = 1e-12):
    """Coalition values and f0 are means of probabilities, clipped to [eps, 1 - eps] before the
    logit.  f(x) is NOT clipped like that: shap applies the link to the model output as it is, and
    the device kernels return the model's own logit (a served LR reaches +-33, beyond
    logit(1 - 1e-12) = 27.6).  Where only a probability is at hand (FunctionKernelExplainer) fx is
    clipped at fp64's resolution of 1 - p, eps = 2^-53, merely to stay finite."""
    if link == "logit":
        v = np.clip(v, eps, 1 - eps)
        return np.log(v / (1 - v))
    return v


def kernelshap_reference(X: np.ndarray, a: np.ndarray, bias: float, B: np.ndarray, Z: np.ndarray, A: np.ndarray,
                         zM: np.ndarray, link: str = "identity") -> tuple:
    """Vectorized fp64 oracle.  X [E, d] raw, B [n_bg, d] raw background, a/bias folded weights.
    link: "identity" (probabilities, shap default), "logit" (shap's logit link on the mean
    probability) or "logit_model" (explain the model's log-odds: equals LinearSHAP exactly).
    Returns (phi [E, d], fx [E], f0)."""
    X = np.asarray(X, np.float64)
    B = np.asarray(B, np.float64)
    d = X.shape[1]
    a = np.asarray(a, np.float64)[:d]
    Zf = Z.astype(np.float64)
    c = B @ a + bias                                 # [n_bg]
    U = a[None, None, :] * (X[:, None, :] - B[None, :, :])  # [E, n_bg, d]
    L = np.einsum("ebd,sd->ebs", U, Zf) + c[None, :, None]  # [E, n_bg, S]
    if link == "logit_model":
        f = L.mean(1)
        f0 = float(c.mean())
        fx = X @ a + bias
    else:
        f = (1.0 / (1.0 + np.exp(-L))).mean(1)
        f0 = float((1.0 / (1.0 + np.exp(-c))).mean())
        fx = 1.0 / (1.0 + np.exp(-(X @ a + bias)))
        f, f0 = _link(f, link), float(_link(np.asarray(f0), link))
        if link == "logit":
            fx = X @ a + bias            # the model's logit itself, unclipped (as the kernels)
    y = f - f0
    delta = fx - f0
    phi = np.empty((X.shape[0], d))
    phi[:, :-1] = y @ A.T - np.outer(delta, A @ zM)
    phi[:, -1] = delta - phi[:, :-1].sum(1)
    return phi, fx, f0


# ------------------------------------------------------------------------------------------
# explainers
# ------------------------------------------------------------------------------------------
class LinearExplainer:
    """phi_i = w_i ((x_i - mu_i)/sigma_i - E_bg[(x_i - mu_i)/sigma_i]) on raw inputs, computed by
    the fused predict + SHAP kernel with the scaler folded into (a, c)."""

    def __init__(self, coef, intercept: float, mean, scale, background: np.ndarray | None = None, device="auto"):
        d = len(mean)
        w = np.zeros(32)
        w[:d] = coef
        w[30] = intercept
        bg_std = None
        if background is not None:
            bg_std = ((np.asarray(background, np.float64) - mean) / scale).mean(0)
        self.a, self.c, self.bias = P.fold_scaler(w, np.asarray(mean), np.asarray(scale), bg_std)
        self.d = d
        self.device = torch.device("cuda", 0) if (device == "auto" and torch.cuda.is_available()) else torch.device(
            "cpu" if device == "auto" else device)
        self.expected_value = float(self.a[:d] @ self.c[:d] + self.bias)

    def shap_values(self, X) -> np.ndarray:
        Xt = torch.as_tensor(np.ascontiguousarray(X, dtype=np.float32)).to(self.device)
        _, phi = P.predict_shap_raw(Xt, torch.from_numpy(self.a).to(self.device),
                                    torch.from_numpy(self.c).to(self.device), self.bias)
        return phi.cpu().numpy()


class KernelExplainer:
    def __init__(self, a: np.ndarray, bias: float, background: np.ndarray, nsamples: int | None = None,
                 link: str = "identity", seed: int = 0, device="auto"):
        B = np.asarray(background, np.float32)
        if B.shape[0] > 128:
            raise ValueError("at most 128 background rows (summarize larger sets, e.g. k-means)")
        self.d = B.shape[1]
        self.a = np.asarray(a, np.float64)
        self.bias = float(bias)
        self.B = B
        self.link = link
        self.Z, self.w, self.A, self.zM = cached_design(self.d, nsamples or None, seed)
        self.device = torch.device("cuda", 0) if (device == "auto" and torch.cuda.is_available()) else torch.device(
            "cpu" if device == "auto" else device)
        self._dev_cache = None

    @property
    def nsamples(self) -> int:
        return self.Z.shape[0]

    def shap_values(self, X) -> np.ndarray:
        return self.explain(X)[0]

    def explain(self, X):
        """-> (phi [E, d], fx [E], f0)."""
        X = np.ascontiguousarray(X, np.float32)
        if self.device.type == "cuda":
            from ..ops.kernelshap import kernelshap

            return kernelshap(torch.from_numpy(X).to(self.device), self)
        return kernelshap_reference(X, self.a, self.bias, self.B, self.Z, self.A, self.zM, self.link)


def _project(f, f0, fx, A, zM):
    """Efficiency-constrained WLS projection of coalition values f [E, S] (fp64 numpy)."""
    y = f - f0
    delta = fx - f0
    phi = np.empty((f.shape[0], A.shape[0] + 1))
    phi[:, :-1] = y @ A.T - np.outer(delta, A @ zM)
    phi[:, -1] = delta - phi[:, :-1].sum(1)
    return phi


def _standardize(X, mean, scale) -> np.ndarray:
    """The device scaler's arithmetic ((x - mean32) * inv32 in fp32, ops/reference.scale_cast)."""
    d = len(mean)
    m32 = np.asarray(mean, np.float64).astype(np.float32)
    i32 = (1.0 / np.asarray(scale, np.float64)).astype(np.float32)
    return ((np.asarray(X, np.float32)[:, :d] - m32[None, :]) * i32[None, :]).astype(np.float32)


def tree_direction_bits(Xs: np.ndarray, ens) -> np.ndarray:
    """uint32 [T, n]: bit n+1 set where row goes right at internal node n (1-based heap; the
    kernel's convention).  Pass-through nodes (feat -1) go left."""
    Xs = np.asarray(Xs, np.float32)
    T, ni = ens.feat.shape
    if ni > 31:
        raise ValueError("tree KernelSHAP supports depth <= 5")
    out = np.zeros((T, Xs.shape[0]), np.uint32)
    for n in range(ni):
        f = ens.feat[:, n]
        v = Xs[:, np.maximum(f, 0)].T                       # [T, n]
        right = (f[:, None] >= 0) & ~(v < ens.thr[:, n][:, None])
        out |= right.astype(np.uint32) << np.uint32(n + 1)
    return out


def _margins_from_bits(R1: np.ndarray, ens) -> np.ndarray:
    """float32 margins (tree order, as the kernel) from direction bits R1 [T, ...]."""
    D = ens.depth
    node = np.ones(R1.shape[1:], np.int64)
    m = np.full(R1.shape[1:], np.float32(ens.base_margin), np.float32)
    for t in range(R1.shape[0]):
        node[...] = 1
        for _ in range(D):
            node = (node << 1) | ((R1[t] >> node.astype(np.uint32)) & 1).astype(np.int64)
        m = (m + ens.leaf[t][node - (1 << D)]).astype(np.float32)
    return m


def kernelshap_tree_reference(Xs: np.ndarray, Bs: np.ndarray, ens, Z: np.ndarray, A: np.ndarray, zM: np.ndarray,
                              link: str = "identity") -> tuple:
    """fp64 oracle of the tree path on STANDARDIZED rows: f(z) = mean_b link(model(z x + (1-z) B_b))
    with float32 margins summed in tree order (the kernel's and the predict kernel's order)."""
    Xs = np.asarray(Xs, np.float32)
    Bs = np.asarray(Bs, np.float32)
    bw = tree_direction_bits(Bs, ens)                      # [T, nb]
    xw = tree_direction_bits(Xs, ens)                      # [T, E]
    T, ni = ens.feat.shape
    fidx = np.maximum(ens.feat, 0)
    zb = Z.astype(bool)
    # node z-bits per (tree, coalition): Zt[t, s] bit n+1 = z_s[feat[t, n]]
    Zt = np.zeros((T, Z.shape[0]), np.uint32)
    for n in range(ni):
        Zt |= zb[:, fidx[:, n]].T.astype(np.uint32) << np.uint32(n + 1)
    sig = (lambda v: v.astype(np.float64)) if link == "logit_model" else (lambda v: 1.0 / (1.0 + np.exp(-v.astype(np.float64))))
    f0 = float(np.mean(sig(_margins_from_bits(bw, ens))))
    mx = _margins_from_bits(xw, ens).astype(np.float64)
    fx = mx if link == "logit_model" else 1.0 / (1.0 + np.exp(-mx))
    f = np.empty((Xs.shape[0], Z.shape[0]))
    for e in range(Xs.shape[0]):
        R1 = (Zt[:, :, None] & xw[:, e][:, None, None]) | (~Zt[:, :, None] & bw[:, None, :])  # [T, S, nb]
        f[e] = sig(_margins_from_bits(R1, ens)).mean(1)
    if link == "logit":
        f, f0, fx = _link(f, link), float(_link(np.asarray(f0), link)), mx   # fx: the margin, unclipped
    return _project(f, f0, fx, A, zM), fx, f0


def _check_tree_features(ens, d: int) -> None:
    """The tree kernels index a 32-bit coalition mask and a [d]-row table by split feature: a model
    whose features do not fit the data's width must not reach them."""
    if d > 30:
        raise ValueError(f"tree explainers support at most 30 features, the background has {d}")
    fmin, fmax = int(ens.feat.min()), int(ens.feat.max())
    if fmin < -1:
        raise ValueError(f"tree ensemble has split feature {fmin}: only -1 (pass-through) may be negative")
    if fmax >= d:
        raise ValueError(f"tree ensemble splits on feature {fmax} (a model of at least {fmax + 1} features) "
                         f"but the background has {d} columns")


def _refuse_default_left(ens, who: str):
    """The tree explainers' kernels send a NaN right at every node (they compare !(x < thr))."""
    dl = getattr(ens, "default_left", None)
    if dl is not None and np.any(dl):
        raise NotImplementedError(f'{who} does not support ensembles with learned missing-value directions '
                                  '(GBDTParams.missing_policy="learn" set default_left on some node)')


class TreeKernelExplainer:
    """KernelSHAP of a tree ensemble (ops/gbdt.TreeEnsemble trained on standardized rows) over RAW
    inputs: the model is standardize -> ensemble, as served.  Background: <= 128 raw rows of the
    width the model was trained on (at most 30 columns, every split feature among them)."""

    def __init__(self, ens, mean, scale, background: np.ndarray, nsamples: int | None = None,
                 link: str = "identity", seed: int = 0, device="auto"):
        B = np.asarray(background, np.float32)
        if B.shape[0] > 128:
            raise ValueError("at most 128 background rows (summarize larger sets)")
        if ens.depth > 5:
            raise ValueError("tree KernelSHAP supports depth <= 5 (the reference trains max_depth=5)")
        _refuse_default_left(ens, "TreeKernelExplainer")
        _check_tree_features(ens, B.shape[1])
        self.ens = ens
        self.d = B.shape[1]
        self.mean = np.asarray(mean, np.float64)
        self.scale = np.asarray(scale, np.float64)
        self.B = B
        self.Bs = _standardize(B, self.mean, self.scale)
        self.bw = tree_direction_bits(self.Bs, ens)         # [T, n_bg]
        self.link = link
        self.Z, self.w, self.A, self.zM = cached_design(self.d, nsamples or None, seed)
        self.zmasks = (self.Z.astype(np.uint64) << np.arange(self.d, dtype=np.uint64)[None, :]).sum(1).astype(np.uint32)
        self.device = torch.device("cuda", 0) if (device == "auto" and torch.cuda.is_available()) else torch.device(
            "cpu" if device == "auto" else device)
        self._dev_cache = None

    @property
    def nsamples(self) -> int:
        return self.Z.shape[0]

    def shap_values(self, X) -> np.ndarray:
        return self.explain(X)[0]

    def explain(self, X):
        """-> (phi [E, d], fx [E], f0) in the link's space (identity: probabilities)."""
        X = np.ascontiguousarray(X, np.float32)
        if self.device.type == "cuda":
            from ..ops.kernelshap import kernelshap_tree

            return kernelshap_tree(torch.from_numpy(X).to(self.device), self)
        return kernelshap_tree_reference(_standardize(X, self.mean, self.scale), self.Bs, self.ens, self.Z, self.A,
                                         self.zM, self.link)


def _treeshap_weights(depth: int):
    """(Wpos, Wneg) [depth+1, depth+1]: (a-1)! b! / (a+b)! and a! (b-1)! / (a+b)!."""
    f = [math.factorial(i) for i in range(2 * depth + 2)]
    wp = np.zeros((depth + 1, depth + 1))
    wn = np.zeros((depth + 1, depth + 1))
    for a in range(depth + 1):
        for b in range(depth + 1 - a):
            if a:
                wp[a, b] = f[a - 1] * f[b] / f[a + b]
            if b:
                wn[a, b] = f[a] * f[b - 1] / f[a + b]
    return wp, wn


def treeshap_reference(Xs: np.ndarray, Bs: np.ndarray, ens) -> tuple:
    """fp64 oracle of interventional TreeSHAP on STANDARDIZED rows (treeshap.hip's algorithm):
    per (x, background z, tree) a depth-first walk over the leaves some hybrid x_S z_~S reaches,
    leaf value v with A (features taken from x where z goes the other way) and B (vice versa)
    contributes v (a-1)! b! / (a+b)! to every i in A and -v a! (b-1)! / (a+b)! to every i in B.
    Returns (phi [E, d] of the margin, margin(x) [E], f0 = mean background margin)."""
    Xs = np.asarray(Xs, np.float32)
    Bs = np.asarray(Bs, np.float32)
    xw = tree_direction_bits(Xs, ens)
    bw = tree_direction_bits(Bs, ens)
    D = ens.depth
    wp, wn = _treeshap_weights(D)
    E, d = Xs.shape
    nb = Bs.shape[0]
    phi = np.zeros((E, d))

    def walk(t, k, level, A, B, xb, zb, acc):
        if level == D:
            if A or B:
                v = float(ens.leaf[t, k - (1 << D)])
                a, b = bin(A).count("1"), bin(B).count("1")
                for i in range(d):
                    if A >> i & 1:
                        acc[i] += v * wp[a, b]
                    if B >> i & 1:
                        acc[i] -= v * wn[a, b]
            return
        f = int(ens.feat[t, k - 1])
        if f < 0:
            return walk(t, 2 * k, level + 1, A, B, xb, zb, acc)
        dx, dz = (xb >> k) & 1, (zb >> k) & 1
        bit = 1 << f
        if dx == dz or A & bit:
            return walk(t, 2 * k + dx, level + 1, A, B, xb, zb, acc)
        if B & bit:
            return walk(t, 2 * k + dz, level + 1, A, B, xb, zb, acc)
        walk(t, 2 * k + dx, level + 1, A | bit, B, xb, zb, acc)
        walk(t, 2 * k + dz, level + 1, A, B | bit, xb, zb, acc)

    for e in range(E):
        acc = np.zeros(d)
        for b in range(nb):
            for t in range(ens.n_trees):
                walk(t, 1, 0, 0, 0, int(xw[t, e]), int(bw[t, b]), acc)
        phi[e] = acc / nb
    fx = _margins_from_bits(xw, ens).astype(np.float64)
    f0 = float(np.mean(_margins_from_bits(bw, ens).astype(np.float64)))
    return phi, fx, f0


class TreeExplainer:
    """Interventional TreeSHAP of a tree ensemble (ops/gbdt.TreeEnsemble on standardized rows)
    over RAW inputs, in margin (log-odds) space -- shap.TreeExplainer(model, data=background,
    feature_perturbation="interventional") semantics, exact (no coalition sampling): the fast
    explainer of the GBDT family (csrc/kernels/treeshap.hip).  Background: <= 1024 raw rows of
    the width the model was trained on (at most 30 columns, every split feature among them)."""

    link = "logit_model"

    def __init__(self, ens, mean, scale, background: np.ndarray, device="auto"):
        B = np.asarray(background, np.float32)
        if B.shape[0] < 1 or B.shape[0] > 1024:
            raise ValueError("1..1024 background rows")
        if ens.depth > 5:
            raise ValueError("TreeSHAP kernel supports depth <= 5 (the reference trains max_depth=5)")
        _refuse_default_left(ens, "TreeExplainer")
        _check_tree_features(ens, B.shape[1])
        self.ens = ens
        self.d = B.shape[1]
        self.mean = np.asarray(mean, np.float64)
        self.scale = np.asarray(scale, np.float64)
        self.B = B
        self.Bs = _standardize(B, self.mean, self.scale)
        self.bw = tree_direction_bits(self.Bs, ens)
        # expected value: mean background margin (float32 tree-order sums, as the predict kernel)
        self.f0 = float(np.mean(_margins_from_bits(self.bw, ens).astype(np.float64)))
        self.device = torch.device("cuda", 0) if (device == "auto" and torch.cuda.is_available()) else torch.device(
            "cpu" if device == "auto" else device)
        self._dev_cache = None

    @property
    def expected_value(self) -> float:
        return self.f0

    def shap_values(self, X) -> np.ndarray:
        return self.explain(X)[0]

    def explain(self, X):
        """-> (phi [E, d], margin(x) [E], f0) in log-odds space; sum(phi) = margin(x) - f0."""
        X = np.ascontiguousarray(X, np.float32)
        if self.device.type == "cuda":
            from ..ops.treeshap import treeshap

            return treeshap(torch.from_numpy(X).to(self.device), self)
        return treeshap_reference(_standardize(X, self.mean, self.scale), self.Bs, self.ens)


def path_fractions(ens) -> np.ndarray:
    """float64 [T, 2^(D+1)]: frac[t, k] = cover[t, k] / cover[t, k >> 1] for heap node k >= 2, the
    weight of child k when its parent's feature is absent.  A split node of cover 0 weighs its
    children 1/2 and 1/2 (the game stays total; the shap package would give NaN); a pass-through
    node sends everything left (1 and 0).  Slots 0 and 1 are 1."""
    if ens.cover is None:
        raise ValueError("the ensemble stores no node cover: run node_cover first")
    T, ni = ens.feat.shape
    cover = np.asarray(ens.cover, np.float64)
    frac = np.ones((T, 2 * (ni + 1)))
    for k in range(2, 2 * (ni + 1)):
        par = k >> 1
        cp = cover[:, par]
        split = ens.feat[:, par - 1] >= 0
        ratio = np.divide(cover[:, k], cp, out=np.full(T, 0.5), where=cp > 0)
        frac[:, k] = np.where(split, ratio, 1.0 if k % 2 == 0 else 0.0)
    return frac


def path_direction_bits(Xs: np.ndarray, ens) -> np.ndarray:
    """tree_direction_bits with NaN routed by default_left (gbdt_predict's walk)."""
    Xs = np.asarray(Xs, np.float32)
    T, ni = ens.feat.shape
    dl = ens.default_left if getattr(ens, "default_left", None) is not None else np.zeros((T, ni), np.uint8)
    out = np.zeros((T, Xs.shape[0]), np.uint32)
    for n in range(ni):
        f = ens.feat[:, n]
        v = Xs[:, np.maximum(f, 0)].T                       # [T, n]
        right = (f[:, None] >= 0) & ~(v < ens.thr[:, n][:, None]) & ~(np.isnan(v) & (dl[:, n][:, None] != 0))
        out |= right.astype(np.uint32) << np.uint32(n + 1)
    return out


def path_expected_value(ens, frac: np.ndarray | None = None) -> float:
    """f0 = base_margin + sum_t v_t(empty set): every leaf weighted by the product of its path's
    fractions, in fp64."""
    frac = path_fractions(ens) if frac is None else frac
    D = ens.depth
    w = np.ones((ens.n_trees, 1 << D))
    for l in range(1 << D):
        heap = (1 << D) + l
        for j in range(D):
            w[:, l] *= frac[:, heap >> (D - j - 1)]
    return float(ens.base_margin + (w * ens.leaf.astype(np.float64)).sum())


def treeshap_path_reference(Xs: np.ndarray, ens) -> tuple:
    """fp64 per-leaf oracle of path-dependent TreeSHAP on STANDARDIZED rows (treeshap_path.hip's
    game; a NaN follows default_left): for leaf L with value v and the distinct split features M
    on its path, z_j = the product of the path's edge fractions at the nodes splitting on j and
    o_j = 1 iff x goes the path's way at all of them; for i in M
        phi_i += v (o_i - z_i) sum_{S in M \\ {i}} |S|! (m - |S| - 1)! / m! prod_{j in S} o_j prod_{j not in S + i} z_j.
    Returns (phi [E, d] of the margin, margin(x) [E], f0 = base margin + sum_t v_t(empty set))."""
    Xs = np.asarray(Xs, np.float32)
    frac = path_fractions(ens)
    xw = path_direction_bits(Xs, ens)
    D = ens.depth
    E, d = Xs.shape
    phi = np.zeros((E, d))
    fact = [math.factorial(i) for i in range(D + 1)]
    feat = ens.feat.tolist()
    for t in range(ens.n_trees):
        for l in range(1 << D):
            heap = (1 << D) + l
            path, dead = [], False                       # (node, child) pairs at split nodes
            for j in range(D):
                k, c = heap >> (D - j), heap >> (D - j - 1)
                if feat[t][k - 1] < 0:
                    dead = dead or bool(c & 1)
                else:
                    path.append((k, c))
            if dead or not path:
                continue
            v = float(ens.leaf[t, l])
            M = sorted({feat[t][k - 1] for k, _ in path})
            m = len(M)
            for e in range(E):
                xb = int(xw[t, e])
                z = {f: 1.0 for f in M}
                o = {f: 1.0 for f in M}
                for k, c in path:
                    f = feat[t][k - 1]
                    z[f] *= frac[t, c]
                    if ((xb >> k) & 1) != (c & 1):
                        o[f] = 0.0
                for i in M:
                    rest = [f for f in M if f != i]
                    W = 0.0
                    for s in range(m):
                        for S in itertools.combinations(rest, s):
                            term = fact[s] * fact[m - s - 1] / fact[m]
                            for f in rest:
                                term *= o[f] if f in S else z[f]
                            W += term
                    phi[e, i] += v * (o[i] - z[i]) * W
    fx = _margins_from_bits(xw, ens).astype(np.float64)
    return phi, fx, path_expected_value(ens, frac)


def treeshap_interactions_reference(Xs: np.ndarray, ens) -> tuple:
    """fp64 per-leaf oracle of the SHAP interaction values of treeshap_path_reference's game on
    STANDARDIZED rows (treeshap_interact.hip's form): for leaf L with value v, distinct path
    features M (m = |M|) and the merged z_j, o_j, every pair i != j in M gets
        Phi_ij += v (o_i - z_i) (o_j - z_j) sum_s s! (m - s - 2)! / (2 (m - 1)!) c_s,
    c_s the coefficient of y^s in prod_{k in M, k != i, j} (z_k + o_k y); the diagonal is
    Phi_ii = phi_i - sum_{j != i} Phi_ij with phi the leaf's ordinary Shapley values.  The matrix
    is symmetric, row i sums to phi_i and everything to margin(x) - f0 (shap's and xgboost's
    convention).  Returns (inter [E, d, d], phi [E, d], margin(x) [E], f0)."""
    Xs = np.asarray(Xs, np.float32)
    frac = path_fractions(ens)
    xw = path_direction_bits(Xs, ens)
    D = ens.depth
    E, d = Xs.shape
    inter = np.zeros((E, d, d))
    phi = np.zeros((E, d))
    fact = [math.factorial(i) for i in range(D + 1)]
    feat = ens.feat.tolist()

    def poly(M, skip, z, o):
        c = [1.0]
        for f in M:
            if f in skip:
                continue
            c = [(c[s] * z[f] if s < len(c) else 0.0) + (c[s - 1] * o[f] if s else 0.0) for s in range(len(c) + 1)]
        return c

    for t in range(ens.n_trees):
        for l in range(1 << D):
            heap = (1 << D) + l
            path, dead = [], False
            for j in range(D):
                k, c = heap >> (D - j), heap >> (D - j - 1)
                if feat[t][k - 1] < 0:
                    dead = dead or bool(c & 1)
                else:
                    path.append((k, c))
            if dead or not path:
                continue
            v = float(ens.leaf[t, l])
            M = sorted({feat[t][k - 1] for k, _ in path})
            m = len(M)
            for e in range(E):
                xb = int(xw[t, e])
                z = {f: 1.0 for f in M}
                o = {f: 1.0 for f in M}
                for k, c in path:
                    f = feat[t][k - 1]
                    z[f] *= frac[t, c]
                    if ((xb >> k) & 1) != (c & 1):
                        o[f] = 0.0
                for i in M:
                    W = sum(fact[s] * fact[m - s - 1] / fact[m] * cs for s, cs in enumerate(poly(M, (i,), z, o)))
                    phi[e, i] += v * (o[i] - z[i]) * W
                for a in range(m):
                    for b in range(a + 1, m):
                        i, j = M[a], M[b]
                        W = sum(fact[s] * fact[m - s - 2] / (2 * fact[m - 1]) * cs
                                for s, cs in enumerate(poly(M, (i, j), z, o)))
                        inter[e, i, j] += v * (o[i] - z[i]) * (o[j] - z[j]) * W
    iu = np.triu_indices(d, 1)
    inter[:, iu[1], iu[0]] = inter[:, iu[0], iu[1]]          # one value per pair: symmetric bit for bit
    idx = np.arange(d)
    inter[:, idx, idx] = phi - inter.sum(2)
    fx = _margins_from_bits(xw, ens).astype(np.float64)
    return inter, phi, fx, path_expected_value(ens, frac)


def _no_cover_message(who: str) -> str:
    return (f"{who} needs the model's node covers: compute them with node_cover "
            "(GBDTClassifier.compute_cover, fit(..., record_cover=True) or train --gbdt-cover)")


class TreePathExplainer:
    """Path-dependent TreeSHAP of a tree ensemble (ops/gbdt.TreeEnsemble on standardized rows) over
    RAW inputs, in margin (log-odds) space -- xgboost's predict(pred_contribs=True) and
    shap.TreeExplainer(model) without data: exact, and with no background set.  The node covers
    stored in the model (ops/gbdt.node_cover) weigh the branches of an absent feature, and a NaN
    in x follows the node's learned default direction, so ensembles with default_left are
    accepted (csrc/kernels/treeshap_path.hip).  At most 30 columns, depth <= 5, <= 2048 trees."""

    link = "logit_model"

    def __init__(self, ens, mean, scale, device="auto"):
        if getattr(ens, "cover", None) is None:
            raise ValueError(_no_cover_message("TreePathExplainer"))
        if not 1 <= ens.depth <= 5:
            raise ValueError("path TreeSHAP supports depth 1..5 (the reference trains max_depth=5)")
        if not 1 <= ens.n_trees <= 2048:
            raise ValueError("path TreeSHAP supports 1..2048 trees")
        self.mean = np.asarray(mean, np.float64)
        self.scale = np.asarray(scale, np.float64)
        self.d = len(self.mean)
        _check_tree_features(ens, self.d)
        if np.asarray(ens.cover).shape != (ens.n_trees, 2 << ens.depth):
            raise ValueError(f"cover must be [{ens.n_trees}, {2 << ens.depth}]")
        if not np.all(np.isfinite(ens.cover)) or np.any(np.asarray(ens.cover) < 0):
            raise ValueError("node covers must be finite and >= 0")
        self.ens = ens
        self.frac = path_fractions(ens)                      # fp64; the device gets it rounded once
        self.f0 = path_expected_value(ens, self.frac)
        self.device = torch.device("cuda", 0) if (device == "auto" and torch.cuda.is_available()) else torch.device(
            "cpu" if device == "auto" else device)
        self._dev_cache = None

    @property
    def expected_value(self) -> float:
        return self.f0

    def shap_values(self, X) -> np.ndarray:
        return self.explain(X)[0]

    def explain(self, X):
        """-> (phi [E, d], margin(x) [E], f0) in log-odds space; sum(phi) = margin(x) - f0."""
        X = np.ascontiguousarray(X, np.float32)
        if self.device.type == "cuda":
            from ..ops.treeshap import treeshap_path

            return treeshap_path(torch.from_numpy(X).to(self.device), self)
        if X.shape[0] == 0:
            return np.zeros((0, self.d)), np.zeros(0), self.f0
        return treeshap_path_reference(_standardize(X, self.mean, self.scale), self.ens)

    def shap_interaction_values(self, X) -> np.ndarray:
        """[E, d, d] -- shap.TreeExplainer(model).shap_interaction_values, xgboost's pred_interactions
        without its bias row and column."""
        return self.explain_interactions(X)[0]

    def explain_interactions(self, X):
        """-> (inter [E, d, d], phi [E, d], margin(x) [E], f0) in log-odds space: inter[e] is
        symmetric, its row i sums to phi[e, i] and the whole matrix to margin(x) - f0
        (csrc/kernels/treeshap_interact.hip on a GPU explainer, the fp64 per-leaf form on CPU)."""
        X = np.ascontiguousarray(X, np.float32)
        if self.device.type == "cuda":
            from ..ops.treeshap import treeshap_interactions

            return treeshap_interactions(torch.from_numpy(X).to(self.device), self)
        if X.shape[0] == 0:
            return np.zeros((0, self.d, self.d)), np.zeros((0, self.d)), np.zeros(0), self.f0
        return treeshap_interactions_reference(_standardize(X, self.mean, self.scale), self.ens)


def partial_dependence_recursion(ens, features) -> np.ndarray:
    """float64 [C]: sklearn's ``method="recursion"`` on the stored node covers, no rows needed --
    the path-dependent game's v({f}) per cell.  rec[c] = base_margin + sum_t sum_leaves leaf * prod
    over the leaf's path of (path_fractions of the child taken) at nodes not on the features and (1
    if the child taken is the side cell c goes, else 0) at nodes on them.  A pair's cells are
    flattened as ca * C_b + cb.  ValueError without covers (path_fractions)."""
    from ..ops.pdp import pd_design

    frac = path_fractions(ens)
    _, _, mask, words = pd_design(ens, features)
    T, D = ens.n_trees, ens.depth
    W = words[0] if len(words) == 1 else (words[0][:, :, None] | words[1][:, None, :]).reshape(T, -1)
    rec = np.full(W.shape[1], float(ens.base_margin))
    for l in range(1 << D):
        heap = (1 << D) + l
        w = np.ones(W.shape)
        for j in range(D):
            k, c = heap >> (D - j), heap >> (D - j - 1)
            on = ((mask >> np.uint32(k)) & 1).astype(bool)
            side = ((W >> np.uint32(k)) & 1) == (c & 1)
            w *= np.where(on[:, None], side, frac[:, c][:, None])
        rec += (w * ens.leaf[:, l].astype(np.float64)[:, None]).sum(0)
    return rec


@dataclass
class PartialDependence:
    """What TreePartialDependence.partial_dependence returns.  ``edges[i]`` / ``edges_raw[i]``: the
    ascending thresholds of ``features[i]`` in standardized / raw units; value cell 0 lies below the
    first edge and cell c >= 1 is [edge c-1, edge c).  ``has_missing_cell``: one more cell, last on
    every axis, holds "the feature is missing".  ``average`` [C_a] or [C_a, C_b] in log-odds;
    ``pd_q`` the exact int64 sums behind it (brute: average = pd_q / 2^30 / n_rows; None for
    recursion); ``ice`` float32 [n, C_a] or [n, C_a, C_b] where asked for."""
    features: tuple
    edges: tuple
    edges_raw: tuple
    has_missing_cell: bool
    average: np.ndarray
    pd_q: np.ndarray | None
    ice: np.ndarray | None
    n_rows: int
    method: str


class TreePartialDependence:
    """Partial dependence and ICE curves of a tree ensemble's margin (ops/gbdt.TreeEnsemble on
    standardized rows) over RAW inputs -- sklearn.inspection.partial_dependence for this family, the
    global counterpart of the tree explainers.  The model is piecewise constant in a feature, so the
    COMPLETE curve has one value per cell between the ensemble's distinct thresholds on it (no grid
    resolution to choose), plus a "missing" cell where the model learned default directions.

    ``method="brute"``: every row's margin with the feature placed in the cell and everything else as
    observed (the interventional v({f}); a NaN elsewhere follows default_left), averaged over the
    rows as an exact int64 sum of llrint(margin * 2^30) -- bitwise reproducible; ICE is bit for bit
    ``predict_margin`` on the modified rows (csrc/kernels/tree_pd.hip on a GPU explainer, the numpy
    oracle on CPU).  ``method="recursion"``: the path-dependent v({f}) from the stored node covers,
    no rows, fp64 on the host.  The two agree at depth 1 (count covers over the same NaN-free rows)
    and differ wherever features interact or are correlated, as in sklearn.  Limits: depth 1..5, at
    most 2048 trees and 30 features, one feature or a pair, at most 65,536 cells."""

    def __init__(self, ens, mean, scale, device="auto"):
        from ..ops import reference_gbdt as R

        self.mean = np.asarray(mean, np.float64)
        self.scale = np.asarray(scale, np.float64)
        self.d = len(self.mean)
        if self.d != ens.n_features:
            raise ValueError(f"model has {ens.n_features} features, the scaler {self.d}")
        R.pd_check(ens, 0, 0)
        _check_tree_features(ens, self.d)
        self.ens = ens
        self.device = torch.device("cuda", 0) if (device == "auto" and torch.cuda.is_available()) else torch.device(
            "cpu" if device == "auto" else device)
        self._dev_cache = None

    def grid(self, f: int):
        """(edges float32 in standardized units, edges float64 in raw units) of feature f."""
        from ..ops.reference_gbdt import pd_grid

        e = pd_grid(self.ens, f)
        return e, e.astype(np.float64) * self.scale[int(f)] + self.mean[int(f)]

    def partial_dependence(self, X=None, features=0, method: str = "brute", ice: bool = False) -> PartialDependence:
        from ..ops import reference_gbdt as R

        if method not in ("brute", "recursion"):
            raise ValueError('method must be "brute" or "recursion"')
        fs = R.pd_features(self.ens, features)
        grids = [self.grid(f) for f in fs]
        shape = tuple(len(R.pd_cells(self.ens, f)[0]) for f in fs)
        common = dict(features=fs, edges=tuple(g[0] for g in grids), edges_raw=tuple(g[1] for g in grids),
                      has_missing_cell=bool(self.ens.has_default_left), method=method)
        if method == "recursion":
            if ice:
                raise ValueError("recursion has no rows and no ICE curves")
            if getattr(self.ens, "cover", None) is None:
                raise ValueError(_no_cover_message("TreePartialDependence"))
            R.pd_check(self.ens, fs, 0)
            return PartialDependence(average=partial_dependence_recursion(self.ens, fs).reshape(shape), pd_q=None,
                                     ice=None, n_rows=0, **common)
        from ..ops.pdp import partial_dependence

        X = np.ascontiguousarray(X, np.float32)
        if X.ndim != 2 or X.shape[0] < 1:
            raise ValueError("brute partial dependence needs at least one row")
        q, ic = partial_dependence(torch.from_numpy(X).to(self.device), self, fs, ice=ice)
        n = X.shape[0]
        return PartialDependence(average=(q.astype(np.float64) / R.PD_SCALE / n).reshape(shape), pd_q=q.reshape(shape),
                                 ice=None if ic is None else ic.reshape((n,) + shape), n_rows=n, **common)


@dataclass
class PermutationImportance:
    """What TreePermutationImportance.permutation_importance returns (the fields of sklearn's
    ``permutation_importance`` Bunch and the exact integers behind them).  ``raw`` int64 [F, R] and
    ``baseline_raw``: the metric kernel's integer per permuted column and for the observed rows
    ("auc": twice_pairs, "aucpr": ap_q, "logloss": loss_q).  ``scores`` / ``baseline_score``: the
    metric, higher is better -- AUC = raw / (2 P N), average precision = raw / 2^30 / P, negative
    log-loss = -raw / 2^30 / n.  ``importances`` = baseline_score - scores, float64 [F, R];
    ``importances_mean`` / ``importances_std`` over the repeats (ddof = 0, as sklearn)."""
    features: tuple
    scoring: str
    n_repeats: int
    seed: int
    baseline_raw: int
    raw: np.ndarray
    baseline_score: float
    scores: np.ndarray
    importances: np.ndarray
    importances_mean: np.ndarray
    importances_std: np.ndarray


class TreePermutationImportance:
    """Permutation feature importance of a tree ensemble (ops/gbdt.TreeEnsemble on standardized rows)
    over RAW inputs -- sklearn.inspection.permutation_importance for this family: how much the
    held-out metric drops when one feature carries no information.

    Column (feature f, repeat r) gives row i the value of feature f of row donor(i) and leaves the
    rest of the row as observed; donor is a keyed Feistel permutation of the rows
    (ops/reference_gbdt.permutation_donors) with the column id 32 r + f, so repeat r of feature f is
    the same permutation whatever ``n_repeats`` and ``features`` are.  The column's margins are bit
    for bit ``predict_margin`` on the explicitly permuted rows (a NaN, the row's own or the donor's,
    follows default_left) and its score is the metric kernel's exact integer, so results are bitwise
    reproducible and equal between the device (csrc/kernels/tree_perm.hip and the metric kernels,
    one read-back) and the CPU (the numpy oracle).  ``scoring``: "auc", "aucpr" (sklearn's average
    precision over tie groups) or "logloss" (sklearn's neg_log_loss, log-loss per row capped at
    -ln 1e-16).  Limits: depth 1..5, at most 2048 trees and 30 features, at most 2^27 rows, labels
    0/1 with both classes for "auc" / "aucpr".  Out of scope: sample weights, data-parallel
    evaluation, the logistic model, other scorers, ``max_samples``."""

    def __init__(self, ens, mean, scale, device="auto"):
        from ..ops import reference_gbdt as R

        self.mean = np.asarray(mean, np.float64)
        self.scale = np.asarray(scale, np.float64)
        self.d = len(self.mean)
        if self.d != ens.n_features:
            raise ValueError(f"model has {ens.n_features} features, the scaler {self.d}")
        R.perm_check(ens, None, 1, 0)
        _check_tree_features(ens, self.d)
        self.ens = ens
        self.device = torch.device("cuda", 0) if (device == "auto" and torch.cuda.is_available()) else torch.device(
            "cpu" if device == "auto" else device)
        self._dev_cache = None

    def permutation_importance(self, X, y, scoring: str = "auc", n_repeats: int = 5, seed: int = 0, features=None,
                               max_bytes: int | None = None) -> PermutationImportance:
        """X [n, d] raw rows and y [n] 0/1 labels, numpy arrays or torch tensors (moved to the
        explainer's device).  ``features``: the feature indices to permute (None: all).
        ``max_bytes``: the cap of the device margin buffer (ops/perm_importance.permutation_scores)."""
        from ..ops import reference_gbdt as R
        from ..ops.perm_importance import DEFAULT_MAX_BYTES, SCORINGS, permutation_scores

        if scoring not in SCORINGS:
            raise ValueError(f"scoring must be one of {SCORINGS}, not {scoring!r}")
        fs = R.perm_check(self.ens, features, n_repeats, seed)
        Xt = X if isinstance(X, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(X, np.float32))
        yt = y if isinstance(y, torch.Tensor) else torch.from_numpy(np.asarray(y))
        if Xt.dim() != 2 or Xt.shape[0] < 1:
            raise ValueError("permutation importance needs at least one row")
        n = int(Xt.shape[0])
        if yt.dim() != 1 or yt.shape[0] != n:
            raise ValueError(f"y must hold one label per row of X ({n}), got shape {tuple(yt.shape)}")
        Xt = Xt.to(self.device, torch.float32)
        yt = (yt.to(self.device) != 0).to(torch.uint8)
        raw, base_raw, P = permutation_scores(Xt, yt, self, fs, scoring, int(n_repeats), int(seed),
                                              DEFAULT_MAX_BYTES if max_bytes is None else int(max_bytes))
        if scoring == "auc":
            to_score = lambda q: q / (2.0 * P * (n - P))  # noqa: E731
        elif scoring == "aucpr":
            to_score = lambda q: q / 2.0 ** 30 / P  # noqa: E731
        else:
            to_score = lambda q: -q / R.LOSS_SCALE / n  # noqa: E731
        scores = to_score(raw.astype(np.float64))
        base = float(to_score(float(base_raw)))
        imp = base - scores
        return PermutationImportance(features=fs, scoring=scoring, n_repeats=int(n_repeats), seed=int(seed),
                                     baseline_raw=int(base_raw), raw=raw, baseline_score=base, scores=scores,
                                     importances=imp, importances_mean=imp.mean(1), importances_std=imp.std(1))


class FunctionKernelExplainer:
    """KernelSHAP of any model given as ``fn(rows: Tensor[N, d]) -> Tensor[N]`` (the model output
    in the link's input space: probabilities for identity / logit, log-odds for logit_model).
    Masked rows are formed on ``device`` in chunks of explanations and the coalition values are
    projected with the shared WLS operator (a plain GEMM: hipBLASLt through torch)."""

    def __init__(self, fn, background: np.ndarray, nsamples: int | None = None, link: str = "identity",
                 seed: int = 0, device="auto", max_rows_per_call: int = 1 << 24):
        self.fn = fn
        self.B = np.asarray(background, np.float32)
        self.d = self.B.shape[1]
        self.link = link
        self.Z, self.w, self.A, self.zM = cached_design(self.d, nsamples or None, seed)
        self.device = torch.device("cuda", 0) if (device == "auto" and torch.cuda.is_available()) else torch.device(
            "cpu" if device == "auto" else device)
        self.max_rows = max_rows_per_call

    @property
    def nsamples(self) -> int:
        return self.Z.shape[0]

    def shap_values(self, X) -> np.ndarray:
        return self.explain(X)[0]

    @torch.no_grad()
    def explain(self, X):
        dev = self.device
        X = torch.as_tensor(np.ascontiguousarray(X, np.float32), device=dev)
        B = torch.from_numpy(self.B).to(dev)
        Z = torch.from_numpy(self.Z.astype(np.float32)).to(dev)            # [S, d]
        E, S, nb = X.shape[0], Z.shape[0], B.shape[0]
        f0 = float(self.fn(B).double().mean())
        fx = self.fn(X).double()
        per = max(1, self.max_rows // (S * nb))
        f = torch.empty((E, S), dtype=torch.float64, device=dev)
        for e0 in range(0, E, per):
            xe = X[e0:e0 + per]                                             # [c, d]
            rows = Z[None, :, None, :] * xe[:, None, None, :] + (1 - Z)[None, :, None, :] * B[None, None, :, :]
            out = self.fn(rows.reshape(-1, self.d)).double().reshape(xe.shape[0], S, nb)
            f[e0:e0 + per] = out.mean(2)
        f, fx = f.cpu().numpy(), fx.cpu().numpy()
        if self.link == "logit":
            f, f0, fx = _link(f, "logit"), float(_link(np.asarray(f0), "logit")), _link(fx, "logit", 2.0 ** -53)
        return _project(f, f0, fx, self.A, self.zM), fx, f0


def kernelshap_throughput(res, dev, comm=None, n_expl: int = 1000, n_bg: int = 100, reps: int = 100) -> dict:
    """bench.py extra: KernelSHAP values/s for 1k explanations/batch (DP: per-rank shards), the
    steady state of a loaded XAI worker.  ~20 ms of back-to-back batches first: the GPU clock
    ramps over milliseconds, and after only 10 warm-up batches (0.6 ms) a 55 us batch measured
    61-63 us (profiles/r2_s5h)."""
    from ..data.synthetic import separable

    a, c, b = res.folded()
    Xb, _ = separable(n_bg, seed=91, device="cpu")
    Xe, _ = separable(n_expl, seed=92 + (comm.rank if comm else 0), device="cpu")
    ke = KernelExplainer(a, b, Xb.numpy(), device=str(dev) if dev.type == "cuda" else "cpu")
    Xd = Xe.to(dev)
    from ..ops.kernelshap import kernelshap

    kernelshap(Xd, ke)
    for _ in range(300):
        kernelshap(Xd, ke, sync=False)
    if comm:
        comm.barrier()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(reps):
        kernelshap(Xd, ke, sync=False)
    torch.cuda.synchronize(dev)
    dt = time.perf_counter() - t0
    if comm:
        dt = comm.max_over_ranks(dt)
    world = comm.world_size if comm else 1
    return {"kernelshap_values_per_sec": round(n_expl * ke.d * reps * world / dt, 1),
            "kernelshap_config": {"explanations_per_batch": n_expl * world, "coalitions": ke.nsamples,
                                  "background": n_bg, "link": ke.link}}
