"""CPU oracles for every HIP kernel (SURVEY.md §7.5 "CPU oracles first").

These are the semantics the kernels implement, written plainly in numpy/torch (fp64 unless the
kernel's storage format says otherwise).  GPU tests compare the kernels against these; CPU
tensors run through them, so the whole framework is exercisable without a GPU.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from .layout import BIAS_COL, LABEL_COL, NCOLS

# ------------------------------------------------------------------------------------------
# Philox4x32-10 (bit-exact with common.h philox4x32_10)
# ------------------------------------------------------------------------------------------
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint32(0x9E3779B9), np.uint32(0xBB67AE85)
_MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0: int, k1: int):
    c0 = np.asarray(c0, dtype=np.uint32).copy()
    c1 = np.asarray(c1, dtype=np.uint32).copy()
    c2 = np.asarray(c2, dtype=np.uint32).copy()
    c3 = np.asarray(c3, dtype=np.uint32).copy()
    k0 = np.uint32(k0 & 0xFFFFFFFF)
    k1 = np.uint32(k1 & 0xFFFFFFFF)
    with np.errstate(over="ignore"):
        for _ in range(10):
            p0 = _M0 * c0.astype(np.uint64)
            p1 = _M1 * c2.astype(np.uint64)
            hi0, lo0 = (p0 >> np.uint64(32)).astype(np.uint32), (p0 & _MASK32).astype(np.uint32)
            hi1, lo1 = (p1 >> np.uint64(32)).astype(np.uint32), (p1 & _MASK32).astype(np.uint32)
            c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
            k0 = np.uint32(k0 + _W0)
            k1 = np.uint32(k1 + _W1)
    return c0, c1, c2, c3


def u32_to_unit(v):
    return (np.asarray(v, dtype=np.uint32) >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)


def u32_range(v, n: int):
    return ((np.asarray(v, dtype=np.uint64) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


# ------------------------------------------------------------------------------------------
# storage codecs
# ------------------------------------------------------------------------------------------
def bf16_round(x: np.ndarray) -> np.ndarray:
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16).float().numpy()


def fp8_decode(b: np.ndarray) -> np.ndarray:
    b = np.asarray(b, dtype=np.uint8).astype(np.int64)
    s = (b >> 7) & 1
    e = (b >> 3) & 0xF
    m = b & 7
    sub = m.astype(np.float64) * 2.0 ** -9
    nor = (1.0 + m / 8.0) * np.exp2(e - 7.0)
    out = np.where(e == 0, sub, nor)
    out = np.where((e == 15) & (m == 7), np.nan, out)
    return np.where(s == 1, -out, out).astype(np.float32)


def fp8_encode(x: np.ndarray) -> np.ndarray:
    """RNE, saturating to +-448 (OCP e4m3fn satfinite); mirrors common.h f32_to_fp8e4m3."""
    x = np.asarray(x, dtype=np.float32)
    out = np.zeros(x.shape, dtype=np.uint8)
    flat_x = x.reshape(-1)
    flat_o = out.reshape(-1)
    for i, v in enumerate(flat_x):  # small arrays only (tests)
        flat_o[i] = _fp8_encode_scalar(float(v))
    return out


def _fp8_encode_scalar(f: float) -> int:
    sign = 0x80 if math.copysign(1.0, f) < 0 else 0
    a = abs(f)
    if a != a:
        return 0x7F
    if a >= 464.0:
        return sign | 0x7E
    if a < 2.0 ** -10:
        return sign
    fr, e = math.frexp(a)
    be = e - 1 + 7
    if be <= 0:
        r = _rint(a * 512.0)
        return sign | int(r)
    mant = (fr * 2.0 - 1.0) * 8.0
    r = _rint(mant)
    if r >= 8.0:
        r = 0.0
        be += 1
    if be > 15 or (be == 15 and r >= 7.0):
        return sign | 0x7E
    return sign | (be << 3) | int(r)


def _rint(v: float) -> float:
    return float(np.rint(np.float32(v)))


def rows_to_f32(rows: torch.Tensor, fp8_scale: float = 4.0, d: int = 30) -> torch.Tensor:
    """Decode a padded row buffer (bf16 / f32 / fp8-as-uint8) to fp32 [n, 32] in model space."""
    if rows.dtype == torch.bfloat16:
        return rows.float()
    if rows.dtype == torch.float32:
        return rows
    if rows.dtype == torch.uint8:
        v = torch.from_numpy(fp8_decode(rows.cpu().numpy()))
        v[:, :d] /= fp8_scale
        return v
    raise ValueError(rows.dtype)


# ------------------------------------------------------------------------------------------
# K1 / K2 scaler
# ------------------------------------------------------------------------------------------
def scaler_sums(X: np.ndarray, pivot: np.ndarray) -> np.ndarray:
    X = np.asarray(X, dtype=np.float32)
    d = X.shape[1]
    D = X.astype(np.float64) - np.asarray(pivot, dtype=np.float32).astype(np.float64)[None, :d]
    out = np.zeros(64)
    out[:d] = D.sum(0)
    out[32 : 32 + d] = (D * D).sum(0)
    return out


def scaler_finalize(sums: np.ndarray, n: float, pivot: np.ndarray, d: int):
    eps = np.finfo(np.float64).eps
    mean = np.zeros(32)
    var = np.zeros(32)
    scale = np.ones(32)
    m = sums[:d] / n
    mean[:d] = np.asarray(pivot[:d], dtype=np.float32).astype(np.float64) + m
    v = np.maximum(sums[32 : 32 + d] / n - m * m, 0.0)
    var[:d] = v
    ub = n * eps * v + (n * mean[:d] * eps) ** 2
    scale[:d] = np.where(v <= ub, 1.0, np.sqrt(v))
    mean32 = mean.astype(np.float32)
    inv32 = np.zeros(32, dtype=np.float32)
    inv32[:d] = (1.0 / scale[:d]).astype(np.float32)
    return mean, var, scale, mean32, inv32


def scale_cast(X, mean32, inv32, labels=None, bias_value=1.0, out_kind="bf16", fp8_scale=4.0, idx=None):
    X = np.asarray(X, dtype=np.float32)
    if idx is not None:
        X = X[np.asarray(idx)]
        if labels is not None:
            labels = np.asarray(labels)[np.asarray(idx)]
    n, d = X.shape
    out = np.zeros((n, NCOLS), dtype=np.float32)
    out[:, :d] = (X - mean32[None, :d]) * inv32[None, :d]
    out[:, BIAS_COL] = bias_value
    if labels is not None:
        out[:, LABEL_COL] = np.asarray(labels, dtype=np.float32)
    if out_kind == "bf16":
        return torch.from_numpy(out).to(torch.bfloat16)
    if out_kind == "f32":
        return torch.from_numpy(out)
    if out_kind == "fp8":
        scaled = out.copy()
        scaled[:, :d] *= fp8_scale
        return torch.from_numpy(fp8_encode(scaled))
    raise ValueError(out_kind)


# ------------------------------------------------------------------------------------------
# K5 / K6 predict + linear SHAP
# ------------------------------------------------------------------------------------------
def sigmoid(z):
    return 1.0 / (1.0 + np.exp(-z))


def predict_rows(rows_f32: np.ndarray, w: np.ndarray):
    w = np.asarray(w, dtype=np.float64).copy()
    w[LABEL_COL] = 0.0
    z = np.asarray(rows_f32, dtype=np.float64) @ w
    return sigmoid(z), z


def predict_shap(X: np.ndarray, a: np.ndarray, c: np.ndarray, bias: float, dz: int, dphi: int):
    X = np.asarray(X, dtype=np.float64)
    a = np.asarray(a, dtype=np.float64)
    c = np.asarray(c, dtype=np.float64)
    z = X[:, :dz] @ a[:dz] + bias
    phi = a[None, :dphi] * (X[:, :dphi] - c[None, :dphi])
    return sigmoid(z), z, phi


# ------------------------------------------------------------------------------------------
# K4 logistic regression
# ------------------------------------------------------------------------------------------
def logreg_pass(rows_f32: np.ndarray, w: np.ndarray, class_w=(1.0, 1.0), hessian=True):
    R = np.asarray(rows_f32, dtype=np.float64)
    y = R[:, LABEL_COL].copy()
    X = R.copy()
    X[:, LABEL_COL] = 0.0
    w = np.asarray(w, dtype=np.float64).copy()
    w[LABEL_COL] = 0.0
    z = X @ w
    p = sigmoid(z)
    s = np.where(y > 0.5, class_w[1], class_w[0])
    r = s * (p - y)
    g = X.T @ r
    loss = float(np.sum(s * (np.logaddexp(0.0, z) - y * z)))
    wsum = float(s.sum())
    H = (X * (s * p * (1 - p))[:, None]).T @ X if hessian else None
    return g, loss, wsum, H


def pack_reduced(g, loss, wsum, H) -> np.ndarray:
    red = np.zeros(1088)
    red[:32] = g
    red[32] = loss
    red[33] = wsum
    if H is not None:
        red[64:] = np.asarray(H).reshape(-1)
    return red


def logreg_grad_abs(rows_f32: np.ndarray, w: np.ndarray, class_w=(1.0, 1.0)) -> np.ndarray:
    """sum_i |r_i x_ij| per column: the absolute-term sum of logreg_pass's gradient, the scale an
    accumulation error of the device pass is measured against (the loss's own terms are all
    positive, so its absolute-term sum is the loss)."""
    R = np.asarray(rows_f32, dtype=np.float64)
    y = R[:, LABEL_COL].copy()
    X = R.copy()
    X[:, LABEL_COL] = 0.0
    w = np.asarray(w, dtype=np.float64).copy()
    w[LABEL_COL] = 0.0
    s = np.where(y > 0.5, class_w[1], class_w[0])
    r = s * (sigmoid(X @ w) - y)
    return np.abs(X).T @ np.abs(r)


def logreg_pass_tiles(rows_f32: np.ndarray, w: np.ndarray, class_w=(1.0, 1.0), hess_stride: int = 1, sub: int = 1,
                      phase: int = 0, gw: int = 4096, hessian: bool = True) -> np.ndarray:
    """The reduced [1088] vector of one device pass (logreg.hip bf16_wave_pass / fp8_wave_pass) over
    the rows, with the pass's tile walk: rows come in tiles of ROW_TILE; the pass visits tile t iff
    t mod sub == phase; the visited tiles are numbered j = t // sub and tile j is the i = j // gw-th
    tile of wave j mod gw (gw = 4 waves x the grid's blocks).  That tile feeds the Hessian iff
    (wave mod hess_stride + i) mod hess_stride == 0.  g, loss and red[33] cover every visited row;
    H = hess_stride x the feeding tiles' Hessian and red[34] = hess_stride x their weight (the
    Newton update rescales H by red[33] / red[34]).  ``hessian`` False: a gradient pass, H and
    red[34] zero.  A CV hole is applied by deleting the block from the rows first."""
    R = np.asarray(rows_f32, dtype=np.float64)
    hs, sub, gw = int(hess_stride), int(sub), int(gw)
    if hs < 1 or sub < 1 or gw < 1 or not 0 <= phase < sub:
        raise ValueError("logreg_pass_tiles: hess_stride, sub, gw >= 1 and 0 <= phase < sub")
    t = np.arange(R.shape[0], dtype=np.int64) // ROW_TILE
    visited = t % sub == phase
    j = t // sub
    wave, i = j % gw, j // gw
    g, loss, wsum, _ = logreg_pass(R[visited], w, class_w, hessian=False)
    red = pack_reduced(g, loss, wsum, None)
    if hessian:
        feeds = visited & ((wave % hs + i) % hs == 0)
        _, _, wh, H = logreg_pass(R[feeds], w, class_w, hessian=True)
        red[34] = hs * wh
        red[64:] = hs * np.asarray(H).reshape(-1)
    return red


def fold_weights(w: np.ndarray, affine: np.ndarray) -> np.ndarray:
    """Standardized-space weights -> weights for pivot-shifted rows s with z = (s - c) inv
    (logreg.hip store_folded; affine = c | inv): v_j = w_j inv_j, v_30 = w_30 - sum_j w_j inv_j c_j,
    label slot 0.  fp64; the device stores it rounded to fp32."""
    w = np.asarray(w, dtype=np.float64)
    a = np.asarray(affine, dtype=np.float64)
    c, inv = a[:32], a[32:]
    v = w * inv
    v[BIAS_COL] = w[BIAS_COL] - float(np.sum(w * inv * c))
    v[LABEL_COL] = 0.0
    return v


def newton_system(red, w, d, C, fit_intercept=True, affine=None):
    """(idx, A, grad, obj, gmax) of one Newton update from the reduced vector: the active
    coordinates, the matrix A = H[idx, idx] / S_H + reg I_pen the update factors, the gradient and
    objective of sklearn's loss at ``w``, and the gradient's max norm over idx.  ``affine`` (c | inv,
    [64]): the sums were taken over pivot-shifted rows s, z = (s - c) inv, and map to standardized
    space first: g_z[j] = inv_j (g_j - c_j g_30),
    H_z[j][k] = inv_j inv_k (H_jk - c_j H_30k - c_k H_j30 + c_j c_k H_30,30)."""
    red = np.asarray(red, dtype=np.float64)
    g = red[:32]
    Hf = red[64:].reshape(32, 32)
    if affine is not None:
        a = np.asarray(affine, dtype=np.float64)
        c, inv = a[:32], a[32:]
        g = inv * (g - c * g[BIAS_COL])
        Hf = np.outer(inv, inv) * (Hf - np.outer(c, Hf[BIAS_COL, :]) - np.outer(Hf[:, BIAS_COL], c)
                                   + np.outer(c, c) * Hf[BIAS_COL, BIAS_COL])
    S = red[33] if red[33] > 0 else 1.0
    reg = 1.0 / (C * S)
    idx = list(range(d)) + ([BIAS_COL] if fit_intercept else [])
    grad = np.zeros(32)
    grad[:d] = g[:d] / S + reg * w[:d]
    if fit_intercept:
        grad[BIAS_COL] = g[BIAS_COL] / S
    obj = red[32] / S + 0.5 * reg * float(np.dot(w[:d], w[:d]))
    gmax = float(np.max(np.abs(grad[idx])))
    SH = red[34] if red[34] > 0 else S  # weight of the rows behind H (device: slot 34)
    A = Hf[np.ix_(idx, idx)] / SH
    for k, j in enumerate(idx):
        if j < d:
            A[k, k] += reg
    return idx, A, grad, obj, gmax


class NewtonStateRef:
    """Mirror of logreg.hip newton_update_kernel (same decisions, fp64)."""

    def __init__(self, w0: np.ndarray):
        self.w = np.asarray(w0, dtype=np.float64).copy()
        self.w_prev = self.w.copy()
        self.step = np.zeros(32)
        self.vel = np.zeros(32)
        self.obj_prev = np.inf
        self.iter = 0
        self.backtracks = 0
        self.gmax = np.inf
        self.obj = np.inf
        self.n_accepted = 0
        self.converged = False
        self.done = False

    def update(self, red, d, C, tol, max_iter, fit_intercept=True, phase_start=False, affine=None):
        """``phase_start``: first iteration of a progressive-Newton phase -- the previous objective
        counts as +inf and the backtrack count as 0 (objectives of different row samples are not
        comparable).  ``affine``: see newton_system."""
        if self.done:
            return
        idx, A, grad, obj, gmax = newton_system(red, self.w, d, C, fit_intercept, affine)
        prev = np.inf if phase_start else self.obj_prev
        nbt = 0 if phase_start else self.backtracks
        self.obj = obj
        if self.iter > 0 and obj > prev + 1e-6 * abs(prev) and nbt < 40:
            self.step *= 0.5
            self.w = self.w_prev + self.step
            self.backtracks = nbt + 1
            dec = 1
        elif gmax <= tol:
            self.gmax = gmax
            self.converged = True
            self.done = True
            dec = 2
        else:
            self.gmax = gmax
            L = np.linalg.cholesky(A)
            st = np.linalg.solve(L.T, np.linalg.solve(L, -grad[idx]))
            self.w_prev = self.w.copy()
            self.step = np.zeros(32)
            self.step[idx] = st
            self.w = self.w_prev + self.step
            self.obj_prev = obj
            self.backtracks = 0
            self.n_accepted += 1
            dec = 0
        self.iter += 1
        if dec != 2 and self.iter >= max_iter:
            self.done = True


WAVES_PER_BLOCK = 4     # logreg.hip kThreads / 64
ROW_TILE = 64           # rows per wave tile
PICK_TILE = 16          # virtual-SMOTE picks per wave tile (bf16 and fp8 passes: 4 lanes per pick)
PICK_TILE_BF16 = PICK_TILE
SGD_MIN_SPAN = 4        # every SGD minibatch spans >= 4 strided blocks of row tiles
SGD_FULL_BLOCKS = 512   # the SGD pass grid of a 256-CU MI355X (logreg.hip sgd_full_blocks: 2 per CU)


def sgd_grid_blocks(n_stored: int, nb: int, full_blocks: int) -> int:
    """Blocks of the SGD pass grid: the full resident grid, shrunk for small shards so that every
    minibatch spans >= SGD_MIN_SPAN strided blocks of G = 4 * blocks row tiles (its rows then come
    from the whole shard, not from one contiguous window)."""
    want = int(n_stored) // (ROW_TILE * WAVES_PER_BLOCK * max(1, int(nb)) * SGD_MIN_SPAN)
    return int(max(1, min(int(full_blocks), want)))


def sgd_row_batches(n_stored: int, nb: int, blocks: int | None = None) -> np.ndarray:
    """Minibatch of every stored row (logreg.hip bf16_wave_pass row_phase walk): row tile
    t = row // 64 belongs to minibatch t mod nb (tile-interleaved: every minibatch samples the whole
    shard at 64-row granularity; the grid size ``blocks`` no longer enters)."""
    return (np.arange(int(n_stored), dtype=np.int64) // ROW_TILE) % int(nb)


def sgd_pick_batches(n_picks: int, nb: int, pick_tile: int = PICK_TILE_BF16) -> np.ndarray:
    """Minibatch of every virtual-SMOTE pick: pick tile t = pick // pick_tile belongs to t mod nb
    (all samples of a pick land in the pick's minibatch)."""
    return (np.arange(int(n_picks), dtype=np.int64) // int(pick_tile)) % int(nb)


SGD_DBAR_FLOOR = 1e-3


def sgd_map_sums(g: np.ndarray, affine) -> np.ndarray:
    """Gradient sums over pivot-shifted rows s, z = (s - c) inv, mapped to standardized space:
    rz_t = inv_t (g_t - c_t g_bias) (logreg.hip wave_sums_fixed / sgd_apply; affine = c | inv)."""
    g = np.asarray(g, dtype=np.float64)[:32]
    a = np.asarray(affine, dtype=np.float64)
    return a[32:] * (g - a[:32] * g[BIAS_COL])


class SgdStateRef:
    """Mirror of logreg.hip sgd_apply (fp64): heavy-ball momentum SGD with the step normalised by
    the minibatch's mean curvature, Polyak averaging, epoch-end convergence state.

    ``dbar`` / ``lr``: the step's clamped mean curvature and step size (state slots 227 / 228).
    ``mag``: per quantity, the sum of the absolute values of the terms of its expression in the last
    step (magnitudes propagated through the chain: |a + b| is charged |a|'s own magnitude plus
    |b|'s) -- the scale a rounding-error bound of another fp64 evaluation order is stated against."""

    def __init__(self, w0: np.ndarray):
        self.w = np.asarray(w0, dtype=np.float64).copy()
        self.v = np.zeros(32)
        self.avg = np.zeros(32)
        self.n_avg = 0
        self.ep_g = np.zeros(32)
        self.ep_loss = 0.0
        self.ep_w = 0.0
        self.iter = 0
        self.gmax = np.inf
        self.obj = np.inf
        self.converged = False
        self.done = False
        self.dbar = 0.0
        self.lr = 0.0
        self.mag = {}

    def step(self, g_raw, loss, wsum, dsum, d, C, c, mom, nb, avg, epoch_end, tol, fit_intercept=True,
             affine=None, mapped=False):
        """``affine`` (c | inv, [64]): the sums were taken over pivot-shifted rows.  ``mapped`` False:
        ``g_raw`` holds the raw sums and is mapped to standardized space first (sgd_map_sums);
        True: it is mapped already (the fused passes map every wave's sums)."""
        if self.done:
            return
        g_raw = np.asarray(g_raw, dtype=np.float64)[:32]
        m_raw = np.abs(g_raw)
        if affine is not None and not mapped:
            a = np.asarray(affine, dtype=np.float64)
            m_raw = np.abs(a[32:]) * (np.abs(g_raw) + np.abs(a[:32] * g_raw[BIAS_COL]))
            g_raw = sgd_map_sums(g_raw, a)
        S = wsum if wsum > 0 else 1.0
        reg = 1.0 / (C * S * nb)
        dbar = max(dsum / S, SGD_DBAR_FLOOR)
        lr = c / dbar
        g = np.zeros(32)
        g[:d] = g_raw[:d] / S + reg * self.w[:d]
        m_g = np.zeros(32)
        m_g[:d] = m_raw[:d] / S + np.abs(reg * self.w[:d])
        if fit_intercept:
            g[BIAS_COL] = g_raw[BIAS_COL] / S
            m_g[BIAS_COL] = m_raw[BIAS_COL] / S
        m_v = np.abs(mom * self.v) + lr * m_g
        m_w = np.abs(self.w) + m_v
        mag = {"v": m_v, "w": m_w, "ep_g": np.abs(self.ep_g) + m_raw, "ep_loss": abs(self.ep_loss) + abs(loss),
               "ep_w": abs(self.ep_w) + abs(wsum), "avg": np.abs(self.avg) + (m_w if avg else 0.0),
               "dbar": abs(dbar), "lr": abs(lr)}
        self.v = mom * self.v - lr * g
        self.w = self.w + self.v
        self.ep_g += g_raw
        self.ep_loss += loss
        self.ep_w += wsum
        if avg:
            self.avg += self.w
            self.n_avg += 1
        self.iter += 1
        self.dbar, self.lr = dbar, lr
        if epoch_end:
            Sw = self.ep_w if self.ep_w > 0 else 1.0
            if self.n_avg > 0:
                self.w = self.avg / self.n_avg
                mag["w"] = mag["avg"] / self.n_avg
            G = np.zeros(32)
            G[:d] = self.ep_g[:d] / Sw + self.w[:d] / (C * Sw)
            m_G = np.zeros(32)
            m_G[:d] = mag["ep_g"][:d] / Sw + mag["w"][:d] / (C * Sw)
            if fit_intercept:
                G[BIAS_COL] = self.ep_g[BIAS_COL] / Sw
                m_G[BIAS_COL] = mag["ep_g"][BIAS_COL] / Sw
            self.gmax = float(np.abs(G).max())
            self.obj = self.ep_loss / Sw + 0.5 * float(self.w[:d] @ self.w[:d]) / (C * Sw)
            mag["gmax"] = float(m_G.max())
            # w^2 moves by 2 |w| dw: charged |w| magnitude squared, without the 1/2
            mag["obj"] = mag["ep_loss"] / Sw + float(mag["w"][:d] @ mag["w"][:d]) / (C * Sw)
            self.ep_g[:] = 0.0
            self.avg[:] = 0.0
            self.ep_loss = self.ep_w = 0.0
            self.n_avg = 0
            if self.gmax <= tol:
                self.converged = self.done = True
        self.mag = mag


def _sgd_members(rows_f64, rsub: int, phase: int, virtual):
    """Rows of minibatch ``phase`` of ``rsub``: the stored rows of the 64-row tiles t with
    t mod rsub == phase, then the virtual samples whose pick tile satisfies the same."""
    R = np.asarray(rows_f64, dtype=np.float64).reshape(-1, NCOLS)
    rsub, phase = int(rsub), int(phase)
    if rsub < 1 or not 0 <= phase < rsub:
        raise ValueError("sgd_pass_sums: rsub >= 1 and 0 <= phase < rsub")
    M = R[(np.arange(R.shape[0], dtype=np.int64) // ROW_TILE) % rsub == phase]
    if virtual is not None:
        samples, pick, n_picks = virtual
        pick = np.asarray(pick).astype(np.int64)
        if pick.size and not (0 <= pick.min() and pick.max() < int(n_picks)):
            raise ValueError("sgd_pass_sums: pick outside [0, n_picks)")
        V = np.asarray(samples, dtype=np.float64).reshape(-1, NCOLS)
        M = np.concatenate([M, V[(pick // PICK_TILE) % rsub == phase]])
    return M


def _sgd_row_terms(M, w, class_w):
    """(X, r, s, loss terms, curvature terms) of the rows M at weights w."""
    y = M[:, LABEL_COL].copy()
    X = M.copy()
    X[:, LABEL_COL] = 0.0
    w = np.asarray(w, dtype=np.float64).copy()
    w[LABEL_COL] = 0.0
    z = X @ w
    with np.errstate(over="ignore"):
        p = sigmoid(z)
    s = np.where(y > 0.5, class_w[1], class_w[0])
    return X, s * (p - y), s, s * (np.logaddexp(0.0, z) - y * z), s * p * (1 - p)


def sgd_pass_sums(rows_f64, w, class_w, rsub: int, phase: int, virtual=None, affine=None) -> np.ndarray:
    """float64 [36], the sums of one SGD minibatch pass (logreg.hip FISH passes): gradient [32] | loss
    | weight | 0 | curvature sum s p (1 - p), over the stored rows with (row // 64) % rsub == phase
    and, with ``virtual`` = (the samples' fp64 rows, every sample's pick, n_picks), the samples with
    (pick // PICK_TILE) % rsub == phase.  A CV hole is applied by deleting the block from the rows
    first.  ``affine`` (c | inv): the gradient mapped to standardized space (sgd_map_sums; the
    device maps every wave's sums -- the map is linear, so mapping the total is the same)."""
    X, r, s, lt, ct = _sgd_row_terms(_sgd_members(rows_f64, rsub, phase, virtual), w, class_w)
    out = np.zeros(36)
    out[:32] = X.T @ r
    out[32], out[33], out[35] = lt.sum(), s.sum(), ct.sum()
    if affine is not None:
        out[:32] = sgd_map_sums(out[:32], affine)
    return out


def sgd_sums_abs(rows_f64, w, class_w, rsub: int, phase: int, virtual=None) -> np.ndarray:
    """sgd_pass_sums (unmapped) over the absolute value of every term: sum |r_i x_it| per gradient
    column, and the loss, weight and curvature sums themselves (their terms are not negative)."""
    X, r, s, lt, ct = _sgd_row_terms(_sgd_members(rows_f64, rsub, phase, virtual), w, class_w)
    out = np.zeros(36)
    out[:32] = np.abs(X).T @ np.abs(r)
    out[32], out[33], out[35] = np.abs(lt).sum(), np.abs(s).sum(), np.abs(ct).sum()
    return out


# ------------------------------------------------------------------------------------------
# K8 / K9 SMOTE
# ------------------------------------------------------------------------------------------
def knn_topk(Q: np.ndarray, C: np.ndarray, k: int, self_offset: int = -1):
    """Exact k nearest neighbours (squared L2 over the 30 feature columns; columns 30/31 of the
    padded layout -- intercept and label -- are not features) with the kernel's tie rule."""
    Q = np.asarray(Q, dtype=np.float64)[:, :30]
    C = np.asarray(C, dtype=np.float64)[:, :30]
    score = Q @ C.T - 0.5 * np.sum(C * C, axis=1)[None, :]
    if self_offset >= 0:
        rows = np.arange(Q.shape[0])
        score[rows, self_offset + rows] = -np.inf
    order = np.lexsort((np.broadcast_to(np.arange(C.shape[0]), score.shape), -score), axis=1)
    idx = order[:, :k].astype(np.int32)
    d2 = np.sum(Q * Q, 1)[:, None] - 2.0 * np.take_along_axis(score, idx.astype(np.int64), 1)
    return idx, d2


SMOTE_MAX_ROWS = 1 << 24  # i / j are packed into 24 bits of a draw (common.h smote_pack_draw)


def smote_check_ranges(n_parents: int, mq: int, k: int) -> None:
    """The packed draw holds i and j in 24 bits and the Lemire pick ranges over mq*k in 32 bits:
    refuse sizes that would silently wrap.  Shard the SMOTE query set above this."""
    if n_parents >= SMOTE_MAX_ROWS:
        raise ValueError(f"SMOTE parent set has {n_parents} rows; the packed draw indexes < 2^24 "
                         f"({SMOTE_MAX_ROWS}) rows -- use smote_scope='shard' or subsample the minority class")
    if mq * k >= 1 << 32:
        raise ValueError(f"SMOTE pick range mq*k = {mq}*{k} does not fit 32 bits")


def smote_plan(nbr: np.ndarray, n_new: int, seed: int, counter_base: int, sample_offset: int = 0) -> np.ndarray:
    """uint32 [n_new, 2] SMOTE draws {i | lam_hi << 24, j | lam_lo << 24} (common.h
    smote_pack_draw): one Philox call per pair of samples -- in 128-sample block m, counter
    64 m + L serves sample 128 m + L with words (x, y) and sample 128 m + 64 + L with (z, w); query
    row i and neighbour slot from one Lemire pick over mq*k, lam = (word >> 16) / 2^16."""
    nbr = np.asarray(nbr)
    mq, k = nbr.shape
    smote_check_ranges(mq, mq, k)
    pick, lam = smote_pick_draws(mq, k, n_new, seed, counter_base, sample_offset)
    i = (pick // k).astype(np.uint32)
    j = nbr[i, pick % k].astype(np.uint32)
    return np.stack([i | ((lam >> np.uint32(8)) << np.uint32(24)), j | ((lam & np.uint32(0xFF)) << np.uint32(24))], 1)


def smote_pick_draws(mq: int, k: int, n_new: int, seed: int, counter_base: int, sample_offset: int = 0):
    """(pick = query row * k + neighbour slot, lam * 2^16) of each sample, uint32 (smote_plan's
    draws before the neighbour lookup; the virtual-SMOTE buckets group samples by pick)."""
    s = np.arange(n_new, dtype=np.uint64) + np.uint64(sample_offset)
    c = (s // np.uint64(128)) * np.uint64(64) + (s % np.uint64(64))
    half = ((s % np.uint64(128)) // np.uint64(64)).astype(bool)
    r = philox4x32_10((c & _MASK32).astype(np.uint32), (c >> np.uint64(32)).astype(np.uint32),
                      np.full(n_new, counter_base & 0xFFFFFFFF, np.uint32),
                      np.full(n_new, (counter_base >> 32) & 0xFFFFFFFF, np.uint32),
                      seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    wp = np.where(half, r[2], r[0])
    wl = np.where(half, r[3], r[1])
    return u32_range(wp, mq * k).astype(np.uint32), wl.astype(np.uint32) >> np.uint32(16)


def smote_draws_decode(plan: np.ndarray):
    """(i, j, lam float32) from smote_plan words."""
    p = np.asarray(plan, dtype=np.uint32)
    lam16 = ((p[:, 0] >> np.uint32(24)) << np.uint32(8)) | (p[:, 1] >> np.uint32(24))
    mask = np.uint32(0xFFFFFF)
    return ((p[:, 0] & mask).astype(np.int64), (p[:, 1] & mask).astype(np.int64),
            lam16.astype(np.float32) * np.float32(1.0 / 65536.0))


def smote_generate(C: np.ndarray, nbr: np.ndarray, q_offset: int, n_new: int, seed: int,
                   counter_base: int, label: float = 1.0, sample_offset: int = 0) -> np.ndarray:
    """fp32 synthetic rows (before bf16/fp8 rounding), bit-exact Philox draws."""
    C = np.asarray(C, dtype=np.float32)
    nbr = np.asarray(nbr)
    i, j, lam = smote_draws_decode(smote_plan(nbr, n_new, seed, counter_base, sample_offset))
    lam = lam[:, None]
    xi = C[q_offset + i]
    xj = C[j]
    out = (xi + lam * (xj - xi)).astype(np.float32)
    out[:, BIAS_COL] = 1.0
    out[:, LABEL_COL] = label
    return out


# ------------------------------------------------------------------------------------------
# K10 metrics
# ------------------------------------------------------------------------------------------
def _tie_groups(scores: np.ndarray):
    """(order, starts, ends): the stable ascending order of the scores and the [start, end) bounds
    of its tie groups.  Bounds come from ``!=`` on neighbours, not from a difference: inf - inf is
    NaN, which would split a group of equal infinite scores into singletons."""
    s = np.asarray(scores, dtype=np.float64).ravel()
    order = np.argsort(s, kind="mergesort")
    ss = s[order]
    bounds = np.flatnonzero(ss[1:] != ss[:-1]) + 1
    return order, np.concatenate([[0], bounds]), np.concatenate([bounds, [len(ss)]])


def roc_auc(scores: np.ndarray, labels: np.ndarray) -> float:
    """Exact ROC-AUC with averaged ties (== sklearn.metrics.roc_auc_score).  +-inf are ordinary
    scores; NaN scores are not supported."""
    y = np.asarray(labels).ravel().astype(bool)
    P, N = int(y.sum()), int((~y).sum())
    if P == 0 or N == 0:
        return float("nan")
    order, starts, ends = _tie_groups(scores)
    ranks = np.empty(len(order))
    avg = (starts + ends + 1) / 2.0  # average ranks over ties
    ranks[order] = np.repeat(avg, ends - starts)
    return float((ranks[y].sum() - P * (P + 1) / 2.0) / (P * N))


def auc_twice_pairs(scores: np.ndarray, labels: np.ndarray) -> int:
    """2 #{s_p > s_n} + #{s_p == s_n} over (positive, negative) pairs as an exact Python integer
    (roc_auc = this / (2 P N)): the sum over positives of twice their average rank,
    start + end + 1 of their tie group, minus P (P + 1).  0 when a class is empty."""
    y = np.asarray(labels).ravel().astype(bool)
    P, N = int(y.sum()), int((~y).sum())
    if P == 0 or N == 0:
        return 0
    order, starts, ends = _tie_groups(scores)
    twice_rank = np.empty(len(order), dtype=np.int64)
    twice_rank[order] = np.repeat((starts + ends + 1).astype(np.int64), ends - starts)
    return int(twice_rank[y].sum(dtype=np.int64)) - P * (P + 1)  # each term <= 2 n + 1: exact below 2^31 rows


def order_key(scores: np.ndarray) -> np.ndarray:
    """Order-preserving uint32 key of float32 scores (auc.hip order_key): a larger score has a
    larger key, -0.0 and +0.0 share one."""
    b = np.ascontiguousarray(scores, dtype=np.float32).ravel().view(np.uint32)
    b = np.where(b == np.uint32(0x80000000), np.uint32(0), b)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def order_key_inv(key: np.ndarray) -> np.ndarray:
    """The float32 score of a key; the -0.0 / +0.0 class comes back as +0.0."""
    k = np.ascontiguousarray(key, dtype=np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


AP_SCALE = float(2 ** 30)  # fixed point of one tie group's average-precision term


def pr_curve(scores: np.ndarray, labels: np.ndarray):
    """(thr float32 [G], tp int64 [G], fp int64 [G]) over the G tie groups of the scores (float32;
    -0.0 == +0.0), descending: tp / fp are the counts of positives / negatives with score >= thr[g].
    precision = tp / (tp + fp), recall = tp / tp[-1] is sklearn.metrics.precision_recall_curve
    without its appended (1, 0) point and in descending-threshold order.  NaN scores are not
    supported (as in roc_auc); +-inf are ordinary scores."""
    key = order_key(scores)
    y = np.asarray(labels).ravel() != 0
    if key.shape[0] == 0:
        return np.zeros(0, np.float32), np.zeros(0, np.int64), np.zeros(0, np.int64)
    order = np.argsort(key, kind="stable")[::-1]
    ks, ys = key[order], y[order]
    last = np.flatnonzero(np.r_[ks[1:] != ks[:-1], True])  # the last row of every group
    tp = np.cumsum(ys, dtype=np.int64)[last]
    fp = (last.astype(np.int64) + 1) - tp
    return order_key_inv(ks[last]), tp, fp


def average_precision_q(scores: np.ndarray, labels: np.ndarray):
    """(ap_q, P, N): ap_q = sum_g rint(dtp[g] * (tp[g] / (tp[g] + fp[g])) * 2^30) over the tie
    groups of pr_curve, dtp[g] = tp[g] - tp[g-1] -- an exact, order-independent integer (every term
    is one correctly rounded fp64 division and product, the sum is int64) with
    |ap_q / 2^30 / P - average_precision_score| <= 2^-31 (each of the <= P non-zero terms is off by
    at most 0.5).  The oracle of auc.hip's pr_ap_kernel."""
    _, tp, fp = pr_curve(scores, labels)
    n = int(np.asarray(labels).size)
    if tp.shape[0] == 0:
        return 0, 0, n
    P = int(tp[-1])
    return ap_q_from_curve(tp, fp), P, n - P


def ap_q_from_curve(tp: np.ndarray, fp: np.ndarray) -> int:
    """sum_g rint(dtp[g] * (tp[g] / (tp[g] + fp[g])) * 2^30) of a curve's cumulative counts."""
    tp = np.asarray(tp, dtype=np.int64)
    fp = np.asarray(fp, dtype=np.int64)
    if tp.shape[0] == 0:
        return 0
    dtp = np.diff(tp, prepend=np.int64(0))
    term = np.rint(dtp.astype(np.float64) * (tp.astype(np.float64) / (tp + fp).astype(np.float64)) * AP_SCALE)
    return int(term.astype(np.int64).sum())


def average_precision(scores: np.ndarray, labels: np.ndarray) -> float:
    """ap_q / 2^30 / P (== sklearn.metrics.average_precision_score within 2^-31); NaN without positives."""
    q, P, _ = average_precision_q(scores, labels)
    return q / AP_SCALE / P if P else float("nan")


def confusion(scores, labels, thr: float):
    s = np.asarray(scores)
    y = np.asarray(labels).astype(bool)
    p = s > thr
    return np.array([np.sum(~y & ~p), np.sum(~y & p), np.sum(y & ~p), np.sum(y & p)], dtype=np.int64)
