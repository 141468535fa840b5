"""Crafted tree ensembles, exact oracles and derived fp32 error bounds for the two kernels that
explain the GBDT family: interventional TreeSHAP (csrc/kernels/treeshap.hip) and the tree path of
KernelSHAP (csrc/kernels/kernelshap.hip).

Plain numpy, no GPU import.  The device tests (test_treeshap_gpu.py, test_kernelshap.py,
test_gbdt_gpu.py) compare a kernel with ``brute_force_shapley`` -- all 2^d coalitions, fp64 leaf
sums, its own tree traversal -- within the bounds below; ``walk_stats`` supplies the magnitudes
those bounds scale with and says which branches of the walk the inputs reached, so a test can
assert its own coverage.  test_treeshap.py runs three mutants of the walk through the same
assertions and shows that each one fails them."""
from __future__ import annotations

import math

import numpy as np

from fraud_detection_amd.ops.gbdt import TreeEnsemble

U = 2.0 ** -24          # unit roundoff of fp32
TS_THREADS = 256        # tree_explain.h kTreeThreads: workgroup size = columns of the LDS phi table
KS_LDS_LEAVES = 8192    # kernelshap.hip kTreeLdsLeaves: leaves staged in LDS by the tree kernel
MUTANTS = ("no_forced", "swap_w32", "le_bits")


# ---------------------------------------------------------------------------------------------
# ensembles
# ---------------------------------------------------------------------------------------------
def make_ensemble(d, depth, feat, thr, leaf, base_score=0.3) -> TreeEnsemble:
    feat = np.ascontiguousarray(feat, np.int32)
    return TreeEnsemble(depth=depth, feat=feat, bin=np.zeros_like(feat), thr=np.ascontiguousarray(thr, np.float32),
                        gain=np.zeros(feat.shape), leaf=np.ascontiguousarray(leaf, np.float32),
                        cuts=np.zeros((d, 256), np.float32), nbins=np.full(d, 256, np.int32), base_score=base_score)


def random_ensemble(d, depth, T, seed, p_pass=0.15) -> TreeEnsemble:
    rng = np.random.default_rng(seed)
    ni = (1 << depth) - 1
    feat = rng.integers(0, d, (T, ni)).astype(np.int32)
    feat[rng.random((T, ni)) < p_pass] = -1  # pass-through nodes
    thr = rng.normal(0, 0.7, (T, ni)).astype(np.float32)
    thr[feat < 0] = np.inf
    leaf = rng.normal(0, 0.3, (T, 1 << depth)).astype(np.float32)
    return make_ensemble(d, depth, feat, thr, leaf)


def truncated(ens: TreeEnsemble, T: int) -> TreeEnsemble:
    """The first T trees of an ensemble."""
    return make_ensemble(ens.n_features, ens.depth, ens.feat[:T], ens.thr[:T], ens.leaf[:T], ens.base_score)


def random_rows(d, E, n_bg, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(E, d)).astype(np.float32), rng.normal(size=(n_bg, d)).astype(np.float32)


def disagree_case(depth: int, seed: int = 0):
    """(ens, Xs [1, d], Bs [2^depth, d]), d = depth + 1: one tree whose level-l nodes all split on
    feature l at thr = 0, x = +1 everywhere, backgrounds = every sign pattern of the first ``depth``
    features (the last feature equals x's: its attribution is exactly 0).  A background that differs
    from x in k features splits the walk at k levels and reaches 2^k leaves, one for every way to
    hand those k features to A or B: all (a, b) with 1 <= a + b <= depth are reached."""
    d = depth + 1
    ni = (1 << depth) - 1
    feat = np.array([[int(math.log2(n + 1)) for n in range(ni)]], np.int32)
    thr = np.zeros((1, ni), np.float32)
    leaf = np.random.default_rng(seed).normal(0, 0.3, (1, 1 << depth)).astype(np.float32)
    Xs = np.ones((1, d), np.float32)
    Bs = np.ones((1 << depth, d), np.float32)
    for m in range(1 << depth):
        for l in range(depth):
            if m >> l & 1:
                Bs[m, l] = -1.0
    return make_ensemble(d, depth, feat, thr, leaf), Xs, Bs


def plant_ties(ens: TreeEnsemble, Xs, Bs, seed: int) -> TreeEnsemble:
    """A copy of ``ens`` with a third of its split thresholds replaced, bit for bit, by the value
    an explained row (even picks) or a background row (odd picks) holds in the node's feature."""
    rng = np.random.default_rng(seed)
    thr = ens.thr.copy()
    tt, nn = np.nonzero(ens.feat >= 0)
    pick = rng.permutation(len(tt))[: max(2, len(tt) // 3)]
    for j, p in enumerate(pick):
        src = Xs if j % 2 == 0 else Bs
        thr[tt[p], nn[p]] = src[rng.integers(len(src)), ens.feat[tt[p], nn[p]]]
    return make_ensemble(ens.n_features, ens.depth, ens.feat, thr, ens.leaf, ens.base_score)


def all_ab(depth: int) -> set:
    return {(a, k - a) for k in range(1, depth + 1) for a in range(k + 1)}


# ---------------------------------------------------------------------------------------------
# exact oracle: brute force over coalitions, fp64, its own traversal
# ---------------------------------------------------------------------------------------------
def leaf_index(R: np.ndarray, ens) -> np.ndarray:
    """int [T, n]: the leaf each fp32 row reaches in each tree -- a plain top-down traversal
    (x[feat] < thr goes left, anything else right; a pass-through node goes left)."""
    R = np.asarray(R, np.float32)
    T = ens.n_trees
    out = np.empty((T, R.shape[0]), np.int64)
    rows = np.arange(R.shape[0])
    for t in range(T):
        k = np.ones(R.shape[0], np.int64)
        for _ in range(ens.depth):
            f = ens.feat[t][k - 1]
            left = (f < 0) | (R[rows, np.maximum(f, 0)] < ens.thr[t][k - 1])
            k = 2 * k + (~left).astype(np.int64)
        out[t] = k - (1 << ens.depth)
    return out


def margins64(R: np.ndarray, ens):
    """(margin [n], sum_t |leaf reached| [n]) with fp64 sums of the fp32 leaves."""
    li = leaf_index(R, ens)
    v = np.take_along_axis(ens.leaf.astype(np.float64), li, axis=1)  # [T, n]
    return ens.base_margin + v.sum(0), np.abs(v).sum(0)


def brute_force_shapley(Xs, Bs, ens) -> np.ndarray:
    """phi [E, d] in fp64: Shapley values of v(S) = mean_b margin(x_S, z_b,~S) summed over all 2^d
    coalitions.  Every hybrid row is walked through every tree by ``leaf_index`` and the leaves are
    summed in fp64, so the only rounding is fp64's."""
    Xs = np.asarray(Xs, np.float32)
    Bs = np.asarray(Bs, np.float32)
    E, d = Xs.shape
    if d > 12:
        raise ValueError("brute force enumerates 2^d coalitions: d <= 12")
    nb = Bs.shape[0]
    m = np.arange(1 << d)
    masks = (m[:, None] >> np.arange(d)[None, :] & 1).astype(bool)            # [2^d, d]
    size = masks.sum(1)
    w = np.array([math.factorial(s) * math.factorial(d - s - 1) / math.factorial(d) for s in range(d)] + [0.0])
    phi = np.zeros((E, d))
    chunk = max(1, (1 << 18) // nb)
    for e in range(E):
        v = np.empty(1 << d)
        for c0 in range(0, 1 << d, chunk):
            mk = masks[c0:c0 + chunk]
            hyb = np.where(mk[:, None, :], Xs[e][None, None, :], Bs[None, :, :])  # [c, nb, d]
            v[c0:c0 + chunk] = margins64(hyb.reshape(-1, d), ens)[0].reshape(-1, nb).mean(1)
        for i in range(d):
            without = m[~masks[:, i]]
            phi[e, i] = np.sum(w[size[without]] * (v[without | (1 << i)] - v[without]))
    return phi


# ---------------------------------------------------------------------------------------------
# instrumented copy of the reference walk (and its mutants)
# ---------------------------------------------------------------------------------------------
def _weights(depth):
    f = [math.factorial(i) for i in range(depth + 2)]
    wp = np.zeros((depth + 1, depth + 1))
    wn = np.zeros((depth + 1, depth + 1))
    for a in range(depth + 1):
        for b in range(depth + 1 - a):
            if a:
                wp[a, b] = f[a - 1] * f[b] / f[a + b]
            if b:
                wn[a, b] = f[a] * f[b - 1] / f[a + b]
    return wp, wn


def _bits(R, ens, le=False):
    """Direction bits [T, n] (bit k: heap node k sends the row right).  ``le``: the mutant that
    sends a row sitting exactly on the threshold left."""
    R = np.asarray(R, np.float32)
    out = np.zeros((ens.n_trees, R.shape[0]), np.int64)
    for n in range(ens.feat.shape[1]):
        f = ens.feat[:, n]
        v = R[:, np.maximum(f, 0)].T
        t = ens.thr[:, n][:, None]
        right = (f[:, None] >= 0) & ~((v <= t) if le else (v < t))
        out |= right.astype(np.int64) << (n + 1)
    return out


def walk_stats(Xs, Bs, ens, mutant: str | None = None) -> dict:
    """The reference walk of models/explainers.treeshap_reference, written out again with counters.

    phi [E, d]      the walk's attributions (fp64)
    S [E, d]        absolute mass (1 / n_bg) sum |v| w: phi's own sum with |.| around every term
    ab              set of (a, b) = (|A|, |B|) over the leaves that contributed
    forced_x / forced_z / split / pass_through
                    visited nodes where x and z part and the feature is already in A (forced to
                    x's side) / already in B (forced to z's side) / in neither (the walk splits),
                    and visited pass-through nodes
    ties_x / ties_z visited split nodes whose threshold equals x's / z's value of the feature
    fx [E], fx_abs [E], f0, f0_abs
                    fp64 margin of x and sum_t |leaf reached|; mean background margin and the
                    mean over the background of |base_margin| + sum_t |leaf reached|

    ``mutant`` (None for the faithful walk) is one of MUTANTS: "no_forced" drops the forced-side
    rule (a repeated feature splits again), "swap_w32" swaps the positive and negative weight at
    (a, b) = (3, 2), "le_bits" uses <= for < in the direction bits."""
    if mutant is not None and mutant not in MUTANTS:
        raise ValueError(mutant)
    Xs = np.asarray(Xs, np.float32)
    Bs = np.asarray(Bs, np.float32)
    D = ens.depth
    E, d = Xs.shape
    nb = Bs.shape[0]
    wp, wn = _weights(D)
    if mutant == "swap_w32" and D >= 5:
        wp[3, 2], wn[3, 2] = wn[3, 2], wp[3, 2]
    xw = _bits(Xs, ens, mutant == "le_bits")
    bw = _bits(Bs, ens, mutant == "le_bits")
    feat, thr, leaf = ens.feat.tolist(), ens.thr, ens.leaf.astype(np.float64)
    st = {"ab": set(), "forced_x": 0, "forced_z": 0, "split": 0, "pass_through": 0, "ties_x": 0, "ties_z": 0}
    phi = np.zeros((E, d))
    S = np.zeros((E, d))

    def walk(t, k, level, A, B, xb, zb, x, z, acc, mass):
        if level == D:
            if A or B:
                v = leaf[t, k - (1 << D)]
                a, b = bin(A).count("1"), bin(B).count("1")
                st["ab"].add((a, b))
                for i in range(d):
                    if A >> i & 1:
                        acc[i] += v * wp[a, b]
                        mass[i] += abs(v) * wp[a, b]
                    if B >> i & 1:
                        acc[i] -= v * wn[a, b]
                        mass[i] += abs(v) * wn[a, b]
            return
        f = feat[t][k - 1]
        if f < 0:
            st["pass_through"] += 1
            return walk(t, 2 * k, level + 1, A, B, xb, zb, x, z, acc, mass)
        st["ties_x"] += int(x[f] == thr[t, k - 1])
        st["ties_z"] += int(z[f] == thr[t, k - 1])
        dx, dz = (xb >> k) & 1, (zb >> k) & 1
        bit = 1 << f
        if dx == dz:
            return walk(t, 2 * k + dx, level + 1, A, B, xb, zb, x, z, acc, mass)
        if mutant != "no_forced":
            if A & bit:
                st["forced_x"] += 1
                return walk(t, 2 * k + dx, level + 1, A, B, xb, zb, x, z, acc, mass)
            if B & bit:
                st["forced_z"] += 1
                return walk(t, 2 * k + dz, level + 1, A, B, xb, zb, x, z, acc, mass)
        st["split"] += 1
        walk(t, 2 * k + dx, level + 1, A | bit, B, xb, zb, x, z, acc, mass)
        walk(t, 2 * k + dz, level + 1, A, B | bit, xb, zb, x, z, acc, mass)

    for e in range(E):
        acc, mass = np.zeros(d), np.zeros(d)
        for b in range(nb):
            for t in range(ens.n_trees):
                walk(t, 1, 0, 0, 0, int(xw[t, e]), int(bw[t, b]), Xs[e], Bs[b], acc, mass)
        phi[e] = acc / nb
        S[e] = mass / nb
    fx, fx_abs = margins64(Xs, ens)
    mb, mb_abs = margins64(Bs, ens)
    st.update(phi=phi, S=S, fx=fx, fx_abs=fx_abs, f0=float(mb.mean()),
              f0_abs=float(abs(ens.base_margin) + mb_abs.mean()))
    return st


# ---------------------------------------------------------------------------------------------
# derived error bounds (u = 2^-24)
# ---------------------------------------------------------------------------------------------
def treeshap_lds_boundary(d: int, depth: int) -> int:
    """Largest tree count T* for which launch_treeshap keeps leaves and split features in LDS: its
    documented rule is (d * 256 + T + T * 2^(depth + 1)) * 4 <= 65536 - 1024."""
    words = (65536 - 1024) // 4
    return (words - d * TS_THREADS) // (1 + (2 << depth))


def phi_bound(S, T: int, n_bg: int, depth: int):
    """|phi_gpu - phi_exact| <= (ceil(T n_bg / 256) 2^depth + 32 + 3 + 8) u S, elementwise.

    treeshap.hip sums the terms v w of one (row, feature) in a fixed tree: thread ``tid`` owns the
    pairs tid, tid + 256, ... (at most ceil(T n_bg / 256) of them) and adds each pair's leaf terms
    -- at most 2^depth, one per reachable leaf -- into its own LDS column one after the other: a
    sequential chain of at most ceil(T n_bg / 256) 2^depth additions.  Eight threads per feature
    then add 32 columns each in sequence (32), and a 3-level butterfly joins the eight partial
    sums (3).  A summand that passes through k additions picks up a relative error of at most
    k u (first order), so the sum's error is at most (longest path) u sum |term|, and
    sum |term| / n_bg is the absolute mass S of walk_stats.  Each term is the fp32 product of the
    fp32 leaf and an fp32 weight (a-1)! b! / (a+b)! built from exact small factorials with one
    division: 2 roundings; the final division by n_bg is one more; 8 covers those three with room
    for the second-order terms dropped above."""
    chain = -(-T * n_bg // TS_THREADS) * (1 << depth)
    return (chain + 32 + 3 + 8) * U * np.asarray(S, np.float64)


def fx_bound(fx_abs, T: int, base_margin: float):
    """|fx_gpu - margin(x)| <= (ceil(T / 256) + 6 + 4 + 2) u (|base_margin| + sum_t |leaf reached|).

    Thread ``tid`` adds the leaves of trees tid, tid + 256, ... in sequence (ceil(T / 256)), a
    6-level butterfly sums the wave's 64 lanes (6), thread 0 adds the 4 wave sums to the base
    margin (4); 2 covers the fp32 rounding of the base margin passed by value and second order."""
    return (-(-T // TS_THREADS) + 6 + 4 + 2) * U * (abs(base_margin) + np.asarray(fx_abs, np.float64))


def f0_bound(f0_abs: float, T: int) -> float:
    """The explainer's f0 is computed on the host as the fp64 mean of fp32 margins, each the base
    margin plus T leaves added in tree order in fp32: T sequential additions, so f0 differs from
    the exact mean background margin by at most T u mean_b(|base_margin| + sum_t |leaf reached|).
    The kernel passes f0 through; this term enters only where f0 meets exact quantities
    (efficiency: sum(phi) = fx - f0 holds exactly for the exact f0 only)."""
    return T * U * f0_abs


def efficiency_bound(S, fx_abs, f0_abs, T, n_bg, depth, base_margin):
    """|sum_f phi_gpu - (fx_gpu - f0)| <= sum_f phi_bound + fx_bound + f0_bound: the exact values
    satisfy efficiency exactly, so the residual is at most the sum of the outputs' own errors."""
    return phi_bound(S, T, n_bg, depth).sum(-1) + fx_bound(fx_abs, T, base_margin) + f0_bound(f0_abs, T)


def leaf_mass(ens) -> float:
    """|base_margin| + sum_t max_l |leaf[t, l]|: bounds |margin| of any row, hybrid rows included."""
    return float(abs(ens.base_margin) + np.abs(ens.leaf.astype(np.float64)).max(1).sum())


def kernelshap_any_order_bound(A: np.ndarray, ens, n_bg: int) -> np.ndarray:
    """[d] a-priori bound on |phi_gpu - Shapley| of kernelshap_tree_kernel with link "logit_model"
    on a fully enumerated design (where the WLS solution IS the Shapley vector), M = leaf_mass(ens):

        i < d - 1:  sum_s |A_is| (T + n_bg + S + 8) u M
        i = d - 1:  the sum of the others' bounds + (2 T + ceil(n_bg / 256) + 11) u M  (delta's)

    A coalition value f_s is a mean over n_bg background rows of margins that are each base + T
    leaves, (T + n_bg) additions in whatever order with partial sums of at most M; y_s = f_s - f0
    goes through a dot product with row i of A of S terms in whatever order (S); 8 covers the fp32
    rounding of A, the 1 / n_bg, the subtraction of f0 and the A z_M delta correction.  It needs
    nothing but the model, and it is loose: M assumes every tree contributes its largest leaf with
    one sign.  ``kernelshap_tree_bound`` follows the kernel's sums with the magnitudes the case
    really has and is the one the tests assert; they also assert that it is the tighter one."""
    T = ens.n_trees
    M = leaf_mass(ens)
    b = np.empty(A.shape[0] + 1)
    b[:-1] = np.abs(A).sum(1) * (T + n_bg + A.shape[1] + 8) * U * M
    b[-1] = b[:-1].sum() + (2 * T + -(-n_bg // 256) + 11) * U * M
    return b


def kernelshap_tree_bound(Xs, Bs, ens, Z, A, zM, parts: int) -> dict:
    """Bound on |phi_gpu - Shapley| [E, d] and on |delta_gpu - delta| [E] for kernelshap_tree_kernel
    (link "logit_model", every proper coalition in the design Z), from the kernel's own sums.

    Magnitudes, all exact (fp64): G = the largest |partial sum| base + leaf_1 + ... + leaf_k over
    every row the kernel evaluates for this explanation (hybrids, background rows, x) and every k;
    y_s = f_s - f0, delta = fx - f0; W_i = sum_s |A_is| |y_s|; |A_i| = sum_s |A_is|; Az = A z_M.

    margin of one row     base (passed as fp32: 1) + T leaves added in tree order (T): (T + 1) u G
    f_s                   n_bg margins added one after the other (n_bg), times the rounded
                          1 / n_bg (2): (T + n_bg + 3) u G
    f0                    per thread rows b, b + 256, ..., a 6-level butterfly, 4 wave sums, times
                          1 / n_bg: (T + 1 + ceil(n_bg / 256) + 6 + 3 + 2) u G
    y_s                   err(f_s) + err(f0) + u |y_s| (the subtraction)
                          = E_y + u |y_s|,  E_y = (2 T + n_bg + ceil(n_bg / 256) + 15) u G
    sum_s A_is y_s        A rounded to fp32 (1); 8 threads per feature, each at most S_pad / 32
                          float4 steps of 4 chained fused multiply-adds (S_pad / 8), 4 accumulators
                          joined (2), a 3-level butterfly (3), the parts summed in order (parts):
                          |A_i| E_y + (S_pad / 8 + parts + 7) u W_i   (the 7: 1 + 2 + 3 + y's own u)
    delta                 fx: (T + 1) u G; f0 as above; the subtraction:
                          E_d = (2 T + ceil(n_bg / 256) + 13) u G + u |delta|
    phi_i, i < d - 1      minus fp32(Az_i) * delta (rounding of Az, the product) and the
                          subtraction:  |Az_i| (E_d + 2 u |delta|) + u (W_i + |Az_i delta|)
    phi_{d-1}             delta - (phi_0 + ... + phi_{d-2}) in fp32, d roundings of partial sums of
                          at most |delta| + sum |phi_i|: the sum of the others' bounds + E_d
                          + d u (|delta| + sum_i |phi_i|)

    First order in u; the result is scaled by 1.01 for the higher orders and for the fp64 error of
    the host's WLS solve (on exact coalition values A reproduces brute-force Shapley to a few
    1e-11 at worst, 256 trees; the tests assert 1e-10 on every case they run).
    Returns {"phi": [E, d], "delta": [E], "shapley": the WLS solution on exact values [E, d]}."""
    Xs = np.asarray(Xs, np.float32)
    Bs = np.asarray(Bs, np.float32)
    E, d = Xs.shape
    nb, T = len(Bs), ens.n_trees
    S = Z.shape[0]
    S_pad = (S + 31) // 32 * 32
    zb = Z.astype(bool)
    leaf = ens.leaf.astype(np.float64)
    A1 = np.abs(A).sum(1)
    Az = A @ zM
    cb = -(-nb // 256)
    out = {"phi": np.empty((E, d)), "delta": np.empty(E), "shapley": np.empty((E, d))}

    def partials(R):  # margins [n] and the largest |partial sum| over rows and prefixes
        v = np.take_along_axis(leaf, leaf_index(R, ens), axis=1)             # [T, n]
        ps = ens.base_margin + np.cumsum(v, axis=0)
        return ps[-1], max(abs(ens.base_margin), float(np.abs(ps).max()))

    mb, Gb = partials(Bs)
    f0 = mb.mean()
    for e in range(E):
        hyb = np.where(zb[:, None, :], Xs[e][None, None, :], Bs[None, :, :]).reshape(-1, d)
        mh, Gh = partials(hyb)
        mx, Gx = partials(Xs[e:e + 1])
        G = max(Gb, Gh, Gx)
        y = mh.reshape(S, nb).mean(1) - f0
        delta = float(mx[0] - f0)
        W = np.abs(A) @ np.abs(y)
        phi = np.empty(d)
        phi[:-1] = A @ y - Az * delta
        phi[-1] = delta - phi[:-1].sum()
        E_y = (2 * T + nb + cb + 15) * U * G
        E_d = (2 * T + cb + 13) * U * G + U * abs(delta)
        b = np.empty(d)
        b[:-1] = (A1 * E_y + (S_pad // 8 + parts + 7) * U * W + np.abs(Az) * (E_d + 2 * U * abs(delta))
                  + U * (W + np.abs(Az * delta)))
        b[-1] = b[:-1].sum() + E_d + d * U * (abs(delta) + np.abs(phi[:-1]).sum())
        out["phi"][e], out["delta"][e], out["shapley"][e] = 1.01 * b, 1.01 * E_d, phi
    return out


# ---------------------------------------------------------------------------------------------
# shared cases and the assertion every comparison goes through
# ---------------------------------------------------------------------------------------------
def oracle_case(depth: int, d: int, T: int = 12, n_bg: int = 9, E: int = 3):
    """(ens, Xs, Bs): a random ensemble with pass-through nodes and random rows.  With d < depth a
    root-to-leaf path of ``depth`` split nodes must repeat a feature: the forced-side rule decides."""
    seed = 100 * depth + d
    return (random_ensemble(d, depth, T, seed),) + random_rows(d, E, n_bg, seed + 1)


def tie_case(d: int = 6, depth: int = 4, T: int = 12, n_bg: int = 9, E: int = 4, seed: int = 77):
    """(ens, Xs, Bs) with a third of the thresholds sitting exactly on row values."""
    Xs, Bs = random_rows(d, E, n_bg, seed + 1)
    return plant_ties(random_ensemble(d, depth, T, seed), Xs, Bs, seed + 2), Xs, Bs


def assert_within(got, want, bound, what: str) -> float:
    """|got - want| <= bound elementwise; prints and returns the largest error / bound."""
    got, want, bound = (np.asarray(v, np.float64) for v in (got, want, bound))
    err = np.abs(got - want)
    ratio = float(np.max(err / np.maximum(bound, np.finfo(np.float64).tiny))) if err.size else 0.0
    print(f"[tree-bound] {what}: max error/bound = {ratio:.3g}")
    assert np.all(err <= bound), f"{what}: error exceeds the derived bound {ratio:.3g} times"
    return ratio


def assert_phi_exact(phi, Xs, Bs, ens, what: str, stats: dict | None = None, oracle=None) -> dict:
    """phi (a device result, or a mutant's) against brute-force Shapley within phi_bound."""
    st = stats if stats is not None else walk_stats(Xs, Bs, ens)
    want = brute_force_shapley(Xs, Bs, ens) if oracle is None else oracle
    assert_within(phi, want, phi_bound(st["S"], ens.n_trees, len(Bs), ens.depth), what)
    return st
