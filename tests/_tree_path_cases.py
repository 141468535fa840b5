"""Exact oracle, instrumented reference, mutants and derived fp32 error bounds for path-dependent
TreeSHAP (csrc/kernels/treeshap_path.hip) and helpers for the node-cover kernel
(csrc/kernels/treecover.hip).

Plain numpy, no GPU import; ensembles come from tests/_tree_cases.py.  ``brute_force`` sums over all
2^d coalitions of the EXPVALUE game with its own recursive traversal in fp64, straight from the
stored covers; ``path_stats`` is the per-leaf form written out again with counters (what the inputs
reach) and the absolute masses the bounds scale with, and it can run as one of three mutants."""
from __future__ import annotations

import itertools
import math

import numpy as np

import _tree_cases as TC

U = TC.U
TP_THREADS = 256   # tree_explain.h kTreeThreads
MUTANTS = ("no_merge", "sibling_frac", "ignore_default_left")


# ---------------------------------------------------------------------------------------------
# ensembles with covers
# ---------------------------------------------------------------------------------------------
def count_cover(ens, rows) -> np.ndarray:
    """int64 [T, 2^(D+1)] rows per heap node: its own traversal (a NaN by default_left)."""
    rows = np.asarray(rows, np.float32)
    D = ens.depth
    out = np.zeros((ens.n_trees, 2 << D), np.int64)
    for t in range(ens.n_trees):
        for x in rows:
            k = 1
            out[t, k] += 1
            for _ in range(D):
                k = 2 * k + int(_goes_right(ens, t, k, x))
                out[t, k] += 1
    return out


def with_count_cover(ens, rows):
    return ens.with_cover(count_cover(ens, rows), "count")


def with_default_left(ens, seed: int, p: float = 0.5):
    """A copy with default_left set on a random half of the split nodes."""
    from dataclasses import replace

    rng = np.random.default_rng(seed)
    dl = ((rng.random(ens.feat.shape) < p) & (ens.feat >= 0)).astype(np.uint8)
    return replace(ens, default_left=dl)


def covered_case(depth: int, d: int, T: int = 6, n_bg: int = 40, E: int = 3):
    """(ens with count covers of the n_bg rows, Xs [E, d], Bs [n_bg, d])."""
    ens, Xs, Bs = TC.oracle_case(depth, d, T=T, n_bg=n_bg, E=E)
    return with_count_cover(ens, Bs), Xs, Bs


def covered_tie_case():
    ens, Xs, Bs = TC.tie_case(n_bg=40)
    return with_count_cover(ens, Bs), Xs, Bs


def _goes_right(ens, t: int, k: int, x) -> bool:
    f = int(ens.feat[t, k - 1])
    if f < 0:
        return False
    xv = x[f]
    if np.isnan(xv):
        return not (ens.default_left is not None and ens.default_left[t, k - 1] != 0)
    return not (xv < ens.thr[t, k - 1])


# ---------------------------------------------------------------------------------------------
# exact oracle: all 2^d coalitions of the EXPVALUE game, fp64, its own traversal
# ---------------------------------------------------------------------------------------------
def game_value(ens, x, S: int) -> float:
    """v(S) = base_margin + sum_t v_t(S): follow x at a split on a feature in S, else average the
    children by cover[child] / cover[node] (1/2 each at cover 0); a pass-through node goes left."""
    D = ens.depth
    cover = ens.cover

    def ev(t, k, level):
        if level == D:
            return float(ens.leaf[t, k - (1 << D)])
        f = int(ens.feat[t, k - 1])
        if f < 0:
            return ev(t, 2 * k, level + 1)
        if S >> f & 1:
            return ev(t, 2 * k + int(_goes_right(ens, t, k, x)), level + 1)
        c = cover[t, k]
        wl, wr = (cover[t, 2 * k] / c, cover[t, 2 * k + 1] / c) if c > 0 else (0.5, 0.5)
        return wl * ev(t, 2 * k, level + 1) + wr * ev(t, 2 * k + 1, level + 1)

    return ens.base_margin + math.fsum(ev(t, 1, 0) for t in range(ens.n_trees))


def brute_force(Xs, ens):
    """(phi [E, d], margin [E], f0) in fp64: Shapley values of ``game_value`` over all coalitions."""
    Xs = np.asarray(Xs, np.float32)
    E, d = Xs.shape
    if d > 10:
        raise ValueError("brute force enumerates 2^d coalitions: d <= 10")
    m = np.arange(1 << d)
    size = np.array([bin(i).count("1") for i in m])
    w = np.array([math.factorial(s) * math.factorial(d - s - 1) / math.factorial(d) for s in range(d)] + [0.0])
    phi = np.zeros((E, d))
    fx = np.zeros(E)
    f0 = 0.0
    for e in range(E):
        v = np.array([game_value(ens, Xs[e], int(S)) for S in m])
        for i in range(d):
            without = m[(m >> i & 1) == 0]
            phi[e, i] = np.sum(w[size[without]] * (v[without | (1 << i)] - v[without]))
        fx[e], f0 = v[-1], v[0]
    return phi, fx, f0


# ---------------------------------------------------------------------------------------------
# instrumented per-leaf reference (and its mutants)
# ---------------------------------------------------------------------------------------------
def path_stats(Xs, ens, mutant: str | None = None) -> dict:
    """models/explainers.treeshap_path_reference written out again with counters.

    phi [E, d]      the per-leaf form's attributions (fp64)
    S [E, d]        absolute mass sum over leaves of |v| (o_i + z_i) W_i, W_i the inner Shapley sum
                    (non-negative terms only): what the fp32 error of phi scales with
    fx [E], fx_abs [E]   fp64 margin of x and sum_t |leaf reached|
    f0, f0_abs      base + sum_t v_t(empty set), and |base| + sum_t sum_leaves |v| prod frac
    zero_cover      split nodes of cover 0 on the path of a live leaf (counted per leaf)
    repeats         live leaves whose path splits twice on one feature
    dead            leaves behind the right branch of a pass-through node
    max_m           most distinct features on one live path
    nan_default_left   (row, node) visits where x is NaN at a node whose default_left is set

    ``mutant``: "no_merge" treats every split node as a feature of its own (a repeated feature is
    not merged), "sibling_frac" takes the edge fraction from the sibling, "ignore_default_left"
    sends every NaN right."""
    if mutant is not None and mutant not in MUTANTS:
        raise ValueError(mutant)
    Xs = np.asarray(Xs, np.float32)
    D = ens.depth
    E, d = Xs.shape
    cover = np.asarray(ens.cover, np.float64)
    fact = [math.factorial(i) for i in range(D + 1)]
    st = {"zero_cover": 0, "repeats": 0, "dead": 0, "max_m": 0, "nan_default_left": 0}
    phi, S = np.zeros((E, d)), np.zeros((E, d))
    fx, fx_abs = np.full(E, ens.base_margin), np.zeros(E)
    f0, f0_abs = ens.base_margin, abs(ens.base_margin)

    def right(t, k, x):
        if mutant == "ignore_default_left":
            f = int(ens.feat[t, k - 1])
            return f >= 0 and not (x[f] < ens.thr[t, k - 1])
        return _goes_right(ens, t, k, x)

    for t in range(ens.n_trees):
        for e in range(E):  # the leaf x reaches
            k = 1
            for _ in range(D):
                f = int(ens.feat[t, k - 1])
                if f >= 0 and np.isnan(Xs[e][f]) and ens.default_left is not None and ens.default_left[t, k - 1]:
                    st["nan_default_left"] += 1
                k = 2 * k + int(_goes_right(ens, t, k, Xs[e]))
            v = float(ens.leaf[t, k - (1 << D)])
            fx[e] += v
            fx_abs[e] += abs(v)
        for l in range(1 << D):
            heap = (1 << D) + l
            path, dead = [], False
            for j in range(D):
                k, c = heap >> (D - j), heap >> (D - j - 1)
                if ens.feat[t, k - 1] < 0:
                    dead = dead or bool(c & 1)
                else:
                    path.append((k, c))
            if dead:
                st["dead"] += 1
                continue
            v = float(ens.leaf[t, l])
            fr = {}
            for k, c in path:
                src = c ^ 1 if mutant == "sibling_frac" else c
                if cover[t, k] > 0:
                    fr[c] = cover[t, src] / cover[t, k]
                else:
                    fr[c] = 0.5
                    st["zero_cover"] += 1
            wleaf = float(np.prod([fr[c] for _, c in path])) if path else 1.0
            f0 += v * wleaf
            f0_abs += abs(v) * wleaf
            if not path:
                continue
            key = (lambda k: k) if mutant == "no_merge" else (lambda k: int(ens.feat[t, k - 1]))
            M = sorted({key(k) for k, _ in path})
            m = len(M)
            st["repeats"] += int(len({int(ens.feat[t, k - 1]) for k, _ in path}) < len(path))
            st["max_m"] = max(st["max_m"], len({int(ens.feat[t, k - 1]) for k, _ in path}))
            for e in range(E):
                z = {g: 1.0 for g in M}
                o = {g: 1.0 for g in M}
                for k, c in path:
                    z[key(k)] *= fr[c]
                    if int(right(t, k, Xs[e])) != (c & 1):
                        o[key(k)] = 0.0
                for i in M:
                    rest = [g for g in M if g != i]
                    W = 0.0
                    for s in range(m):
                        for sub in itertools.combinations(rest, s):
                            term = fact[s] * fact[m - s - 1] / fact[m]
                            for g in rest:
                                term *= o[g] if g in sub else z[g]
                            W += term
                    fi = int(ens.feat[t, i - 1]) if mutant == "no_merge" else i
                    phi[e, fi] += v * (o[i] - z[i]) * W
                    S[e, fi] += abs(v) * (o[i] + z[i]) * W
    st.update(phi=phi, S=S, fx=fx, fx_abs=fx_abs, f0=float(f0), f0_abs=float(f0_abs))
    return st


# ---------------------------------------------------------------------------------------------
# launcher rules, restated
# ---------------------------------------------------------------------------------------------
def path_lds_boundary(d: int, depth: int) -> int:
    """Largest tree count T* for which launch_treeshap_path keeps leaves, split features and
    fractions in LDS: its rule is (d * 256 + T + T * (4 * 2^depth - 1)) * 4 <= 65536 - 1024."""
    words = (65536 - 1024) // 4
    return (words - d * TP_THREADS) // (4 << depth)


def cover_chunk(depth: int) -> int:
    """Trees per tree_cover launch: (32768 - 1024) // ((2 (2^D - 1) + 2^D) * 4 + 2^D * 8)."""
    return (32768 - 1024) // ((2 * ((1 << depth) - 1) + (1 << depth)) * 4 + (1 << depth) * 8)


# ---------------------------------------------------------------------------------------------
# derived error bounds (u = 2^-24)
# ---------------------------------------------------------------------------------------------
def phi_bound(S, T: int, depth: int):
    """|phi_gpu - phi_exact| <= (ceil(T 2^D / 256) + 32 + 3 + 5 D + 1 + 2) u S, elementwise.

    One leaf's term for feature i is v (o_i - z_i) W_i.  W_i is a sum of non-negative products, so
    its relative error is at most the number of roundings on the longest chain into it: every edge
    fraction is the fp64 quotient rounded to fp32 once and a monomial holds at most D of them (D);
    the merged z's cost at most D - 1 multiplications (D - 1); the polynomial prod_(j != i)
    (z_j + o_j y) takes D - 1 factors at a multiply and an add per coefficient (2 (D - 1)); the
    weight s! (m - s - 1)! / m! is exact small integers with one division (1), its product with the
    coefficient (1) and the sum over s (D - 1).  o_i - z_i is one subtraction (1), but z_i itself
    carries up to 2 D - 1 roundings and 1 - z_i cancels: its ABSOLUTE error is what z_i's relative
    error leaves, which is why the mass S of path_stats carries (o_i + z_i), not |o_i - z_i|.  Two
    more products, by W_i and by v (2).  Together 5 D + 1 roundings, each at most u of
    |v| (o_i + z_i) W_i.  The terms of one (row, feature) are then added in a fixed tree: thread
    ``tid`` owns the (tree, leaf) pairs tid, tid + 256, ... and adds them into its own LDS column
    one after the other (ceil(T 2^D / 256)); eight threads per feature add 32 columns each (32)
    and a 3-level butterfly joins them (3).  2 covers the second-order terms."""
    chain = -(-T * (1 << depth) // TP_THREADS)
    return (chain + 32 + 3 + 5 * depth + 1 + 2) * U * np.asarray(S, np.float64)


def fx_bound(fx_abs, T: int, base_margin: float):
    """treeshap_path.hip sums margin(x) exactly as treeshap.hip does: _tree_cases.fx_bound."""
    return TC.fx_bound(fx_abs, T, base_margin)


def f0_bound(f0_abs: float, T: int, depth: int) -> float:
    """f0 is computed on the host in fp64: D products per leaf and T 2^D additions, at 2^-53 each,
    of at most f0_abs; the kernel passes it through."""
    return (depth + T * (1 << depth) + 2) * 2.0 ** -53 * f0_abs


def efficiency_bound(S, fx_abs, f0_abs, T: int, depth: int, base_margin: float):
    """|sum_f phi_gpu - (fx_gpu - f0)| <= sum_f phi_bound + fx_bound + f0_bound: the exact values
    satisfy efficiency exactly."""
    return phi_bound(S, T, depth).sum(-1) + fx_bound(fx_abs, T, base_margin) + f0_bound(f0_abs, T, depth)


assert_within = TC.assert_within
