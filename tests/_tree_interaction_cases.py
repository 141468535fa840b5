"""Exact oracle, instrumented reference, mutants and derived error bounds for the SHAP interaction
values of the path-dependent game (csrc/kernels/treeshap_interact.hip).

Plain numpy, no GPU import; ensembles, covers and the game come from tests/_tree_cases.py and
tests/_tree_path_cases.py.  ``brute_force_interactions`` is the Shapley interaction index summed
over all 2^d coalitions of ``_tree_path_cases.game_value`` in fp64; ``interaction_stats`` is the
per-leaf form written out again (independently of models/explainers.py) with the absolute masses
the bounds scale with, and it can run as one of five mutants."""
from __future__ import annotations

import itertools
import math

import numpy as np

import _tree_cases as TC
import _tree_path_cases as PC

U = TC.U
TI_FRAC_BITS = 46    # kTIFracBits: the fixed-point unit is 2^(e - 46)
MUTANTS = ("no_merge", "phi_weight", "no_half", "sibling_frac", "ignore_default_left")


# ---------------------------------------------------------------------------------------------
# exact oracle: all 2^d coalitions, fp64
# ---------------------------------------------------------------------------------------------
def brute_force_interactions(Xs, ens, phi=None):
    """(inter [E, d, d], phi [E, d], margin [E], f0) in fp64.  Off the diagonal
        Phi_ij = sum_{S in N \\ {i, j}} |S|! (d - |S| - 2)! / (2 (d - 1)!) [v(S+ij) - v(S+i) - v(S+j) + v(S)]
    over ``_tree_path_cases.game_value``; the diagonal is phi_i - sum_{j != i} Phi_ij with phi from
    ``_tree_path_cases.brute_force`` (pass it in where it is at hand already)."""
    Xs = np.asarray(Xs, np.float32)
    E, d = Xs.shape
    if d > 10:
        raise ValueError("brute force enumerates 2^d coalitions: d <= 10")
    bphi, bfx, bf0 = PC.brute_force(Xs, ens) if phi is None else phi
    m = np.arange(1 << d)
    size = np.array([bin(i).count("1") for i in m])
    w = np.array([math.factorial(s) * math.factorial(d - s - 2) / (2 * math.factorial(d - 1))
                  for s in range(d - 1)] + [0.0, 0.0])
    inter = np.zeros((E, d, d))
    for e in range(E):
        v = np.array([PC.game_value(ens, Xs[e], int(S)) for S in m])
        for i in range(d):
            for j in range(i + 1, d):
                bi, bj = 1 << i, 1 << j
                S = m[(m & (bi | bj)) == 0]
                inter[e, i, j] = inter[e, j, i] = np.sum(w[size[S]] * (v[S | bi | bj] - v[S | bi] - v[S | bj] + v[S]))
        for i in range(d):
            inter[e, i, i] = bphi[e, i] - (inter[e, i].sum() - inter[e, i, i])
    return inter, bphi, bfx, bf0


# ---------------------------------------------------------------------------------------------
# instrumented per-leaf form (and its mutants)
# ---------------------------------------------------------------------------------------------
def interaction_stats(Xs, ens, mutant: str | None = None) -> dict:
    """The per-leaf form of the interaction index with the masses its fp32 error scales with.

    inter [E, d, d]   the interaction matrix (fp64): pair terms v (o_i - z_i) (o_j - z_j) W2_ij off the
                      diagonal, W2_ij = sum over S in M \\ {i, j} of |S|! (m - |S| - 2)! / (2 (m - 1)!)
                      prod_{k in S} o_k prod_{k in M \\ S \\ {i, j}} z_k; diagonal phi_i - sum_{j != i}
    S2 [E, d, d]      S_ij = sum over leaves of |v| (o_i + z_i) (o_j + z_j) W2_ij (0 on the diagonal)
    phi, S, fx, fx_abs, f0, f0_abs and the counters: ``_tree_path_cases.path_stats``'s
    e                 the smallest integer with max |leaf| <= 2^e (0 for an all-zero model)

    ``mutant``: "no_merge", "sibling_frac" and "ignore_default_left" as in path_stats (and passed
    on to it, so phi and the diagonal are the mutant's too); "phi_weight" weighs a pair's
    coefficient c_s by the phi form's s! (m - s - 1)! / m!; "no_half" drops the factor 1/2."""
    if mutant is not None and mutant not in MUTANTS:
        raise ValueError(mutant)
    st = PC.path_stats(Xs, ens, mutant if mutant in PC.MUTANTS else None)
    Xs = np.asarray(Xs, np.float32)
    D = ens.depth
    E, d = Xs.shape
    cover = np.asarray(ens.cover, np.float64)
    fact = [math.factorial(i) for i in range(D + 1)]
    inter, S2 = np.zeros((E, d, d)), np.zeros((E, d, d))

    def weight(s, m):
        if mutant == "phi_weight":
            return fact[s] * fact[m - s - 1] / fact[m]
        if mutant == "no_half":
            return fact[s] * fact[m - s - 2] / fact[m - 1]
        return fact[s] * fact[m - s - 2] / (2 * fact[m - 1])

    def right(t, k, x):
        if mutant == "ignore_default_left":
            f = int(ens.feat[t, k - 1])
            return f >= 0 and not (x[f] < ens.thr[t, k - 1])
        return PC._goes_right(ens, t, k, x)

    for t in range(ens.n_trees):
        for l in range(1 << D):
            heap = (1 << D) + l
            path, dead = [], False
            for j in range(D):
                k, c = heap >> (D - j), heap >> (D - j - 1)
                if ens.feat[t, k - 1] < 0:
                    dead = dead or bool(c & 1)
                else:
                    path.append((k, c))
            if dead or len(path) < 2:
                continue
            v = float(ens.leaf[t, l])
            fr = {}
            for k, c in path:
                src = c ^ 1 if mutant == "sibling_frac" else c
                fr[c] = cover[t, src] / cover[t, k] if cover[t, k] > 0 else 0.5
            key = (lambda k: k) if mutant == "no_merge" else (lambda k: int(ens.feat[t, k - 1]))
            col = (lambda g: int(ens.feat[t, g - 1])) if mutant == "no_merge" else (lambda g: g)
            M = sorted({key(k) for k, _ in path})
            m = len(M)
            for e in range(E):
                z = {g: 1.0 for g in M}
                o = {g: 1.0 for g in M}
                for k, c in path:
                    z[key(k)] *= fr[c]
                    if int(right(t, k, Xs[e])) != (c & 1):
                        o[key(k)] = 0.0
                for i, j in itertools.combinations(M, 2):
                    rest = [g for g in M if g != i and g != j]
                    W = 0.0
                    for s in range(m - 1):
                        for sub in itertools.combinations(rest, s):
                            term = weight(s, m)
                            for g in rest:
                                term *= o[g] if g in sub else z[g]
                            W += term
                    a, b = col(i), col(j)
                    if a == b:      # no_merge only: two nodes of one feature; stays on the diagonal
                        continue
                    val = v * (o[i] - z[i]) * (o[j] - z[j]) * W
                    mass = abs(v) * (o[i] + z[i]) * (o[j] + z[j]) * W
                    inter[e, a, b] += val
                    inter[e, b, a] += val
                    S2[e, a, b] += mass
                    S2[e, b, a] += mass
    idx = np.arange(d)
    inter[:, idx, idx] = st["phi"] - inter.sum(2)   # the diagonal is still 0 in the sum
    v = np.abs(np.asarray(ens.leaf, np.float64))
    vmax = float(v.max())
    e2 = 0
    if vmax > 0:
        mant, ex = math.frexp(vmax)
        e2 = ex - 1 if mant == 0.5 else ex
    st.update(inter=inter, S2=S2, e=e2)
    return st


# ---------------------------------------------------------------------------------------------
# launcher rule, restated
# ---------------------------------------------------------------------------------------------
def interactions_lds_boundary(d: int, depth: int) -> int:
    """Largest tree count T* for which launch_treeshap_interactions keeps leaves, split features
    and fractions in LDS.  Its rule: d (d + 1) / 2 int64 cells, T direction words and
    T (4 2^depth - 1) words of tree constants fit in 32768 - 1024 bytes (five workgroups per CU)."""
    room = 32768 - 1024 - (d * (d + 1) // 2) * 8
    return room // (4 * (4 << depth))


# ---------------------------------------------------------------------------------------------
# derived error bounds (u = 2^-24)
# ---------------------------------------------------------------------------------------------
def fixed_point_term(e: int, T: int, depth: int) -> float:
    """A cell receives at most one term per leaf, T 2^D of them, and every term is rounded to the
    unit 2^(e - 46) by one llrint: at most half a unit, 2^(e - 47), each.  The integer sum and the
    integer diagonal are exact; the one fp64 rounding of the result is 2^-53 of a value no larger
    than its mass and sits in the second-order allowance of the bounds below."""
    return T * (1 << depth) * 2.0 ** (e - TI_FRAC_BITS - 1)


def oracle_term(ens, d: int) -> float:
    """The brute-force oracle's own fp64 error, per entry.  G = |base| + sum_t max |leaf| bounds
    every game value.  ``game_value`` averages over D levels, each two quotients, two products and
    an addition (5 D roundings of at most a tree's largest leaf), sums the trees with an exact fsum
    and adds the base (1): |err v(S)| <= (5 D + 1) 2^-53 G.  A bracket v(S+ij) - v(S+i) - v(S+j) +
    v(S) carries four such errors and 3 roundings of partial sums of at most 4 G; the weights sum
    to 1/2; numpy's sum over the 2^(d-2) subsets adds at most 2^(d-2) roundings of
    sum |w bracket| <= 2 G.  In all ((20 D + 4 + 12) / 2 + 2^(d-1)) 2^-53 G =
    (10 D + 8 + 2^(d-1)) 2^-53 G.  The figure used is twice that, (20 D + 16 + 2^d) 2^-53 G, which
    also covers phi's brute force on the diagonal (two-term brackets, weights summing to 1 over
    2^(d-1) subsets).  It matters only where the mass is 0: at depth 1 the exact off-diagonal is 0
    and the kernel returns 0, while the second difference a - b - a + b leaves noise of 1e-17."""
    return (20 * ens.depth + 16 + 2 ** d) * 2.0 ** -53 * TC.leaf_mass(ens)


def pair_bound(S2, e: int, T: int, depth: int, oracle: float = 0.0):
    """|Phi_ij gpu - exact| <= (5 D + 3) u S_ij + T 2^D 2^(e - 47) + oracle, off the diagonal.

    One leaf's pair term is v (o_i - z_i) (o_j - z_j) W2, W2 = sum_s w2(s, m) c_s a sum of
    non-negative products, so its relative error is at most the roundings on the longest chain into
    it.  A monomial of the whole term holds at most D edge fractions, each an fp64 quotient rounded
    to fp32 once (D); merging repeated features costs at most D - 1 multiplications (D - 1); the
    polynomial prod_(k != i, j) (z_k + o_k y) has at most D - 2 factors at a multiply and an add per
    coefficient (2 (D - 2)); w2 is exact small integers with one division (1), its product with the
    coefficient (1), the sum over s (at most D - 1 additions).  The two differences o - z are one
    subtraction each (2): their absolute error is what z's relative error leaves, which is why the
    mass S_ij of interaction_stats carries (o + z), not |o - z|.  Three products join v, the two
    differences and W2 (3).  Together D + D - 1 + 2 D - 4 + 2 + D - 1 + 2 + 3 = 5 D + 1, each at
    most u of |v| (o_i + z_i) (o_j + z_j) W2; 2 more cover the second-order terms.  The sum over
    leaves is exact integer arithmetic after one llrint per term (``fixed_point_term``), and the
    fp64 output holds it rounded once.  ``oracle`` is the comparison value's own error
    (``oracle_term`` against brute force, 0 against nothing)."""
    return (5 * depth + 3) * U * np.asarray(S2, np.float64) + fixed_point_term(e, T, depth) + oracle


def phi_cell_bound(S, e: int, T: int, depth: int):
    """|sum of the phi_i cell - exact| <= (5 D + 3) u S_i + T 2^D 2^(e - 47): the chain of
    ``_tree_path_cases.phi_bound`` (5 D + 1 roundings into one leaf's term, 2 for second order)
    without its summation chain -- the cells are added in integers."""
    return (5 * depth + 3) * U * np.asarray(S, np.float64) + fixed_point_term(e, T, depth)


def phi_bound(S, e: int, T: int, depth: int):
    """The kernel's fp32 ``phi`` output: the cell's bound and one rounding to fp32 (|phi_i| <= S_i)."""
    return phi_cell_bound(S, e, T, depth) + U * np.asarray(S, np.float64)


def inter_bound(S2, S, e: int, T: int, depth: int, oracle: float = 0.0):
    """[E, d, d]: ``pair_bound`` off the diagonal; on it the phi cell's bound plus the row's pair
    bounds (Phi_ii = phi_i - sum_{j != i} Phi_ij, formed exactly in integers) -- the oracle's
    diagonal is formed in the same way, so its term enters d times there.  A pair that no leaf
    carries has no cell error at all, but is held to the fixed-point term all the same."""
    S2 = np.asarray(S2, np.float64)
    d = S2.shape[-1]
    b = pair_bound(S2, e, T, depth, oracle)
    idx = np.arange(d)
    b[..., idx, idx] = 0.0
    diag = phi_cell_bound(S, e, T, depth) + oracle + b.sum(-1)
    b[..., idx, idx] = diag
    return b


def fp64_bound(S2, S, T: int, depth: int, oracle: float = 0.0):
    """[E, d, d] bound on an fp64 evaluation of the per-leaf form (models/explainers.
    treeshap_interactions_reference, or interaction_stats itself) against an exact value: the
    5 D + 3 roundings of ``pair_bound``'s chain and the T 2^D additions of the sum over leaves, at
    2^-53 each, of the mass; the diagonal phi_i - sum_{j != i} Phi_ij takes the phi term (same
    count, mass S_i), the row's pair bounds and d more roundings of S_i + sum_j S_ij."""
    S2, S = np.asarray(S2, np.float64), np.asarray(S, np.float64)
    d = S2.shape[-1]
    n = (T * (1 << depth) + 5 * depth + 3) * 2.0 ** -53
    b = n * S2 + oracle
    idx = np.arange(d)
    b[..., idx, idx] = 0.0
    diag = n * S + oracle + b.sum(-1) + d * 2.0 ** -53 * (S + S2.sum(-1))
    b[..., idx, idx] = diag
    return b


def row_sum_bound(inter_abs_row, phi_abs, d: int, e: int):
    """|inter.sum(2) - phi_out|.  Row i of the integer matrix sums EXACTLY to the phi_i cell, and an
    entry below 2^53 units = 2^(e + 7) converts to fp64 exactly (asserted on the row's mass
    sum_j |Phi_ij|).  What is left: the d - 1 fp64 additions of the test's own sum and the fp64
    step of phi's conversion, d roundings of at most the row's mass, and the single fp32 rounding
    of phi."""
    mass = np.asarray(inter_abs_row, np.float64)
    assert np.all(mass < 2.0 ** (e + 7)), "an entry may exceed 2^53 units: its conversion would round"
    return d * 2.0 ** -53 * mass + U * np.asarray(phi_abs, np.float64)


fx_bound = PC.fx_bound
f0_bound = PC.f0_bound
assert_within = TC.assert_within
