"""Interventional TreeSHAP (GBDT family explainer): the numpy oracle of treeshap.hip's algorithm
against brute-force exact Shapley values, efficiency, and agreement with exact (fully
enumerated) KernelSHAP on the margin -- two independent algorithms, one answer.  Also the helpers
the device tests stand on (tests/_tree_cases.py): its oracles agree, its cases reach the branches
they claim, its assertions reject three mutants of the walk; and the explainers' host validation."""
import itertools
import math

import numpy as np
import pytest

from fraud_detection_amd.models.explainers import (
    KernelExplainer, _margins_from_bits, cached_design, kernelshap_tree_reference, tree_direction_bits,
    treeshap_reference,
)

import _tree_cases as TC
from _tree_cases import random_ensemble  # noqa: F401  (test_scripts.py imports it from this module)


def exact_shapley(Xs, Bs, ens):
    """Brute force over all 2^d coalitions of v(S) = mean_b margin(x_S, z_~S)."""
    E, d = Xs.shape
    masks = np.array(list(itertools.product([0, 1], repeat=d)), bool)  # [2^d, d]
    phi = np.zeros((E, d))
    w = {s: math.factorial(s) * math.factorial(d - s - 1) / math.factorial(d) for s in range(d)}
    for e in range(E):
        hyb = np.where(masks[:, None, :], Xs[e][None, None, :], Bs[None, :, :])  # [2^d, nb, d]
        m = _margins_from_bits(tree_direction_bits(hyb.reshape(-1, d), ens), ens).astype(np.float64)
        v = m.reshape(len(masks), -1).mean(1)
        idx = {tuple(mk): i for i, mk in enumerate(masks)}
        for i in range(d):
            for k, mk in enumerate(masks):
                if mk[i]:
                    continue
                with_i = mk.copy()
                with_i[i] = True
                phi[e, i] += w[int(mk.sum())] * (v[idx[tuple(with_i)]] - v[k])
    return phi


@pytest.mark.parametrize("d,depth,T,seed", [(4, 3, 6, 0), (6, 5, 8, 1), (7, 4, 12, 2), (5, 5, 20, 3)])
def test_treeshap_equals_brute_force_shapley(d, depth, T, seed):
    ens = random_ensemble(d, depth, T, seed)
    rng = np.random.default_rng(seed + 10)
    Xs = rng.normal(size=(3, d)).astype(np.float32)
    Bs = rng.normal(size=(5, d)).astype(np.float32)
    phi, fx, f0 = treeshap_reference(Xs, Bs, ens)
    np.testing.assert_allclose(phi, exact_shapley(Xs, Bs, ens), atol=1e-6)  # brute force sums fp32 margins
    np.testing.assert_allclose(phi.sum(1), fx - f0, atol=1e-6)  # efficiency (fx, f0: fp32 tree sums)


def test_treeshap_matches_exact_kernelshap_on_the_margin():
    """KernelSHAP with every coalition enumerated (d = 8: 254 <= nsamples) is exact Shapley too."""
    d = 8
    ens = random_ensemble(d, 5, 15, 7)
    rng = np.random.default_rng(8)
    Xs = rng.normal(size=(4, d)).astype(np.float32)
    Bs = rng.normal(size=(6, d)).astype(np.float32)
    Z, _, A, zM = cached_design(d, 4096, 0)
    assert Z.shape[0] == 2 ** d - 2
    phi_k, _, _ = kernelshap_tree_reference(Xs, Bs, ens, Z, A, zM, link="logit_model")
    phi_t, _, _ = treeshap_reference(Xs, Bs, ens)
    np.testing.assert_allclose(phi_t, phi_k, atol=1e-6)


def test_tree_explainer_cpu_path_on_raw_rows():
    from fraud_detection_amd.models.explainers import TreeExplainer, _standardize

    d = 6
    ens = random_ensemble(d, 4, 10, 4)
    rng = np.random.default_rng(5)
    mean, scale = rng.normal(size=d) * 10, rng.uniform(0.5, 3, d)
    B = (rng.normal(size=(7, d)) * scale + mean).astype(np.float32)
    X = (rng.normal(size=(3, d)) * scale + mean).astype(np.float32)
    te = TreeExplainer(ens, mean, scale, B, device="cpu")
    phi, fx, f0 = te.explain(X)
    ref = treeshap_reference(_standardize(X, mean, scale), _standardize(B, mean, scale), ens)
    np.testing.assert_allclose(phi, ref[0], atol=1e-12)
    assert f0 == pytest.approx(te.expected_value)
    np.testing.assert_allclose(phi.sum(1), fx - f0, atol=1e-6)


# ---------------------------------------------------------------------------------------------
# the helpers the device tests stand on (tests/_tree_cases.py): oracles agree, cases cover what
# they claim, and the assertions the device goes through reject three mutants of the walk
# ---------------------------------------------------------------------------------------------
def _as_device(phi):
    """What a correct kernel would hand back at best: the exact values rounded to fp32."""
    return phi.astype(np.float32).astype(np.float64)


@pytest.mark.parametrize("depth,d", [(1, 2), (3, 2), (5, 3), (4, 8)])
def test_oracles_agree(depth, d):
    ens, Xs, Bs = TC.oracle_case(depth, d)
    st = TC.walk_stats(Xs, Bs, ens)
    bf = TC.brute_force_shapley(Xs, Bs, ens)
    np.testing.assert_allclose(st["phi"], bf, atol=1e-14)
    np.testing.assert_allclose(st["phi"], treeshap_reference(Xs, Bs, ens)[0], atol=1e-14)
    np.testing.assert_allclose(bf, exact_shapley(Xs, Bs, ens), atol=1e-6)
    assert np.all(np.abs(st["phi"]) <= st["S"] + 1e-15)
    np.testing.assert_allclose(st["phi"].sum(1), st["fx"] - st["f0"], atol=1e-13)  # exact efficiency
    np.testing.assert_allclose(st["fx"], treeshap_reference(Xs, Bs, ens)[1], atol=1e-6)


@pytest.mark.parametrize("depth", [1, 2, 3, 4, 5])
def test_disagree_case_reaches_every_weight(depth):
    ens, Xs, Bs = TC.disagree_case(depth)
    st = TC.assert_phi_exact(_as_device(TC.brute_force_shapley(Xs, Bs, ens)), Xs, Bs, ens, f"disagree depth {depth}")
    assert st["ab"] == TC.all_ab(depth)
    assert st["forced_x"] == st["forced_z"] == st["pass_through"] == 0
    assert np.all(st["phi"][:, -1] == 0) and np.all(st["S"][:, -1] == 0)  # the feature x and z share


@pytest.mark.parametrize("depth,d", [(depth, d) for depth in range(2, 6) for d in (2, 3) if d < depth])
def test_oracle_cases_force_both_sides(depth, d):
    ens, Xs, Bs = TC.oracle_case(depth, d)
    st = TC.walk_stats(Xs, Bs, ens)
    assert st["forced_x"] > 0 and st["forced_z"] > 0 and st["pass_through"] > 0 and st["split"] > 0


def test_lds_boundary_follows_the_launcher_rule():
    for d, depth, want in ((30, 5, 129), (8, 5, 216)):
        T = TC.treeshap_lds_boundary(d, depth)
        assert T == want
        assert (d * 256 + T + T * (2 << depth)) * 4 <= 65536 - 1024 < (d * 256 + (T + 1) * (1 + (2 << depth))) * 4


def test_kernelshap_bound_helper_on_the_host_path():
    """The tree KernelSHAP bound's own Shapley vector (WLS on exact coalition values over the
    enumerated design) is brute force's, the structural bound is the tighter one, and the host
    path -- fp32 margins in tree order, everything else fp64 -- sits well inside it."""
    from fraud_detection_amd.models.explainers import TreeKernelExplainer

    d, n_bg = 8, 6
    ens = random_ensemble(d, 5, 12, 41)
    Xs, Bs = TC.random_rows(d, 2, n_bg, 42)
    tk = TreeKernelExplainer(ens, np.zeros(d), np.ones(d), Bs, nsamples=4096, link="logit_model", device="cpu")
    assert tk.nsamples == 2 ** d - 2
    kb = TC.kernelshap_tree_bound(Xs, Bs, ens, tk.Z, tk.A, tk.zM, 4)
    brute = TC.brute_force_shapley(Xs, Bs, ens)
    np.testing.assert_allclose(kb["shapley"], brute, rtol=0, atol=1e-10)
    assert np.all(kb["phi"] <= TC.kernelshap_any_order_bound(tk.A, ens, n_bg)[None, :])
    TC.assert_within(tk.explain(Xs)[0], brute, kb["phi"], "host tree KernelSHAP vs brute force")


def _mutant_inputs(mutant):
    if mutant == "no_forced":
        return TC.oracle_case(5, 3)
    if mutant == "swap_w32":
        return TC.disagree_case(5)
    return TC.tie_case()


@pytest.mark.parametrize("mutant", TC.MUTANTS)
def test_device_assertions_reject_mutants(mutant):
    """The faithful walk, rounded to fp32 as a perfect kernel's output would be, passes the
    assertion the device tests make; each mutant of it, on the same inputs, fails it."""
    ens, Xs, Bs = _mutant_inputs(mutant)
    st = TC.walk_stats(Xs, Bs, ens)
    if mutant == "no_forced":
        assert st["forced_x"] > 0 and st["forced_z"] > 0
    elif mutant == "swap_w32":
        assert (3, 2) in st["ab"]
    else:
        assert st["ties_x"] > 0 and st["ties_z"] > 0
    oracle = TC.brute_force_shapley(Xs, Bs, ens)
    TC.assert_phi_exact(_as_device(st["phi"]), Xs, Bs, ens, f"faithful walk ({mutant} inputs)", st, oracle)
    bad = TC.walk_stats(Xs, Bs, ens, mutant)["phi"]
    with pytest.raises(AssertionError, match="exceeds the derived bound"):
        TC.assert_phi_exact(_as_device(bad), Xs, Bs, ens, f"mutant {mutant}", st, oracle)


def test_mutants_are_invisible_where_their_branch_is_not_reached():
    """Why the coverage assertions matter: on inputs that never reach the mutated branch the
    mutant computes the same values, so only a case that asserts its coverage can catch it."""
    ens, Xs, Bs = TC.disagree_case(3)  # no repeated feature, a + b <= 3, no row on a threshold
    st = TC.walk_stats(Xs, Bs, ens)
    for mutant in TC.MUTANTS:
        assert np.array_equal(TC.walk_stats(Xs, Bs, ens, mutant)["phi"], st["phi"])


# ---------------------------------------------------------------------------------------------
# host validation: a model whose features do not fit the data never reaches a kernel
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", ["TreeExplainer", "TreeKernelExplainer"])
def test_wrong_width_background_raises(cls):
    from fraud_detection_amd.models import explainers as EX

    ens = random_ensemble(8, 3, 6, 0, p_pass=0.0)
    ens.feat[0, 0] = 7
    make = getattr(EX, cls)
    make(ens, np.zeros(8), np.ones(8), np.zeros((4, 8), np.float32), device="cpu")  # matching width: fine
    with pytest.raises(ValueError) as ei:
        make(ens, np.zeros(5), np.ones(5), np.zeros((4, 5), np.float32), device="cpu")
    assert "8 features" in str(ei.value) and "5 columns" in str(ei.value)  # names both widths
    bad = random_ensemble(8, 3, 6, 0)
    bad.feat[1, 2] = -2
    with pytest.raises(ValueError, match="-2"):
        make(bad, np.zeros(8), np.ones(8), np.zeros((4, 8), np.float32), device="cpu")
    wide = random_ensemble(31, 3, 6, 0)
    with pytest.raises(ValueError, match="at most 30 features"):
        make(wide, np.zeros(31), np.ones(31), np.zeros((4, 31), np.float32), device="cpu")
