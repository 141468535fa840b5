"""CPU-side proof obligations of the linear KernelSHAP oracle (tests/_ks_cases.py): the exact
oracles agree with each other, the operand oracle is bit-faithful to what the host uploads and stays
within operand_bound of the exact one, the faithful emulation of both kernels stays within
device_bound on every run of the GPU list, every planted mutant leaves it on a named run, and the
list reaches every template instantiation and path by the launchers' own formulas."""
import numpy as np
import pytest
import torch

import _ks_cases as K
from fraud_detection_amd.models import explainers as EX
from fraud_detection_amd.ops import kernelshap as OK

RUNS = {r.id: r for r in K.all_runs()}
ENUM_D = (2, 3, 8, 9, 11)


def _wls_tolerance(d, phi):
    """What the 1e-12 ridge of wls_operator and its fp64 solve may cost: (G + r I)^-1 = G^-1 -
    r G^-2 + ..., so phi_{<d} moves by at most r |G^-1|_2 |phi|_2, and the solve itself by
    cond(G) 2^-52 per equation (d of them); the last feature collects all d - 1 differences."""
    Z, w, _, _ = EX.cached_design(d)
    Zf = Z.astype(np.float64)
    Xm = Zf[:, :-1] - Zf[:, -1:]
    G = (Xm.T * w[None, :]) @ Xm
    sv = np.linalg.svd(G, compute_uv=False)
    return d * (1e-12 / sv[-1] + d * 2.0 ** -52 * sv[0] / sv[-1]) * np.linalg.norm(phi, axis=1, keepdims=True)


@pytest.mark.parametrize("link", K.LINKS)
@pytest.mark.parametrize("d", ENUM_D)
def test_brute_force_equals_wls_on_enumerated_designs(d, link):
    case = K.random_case(d, 7, 2, 500 + d)
    Z, _, A, zM = case.design()
    assert Z.shape[0] == 2 ** d - 2                              # every proper coalition
    K.assert_unclamped(case)                                       # neither clip binds: one game for both
    phi, fx, f0 = K.brute_force_shapley(case.X, case.B, case.a, case.bias, link)
    ref = EX.kernelshap_reference(case.X, case.a, case.bias, case.B, Z, A, zM, link)
    tol = _wls_tolerance(d, phi)
    assert tol.max() < 2e-10                                       # "about 1e-11": the ridge, not a free knob
    K.assert_within(ref[0], phi, tol + np.zeros_like(phi), f"wls vs brute force d={d} {link}")
    np.testing.assert_allclose(ref[1], fx, rtol=0, atol=1e-13 * (1 + np.abs(fx).max()))
    assert abs(ref[2] - f0) <= 1e-13 * (1 + abs(f0))
    np.testing.assert_allclose(phi.sum(1), fx - f0, rtol=0, atol=1e-12 * (1 + np.abs(phi).sum()))   # efficiency


@pytest.mark.parametrize("d", ENUM_D)
def test_brute_force_equals_closed_form_for_log_odds(d):
    case = K.random_case(d, 13, 3, 520 + d)
    phi, fx, f0 = K.brute_force_shapley(case.X, case.B, case.a, case.bias, "logit_model")
    cphi, cfx, cf0 = K.closed_form(case.X, case.B, case.a, case.bias)
    # 2^d terms of magnitude <= max |v| summed in fp64
    tol = 2.0 ** d * 2.0 ** -52 * (np.abs(fx).max() + abs(f0) + np.abs(cphi).sum())
    np.testing.assert_allclose(phi, cphi, rtol=0, atol=tol)
    np.testing.assert_allclose(fx, cfx, rtol=0, atol=tol)
    assert abs(f0 - cf0) <= tol


def test_pairing_of_enumerated_and_sampled_designs():
    """The facts the case list leans on: enumerated designs pair perfectly (127 / 255 / 1023 pairs),
    the sampled d = 30 design has bases without a complement (the zero-A-column path) and 33 tiles."""
    for d, pairs in ((8, 127), (9, 255), (11, 1023)):
        base, comp = OK.complement_pairs(EX.cached_design(d)[0])
        assert len(base) == pairs and np.all(comp >= 0)
    Z = EX.cached_design(30)[0]
    base, comp = OK.complement_pairs(Z)
    assert np.sum(comp < 0) > 0 and (len(base) + 31) // 32 == 33 and Z.shape[0] > len(base)


@pytest.mark.parametrize("paired", [False, True])
@pytest.mark.parametrize("key", [("random", 8, 37, 3, 137), ("random", 30, 100, 1, 430), ("regime", "exp_overflow", 0)])
def test_operands_reproduce_the_uploaded_design_bit_for_bit(key, paired):
    case = K.case_of(key)
    ke = case.explainer("identity")
    t = OK._device_design(ke, torch.device("cpu"), paired)
    ops = K.operands(case, False)
    assert np.array_equal(t["bg"].numpy().view(np.uint32), ops["W"].view(np.uint32))
    assert np.array_equal(t["cb"].numpy().view(np.uint32), ops["cb"].view(np.uint32))
    assert np.array_equal(t["a"].numpy().view(np.uint32), ops["a32"].view(np.uint32))
    # hi + lo carries 16 of u's 24 bits; T_b - L_b(z) is L_b(1 - z) from the same halves, exactly
    assert np.all(np.abs(ops["op"] - ops["u"].astype(np.float64)) <= K.UB * K.UB * np.abs(ops["u"]))
    Z = case.design()[0].astype(np.float64)
    d = case.d
    acc = np.einsum("ebk,sk->ebs", ops["op"][:, :, :d], Z) + ops["op"][:, :, 31][:, :, None]
    accc = np.einsum("ebk,sk->ebs", ops["op"][:, :, :d], 1.0 - Z) + ops["op"][:, :, 31][:, :, None]
    np.testing.assert_allclose(ops["T"][:, :, None] - acc, accc, rtol=0, atol=1e-12 * np.abs(acc).max())


@pytest.mark.parametrize("rid", sorted({(r.key, r.link) for r in RUNS.values()}, key=str),
                         ids=lambda t: "-".join(str(k) for k in t[0]) + "-" + t[1])
def test_operand_oracle_within_operand_bound(rid):
    key, link = rid
    o = K.oracles(key, link)
    case = K.case_of(key)
    # sampled designs: kernelshap_reference solves with the ridge; its cost is far below the bound
    K.assert_outputs_within(o["at"], o["exact"], o["ob"], f"operands vs exact {case.name} {link}")


@pytest.mark.parametrize("rid", sorted(RUNS))
def test_faithful_emulation_within_device_bound(rid):
    r = RUNS[rid]
    case = K.case_of(r.key)
    em = K.emulate(case, r.link, r.paired, r.parts)
    assert np.all(np.isfinite(em["phi"]))
    K.assert_outputs_within(em, K.oracles(r.key, r.link)["at"], K.bound_of(r), f"emulation {rid}")
    if case.clamped:
        K.assert_outputs_within(em, K.oracles(r.key, r.link)["at"], K.bound_of(r, True), f"emulation, clamp taken {rid}")


@pytest.mark.parametrize("mutant", K.MUTANTS)
def test_every_mutant_leaves_the_bound_on_its_named_run(mutant):
    assert K.MUTANT_WITNESS[mutant]
    for rid in K.MUTANT_WITNESS[mutant]:
        r = RUNS[rid]
        em = K.emulate(K.case_of(r.key), r.link, r.paired, r.parts, mutant=mutant)
        err = np.abs(em["phi"] - K.oracles(r.key, r.link)["at"]["phi"])
        ratio = float(np.nanmax(err / K.bound_of(r)["phi"])) if np.all(np.isfinite(err)) else np.inf
        print(f"[ks-mutant] {mutant} on {rid}: error/bound = {ratio:.3g}")
        assert ratio > 1.0, f"{mutant} passes on {rid}"


def test_mutants_exist_only_where_named():
    with pytest.raises(ValueError):
        K.emulate(K.case_of(("random", 2, 5, 3, 302)), "identity", False, 1, mutant="nope")
    assert set(K.MUTANT_WITNESS) == set(K.MUTANTS)


def test_gpu_list_reaches_every_instantiation_and_path():
    cov = K.coverage(K.gpu_runs())
    every = {(ntb, ngl, lg) for ntb in range(1, 5) for ngl in range(1, 5) for lg in (False, True)}
    print(f"[ks-coverage] unpaired {len(cov['unpaired'])}/32, paired {len(cov['paired'])}/32, "
          f"remainders {cov['rem_at']}, parts {sorted(cov['parts'])}, null rows {sorted(cov['nulls'])}")
    assert cov["unpaired"] == every and cov["paired"] == every
    for ntb in range(1, 5):
        assert cov["rem_at"][ntb] == {0, 1, 2, 3}, (ntb, cov["rem_at"][ntb])
    assert cov["parts"] == set(range(1, 9))
    assert {7, 3, 0} <= cov["nulls"]
    nbg = {K.case_of(r.key).n_bg for r in K.gpu_runs()}
    assert min(nbg) == 1 and max(nbg) == 128
    for r in K.gpu_runs():                                         # the launch guards hold for every run
        assert 1 <= r.parts <= K.n_tiles_of(K.case_of(r.key), r.paired)
    widths = {K.case_of(r.key).d for r in K.gpu_runs()}
    assert {2, 3, 8, 9, 11, 12, 17, 29, 30} <= widths


def test_regime_builder_refuses_a_case_outside_its_regime():
    for regime in K.REGIMES:
        for feature in (0, 7):
            K.assert_regime(K.regime_case(regime, feature), regime)
    mod = K.regime_case("moderate")
    for regime in ("pair_overflow", "exp_overflow", "tb_low", "high"):
        with pytest.raises(AssertionError):
            K.assert_regime(mod, regime)
    with pytest.raises(AssertionError):
        K.assert_regime(K.regime_case("high"), "moderate")
    with pytest.raises(AssertionError):
        K.assert_unclamped(K.clamp_case("near_one"))


def test_host_reference_takes_fx_from_the_logit():
    """link "logit": f(x) is the model's own logit (shap applies the link to the model output), not
    a probability clipped at 1 - 1e-12 (27.6); coalition values and f0 keep their clip, which the
    exact oracle reproduces through its clamp parameter."""
    case = K.clamp_case("wide_fx")
    Z, _, A, zM = case.design()
    phi, fx, f0 = EX.kernelshap_reference(case.X, case.a, case.bias, case.B, Z, A, zM, "logit")
    lx = case.X.astype(np.float64) @ case.a[: case.d] + case.bias
    assert np.abs(lx).min() > 28.0
    np.testing.assert_allclose(fx, lx, rtol=0, atol=1e-12)
    np.testing.assert_allclose(phi.sum(1), fx - f0, rtol=0, atol=1e-9)
    bphi, bfx, bf0 = K.brute_force_shapley(case.X, case.B, case.a, case.bias, "logit", K.CLAMP_HOST)
    K.assert_within(phi, bphi, _wls_tolerance(case.d, bphi) + np.zeros_like(bphi), "host reference vs brute force at the host clamp")
    np.testing.assert_allclose(bfx, lx, rtol=0, atol=1e-12)
    # the device's clamp is another game: 15.9 where the host has 27.6
    dphi = K.brute_force_shapley(case.X, case.B, case.a, case.bias, "logit", K.CLAMP_DEVICE)[0]
    assert np.abs(dphi - bphi).max() > 1.0
    # the generic path has only the probability: finite, and the same logit while fp64 resolves 1 - p
    near = K.clamp_case("near_one")
    fn = lambda R: torch.sigmoid(R.double() @ torch.from_numpy(near.a[: near.d]) + near.bias)  # noqa: E731
    fe = EX.FunctionKernelExplainer(fn, near.B, link="logit", device="cpu")
    lxn = near.X.astype(np.float64) @ near.a[: near.d] + near.bias
    np.testing.assert_allclose(fe.explain(near.X)[1], lxn, rtol=1e-4)


def test_choose_parts_edges():
    assert OK.choose_parts(0, 64, 256) == 1 and OK.choose_parts(-3, 64, 256) == 1
    assert OK.choose_parts(1, 1, 256) == 1 and OK.choose_parts(1, 3, 256) == 1      # one tile, < 4 tiles
    assert OK.choose_parts(1, 4, 256) == 1 and OK.choose_parts(1, 8, 256) == 2
    assert OK.choose_parts(1, 64, 256) == OK.MAX_PARTS == 8
    assert OK.choose_parts(64, 64, 256) == 4 and OK.choose_parts(256, 64, 256) == 1
    assert OK.choose_parts(10 ** 6, 64, 256) == 1
    for E in (1, 7, 64, 300):
        for tiles in (1, 4, 33, 128):
            p = OK.choose_parts(E, tiles, 256)
            assert 1 <= p <= 8 and p <= max(1, tiles // 4)


def test_complement_pairs_edges():
    # one coalition whose complement is absent
    b, c = OK.complement_pairs(np.array([[1, 0, 0]], np.uint8))
    assert b.tolist() == [0] and c.tolist() == [-1]
    # an odd count: 3 rows, one pair and one single; no row is its own complement
    Z = np.array([[1, 0, 0], [0, 1, 1], [0, 1, 0]], np.uint8)
    b, c = OK.complement_pairs(Z)
    assert b.tolist() == [0, 2] and c.tolist() == [1, -1]
    # d = 2: the two proper coalitions are each other's complement (one pair, Ppad = 32)
    Z2 = EX.cached_design(2)[0]
    b, c = OK.complement_pairs(Z2)
    assert len(Z2) == 2 and len(b) == 1 and c[0] >= 0
    # designs hold no duplicates, and every row lands in exactly one slot
    for d in (3, 12, 30):
        Zd = EX.cached_design(d)[0]
        assert len({z.tobytes() for z in Zd}) == len(Zd)
        b, c = OK.complement_pairs(Zd)
        assert np.array_equal(np.sort(np.r_[b, c[c >= 0]]), np.arange(len(Zd)))
        assert np.array_equal(Zd[c[c >= 0]], 1 - Zd[b[c >= 0]])
