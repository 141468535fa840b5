"""kernelshap_linear_kernel and kernelshap_paired_kernel on the device against the two-stage oracle
of tests/_ks_cases.py: every (NTB, NGL, LOGITS) instantiation of both kernels, coalition parts 1..8,
the paired kernel's remainder-tile path at every NTB, design widths from d = 2 to d = 30, the logit
regimes around the shifted pair reciprocal, the "logit" link's clamps, determinism, the workspace and
the host-side guards.  Every tolerance is a derived bound (device_bound, operand_bound); the run list
is the one test_kernelshap_oracle.py proves complete and mutant-sensitive on the CPU."""
import numpy as np
import pytest
import torch

import _ks_cases as K
from fraud_detection_amd.models import explainers as EX

pytestmark = pytest.mark.gpu


def _pairs(runs):
    """[(unpaired run, paired run)] of a run list that holds every configuration for both kernels."""
    un = {(r.group, r.key, r.link, r.parts): r for r in runs if not r.paired}
    pa = {(r.group, r.key, r.link, r.parts): r for r in runs if r.paired}
    assert set(un) == set(pa)
    return [(un[k], pa[k]) for k in sorted(un, key=str)]


def _pid(p):
    return p[0].id.replace("-unpaired", "")


def _launch(dev, r, X=None, **kw):
    from fraud_detection_amd.ops.kernelshap import kernelshap

    case = K.case_of(r.key)
    ke = case.explainer(r.link, str(dev))
    Xd = torch.from_numpy(case.X if X is None else X).to(dev)
    phi, fx, f0 = kernelshap(Xd, ke, parts=r.parts, paired=r.paired, **kw)
    return {"phi": phi, "fx": fx, "f0": f0, "delta": fx - f0}, ke


def _check(dev, r, pow2=False):
    """One run against the operand oracle (device_bound), the exact oracle (+ operand_bound) and
    efficiency.  -> (device outputs, bound)."""
    case = K.case_of(r.key)
    got, _ = _launch(dev, r)
    assert np.all(np.isfinite(got["phi"])) and np.all(np.isfinite(got["fx"])) and np.isfinite(got["f0"])
    o, b = K.oracles(r.key, r.link), K.bound_of(r, pow2)
    tag = f"[{r.group}{'-taken' if pow2 else ''}]"
    K.assert_outputs_within(got, o["at"], b, f"{tag} device vs operands {r.id}")
    ref = "brute force" if case.d <= 11 else "kernelshap_reference"
    K.assert_outputs_within(got, o["exact"], b, f"{tag} device vs {ref} {r.id}", extra=o["ob"])
    K.assert_within(got["phi"].sum(1), got["delta"], K.efficiency_bound(got["phi"], got["fx"], got["f0"], case.d),
                    f"[{r.group}] efficiency {r.id}")
    return got, b


def _check_pair(dev, ru, rp, pow2=False):
    gu, bu = _check(dev, ru, pow2)
    gp, bp = _check(dev, rp, pow2)
    K.assert_outputs_within(gp, gu, bu, f"[{ru.group}{'-taken' if pow2 else ''}] paired vs unpaired {_pid((ru, rp))}", extra=bp)
    return gu, gp


@pytest.mark.parametrize("pair", _pairs(K.gpu_runs()), ids=_pid)
def test_kernels_match_the_oracles(dev, pair):
    """Instantiations (16 n_bg x 3 links at d = 8), parts and remainders (d = 8, 9, 11), widths
    (d = 2, 3) and sampled designs (d = 12, 17, 29, 30): both kernels, each against both oracles,
    and against each other within the sum of their bounds."""
    _check_pair(dev, *pair)


@pytest.mark.parametrize("pair", _pairs(K.regime_runs()), ids=_pid)
def test_logit_regimes(dev, pair):
    """Every regime of regime_case in both kernels, the extreme row on base and on complement
    columns (asserted by the builder).  Under exp2 overflow the fallback must keep the partner rows'
    sigmas: the mutant that drops them leaves this very bound on this very case."""
    ru, rp = pair
    case = K.case_of(ru.key)
    regime = ru.key[1]
    K.assert_regime(case, regime)
    if ru.link == "logit":
        K.assert_unclamped(case)
    _check_pair(dev, ru, rp)
    if regime == "exp_overflow":
        for r in (ru, rp):
            em = K.emulate(case, r.link, r.paired, r.parts, mutant="pair_drop")
            assert np.max(np.abs(em["phi"] - K.oracles(r.key, r.link)["at"]["phi"]) / K.bound_of(r)["phi"]) > 1.0


@pytest.mark.parametrize("pair", _pairs(K.clamp_runs()), ids=_pid)
def test_logit_link_clamps(dev, pair):
    """fx is the model's logit, unclamped, on the device and in the host reference; coalition
    probabilities within 1e-7 of 1 take the device's clamp (logit 15.9), which the oracles reproduce
    through their clamp parameter.  Asserted within the derived bound, and within the bound that
    holds once the saturated coalitions are known to clamp (device_bound, rcp_pow2_exact)."""
    ru, rp = pair
    case = K.case_of(ru.key)
    gu, gp = _check_pair(dev, ru, rp)
    _check_pair(dev, ru, rp, pow2=True)
    lx = case.X.astype(np.float64) @ case.a[: case.d] + case.bias
    if ru.key[1] == "wide_fx":
        assert np.abs(gu["fx"]).min() > 28.0 and np.abs(gp["fx"]).min() > 28.0
    Z, _, A, zM = case.design()
    host = EX.kernelshap_reference(case.X, case.a, case.bias, case.B, Z, A, zM, "logit")
    o, b = K.oracles(ru.key, "logit"), K.bound_of(ru)
    K.assert_within(gu["fx"], host[1], b["fx"] + o["ob"]["fx"], f"[clamp] device fx vs host reference {ru.id}")
    np.testing.assert_allclose(host[1], lx, rtol=0, atol=1e-12)


DET_KEY = ("random", 11, 37, 1, 211)


@pytest.mark.parametrize("paired", [False, True])
@pytest.mark.parametrize("link", ["identity", "logit_model"])
def test_reruns_are_bit_identical_and_counters_return_to_zero(dev, link, paired):
    first = None
    for parts in range(1, 9):
        r = K.Run("determinism", DET_KEY, link, paired, parts)
        a, ke = _launch(dev, r)
        b, _ = _launch(dev, r)
        assert np.array_equal(a["phi"], b["phi"]) and np.array_equal(a["fx"], b["fx"]) and a["f0"] == b["f0"]
        K.assert_outputs_within(a, K.oracles(r.key, link)["at"], K.bound_of(r), f"[determinism] {r.id}")
        first = a if first is None else first
        assert np.array_equal(a["fx"], first["fx"]) and a["f0"] == first["f0"]      # parts touch only the projection
    # the explainer of the last launch ran parts = 2..8 through its workspace: all counters are back to 0
    ke = K.case_of(DET_KEY).explainer(link, str(dev))
    from fraud_detection_amd.ops.kernelshap import kernelshap

    Xd = torch.from_numpy(K.case_of(DET_KEY).X).to(dev)
    for parts in range(2, 9):
        kernelshap(Xd, ke, parts=parts, paired=paired)
        cnt = ke._dev_cache[1]["ws"].cnt
        assert cnt is not None and int(cnt.abs().sum().item()) == 0, parts


@pytest.mark.parametrize("paired", [False, True])
def test_workspace_grows_past_its_first_capacity(dev, paired):
    """parts = 2: 8 explanations (capacity 1024), 1500 (the workspace is reallocated), 8 again."""
    from fraud_detection_amd.ops.kernelshap import kernelshap

    big_key = ("random", 8, 21, 1500, 608)
    big = K.case_of(big_key)
    small = K.Case("first 8 rows", big.a, big.bias, big.B, big.X[:8].copy())
    ke = big.explainer("identity", str(dev))
    outs = []
    caps = []
    for X in (small.X, big.X, small.X):
        phi, fx, f0 = kernelshap(torch.from_numpy(X).to(dev), ke, parts=2, paired=paired)
        outs.append({"phi": phi, "fx": fx, "f0": f0, "delta": fx - f0})
        ws = ke._dev_cache[1]["ws"]
        caps.append(ws.ws.shape[0])
        assert int(ws.cnt.abs().sum().item()) == 0
    assert caps[0] == 1024 and caps[1] >= 1500 and caps[2] == caps[1]
    bb = K.device_bound(big, "identity", paired, 2)
    K.assert_outputs_within(outs[1], K.oracle_at_operands(big, "identity"), bb, f"[workspace] 1500 rows paired={paired}")
    bs, os_ = K.device_bound(small, "identity", paired, 2), K.oracle_at_operands(small, "identity")
    for i in (0, 2):
        K.assert_outputs_within(outs[i], os_, bs, f"[workspace] 8 rows, launch {i} paired={paired}")
    assert np.array_equal(outs[0]["phi"], outs[2]["phi"]) and np.array_equal(outs[0]["fx"], outs[2]["fx"])
    assert np.array_equal(outs[1]["phi"][:8], outs[0]["phi"])           # a row's result does not depend on the batch


@pytest.mark.parametrize("paired", [False, True])
def test_out_views_and_async_results(dev, paired):
    from fraud_detection_amd.ops.kernelshap import kernelshap

    r = K.Run("out", ("random", 9, 40, 1, 209), "logit", paired, 3)
    case = K.case_of(r.key)
    want, ke = _launch(dev, r)
    E, d = case.X.shape
    Xd = torch.from_numpy(case.X).to(dev)
    buf = torch.full((E * (d + 2) + 3,), float("nan"), device=dev)
    out = (buf[: E * d].view(E, d), buf[E * d: E * d + E], buf[E * d + E: E * d + 2 * E])
    res = kernelshap(Xd, ke, parts=r.parts, paired=paired, out=out, sync=False)
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(res, out))
    torch.cuda.synchronize()
    assert np.array_equal(buf[: E * d].view(E, d).cpu().numpy().astype(np.float64), want["phi"])
    assert np.array_equal(out[1].cpu().numpy().astype(np.float64), want["fx"]) and float(out[2][0]) == want["f0"]
    assert bool(torch.isnan(buf[E * d + 2 * E:]).all())                  # nothing written past the views
    phi, fx, f0 = kernelshap(Xd, ke, parts=r.parts, paired=paired, sync=False)
    assert phi.is_cuda and fx.is_cuda and f0.is_cuda
    assert np.array_equal(phi.cpu().numpy().astype(np.float64), want["phi"])
    assert np.array_equal(fx.cpu().numpy().astype(np.float64), want["fx"]) and float(f0[0]) == want["f0"]


def test_guards_throw_on_the_host(dev):
    """Every guard of launch_kernelshap / launch_kernelshap_paired throws before a launch.  The
    buffers are real and large enough for every argument below, so nothing here can reach past one."""
    from fraud_detection_amd.ops.native import native, ptr, stream_of

    m = native()
    f = lambda *s: torch.zeros(*s, device=dev, dtype=torch.float32)  # noqa: E731
    X, a, bg, cb = f(8, 32), f(32), f(256, 32), f(256)
    Zb = torch.zeros(8192, 32, device=dev, dtype=torch.bfloat16)
    Zm = torch.zeros(8192, device=dev, dtype=torch.int32)
    A, Az = f(32, 8192), f(32)
    phi, fx, f0 = f(8, 32), f(8), f(8)
    ws, cnt = f(16, 8, 32), torch.zeros(16, device=dev, dtype=torch.int32)
    s = stream_of(X)

    def unpaired(d=8, n_bg=10, S=254, S_pad=256, parts=1, ws_=ws, cnt_=cnt):
        m.kernelshap(ptr(X), 2, d, ptr(a), 0.0, ptr(bg), ptr(cb), n_bg, ptr(Zb), S, S_pad, parts, ptr(A), ptr(Az), 0,
                     ptr(phi), ptr(fx), ptr(f0), ptr(ws_), ptr(cnt_), s, 0)

    def paired(d=8, n_bg=10, Ppad=128, parts=1, ws_=ws, cnt_=cnt):
        m.kernelshap_paired(ptr(X), 2, d, ptr(a), 0.0, ptr(bg), ptr(cb), n_bg, ptr(Zm), Ppad, parts, ptr(A), ptr(Az), 0,
                            ptr(phi), ptr(fx), ptr(f0), ptr(ws_), ptr(cnt_), s)

    bad_unpaired = [dict(d=1), dict(d=31), dict(S=40, S_pad=40), dict(S=4100, S_pad=4128), dict(parts=0), dict(parts=9),
                    dict(S=60, S_pad=64, parts=3), dict(n_bg=0), dict(n_bg=129), dict(parts=2, ws_=None),
                    dict(parts=2, cnt_=None), dict(S=300, S_pad=256), dict(S=0)]
    bad_paired = [dict(d=1), dict(d=31), dict(Ppad=40), dict(Ppad=2080), dict(parts=0), dict(parts=9),
                  dict(Ppad=64, parts=3), dict(n_bg=0), dict(n_bg=129), dict(parts=2, ws_=None), dict(parts=2, cnt_=None)]
    for fn, bad in ((unpaired, bad_unpaired), (paired, bad_paired)):
        for kw in bad:
            with pytest.raises(RuntimeError, match="kernelshap"):
                fn(**kw)
    phi.fill_(7.0)
    torch.cuda.synchronize()
    assert bool((phi == 7.0).all())                                       # no refused call launched anything
    unpaired()                                                            # the defaults are a valid launch
    paired()
    torch.cuda.synchronize()


def test_python_level_guards(dev):
    from fraud_detection_amd.ops.kernelshap import kernelshap

    case = K.case_of(("random", 8, 9, 3, 109))
    ke = case.explainer("identity", str(dev))
    wide = torch.zeros(3, 16, device=dev)
    for X in (wide[:, :8], wide[:, ::2], torch.zeros(3, 7, device=dev), torch.zeros(3, 8, device=dev, dtype=torch.float64),
              torch.zeros(8, device=dev)):
        with pytest.raises(ValueError, match="contiguous float32"):
            kernelshap(X, ke)
    with pytest.raises(ValueError, match="out ="):
        kernelshap(torch.zeros(3, 8, device=dev), ke, out=(torch.zeros(2, 8, device=dev), torch.zeros(3, device=dev),
                                                           torch.zeros(3, device=dev)))
    # designs beyond the kernels' capacity are refused when they are uploaded
    rng = np.random.default_rng(0)
    too_big = EX.KernelExplainer(np.r_[rng.normal(size=30), 0, 0], 0.0, rng.normal(size=(4, 30)).astype(np.float32),
                                 nsamples=6000, device=str(dev))
    assert too_big.nsamples > 4096
    for paired in (False, True):
        with pytest.raises(ValueError, match="at most"):
            kernelshap(torch.zeros(1, 30, device=dev), too_big, paired=paired)
    phi, fx, f0 = kernelshap(torch.zeros(0, 8, device=dev), ke)            # no rows: no launch, empty result
    assert phi.shape == (0, 8) and fx.shape == (0,)
