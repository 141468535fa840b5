"""Every kernel of smote.hip against the oracles of _smote_cases.py on MI355X: equality of the stored
bits over every element (no share of unequal elements, no tolerance), at the smallest shapes that can
break the kernel.

Which test launches which kernel:

  smote_parents_kernel                          test_parents[*]
  smote_generate_kernel<0, NT, PB, G2>          test_generate_edges / _variants / _sweep[pbf16-bf16], test_slices[bf16]
  smote_generate_kernel<0, NT, false>           test_generate_edges / _variants / _sweep[pf32-bf16, pf32aff-bf16]
  smote_generate_kernel<1, false, PB>           ...[pbf16-f32]
  smote_generate_kernel<1, false, false>        ...[pf32-f32, pf32aff-f32]
  smote_generate_kernel<2, false, PB>           ...[pbf16-fp8], test_slices[fp8]
  smote_generate_kernel<2, false, false>        ...[pf32-fp8, pf32aff-fp8]
  one rounding (fmaf), not two, in each         test_generate_single_rounding[*] (all rows of 131 072)
  the pipelined grid-stride loop of each        test_generate_sweep[*] (more samples than any resident grid
                                                covers in one sweep; the next iteration's draws in flight)
  smote_bucket_l1_kernel<false / true>,         test_buckets[*] (staged bins, a bin exactly at the stage's
  smote_bucket_l2_kernel                        size, unstaged bins, fb = 7 with a partial last bin, one
                                                sample, one pick, level-1 block boundaries, sample offsets)
  logreg.hip pick_terms over an unstaged run    test_virtual_pass_reads_the_unstaged_layout
"""
import numpy as np
import pytest
import torch

import _smote_cases as SC
from fraud_detection_amd.ops import knn as K
from fraud_detection_amd.ops import logreg as L
from fraud_detection_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

_STORAGE = {"f32": (torch.float32, 128), "bf16": (torch.bfloat16, 64), "fp8": (torch.uint8, 32)}
_SENTINEL, _PAD = 0xA5, 32


def _bits(t: torch.Tensor) -> np.ndarray:
    """Stored elements on the host: float32 bits (uint32), bf16 bits (uint16) or e4m3 codes (uint8)."""
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    if t.dtype == torch.float32:
        return t.view(torch.int32).cpu().numpy().view(np.uint32)
    return t.cpu().numpy()


def _out(n: int, kind: str, dev):
    """([n, 32] rows of ``kind``, the 32 sentinel bytes after the last row)."""
    dt, rb = _STORAGE[kind]
    buf = torch.full((n * rb + _PAD,), _SENTINEL, dtype=torch.uint8, device=dev)
    return buf[: n * rb].view(dt).view(n, 32), buf[n * rb:]


def _parents(m: int, ptype: str, dev) -> torch.Tensor:
    if ptype == "bf16":
        return torch.from_numpy(SC.parents_bf16(m).view(np.int16)).to(dev).view(torch.bfloat16)
    return torch.from_numpy(np.array(SC.parents(m))).to(dev)


def _assert_rows(got: np.ndarray, exp: np.ndarray, what) -> None:
    assert got.shape == exp.shape and got.dtype == exp.dtype, (what, got.shape, exp.shape, got.dtype, exp.dtype)
    bad = np.argwhere(got != exp)
    assert bad.size == 0, (what, f"{bad.shape[0]} of {got.size} elements differ", "first (row, col):",
                           bad[:5].tolist(), [(hex(int(got[r, c])), hex(int(exp[r, c]))) for r, c in bad[:5]])


def _generate(dev, pname, kind, n_new, m=SC.GEN_M, mq=SC.GEN_MQ, q_off=SC.GEN_QOFF, k=SC.GEN_K, label=1.0,
              fp8_scale=SC.FP8_SCALE, s_off=0):
    """Launch one smote_generate; returns (out tensor, pad bytes, oracle(rows) -> stored bits)."""
    ptype, use_aff = SC.GEN_PARENTS[pname]
    aff = SC.affine() if use_aff else None
    nbr = SC.neighbours(mq, k, m)
    out, pad = _out(n_new, kind, dev)
    K.smote_generate(_parents(m, ptype, dev), torch.from_numpy(nbr).to(dev), q_off, n_new, out, seed=SC.SEED,
                     counter_base=SC.COUNTER_BASE, label=label, fp8_scale=fp8_scale,
                     affine=None if aff is None else torch.from_numpy(aff).to(dev), sample_offset=s_off)

    def oracle(rows=None):
        return SC.generate_oracle(SC.parent_values(m, ptype), nbr, q_off, SC.sample_ids(n_new, s_off, rows), kind,
                                  label, aff, fp8_scale)

    return out, pad, oracle


# ---- a. smote_parents_kernel ---------------------------------------------------------------------
@pytest.mark.parametrize("use_aff", [False, True], ids=["plain", "affine"])
@pytest.mark.parametrize("m", SC.PARENT_ROWS)
def test_parents(dev, m, use_aff):
    """bf16(v * sig + cc) as a float32 multiply, then a float32 add, then integer round-to-nearest-even;
    the input holds exact bf16 ties of both parities, -0.0 and magnitudes up to 1e30."""
    X = SC.parents_case(m)
    aff = SC.affine() if use_aff else None
    P = K.smote_parents(torch.from_numpy(X).to(dev), None if aff is None else torch.from_numpy(aff).to(dev))
    _assert_rows(_bits(P), SC.parents_oracle(X, aff), (m, use_aff))


# ---- b. every smote_generate_kernel variant at the edges -----------------------------------------
@pytest.mark.parametrize("kind", SC.KINDS)
@pytest.mark.parametrize("pname", list(SC.GEN_PARENTS))
def test_generate_edges(dev, pname, kind):
    """n_new at every boundary of the lane groups (16), the Philox halves (64), a wave's iteration (128)
    and a block (512); neighbours below q_offset; the bytes after the last row untouched."""
    for n_new in SC.GEN_N:
        out, pad, oracle = _generate(dev, pname, kind, n_new)
        _assert_rows(_bits(out), oracle(), (pname, kind, n_new))
        assert bool(torch.all(pad == _SENTINEL)), (pname, kind, n_new, "wrote past the last row")


_VARIANTS = {"k1": dict(k=1), "k3": dict(k=3), "k8": dict(k=8), "label0": dict(label=0.0),
             "scale3": dict(fp8_scale=3.0), "offset128": dict(s_off=128), "offset_high": dict(s_off=SC.HIGH_OFFSET)}


@pytest.mark.parametrize("variant", list(_VARIANTS))
@pytest.mark.parametrize("kind", SC.KINDS)
@pytest.mark.parametrize("pname", list(SC.GEN_PARENTS))
def test_generate_variants(dev, pname, kind, variant):
    """Other k, label 0, a rounding fp8 scale (on the features only) and sample offsets, one of which
    needs the high word of the Philox counter."""
    out, pad, oracle = _generate(dev, pname, kind, SC.GEN_N_VARIANTS, **_VARIANTS[variant])
    _assert_rows(_bits(out), oracle(), (pname, kind, variant))
    assert bool(torch.all(pad == _SENTINEL))


# ---- c. the pipelined grid-stride loop -----------------------------------------------------------
@pytest.mark.parametrize("pname,kind", [("pbf16", "bf16"), ("pf32aff", "bf16"), ("pbf16", "f32"), ("pf32aff", "f32"),
                                        ("pbf16", "fp8"), ("pf32aff", "fp8")])
def test_generate_sweep(dev, pname, kind):
    """More samples than one sweep of any resident grid: a 256-thread block covers 512 samples per
    iteration and at most 8 blocks are resident per CU, so past 8 x CUs x 512 samples every launch is in
    its grid-stride loop, whose next draws are issued behind the current gathers.  Checked: every row
    from 1024 before that point to the end, and every 97th row before."""
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    first = 8 * cus * 512
    n_new = first + 137
    out, pad, oracle = _generate(dev, pname, kind, n_new, m=SC.SWEEP_M, mq=SC.SWEEP_MQ, q_off=SC.SWEEP_M - SC.SWEEP_MQ,
                                 k=SC.SWEEP_K)
    rows = SC.sweep_rows(n_new, first)
    got = _bits(out[torch.from_numpy(rows).to(dev)])
    _assert_rows(got, oracle(rows), (pname, kind, n_new))
    assert bool(torch.all(pad == _SENTINEL))


@pytest.mark.parametrize("kind", SC.KINDS)
@pytest.mark.parametrize("pname", ["pbf16", "pf32"])
def test_generate_single_rounding(dev, pname, kind):
    """All 131 072 rows of one launch: enough elements that an interpolation rounded twice (a multiply,
    then an add) instead of once changes stored bf16 bits too, not only fp32 ones
    (test_smote_oracle.py::test_rounding_case_tells_one_rounding_from_two counts them)."""
    out, pad, oracle = _generate(dev, pname, kind, SC.ROUNDING_N, m=SC.SWEEP_M, mq=SC.SWEEP_MQ,
                                 q_off=SC.SWEEP_M - SC.SWEEP_MQ, k=SC.SWEEP_K)
    _assert_rows(_bits(out), oracle(), (pname, kind))
    assert bool(torch.all(pad == _SENTINEL))


# ---- d. slices of one draw sequence --------------------------------------------------------------
@pytest.mark.parametrize("kind", ["bf16", "fp8"])
def test_slices(dev, kind):
    """128-aligned sample_offset slices == one launch == the oracle."""
    n = SC.SLICES[-1][1]
    whole, _, oracle = _generate(dev, "pbf16", kind, n)
    parts, pad = _out(n, kind, dev)
    P = _parents(SC.GEN_M, "bf16", dev)
    nbr = torch.from_numpy(SC.neighbours(SC.GEN_MQ, SC.GEN_K, SC.GEN_M)).to(dev)
    for a, b in SC.SLICES:
        assert a % 128 == 0
        K.smote_generate(P, nbr, SC.GEN_QOFF, b - a, parts[a:b], seed=SC.SEED, counter_base=SC.COUNTER_BASE,
                         sample_offset=a)
    exp = oracle()
    _assert_rows(_bits(whole), exp, ("one launch", kind))
    _assert_rows(_bits(parts), exp, ("slices", kind))
    assert bool(torch.all(pad == _SENTINEL))


# ---- e. the bucket sort --------------------------------------------------------------------------
def _bucket(dev, name):
    """Run the sort into a workspace with sentinel-filled slack after every output."""
    mq, k, n_new, s_off = SC.BUCKET_CASES[name]
    R = mq * k
    m = L.native()
    ws = L.BucketWorkspace().get(dev, m.smote_bucket_bins(R, n_new) * m.smote_bucket_blocks(n_new), n_new + 64, R + 64)
    ws.off.fill_(-7)
    ws.cnt.fill_(-7)
    ws.lam.fill_(-1)
    w = L.bucket_lambdas(mq, k, n_new, s_off, SC.SEED, SC.COUNTER_BASE, dev, ws)
    assert w is ws and w.off.shape[0] == R + 64  # the sentinel-filled buffers were used
    torch.cuda.synchronize(dev)
    return w, R, n_new


@pytest.mark.parametrize("name", list(SC.BUCKET_CASES))
def test_buckets(dev, name):
    """cnt == the bincount of all picks, the runs tile [0, n_new), and every run holds exactly its pick's
    lambdas -- all picks, all samples; nothing is written past the outputs."""
    w, R, n_new = _bucket(dev, name)
    SC.check_buckets(name, w.off[:R].cpu().numpy(), w.cnt[:R].cpu().numpy(), w.lam[:n_new].cpu().numpy())
    assert bool(torch.all(w.off[R:] == -7)) and bool(torch.all(w.cnt[R:] == -7)) and bool(torch.all(w.lam[n_new:] == -1))


# ---- f. the consumer of the unstaged layout ------------------------------------------------------
def test_virtual_pass_reads_the_unstaged_layout(dev):
    """One logistic pass over a handful of real bf16 rows plus the 70 001 virtual samples of the
    all-unstaged bucket case (about 11 700 samples per pick, every lambda run written from global
    memory) against the fp64 pass over the samples' fp32 interpolants, with the bounds of
    test_virtual_smote_gpu.py::test_virtual_pass_matches_oracle.  Measured on MI355X: gradient within
    0.011 absolute at components up to 2.2e5, loss within 3e-8 relative, Hessian within 1.3e-3 in the
    Frobenius norm -- the per-pick float32 sums over 11 700 lambdas stay inside the project's bounds."""
    name = "all_unstaged"
    mq, k, n_new, s_off = SC.BUCKET_CASES[name]
    g = torch.Generator().manual_seed(n_new)
    real = torch.randn(7, 32, generator=g) * 1.5
    real[:, 30] = 1.0
    real[:, 31] = torch.tensor([0.0, 1.0, 0.0, 0.0, 1.0, 0.0, 0.0])
    par = torch.randn(8, 32, generator=g) + 0.7
    par[:, 30] = 1.0
    par[:, 31] = 1.0
    nbr = torch.stack([torch.randperm(8, generator=g)[:k] for _ in range(mq)]).to(torch.int32)
    rows = real.to(torch.bfloat16).to(dev)
    v = L.VirtualSmote(par.to(torch.bfloat16).to(dev), nbr.to(dev), n_new, q_offset=3, sample_offset=s_off,
                       seed=SC.SEED, counter_base=SC.COUNTER_BASE).prepare()
    SC.check_buckets(name, v.off[: mq * k].cpu().numpy(), v.cnt[: mq * k].cpu().numpy(), v.lam[:n_new].cpu().numpy())
    R = np.concatenate([ref.rows_to_f32(rows.cpu(), 4.0).numpy(), v.rows_f32().numpy()])
    w = np.r_[np.random.default_rng(3).normal(0, 0.3, 30), -0.5, 0.0]
    g_r, loss_r, ws_r, H_r = ref.logreg_pass(R, w, (1.0, 3.0), True)
    for hess in (True, False):
        gr, loss, ws, H = L.logreg_pass(rows, torch.from_numpy(w), (1.0, 3.0), hessian=hess, fp8_scale=4.0, virtual=v)
        print(f"hessian={hess}: max |g - g_r| {np.max(np.abs(gr - g_r)):.3g} (|g_r| max {np.max(np.abs(g_r)):.3g}), "
              f"loss rel {abs(loss - loss_r) / loss_r:.3g}, wsum {ws} vs {ws_r}")
        np.testing.assert_allclose(gr, g_r, rtol=1e-4, atol=1e-2)
        assert abs(loss - loss_r) / loss_r < 1e-5
        assert ws == pytest.approx(ws_r)
        if hess:
            rel = np.linalg.norm(H - H_r) / np.linalg.norm(H_r)
            print(f"H rel {rel:.3g}")
            assert rel < 5e-3, rel
            np.testing.assert_allclose(H, H.T, atol=1e-6 * np.abs(H).max())
