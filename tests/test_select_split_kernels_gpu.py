"""Every kernel of quantile.hip and split.hip (with the count and scan kernels that feed the split)
against the exact oracles of _metric_cases.py, at the smallest shapes that can break it, on MI355X.

Which test launches which kernel:

  qsel_hist_kernel, qsel_plan_kernel, qsel_scatter_kernel, qsel_final_kernel
                                test_quantile_select[d-max_bin] (m over the 4096-row block boundary, both
                                row layouts), test_quantile_select_counts[*] (the plan's clamp of counts),
                                test_quantile_select_dirty_workspace; test_quantile_select_guards launches
                                nothing
  strat_assign_kernel           test_strat_assign[n] (through ops.split.assign), test_strat_assign_direct[*]
                                (the three native calls, grids the wrapper never picks),
                                test_strat_assign_unaligned_view, test_strat_assign_seeds_differ;
                                test_strat_assign_guards launches nothing
  compact_count16_kernel, exclusive_scan_small_kernel
                                the same tests (they feed the assignment its block offsets)

The raw [max_bin, d] picks are compared with np.sort at the oracle's ranks by value, NaN for NaN,
every zero as +0.0; the split codes bit for bit with assign_numpy, and the properties the kernel
exists to deliver (_metric_cases.split_properties) are asserted on the device output itself.
"""
import numpy as np
import pytest
import torch

import _metric_cases as C
from fraud_detection_amd.ops import split as SP
from fraud_detection_amd.ops.native import native, ptr, stream_of

pytestmark = pytest.mark.gpu

ROWS = [1, 3, 255, 256, 257, 4095, 4096, 4097, 8193]  # 4096: the rows of one histogram / scatter block


# ---- A. quantile_select ---------------------------------------------------------------------------
def _select(sample: np.ndarray, max_bin: int, dev, stride: int = 1, pad: int = 0, counts=None, ws_fill: int = 0):
    """Raw picks of the native select over ``sample`` laid out with a row stride and ``pad`` padding
    columns; the skipped rows and the padding hold NaN, so a stray read surfaces as a NaN pick."""
    m, d = sample.shape
    ld = d + pad
    buf = np.full((m * stride, ld), np.nan, dtype=np.float32)
    buf[::stride, :d] = sample
    X = torch.from_numpy(buf).to(dev)
    nat = native()
    ws = torch.full((int(nat.quantile_select_ws_bytes(m, d)),), ws_fill, dtype=torch.uint8, device=dev)
    out = torch.full((max_bin, d), 1234.5, dtype=torch.float32, device=dev)
    cd = None if counts is None else torch.from_numpy(np.asarray(counts, dtype=np.int64)).to(dev)
    extra = () if cd is None else (ptr(cd),)
    nat.quantile_select(ptr(X), m, stride, ld, d, max_bin, ptr(ws), ptr(out), stream_of(X), *extra)
    return out.cpu().numpy()


@pytest.mark.parametrize("max_bin", [2, 37, 255, 256])
@pytest.mark.parametrize("d", [1, 4, 5, 32])
def test_quantile_select(dev, d, max_bin):
    """d = 4: one full feature group; 5: a group of one; 32: the maximum, every value kind at once.
    m < max_bin: many targets share a rank."""
    seen = set()
    for i, m in enumerate(ROWS):
        sample, kinds = C.select_sample(m, d, offset=i + max_bin)
        seen |= set(kinds)
        exp = C.select_picks(sample, max_bin)
        for stride, pad in ((1, 0), (3, 2)):
            bad = C.picks_mismatch(_select(sample, max_bin, dev, stride, pad), exp)
            assert bad is None, (m, stride, bad, kinds)
    if d >= 4:
        assert seen == set(C.SELECT_KINDS)


@pytest.mark.parametrize("m", [257, 4097])
def test_quantile_select_counts(dev, m):
    """Per-feature rank bases m_f in {0, 1, m - 1, m}, and one above m and a negative one, which the
    plan kernel clamps to [0, m]."""
    counts = [0, 1, m - 1, m, m + 1000, -5, m // 2]
    for offset in (0, 5):
        sample, kinds = C.select_sample(m, len(counts), offset)
        for max_bin in (2, 255):
            exp = C.select_picks(sample, max_bin, counts)
            bad = C.picks_mismatch(_select(sample, max_bin, dev, 3, 2, counts), exp)
            assert bad is None, (m, max_bin, bad, kinds)
    # m_f below the non-NaN count keeps every pick off the NaN tail
    sample, _ = C.select_sample(m, 1, offset=C.SELECT_KINDS.index("nan_some"))
    valid = int(np.count_nonzero(~np.isnan(sample[:, 0])))
    got = _select(sample, 64, dev, counts=[valid])
    assert not np.isnan(got).any() and C.picks_mismatch(got, C.select_picks(sample, 64, [valid])) is None


def test_quantile_select_dirty_workspace(dev):
    """The launcher clears what it accumulates into: a workspace of 0xFF bytes gives the same picks."""
    sample, _ = C.select_sample(4097, 5, offset=0)
    clean = _select(sample, 37, dev, ws_fill=0)
    dirty = _select(sample, 37, dev, ws_fill=0xFF)
    assert np.array_equal(clean.view(np.uint32), dirty.view(np.uint32))
    assert C.picks_mismatch(dirty, C.select_picks(sample, 37)) is None


def test_quantile_select_guards(dev):
    """launch_quantile_select checks d, max_bin and m before its first call into the runtime."""
    X = torch.zeros((8, 40), dtype=torch.float32, device=dev)
    ws = torch.zeros(int(native().quantile_select_ws_bytes(8, 32)), dtype=torch.uint8, device=dev)
    out = torch.full((256, 32), 7.0, dtype=torch.float32, device=dev)
    for m, d, max_bin in ((8, 0, 16), (8, 33, 16), (8, 4, 1), (8, 4, 257), (0, 4, 16)):
        with pytest.raises(RuntimeError, match="quantile_select"):
            native().quantile_select(ptr(X), m, 1, 40, d, max_bin, ptr(ws), ptr(out), stream_of(X))
    assert bool((out == 7.0).all())


# ---- B. strat_assign ------------------------------------------------------------------------------
FRACS = (0.0, 0.2, 0.5, 1.0)
FOLDS = (0, 1, 2, 5, 254)


def _check(codes: np.ndarray, y: np.ndarray, frac: float, k: int, seed: int, where):
    assert codes.dtype == np.uint8
    assert np.array_equal(codes, SP.assign_numpy(y, frac, k, seed)), where
    assert C.split_properties(codes, y, frac, k) == [], where


@pytest.mark.parametrize("n", [1, 15, 16, 17, 4095, 4096, 4097, 65_537])
def test_strat_assign(dev, n):
    """n on both sides of a 16-label group and of a block's 4096 rows; class sizes from nothing to
    everything, around k, and 4, 5, 2^j, 2^j + 1 (cycle walking in a domain two to four times the
    class); label bytes 2 and 255 count as class 0."""
    for k in FOLDS:
        for i, n1 in enumerate(C.class_sizes(n, k)):
            y = C.split_labels(n, n1, seed=k, other_bytes=i % 2 == 0)
            yd = torch.from_numpy(y).to(dev)
            for frac in FRACS:
                nblocks = (1, 3, 512)[(i + int(frac * 10)) % 3]
                codes = SP.assign(yd, frac, k, 42, nblocks=nblocks).cpu().numpy()
                _check(codes, y, frac, k, 42, (n, n1, frac, k, nblocks))


def _assign_direct(y: np.ndarray, frac: float, k: int, seed: int, nb: int, dev) -> np.ndarray:
    n = y.shape[0]
    yd = torch.from_numpy(y).to(dev)
    assert yd.data_ptr() % 16 == 0
    m, s = native(), stream_of(yd)
    counts = torch.empty(nb, device=dev, dtype=torch.int64)
    total = torch.empty(1, device=dev, dtype=torch.int64)
    out = torch.full((n + 16,), 0xAB, device=dev, dtype=torch.uint8)
    m.compact_count(ptr(yd), n, 1, ptr(counts), nb, s)
    m.exclusive_scan_small(ptr(counts), nb, ptr(total), s)
    m.strat_assign(ptr(yd), n, ptr(counts), ptr(total), seed, frac, k, ptr(out), nb, s)
    got = out.cpu().numpy()
    assert int(total.item()) == int(np.count_nonzero(y == 1))
    assert np.all(got[n:] == 0xAB)  # nothing past row n - 1, whole-group stores included
    return got[:n]


@pytest.mark.parametrize("n,nb", [(17, 8), (17, 1), (4097, 3), (4097, 512), (65_537, 1), (65_537, 3), (65_537, 512),
                                  (1, 4)])
def test_strat_assign_direct(dev, n, nb):
    """The three native calls with grids ops.split.assign never picks: more blocks than 16-label
    groups (n = 17 with 8 blocks: six blocks own nothing), one block walking every group, 512 blocks
    over 4097 groups."""
    for n1 in sorted({0, 1, n // 3, n}):
        y = C.split_labels(n, n1, seed=nb, other_bytes=True)
        for frac, k in ((0.2, 5), (0.5, 2), (0.0, 254), (1.0, 0)):
            _check(_assign_direct(y, frac, k, 7, nb, dev), y, frac, k, 7, (n, nb, n1, frac, k))


def test_strat_assign_unaligned_view(dev):
    """A label view at byte offset 3 gives the codes of its aligned copy."""
    n = 4097
    y = C.split_labels(n, 300, other_bytes=True)
    buf = torch.zeros(n + 16, dtype=torch.uint8, device=dev)
    buf[3:3 + n] = torch.from_numpy(y).to(dev)
    view = buf[3:3 + n]
    assert view.data_ptr() % 16 == 3
    codes = SP.assign(view, 0.2, 5, 42).cpu().numpy()
    assert np.array_equal(codes, SP.assign(view.clone(), 0.2, 5, 42).cpu().numpy())
    _check(codes, y, 0.2, 5, 42, "view")


def test_strat_assign_seeds_differ(dev):
    y = C.split_labels(4097, 300)
    yd = torch.from_numpy(y).to(dev)
    a, b = (SP.assign(yd, 0.2, 5, seed).cpu().numpy() for seed in (42, 43))
    assert not np.array_equal(a, b)
    _check(a, y, 0.2, 5, 42, 42)
    _check(b, y, 0.2, 5, 43, 43)


def test_strat_assign_guards(dev):
    """launch_strat_assign checks both alignments and k before the launch."""
    buf = torch.zeros(64, dtype=torch.uint8, device=dev)
    out = torch.full((64,), 0xAB, dtype=torch.uint8, device=dev)
    offs = torch.zeros(1, dtype=torch.int64, device=dev)
    s = stream_of(buf)
    assert buf.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    for lab, dst, k in ((buf[3:], out, 5), (buf, out[8:], 5), (buf, out, 255), (buf, out, -1)):
        with pytest.raises(ValueError, match="strat_assign"):
            native().strat_assign(ptr(lab), 32, ptr(offs), ptr(offs), 42, 0.2, k, ptr(dst), 1, s)
    assert bool((out == 0xAB).all())
    with pytest.raises(ValueError):
        SP.assign(buf, 0.2, 255)
