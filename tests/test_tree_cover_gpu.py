"""treecover.hip on the device against the numpy oracle reference_gbdt.node_cover.

The count kind is integer arithmetic on both sides and must agree bit for bit.  The hessian kind
sums llrint(p (1 - p) 2^30) with p from an fp64 sigmoid whose exp is the device's on one side and
numpy's on the other: both are within an ulp or so of the true value and p (1 - p) 2^30 <= 2^28, so
the two real numbers differ by far less than 1 and the rounded integers by at most 1 per row --
|cover_gpu - cover_oracle| <= count[node] -- while everything after the rounding is exact: internal
nodes equal their children's sum and two runs agree bit for bit.  Each hessian case prints how many
entries differ at all."""
import numpy as np
import pytest
import torch

import _tree_cases as TC
import _tree_path_cases as PC
from fraud_detection_amd.ops import gbdt as gb
from fraud_detection_amd.ops import reference_gbdt as R

pytestmark = pytest.mark.gpu


def _oracle(ens, rows, kind):
    dl = ens.default_left if ens.has_default_left else None
    return R.node_cover(rows, ens.feat, ens.thr, ens.leaf, ens.depth, ens.base_margin, dl, kind)


def _device(dev, ens, rows, kind):
    return gb.node_cover(torch.from_numpy(rows).to(dev), ens, kind).cpu().numpy()


def _check(dev, ens, rows, what):
    """Both kinds of one case; returns the device tables."""
    cnt = _device(dev, ens, rows, "count")
    want = _oracle(ens, rows, "count")
    assert cnt.dtype == np.int64 and cnt.shape == (ens.n_trees, 2 << ens.depth)
    assert np.array_equal(cnt, want), f"{what}: count cover differs"
    assert np.all(cnt[:, 1] == len(rows)) and np.all(cnt[:, 0] == 0)
    hes = _device(dev, ens, rows, "hessian")
    hw = _oracle(ens, rows, "hessian")
    diff = np.abs(hes - hw)
    print(f"[tree-cover] {what}: {int((diff != 0).sum())} of {diff.size} hessian entries differ, max {int(diff.max())}")
    assert np.all(diff <= cnt), f"{what}: hessian cover outside one unit per contributing row"
    nl = 1 << ens.depth
    for k in range(1, nl):
        assert np.array_equal(hes[:, k], hes[:, 2 * k] + hes[:, 2 * k + 1])
    assert np.all(hes[:, 0] == 0)
    assert np.array_equal(hes, _device(dev, ens, rows, "hessian"))
    return cnt, hes


@pytest.mark.parametrize("depth", [1, 2, 3, 4, 5])
def test_every_depth(dev, depth):
    ens, _, rows = TC.oracle_case(depth, 6, T=9, n_bg=700)
    assert (ens.feat < 0).any()  # pass-through nodes
    _check(dev, ens, rows, f"depth {depth}")


@pytest.mark.parametrize("n", [1, 255, 257, 5 * 256 + 17, 600 * 256 + 44])
def test_row_counts(dev, n):
    """One row, one short of / one past a block, several blocks and a tail, and more tiles than the
    launcher's grid (2 blocks per CU), where blocks stride over tiles."""
    ens = TC.random_ensemble(6, 4, 5, 31)
    rows = np.random.default_rng(n).normal(size=(n, 6)).astype(np.float32)
    _check(dev, ens, rows, f"n {n}")


def test_thresholds_on_row_values(dev):
    ens, Xs, rows = TC.oracle_case(4, 6, T=12, n_bg=400)
    ens = TC.plant_ties(ens, rows, rows, 5)
    on = (rows[:, np.maximum(ens.feat, 0)] == ens.thr[None]) & (ens.feat >= 0)[None]
    assert on.any()
    _check(dev, ens, rows, "ties")


@pytest.mark.parametrize("dleft", [False, True])
def test_nan_rows(dev, dleft):
    ens, _, rows = TC.oracle_case(4, 6, T=8, n_bg=500)
    if dleft:
        ens = PC.with_default_left(ens, 7)
    rows = rows.copy()
    rows[::5, 1] = np.nan
    rows[3] = np.nan
    cnt, _ = _check(dev, ens, rows, f"NaN rows, default_left {dleft}")
    if dleft:  # and the directions matter: without them the same rows count differently
        from dataclasses import replace

        assert not np.array_equal(cnt, _oracle(replace(ens, default_left=None), rows, "count"))


def test_rows_that_agree_on_every_leaf(dev):
    """Identical rows: all 64 lanes of every wave meet on one LDS accumulator per tree."""
    ens = TC.random_ensemble(6, 5, 10, 41)
    rows = np.tile(np.random.default_rng(1).normal(size=(1, 6)).astype(np.float32), (1000, 1))
    cnt, _ = _check(dev, ens, rows, "identical rows")
    assert np.all((cnt[:, 32:] == 0) | (cnt[:, 32:] == 1000))


@pytest.mark.parametrize("over", [0, 1, 51])
def test_both_sides_of_the_lds_chunk(dev, over):
    """chunk trees run in one launch; chunk + 1 and 2 chunk + 1 in two and three, the hessian kind
    carrying every row's margin from launch to launch."""
    chunk = gb.tree_cover_chunk(5)
    assert chunk == PC.cover_chunk(5) == 50
    ens = TC.random_ensemble(8, 5, chunk + over, 51)
    rows = np.random.default_rng(52).normal(size=(3 * 256 + 9, 8)).astype(np.float32)
    _check(dev, ens, rows, f"T {chunk + over}")


def test_strided_rows_and_no_rows(dev):
    ens = TC.random_ensemble(6, 3, 4, 61)
    wide = torch.from_numpy(np.random.default_rng(62).normal(size=(300, 32)).astype(np.float32)).to(dev)
    got = gb.node_cover(wide[:, :6], ens, "count").cpu().numpy()
    assert np.array_equal(got, _oracle(ens, wide[:, :6].cpu().numpy(), "count"))
    empty = gb.node_cover(wide[:0, :6], ens, "hessian").cpu().numpy()
    assert empty.shape == (4, 16) and not empty.any()


def test_launcher_limits(dev):
    from fraud_detection_amd.ops.native import native, ptr, stream_of

    z = torch.zeros(4096, device=dev)
    zi = torch.zeros(4096, device=dev, dtype=torch.int32)
    out = torch.zeros(4096, device=dev, dtype=torch.int64)

    def launch(n=1, ld=6, d=6, T=2, depth=2, kind=0, ws=0):
        native().tree_cover(ptr(z), n, ld, d, ptr(zi), ptr(z), ptr(z), 0, T, depth, 0.0, kind, ws, ptr(out),
                            stream_of(z))

    for kw, msg in (({"depth": 0}, "depth"), ({"depth": 9}, "depth"), ({"d": 31, "ld": 31}, "30 features"),
                    ({"ld": 5}, "stride"), ({"T": 0}, "tree"), ({"kind": 2}, "kind"),
                    ({"T": 1000, "depth": 1, "kind": 1}, "workspace")):
        with pytest.raises(Exception, match=msg):
            launch(**kw)
    torch.cuda.synchronize(dev)
