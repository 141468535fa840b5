"""treeshap.hip on the device against brute-force Shapley values, path by path.

Every case drives the public wrapper ops.treeshap.treeshap through TreeExplainer(ens, mean = 0,
scale = 1, B): (x - 0) * 1 is exact, so the oracle sees bit-identical fp32 rows.  The oracle is
tests/_tree_cases.brute_force_shapley (all 2^d coalitions, fp64, its own traversal), the tolerance
the derived bound of _tree_cases.phi_bound / fx_bound, and every case asserts from walk_stats that
its inputs reach the branch it is there for -- tests/test_treeshap.py shows that the same
assertions reject a walk without the forced-side rule, with one swapped weight, or with <= for <.
Each case prints its largest error / bound."""
import numpy as np
import pytest
import torch

import _tree_cases as TC
from fraud_detection_amd.models.explainers import TreeExplainer, treeshap_reference
from fraud_detection_amd.ops.treeshap import treeshap

pytestmark = pytest.mark.gpu


def _explainer(ens, Bs, dev):
    d = Bs.shape[1]
    return TreeExplainer(ens, np.zeros(d), np.ones(d), Bs, device=str(dev))


def _check(dev, ens, Xs, Bs, what, brute=True, reference=False, st=None):
    """Run the kernel and hold phi, fx, f0 and efficiency to the derived bounds.  Returns
    (walk_stats, (phi, fx, f0))."""
    te = _explainer(ens, Bs, dev)
    phi, fx, f0 = te.explain(Xs)
    T, n_bg, D = ens.n_trees, len(Bs), ens.depth
    st = st if st is not None else TC.walk_stats(Xs, Bs, ens)
    pb = TC.phi_bound(st["S"], T, n_bg, D)
    assert phi.shape == Xs.shape and fx.shape == (len(Xs),)
    if brute:
        TC.assert_within(phi, TC.brute_force_shapley(Xs, Bs, ens), pb, f"{what} phi vs brute force")
    if reference:
        TC.assert_within(phi, treeshap_reference(Xs, Bs, ens)[0], pb, f"{what} phi vs reference walk")
    TC.assert_within(fx, st["fx"], TC.fx_bound(st["fx_abs"], T, ens.base_margin), f"{what} fx")
    assert f0 == te.f0
    TC.assert_within(phi.sum(1), fx - f0, TC.efficiency_bound(st["S"], st["fx_abs"], st["f0_abs"], T, n_bg, D,
                                                               ens.base_margin), f"{what} efficiency")
    return st, (phi, fx, f0)


@pytest.mark.parametrize("d", [2, 3, 8])
@pytest.mark.parametrize("depth", [1, 2, 3, 4, 5])
def test_every_depth_matches_brute_force(dev, depth, d):
    ens, Xs, Bs = TC.oracle_case(depth, d)
    assert (ens.feat < 0).any()
    st, _ = _check(dev, ens, Xs, Bs, f"depth {depth} d {d}")
    assert st["split"] > 0
    if depth >= 2 and d < depth:  # a path of `depth` splits over d < depth features repeats one
        assert st["forced_x"] > 0 and st["forced_z"] > 0 and st["pass_through"] > 0


@pytest.mark.parametrize("depth", [1, 2, 3, 4, 5])
def test_weight_table_fully_reached(dev, depth):
    ens, Xs, Bs = TC.disagree_case(depth)
    st, (phi, _, _) = _check(dev, ens, Xs, Bs, f"weights depth {depth}")
    assert st["ab"] == TC.all_ab(depth)
    assert np.all(phi[:, -1] == 0.0)  # the feature every background shares with x


@pytest.fixture(scope="module")
def switch_trees():
    """One ensemble per d, one tree longer than the LDS limit; the tests truncate it."""
    out = {}
    for d in (30, 8):
        Ts = TC.treeshap_lds_boundary(d, 5)
        ens = TC.random_ensemble(d, 5, Ts + 1, 900 + d)
        Xs, Bs = TC.random_rows(d, 2, 3, 901 + d)
        out[d] = (Ts, ens, Xs, Bs)
    return out


@pytest.mark.parametrize("d,want", [(30, 129), (8, 216)])
@pytest.mark.parametrize("over", [0, 1])
def test_both_memory_paths_at_the_switch(dev, switch_trees, d, want, over):
    """T* trees keep leaves and split features in LDS, T* + 1 read them from global memory."""
    Ts, full, Xs, Bs = switch_trees[d]
    assert Ts == want
    words = lambda T: d * 256 + T + T * (2 << 5)  # noqa: E731  (launch_treeshap's rule)
    assert words(Ts) * 4 <= 65536 - 1024 < words(Ts + 1) * 4
    ens = TC.truncated(full, Ts + over)
    _check(dev, ens, Xs, Bs, f"switch d {d} T {Ts + over}", brute=d <= 8, reference=True)


def test_global_path_at_the_tree_limit(dev):
    ens = TC.random_ensemble(8, 5, 2048, 950)
    assert ens.n_trees > TC.treeshap_lds_boundary(8, 5)
    Xs, Bs = TC.random_rows(8, 1, 1, 951)
    _check(dev, ens, Xs, Bs, "T 2048 n_bg 1", reference=True)


@pytest.mark.parametrize("T,n_bg", [(1, 1), (3, 2), (2, 255), (2, 256), (2, 257), (2, 1024)])
def test_pair_loop_edges(dev, T, n_bg):
    """T * n_bg pairs strided by 256 threads: fewer pairs than threads, one short of / exactly /
    one past a full stride, the documented background maximum."""
    ens = TC.random_ensemble(6, 4, T, 960 + T)
    Xs, Bs = TC.random_rows(6, 2, n_bg, 961 + n_bg)
    _check(dev, ens, Xs, Bs, f"pairs T {T} n_bg {n_bg}")


def test_padded_background_words_are_never_read(dev):
    """native().treeshap with bw_ld = n_bg + 5 and all-ones padding: a read of the padding would
    walk a background that goes right everywhere."""
    from fraud_detection_amd.ops.native import native, ptr, stream_of

    ens, Xs, Bs = TC.oracle_case(4, 6, T=5, n_bg=7, E=3)
    te = _explainer(ens, Bs, dev)
    want = te.explain(Xs)
    T, n_bg, d, E = ens.n_trees, len(Bs), Xs.shape[1], len(Xs)
    bw = np.full((T, n_bg + 5), 0xFFFFFFFF, np.uint32)
    bw[:, :n_bg] = te.bw
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in
         (("feat", ens.feat), ("thr", ens.thr), ("leaf", ens.leaf), ("bw", bw.view(np.int32)), ("x", Xs))}
    phi = torch.full((E, d), float("nan"), device=dev)
    fx = torch.full((E,), float("nan"), device=dev)
    f0 = torch.full((E,), float("nan"), device=dev)
    native().treeshap(ptr(t["x"]), d, E, d, ptr(t["feat"]), ptr(t["thr"]), ptr(t["leaf"]), T, ens.depth,
                      float(ens.base_margin), ptr(t["bw"]), n_bg + 5, n_bg, float(te.f0), ptr(phi), ptr(fx), ptr(f0),
                      stream_of(phi))
    torch.cuda.synchronize(dev)
    assert np.array_equal(phi.cpu().numpy().astype(np.float64), want[0])  # same pairs, same order: same bits
    assert np.array_equal(fx.cpu().numpy().astype(np.float64), want[1])
    assert np.all(f0.cpu().numpy() == np.float32(te.f0))
    st = TC.walk_stats(Xs, Bs, ens)
    TC.assert_within(want[0], TC.brute_force_shapley(Xs, Bs, ens), TC.phi_bound(st["S"], T, n_bg, ens.depth),
                     "padded bw phi vs brute force")


def test_rows_exactly_on_thresholds(dev):
    """x == thr and z == thr go right ("not less"), in the kernel's own bits for x and in the
    host's tree_direction_bits for the background."""
    ens, Xs, Bs = TC.tie_case()
    split = ens.feat >= 0
    on = lambda R: (R[:, np.maximum(ens.feat, 0)] == ens.thr[None]) & split[None]  # noqa: E731  [n, T, ni]
    assert on(Xs).any() and on(Bs).any()
    st, _ = _check(dev, ens, Xs, Bs, "ties")
    assert st["ties_x"] > 0 and st["ties_z"] > 0  # and the walk visits such nodes


def test_fx_matches_the_predict_path(dev):
    from fraud_detection_amd.ops import gbdt as gb

    ens, Xs, Bs = TC.oracle_case(5, 8, E=4)
    st, (_, fx, _) = _check(dev, ens, Xs, Bs, "predict-path case")
    m = gb.predict_margin(torch.from_numpy(Xs).to(dev), ens).cpu().numpy().astype(np.float64)
    TC.assert_within(fx, m, TC.fx_bound(st["fx_abs"], ens.n_trees, ens.base_margin), "fx vs predict path")


@pytest.mark.parametrize("T", [1, 300])
def test_margin_sum_is_shared_by_the_tree_kernels(dev, T):
    """treeshap.hip, treeshap_path.hip and treeshap_interact.hip sum margin(x) with one routine
    (tree_explain.h): the same fx bit for bit, at one tree and at 300, where a thread owns two
    trees and the waves beyond the first carry partial sums.  No default_left and no NaN, so the
    three kernels walk the same direction bits."""
    import _tree_path_cases as PC
    from fraud_detection_amd.models.explainers import TreePathExplainer, _margins_from_bits, path_direction_bits
    from fraud_detection_amd.ops.treeshap import treeshap_interactions, treeshap_path

    d = 4
    Xs, Bs = TC.random_rows(d, 3, 40, 991 + T)
    ens = PC.with_count_cover(TC.random_ensemble(d, 5, T, 990 + T), Bs)
    assert not ens.has_default_left and not np.isnan(Xs).any()
    Xd = torch.from_numpy(Xs).to(dev)
    tp = TreePathExplainer(ens, np.zeros(d), np.ones(d), device=str(dev))
    fx = {"treeshap": treeshap(Xd, _explainer(ens, Bs, dev))[1], "treeshap_path": treeshap_path(Xd, tp)[1],
          "treeshap_interactions": treeshap_interactions(Xd, tp)[2]}
    want = _margins_from_bits(path_direction_bits(Xs, ens), ens).astype(np.float64)
    bound = PC.fx_bound(TC.margins64(Xs, ens)[1], T, ens.base_margin)
    for name, got in fx.items():
        print(f"[margin-sum] T {T} {name}: fx = {got.tolist()}")
    assert np.array_equal(fx["treeshap"], fx["treeshap_path"])
    assert np.array_equal(fx["treeshap"], fx["treeshap_interactions"])
    assert np.array_equal(fx["treeshap_path"], fx["treeshap_interactions"])
    TC.assert_within(fx["treeshap"], want, bound, f"T {T} fx vs the fp32 tree-order sum")


def test_deterministic_and_async_form(dev):
    """A second call gives the same bits, and so does the serving engine's form: preallocated
    outputs, no synchronisation, on a stream of its own."""
    ens, Xs, Bs = TC.oracle_case(5, 8, E=4)
    te = _explainer(ens, Bs, dev)
    Xd = torch.from_numpy(Xs).to(dev)
    phi, fx, f0 = treeshap(Xd, te)
    phi2, fx2, _ = treeshap(Xd, te)
    assert np.array_equal(phi, phi2) and np.array_equal(fx, fx2)
    out = (torch.full((4, 8), float("nan"), device=dev), torch.full((4,), float("nan"), device=dev),
           torch.full((6,), float("nan"), device=dev))
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        got = treeshap(Xd, te, sync=False, out=out)
    side.synchronize()
    assert all(g is o for g, o in zip(got, out))
    assert np.array_equal(out[0].cpu().numpy().astype(np.float64), phi)
    assert np.array_equal(out[1].cpu().numpy().astype(np.float64), fx)
    f0o = out[2].cpu().numpy()
    assert np.all(f0o[:4] == np.float32(te.f0)) and f0 == te.f0
    assert np.all(np.isnan(f0o[4:]))  # nothing past E is written


def test_no_rows(dev):
    ens, Xs, Bs = TC.oracle_case(3, 3)
    te = _explainer(ens, Bs, dev)
    phi, fx, f0 = te.explain(Xs[:0])
    assert phi.shape == (0, 3) and fx.shape == (0,) and f0 == te.f0
    phi, fx, f0 = treeshap(torch.empty((0, 3), device=dev), te, sync=False)
    assert phi.shape == (0, 3) and fx.shape == (0,) and phi.device.type == "cuda"


def test_launcher_limits_raise_before_any_launch(dev):
    """T = 2049, depth 6 and n_bg = 0 are refused on the host, by the launcher itself."""
    from fraud_detection_amd.ops.native import native, ptr, stream_of

    n = 2049 * 64  # larger than anything the refused shapes could index
    z = torch.zeros(n, device=dev)
    zi = torch.zeros(n, device=dev, dtype=torch.int32)

    def launch(T=2, depth=2, n_bg=1, bw_ld=1):
        native().treeshap(ptr(z), 32, 1, 2, ptr(zi), ptr(z), ptr(z), T, depth, 0.0, ptr(zi), bw_ld, n_bg, 0.0,
                          ptr(z), ptr(z), ptr(z), stream_of(z))

    for kw, msg in (({"T": 2049}, "trees"), ({"depth": 6}, "depth"), ({"n_bg": 0}, "background"),
                    ({"n_bg": 2, "bw_ld": 1}, "background")):
        with pytest.raises(Exception, match=msg):
            launch(**kw)
    torch.cuda.synchronize(dev)
    # and the explainer refuses the same on the way in
    ens, Xs, Bs = TC.oracle_case(3, 3)
    with pytest.raises(ValueError):
        _explainer(ens, Bs[:0], dev)
    with pytest.raises(ValueError):
        _explainer(TC.random_ensemble(3, 6, 2, 0), Bs, dev)
