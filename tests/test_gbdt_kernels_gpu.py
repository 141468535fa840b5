"""Every K11 GBDT kernel (csrc/kernels/gbdt.hip) on its own against exact oracles.

test_gbdt_gpu.py compares whole fits, where a wrong value shows only if it flips an arg-max on
Gaussian data at the default parameters.  Here each kernel runs on crafted state (_gbdt_state.py):
every histogram entry, every partition output, every split decision (gains bitwise, fp64 with
contraction off) and every margin is compared with numpy -- np.array_equal / torch.equal
throughout; the one tolerance of the family stays in test_gbdt_gpu.py (gbdt_grad against libm)."""
import numpy as np
import pytest
import torch

import _gbdt_state as S
from fraud_detection_amd.ops import gbdt as gb
from fraud_detection_amd.ops import reference_gbdt as R
from fraud_detection_amd.ops.native import native, ptr, stream_of

pytestmark = pytest.mark.gpu

VARIANTS = [0, 1, 2, 3]  # lockstep, rotated, split, lane (the default)


@pytest.fixture
def hist_variant():
    m = native()

    def use(v):
        m.set_gbdt_hist_variant(v)

    try:
        yield use
    finally:
        m.set_gbdt_hist_variant(-1)


def _blocks():
    return int(native().gbdt_hist_blocks())


def _check_hist(st, dev, flush_rows=0):
    got = S.run_hist(st, dev, flush_rows)
    exp = S.to_dev(st.hist_oracle().reshape(-1), dev)
    if not torch.equal(got, exp):
        bad = torch.nonzero(got != exp).flatten()
        e = int(bad[0])
        node, r = divmod(e, S.HIST_ENTRIES)
        raise AssertionError(f"{bad.numel()} histogram words differ; first: node {node} feature {r // 512} "
                             f"bin {(r % 512) // 2} {'gh'[r % 2]}: got {int(got[e])} expected {int(exp[e])}")


# ---- gbdt_hist + reduce -------------------------------------------------------------------------
L0_ROWS = {"1": lambda B: 1, "127": lambda B: 127, "128": lambda B: 128, "129": lambda B: 129, "B-1": lambda B: B - 1,
           "B": lambda B: B, "B+1": lambda B: B + 1, "4B+3": lambda B: 4 * B + 3}


@pytest.mark.parametrize("nkey", list(L0_ROWS))
@pytest.mark.parametrize("var", VARIANTS)
def test_hist_level0_every_entry(dev, hist_variant, var, nkey):
    """The root histogram, every (feature, bin, g|h) word; features >= d and the other levels stay 0."""
    hist_variant(var)
    n = L0_ROWS[nkey](_blocks())
    for d in (1, 4, 29, 30):
        nb = np.array([(1, 2, 256, 37)[f % 4] for f in range(d)], np.int32)
        _check_hist(S.level_state(0, [n], d=d, nbins=nb, seed=n + d), dev)


@pytest.mark.parametrize("where", ["start", "middle", "end", "empty"])
@pytest.mark.parametrize("var", VARIANTS)
def test_hist_level0_hole(dev, hist_variant, var, where):
    """Level 0 walks the table around a hole of rows (a cross-validation fold's validation block)."""
    hist_variant(var)
    B = _blocks()
    for n_fit, d in ((B + 1, 30), (4 * B + 3, 4), (130, 29)):
        at = {"start": 0, "middle": n_fit // 3, "end": n_fit, "empty": n_fit // 2}[where]
        ln = 0 if where == "empty" else 777
        # the hole's rows carry extreme gradients: adding any of them would show
        def gh(rng, nt, at=at, ln=ln):
            q = np.stack([rng.integers(-100, 101, nt), rng.integers(0, 200, nt)], 1).astype(np.int16)
            q[at:at + ln] = (-(1 << 14), 1 << 14)
            return q
        _check_hist(S.level_state(0, [n_fit], d=d, hole=(at, ln), gh=gh, seed=n_fit), dev)


def _level6_sizes():
    s = np.zeros(64, np.int64)
    s[0:2] = (12000, 9010)      # the right one is built: 9010 rows
    s[2:4] = (2, 9)             # three tiny built nodes in a row ...
    s[4:6] = (5, 1)
    s[6:8] = (3, 8)
    s[8:10] = (10000, 14000)    # ... then the head of a big one
    s[10:12] = (0, 0)           # an empty sibling pair
    s[12:14] = (0, 50)          # an empty built node
    s[14:16] = (40, 40)         # equal siblings: the left one is built
    s[62:64] = (7, 3)
    return s


LEVEL_CASES = {
    "l1_equal": (1, [5000, 5000]),
    "l1_empty_built": (1, [0, 9000]),
    "l1_tiny": (1, [3, 2]),
    "l3": (3, [0, 1, 5000, 0, 3, 3, 40000, 1]),
    "l3_perm": (3, [40000, 1, 3, 3, 0, 5000, 1, 0]),
    "l3_empty_pair": (3, [0, 0, 6000, 7000, 0, 0, 1, 1]),
    "l6": (6, _level6_sizes()),
}


def _situations(level, sizes, B):
    """Which of the situations the level tests must contain occur for these sizes (gc = sizes)."""
    sizes = np.asarray(sizes, np.int64)
    built = S.built_mask(level, sizes)
    chunk, blocks = S.hist_blocks_touching(sizes, built, B)
    out = set()
    for k in range(0, len(sizes), 2):
        a, b = int(sizes[k]), int(sizes[k + 1])
        if a == 0 and b == 0:
            out.add("empty_pair")
        elif min(a, b) == 0:
            out.add("empty_built")
        elif a == b:
            assert built[k] and not built[k + 1]
            out.add("equal_siblings")
    total = int(sizes[built].sum())
    if 0 < total < B:
        assert chunk == 1
        out.add("chunk1_idle_blocks")
    ks = sorted(blocks)
    for i, k in enumerate(ks):  # block b: the tail of a big node, >= 2 whole tiny nodes, the head of the next
        b = blocks[k][1]
        if blocks[k][0] == b:
            continue
        inside = [j for j in ks[i + 1:] if blocks[j] == (b, b)]
        after = [j for j in ks[i + 1:] if blocks[j][0] == b and blocks[j][1] > b]
        if len(inside) >= 2 and after:
            out.add("straddle")
    return out


def test_hist_level_cases_cover_the_situations(dev):
    seen = set()
    for level, sizes in LEVEL_CASES.values():
        seen |= _situations(level, sizes, _blocks())
    assert seen == {"empty_pair", "empty_built", "equal_siblings", "chunk1_idle_blocks", "straddle"}, seen


@pytest.mark.parametrize("case", list(LEVEL_CASES))
@pytest.mark.parametrize("var", VARIANTS)
def test_hist_levels_crafted_sizes(dev, hist_variant, var, case):
    """Levels 1, 3 and 6: built nodes carry their exact histogram, derived nodes and every other
    word stay zero -- empty nodes and pairs, equal siblings, a block range across several nodes."""
    hist_variant(var)
    level, sizes = LEVEL_CASES[case]
    nb = np.array([(256, 2, 1, 100)[f % 4] for f in range(30)], np.int32)
    _check_hist(S.level_state(level, sizes, d=30, nbins=nb, seed=level), dev)
    _check_hist(S.level_state(level, sizes, d=5, seed=level + 1), dev)


GC_CASES = {
    "l1_left": (1, [6000, 4000], [9000, 9500]),           # locally larger, globally smaller: built
    "l1_right": (1, [3000, 5000], [9000, 8000]),
    "l1_global_tie": (1, [4000, 10], [7000, 7000]),        # a global tie builds the left one
    "l3": (3, [500, 20, 0, 3000, 700, 700, 1, 0], [600, 900, 50, 40, 800, 700, 5, 5]),
}


@pytest.mark.parametrize("case", list(GC_CASES))
@pytest.mark.parametrize("var", VARIANTS)
def test_hist_build_rule_uses_global_counts(dev, hist_variant, var, case):
    """Under data parallelism gcnt (all ranks) decides which sibling is built, not the local sizes."""
    hist_variant(var)
    level, sizes, gc = GC_CASES[case]
    st = S.level_state(level, sizes, gc=gc, d=30, seed=7)
    local, glob = S.built_mask(level, sizes), st.built
    assert (local != glob).any()  # the case does separate the two rules
    for k in range(0, len(sizes), 2):
        assert glob[k] != glob[k + 1]
    _check_hist(st, dev)


def _gh_const(g, h):
    return lambda rng, nt: np.tile(np.array([[g, h]], np.int16), (nt, 1))


def _gh_alternating(rng, nt):
    q = np.empty((nt, 2), np.int16)
    q[0::2] = (-(1 << 14), 1 << 14)
    q[1::2] = (1 << 14, 0)
    return q


@pytest.mark.parametrize("gh", ["neg_max", "pos_zero_h", "alternating"])
@pytest.mark.parametrize("var", VARIANTS)
def test_hist_extreme_gradients(dev, hist_variant, var, gh):
    """(g, h) at the ends of their ranges, 65,537 rows in one node: the borrow / carry between the
    packed halves of the LDS words, with one- and two-bin features taking every row."""
    hist_variant(var)
    fn = {"neg_max": _gh_const(-(1 << 14), 1 << 14), "pos_zero_h": _gh_const(1 << 14, 0), "alternating": _gh_alternating}[gh]
    nb = np.array([(1, 2, 256)[f % 3] for f in range(30)], np.int32)
    _check_hist(S.level_state(0, [65537], d=30, nbins=nb, gh=fn), dev)
    _check_hist(S.level_state(1, [65537, 70000], d=30, nbins=nb, gh=fn), dev)


@pytest.mark.parametrize("flush", [1, 1000])
@pytest.mark.parametrize("var", VARIANTS)
def test_hist_multiple_flushes_equal_one(dev, hist_variant, var, flush):
    """Several flushes of a block into its slot (the first stores over the poison, the later add)."""
    hist_variant(var)
    B = _blocks()
    # > 1 flush per block either way (at 1000 rows per flush that takes ~1M rows: 4 features keep it cheap)
    big = 2 * 1000 * B + 17 if flush == 1000 else 4 * B + 3
    for st in (S.level_state(0, [big], d=4 if flush == 1000 else 30, seed=1),
               S.level_state(3, [0, 1, 5000, 0, 3, 3, 40000, 1], d=30, seed=2),
               S.level_state(6, _level6_sizes(), d=30, seed=3)):
        if st.level != 3:  # (level 3 builds 4 rows in all: one row, one flush per block)
            chunk, _ = S.hist_blocks_touching(st.sizes, st.built, B // 2 if var == 1 else B)
            assert chunk > flush or st.level == 6 and flush == 1000
        _check_hist(st, dev, flush_rows=flush)


# ---- gbdt_split ---------------------------------------------------------------------------------
GS, HS = R.grad_scales(1.0)
GINV, HINV = 1.0 / GS, 1.0 / HS


def _cuts(rng, d):
    c = np.sort(rng.normal(size=(d, 256)).astype(np.float32), axis=1)
    c[:, 255] = np.inf
    return c


def _split_both(dev, hist, gcnt, level, d, nbins, cuts, lam, mcw, gamma, ginv=GINV, hinv=HINV):
    ref = S.split_level_oracle(hist, gcnt, level, d, nbins, cuts, ginv, hinv, lam, mcw, gamma)
    got = S.run_split(hist, gcnt, level, d, nbins, cuts, ginv, hinv, lam, mcw, gamma, dev)
    S.assert_split_equal(got, ref, level)
    return ref


def _level_hists(rng, level, d, nbins, hmax, gmax, empty=()):
    """Histogram tensor [2^(level+1) - 1, 30, 256, 2] for a split at `level`: one sibling of every
    pair is built (written), the other derived -- its histogram D exists only as parent - sibling,
    the parent being written as S + D.  Returns (hist, gcnt)."""
    ni = (2 << level) - 1
    h0, nn = S.heap_first(level), 1 << level
    hist = np.zeros((ni, S.MAX_FEAT, 256, 2), np.int64)
    gcnt = np.zeros(2 * ni + 1, np.int64)
    gcnt[h0:h0 + nn] = rng.integers(0, 1000, nn)
    if level == 0:
        hist[0] = S.hist_with_totals(rng, d, nbins, int(rng.integers(-gmax, gmax)), int(rng.integers(1, hmax)), gmax)
        return hist, gcnt
    for k in range(0, nn, 2):
        if k in empty:
            continue
        if k % 4 == 0:
            gcnt[h0 + k + 1] = gcnt[h0 + k]  # ties build the left one
        tot = lambda: (int(rng.integers(-gmax, gmax)), int(rng.integers(1, hmax)))  # noqa: E731
        a = S.hist_with_totals(rng, d, nbins, *tot(), gmax)
        b = S.hist_with_totals(rng, d, nbins, *tot(), gmax)
        built = S.built_mask(level, gcnt[h0:h0 + nn])
        hist[h0 + k + (0 if built[k] else 1)] = a
        hist[(h0 + k - 1) >> 1] = a + b
    return hist, gcnt


@pytest.mark.parametrize("lam", [0.0, 1.0, 10.0])
@pytest.mark.parametrize("d", [1, 17, 30])
@pytest.mark.parametrize("level", [0, 1, 5])
def test_split_random_histograms(dev, level, d, lam):
    """Every node of a level: built and derived (parent - sibling, stored exactly), mixed 1 / 2 /
    256-bin features, an empty pair, min_child_weight 0 and 1."""
    rng = np.random.default_rng(100 * level + d)
    nb = np.array([(256, 1, 2, 77, 256)[f % 5] for f in range(d)], np.int32)
    cuts = _cuts(rng, d)
    for mcw in (0.0, 1.0):
        hist, gcnt = _level_hists(rng, level, d, nb, 1 << 30, 1 << 24, empty=(2,) if level == 5 else ())
        ref = _split_both(dev, hist, gcnt, level, d, nb, cuts, lam, mcw, 0.0)
        if level:
            h0, nn = S.heap_first(level), 1 << level
            derived = ~S.built_mask(level, gcnt[h0:h0 + nn])
            assert derived.sum() == nn // 2 and np.any(ref[0][h0:h0 + nn][derived] != 0)
        if d > 1 and 256 in nb[1:]:
            assert (ref[1] >= 0).any()  # some node of the level does split


def test_split_ties_lowest_feature_then_lowest_bin(dev):
    rng = np.random.default_rng(5)
    for d in (17, 30):  # 17+: a wave's second feature ties with its first
        nb = np.full(d, 64, np.int32)
        hist = np.zeros((1, S.MAX_FEAT, 256, 2), np.int64)
        one = S.hist_with_totals(rng, 1, nb[:1], 12345, 1 << 22, 1 << 18)[0]
        hist[0, :d] = one
        ref = _split_both(dev, hist, np.zeros(3, np.int64), 0, d, nb, _cuts(rng, d), 1.0, 1.0, 0.0)
        assert ref[1][0] == 0
    # equal gains in bins 0 .. 7 (empty bins between two mirrored ones: the candidates sit in two
    # lanes of the scanning wave), also in the last feature
    for d in (1, 2, 18):
        nb = np.full(d, 9, np.int32)
        hist = np.zeros((1, S.MAX_FEAT, 256, 2), np.int64)
        hist[0, :d, 0], hist[0, :d, 8] = (4 << 14, 2 << 16), (-(4 << 14), 2 << 16)
        if d > 1:  # the earlier features gain nothing: everything in one bin
            hist[0, :d - 1, 0], hist[0, :d - 1, 8] = (0, 4 << 16), (0, 0)
        ref = _split_both(dev, hist, np.zeros(3, np.int64), 0, d, nb, _cuts(rng, d), 1.0, 1.0, 0.0)
        assert (ref[1][0], ref[2][0]) == (d - 1, 0) and ref[4][0] > 1e-6


@pytest.mark.parametrize("lam", [0.0, 1.0])
def test_split_all_mass_in_last_bin(dev, lam):
    rng = np.random.default_rng(6)
    d = 4
    nb = np.array([256, 2, 1, 9], np.int32)
    hist = np.zeros((1, S.MAX_FEAT, 256, 2), np.int64)
    for f in range(d):
        hist[0, f, nb[f] - 1] = (-(7 << 14), 5 << 16)
    for mcw in (0.0, 1.0):
        ref = _split_both(dev, hist, np.zeros(3, np.int64), 0, d, nb, _cuts(rng, d), lam, mcw, 0.0)
        assert ref[1][0] == -1 and ref[5][1] == (-(7 << 14), 5 << 16) and ref[5][2] == (0, 0)


@pytest.mark.parametrize("side", ["left", "right"])
def test_split_child_weight_exactly_at_the_minimum(dev, side):
    """HL == min_child_weight (HR ==) exactly -- hscale is a power of two -- is a valid split."""
    rng = np.random.default_rng(7)
    mcw = 8.0
    small, big = (-(3 << 14), int(mcw * HS)), (5 << 14, int(24 * HS))
    hist = np.zeros((1, S.MAX_FEAT, 256, 2), np.int64)
    hist[0, 0, 0], hist[0, 0, 1] = (small, big) if side == "left" else (big, small)
    nb = np.array([2], np.int32)
    ref = _split_both(dev, hist, np.zeros(3, np.int64), 0, 1, nb, _cuts(rng, 1), 1.0, mcw, 0.0)
    assert ref[1][0] == 0 and ref[2][0] == 0
    child = ref[5][1] if side == "left" else ref[5][2]
    assert child[1] * HINV == mcw
    # one quantum less on that side: below the minimum, no split
    hist[0, 0, 0 if side == "left" else 1, 1] -= 1
    ref = _split_both(dev, hist, np.zeros(3, np.int64), 0, 1, nb, _cuts(rng, 1), 1.0, mcw, 0.0)
    assert ref[1][0] == -1


def test_split_gamma_at_and_one_ulp_above_the_best_gain(dev):
    rng = np.random.default_rng(8)
    d = 6
    nb = np.full(d, 256, np.int32)
    cuts = _cuts(rng, d)
    hist, gcnt = _level_hists(rng, 1, d, nb, 1 << 28, 1 << 24)
    base = _split_both(dev, hist, gcnt, 1, d, nb, cuts, 1.0, 1.0, 0.0)
    k = int(np.argmax(base[4]))
    g = float(base[4][k])
    assert g > 1e-6
    at = _split_both(dev, hist, gcnt, 1, d, nb, cuts, 1.0, 1.0, g)
    assert at[1][k] >= 0 and at[4][k] == g
    above = _split_both(dev, hist, gcnt, 1, d, nb, cuts, 1.0, 1.0, float(np.nextafter(g, np.inf)))
    assert above[1][k] == -1 and above[4][k] == 0.0


def test_split_gain_not_above_1e_6(dev):
    """A best gain in (0, 1e-6] does not split (xgboost's kRtEps)."""
    rng = np.random.default_rng(9)
    hist = np.zeros((1, S.MAX_FEAT, 256, 2), np.int64)
    hist[0, 0, 0], hist[0, 0, 1] = (1000, 1000 << 16), (1400, 1000 << 16)  # (400 / 2^14)^2 / 2000 = 2.98e-7
    nb = np.array([2], np.int32)
    g = R.best_split(hist[0, :1], nb, GINV, HINV, 0.0, 1.0)[0]
    assert 0.0 < g <= 1e-6
    ref = _split_both(dev, hist, np.zeros(3, np.int64), 0, 1, nb, _cuts(rng, 1), 0.0, 1.0, 0.0)
    assert ref[1][0] == -1 and ref[4][0] == 0.0


@pytest.mark.parametrize("lam", [0.0, 1.0, 10.0])
def test_split_sums_around_2_pow_40(dev, lam):
    rng = np.random.default_rng(10)
    d = 17
    nb = np.array([(256, 2, 31)[f % 3] for f in range(d)], np.int32)
    hist = np.zeros((3, S.MAX_FEAT, 256, 2), np.int64)
    gcnt = np.array([0, 5, 5, 0, 0, 0, 0], np.int64)
    a = S.hist_with_totals(rng, d, nb, -(1 << 40) + 999, (1 << 40) + 12345, 1 << 38)
    b = S.hist_with_totals(rng, d, nb, (1 << 39) + 7, (1 << 40) - 3, 1 << 38)
    hist[1], hist[0] = a, a + b
    _split_both(dev, hist, gcnt, 0, d, nb, _cuts(rng, d), lam, 1.0, 0.0)
    ref = _split_both(dev, hist, gcnt, 1, d, nb, _cuts(rng, d), lam, 1.0, 0.0)
    assert np.array_equal(ref[0][2], b)


@pytest.mark.parametrize("mcw", [0.0, 1.0])
def test_split_lambda_zero_degenerate_terms(dev, mcw):
    """reg_lambda = 0: leading empty bins (0/0 on the left), a bin range with h = 0, g != 0 (G^2/0),
    an empty node and a node whose whole H is 0 -- the term with a denominator <= 0 counts as 0."""
    rng = np.random.default_rng(11)
    d = 3
    nb = np.array([8, 8, 2], np.int32)
    hist = np.zeros((3, S.MAX_FEAT, 256, 2), np.int64)
    gcnt = np.array([0, 1, 1, 0, 0, 0, 0], np.int64)
    lead = np.zeros((S.MAX_FEAT, 256, 2), np.int64)
    lead[0, 3:8] = [(-(9 << 14), 3 << 16), (2 << 14, 1 << 16), (5 << 14, 2 << 16), (-(1 << 14), 4 << 16), (1 << 14, 1 << 16)]
    lead[1, 0:3] = [(4 << 14, 0), (-(2 << 14), 0), (1 << 14, 0)]             # h = 0, g != 0
    lead[1, 3:8] = [(-(8 << 14), 3 << 16), (1 << 14, 2 << 16), (0, 2 << 16), (1 << 14, 2 << 16), (1 << 14, 2 << 16)]
    lead[2, 0], lead[2, 1] = (-(1 << 14), 5 << 16), (-(1 << 14), 6 << 16)
    assert len({tuple(lead[f].sum(0)) for f in range(d)}) == 1
    zero_h = np.zeros_like(lead)                                            # a node with H = 0, G != 0
    zero_h[:d, 0, 0], zero_h[:d, 1, 0] = 3 << 14, -(1 << 14)
    hist[0] = lead
    ref = _split_both(dev, hist, gcnt, 0, d, nb, _cuts(rng, d), 0.0, mcw, 0.0)
    assert np.isfinite(ref[4]).all() and ref[1][0] >= 0
    hist[0], hist[1] = lead + zero_h, lead       # level 1: node 1 built, node 2 = zero_h derived
    ref = _split_both(dev, hist, gcnt, 1, d, nb, _cuts(rng, d), 0.0, mcw, 0.0)
    assert ref[1][1] == -1 and np.array_equal(ref[0][2], zero_h)
    hist[0], hist[1] = lead, lead                # node 2 derived and empty
    ref = _split_both(dev, hist, gcnt, 1, d, nb, _cuts(rng, d), 0.0, mcw, 0.0)
    assert ref[1][1] == -1 and not ref[0][2].any()
    _split_both(dev, hist, gcnt, 1, d, nb, _cuts(rng, d), 0.0, mcw, 2.0)


# ---- gbdt_partition -------------------------------------------------------------------------------
def _part_sizes(rng, level, n, pattern):
    nn = 1 << level
    if pattern == "tiny_next_to_big" and nn > 1:
        w = np.where(np.arange(nn) % 3 == 0, 1000.0, 1.0)
    else:
        w = np.ones(nn)
    s = rng.multinomial(n, w / w.sum())
    if nn > 2 and n > 8:
        s[0] += s[1]
        s[1] = 0  # an empty node in the level
    return s


def _part_tree(rng, st, pattern):
    ni = (2 << st.level) - 1
    feat = rng.integers(0, st.d, ni).astype(np.int32)
    binv = np.array([rng.integers(0, max(1, int(st.nbins[f]) - 1)) for f in feat], np.int32)
    h0, nn = S.heap_first(st.level), 1 << st.level
    sel = slice(h0, h0 + nn)
    if pattern == "no_split":
        feat[sel], binv[sel] = -1, 255
    elif pattern == "all_right":      # bins > -1: every row goes right
        binv[sel] = -1
    elif pattern == "all_left":
        binv[sel] = 255
    elif pattern == "tiny_next_to_big" and nn > 1:
        feat[h0 + 1], binv[h0 + 1] = -1, 255  # a pass-through among the splits
    return feat, binv


PART_NAMES = ("ridx_out", "nid_out", "flag", "seg", "node_r", "gcnt")


@pytest.mark.parametrize("pattern", ["mixed", "no_split", "all_right", "all_left", "tiny_next_to_big"])
@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 20001])
@pytest.mark.parametrize("level", [0, 2, 5])
def test_partition_matches_stable_oracle(dev, monkeypatch, level, n, pattern):
    """ridx / nid of the children, their segments and counts, node_r and the go-right flags -- with
    the fit's block count and again with 3 and 1 blocks (the result does not depend on it)."""
    rng = np.random.default_rng(1000 * level + n)
    holes = [None] + ([(n // 2, 333), (0, 5), (n, 9)] if level == 0 else [])
    default_blocks = gb.PART_BLOCKS  # the fit's own grid, also for n = 1
    assert default_blocks >= 1024
    for hole in holes:
        st = S.level_state(level, _part_sizes(rng, level, n, pattern), d=9, hole=hole, seed=n,
                           nbins=np.array([256, 2, 1, 16, 256, 3, 100, 2, 256], np.int32), depth=level + 1)
        feat, binv = _part_tree(rng, st, pattern)
        ref = S.partition_level(st, feat, binv)
        for blocks in (default_blocks, 3, 1):
            monkeypatch.setattr(gb, "PART_BLOCKS", blocks)
            got = S.run_partition(st, feat, binv, dev)
            for name, g, r in zip(PART_NAMES, got, ref):
                assert np.array_equal(g, r), (name, blocks, hole)
        monkeypatch.setattr(gb, "PART_BLOCKS", default_blocks)


# ---- gbdt_leaf -----------------------------------------------------------------------------------
@pytest.mark.parametrize("lam", [0.0, 1.0])
@pytest.mark.parametrize("mcw", [0.0, 1.0, 2.5])
@pytest.mark.parametrize("depth", [1, 5, 7])
def test_leaf_kernel_bitwise(dev, depth, mcw, lam):
    rng = np.random.default_rng(depth)
    nl, ni = 1 << depth, (1 << depth) - 1
    ng = rng.integers(-(1 << 40), 1 << 40, 2 * nl - 1)
    nh = rng.integers(0, 1 << 40, 2 * nl - 1)
    edge = int(mcw * HS)
    crafted = [edge - 1, edge, edge + 1, 0, 1]  # H below / at / above the minimum, H = 0, one quantum
    for i in range(nl):
        if i % 2 == 0:
            nh[ni + i] = max(0, crafted[(i // 2) % len(crafted)])
    ref = R.leaf_values(ng, nh, depth, GINV, HINV, lam, mcw, 0.3)
    out = torch.full((nl,), 9.0, dtype=torch.float32, device=dev)
    ngd, nhd = S.to_dev(ng, dev), S.to_dev(nh, dev)
    native().gbdt_leaf(ptr(ngd), ptr(nhd), depth, GINV, HINV, lam, mcw, 0.3, ptr(out), stream_of(out))
    assert np.array_equal(out.cpu().numpy().view(np.uint32), ref.view(np.uint32))
    assert np.isfinite(ref).all() and (ref[nh[ni:] == 0] == 0).all()


# ---- gbdt_transpose ------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 30])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_transpose_kernel(dev, n, d):
    rng = np.random.default_rng(n)
    bins = S.random_bins(rng, n, d, np.full(d, 256))
    ref, ldt = S.transpose_bins(bins, d)
    out = torch.full((d * ldt,), 0xEE, dtype=torch.uint8, device=dev)
    bd = S.to_dev(bins, dev)
    native().gbdt_transpose(ptr(bd), n, d, ptr(out), ldt, stream_of(bd))
    got = out.cpu().numpy().reshape(d, ldt)
    assert np.array_equal(got[:, :n], ref.reshape(d, ldt)[:, :n])  # pad rows up to ldt are not compared


# ---- gbdt_margin<GRAD> and gbdt_hist_l0_fused ------------------------------------------------------
def _crafted_tree(rng, bins, d, depth):
    """A heap tree whose split bins come from the data (bin == split bin occurs and goes left),
    with pass-through nodes and a split at bin 255's neighbour."""
    ni, nl = (1 << depth) - 1, 1 << depth
    feat = rng.integers(0, d, ni).astype(np.int32)
    binv = np.array([bins[rng.integers(0, bins.shape[0]), f] for f in feat], np.int32)
    passthrough = rng.random(ni) < 0.25
    if ni > 1:
        passthrough[0] = False
        passthrough[1] = True
    feat[passthrough], binv[passthrough] = -1, 255
    if ni > 2 and d > 1:
        feat[2], binv[2] = 0, 254  # only bin 255 of feature 0 goes right
    leaf = rng.normal(scale=0.3, size=nl).astype(np.float32)
    return feat, binv, leaf


MARGIN_ROWS = {"1": lambda B: 1, "1023": lambda B: 1023, "1024": lambda B: 1024, "1025": lambda B: 1025,
               "3B+1": lambda B: 3 * B + 1}


@pytest.mark.parametrize("nkey", list(MARGIN_ROWS))
@pytest.mark.parametrize("depth", [1, 5, 7])
def test_margin_walk_and_fused_level0(dev, depth, nkey):
    """gbdt_margin<GRAD> equals the oracle's walk on the bins exactly; the fused level-0 launch
    (FDX_GBDT_FUSE_MARGIN) equals gbdt_margin<GRAD> followed by gbdt_hist level 0 bit for bit --
    margins (hole rows too), (g, h) words and the root histogram, at both flush settings."""
    _margin_fused_case(dev, depth, MARGIN_ROWS[nkey](_blocks()))


def test_fused_level0_many_steps_per_block(dev):
    """The sizes above give a block a handful of rows.  The fused kernel works in steps of 1024
    root positions per block and flushes every flush_rows: 1100 B + 7 rows put more than one step
    (and, at 1000 rows per flush, more than one flush) into every block."""
    B = _blocks()
    n_fit = 1100 * B + 7
    assert -(-n_fit // B) > 1024
    _margin_fused_case(dev, 5, n_fit)


def _margin_fused_case(dev, depth, n_fit):
    m = native()
    rng = np.random.default_rng(depth * 10000 + n_fit)
    d, spw = 11, 3.0
    gs, hs = R.grad_scales(spw)
    nb = np.array([256, 2, 256, 5, 1, 256, 17, 256, 3, 256, 64], np.int32)
    for hole in ((0, 0), (n_fit // 2, 300)):
        st = S.level_state(0, [n_fit], d=d, nbins=nb, hole=hole, seed=n_fit + depth, depth=1)
        N = st.n_table
        st.bins[rng.integers(0, N, max(1, N // 8)), 0] = 255
        feat, binv, leaf = _crafted_tree(rng, st.bins, d, depth)
        m0 = rng.normal(scale=2.0, size=N).astype(np.float32)
        y = (rng.random(N) < 0.3).astype(np.uint8)
        walk = R.predict_margin_bins(st.bins, feat[None], binv[None], leaf[None], depth, 0.0)
        exp_margin = (m0 + walk).astype(np.float32)
        if n_fit > 1000 and depth > 1:
            assert (st.bins[:, 0] == 255).any() and (feat == -1).any()
            assert any((st.bins[:, f] == b).any() for f, b in zip(feat, binv) if f >= 0)
        bt, ldt = S.transpose_bins(st.bins, d)
        binsT, bins = S.to_dev(bt, dev), S.to_dev(st.bins, dev)
        fd, bd, ld, yd = S.to_dev(feat, dev), S.to_dev(binv, dev), S.to_dev(leaf, dev), S.to_dev(y, dev)
        seg, gcnt = S.to_dev(st.seg, dev), S.to_dev(st.gcnt, dev)
        ridx = S.to_dev(st.ridx, dev)
        # the two-launch form
        margin_a = S.to_dev(m0, dev)
        gh_a = torch.full((N, 2), -1, dtype=torch.int16, device=dev)
        m.gbdt_margin(ptr(binsT), ldt, N, ptr(fd), ptr(bd), ptr(ld), depth, ptr(margin_a), ptr(yd), spw, gs, hs,
                      ptr(gh_a), stream_of(bins))
        assert np.array_equal(margin_a.cpu().numpy().view(np.uint32), exp_margin.view(np.uint32))
        # ... whose gradients are gbdt_grad's of the new margin, bit for bit (same device function)
        gh_g = torch.empty((N, 2), dtype=torch.int16, device=dev)
        m.gbdt_grad(ptr(margin_a), ptr(yd), N, spw, gs, hs, ptr(gh_g), stream_of(bins))
        assert torch.equal(gh_a, gh_g)
        margin_ng = S.to_dev(m0, dev)  # GRAD = false: the same margins, gh untouched
        m.gbdt_margin(ptr(binsT), ldt, N, ptr(fd), ptr(bd), ptr(ld), depth, ptr(margin_ng), ptr(yd), spw, gs, hs, 0,
                      stream_of(bins))
        assert torch.equal(margin_ng, margin_a)
        st_a = S.LevelState(0, 1, d, n_fit, st.hole, nb, st.bins, gh_a.cpu().numpy(), st.ridx, st.nid, st.seg,
                            st.gcnt, st.sizes)
        hist_exp = S.to_dev(st_a.hist_oracle().reshape(-1), dev)
        for flush in (0, 1000):
            hist_a = torch.zeros(S.HIST_ENTRIES, dtype=torch.int64, device=dev)
            m.gbdt_hist(ptr(bins), ptr(gh_a), ptr(ridx), ptr(seg), ptr(gcnt), 0, d, ptr(hist_a), ptr(S.slots_for(dev)),
                        stream_of(bins), flush, hole[0], hole[1])
            assert torch.equal(hist_a, hist_exp)
            margin_f = S.to_dev(m0, dev)
            gh_f = torch.full((N, 2), -1, dtype=torch.int16, device=dev)
            hist_f = torch.zeros(S.HIST_ENTRIES, dtype=torch.int64, device=dev)
            m.gbdt_hist_l0_fused(ptr(bins), ptr(gh_f), ptr(seg), ptr(gcnt), d, ptr(hist_f), ptr(S.slots_for(dev)),
                                 stream_of(bins), flush, hole[0], hole[1], ptr(fd), ptr(bd), ptr(ld), depth,
                                 ptr(margin_f), ptr(yd), spw, gs, hs)
            torch.cuda.synchronize()
            assert torch.equal(margin_f, margin_a), (hole, flush)
            assert torch.equal(gh_f, gh_a), (hole, flush)
            assert torch.equal(hist_f, hist_a), (hole, flush)


# ---- the FDX_GBDT_FUSE_MARGIN switch end to end ----------------------------------------------------
def _fit_data(n, d, seed, dev):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, d)).astype(np.float32)
    if d > 1:
        X[:, 1] = np.round(X[:, 1] * 3) / 3
    logit = 1.2 * X[:, 0] - 1.5 * (X[:, min(1, d - 1)] > 0.3) - 1.0
    y = (rng.random(n) < 1 / (1 + np.exp(-logit))).astype(np.uint8)
    return torch.from_numpy(X).to(dev), torch.from_numpy(y).to(dev), X, y


def _same_trees(a, b):
    for k in ("feat", "bin", "thr", "gain", "leaf"):
        x, y = getattr(a, k), getattr(b, k)
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), k


@pytest.mark.parametrize("hole", [None, (5000, 3000), (0, 100), (19900, 100)])
def test_fuse_margin_switch_bitwise(dev, monkeypatch, hole):
    """FDX_GBDT_FUSE_MARGIN=1 (the deferred walk + gbdt_hist_l0_fused) against the default launch
    sequence: 6 rounds at depth 5, every tree array and the returned margins -- hole rows and the
    last, undeferred round included."""
    Xd, yd, X, y = _fit_data(20_000, 12, 3, dev)
    p = gb.GBDTParams(n_estimators=6, max_depth=5, scale_pos_weight=4.0)
    cuts = R.quantile_cuts(X, 256)
    bins = gb.bin_rows(Xd, *cuts)
    out = {}
    for flag in ("0", "1"):
        monkeypatch.setenv("FDX_GBDT_FUSE_MARGIN", flag)
        if hole is None:
            out[flag] = gb.fit(Xd, yd, p, cuts=cuts, return_margin=True, use_graph=False)
        else:
            out[flag] = gb.fit_binned(bins, yd, cuts, p, hole=hole, return_margin=True, use_graph=False)
    _same_trees(out["0"][0], out["1"][0])
    assert torch.equal(out["0"][1], out["1"][1])
    assert (out["0"][0].feat >= 0).any()


# ---- every round exact, given the device's own gradients ---------------------------------------------
def test_every_round_equals_oracle_on_device_gradients(dev):
    """Tree t of a device fit is the oracle's tree on the device's own quantised gradients of the
    margins after t trees: no tolerance for libm, no tree excepted."""
    T, depth, spw = 8, 5, 5.0
    Xd, yd, X, y = _fit_data(20_011, 12, 5, dev)
    p = gb.GBDTParams(n_estimators=T, max_depth=depth, scale_pos_weight=spw)
    cuts = R.quantile_cuts(X, 256)
    ens, margin = gb.fit(Xd, yd, p, cuts=cuts, return_margin=True)
    bins = gb.bin_rows(Xd, *cuts).cpu().numpy()
    assert np.array_equal(bins, R.bin_rows(X, *cuts))
    gs, hs = R.grad_scales(spw)
    n = X.shape[0]
    for t in range(T + 1):
        mt = gb.predict_margin(Xd, ens, n_trees=t)
        if t == T:
            assert torch.equal(mt, margin)
            break
        gh = torch.empty((n, 2), dtype=torch.int16, device=dev)
        native().gbdt_grad(ptr(mt), ptr(yd), n, spw, gs, hs, ptr(gh), stream_of(mt))
        q = gh.cpu().numpy().astype(np.int32)
        ref, _ = R.build_tree(bins, q, cuts[0], cuts[1], depth, p.reg_lambda, p.min_child_weight, p.gamma,
                              p.learning_rate, gs, hs)
        for k in ("feat", "bin", "thr", "gain", "leaf"):
            assert getattr(ref, k).tobytes() == getattr(ens, k)[t].tobytes(), (t, k)


# ---- parameter sweep: first tree, device against the CPU path ---------------------------------------
REG = [(0, 0, 0), (0, 1, 0), (1, 0, 0), (1, 1, 5), (10, 50, 0), (0, 0, 2)]


def _sweep_data(kind):
    rng = np.random.default_rng(len(kind))
    n, d, depth, spw, max_bins = 4000, 6, 5, 3.0, (2, 37)
    if kind == "d1":
        d = 1
    elif kind == "n3":
        n, depth = 3, 7
    elif kind == "n50":
        n, depth = 50, 7
    elif kind == "spw600":
        spw = 600.0
    X = rng.normal(size=(n, d)).astype(np.float32)
    y = (rng.random(n) < 1 / (1 + np.exp(-(1.5 * X[:, 0] - 1.0)))).astype(np.uint8)
    if kind == "const_feature":
        X[:, 2] = -3.5
    elif kind == "nonfinite":
        X[rng.random(n) < 0.1, 1] = np.nan
        X[rng.random(n) < 0.05, 1] = np.inf
        X[rng.random(n) < 0.05, 1] = -np.inf
        X[rng.random(n) < 0.3, 3] = np.nan
    elif kind == "labels0":
        y[:] = 0
    elif kind == "labels1":
        y[:] = 1
    elif kind in ("n3", "n50"):
        y[0], y[1] = 0, 1
    return X, y, depth, spw, max_bins


@pytest.mark.parametrize("kind", ["plain", "const_feature", "nonfinite", "labels0", "labels1", "d1", "n3", "n50",
                                  "spw600"])
@pytest.mark.parametrize("reg", REG, ids=lambda r: "l%g_w%g_g%g" % r)
def test_first_tree_parameter_sweep(dev, reg, kind):
    """reg_lambda, min_child_weight and gamma off their defaults, few bins, degenerate features and
    labels, nearly empty trees: the device's first tree and margins equal the CPU path's exactly."""
    lam, mcw, gamma = (float(v) for v in reg)
    X, y, depth, spw, max_bins = _sweep_data(kind)
    Xd, yd = torch.from_numpy(X).to(dev), torch.from_numpy(y).to(dev)
    for max_bin in max_bins:
        p = gb.GBDTParams(n_estimators=1, max_depth=depth, scale_pos_weight=spw, reg_lambda=lam,
                          min_child_weight=mcw, gamma=gamma, max_bin=max_bin)
        cuts = R.quantile_cuts(X, max_bin)
        ens, margin = gb.fit(Xd, yd, p, cuts=cuts, return_margin=True)
        ref, rmargin = gb.fit(torch.from_numpy(X), torch.from_numpy(y), p, cuts=cuts, return_margin=True)
        assert np.array_equal(ens.feat, ref.feat) and np.array_equal(ens.bin, ref.bin), max_bin
        assert np.array_equal(ens.thr, ref.thr), max_bin
        assert np.array_equal(ens.gain, ref.gain), max_bin
        assert np.array_equal(ens.leaf, ref.leaf), max_bin
        assert np.array_equal(margin.cpu().numpy(), rmargin.numpy()), max_bin


# ---- gbdt_bin --------------------------------------------------------------------------------------
NEG_NAN = np.array([0xFFC00001], np.uint32).view(np.float32)[0]


def _bin_case(rng, n, d):
    """Cuts with 0.0 and a denormal among them; values on the cuts, one ulp either side, +-inf, NaN
    of both signs, -0.0, denormals."""
    nbins = np.array([(256, 1, 2)[f % 3] for f in range(d)], np.int32)
    cuts = np.full((d, 256), np.inf, np.float32)
    X = np.empty((n, d), np.float32)
    for f in range(d):
        nb = int(nbins[f])
        c = np.unique(np.concatenate([rng.normal(size=2 * nb).astype(np.float32),
                                      np.array([0.0, 1e-40, -1e-40, 3e38, -3e38], np.float32)]))
        c = np.sort(rng.choice(c, nb - 1, replace=False)) if nb > 1 else c[:0]
        if nb == 2:
            c[:] = 0.0
        elif nb > 2 and not (c == 0.0).any():
            c[np.searchsorted(c, 0.0)] = 0.0
            c = np.sort(c)
        cuts[f, :nb - 1] = c
        fin = cuts[f, :max(nb - 1, 1)]
        fin = fin[np.isfinite(fin)] if np.isfinite(fin).any() else np.array([0.0], np.float32)
        pool = np.concatenate([fin, np.nextafter(fin, np.float32(np.inf)), np.nextafter(fin, np.float32(-np.inf)),
                               np.array([np.inf, -np.inf, np.nan, NEG_NAN, 0.0, -0.0, 1e-40, -1e-40, 1e-45, -1e-45,
                                         3.4e38, -3.4e38], np.float32),
                               rng.normal(size=8).astype(np.float32)]).astype(np.float32)
        X[:, f] = pool[rng.integers(0, len(pool), n)]
    return X, cuts, nbins


@pytest.mark.parametrize("layout", ["tail_of_nan_buffer", "view_of_32", "offset_one_float"])
@pytest.mark.parametrize("d", [1, 3, 4, 8, 12, 28, 29, 30])
def test_bin_kernel_layouts_and_edge_values(dev, d, layout):
    """Both load paths of gbdt_bin on every row layout: contiguous [n, d] rows at the end of a
    NaN-filled buffer, the pipeline's [:, :d] view of [n, 32] rows (vector loads), a base off by one
    float (scalar loads) -- exact against the oracle on cut-edge, non-finite and denormal values."""
    rng = np.random.default_rng(d)
    for n in (1, 31, 32, 33, 8191):
        X, cuts, nbins = _bin_case(rng, n, d)
        Xh = torch.from_numpy(X)
        if layout == "tail_of_nan_buffer":
            buf = torch.full(((n + 4) * d,), float("nan"), dtype=torch.float32, device=dev)
            Xd = buf[4 * d:].view(n, d)
            assert Xd.data_ptr() % 16 == 0
        elif layout == "view_of_32":
            buf = torch.full((n, 32), float("nan"), dtype=torch.float32, device=dev)
            Xd = buf[:, :d]
        else:
            buf = torch.full((n * d + 1,), float("nan"), dtype=torch.float32, device=dev)
            Xd = buf[1:].view(n, d)
            assert Xd.data_ptr() % 16 == 4
        Xd.copy_(Xh)
        assert np.array_equal(Xd.cpu().numpy(), X, equal_nan=True)
        got = gb.bin_rows(Xd, cuts, nbins).cpu().numpy()
        ref = R.bin_rows(X, cuts, nbins)
        assert np.array_equal(got, ref), (n, np.argwhere(got != ref)[:5])
        assert not got[:, d:].any()


# ---- gbdt_predict ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257])
@pytest.mark.parametrize("depth", [1, 4, 7])
def test_predict_kernel_crafted_ensembles(dev, depth, n):
    """Random heap trees (pass-through nodes, thresholds taken from the data so x == thr occurs and
    goes right), tree counts around the LDS chunk size c, strided rows, NaN / +-inf / -0.0 inputs."""
    rng = np.random.default_rng(depth * 1000 + n)
    d = 7
    ni, nl = (1 << depth) - 1, 1 << depth
    c = 12288 // (2 * ni + nl)
    T = c + 1
    X = rng.normal(size=(n, d)).astype(np.float32)
    X[:, 1] = np.round(X[:, 1] * 2) / 2
    special = np.array([np.nan, NEG_NAN, np.inf, -np.inf, -0.0, 0.0], np.float32)
    mask = rng.random((n, d)) < 0.2
    X[mask] = special[rng.integers(0, len(special), int(mask.sum()))]
    feat = rng.integers(-1, d, (T, ni)).astype(np.int32)
    thr = X[rng.integers(0, n, (T, ni)), np.maximum(feat, 0)].astype(np.float32)
    thr[rng.random((T, ni)) < 0.1] = 0.0
    thr[feat < 0] = np.inf
    leaf = rng.normal(scale=0.05, size=(T, nl)).astype(np.float32)
    ens = gb.TreeEnsemble(depth=depth, feat=feat, bin=np.zeros_like(feat), thr=thr, gain=np.zeros((T, ni)), leaf=leaf,
                          cuts=np.full((d, 256), np.inf, np.float32), nbins=np.ones(d, np.int32), base_score=0.3)
    assert (feat == -1).any() and np.isin(thr[np.isfinite(thr)], X).any()
    buf = torch.zeros((n, 37), dtype=torch.float32, device=dev)
    buf[:, 3:3 + d] = torch.from_numpy(X).to(dev)
    Xs = buf[:, 3:3 + d]
    Xc = torch.from_numpy(X).to(dev)
    for k in (0, 1, c - 1, c, c + 1):
        ref = R.predict_margin(X, feat[:k], thr[:k], leaf[:k], depth, ens.base_margin)
        for Xd in (Xc, Xs):
            got = gb.predict_margin(Xd, ens, n_trees=k).cpu().numpy()
            assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (k, Xd.stride())
