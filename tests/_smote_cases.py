"""Inputs and oracles of the SMOTE kernel tests (test_smote_oracle.py, test_smote_kernels_gpu.py):
smote.hip's smote_parents_kernel, every smote_generate_kernel instantiation and the two-level bucket
sort (smote_bucket_l1_kernel, smote_bucket_l2_kernel).

numpy only.  Nothing here calls ops/reference.py: Philox4x32-10 is written from its definition, the
draws from the header of smote.hip, the interpolation is ONE rounding of L / 65536 * d + a (the
kernel's fmaf) emulated through fp64 with round-to-odd, bf16 is rounded by integer arithmetic on the
fp32 bits and e4m3 by _stream_cases' exact quantiser.  The oracles assume no NaN, no infinity and no
fp32-subnormal result (test_smote_oracle.py asserts that of the cases).
"""
import functools

import numpy as np

from _stream_cases import BIAS_COL, LABEL_COL, NCOLS, bf16_bits, bf16_values, fp8_encode

SEED, COUNTER_BASE = 5, 7
FP8_SCALE = 4.0
HIGH_OFFSET = 2 ** 33 + 384  # a sample offset whose Philox counter (offset / 2 + lane) has high word 1
NFEAT = 30

# generate: the edge shape, and n_new at the boundaries of a lane group's 16 samples, a Philox
# half (64), a wave-iteration (128) and a 256-thread block (512)
GEN_M, GEN_MQ, GEN_QOFF, GEN_K = 37, 29, 8, 5
GEN_N = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 511, 512, 513, 5000)
GEN_N_VARIANTS = 5000
# (parents, affine): bf16 output-space parents, fp32 parents, fp32 parents mapped per sample
GEN_PARENTS = {"pbf16": ("bf16", False), "pf32": ("f32", False), "pf32aff": ("f32", True)}
KINDS = ("bf16", "f32", "fp8")
# the grid-stride sweep
SWEEP_M, SWEEP_MQ, SWEEP_K = 4096, 4000, 5
SWEEP_TAIL, SWEEP_STRIDE = 1024, 97
# one rounding, not two: rows of the sweep shape checked in full (see ROUNDING_N below)
ROUNDING_N = 131_072
# slices of one draw sequence
SLICES = ((0, 1280), (1280, 7296), (7296, 10_000))
PARENT_ROWS = (1, 7, 8, 9, 1000)

# bucket sort: (mq, k, n_new, sample_offset)
BUCKET_CASES = {
    "staged_and_unstaged": (2, 3, 49_152, 0),
    "all_unstaged": (2, 3, 70_001, 0),
    "fb7_partial_last_bin": (8000, 5, 1000, 0),
    "one_sample": (7, 8, 1, 0),
    "one_pick": (1, 1, 129, 0),
    "l1_block_full": (37, 3, 16_384, 0),
    "l1_block_plus_one": (37, 3, 16_385, 0),
    "existing_shape": (300, 5, 123_457, 384),
    "high_counter": (2, 3, 49_153, 2 ** 33 + 128),
}
BUCKET_PAIRS, STAGE_RECS, FINE_MAX = 8192, 8192, 128  # smote.hip kBucketPairs, kStageRecs, kFineMax


# ---- Philox4x32-10 -----------------------------------------------------------------------------
# Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3" (SC'11).  One round:
# (hi0, lo0) = M0 * c0, (hi1, lo1) = M1 * c2; c' = (hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0); the key
# is bumped by the Weyl constants between rounds.
PHILOX_M = (0xD2511F53, 0xCD9E8D57)
PHILOX_W = (0x9E3779B9, 0xBB67AE85)
_U32 = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """ctr: four uint32 arrays (or ints) c0..c3; key: two ints.  Returns the four output words."""
    c = [np.atleast_1d(np.asarray(x, dtype=np.uint64)) & np.uint64(_U32) for x in ctr]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & _U32, int(key[1]) & _U32
    m0, m1, sh, lo = np.uint64(PHILOX_M[0]), np.uint64(PHILOX_M[1]), np.uint64(32), np.uint64(_U32)
    for _ in range(10):
        p0, p1 = c[0] * m0, c[2] * m1  # 32 x 32 bits: no uint64 overflow
        c = [(p1 >> sh) ^ c[1] ^ np.uint64(k0), p1 & lo, (p0 >> sh) ^ c[3] ^ np.uint64(k1), p0 & lo]
        k0, k1 = (k0 + PHILOX_W[0]) & _U32, (k1 + PHILOX_W[1]) & _U32
    return tuple(x.astype(np.uint32) for x in c)


PHILOX_KAT = (  # (counter words, key words, output words): the Random123 known-answer tests
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((_U32,) * 4, (_U32,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
)


# ---- draws -------------------------------------------------------------------------------------
def draws(mq: int, k: int, s, seed: int = SEED, counter_base: int = COUNTER_BASE):
    """(pick, L) int64 of the samples with GLOBAL indices ``s`` (sample_offset already added): in
    128-sample block s // 128 the counter (64 (s // 128) + s % 64, counter_base) -- each a 64-bit
    number split into two words -- keyed by the seed serves sample s with words (x, y) in the first
    half of the block and (z, w) in the second; pick = (word * mq k) >> 32, L = word >> 16."""
    s = np.asarray(s, dtype=np.uint64)
    c = (s // np.uint64(128)) * np.uint64(64) + s % np.uint64(64)
    cb = int(counter_base) & (2 ** 64 - 1)
    r = philox4x32_10((c & np.uint64(_U32), c >> np.uint64(32), cb & _U32, cb >> 32),
                      (int(seed) & _U32, (int(seed) >> 32) & _U32))
    second = (s % np.uint64(128)) >= np.uint64(64)
    wp = np.where(second, r[2], r[0]).astype(np.uint64)
    wl = np.where(second, r[3], r[1]).astype(np.uint64)
    pick = (wp * np.uint64(mq * k)) >> np.uint64(32)
    return pick.astype(np.int64), (wl >> np.uint64(16)).astype(np.int64)


def sample_ids(n_new: int, sample_offset: int = 0, rows=None) -> np.ndarray:
    r = np.arange(n_new, dtype=np.int64) if rows is None else np.asarray(rows, dtype=np.int64)
    return r.astype(np.uint64) + np.uint64(sample_offset)


# ---- one-rounding interpolation ------------------------------------------------------------------
def fma32(L, d, a) -> np.ndarray:
    """float32(L / 65536 * d + a) with ONE rounding, for integer 0 <= L < 65536 and float32 d, a.

    The product L d 2^-16 (16 x 24 bits) is exact in fp64.  TwoSum gives the fp64 sum s and its exact
    error e.  Where e != 0 the exact sum lies strictly between s and its neighbour on e's side; of
    those two the one with an odd last bit is taken (round to odd), which keeps a 53-bit value whose
    rounding to 24 bits equals the rounding of the exact sum (53 >= 24 + 2)."""
    L = np.asarray(L, dtype=np.int64)
    d, a = np.asarray(d, dtype=np.float32), np.asarray(a, dtype=np.float32)
    p = L.astype(np.float64) * d.astype(np.float64) * 2.0 ** -16
    a64 = a.astype(np.float64)
    p, a64 = np.broadcast_arrays(p, a64)
    s = p + a64
    bb = s - p
    e = (p - (s - bb)) + (a64 - bb)
    bits = np.array(s, dtype=np.float64).view(np.uint64)
    fix = (e != 0.0) & ((bits & np.uint64(1)) == 0)
    away = (e > 0.0) == (s > 0.0)  # the exact sum is larger in magnitude than s
    bits = np.where(fix, np.where(away, bits + np.uint64(1), bits - np.uint64(1)), bits)
    return bits.view(np.float64).astype(np.float32)


# ---- parents, neighbours, affine ---------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _parent_master(m: int) -> np.ndarray:
    rng = np.random.default_rng(1000 + m)
    C = np.empty((m, NCOLS), dtype=np.float32)
    sign = lambda: np.where(rng.random(m) < 0.5, -1.0, 1.0)  # noqa: E731
    for j in range(NFEAT):
        kind = j % 6
        if kind == 0:
            C[:, j] = rng.normal(0.0, 1.0, m)
        elif kind == 1:
            C[:, j] = sign() * 10.0 ** rng.uniform(-3.0, 3.0, m)
        elif kind == 2:
            C[:, j] = rng.choice(np.array([0.7, -1.3], dtype=np.float32), m)
        elif kind == 3:
            C[:, j] = sign() * rng.choice(np.array([0.3, 5.5], dtype=np.float32), m)
        elif kind == 4:
            C[:, j] = sign() * rng.uniform(100.0, 200.0, m)
        else:
            C[:, j] = sign() * 2.0 ** rng.uniform(-14.0, -9.0, m)
    C[:, BIAS_COL] = 1.0
    C[:, LABEL_COL] = 3.0  # neither label used by the tests: the kernel must overwrite it
    C.setflags(write=False)
    return C


def parents(m: int) -> np.ndarray:
    """[m, 32] float32 parents.  Feature column j is of kind j % 6: 0 N(0, 1); 1 +-magnitudes spread
    log-uniformly over 1e-3 .. 1e3 (b - a rounds in fp32); 2 one of two values (about half of the pairs
    repeat their neighbour: d = 0); 3 +-0.3 or +-5.5 (pairs of exact negatives: the result crosses zero
    and is exactly zero at lambda = 1/2); 4 +-100 .. 200 (saturates e4m3 at scale 4 above 112); 5
    +-2^-14 .. 2^-9 (e4m3 subnormals and underflow at scale 4).  Column 30 is 1 and column 31 is 3."""
    return _parent_master(m)


def parents_bf16(m: int) -> np.ndarray:
    """uint16 bf16 bits of parents(m)."""
    return bf16_bits(parents(m))


def neighbours(mq: int, k: int, m: int) -> np.ndarray:
    """int32 [mq, k] neighbour rows drawn over ALL m parent rows (some below q_offset)."""
    return np.random.default_rng(17 * mq + k).integers(0, m, size=(mq, k)).astype(np.int32)


def affine() -> np.ndarray:
    """float64 [64]: the kernel reads the centre of column c at aff[c] and takes the reciprocal of
    aff[32 + c]; both non-dyadic.  Slots 30 / 31 hold values a kernel must never apply."""
    a = np.empty(64)
    c = np.arange(32)
    a[:32] = 0.1 * (c + 1) - 1.37
    a[32:] = 0.31 + 0.0713 * c
    a[30], a[31], a[62], a[63] = 5.0, -7.0, 3.0, 0.125
    return a


def affine_f32(aff: np.ndarray):
    """(sig [30], cc [30]) float32 as the kernels form them: float32(1.0 / aff[32 + c]) from an fp64
    division, float32(aff[c])."""
    aff = np.asarray(aff, dtype=np.float64)
    return (1.0 / aff[32:32 + NFEAT]).astype(np.float32), aff[:NFEAT].astype(np.float32)


def store(vals: np.ndarray, kind: str, fp8_scale: float = FP8_SCALE) -> np.ndarray:
    """float32 row values -> stored elements: float32 bits (uint32), bf16 bits (uint16) or e4m3 codes
    (uint8; features times fp8_scale in float32 first, columns 30 / 31 unscaled)."""
    vals = np.asarray(vals, dtype=np.float32)
    if kind == "f32":
        return vals.view(np.uint32)
    if kind == "bf16":
        return bf16_bits(vals)
    v = vals.copy()
    v[:, :NFEAT] = v[:, :NFEAT] * np.float32(fp8_scale)
    return fp8_encode(v)


def parents_oracle(C: np.ndarray, aff=None) -> np.ndarray:
    """smote_parents_kernel: bf16 bits of v * sig + cc (two float32 operations) on the feature columns,
    of v itself without aff and on columns 30 / 31."""
    v = np.array(C, dtype=np.float32)
    if aff is not None:
        sig, cc = affine_f32(aff)
        v[:, :NFEAT] = v[:, :NFEAT] * sig[None, :] + cc[None, :]
    return bf16_bits(v)


def parents_case(m: int) -> np.ndarray:
    """[m, 32] float32 input of the parents kernel: N(0, 1) with every third cell cycling through exact
    bf16 ties (odd and even kept bit, both signs, 2^-95 .. 2^97), +-0.0, +-1e30 and +-3e-30."""
    rng = np.random.default_rng(50 + m)
    C = rng.normal(0.0, 1.0, (m, NCOLS)).astype(np.float32)
    up = np.array([(ex << 7) | mant for ex in (0x20, 0x70, 0x7E, 0x7F, 0x80, 0x85, 0x8A, 0x96, 0xE0)
                   for mant in (0x00, 0x01, 0x02, 0x7E, 0x7F)], dtype=np.uint32)
    up = np.concatenate([up, up | np.uint32(0x8000)])
    ties = ((up << np.uint32(16)) | np.uint32(0x8000)).view(np.float32)
    edges = np.concatenate([ties, np.array([-0.0, 0.0, 1e30, -1e30, 3e-30, -3e-30], dtype=np.float32)])
    flat = C.reshape(-1)
    cells = np.arange(0, flat.shape[0], 3)
    flat[cells] = edges[(cells // 3 + 7 * m) % edges.shape[0]]
    return C


# ---- the row oracle ----------------------------------------------------------------------------
def generate_values(par, nbr, q_offset: int, s, label: float = 1.0, aff=None, seed: int = SEED,
                    counter_base: int = COUNTER_BASE) -> np.ndarray:
    """float32 [len(s), 32] rows of the samples with global indices ``s`` before the store, as the kernel
    forms them: row i = pick // k, neighbour j = nbr[i, pick % k], a = par[q_offset + i], b = par[j],
    d = fl32(b - a), o = fma32(L, d, a) on all 32 columns; with aff (fp32 parents only)
    o * sig + cc as two float32 operations on the features; then column 30 = 1, column 31 = label."""
    par = np.asarray(par, dtype=np.float32)
    nbr = np.asarray(nbr)
    mq, k = nbr.shape
    pick, L = draws(mq, k, s, seed, counter_base)
    i = pick // k
    j = nbr[i, pick % k].astype(np.int64)
    a, b = par[q_offset + i], par[j]
    o = fma32(L[:, None], b - a, a)
    if aff is not None:
        sig, cc = affine_f32(aff)
        o[:, :NFEAT] = o[:, :NFEAT] * sig[None, :] + cc[None, :]
    o[:, BIAS_COL] = np.float32(1.0)
    o[:, LABEL_COL] = np.float32(label)
    return o


def generate_oracle(par, nbr, q_offset, s, kind, label=1.0, aff=None, fp8_scale=FP8_SCALE, seed=SEED,
                    counter_base=COUNTER_BASE) -> np.ndarray:
    """The stored bits of generate_values (store())."""
    return store(generate_values(par, nbr, q_offset, s, label, aff, seed, counter_base), kind, fp8_scale)


def parent_values(m: int, ptype: str) -> np.ndarray:
    """The float32 values the kernel gathers: parents(m), or their bf16 rounding."""
    return parents(m) if ptype == "f32" else bf16_values(parents_bf16(m))


def two_rounding_values(par, nbr, q_offset: int, s, label: float = 1.0, seed: int = SEED,
                        counter_base: int = COUNTER_BASE) -> np.ndarray:
    """generate_values with the WRONG interpolation fl32(fl32(l d) + a) (a multiply, then an add): what a
    kernel without the fused multiply-add would produce.  Not an oracle: test_smote_oracle.py counts the
    stored elements on which it differs from generate_values, i.e. how many elements of a device test can
    tell the two apart."""
    par = np.asarray(par, dtype=np.float32)
    nbr = np.asarray(nbr)
    mq, k = nbr.shape
    pick, L = draws(mq, k, s, seed, counter_base)
    i = pick // k
    a, b = par[q_offset + i], par[nbr[i, pick % k].astype(np.int64)]
    o = ((L[:, None].astype(np.float32) / np.float32(65536.0)) * (b - a) + a).astype(np.float32)
    o[:, BIAS_COL] = np.float32(1.0)
    o[:, LABEL_COL] = np.float32(label)
    return o


def sweep_rows(n_new: int, first_sweep: int) -> np.ndarray:
    """Rows checked by the grid-stride test: every SWEEP_STRIDE-th row, and every row from SWEEP_TAIL
    rows before the end of the first sweep on."""
    lo = first_sweep - SWEEP_TAIL
    return np.concatenate([np.arange(0, lo, SWEEP_STRIDE), np.arange(lo, n_new)]).astype(np.int64)


# ---- the bucket sort ---------------------------------------------------------------------------
def bucket_fine_bits(R: int, n_new: int) -> int:
    """smote.hip smote_bucket_fine_bits: at most 16384 coarse bins, about 4096 samples per bin, at most
    2^7 picks per bin."""
    fb = 0
    while fb < 7 and ((R + (1 << fb) - 1) >> fb) > 16384:
        fb += 1
    while fb < 7 and float(n_new) * float(1 << (fb + 1)) / float(R) <= 4096.0:
        fb += 1
    return fb


def bucket_bins(R: int, n_new: int) -> int:
    fb = bucket_fine_bits(R, n_new)
    return (R + (1 << fb) - 1) >> fb


def bucket_blocks(n_new: int) -> int:
    npairs = ((n_new + 127) >> 7) << 6
    return max(1, (npairs + BUCKET_PAIRS - 1) // BUCKET_PAIRS)


@functools.lru_cache(maxsize=None)
def bucket_oracle(name: str):
    """(pick, L, cnt, sorted pick, sorted L) of a bucket case: the draws in sample order, the
    per-pick counts over all mq k picks and the (pick, L) pairs sorted by pick, then L."""
    mq, k, n_new, s_off = BUCKET_CASES[name]
    pick, L = draws(mq, k, sample_ids(n_new, s_off))
    cnt = np.bincount(pick, minlength=mq * k)
    order = np.lexsort((L, pick))
    out = (pick, L, cnt, pick[order], L[order])
    for a in out:
        a.setflags(write=False)
    return out


def bin_loads(name: str) -> np.ndarray:
    """Records per coarse bin (level 2 stages a bin in LDS iff its load is <= STAGE_RECS)."""
    mq, k, n_new, _ = BUCKET_CASES[name]
    fb = bucket_fine_bits(mq * k, n_new)
    return np.bincount(bucket_oracle(name)[0] >> fb, minlength=bucket_bins(mq * k, n_new))


def check_buckets(name: str, off, cnt, lam) -> None:
    """cnt == the bincount over ALL picks; the non-empty runs tile [0, n_new); sorted inside each run,
    the (pick, lambda) sequence equals the oracle's sorted pairs -- every sample, every pick."""
    mq, k, n_new, _ = BUCKET_CASES[name]
    _, _, ecnt, spick, sL = bucket_oracle(name)
    off, cnt = np.asarray(off, dtype=np.int64), np.asarray(cnt, dtype=np.int64)
    lam = np.asarray(lam).view(np.uint16).astype(np.int64)
    assert off.shape == cnt.shape == (mq * k,) and lam.shape == (n_new,)
    assert np.array_equal(cnt, ecnt), ("counts", np.flatnonzero(cnt != ecnt)[:10])
    live = np.flatnonzero(cnt)
    live = live[np.argsort(off[live], kind="stable")]
    ends = np.cumsum(cnt[live])
    assert np.array_equal(off[live], ends - cnt[live]) and ends[-1] == n_new, "the runs do not tile [0, n_new)"
    pos_pick = np.repeat(live, cnt[live])  # the pick owning each position of lam
    order = np.lexsort((lam, pos_pick))
    assert np.array_equal(pos_pick[order], spick)
    bad = np.flatnonzero(lam[order] != sL)
    assert bad.size == 0, ("lambdas", bad.size, spick[bad[:10]])
