// K4 logreg_fused_step: logistic-regression training on MI355X.
//
// Reference behaviour being replaced: sklearn LogisticRegression(C=1, l2, lbfgs, max_iter=1000)
// that produced models/logistic_model.joblib and the XGB fit loop of
// train_model.py:58-106.  Objective (sklearn/linear_model/_logistic.py:453-470):
//     obj(w) = (1/S) sum_i s_i * logloss_i + 1/(2 C S) * ||w_{0..d-1}||^2,  S = sum_i s_i,
// intercept (w[30], the constant-1 column) unpenalised.
//
// One streaming pass per iteration over the padded bf16 (or fp8) training rows (col 31 = label):
//   z = x.w -> p = sigmoid(z) -> r = s (p - y):   g += r x,  loss += s (softplus(z) - y z)
//   H += (sqrt(s p (1-p)) x)(sqrt(s p (1-p)) x)^T          (only for the Newton solver)
// The gradient/loss part runs on the VALU in fp32 (exact enough that the optimum is not biased by
// bf16 rounding of the update terms); the 32x32 Hessian is an MFMA GEMM over the row axis:
// each wave stages its 64 scaled rows (4 KiB) in a private LDS tile and reads them back with the
// gfx950 transpose read ds_read_b64_tr_b16, which delivers exactly the A (= S^T) and B (= S)
// fragments of v_mfma_f32_32x32x16_bf16 (cdna_hip_programming.md §3, T10) -- one register
// fragment serves both operands.  4 MFMAs per 64 rows keep the Hessian far under the HBM time.
//
// Per-block partials are reduced in a fixed order (fp64) by a second kernel, so a fit is bitwise
// reproducible run to run (no float atomics).  The Newton system (<= 32 unknowns) is solved on
// device by a one-block fp64 Cholesky with backtracking, so a whole fit is a sequence of launches
// with no host synchronisation (hipGraph-capturable); a device-side `done` flag turns the
// remaining iterations into no-ops once converged.  With data parallelism the reduced 1088-double
// vector is all-reduced over RCCL between the reduce and the update kernels (parallel/dp.py).
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <type_traits>

#include "common.h"
#include "launchers.h"

namespace fdx {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kPassBlocks = 1024;  // 4 per CU x 4 waves: 16 waves/CU of streaming loads

typedef short lds_s4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void unpack8(const uint4& v, float x[8]) {
  x[0] = bf16lo(v.x); x[1] = bf16hi(v.x); x[2] = bf16lo(v.y); x[3] = bf16hi(v.y);
  x[4] = bf16lo(v.z); x[5] = bf16hi(v.z); x[6] = bf16lo(v.w); x[7] = bf16hi(v.w);
}

// ---- virtual SMOTE rows (launchers.h SmoteView) -------------------------------------------------
// A SMOTE sample is x = a + lam (b - a) with a = parent row q_offset + pick / k, b = parent row
// nbr[pick] (bf16, the training rows' space) and lam on a 2^-16 grid, so z = w.x = za + lam (zb - za)
// and, summed over the samples of one pick,
//   gradient  sum r x       = (S_r - S_rl) a + S_rl b                 r = s (p - 1)
//   Hessian   sum d x x^T   = [a b] M [a b]^T,  M = sum d [(1-lam)^2, lam(1-lam); lam(1-lam), lam^2]
// with d = s p (1 - p).  M is PSD 2x2: M = L L^T gives two rank-1 terms u1 = l11 a + l21 b,
// u2 = l22 b that go through the same LDS tile + MFMA as stored rows.  A pass therefore streams
// the stored rows from HBM plus 2 bytes of lambda per sample (bucketed by pick once per fit,
// smote.hip smote_bucket_kernel) and reads each pick's two parent rows (L2-resident) once --
// instead of 64 B per stored SMOTE row plus their 512 MB write.  The synthetic rows enter at full
// fp32 precision (no bf16 rounding of the interpolant).  Per-sample terms are summed in fixed
// point (int64), so the bucket order the fill's atomics produce does not change a bit: fits stay
// bitwise reproducible.
constexpr float kSynQ = 4194304.0f;   // 2^22: r, r lam, d, d lam, d lam^2 (|v| <= s <= 32)
constexpr float kSynQL = 16384.0f;    // 2^14: per-sample loss (<= 80 s; what lies beyond: per pick)

template <int G>
__device__ __forceinline__ long long group_sum_i64(long long v) {
#pragma unroll
  for (int o = 1; o < G; o <<= 1) {
    const unsigned long long u = (unsigned long long)v;
    const unsigned lo = (unsigned)__shfl_xor((int)(u & 0xffffffffu), o, kWave);
    const unsigned hi = (unsigned)__shfl_xor((int)(u >> 32), o, kWave);
    v += (long long)(((unsigned long long)hi << 32) | lo);
  }
  return v;
}

// One pick's inputs (pick_terms' load stage): its lambda run (off, cnt), the first L lambdas of
// this lane, and this lane's columns of the two parent rows.  Nothing here depends on the weights,
// so the persistent SGD launch loads the next step's pick before the grid barrier (the two
// dependent round trips -- off / cnt / nbr, then lambdas / parents -- hide behind the barrier).
template <int LPR, int L>
struct PickIn {
  static_assert(L % 2 == 0, "lambdas are held in pairs");
  int o0 = 0, cnt = 0;
  uint4 ra[(32 / LPR) / 8], rb[(32 / LPR) / 8];
  uint32_t lv[L / 2];  // lambda u in bits [16 (u & 1), 16 (u & 1) + 16) of lv[u / 2]
  __device__ __forceinline__ uint32_t lam(int u) const { return (lv[u >> 1] >> (16 * (u & 1))) & 0xffffu; }
};

// lambdas u = 0 .. L-1 of this lane from j0 (j = j0 + u * LPR), packed in pairs
template <int LPR, int L>
__device__ __forceinline__ void load_lam_pairs(const SmoteView& sv, int o0, int cnt, int j0, uint32_t (&lv)[L / 2]) {
#pragma unroll
  for (int u = 0; u < L; u += 2) {
    const int j = j0 + u * LPR;
    const uint32_t lo = j < cnt ? sv.lam[o0 + j] : 0u;
    const uint32_t hi = j + LPR < cnt ? sv.lam[o0 + j + LPR] : 0u;
    lv[u >> 1] = lo | (hi << 16);
  }
}

template <int LPR, int L>
__device__ __forceinline__ void pick_load(const SmoteView& sv, int64_t p, int q, PickIn<LPR, L>& in) {
  constexpr int C = 32 / LPR;
  const bool ok = p >= 0;
  const int64_t pp = ok ? p : 0;
  const int64_t ra = sv.q_offset + pp / sv.k, rb = sv.nbr[pp];
  const uint4* Pb = reinterpret_cast<const uint4*>(sv.parents);
  in.o0 = ok ? sv.off[pp] : 0;
  in.cnt = ok ? sv.cnt[pp] : 0;
  // L lambdas per lane in flight: the lambda loads are issued before the parent rows arrive, so a
  // pick of <= LPR * L samples (the bench's ~117) costs one round trip for its lambdas, overlapped
  // with the parents' -- not one per 8 samples after them (the chain a wave's pick tile adds to a
  // latency-bound sub-sampled pass).
  load_lam_pairs<LPR, L>(sv, in.o0, in.cnt, q, in.lv);
#pragma unroll
  for (int h = 0; h < C / 8; ++h) {
    in.ra[h] = Pb[ra * 4 + (C / 8) * q + h];
    in.rb[h] = Pb[rb * 4 + (C / 8) * q + h];
  }
}

// One pick's terms for the LPR lanes that share it (lane q owns columns [C q, C q + C)), from its
// loaded inputs (pick_load; a pick of more than LPR * L samples loads the rest here, L at a time).
// wl: this lane's weights in the kernel's row units; xs: the unit scale of feature columns (fp8
// rows hold features * x_scale); an empty pick (p < 0 at load) still joins the shuffles.  The
// pick's gradient is added into gacc; xa / xb are the caller's scratch for the two parent rows and,
// for HESS, come back holding the two rank-1 Hessian rows u1 / u2 (in place: no extra registers
// live beside a mid-loop pick, which is what lets the fp8 pass run its picks mid-loop).  Per-sample
// terms are summed as integers (groups of 8 in int32, |term| < 2^30 / 8): the grouping -- and L --
// changes no bit.
template <int LPR, bool HESS, bool FISH, int L>
__device__ __forceinline__ void pick_compute(const SmoteView& sv, const PickIn<LPR, L>& in, int q, const float* wl,
                                             float xs, float sw1, float hrs, float* gacc, float* xa, float* xb,
                                             float& loss, float& wsum, float& dsum) {
  constexpr int C = 32 / LPR;
  constexpr int kLamGroup = 8;
  const int o0 = in.o0, cnt = in.cnt;
#pragma unroll
  for (int h = 0; h < C / 8; ++h) {
    unpack8(in.ra[h], xa + 8 * h);
    unpack8(in.rb[h], xb + 8 * h);
  }
  float za = 0.0f, zb = 0.0f;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const int col = C * q + c;
    const float cs = col == kLabelCol ? 0.0f : (col < kBiasCol ? xs : 1.0f);
    xa[c] *= cs;
    xb[c] *= cs;
    za = fmaf(wl[c], xa[c], za);
    zb = fmaf(wl[c], xb[c], zb);
  }
  za = group_sum<LPR>(za);
  zb = group_sum<LPR>(zb);
  const float dz = zb - za;
  long long sr = 0, srl = 0, sd = 0, sdl = 0, sdll = 0, sl = 0;
  uint32_t lv[L / 2];
#pragma unroll
  for (int u = 0; u < L / 2; ++u) lv[u] = in.lv[u];
  for (int j0 = q; j0 < cnt; j0 += LPR * L) {
    if (j0 != q) load_lam_pairs<LPR, L>(sv, o0, cnt, j0, lv);
#pragma unroll
    for (int g0 = 0; g0 < L; g0 += kLamGroup) {
      if (j0 + g0 * LPR >= cnt) break;
      int br = 0, brl = 0, bd = 0, bdl = 0, bdll = 0, bl = 0;
#pragma unroll
      for (int u = g0; u < g0 + kLamGroup; ++u) {
        if (j0 + u * LPR >= cnt) break;
        const float lam = (float)((lv[u >> 1] >> (16 * (u & 1))) & 0xffffu) * (1.0f / 65536.0f);
        const float z = fmaf(lam, dz, za);
        const float zc = fminf(fmaxf(z, -80.0f), 80.0f);
        const float eh = __expf(-0.5f * zc);
        const float e2 = eh * eh;  // exp(-z)
        const float pr = fast_rcp(1.0f + e2);
        const float r = -sw1 * pr * e2;  // s (p - 1) without the cancellation
        br += __float2int_rn(r * kSynQ);
        brl += __float2int_rn(r * lam * kSynQ);
        if constexpr (HESS || FISH) {
          const float d = sw1 * pr * pr * e2;  // s p (1 - p)
          bd += __float2int_rn(d * kSynQ);
          if constexpr (HESS) {
            bdl += __float2int_rn(d * lam * kSynQ);
            bdll += __float2int_rn(d * lam * lam * kSynQ);
          }
        }
        bl += __float2int_rn(sw1 * log1p_fast(e2) * kSynQL);  // s softplus(-z) = -s log p
      }
      sr += br; srl += brl; sl += bl;
      if constexpr (HESS || FISH) sd += bd;
      if constexpr (HESS) { sdl += bdl; sdll += bdll; }
    }
  }
  // The clamp above keeps every fixed-point term in range, but it also cuts a sample's loss at
  // 80 s, where a stored row's loss keeps growing as -z.  z is linear in lambda, so samples
  // below the clamp exist only when a parent's logit is (rare: a model wrong by 80 logits on a
  // minority row); then the missing s sum (-80 - z) = s (n (-80 - za) - dz sum lam) over those
  // samples.  The branch is uniform over the pick's LPR lanes (za, zb are group sums).  Their count
  // n and lambda sum are integers, summed over the lanes FIRST; the term is then rounded to fixed
  // point ONCE per pick and added in one lane -- a function of the pick's sample set only, whatever
  // order the bucket fill dealt the lambdas to the lanes in (one rounding of 0.5 / kSynQL per pick).
  if (fminf(za, zb) < -80.0f) {
    long long n_lo = 0, l_lo = 0;
    for (int j = q; j < cnt; j += LPR) {
      const uint32_t li = sv.lam[o0 + j];
      if (fmaf((float)li * (1.0f / 65536.0f), dz, za) < -80.0f) {
        n_lo += 1;
        l_lo += (long long)li;
      }
    }
    n_lo = group_sum_i64<LPR>(n_lo);
    l_lo = group_sum_i64<LPR>(l_lo);
    const double cut = (double)n_lo * (-80.0 - (double)za) - (double)dz * ((double)l_lo * (1.0 / 65536.0));
    if (q == 0) sl += (long long)__builtin_rint((double)sw1 * cut * (double)kSynQL);
  }
  sr = group_sum_i64<LPR>(sr);
  srl = group_sum_i64<LPR>(srl);
  sl = group_sum_i64<LPR>(sl);
  const double inv = 1.0 / (double)kSynQ;
  const float ca = (float)((double)(sr - srl) * inv), cb = (float)((double)srl * inv);
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const float gc = fmaf(ca, xa[c], cb * xb[c]);
    gacc[c] += gc;
  }
  if constexpr (HESS) {
    sd = group_sum_i64<LPR>(sd);
    sdl = group_sum_i64<LPR>(sdl);
    sdll = group_sum_i64<LPR>(sdll);
    const double m11 = (double)(sd - 2 * sdl + sdll) * inv, m21 = (double)(sdl - sdll) * inv;
    const double m22 = (double)sdll * inv;
    const double l11 = sqrt(fmax(m11, 0.0));
    const double l21 = l11 > 0.0 ? m21 / l11 : 0.0;
    const double l22 = sqrt(fmax(m22 - l21 * l21, 0.0));
    const float f11 = (float)(l11 * hrs), f21 = (float)(l21 * hrs), f22 = (float)(l22 * hrs);
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float a = xa[c], b = xb[c];
      xa[c] = fmaf(f11, a, f21 * b);  // u1
      xb[c] = f22 * b;                // u2
    }
  }
  loss = (float)((double)sl * (1.0 / (double)kSynQL));
  wsum = (float)cnt * sw1;
  if constexpr (FISH && !HESS) sd = group_sum_i64<LPR>(sd);
  dsum = (HESS || FISH) ? (float)((double)sd * inv) : 0.0f;
}

// Load + compute of one pick (kLamLoads: as many lambdas in flight as the caller's register budget
// allows; Hessian passes 8).
template <int LPR, bool HESS, bool FISH = false, int kLamLoads = 8>
__device__ __forceinline__ void pick_terms(const SmoteView& sv, int64_t p, int q, const float* wl, float xs,
                                           float sw1, float hrs, float* gacc, float* xa, float* xb, float& loss,
                                           float& wsum, float& dsum) {
  PickIn<LPR, kLamLoads> in;
  pick_load<LPR, kLamLoads>(sv, p, q, in);
  pick_compute<LPR, HESS, FISH, kLamLoads>(sv, in, q, wl, xs, sw1, hrs, gacc, xa, xb, loss, wsum, dsum);
}

// ---- fused SGD step (FUSE passes: one launch per SGD step) ------------------------------------
// Instead of writing [nblocks][36] float partials for a separate reduce + update launch, every block
// maps its sums to standardized space (the affine map of pivot-shifted rows), rounds them to 2^-20
// fixed point and adds them into 36 int64 device accumulators with agent-scope atomics -- integer
// addition is associative, so the totals are bitwise the same whatever the arrival order -- then
// takes a ticket; the block that draws the last ticket swaps the accumulators back to zero, turns
// them into the step's sums and applies the update (sgd_apply).  Producer and consumer touch the
// hand-off words with 8-byte agent atomics only (MI355X_MICROARCH.md: valid without fences).
// The accumulators are replicated kSgdReplicas times (block b adds into replica b mod R): 768
// blocks adding into ONE set of 36 words serialise at the memory-side atomic unit (a fused step
// measured 41 us against ~26 us for the pass alone, profiles/r4_f); R replicas cut the queue per
// word R-fold, and the last block folds the replicas in a fixed order.
constexpr int kSgdReplicas = 32;
constexpr int kSgdAccWords = kSgdReplicas * 36;
struct SgdFuse {
  unsigned long long* acc = nullptr;  // [kSgdReplicas][36] fixed-point sums (zero between steps)
  unsigned int* ticket = nullptr;     // arrivals (zero between steps)
  double* st = nullptr;               // solver state
  float* w32 = nullptr;               // the weights the next pass reads
  int* done = nullptr;
  const double* aff = nullptr;        // pivot-shifted rows: (c | 1/sigma)
  long long* sums = nullptr;          // non-null: the last block writes the folded [36] sums here
                                      // instead of applying the update (data parallel lean step)
  SgdArgs a;
};
constexpr double kFixScale = 1048576.0;  // 2^20
template <bool kWaveOnly = false>
__device__ void sgd_apply(const double* rd, double* __restrict__ st, float* __restrict__ w32, int* __restrict__ done,
                          const double* __restrict__ aff, const SgdArgs& a, int t, bool mapped);

// Slot t of NW waves' [36] sums: each wave's sum mapped to standardized space (pivot-shifted rows)
// and rounded to 2^-20 fixed point ON ITS OWN, then added as integers -- so the step's sums depend
// only on each wave's rows, not on how waves are grouped into blocks (the per-step launch and the
// persistent launch group them differently and get bitwise the same sums).
template <int NW>
__device__ __forceinline__ long long wave_sums_fixed(const float (*red)[36], const double* aff, int t) {
  long long q = 0;
#pragma unroll
  for (int w = 0; w < NW; ++w) {
    double v = (double)red[w][t];
    if (aff != nullptr && t < 32) v = aff[32 + t] * (v - aff[t] * (double)red[w][kBiasCol]);
    q += (long long)__builtin_rint(v * kFixScale);
  }
  return q;
}

// Called by every thread of the block after `red` (the 4 waves' [36] sums) is complete in LDS.
template <int NW>
__device__ __forceinline__ void sgd_fused_tail(const float (*red)[36], const SgdFuse& fz) {
  __shared__ int s_last;
  __shared__ double rd[36];
  const int t = threadIdx.x;
  if (t < 64) {  // wave 0: each wave's sums -> standardized space -> fixed point -> atomics
    if (t < 36) {
      const long long q = wave_sums_fixed<NW>(red, fz.aff, t);
      if (t != 34 && q != 0)
        __hip_atomic_fetch_add(fz.acc + (blockIdx.x % kSgdReplicas) * 36 + t, (unsigned long long)q, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (t == 0) {
      const unsigned k = __hip_atomic_fetch_add(fz.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      s_last = (k == gridDim.x - 1) ? 1 : 0;
    }
  }
  __syncthreads();
  if (!s_last) return;  // uniform per block
  __shared__ unsigned long long rep[kSgdAccWords];
  for (int e = t; e < kSgdAccWords; e += blockDim.x)  // every replica word: read and zero it
    rep[e] = __hip_atomic_exchange(fz.acc + e, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (t == 0) __hip_atomic_exchange(fz.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  if (t < 36) {  // fixed-order fold of the replicas (integer: exact in any order anyway)
    unsigned long long q = 0;
#pragma unroll 8
    for (int r = 0; r < kSgdReplicas; ++r) q += rep[r * 36 + t];
    if (fz.sums != nullptr) fz.sums[t] = (long long)q;
    rd[t] = (double)(long long)q * (1.0 / kFixScale);
  }
  if (fz.sums != nullptr) return;  // uniform: the ranks all-reduce the sums, then sgd_update_fixed
  __syncthreads();
  sgd_apply(rd, fz.st, fz.w32, fz.done, fz.aff, fz.a, t, true);
}

__device__ constexpr uint4 kNoTiles[4] = {};  // the `pre` argument of a pass that loads its own first tile

// Stored rows a pass walks (a CV fold's validation block [hole.at, hole.at + hole.len) excluded).
template <bool VIRT>
__device__ __forceinline__ int64_t pass_stored_rows(int64_t row_begin, int64_t row_end, const SmoteView& sv,
                                                    const RowHole& hole) {
  return (VIRT ? min(row_end, sv.n_real) : row_end) - row_begin - hole.len;
}

// One 64-row bf16 tile of a wave (4 lanes per row, 16 rows per load): logical row b + 16 u + rr.
__device__ __forceinline__ void bf16_load_tile(const void* __restrict__ Xv, int64_t row_begin, int64_t n,
                                               const RowHole& hole, int64_t b, uint4 (&v)[4]) {
  const int lane = lane_id();
  const int q = lane & 3, rr = lane >> 2;
  const uint4* X = reinterpret_cast<const uint4*>(Xv);
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int64_t row = b + 16 * u + rr;
    const int64_t ph = row + (row >= hole.at ? hole.len : 0);
    v[u] = row < n ? X[(row_begin + ph) * 4 + q] : make_uint4(0, 0, 0, 0);
  }
}

// The share of one pass that ONE wave owns, bf16 rows (4 lanes per row, 8 columns per lane),
// accumulated into this lane's sums.  `wave` / `Gw`: the wave's index in the pass grid and the
// grid's wave count -- the row-tile walk and the pick-tile walk depend on them only, so a
// persistent launch with another block shape walks exactly the rows of the per-pass launches.
// pre (nullable): the wave's first tile, already loaded (a persistent launch prefetches it across
// the grid barrier that precedes the pass).
// kDepth: stored tiles in flight (1: the next tile loads while this one computes; 2: the two next
// -- the persistent SGD launch runs 2 waves per SIMD, too few to cover HBM latency one tile ahead).
template <bool HESS, bool VIRT, bool FISH, int kPickLams = (HESS ? 8 : 32), int kPreLams = 32, int kDepth = 1>
__device__ __forceinline__ void bf16_wave_pass(
    const void* __restrict__ Xv, int64_t row_begin, int64_t row_end, const float (&wl)[8], float cw0, float cw1,
    int hess_stride, int row_sub, int row_phase, const SmoteView& sv, const RowHole& hole, int64_t wave,
    int64_t Gw, uint16_t* my_tile, float (&g)[8], float& lacc, float& wacc, float& whacc, float& dacc,
    f32x16_t& acc, const uint4 (&pre)[4], bool use_pre, const PickIn<4, kPreLams>& ppre, bool use_ppre) {
  wave = __builtin_amdgcn_readfirstlane((int)wave);  // wave-uniform: the tile walk lives in SGPRs
  const int lane = lane_id();
  const int q = lane & 3, rr = lane >> 2;
  // transpose-read lane geometry (constant per lane): 16-lane group grp reads 4 rows x 16 cols
  const int grp = lane >> 4, gi = lane & 15;
  const int tr_off = (8 * (grp >> 1) + (gi >> 2)) * kCols + 16 * (grp & 1) + 4 * (gi & 3);

  // stored rows (a CV fold's validation block [hole.at, hole.at + hole.len) is stepped over)
  const int64_t n = pass_stored_rows<VIRT>(row_begin, row_end, sv, hole);
  // row_sub > 1: only 64-row tiles t with (t mod G*row_sub) < G are visited (G = waves in the
  // grid): a uniform 1/row_sub subsample used by the early progressive-Newton iterations.
  const int64_t step = Gw * 64 * row_sub;
  const float scw0 = sqrtf(cw0), scw1 = sqrtf(cw1);
  // virtual SMOTE samples: tiles of 16 picks (row_sub: every row_sub-th tile).  A wave's pick
  // tile runs in the middle of its stored-row loop (at a wave-dependent iteration), so the
  // latency-bound pick work of some waves overlaps the streaming of the others instead of
  // forming a phase of its own at the end of the kernel (+33 us per full pass measured).
  const float hrs = rsqrtf((float)hess_stride);  // the final x hess_stride restores u u^T
  const int64_t npick = VIRT ? (int64_t)sv.mq * sv.k : 0;
  const int64_t ntile = (npick + 15) >> 4;
  // this wave's next pick tile (the low wave indices: in the per-pass grids they are the first
  // blocks dispatched; carrying the picks on the high ones -- the waves with one stored tile
  // fewer -- made the Newton step 1.094 -> 1.123 ms and the persistent SGD fit 585 -> 655 us, r5_v)
  int64_t ptile = wave * row_sub + row_phase;
  // pre: the tile's inputs are in ppre already (pick_load, issued before the grid barrier)
  auto pick_tile = [&](int64_t t, bool pre) __attribute__((always_inline)) {
    const int64_t p = t * 16 + rr;
    float u1[8], u2[8], ls, ws, ds;
    if (pre)
      pick_compute<4, HESS, FISH, kPreLams>(sv, ppre, q, wl, 1.0f, cw1, hrs, g, u1, u2, ls, ws, ds);
    else
      pick_terms<4, HESS, FISH, kPickLams>(sv, p < npick ? p : -1, q, wl, 1.0f, cw1, hrs, g, u1, u2, ls, ws, ds);
    if (q == 0) {
      lacc += ls;
      wacc += ws;
      if (HESS) whacc += ws / (float)hess_stride;
      if (FISH) dacc += ds;
    }
    if constexpr (HESS) {  // rows rr (u1) and 16 + rr (u2) of the wave's tile: 2 MFMAs
      uint4 a, b;
      a.x = pack_bf16x2(u1[0], u1[1]); a.y = pack_bf16x2(u1[2], u1[3]);
      a.z = pack_bf16x2(u1[4], u1[5]); a.w = pack_bf16x2(u1[6], u1[7]);
      b.x = pack_bf16x2(u2[0], u2[1]); b.y = pack_bf16x2(u2[2], u2[3]);
      b.z = pack_bf16x2(u2[4], u2[5]); b.w = pack_bf16x2(u2[6], u2[7]);
      *reinterpret_cast<uint4*>(my_tile + rr * kCols + 8 * q) = a;
      *reinterpret_cast<uint4*>(my_tile + (16 + rr) * kCols + 8 * q) = b;
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const lds_s4 a0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (__attribute__((address_space(3))) lds_s4*)(my_tile + s * 16 * kCols + tr_off));
        const lds_s4 a1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (__attribute__((address_space(3))) lds_s4*)(my_tile + s * 16 * kCols + tr_off + 4 * kCols));
        bf16x8_t f;
        f[0] = a0[0]; f[1] = a0[1]; f[2] = a0[2]; f[3] = a0[3];
        f[4] = a1[0]; f[5] = a1[1]; f[6] = a1[2]; f[7] = a1[3];
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f, f, acc, 0, 0, 0);
      }
      __builtin_amdgcn_wave_barrier();
    }
  };
  // tile-interleaved phases: wave w's i-th tile is (i Gw + w) row_sub + row_phase, so phase b of
  // row_sub is every row_sub-th 64-row tile of the shard (t mod row_sub == b) -- a minibatch samples
  // the whole shard at 64-row granularity whatever order the rows are stored in (the CV job's
  // fold-sorted table of time-sorted rows made group-strided minibatches differ in mean Time:
  // SGD stalled at an epoch gradient of 3.7e-3, profiles/r6_b)
  int64_t base = ((int64_t)wave * row_sub + row_phase) * 64;
  // Register double buffer: the next tile's 4 row loads are in flight while this tile computes
  // (kDepth 2: a third buffer, the tile after it too).
  uint4 cur[4], nx2[4];
  if (use_pre) {
#pragma unroll
    for (int u = 0; u < 4; ++u) cur[u] = pre[u];
  } else if (base < n) {
    bf16_load_tile(Xv, row_begin, n, hole, base, cur);
  }
  if constexpr (kDepth >= 2) {
    if (base + step < n) bf16_load_tile(Xv, row_begin, n, hole, base + step, nx2);
  }
  if constexpr (VIRT && FISH) {  // SGD passes: the wave's first pick tile ahead of its stored rows
    if (ptile < ntile) {
      pick_tile(ptile, use_ppre);
      ptile += Gw * row_sub;
    }
  }
  // Sub-sampled Hessian (hess_stride > 1): only every hess_stride-th tile of this wave feeds H
  // (scaled back at the end).  Gradient and loss always use every row, so the Newton fixed point
  // is unchanged; H only shapes the step (sub-sampled Newton).
  int hphase = (int)(wave % hess_stride);
  // pick tile after the ptrig-th stored tile of this wave (spread over the wave's iterations)
  const int64_t witers = n > base ? (n - base + step - 1) / step : 0;
  const int64_t ptrig = witers > 0 ? 1 + (wave % witers) : 0;
  int64_t pit = 0;
  for (; base < n; base += step) {
    uint4 nxt[4];
    if (base + kDepth * step < n) bf16_load_tile(Xv, row_begin, n, hole, base + kDepth * step, nxt);
    const bool do_h = HESS && hphase == 0;
    hphase = hphase + 1 == hess_stride ? 0 : hphase + 1;
    float xs[4][8];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      unpack8(cur[u], xs[u]);
    }
    float zq = 0.0f, yq = 0.0f, swq = 0.0f, dq = 0.0f;  // the row (u == q) this lane accounts for
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      float* x = xs[u];
      float y = (q == 3) ? x[7] : 0.0f;
      if (q == 3) x[7] = 0.0f;
      float zp = 0.0f;
#pragma unroll
      for (int j = 0; j < 8; ++j) zp = fmaf(wl[j], x[j], zp);
      zp = group_sum<4>(zp);
      y = group_sum<4>(y);
      const bool ok = base + 16 * u + rr < n;
      const bool pos = y > 0.5f;
      const float sw = ok ? (pos ? cw1 : cw0) : 0.0f;
      const float zc = fminf(fmaxf(zp, -80.0f), 80.0f);
      const float eh = __expf(-0.5f * zc);   // exp(-z/2)
      const float p = fast_rcp(fmaf(eh, eh, 1.0f));
      const float r = sw * (p - y);
#pragma unroll
      for (int j = 0; j < 8; ++j) g[j] = fmaf(r, x[j], g[j]);
      if (q == u) { zq = zp; yq = y; swq = sw; if (FISH) dq = sw * p * p * (eh * eh); }
      if (do_h) {
        // sqrt(s p (1-p)) = sqrt(s) * p * exp(-z/2)   (1-p = p e^{-z}): no sqrt, no cancellation
        const float dd = ok ? (pos ? scw1 : scw0) * p * eh : 0.0f;
        uint4 pk;
        pk.x = pack_bf16x2(x[0] * dd, x[1] * dd);
        pk.y = pack_bf16x2(x[2] * dd, x[3] * dd);
        pk.z = pack_bf16x2(x[4] * dd, x[5] * dd);
        pk.w = pack_bf16x2(x[6] * dd, x[7] * dd);
        *reinterpret_cast<uint4*>(my_tile + (16 * u + rr) * kCols + 8 * q) = pk;
      }
    }
    if (do_h) {
      // Wave-private tile: LDS instructions of one wave execute in order, so the transpose
      // reads below observe this wave's writes; the wave_barrier only pins compiler order.
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const lds_s4 a0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (__attribute__((address_space(3))) lds_s4*)(my_tile + s * 16 * kCols + tr_off));
        const lds_s4 a1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (__attribute__((address_space(3))) lds_s4*)(my_tile + s * 16 * kCols + tr_off +
                                                        4 * kCols));
        bf16x8_t f;
        f[0] = a0[0]; f[1] = a0[1]; f[2] = a0[2]; f[3] = a0[3];
        f[4] = a1[0]; f[5] = a1[1]; f[6] = a1[2]; f[7] = a1[3];
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f, f, acc, 0, 0, 0);
      }
      __builtin_amdgcn_wave_barrier();
    }
    // weighted log-loss of this lane's row: max(z,0) - y z + log1p(exp(-|z|))
    lacc = fmaf(swq, fmaxf(zq, 0.0f) - yq * zq + log1p_fast(__expf(-fabsf(zq))), lacc);
    wacc += swq;
    if (do_h) whacc += swq;
    if (FISH) dacc += dq;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if constexpr (kDepth >= 2) {
        cur[u] = nx2[u];
        nx2[u] = nxt[u];
      } else {
        cur[u] = nxt[u];
      }
    }
    if constexpr (VIRT && !FISH) {
      if (ptile < ntile && ++pit == ptrig) {
        pick_tile(ptile, false);
        ptile += Gw * row_sub;
      }
    }
  }

  if constexpr (VIRT) {  // the wave's remaining pick tiles
    for (; ptile < ntile; ptile += Gw * row_sub) pick_tile(ptile, false);
  }
}

// Agent-scope relaxed loads/stores: coherent across the XCDs' L2s within one launch.
template <typename T>
__device__ __forceinline__ T ld_agent(const T* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <typename T>
__device__ __forceinline__ void st_agent(T* p, T v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The Newton update's LDS (one wave).  Lc, the Cholesky factor's columns ([column][row], rows
// padded to 33), reuses sr's Hessian words [64, 64 + 32*33): H is in registers by then.  Fits in
// the pass kernels' 16 KiB row tile, so a pass that runs the update in its last block
// (newton_fused_tail) needs no extra LDS.
struct NewtonLds {
  double sr[64 + 32 * 33];  // >= kLRPartStride
  double cA[32], iA[32], h30[32];
  double ss[256];  // kStateSize
  double grad[32];
  double dv[32];
  int idx[32];
};
static_assert(64 + 32 * 33 >= kLRPartStride, "NewtonLds::sr holds the reduced vector");

// One-wave LDS ordering: LDS ops of one wave retire in order; this keeps the compiler from moving
// them across (the update runs on one wave, alone or as the last wave standing in a pass block).
__device__ __forceinline__ void nsync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// A Newton iteration's fused tail (launchers.h NewtonFuse), behind the partials of a pass block;
// defined with the update (newton_update_body).  lds: the block's row tile, free by then.
template <bool HESS>
__device__ __forceinline__ void newton_fused_tail(const float* __restrict__ partial, const NewtonFuse nf, void* lds);

// VIRT: the rows past the stored ones are virtual SMOTE samples (pick_terms above); the stored
// rows stream as usual, then the grid walks tiles of 16 picks (4 lanes per pick, 8 columns each).
// row_sub / row_phase: the pass visits the row tiles t with t mod row_sub == row_phase and the pick
// tiles with t mod row_sub == row_phase -- phase 0 of a
// 1/row_sub sub-sample is the progressive-Newton warm-up, phases 0..row_sub-1 are the disjoint
// minibatches of one SGD epoch (every stored row and every SMOTE sample in exactly one of them).
// FISH (gradient-only SGD passes): slot 35 also receives sum s p (1 - p), the minibatch's
// Gauss-Newton curvature scalar that sets the SGD step size (sgd_step_kernel).
template <bool HESS, bool VIRT = false, bool FISH = false, bool FUSE = false>  // bf16 rows; fp8: logreg_pass_fp8w_kernel
__global__ __launch_bounds__(kThreads, 3) void logreg_pass_kernel(
    const void* __restrict__ Xv, int64_t row_begin, int64_t row_end, const float* w,
    const float* __restrict__ class_w, const int* __restrict__ done, int hess_stride, int row_sub,
    int row_phase, float* __restrict__ partial, SmoteView sv, RowHole hole, SgdFuse fz, NewtonFuse nf) {
  if (done != nullptr && *done) {  // converged: uniform early exit for the whole grid
    if (nf.done_host != nullptr && blockIdx.x == 0 && threadIdx.x == 0)  // the update's flag word
      __hip_atomic_store(nf.done_host, (nf.seq << 1) | 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    return;
  }
  __shared__ __attribute__((aligned(16))) uint16_t tile[kWaves][64 * kCols];  // 16 KiB
  static_assert(sizeof(NewtonLds) <= sizeof(tile), "the fused Newton update reuses the row tile");
  __shared__ float red[kWaves][36];
  const int lane = lane_id(), wv = wave_id();
  const int q = lane & 3;
  float wl[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) wl[j] = (q * 8 + j == kLabelCol) ? 0.0f : w[q * 8 + j];
  const float cw0 = class_w[0], cw1 = class_w[1];
  float g[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) g[j] = 0.0f;
  float lacc = 0.0f, wacc = 0.0f, whacc = 0.0f;  // whacc: weight of the rows feeding H
  float dacc = 0.0f;                              // FISH: sum s p (1 - p)
  f32x16_t acc = {};
  PickIn<4, 32> nopick;
  bf16_wave_pass<HESS, VIRT, FISH>(Xv, row_begin, row_end, wl, cw0, cw1, hess_stride, row_sub, row_phase, sv, hole,
                                   (int64_t)blockIdx.x * kWaves + wv, (int64_t)gridDim.x * kWaves, tile[wv], g, lacc,
                                   wacc, whacc, dacc, acc, kNoTiles, false, nopick, false);

  // ---- block reduction (fixed order) ----
#pragma unroll
  for (int j = 0; j < 8; ++j) g[j] = strided_sum<4>(g[j]);
  lacc = wave_sum(lacc);
  wacc = wave_sum(wacc);
  whacc = wave_sum(whacc);
  if (FISH) dacc = wave_sum(dacc);
  if (lane < 4) {
#pragma unroll
    for (int j = 0; j < 8; ++j) red[wv][8 * lane + j] = g[j];
  }
  if (lane == 0) {
    red[wv][32] = lacc;
    red[wv][33] = wacc;
    red[wv][34] = HESS ? whacc * (float)hess_stride : 0.0f;
    red[wv][35] = dacc;
  }
  float* hb = reinterpret_cast<float*>(&tile[0][0]);  // 4 x 1024 floats = the 16 KiB tile
  if constexpr (HESS) {
    // each wave overwrites only its own tile region (same bytes it read from)
    const float hscale = (float)hess_stride;
    const int hcol = lane & 31;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int row = (k & 3) + 8 * (k >> 2) + 4 * (lane >> 5);
      hb[wv * 1024 + row * kCols + hcol] = acc[k] * hscale;
    }
  }
  __syncthreads();
  if constexpr (FUSE) {  // one launch per SGD step: fixed-point atomics + last-block update
    sgd_fused_tail<kWaves>(red, fz);
    return;
  }
  float* out = partial + (int64_t)blockIdx.x * kLRPartStride;
  const bool coherent = !FISH && nf.red != nullptr;  // a fused Newton tail reads them in this launch
  // slot 34 (Hessian weight) only from Hessian passes, slot 35 (curvature sum) from FISH passes
  if (threadIdx.x < (HESS ? 35 : 34) || (FISH && threadIdx.x == 35)) {
    const int t = threadIdx.x;
    const float v = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
    if (coherent) st_agent(out + t, v);
    else out[t] = v;
  }
  if constexpr (HESS) {
    for (int e = threadIdx.x; e < 1024; e += kThreads) {
      const float v = ((hb[e] + hb[1024 + e]) + hb[2048 + e]) + hb[3072 + e];
      if (coherent) st_agent(out + 64 + e, v);
      else out[64 + e] = v;
    }
  }
  if constexpr (!FISH) {
    if (nf.red != nullptr) {  // uniform: this launch also reduces and applies the Newton update
      __syncthreads();        // hb (the row tile) read out before the tail reuses it
      newton_fused_tail<HESS>(partial, nf, &tile[0][0]);
    }
  }
}

// fp8 rows, TWO lanes per row: each lane loads 16 columns (one 16 B load), 32 rows per wave
// load instruction, and the per-row work that every lane of a row repeats (the dot-product
// butterfly, sigmoid, loss bookkeeping) is shared by 2 lanes instead of 4.  The dot product and
// the gradient run on packed fp32 (v_pk_fma_f32, 2 columns per instruction).  The Hessian tile
// and its MFMA are those of the bf16 kernel.  Measured against the previous 4-lane fp8 kernel
// (profiles/r3_s): gradient pass 125 -> 99 us, sub-sampled Hessian pass 137 -> 112 us over
// 16M rows (5.2 TB/s), fp8 bench step 1.164 -> 1.099 ms.
// VIRT: virtual SMOTE samples as in the bf16 kernel: tiles of 16 picks in its 4-lane layout, mid-loop.
typedef float f32x2_t __attribute__((ext_vector_type(2)));
// One wave's two 32-row fp8 tiles (2 lanes per row, 16 columns per lane): rows b + 32 u + rr.
__device__ __forceinline__ void fp8_load_tile(const uint8_t* __restrict__ X8, int64_t row_begin, int64_t n,
                                              const RowHole& hole, int64_t b, uint4 (&v)[2]) {
  const int lane = lane_id();
  const int q = lane & 1, rr = lane >> 1;
  const uint4* X = reinterpret_cast<const uint4*>(X8);
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int64_t row = b + 32 * u + rr;
    const int64_t ph = row + (row >= hole.at ? hole.len : 0);
    v[u] = row < n ? X[(row_begin + ph) * 2 + q] : make_uint4(0, 0, 0, 0);
  }
}

// The share of one fp8 pass that ONE wave owns (bf16_wave_pass's contract).  wl: this lane's
// weights in fp8 row units (registers; read when !VIRT); wsh: the same 32 weights in LDS (VIRT
// reads them where used, see below).  pre (nullable): the wave's first two tiles, loaded already.
template <bool HESS, bool VIRT, bool FISH, int kPickLams = (HESS ? 8 : 24), int kPreLams = 32>
__device__ __forceinline__ void fp8_wave_pass(
    const uint8_t* __restrict__ X8, int64_t row_begin, int64_t row_end, const f32x2_t (&wl)[8], const float* wsh,
    float x_scale, float cw0, float cw1, int hess_stride, int row_sub, int row_phase, const SmoteView& sv,
    const RowHole& hole, int64_t wave, int64_t Gw, uint16_t* my_tile, f32x2_t (&g)[8], float& lacc, float& wacc,
    float& whacc, float& dacc, f32x16_t& acc, const uint4 (&pre)[4], bool use_pre, const PickIn<4, kPreLams>& ppre,
    bool use_ppre) {
  wave = __builtin_amdgcn_readfirstlane((int)wave);  // wave-uniform: the tile walk lives in SGPRs
  const int lane = lane_id();
  const int q = lane & 1, rr = lane >> 1;
  const int grp = lane >> 4, gi = lane & 15;
  const int tr_off = (8 * (grp >> 1) + (gi >> 2)) * kCols + 16 * (grp & 1) + 4 * (gi & 3);
  const int64_t n = pass_stored_rows<VIRT>(row_begin, row_end, sv, hole);  // stored rows
  const int64_t step = Gw * 64 * row_sub;
  const float scw0 = sqrtf(cw0), scw1 = sqrtf(cw1);
  // virtual SMOTE samples: tiles of 16 picks in the bf16 pass's 4-lane layout (lane q4 owns columns
  // [8 q4, 8 q4 + 8)), run in the middle of the stored-row loop as in the bf16 pass.  The 2-lane
  // layout of the stored rows would give a pick 16 columns per lane -- with the two prefetched fp8
  // tiles live that spilled 92 B/lane, which is why picks used to run after the loop (+ ~30 us
  // of pick latency per pass).  A pick's gradient is moved into the 2-lane
  // accumulator with one lane swap.
  const float hrs = rsqrtf((float)hess_stride);
  const int64_t npick = VIRT ? (int64_t)sv.mq * sv.k : 0;
  const int64_t ntile = (npick + 15) >> 4;
  int64_t ptile = wave * row_sub + row_phase;
  const int q4 = lane & 3, r4 = lane >> 2;
  auto pick_tile = [&](int64_t t, bool pre) __attribute__((always_inline)) {
    float wf[8];  // this lane's 4-lane-layout weights in fp8 row units, from LDS (not held in VGPRs
    asm volatile("" ::: "memory");  // across the stored loop: keeps the loads here)
#pragma unroll
    for (int j = 0; j < 8; ++j) wf[j] = wsh[8 * q4 + j];
    const int64_t p = t * 16 + r4;
    float gc[8], u1[8], u2[8], ls, ws, ds;
#pragma unroll
    for (int j = 0; j < 8; ++j) gc[j] = 0.0f;
    if (pre)
      pick_compute<4, HESS, FISH, kPreLams>(sv, ppre, q4, wf, x_scale, cw1, hrs, gc, u1, u2, ls, ws, ds);
    else
      pick_terms<4, HESS, FISH, kPickLams>(sv, p < npick ? p : -1, q4, wf, x_scale, cw1, hrs, gc, u1, u2, ls, ws,
                                           ds);
    {  // 4-lane columns [8 q4, 8 q4 + 8) -> the 2-lane accumulator g (lane parity h: columns
       // [16 h, 16 h + 16)): lanes q4 = 1, 2 swap, then each adds at offset 8 (q4 >> 1)
      const int src = (q4 == 1 || q4 == 2) ? (lane ^ 3) : lane;
      const bool hi = q4 >= 2;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float a = __shfl(gc[2 * k], src, kWave), b = __shfl(gc[2 * k + 1], src, kWave);
        g[k] += hi ? f32x2_t{0.0f, 0.0f} : f32x2_t{a, b};
        g[4 + k] += hi ? f32x2_t{a, b} : f32x2_t{0.0f, 0.0f};
      }
    }
    if (q4 == 0) {
      lacc += ls;
      wacc += ws;
      if (HESS) whacc += ws / (float)hess_stride;
      if (FISH) dacc += ds;
    }
    if constexpr (HESS) {  // rows r4 (u1) and 16 + r4 (u2) of the wave's tile: 2 MFMAs
      uint4 a, b;
      a.x = pack_bf16x2(u1[0], u1[1]); a.y = pack_bf16x2(u1[2], u1[3]);
      a.z = pack_bf16x2(u1[4], u1[5]); a.w = pack_bf16x2(u1[6], u1[7]);
      b.x = pack_bf16x2(u2[0], u2[1]); b.y = pack_bf16x2(u2[2], u2[3]);
      b.z = pack_bf16x2(u2[4], u2[5]); b.w = pack_bf16x2(u2[6], u2[7]);
      *reinterpret_cast<uint4*>(my_tile + r4 * kCols + 8 * q4) = a;
      *reinterpret_cast<uint4*>(my_tile + (16 + r4) * kCols + 8 * q4) = b;
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const lds_s4 a0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (__attribute__((address_space(3))) lds_s4*)(my_tile + s * 16 * kCols + tr_off));
        const lds_s4 a1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (__attribute__((address_space(3))) lds_s4*)(my_tile + s * 16 * kCols + tr_off + 4 * kCols));
        bf16x8_t f;
        f[0] = a0[0]; f[1] = a0[1]; f[2] = a0[2]; f[3] = a0[3];
        f[4] = a1[0]; f[5] = a1[1]; f[6] = a1[2]; f[7] = a1[3];
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f, f, acc, 0, 0, 0);
      }
      __builtin_amdgcn_wave_barrier();
    }
  };
  // tile-interleaved phases: wave w's i-th tile is (i Gw + w) row_sub + row_phase, so phase b of
  // row_sub is every row_sub-th 64-row tile of the shard (t mod row_sub == b) -- a minibatch samples
  // the whole shard at 64-row granularity whatever order the rows are stored in (the CV job's
  // fold-sorted table of time-sorted rows made group-strided minibatches differ in mean Time:
  // SGD stalled at an epoch gradient of 3.7e-3, profiles/r6_b)
  int64_t base = ((int64_t)wave * row_sub + row_phase) * 64;
  // two tiles in flight ahead of the one being computed (4 KiB per wave, as the bf16 stream)
  uint4 cur[2], nx1[2];
  if (use_pre) {
    cur[0] = pre[0]; cur[1] = pre[1]; nx1[0] = pre[2]; nx1[1] = pre[3];
  } else {
    if (base < n) fp8_load_tile(X8, row_begin, n, hole, base, cur);
    if (base + step < n) fp8_load_tile(X8, row_begin, n, hole, base + step, nx1);
  }
  if constexpr (VIRT && FISH) {  // SGD passes: the wave's first pick tile ahead of its stored rows
    if (ptile < ntile) {
      pick_tile(ptile, use_ppre);
      ptile += Gw * row_sub;
    }
  }
  int hphase = (int)(wave % hess_stride);
  const int64_t witers = n > base ? (n - base + step - 1) / step : 0;
  const int64_t ptrig = witers > 0 ? 1 + (wave % witers) : 0;
  int64_t pit = 0;
  for (; base < n; base += step) {
    if constexpr (VIRT) asm volatile("" ::: "memory");  // the LDS weight reads stay in the loop
    uint4 nxt[2];
    if (base + 2 * step < n) fp8_load_tile(X8, row_begin, n, hole, base + 2 * step, nxt);
    const bool do_h = HESS && hphase == 0;
    hphase = hphase + 1 == hess_stride ? 0 : hphase + 1;
    float zq = 0.0f, yq = 0.0f, swq = 0.0f, dq = 0.0f;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      float x[16];
      fp8x4_to_f32(cur[u].x, x);
      fp8x4_to_f32(cur[u].y, x + 4);
      fp8x4_to_f32(cur[u].z, x + 8);
      fp8x4_to_f32(cur[u].w, x + 12);
      float y = (q == 1) ? x[15] : 0.0f;
      if (q == 1) x[15] = 0.0f;
      f32x2_t zz = f32x2_t{0.0f, 0.0f};
#pragma unroll
      for (int p = 0; p < 8; ++p) {
        const f32x2_t wp = VIRT ? *reinterpret_cast<const f32x2_t*>(wsh + 16 * q + 2 * p) : wl[p];
        zz = __builtin_elementwise_fma(wp, f32x2_t{x[2 * p], x[2 * p + 1]}, zz);
      }
      float zp = group_sum<2>(zz[0] + zz[1]);
      y = group_sum<2>(y);
      const bool ok = base + 32 * u + rr < n;
      const bool pos = y > 0.5f;
      const float sw = ok ? (pos ? cw1 : cw0) : 0.0f;
      const float zc = fminf(fmaxf(zp, -80.0f), 80.0f);
      const float eh = __expf(-0.5f * zc);
      const float pr = fast_rcp(fmaf(eh, eh, 1.0f));
      const float r = sw * (pr - y);
      const f32x2_t r2 = f32x2_t{r, r};
#pragma unroll
      for (int p = 0; p < 8; ++p) g[p] = __builtin_elementwise_fma(r2, f32x2_t{x[2 * p], x[2 * p + 1]}, g[p]);
      if (q == u) { zq = zp; yq = y; swq = sw; if (FISH) dq = sw * pr * pr * (eh * eh); }
      if (do_h) {
        const float dd = ok ? (pos ? scw1 : scw0) * pr * eh : 0.0f;
        uint4 p0, p1;
        p0.x = pack_bf16x2(x[0] * dd, x[1] * dd);
        p0.y = pack_bf16x2(x[2] * dd, x[3] * dd);
        p0.z = pack_bf16x2(x[4] * dd, x[5] * dd);
        p0.w = pack_bf16x2(x[6] * dd, x[7] * dd);
        p1.x = pack_bf16x2(x[8] * dd, x[9] * dd);
        p1.y = pack_bf16x2(x[10] * dd, x[11] * dd);
        p1.z = pack_bf16x2(x[12] * dd, x[13] * dd);
        p1.w = pack_bf16x2(x[14] * dd, x[15] * dd);
        uint4* dst = reinterpret_cast<uint4*>(my_tile + (32 * u + rr) * kCols + 16 * q);
        dst[0] = p0;
        dst[1] = p1;
      }
    }
    if (do_h) {
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const lds_s4 a0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (__attribute__((address_space(3))) lds_s4*)(my_tile + s * 16 * kCols + tr_off));
        const lds_s4 a1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (__attribute__((address_space(3))) lds_s4*)(my_tile + s * 16 * kCols + tr_off + 4 * kCols));
        bf16x8_t f;
        f[0] = a0[0]; f[1] = a0[1]; f[2] = a0[2]; f[3] = a0[3];
        f[4] = a1[0]; f[5] = a1[1]; f[6] = a1[2]; f[7] = a1[3];
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f, f, acc, 0, 0, 0);
      }
      __builtin_amdgcn_wave_barrier();
    }
    lacc = fmaf(swq, fmaxf(zq, 0.0f) - yq * zq + log1p_fast(__expf(-fabsf(zq))), lacc);
    wacc += swq;
    if (do_h) whacc += swq;
    if (FISH) dacc += dq;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      cur[u] = nx1[u];
      nx1[u] = nxt[u];
    }
    if constexpr (VIRT && !FISH) {
      if (ptile < ntile && ++pit == ptrig) {
        pick_tile(ptile, false);
        ptile += Gw * row_sub;
      }
    }
  }

  if constexpr (VIRT) {  // the wave's remaining pick tiles
    for (; ptile < ntile; ptile += Gw * row_sub) pick_tile(ptile, false);
  }

}

template <bool HESS, bool VIRT = false, bool FISH = false, bool FUSE = false>
__global__ __launch_bounds__(kThreads, 3) void logreg_pass_fp8w_kernel(
    const uint8_t* __restrict__ X8, int64_t row_begin, int64_t row_end, const float* w,
    const float* __restrict__ class_w, const int* __restrict__ done, float x_scale, int d_feat,
    int hess_stride, int row_sub, int row_phase, float* __restrict__ partial, SmoteView sv, RowHole hole,
    SgdFuse fz, NewtonFuse nf) {
  if (done != nullptr && *done) {
    if (nf.done_host != nullptr && blockIdx.x == 0 && threadIdx.x == 0)
      __hip_atomic_store(nf.done_host, (nf.seq << 1) | 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    return;
  }
  __shared__ __attribute__((aligned(16))) uint16_t tile[kWaves][64 * kCols];  // 16 KiB
  __shared__ float red[kWaves][36];
  const int lane = lane_id(), wv = wave_id();
  const int q = lane & 1;
  const float inv_s = 1.0f / x_scale;
  // VIRT: the weights are read from LDS where used (wsh) instead of living in 16 VGPRs across
  // the loop -- the room a mid-loop pick tile needs to run without spilling
  __shared__ __attribute__((aligned(16))) float wsh[32];
  if (VIRT && threadIdx.x < 32) {
    const int col = threadIdx.x;
    wsh[col] = col == kLabelCol ? 0.0f : w[col] * (col < d_feat ? inv_s : 1.0f);
  }
  if (VIRT) __syncthreads();
  f32x2_t wl[8];
#pragma unroll
  for (int p = 0; p < 8; ++p) {
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int col = 16 * q + 2 * p + e;
      const float cs = col < d_feat ? inv_s : 1.0f;
      wl[p][e] = (col == kLabelCol) ? 0.0f : w[col] * cs;
    }
  }
  const float cw0 = class_w[0], cw1 = class_w[1];
  f32x2_t g[8];
#pragma unroll
  for (int p = 0; p < 8; ++p) g[p] = f32x2_t{0.0f, 0.0f};
  float lacc = 0.0f, wacc = 0.0f, whacc = 0.0f, dacc = 0.0f;
  f32x16_t acc = {};
  PickIn<4, 32> nopick;
  fp8_wave_pass<HESS, VIRT, FISH>(X8, row_begin, row_end, wl, wsh, x_scale, cw0, cw1, hess_stride, row_sub, row_phase,
                                  sv, hole, (int64_t)blockIdx.x * kWaves + wv, (int64_t)gridDim.x * kWaves, tile[wv],
                                  g, lacc, wacc, whacc, dacc, acc, kNoTiles, false, nopick, false);

  // ---- block reduction (fixed order) ----
  float gs[16];
#pragma unroll
  for (int p = 0; p < 8; ++p) {
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int col = 16 * q + 2 * p + e;
      gs[2 * p + e] = strided_sum<2>(g[p][e]) * (col < d_feat ? inv_s : 1.0f);
    }
  }
  lacc = wave_sum(lacc);
  wacc = wave_sum(wacc);
  whacc = wave_sum(whacc);
  if (FISH) dacc = wave_sum(dacc);
  if (lane < 2) {
#pragma unroll
    for (int j = 0; j < 16; ++j) red[wv][16 * lane + j] = gs[j];
  }

  if (lane == 0) {
    red[wv][32] = lacc;
    red[wv][33] = wacc;
    red[wv][34] = HESS ? whacc * (float)hess_stride : 0.0f;
    red[wv][35] = dacc;
  }
  float* hb = reinterpret_cast<float*>(&tile[0][0]);
  if constexpr (HESS) {
    const float hscale = (float)hess_stride;
    const int hcol = lane & 31;
    const float ccol = hcol < d_feat ? hscale * inv_s : hscale;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int row = (k & 3) + 8 * (k >> 2) + 4 * (lane >> 5);
      const float crow = row < d_feat ? inv_s : 1.0f;
      hb[wv * 1024 + row * kCols + hcol] = acc[k] * (ccol * crow);
    }
  }
  __syncthreads();
  if constexpr (FUSE) {
    sgd_fused_tail<kWaves>(red, fz);
    return;
  }
  float* out = partial + (int64_t)blockIdx.x * kLRPartStride;
  const bool coherent = !FISH && nf.red != nullptr;
  if (threadIdx.x < (HESS ? 35 : 34) || (FISH && threadIdx.x == 35)) {
    const int t = threadIdx.x;
    const float v = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
    if (coherent) st_agent(out + t, v);
    else out[t] = v;
  }
  if constexpr (HESS) {
    for (int e = threadIdx.x; e < 1024; e += kThreads) {
      const float v = ((hb[e] + hb[1024 + e]) + hb[2048 + e]) + hb[3072 + e];
      if (coherent) st_agent(out + 64 + e, v);
      else out[64 + e] = v;
    }
  }
  if constexpr (!FISH) {
    if (nf.red != nullptr) {  // uniform: this launch also reduces and applies the Newton update
      __syncthreads();        // hb (the row tile) read out before the tail reuses it
      newton_fused_tail<HESS>(partial, nf, &tile[0][0]);
    }
  }
}

// Stage 2: fixed-order fp64 reduction of [nblocks][1088] partials.  Block = 16 columns x 64
// row-groups (1024 threads), 68 blocks for the full 1088-wide vector: the partials were just
// written by the pass and sit in L2/MALL, so the kernel is load-LATENCY bound -- each thread's
// <= 12 loads are all in flight at once (one round trip, not six as with 16 row-groups), and the
// 64 row-group sums are combined in a fixed tree order (bitwise reproducible run to run).
constexpr int kRedCols = 16, kRedGroups = 64, kRedLoads = 12;  // kRedGroups * kRedLoads >= nblocks
__global__ __launch_bounds__(1024) void logreg_reduce_kernel(const float* __restrict__ partial,
                                                             int nblocks, int ncols,
                                                             double* __restrict__ out,
                                                             const int* __restrict__ done) {
  if (done != nullptr && *done) return;
  __shared__ double red[kRedGroups][kRedCols + 1];
  const int c = threadIdx.x & (kRedCols - 1), grp = threadIdx.x / kRedCols;
  const int col = blockIdx.x * kRedCols + c;
  double acc = 0.0;
  if (col < ncols) {
    for (int b0 = grp; b0 < nblocks; b0 += kRedGroups * kRedLoads) {
      float v[kRedLoads];
#pragma unroll
      for (int u = 0; u < kRedLoads; ++u) {
        const int b = b0 + u * kRedGroups;
        v[u] = b < nblocks ? partial[(int64_t)b * kLRPartStride + col] : 0.0f;
      }
      double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
#pragma unroll
      for (int u = 0; u < kRedLoads; u += 4) {
        a0 += (double)v[u];
        a1 += (double)v[u + 1];
        a2 += (double)v[u + 2];
        a3 += (double)v[u + 3];
      }
      acc += (a0 + a1) + (a2 + a3);
    }
  }
  red[grp][c] = acc;
  __syncthreads();
  // fixed-order tree over the 64 row-groups: 32 -> 16 -> ... -> 1
#pragma unroll
  for (int h = kRedGroups / 2; h > 0; h >>= 1) {
    if (grp < h) red[grp][c] += red[grp + h][c];
    __syncthreads();
  }
  if (grp == 0 && col < ncols) out[col] = red[0][c];
}

// ---- Newton / SGD state (fp64, on device) -------------------------------------------------
enum : int {
  kW = 0, kWPrev = 32, kStep = 64, kVel = 96,
  kObjPrev = 128, kIter = 129, kBacktracks = 130, kGmax = 131, kObj = 132, kNAccepted = 133,
  kConverged = 134, kStateSize = 256
};
static_assert(kStateSize == 256, "NewtonLds::ss is sized for the state");

__device__ void build_grad(const double* red, const double* st, int d, int fit_intercept,
                           double reg, double S, double* grad, int t) {
  if (t < kCols) {
    double gv = 0.0;
    if (t < d) gv = red[t] / S + reg * st[kW + t];
    else if (t == kBiasCol && fit_intercept) gv = red[t] / S;
    grad[t] = gv;
  }
}

// One wave (64 threads).  The kernel is latency-bound, so: all global loads (the reduced
// 1088-double vector, the 256-double state, the done flag) are in flight together before the
// first wait; reductions are wave-parallel; the Cholesky gives lane i row i (no integer
// division, one fp64 reciprocal per column); the triangular solves keep b in lane registers
// and broadcast with shuffles; barriers of a single-wave workgroup are nearly free.
// Weights for pivot-shifted rows s = x - pivot from the standardized-space state:
// v_j = w_j inv_j, v_30 = w_30 - sum_j w_j inv_j c_j (c = 0 off the feature columns).
__device__ __forceinline__ void store_folded(const double* ss, const double* cA, const double* iA,
                                             float* __restrict__ w32, int t) {
  double p = (t < 32) ? ss[kW + t] * iA[t] * cA[t] : 0.0;
  p = wave_sum(p);
  if (t < kCols)
    w32[t] = (t == kLabelCol) ? 0.0f : (t == kBiasCol) ? (float)(ss[kW + t] - p) : (float)(ss[kW + t] * iA[t]);
}

// In-kernel phase stamps (STAMP = true, tools/newton_stamps.py only): s_memtime at the phase
// boundaries, one asm statement with its own lgkmcnt(0) (cdna_hip_programming.md §7).
#define FDX_STAMP(i)                                                                              \
  do {                                                                                            \
    if constexpr (STAMP) {                                                                        \
      __builtin_amdgcn_sched_barrier(0);                                                          \
      unsigned long long t_;                                                                      \
      asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");                 \
      __builtin_amdgcn_sched_barrier(0);                                                          \
      tsv[i] = t_;                                                                                \
    }                                                                                             \
  } while (0)

// MT > 0: compile-time number of active coordinates (identity index map).  Lane t of one wave.
// SR_READY: L.sr already holds the reduced vector (the fused tail wrote it): no reload of red.
template <int MT, bool STAMP = false, bool SR_READY = false>
__device__ __forceinline__ void newton_update_body(const double* __restrict__ red, double* __restrict__ st, float* __restrict__ w32,
                                   int* __restrict__ done, int d, double C, double tol, int max_iter,
                                   int fit_intercept, int phase_start, const double* __restrict__ aff,
                                   unsigned long long* __restrict__ stamps, int* __restrict__ done_host, int seq,
                                   NewtonLds& L, int t) {
  unsigned long long tsv[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  FDX_STAMP(0);
  double* sr = L.sr;
  double* cA = L.cA;
  double* iA = L.iA;
  double* h30 = L.h30;
  double* ss = L.ss;
  double* grad = L.grad;
  int* idx = L.idx;
  auto Lc = [&L](int k, int r) -> double& { return L.sr[64 + k * 33 + r]; };
  {
    // Issue every global load before the first wait: 17 + 4 independent loads per lane plus
    // the done flag, instead of a load -> wait -> ds_write chain per element.
    constexpr int NR = kLRPartStride / 64, NS = kStateSize / 64;
    const int dn = *done;
    const double av = aff ? aff[t] : 0.0;
    double v[NR], u[NS];
    if constexpr (!SR_READY) {
#pragma unroll
      for (int i = 0; i < NR; ++i) v[i] = red[t + 64 * i];
    }
#pragma unroll
    for (int i = 0; i < NS; ++i) u[i] = st[t + 64 * i];
    if (dn) {
      if (done_host != nullptr && t == 0)
        __hip_atomic_store(done_host, (seq << 1) | 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      return;
    }
    if constexpr (!SR_READY) {
#pragma unroll
      for (int i = 0; i < NR; ++i) sr[t + 64 * i] = v[i];
    }
#pragma unroll
    for (int i = 0; i < NS; ++i) ss[t + 64 * i] = u[i];
    if (t < 32) cA[t] = av; else iA[t - 32] = av;
  }
  nsync();
  FDX_STAMP(1);
  if (aff) {
    // Rows hold s = x - pivot; standardized z = (s - c) * inv with c = inv = identity on the
    // intercept/label/padding columns.  The sums map exactly: g_z[j] = inv_j (g_j - c_j g_30),
    // H_z[j][k] = inv_j inv_k (H_jk - c_j H_30k - c_k H_j30 + c_j c_k H_30,30) (H symmetric).
    const double g30 = sr[kBiasCol];
    if (t < 32) h30[t] = sr[64 + kBiasCol * kCols + t];
    nsync();
    if (t < 32) sr[t] = iA[t] * (sr[t] - cA[t] * g30);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int e = t + 64 * i, j = e >> 5, k = e & 31;
      const double hv = sr[64 + e] - cA[j] * h30[k] - cA[k] * h30[j] + cA[j] * cA[k] * h30[kBiasCol];
      sr[64 + e] = iA[j] * iA[k] * hv;
    }
    nsync();
  }
  FDX_STAMP(2);
  const double S = sr[33] > 0.0 ? sr[33] : 1.0;
  const double reg = 1.0 / (C * S);
  const double invS = 1.0 / S;
  const int m = MT > 0 ? MT : d + (fit_intercept ? 1 : 0);
  const int my = (t < d) ? t : (t == d && fit_intercept ? kBiasCol : -1);
  if (t < 32) idx[t] = my;
  build_grad(sr, ss, d, fit_intercept, reg, S, grad, t);
  nsync();
  double w2 = (t < d) ? ss[kW + t] * ss[kW + t] : 0.0;
  double ga = (t < m) ? fabs(grad[my]) : 0.0;
  w2 = wave_sum(w2);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ga = fmax(ga, __shfl_xor(ga, o, kWave));
  const double obj = sr[32] * invS + 0.5 * reg * w2;
  const double gmax = ga;
  const int it = (int)ss[kIter];
  // phase_start: first iteration of a progressive-Newton phase -- objectives of different row
  // samples are not comparable, so no backtracking against the previous phase.
  const double prev = phase_start ? __builtin_inf() : ss[kObjPrev];
  const double nbt = phase_start ? 0.0 : ss[kBacktracks];
  // Backtrack only on a real increase: the loss is accumulated in fp32 per block (relative
  // noise ~1e-7), so near the optimum a true decrease can hide below that noise floor.
  int dec;
  if (it > 0 && obj > prev + 1e-6 * fabs(prev) && nbt < 40.0) dec = 1;
  else if (gmax <= tol) dec = 2;
  else dec = 0;
  nsync();
  if (t == 0) {
    ss[kObj] = obj;
    if (dec != 1) ss[kGmax] = gmax;
  }
  if (dec == 1) {  // objective went up: halve the last step from the last accepted point
    if (t < kCols) {
      ss[kStep + t] *= 0.5;
      ss[kW + t] = ss[kWPrev + t] + ss[kStep + t];
    }
    if (t == 0) ss[kBacktracks] = nbt + 1.0;
  } else if (dec == 2) {
    if (t == 0) {
      ss[kConverged] = 1.0;
      *done = 1;
    }
  } else {
    // Solve (H + reg*S*I_pen) s = -S*grad, i.e. (H/S + reg I_pen) s = -grad, by Cholesky in fp64.
    // Lane t owns row t of A in registers (a[32], fully unrolled: static indices).  With MT > 0
    // (compile-time m; the index map is then the identity) every guard below is static, so the
    // single wave -- whose cost is its instruction count -- runs a branch-free stream.  Column k
    // of L goes to LDS once (Lc[k][t]) for the back substitution, which reads column t
    // (Lc[t][k]).  1/sqrt: v_rsq_f64 + one
    // Newton refinement (~46 bits; the Newton step only needs to be a good descent direction).
    // Rows/columns >= m are identity-padded and never read back.
    const double regS = reg * S;
    // H may come from another row sample than g (sub-sampled warm-up, or a lazy-Hessian pass
    // reusing an older H): red[34] is the weight of the rows behind H, so H * S / S_H is the
    // sample-mean Hessian at the gradient's scale.
    const double hw = sr[34] > 0.0 ? S / sr[34] : 1.0;
    double a[32];
    {
      const int row = (MT > 0) ? (t < 32 ? t : 0) : (my >= 0 ? my : 0);
      const double* hr = sr + 64 + row * kCols;
#pragma unroll
      for (int k = 0; k < 32; ++k) {
        const int col = (MT > 0) ? k : idx[k];
        const double hv = hr[col < 0 ? 0 : col];
        const bool act = (t < m) && (k < m);
        const double dg = (k == t && my < d) ? regS : 0.0;
        a[k] = act ? fma(hv, hw, dg) : (k == t ? 1.0 : 0.0);
      }
    }
    double bi = (t < m) ? -grad[my < 0 ? 0 : my] * S : 0.0;
    nsync();  // every read of H (sr[64..]) before the first write of Lc, which reuses it
    FDX_STAMP(3);
    constexpr int JE = MT > 0 ? MT : 32;
    // Column k of L is broadcast to the trailing update with v_readlane (L[j][k] lives in lane j:
    // an SGPR operand of the fma) instead of an LDS write + wait + read-back per column, which
    // was ~680 cycles of a 31-step dependent chain (tools/newton_stamps.py).  The forward solve
    // L y = b rides in the same sweep (b is one more column of the right-hand side).
#pragma unroll
    for (int k = 0; k < 32; ++k) {
      if (k < m) {
        const double akk = fmax(rdlane(a[k], k), 1e-300);
        double inv = __builtin_amdgcn_rsq(akk);
        inv = inv * fma(-0.5 * akk * inv, inv, 1.5);
        if (t == k) L.dv[k] = inv;  // uniform: read back by the back substitution
        const double ak = (t == k) ? akk * inv : a[k] * inv;  // column k of L (rows t > k)
        a[k] = ak;
        if (t < 32) Lc(k, t) = ak;  // only the back substitution reads it (column t of lane t's row)
        const double yk = rdlane(bi, k) * inv;
        bi = (t == k) ? yk : (t > k ? fma(-ak, yk, bi) : bi);
#pragma unroll
        for (int j = k + 1; j < JE; ++j) a[j] = fma(-ak, rdlane(ak, j), a[j]);
      } else {
        if (t == 0) L.dv[k] = 0.0;
      }
    }
    FDX_STAMP(4);
    nsync();  // Lc and dv complete
#pragma unroll
    for (int k = 31; k >= 0; --k) {  // L^T x = y (column sweep): lane t < k needs L[k][t] = Lc[t][k]
      if (k < m) {
        const double xk = rdlane(bi, k) * L.dv[k];
        const double lkt = Lc(t & 31, k);
        bi = (t == k) ? xk : (t < k ? fma(-lkt, xk, bi) : bi);
      }
    }
    FDX_STAMP(5);
    if (t < kCols) {
      ss[kWPrev + t] = ss[kW + t];
      ss[kStep + t] = 0.0;
    }
    nsync();
    if (t < m) {
      ss[kStep + my] = bi;
      ss[kW + my] = ss[kWPrev + my] + bi;
    }
    if (t == 0) {
      ss[kObjPrev] = obj;
      ss[kBacktracks] = 0.0;
      ss[kNAccepted] += 1.0;
    }
  }
  nsync();
  if (t == 0) {
    ss[kIter] += 1.0;
    if (dec != 2 && (int)ss[kIter] >= max_iter) *done = 1;
    // done_host: a mapped pinned word (seq << 1 | done) the host polls -- no D2H copy kernel
    // and no event per convergence check; seq tells it that this launch has run.  A system-scope
    // store (written through to host memory, not left in L2 until the end of the stream)
    if (done_host != nullptr)
      __hip_atomic_store(done_host, (seq << 1) | *done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  nsync();
  if (aff) {
    store_folded(ss, cA, iA, w32, t);
  } else if (t < kCols) {
    w32[t] = (t == kLabelCol) ? 0.0f : (float)ss[kW + t];
  }
#pragma unroll
  for (int i = 0; i < kStateSize / 64; ++i) st[t + 64 * i] = ss[t + 64 * i];
  FDX_STAMP(6);
  if constexpr (STAMP) {
    if (t < 8) stamps[t] = tsv[t];
  }
}

template <int MT, bool STAMP = false>
__global__ __launch_bounds__(64) void newton_update_kernel(const double* __restrict__ red,
                                                           double* __restrict__ st,
                                                           float* __restrict__ w32,
                                                           int* __restrict__ done, int d, double C,
                                                           double tol, int max_iter,
                                                           int fit_intercept, int phase_start,
                                                           const double* __restrict__ aff,
                                                           unsigned long long* __restrict__ stamps = nullptr,
                                                           int* __restrict__ done_host = nullptr, int seq = 0) {
  __shared__ NewtonLds L;
  newton_update_body<MT, STAMP>(red, st, w32, done, d, C, tol, max_iter, fit_intercept, phase_start, aff, stamps,
                                done_host, seq, L, threadIdx.x);
}
#undef FDX_STAMP

// Behind a pass block's partials (NewtonFuse): group tickets, then the global one.  The last block
// of each group of kNewtonGroup blocks sums the group's partials in block order (fp64), the last
// group reducer sums the groups in order into nf.red and its first wave runs newton_update_body.
// Columns: [0, 35) and the Hessian [64, 1088) after a Hessian pass; [0, 34) after a gradient pass,
// whose update keeps red[34..] (the held Hessian and its weight), as logreg_reduce does.
// Cross-block data moves through agent-scope relaxed atomic stores and loads (coherent across the
// XCDs' L2s) ordered by vmcnt(0) before each arrival: no release/acquire fence, whose L2 write-back
// cost ~115 us per launch here (profiles/r6_t).
// Compact column i of the fused reduction -> its slot in the [1088] vector: [0, 35) as is, then the
// Hessian's upper triangle (j <= k) row by row.
__device__ __forceinline__ void newton_col(int i, int kLo, int& j, int& k) {
  if (i < kLo) {
    j = -1;
    k = i;
    return;
  }
  int e = i - kLo, r = 0;  // i < kLo + 528
  while (r < 31 && e >= 32 - r) {  // <= 31 steps, once per column
    e -= 32 - r;
    ++r;
  }
  j = r;
  k = r + e;
}

template <bool HESS>
__device__ __forceinline__ void newton_fused_tail(const float* __restrict__ partial, const NewtonFuse nf, void* lds) {
  __shared__ int s_last;
  const int t = threadIdx.x;
  const int nblk = gridDim.x, grp = blockIdx.x / kNewtonGroup;
  const int g0 = grp * kNewtonGroup, g1 = min(g0 + kNewtonGroup, nblk);
  const int ngroups = (nblk + kNewtonGroup - 1) / kNewtonGroup;
  unsigned int* tickets = reinterpret_cast<unsigned int*>(nf.ws);
  double* gsum = reinterpret_cast<double*>(nf.ws + (kNewtonMaxGroups + 2) / 2);
  constexpr int kLo = HESS ? 35 : 34;
  constexpr int kCnt = HESS ? kLo + 528 : kLo;
  constexpr int kPer = (kCnt + kThreads - 1) / kThreads;  // compact columns per thread (<= 3)
  auto slot = [](int j, int k) { return j < 0 ? k : 64 + j * kCols + k; };
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this thread's partial stores have landed
  __syncthreads();
  if (t == 0) {
    const unsigned q = __hip_atomic_fetch_add(tickets + grp, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_last = q == (unsigned)(g1 - g0 - 1) ? 1 : 0;
  }
  __syncthreads();
  if (!s_last) return;  // uniform per block
  int cj[kPer], ck[kPer];  // this thread's compact columns (out-of-range ones: unused)
#pragma unroll
  for (int r = 0; r < kPer; ++r) newton_col(min(t + r * kThreads, kCnt - 1), kLo, cj[r], ck[r]);
  if (t == 0) st_agent(tickets + grp, 0u);
  {  // the group's partials: every load of this thread in flight at once, summed in block order
    float v[kPer][kNewtonGroup];
#pragma unroll
    for (int r = 0; r < kPer; ++r) {
      const bool on = t + r * kThreads < kCnt;
      const float* p = partial + slot(cj[r], ck[r]);
#pragma unroll
      for (int u = 0; u < kNewtonGroup; ++u)
        v[r][u] = (on && g0 + u < g1) ? ld_agent(p + (int64_t)(g0 + u) * kLRPartStride) : 0.0f;
    }
#pragma unroll
    for (int r = 0; r < kPer; ++r) {
      double acc = 0.0;
#pragma unroll
      for (int u = 0; u < kNewtonGroup; ++u) acc += (double)v[r][u];
      if (t + r * kThreads < kCnt) st_agent(gsum + (int64_t)grp * kNewtonColStride + t + r * kThreads, acc);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (t == 0) {
    const unsigned q =
        __hip_atomic_fetch_add(tickets + kNewtonMaxGroups, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_last = q == (unsigned)(ngroups - 1) ? 1 : 0;
  }
  __syncthreads();
  if (!s_last) return;
  if (t == 0) st_agent(tickets + kNewtonMaxGroups, 0u);
  NewtonLds& L = *reinterpret_cast<NewtonLds*>(lds);
  // the groups, in order, kB loads per column in flight -> L.sr (H mirrored) and nf.red
  double acc[kPer];
#pragma unroll
  for (int r = 0; r < kPer; ++r) acc[r] = 0.0;
  constexpr int kB = 8;  // group sums per column in flight (registers: the pass's budget)
  for (int g = 0; g < ngroups; g += kB) {
    double v[kPer][kB];
#pragma unroll
    for (int r = 0; r < kPer; ++r) {
      const bool on = t + r * kThreads < kCnt;
      const double* p = gsum + t + r * kThreads;
#pragma unroll
      for (int u = 0; u < kB; ++u) v[r][u] = (on && g + u < ngroups) ? ld_agent(p + (int64_t)(g + u) * kNewtonColStride) : 0.0;
    }
#pragma unroll
    for (int r = 0; r < kPer; ++r) {
#pragma unroll
      for (int u = 0; u < kB; ++u) acc[r] += v[r][u];
    }
  }
  if constexpr (!HESS) {  // a gradient pass keeps the held Hessian and its weight: red[34..]
    for (int e = 34 + t; e < kLRPartStride; e += kThreads) L.sr[e] = nf.red[e];
  } else {
    if (t < 64 - kLo) L.sr[kLo + t] = 0.0;  // slots [35, 64): unused
  }
#pragma unroll
  for (int r = 0; r < kPer; ++r) {
    if (t + r * kThreads < kCnt) {
      const int j = cj[r], k = ck[r];
      L.sr[slot(j, k)] = acc[r];
      nf.red[slot(j, k)] = acc[r];
      if (j >= 0 && j != k) {
        L.sr[slot(k, j)] = acc[r];
        nf.red[slot(k, j)] = acc[r];
      }
    }
  }
  __syncthreads();
  if (t >= kWave) return;  // whole waves: the update is one wave's work
  if (nf.d == 30 && nf.fit_intercept)
    newton_update_body<31, false, true>(nf.red, nf.st, nf.w32, nf.done, nf.d, nf.C, nf.tol, nf.max_iter,
                                        nf.fit_intercept, nf.phase_start, nf.aff, nullptr, nf.done_host, nf.seq, L, t);
  else
    newton_update_body<0, false, true>(nf.red, nf.st, nf.w32, nf.done, nf.d, nf.C, nf.tol, nf.max_iter,
                                       nf.fit_intercept, nf.phase_start, nf.aff, nullptr, nf.done_host, nf.seq, L, t);
}


// Standardized-space weights (state) -> weights for pivot-shifted rows.  One wave.
__global__ __launch_bounds__(64) void logreg_fold_kernel(const double* __restrict__ st,
                                                         const double* __restrict__ aff,
                                                         float* __restrict__ w32) {
  __shared__ double ss[kW + 32], cA[32], iA[32];
  const int t = threadIdx.x;
  const double av = aff[t];
  if (t < 32) { cA[t] = av; ss[kW + t] = st[kW + t]; } else { iA[t - 32] = av; }
  __syncthreads();
  store_folded(ss, cA, iA, w32, t);
}

// Fit start: the whole workspace blob (state, w32, class weights, done flag) from kernel
// arguments, with the affine fold of w0 when the rows are pivot-shifted -- one launch instead of
// a pinned-staging H2D blit plus the fold kernel (a blit to/from host memory is ~9 us in the
// step timeline, profiles/r3_f/timeline_bf16_step.txt).
// w0_dev (nullable): the initial weights from device memory instead of the arguments -- another
// fit's standardized-space state (a CV fold warm-started from the previous fold, stream-ordered
// after that fit's enqueued iterations, no host round trip).
__device__ void persist_prep_block(unsigned long long* ws, const double* st, const float* w32, int done, int t,
                                   int nt);  // defined with the persistent workspace layout below

// pws (nullable): the persistent SGD workspace -- its prep (persist_prep_block) runs here too, one
// launch less per fit (SgdPersistArgs::prepped).
__global__ __launch_bounds__(64) void logreg_init_kernel(LRInitArgs a, double* __restrict__ st,
                                                         float* __restrict__ w32, float* __restrict__ cw,
                                                         int* __restrict__ done, const double* __restrict__ aff,
                                                         const double* __restrict__ w0_dev,
                                                         unsigned long long* __restrict__ pws) {
  __shared__ double ss[kW + 32], cA[32], iA[32];
  const int t = threadIdx.x;
  double w0 = 0.0;
#pragma unroll
  for (int j = 0; j < 32; ++j)  // static indices: no dynamic addressing of the argument struct
    if ((t & 31) == j) w0 = a.w0[j];
  if (w0_dev != nullptr) w0 = (t & 31) == kLabelCol ? 0.0 : w0_dev[t & 31];
  if (t < 32) ss[kW + t] = w0;
#pragma unroll
  for (int i = 0; i < kStateSize / 64; ++i) {
    const int e = t + 64 * i;
    double v = 0.0;
    if (e < 64) v = w0;  // kW and kWPrev
    else if (e == kObjPrev) v = __builtin_inf();
    st[e] = v;
  }
  if (t == 0) {
    cw[0] = a.cw0;
    cw[1] = a.cw1;
    *done = 0;
  }
  if (aff) {
    const double av = aff[t];
    if (t < 32) cA[t] = av; else iA[t - 32] = av;
    __syncthreads();
    store_folded(ss, cA, iA, w32, t);
  } else if (t < kCols) {
    w32[t] = (t == kLabelCol) ? 0.0f : (float)w0;
  }
  if (pws != nullptr) {
    // the state and weights this block just stored: one work-group on one CU, so a barrier is the
    // only ordering its own global reads need
    __syncthreads();
    persist_prep_block(pws, st, w32, 0, t, 64);
  }
}

// Solver state -> host: plain vector stores into a mapped pinned buffer (device address of the
// host allocation), replacing a D2H blit at the end of every fit.  seq != 0: then the stamp into
// word kStateSize once the wave's stores have landed -- the host polls it instead of an event.
__global__ __launch_bounds__(64) void logreg_export_kernel(const double* __restrict__ st, double* __restrict__ host,
                                                           long long seq) {
  const int t = threadIdx.x;
#pragma unroll
  for (int i = 0; i < kStateSize / 64; ++i)  // system scope: written through to host memory
    __hip_atomic_store(host + t + 64 * i, st[t + 64 * i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  if (seq != 0) {  // one wave: its vmcnt covers every lane's stores
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (t == 0)
      __hip_atomic_store(reinterpret_cast<long long*>(host + kStateSize), seq, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// ---- minibatch SGD (config 3: "SMOTE k-NN + logistic SGD") --------------------------------------
// One step = one pass over minibatch b of the epoch (row_phase b: 1/nb of the stored row tiles and
// of the virtual-SMOTE pick tiles, logreg_pass_kernel) + this update.  Heavy-ball momentum on the
// minibatch gradient of sklearn's objective, with the step size normalised by the minibatch's mean
// Gauss-Newton curvature dbar = sum s p (1-p) / sum s (slot 35 of the FISH pass):
//     lr_t = c_epoch / dbar_t,   v <- mom v - lr_t g_b(w),   w <- w + v.
// Standardized features make the curvature ~ dbar x (feature covariance), so c is a
// dimensionless step that stays valid as the model sharpens (dbar falls 0.25 -> ~0.05 on the
// bench data while the curvature falls with it).  Polyak-Ruppert averaging (sklearn
// SGDClassifier(average=True)): the steps flagged `avg` add w to a running sum and the epoch end
// returns their mean.  Every epoch end also settles the convergence state from the epoch's sums:
// the epoch gradient sum_b g_b(w_b) / sum_b S_b (for a near-quadratic objective, the gradient at
// the averaged iterate) -> kGmax, the epoch's mean loss + penalty -> kObj, kConverged when
// kGmax <= tol, and `done` (every later pass and update of the fit is a no-op).
enum : int { kAvg = 160, kEpG = 192, kEpLoss = 224, kEpW = 225, kNAvg = 226, kDbar = 227, kLr = 228 };
constexpr double kDbarFloor = 1e-3;  // lr_t <= c / 1e-3: a saturated minibatch cannot blow the step up
constexpr int kSgdSlots = 36;        // grad[32] | loss | weight | (34: unused) | curvature sum

// The barrier between sgd_apply's phases: the whole block's (kWaveOnly false) or the calling wave's.
template <bool kWaveOnly>
__device__ __forceinline__ void sgd_sync() {
  if constexpr (kWaveOnly) nsync();
  else __syncthreads();
}

// kWaveOnly: ONE wave calls it (t = its lane) and its phases are ordered by wave barriers only --
// the persistent launch's arriving wave applies the step while the block's other waves wait at
// one block barrier (the same operations in the same order: bitwise the block version's state).
template <bool kWaveOnly>
__device__ void sgd_apply(const double* rd, double* __restrict__ st, float* __restrict__ w32, int* __restrict__ done,
                          const double* __restrict__ aff, const SgdArgs& a, int t, bool mapped) {
  // rd: the reduced [36] sums in LDS (raw row space; standardized space when `mapped`).  kWaveOnly
  // false: EVERY thread of the block calls this from block-uniform control flow -- it holds block
  // barriers, under conditions (aff, a.epoch_end) that are kernel arguments; only the first wave
  // (t < 64) reads or writes state.
  __shared__ double rz[32], ss[kW + 32], cA[32], iA[32];
  if (aff) {
    if (t < 64) {
      const double av = aff[t];
      if (t < 32) cA[t] = av; else iA[t - 32] = av;
    }
    sgd_sync<kWaveOnly>();
  }
  const double S = rd[33] > 0.0 ? rd[33] : 1.0;
  // mapped: the sums arrive in standardized space already (fused passes map them per block)
  if (t < 32) rz[t] = (aff && !mapped) ? iA[t] * (rd[t] - cA[t] * rd[kBiasCol]) : rd[t];
  const double reg = 1.0 / (a.C * S * (double)a.nb);  // the minibatch estimates sum s over the epoch as nb S
  const double dbar = fmax(rd[35] / S, kDbarFloor);
  const double lr = a.c / dbar;
  sgd_sync<kWaveOnly>();
  if (t < kCols) {
    double g = 0.0;
    if (t < a.d) g = rz[t] / S + reg * st[kW + t];
    else if (t == kBiasCol && a.fit_intercept) g = rz[t] / S;
    const double v = a.momentum * st[kVel + t] - lr * g;
    const double wn = st[kW + t] + v;
    st[kVel + t] = v;
    st[kEpG + t] += rz[t];
    if (a.avg) st[kAvg + t] += wn;
    ss[kW + t] = wn;
  }
  sgd_sync<kWaveOnly>();
  if (t == 0) {
    st[kEpLoss] += rd[32];
    st[kEpW] += rd[33];
    if (a.avg) st[kNAvg] += 1.0;
    st[kIter] += 1.0;
    st[kDbar] = dbar;
    st[kLr] = lr;
  }
  sgd_sync<kWaveOnly>();
  if (a.epoch_end) {
    const double Sw = st[kEpW] > 0.0 ? st[kEpW] : 1.0;
    const double na = st[kNAvg];
    if (t < kCols && na > 0.0) ss[kW + t] = st[kAvg + t] / na;  // the averaged iterate is the model
    sgd_sync<kWaveOnly>();
    double g = 0.0;
    if (t < a.d) g = st[kEpG + t] / Sw + ss[kW + t] / (a.C * Sw);
    else if (t == kBiasCol && a.fit_intercept) g = st[kEpG + t] / Sw;
    double ga = t < kCols ? fabs(g) : 0.0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ga = fmax(ga, __shfl_xor(ga, o, kWave));
    double w2 = (t < a.d) ? ss[kW + t] * ss[kW + t] : 0.0;
    w2 = wave_sum(w2);
    if (t < kCols) {
      st[kEpG + t] = 0.0;
      st[kAvg + t] = 0.0;
    }
    sgd_sync<kWaveOnly>();
    if (t == 0) {
      st[kGmax] = ga;
      st[kObj] = st[kEpLoss] / Sw + 0.5 * w2 / (a.C * Sw);
      st[kEpLoss] = 0.0;
      st[kEpW] = 0.0;
      st[kNAvg] = 0.0;
      if (ga <= a.tol) {
        st[kConverged] = 1.0;
        *done = 1;
      }
    }
  }
  sgd_sync<kWaveOnly>();
  if (t < kCols) st[kW + t] = ss[kW + t];
  if (aff) {
    store_folded(ss, cA, iA, w32, t);
  } else if (t < kCols) {
    w32[t] = (t == kLabelCol) ? 0.0f : (float)ss[kW + t];
  }
}

// One process: the fixed-order fp64 reduction of the pass's [nblocks][36] partials and the update in
// ONE launch (the reduce kernel + update kernel pair costs a kernel boundary and a second launch per
// step).  1008 threads = 36 columns x 28 row-groups; every thread's loads are issued before the
// first wait (the partials sit in L2/MALL: the kernel is load-latency bound); the 28 row-group
// sums are combined in a fixed order, then wave 0 applies the step.
constexpr int kSgdGroups = 28, kSgdLoads = 12;
__global__ __launch_bounds__(1024) void sgd_step_kernel(const float* __restrict__ partial, int nblocks,
                                                       double* __restrict__ st, float* __restrict__ w32,
                                                       int* __restrict__ done, const double* __restrict__ aff,
                                                       SgdArgs a) {
  if (*done) return;
  __shared__ double part[kSgdGroups][kSgdSlots];
  __shared__ double rd[kSgdSlots];
  const int c = threadIdx.x % kSgdSlots, grp = threadIdx.x / kSgdSlots;
  if (grp < kSgdGroups) {
    double acc = 0.0;
    for (int b0 = grp; b0 < nblocks; b0 += kSgdGroups * kSgdLoads) {
      float v[kSgdLoads];
#pragma unroll
      for (int u = 0; u < kSgdLoads; ++u) {
        const int b = b0 + u * kSgdGroups;
        v[u] = (b < nblocks && c != 34) ? partial[(int64_t)b * kLRPartStride + c] : 0.0f;
      }
      double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
#pragma unroll
      for (int u = 0; u < kSgdLoads; u += 4) {
        a0 += (double)v[u];
        a1 += (double)v[u + 1];
        a2 += (double)v[u + 2];
        a3 += (double)v[u + 3];
      }
      acc += (a0 + a1) + (a2 + a3);
    }
    part[grp][c] = acc;
  }
  __syncthreads();
  if (threadIdx.x < kSgdSlots) {
    double r = 0.0;
#pragma unroll 4
    for (int g = 0; g < kSgdGroups; ++g) r += part[g][threadIdx.x];
    rd[threadIdx.x] = r;
  }
  __syncthreads();
  sgd_apply(rd, st, w32, done, aff, a, threadIdx.x, false);
}

// Data parallel: the reduced sums were all-reduced across ranks in `red` (logreg_reduce with 36
// columns, then the collective); the same update from global memory.
__global__ __launch_bounds__(64) void sgd_update_kernel(const double* __restrict__ red, double* __restrict__ st,
                                                        float* __restrict__ w32, int* __restrict__ done,
                                                        const double* __restrict__ aff, SgdArgs a) {
  if (*done) return;
  __shared__ double rd[kSgdSlots];
  const int t = threadIdx.x;
  if (t < kSgdSlots) rd[t] = red[t];
  __syncthreads();
  sgd_apply(rd, st, w32, done, aff, a, t, false);
}

// Data parallel lean step: the update from the all-reduced fixed-point sums of
// launch_sgd_pass_sums (int64, 2^-20 units; slot 34 unused).
__global__ __launch_bounds__(64) void sgd_update_fixed_kernel(const long long* __restrict__ sums,
                                                              double* __restrict__ st, float* __restrict__ w32,
                                                              int* __restrict__ done,
                                                              const double* __restrict__ aff, SgdArgs a) {
  if (*done) return;
  __shared__ double rd[kSgdSlots];
  const int t = threadIdx.x;
  if (t < kSgdSlots) rd[t] = (double)sums[t] * (1.0 / kFixScale);
  __syncthreads();
  sgd_apply(rd, st, w32, done, aff, a, t, true);
}

// ---- persistent SGD: the whole schedule in ONE launch --------------------------------------------
// The per-step launches pay, per step, a kernel boundary, the grid's fill and drain, and the serial
// update in the last-arriving block (~14 us of a ~26 us step at the bench shape, profiles/r4_g).
// Here one 512-thread block (kPersistWaves = 8 waves) per CU runs every step: wave wv of block b is
// wave wv * B + b of the per-step grid (B = blocks; bf16_wave_pass / fp8_wave_pass walk the same row
// and pick tiles), so a step's sums are the per-step launch's sums.  Step t:
//   pass over minibatch b -> every wave's [36] sums in LDS -> the block's LAST wave (kArriveWave)
//   turns each wave's sums into 2^-20 fixed point exactly as sgd_fused_tail does, adds the block's
//   total into replica (block mod kPersistReplicas = 16) of accumulator set t mod 3 with
//   agent-scope int64 atomics, and arrives at the grid barrier -> in every block that same wave
//   reads the set with agent-scope loads and applies the SAME update (sgd_apply<true>: wave
//   barriers only, while the block's other waves wait at one block barrier; 3.5 -> 2.0 us per step,
//   profiles/r6_wave_update) to the block's LDS copy of the solver state.  Integer sums are order-free and every block runs the same fp64 code on the same
//   inputs, so every block holds bitwise the same state -- and bitwise the per-step launches'
//   state; the convergence flag is therefore uniform across the grid with no broadcast.
// Hand-offs (MI355X_MICROARCH.md, inter-workgroup visibility): the payload is written only by
// agent-scope atomics and read only by agent-scope atomic loads after the barrier, the arrival is an
// agent atomic add made after the adding wave's vmcnt(0), the poll a relaxed agent load -- the
// "8-B agent atomics both sides" form, one workgroup per CU.  Sets rotate over three: set t is read
// after barrier t; set t + 1 is zeroed by block 0 during step t (after barrier t - 1, when every
// block has finished reading it as set t - 2; before block 0 arrives at barrier t).
// Residency: the grid is sized from the occupancy query (FDX_SGD_COOP=1 launches it through
// hipLaunchCooperativeKernel, which re-checks that at launch and refuses an oversize grid; the caller
// then launches per step), but co-residency can still fail at run time when another stream or
// process holds CUs.  So every wait is bounded: a block
// whose barrier poll times out (or that sees another block's timeout) raises the workspace's fault
// word and leaves; blocks dispatched after that exit at once; nothing is published from a faulted
// grid.  The one-block recovery launch queued behind every persistent launch (sgd_recover_kernel)
// is a no-op unless the fault word is set; then it re-runs the steps from the backup of the
// initial state (sgd_persist_prep_kernel) with the same per-wave fixed-point sums -- bitwise the fit
// the persistent launch would have produced, at one CU's speed.
constexpr int kPersistWaves = 8;
constexpr int kPersistThreads = kPersistWaves * kWave;
constexpr int kBarShards = 8, kBarStride = 32;  // arrival shards, one 128-B line each (u32 words)
enum : int { kSgdFault = 229 };                 // state slot: 2 = the fit ran on the recovery launch
// stamps (tools/sgd_stamps.py): [step][kStampRows][block] wall_clock64 -- pass end, barrier exit,
// update end, then every wave's own pass end
constexpr int kStampRows = 3 + kPersistWaves;
// The wave that reduces the block's sums, zeroes the next accumulator set (block 0) and arrives at
// the barrier: the LAST wave of the block.  The pick tiles of a step sit on the low wave indices
// (wave wv of block b is wave wv * B + b of the pass grid), i.e. on wave 0 of every block, whose
// next-pick input chain (dependent loads) would otherwise delay the arrival (r5_h stamps: an
// 8.4 us block epilogue after the last wave's pass).
constexpr int kArriveWave = kPersistWaves - 1;
// Accumulator replicas of the persistent launch: 256 blocks over 16 replicas (16 adds per word;
// 16 and 8 both took the fit 608 -> 585 us, r5_t / r5_u).
// Every block folds all of them after the barrier, so fewer replicas is fewer loads per update.
constexpr int kPersistReplicas = 16;
constexpr int kPersistAccWords = kPersistReplicas * 36;
// Workspace layout (int64 words, launchers.h kSgdPersistWords): barrier shards | 3 accumulator sets
// | fault word | backup of the initial state [kStateSize], weights [16 words = 32 floats], done.
enum : int {
  kWsAcc = 128,
  kWsFault = kWsAcc + 3 * kPersistAccWords,
  kWsBackup = kWsFault + 8,  // zeroed per launch: [0, kWsBackup)
  kWsBackupW = kWsBackup + kStateSize,
  kWsBackupDone = kWsBackupW + 16,
  kWsEnd = kWsBackupDone + 1
};
static_assert(kWsEnd <= kSgdPersistWords, "launchers.h kSgdPersistWords too small for the persistent workspace");
static_assert(kBarShards * kBarStride <= 2 * kWsAcc, "barrier shards overlap the accumulator sets");
// Template knobs: LAMS = lambdas in flight per lane in a pick (integer sums: any grouping gives the
// same bits); PF = what is loaded for the next step before the barrier: 0 nothing; 1 the first pick
// tile's inputs and the first stored tile into registers; 2 the pick inputs + an L2 touch of the
// stored tile; 3 the pick inputs only; DEPTH = stored bf16 tiles in flight per wave (bf16_wave_pass
// kDepth).  LAMS 16/32 x PF 0-3 all ran within 735-778 us per fit (profiles/r5_e/sgd_lab.json);
// FDX_SGD_PERSIST_CFG=1 (lab) selects DEPTH 1, the round-4 stored-tile pipeline.

// The arriving wave of a block: arrive at the grid barrier and wait until `target` arrivals in all.
// false: the wait timed out (spin_limit polls) or another block had already given up (fault word);
// the fault word is raised either way.
__device__ __forceinline__ bool persist_barrier(unsigned int* bar, unsigned target, int lane, unsigned int* fault,
                                                unsigned spin_limit) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's accumulator adds have landed
  if (lane == 0)
    __hip_atomic_fetch_add(bar + (blockIdx.x % kBarShards) * kBarStride, 1u, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
  for (unsigned spins = 0;; ++spins) {
    int v = lane < kBarShards ? (int)__hip_atomic_load(bar + lane * kBarStride, __ATOMIC_RELAXED,
                                                       __HIP_MEMORY_SCOPE_AGENT) : 0;
    const int f = lane == kBarShards ? (int)__hip_atomic_load(fault, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
    v += __shfl_xor(v, 1, kWave);
    v += __shfl_xor(v, 2, kWave);
    v += __shfl_xor(v, 4, kWave);
    v = __shfl(v, 0, kWave);
    if ((unsigned)v >= target) return true;
    if (__shfl(f, kBarShards, kWave) != 0 || spins > spin_limit) {  // not every block is resident
      if (lane == 0) __hip_atomic_store(fault, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      return false;
    }
  }
}

// One wave's share of a step's pass -- wave `wave` of the per-step grid of Gw waves, minibatch b of
// a grid of rsub -- into red[wv][0..35] (gradient in row units | loss | weight | 0 | curvature).  The
// persistent launch (with the next tiles prefetched across its barrier) and the one-block recovery
// launch (a loop over the grid's waves) run the same code, so their per-wave sums are equal.
template <bool FP8, bool VIRT, int kLams, int kPreLams, int kDepth>
__device__ __forceinline__ void persist_wave_sums(const void* __restrict__ X, int64_t row_end, float x_scale,
                                                  float inv_s, float cw0, float cw1, const float* wsh,
                                                  const SmoteView& sv, const RowHole& hole, int64_t wave, int64_t Gw,
                                                  bool active, int rsub, int b, float (*red)[36], int wv, int lane,
                                                  const uint4 (&pre)[4], bool have_pre,
                                                  const PickIn<4, kPreLams>& ppre, bool have_ppre) {
  constexpr int d_feat = 30;
  float lacc = 0.0f, wacc = 0.0f, whacc = 0.0f, dacc = 0.0f;
  f32x16_t hacc = {};
  if constexpr (FP8) {
    const int q = lane & 1;
    f32x2_t wl[8], g[8];
#pragma unroll
    for (int p = 0; p < 8; ++p) {
      wl[p] = f32x2_t{wsh[16 * q + 2 * p], wsh[16 * q + 2 * p + 1]};
      g[p] = f32x2_t{0.0f, 0.0f};
    }
    if (active)
      fp8_wave_pass<false, VIRT, true, kLams, kPreLams>(static_cast<const uint8_t*>(X), 0, row_end, wl, wsh, x_scale,
                                                        cw0, cw1, 1, rsub, b, sv, hole, wave, Gw, nullptr, g, lacc,
                                                        wacc, whacc, dacc, hacc, pre, have_pre, ppre, have_ppre);
    float gs[16];
#pragma unroll
    for (int p = 0; p < 8; ++p) {
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int col = 16 * q + 2 * p + e;
        gs[2 * p + e] = strided_sum<2>(g[p][e]) * (col < d_feat ? inv_s : 1.0f);
      }
    }
    if (lane < 2) {
#pragma unroll
      for (int j = 0; j < 16; ++j) red[wv][16 * lane + j] = gs[j];
    }
  } else {
    const int q = lane & 3;
    float wl[8], g[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      wl[j] = wsh[q * 8 + j];
      g[j] = 0.0f;
    }
    if (active)
      bf16_wave_pass<false, VIRT, true, kLams, kPreLams, kDepth>(X, 0, row_end, wl, cw0, cw1, 1, rsub, b, sv, hole,
                                                                 wave, Gw, nullptr, g, lacc, wacc, whacc, dacc, hacc,
                                                                 pre, have_pre, ppre, have_ppre);
#pragma unroll
    for (int j = 0; j < 8; ++j) g[j] = strided_sum<4>(g[j]);
    if (lane < 4) {
#pragma unroll
      for (int j = 0; j < 8; ++j) red[wv][8 * lane + j] = g[j];
    }
  }
  lacc = wave_sum(lacc);
  wacc = wave_sum(wacc);
  dacc = wave_sum(dacc);
  if (lane == 0) {
    red[wv][32] = lacc;
    red[wv][33] = wacc;
    red[wv][34] = 0.0f;
    red[wv][35] = dacc;
  }
}

// Step st of the schedule -> (epoch, position in it, minibatch phase, grid of the epoch's minibatches):
// an epoch with sub-sample s visits every s-th phase of a grid of nbe * s minibatches.
struct PersistStep {
  int ep, pos, phase, rsub;
  __device__ __forceinline__ PersistStep(const SgdPersistArgs& P, int st) {
    int e = 0;
    while (e + 1 < P.epochs && st >= P.estart[e + 1]) ++e;
    ep = e;
    pos = st - P.estart[e];
    phase = ((P.serpentine && (e & 1)) ? P.nbe[e] - 1 - pos : pos) * P.sub[e];
    rsub = P.nbe[e] * P.sub[e];
  }
  __device__ __forceinline__ SgdArgs args(const SgdPersistArgs& P) const {
    SgdArgs a;
    a.d = P.d;
    a.C = P.C;
    a.c = P.lr[ep];
    a.momentum = P.momentum;
    a.fit_intercept = P.fit_intercept;
    a.nb = rsub;  // the minibatch estimates the epoch's weight as rsub x its own
    a.avg = ep >= P.avg_from;
    a.epoch_end = pos == P.nbe[ep] - 1;
    a.tol = P.sub[ep] > 1 ? -1.0 : P.tol;  // a sub-sampled epoch never decides convergence
    return a;
  }
};

template <bool FP8, bool VIRT, int kPersistLams = 16, int kPersistPrefetch = 2, int kPersistDepth = 2>
__global__ __launch_bounds__(kPersistThreads, 1) void sgd_persist_kernel(const void* __restrict__ X,
                                                                         int64_t row_end, float x_scale,
                                                                         const float* __restrict__ class_w,
                                                                         SmoteView sv, RowHole hole,
                                                                         SgdPersistArgs P) {
  __shared__ double sst[kStateSize];                      // this block's copy of the solver state
  __shared__ __attribute__((aligned(16))) float wsh[32];  // weights of the passes (fp8: row units)
  __shared__ float wnew[32];                              // sgd_apply's folded weights
  __shared__ float red[kPersistWaves][36];
  __shared__ double rd[kSgdSlots];
  __shared__ int s_done, s_ok;
  __shared__ double saff[64];  // the affine map, read from LDS by every step's reduce and update
  const int t = threadIdx.x, lane = lane_id(), wv = wave_id();
  constexpr int d_feat = 30;
  unsigned int* bar = reinterpret_cast<unsigned int*>(P.ws);
  unsigned long long* accs = P.ws + kWsAcc;
  unsigned int* fault = reinterpret_cast<unsigned int*>(P.ws + kWsFault);
  if (t == 0) {  // dispatched after another block gave up: leave at once (nothing to wait for)
    s_done = *P.done;
    s_ok = __hip_atomic_load(fault, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u;
  }
  if (P.aff != nullptr && t < 64) saff[t] = P.aff[t];
  const double* affl = P.aff != nullptr ? saff : nullptr;
  const float inv_s = FP8 ? 1.0f / x_scale : 1.0f;
  for (int e = t; e < kStateSize; e += kPersistThreads) sst[e] = P.st[e];
  if (t < 32) {
    const float w = P.w32[t];
    wnew[t] = w;
    wsh[t] = t == kLabelCol ? 0.0f : w * ((FP8 && t < d_feat) ? inv_s : 1.0f);
  }
  __syncthreads();
  if (!s_ok) return;  // uniform in the block
  if (t == 0) sst[kSgdFault] = 0.0;
  const float cw0 = class_w[0], cw1 = class_w[1];
  // wave wv of block b is wave wv * B + b of the per-step grid: the waves that carry the pick tiles
  // (the low wave indices) spread over every CU instead of filling the first ones
  const int64_t wave = (int64_t)wv * gridDim.x + blockIdx.x;
  const bool active = wave < P.Gw;
  const int64_t n = pass_stored_rows<VIRT>(0, row_end, sv, hole);
  uint4 pre[4];
  bool have_pre = false;
  constexpr int kPreLams = 32;
  PickIn<4, kPreLams> ppre;  // the wave's next pick tile, loaded before the barrier
  bool have_ppre = false;
  const int64_t npick = VIRT ? (int64_t)sv.mq * sv.k : 0;
  const int64_t ntile = (npick + 15) >> 4;
  unsigned touch = 0;  // FDX_PERSIST_PREFETCH 2: the dummy destination of the L2 touch loads
  unsigned arrivals = 0;
  auto prefetch = [&](int st) {  // the wave's first tile(s) of step st: rows do not depend on w
    have_pre = false;
    have_ppre = false;
    if (kPersistPrefetch == 0 || !active || st >= P.s1) return;
    const PersistStep S(P, st);
    if constexpr (VIRT) {  // the inputs of the wave's first pick tile of step st
      const int64_t pt = wave * S.rsub + S.phase;
      if (pt < ntile) {
        const int64_t p = pt * 16 + (lane >> 2);
        pick_load<4, kPreLams>(sv, p < npick ? p : -1, lane & 3, ppre);
        have_ppre = true;
      }
    }
    const int64_t base = ((int64_t)wave * S.rsub + S.phase) * 64;  // bf16_wave_pass tile walk
    if (kPersistPrefetch == 3 || base >= n) return;
    if constexpr (kPersistPrefetch == 2) {
      // L2 touch: one dword per row of the first tile, into a register nobody reads (held until
      // the next step's explicit vmcnt(0) so the compiler never reuses it while in flight)
      const int64_t row = base + lane;
      if (row < n) {
        const int64_t ph = row + (row >= hole.at ? hole.len : 0);
        const char* a = static_cast<const char*>(X) + ph * (FP8 ? 32 : 64);
        asm volatile("global_load_dword %0, %1, off" : "=v"(touch) : "v"(a) : "memory");
      }
      return;
    }
    if constexpr (FP8) {
      const uint8_t* X8 = static_cast<const uint8_t*>(X);
      uint4 a[2], b[2] = {make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0)};
      fp8_load_tile(X8, 0, n, hole, base, a);
      const int64_t step_rows = P.Gw * 64 * S.rsub;
      if (base + step_rows < n) fp8_load_tile(X8, 0, n, hole, base + step_rows, b);
      pre[0] = a[0]; pre[1] = a[1]; pre[2] = b[0]; pre[3] = b[1];
    } else {
      bf16_load_tile(X, 0, n, hole, base, pre);
    }
    have_pre = true;
  };

  for (int st = P.s0; st < P.s1 && !s_done; ++st) {
    if constexpr (kPersistPrefetch == 2) asm volatile("s_waitcnt vmcnt(0)" : "+v"(touch) : : "memory");
    const PersistStep S(P, st);
    unsigned long long* acc = accs + (st % 3) * kPersistAccWords;
    if (blockIdx.x == 0 && wv == kArriveWave) {  // set st + 1 (read as set st - 2 before barrier st - 1)
      unsigned long long* nx = accs + ((st + 1) % 3) * kPersistAccWords;
      for (int e = lane; e < kPersistAccWords; e += kWave)
        __hip_atomic_store(nx + e, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // ---- the pass over minibatch S.phase (this wave's share) ----
    persist_wave_sums<FP8, VIRT, kPersistLams, kPreLams, kPersistDepth>(
        X, row_end, x_scale, inv_s, cw0, cw1, wsh, sv, hole, wave, P.Gw, active, S.rsub, S.phase, red, wv, lane, pre,
        have_pre, ppre, have_ppre);
    if (P.stamps != nullptr && lane == 0)
      P.stamps[((int64_t)(st - P.s0) * kStampRows + 3 + wv) * gridDim.x + blockIdx.x] = wall_clock64();
    __syncthreads();
    if (wv != kArriveWave) {
      prefetch(st + 1);  // the pick tiles' waves run their pick-input chains during the barrier
    } else {
      // sgd_fused_tail's per-wave fixed point (inactive waves hold zeros)
      const long long qs = lane < kSgdSlots ? wave_sums_fixed<kPersistWaves>(red, affl, lane) : 0;
      prefetch(st + 1);  // no pick tile on this wave: an L2 touch, in flight beside the adds
      if (lane < kSgdSlots && lane != 34 && qs != 0)
        __hip_atomic_fetch_add(acc + (blockIdx.x % kPersistReplicas) * 36 + lane, (unsigned long long)qs,
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      // the fault-test knob: barrier s0 waits for one arrival more than the grid has
      arrivals += gridDim.x + ((P.fault_test && st == P.s0) ? 1u : 0u);
      if (P.stamps != nullptr && lane == 0)
        P.stamps[((int64_t)(st - P.s0) * kStampRows + 0) * gridDim.x + blockIdx.x] = wall_clock64();
      const bool ok = persist_barrier(bar, arrivals, lane, fault, P.spin_limit);
      if (P.stamps != nullptr && lane == 0)
        P.stamps[((int64_t)(st - P.s0) * kStampRows + 1) * gridDim.x + blockIdx.x] = wall_clock64();
      if (!ok) {
        if (lane == 0) s_ok = 0;
      } else {
        // ---- the update, redundantly in every block, by this wave alone (wave barriers only;
        // the block's other waves wait at the one block barrier below) ----
        if (lane < kSgdSlots) {  // the replicas' sums (integer: exact in any order)
          unsigned long long v[kPersistReplicas];
#pragma unroll
          for (int r = 0; r < kPersistReplicas; ++r)
            v[r] = __hip_atomic_load(acc + r * 36 + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          unsigned long long q = 0;
#pragma unroll
          for (int r = 0; r < kPersistReplicas; ++r) q += v[r];
          rd[lane] = (double)(long long)q * (1.0 / kFixScale);
        }
        nsync();
        sgd_apply<true>(rd, sst, wnew, &s_done, affl, S.args(P), lane, true);
        nsync();
        if (lane < 32) wsh[lane] = lane == kLabelCol ? 0.0f : wnew[lane] * ((FP8 && lane < d_feat) ? inv_s : 1.0f);
      }
    }
    __syncthreads();
    if (!s_ok) return;  // uniform in the block: a faulted grid publishes nothing
    if (P.stamps != nullptr && t == 0)
      P.stamps[((int64_t)(st - P.s0) * kStampRows + 2) * gridDim.x + blockIdx.x] = wall_clock64();
  }
  if (blockIdx.x == 0) {  // every block holds the same state: block 0 publishes it
    for (int e = t; e < kStateSize; e += kPersistThreads) P.st[e] = sst[e];
    if (t < 32) P.w32[t] = wnew[t];
    if (t == 0) *P.done = s_done;
  }
}

// In front of every persistent launch (replaces a memset): zero the barrier shards, the accumulator
// sets and the fault word, and back up the initial solver state, weights and done flag for the
// recovery launch (a faulted grid may have advanced some blocks' copies; the recovery restarts from
// exactly what the persistent launch started from).
__device__ void persist_prep_block(unsigned long long* ws, const double* st, const float* w32, int done, int t,
                                   int nt) {
  for (int e = t; e < kWsBackup; e += nt) ws[e] = 0ull;
  double* bst = reinterpret_cast<double*>(ws + kWsBackup);
  for (int e = t; e < kStateSize; e += nt) bst[e] = st[e];
  float* bw = reinterpret_cast<float*>(ws + kWsBackupW);
  if (t < 32) bw[t] = w32[t];
  if (t == 0) ws[kWsBackupDone] = (unsigned long long)(unsigned)done;
}

__global__ __launch_bounds__(256) void sgd_persist_prep_kernel(unsigned long long* __restrict__ ws,
                                                               const double* __restrict__ st,
                                                               const float* __restrict__ w32,
                                                               const int* __restrict__ done) {
  persist_prep_block(ws, st, w32, *done, threadIdx.x, 256);
}

// The fit's final state -> the mapped pinned slot (system-scope stores, written through to host
// memory), then the slot's stamp once every thread's stores have landed: the host polls the stamp
// (PendingFit) instead of an event recorded behind the launch.  Whole block, uniform.
__device__ __forceinline__ void export_state_stamped(double* host, const double* src, long long seq, int t) {
  for (int e = t; e < kStateSize; e += kPersistThreads)
    __hip_atomic_store(host + e, src[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (t == 0)
    __hip_atomic_store(reinterpret_cast<long long*>(host + kStateSize), seq, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_SYSTEM);
}

// Behind every persistent launch: a no-op unless its fault word is set.  Then one block re-runs
// steps [s0, s1) from the backup: its 8 waves walk the per-step grid's Gw waves in turn, each
// wave's sums go to fixed point on their own (the persistent launch converts per wave too), so the
// integer step sums -- and the fit -- are bitwise those of a persistent launch that had run; state
// slot kSgdFault = 2 records the recovery.  Its barrier is __syncthreads: one block is always
// resident eventually.
template <bool FP8, bool VIRT>
__global__ __launch_bounds__(kPersistThreads, 1) void sgd_recover_kernel(const void* __restrict__ X, int64_t row_end,
                                                                         float x_scale,
                                                                         const float* __restrict__ class_w,
                                                                         SmoteView sv, RowHole hole,
                                                                         SgdPersistArgs P) {
  if (__hip_atomic_load(reinterpret_cast<unsigned int*>(P.ws + kWsFault), __ATOMIC_RELAXED,
                        __HIP_MEMORY_SCOPE_AGENT) == 0u) {  // uniform: the word the previous launch left
    if (P.export_host != nullptr)  // the fit's final state -> the mapped pinned slot (logreg_export)
      export_state_stamped(P.export_host, P.st, P.export_seq, threadIdx.x);
    return;
  }
  __shared__ double sst[kStateSize];
  __shared__ __attribute__((aligned(16))) float wsh[32];
  __shared__ float wnew[32];
  __shared__ float red[kPersistWaves][36];
  __shared__ long long qw[kPersistWaves][36];
  __shared__ double rd[kSgdSlots];
  __shared__ int s_done;
  __shared__ double saff[64];
  const int t = threadIdx.x, lane = lane_id(), wv = wave_id();
  constexpr int d_feat = 30;
  const double* bst = reinterpret_cast<const double*>(P.ws + kWsBackup);
  const float* bw = reinterpret_cast<const float*>(P.ws + kWsBackupW);
  if (P.aff != nullptr && t < 64) saff[t] = P.aff[t];
  const double* affl = P.aff != nullptr ? saff : nullptr;
  const float inv_s = FP8 ? 1.0f / x_scale : 1.0f;
  for (int e = t; e < kStateSize; e += kPersistThreads) sst[e] = bst[e];
  if (t < 32) {
    const float w = bw[t];
    wnew[t] = w;
    wsh[t] = t == kLabelCol ? 0.0f : w * ((FP8 && t < d_feat) ? inv_s : 1.0f);
  }
  if (t == 0) s_done = (int)P.ws[kWsBackupDone];
  __syncthreads();
  const float cw0 = class_w[0], cw1 = class_w[1];
  PickIn<4, 32> nopick;
  for (int st = P.s0; st < P.s1 && !s_done; ++st) {
    const PersistStep S(P, st);
    long long q = 0;
    for (int64_t w = wv; w < P.Gw; w += kPersistWaves) {
      persist_wave_sums<FP8, VIRT, 16, 32, 1>(X, row_end, x_scale, inv_s, cw0, cw1, wsh, sv, hole, w, P.Gw, true,
                                              S.rsub, S.phase, red, wv, lane, kNoTiles, false, nopick, false);
      __builtin_amdgcn_wave_barrier();  // this wave's row of red (LDS ops of one wave retire in order)
      if (lane < kSgdSlots) q += wave_sums_fixed<1>(&red[wv], affl, lane);
      __builtin_amdgcn_wave_barrier();
    }
    if (lane < kSgdSlots) qw[wv][lane] = q;
    __syncthreads();
    if (t < kSgdSlots) {
      unsigned long long s = 0;
      for (int w = 0; w < kPersistWaves; ++w) s += (unsigned long long)qw[w][t];
      rd[t] = t == 34 ? 0.0 : (double)(long long)s * (1.0 / kFixScale);
    }
    __syncthreads();
    sgd_apply(rd, sst, wnew, &s_done, affl, S.args(P), t, true);
    __syncthreads();
    if (t < 32) wsh[t] = t == kLabelCol ? 0.0f : wnew[t] * ((FP8 && t < d_feat) ? inv_s : 1.0f);
    __syncthreads();
  }
  if (t == 0) sst[kSgdFault] = 2.0;
  __syncthreads();
  for (int e = t; e < kStateSize; e += kPersistThreads) P.st[e] = sst[e];
  if (t < 32) P.w32[t] = wnew[t];
  if (t == 0) *P.done = s_done;
  if (P.export_host != nullptr) export_state_stamped(P.export_host, sst, P.export_seq, t);
}

}  // namespace

// Grid = resident capacity of the Hessian pass (blocks/CU from the occupancy query x CUs): a
// grid-stride stream must not launch a partial second round of blocks, which would double the
// tail (every block owns an equal share of rows).
// fmt: 0 bf16 rows, 1 fp8 rows (each format's own Hessian-kernel occupancy).
int logreg_pass_blocks(int fmt) {
  static int cached[2] = {0, 0};
  fmt = fmt ? 1 : 0;
  if (cached[fmt]) return cached[fmt];
  int dev = 0, cus = 256, per_cu = 3;
  if (hipGetDevice(&dev) == hipSuccess) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) == hipSuccess) cus = prop.multiProcessorCount;
    int occ = 0;
    hipError_t e = fmt ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, logreg_pass_fp8w_kernel<true>, kThreads, 0)
                       : hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, logreg_pass_kernel<true>, kThreads, 0);
    // at most 3 per CU (12 waves): the SGD minibatch partition is defined on this grid (ops/logreg
    // sgd_grid_blocks; the CPU mirror assumes 768 blocks on 256 CUs) and the persistent SGD launch
    // maps its 12-wave blocks onto it -- it must not move with the compiler's register allocation
    if (e == hipSuccess && occ > 0) per_cu = occ < 3 ? occ : 3;
  }
  int c = cus * per_cu;
  if (c < 64) c = 64;
  if (c > kPassBlocks * 2) c = kPassBlocks * 2;
  cached[fmt] = c;
  return c;
}

// The view a pass launches with: empty without virtual rows; validated otherwise (a virtual
// pass covers all rows: the picks are not split by row range).
static SmoteView checked_view(const SmoteView* sv, int64_t row_begin, int64_t row_end) {
  SmoteView v;
  if (sv == nullptr || sv->parents == nullptr) return v;
  v = *sv;
  if (v.nbr == nullptr || v.lam == nullptr || v.off == nullptr || v.cnt == nullptr || v.mq <= 0 || v.k <= 0 || v.n_real < 0 ||
      v.q_offset < 0 || (uint64_t)v.mq * (uint64_t)v.k >= (1ull << 31) || row_begin != 0 || row_end < v.n_real)
    throw std::runtime_error("logreg_pass: invalid virtual SMOTE view");
  return v;
}

// The skipped block must lie inside the stored rows (the kernel maps logical row r >= hole.at to
// physical row r + hole.len: a hole past the end would read beyond the buffer).
static void check_hole(const RowHole& h, int64_t row_begin, int64_t stored_end) {
  if (h.len < 0 || h.at < 0 || (h.len > 0 && row_begin + h.at + h.len > stored_end))
    throw std::runtime_error("logreg_pass: row hole outside the stored rows");
}

// A fused Newton iteration (NewtonFuse) needs its buffers, a gradient or Hessian pass (not the
// SGD curvature pass), the grid within the group workspace, and the pass's own done flag.
static NewtonFuse checked_fuse(const NewtonFuse* nf, int nblocks, bool fisher, const int* done) {
  if (nf == nullptr || nf->red == nullptr) return NewtonFuse{};
  if (fisher) throw std::runtime_error("logreg_pass: a fused Newton update follows a gradient or Hessian pass");
  if (nf->ws == nullptr || nf->st == nullptr || nf->w32 == nullptr || nf->done == nullptr || done != nf->done)
    throw std::runtime_error("logreg_pass: fused Newton update needs ws/state/w32 and the pass's done flag");
  if (nblocks < 1 || nblocks > kNewtonGroup * kNewtonMaxGroups)
    throw std::runtime_error("logreg_pass: grid too large for the fused Newton workspace");
  return *nf;
}

void launch_logreg_pass(const uint16_t* X, int64_t row_begin, int64_t row_end, const float* w,
                        const float* class_w, const int* done, int hessian, int row_sub,
                        float* partial, int nblocks, hipStream_t stream, const SmoteView* sv, int row_phase,
                        bool fisher, RowHole hole, const NewtonFuse* nf) {
  // hessian: 0 = gradient/loss only; h >= 1 = also the Hessian, from every h-th row tile.
  // row_sub >= 1, 0 <= row_phase < row_sub: visit the 1/row_sub tile subset row_phase (progressive
  // Newton: phase 0; SGD: minibatch row_phase of an epoch of row_sub minibatches).
  // sv (nullable): virtual SMOTE samples after the stored rows.  fisher (gradient-only passes):
  // also the curvature sum s p (1 - p) in slot 35.
  if (row_sub < 1) row_sub = 1;
  if (row_phase < 0 || row_phase >= row_sub) throw std::runtime_error("logreg_pass: row_phase out of range");
  if (fisher && hessian > 0) throw std::runtime_error("logreg_pass: the curvature sum is a gradient-pass output");
  const SmoteView v = checked_view(sv, row_begin, row_end);
  check_hole(hole, row_begin, v.parents != nullptr ? v.n_real : row_end);
  const bool virt = v.parents != nullptr;
  const int hs = hessian > 0 ? hessian : 1;
  const NewtonFuse nfa = checked_fuse(nf, nblocks, fisher, done);
#define FDX_LRP(H, V, F)                                                                                    \
  logreg_pass_kernel<H, V, F><<<nblocks, kThreads, 0, stream>>>(X, row_begin, row_end, w, class_w, done, hs, \
                                                                row_sub, row_phase, partial, v, hole, SgdFuse{}, nfa)
  if (hessian > 0) {
    if (virt) FDX_LRP(true, true, false);
    else FDX_LRP(true, false, false);
  } else if (fisher) {
    if (virt) FDX_LRP(false, true, true);
    else FDX_LRP(false, false, true);
  } else {
    if (virt) FDX_LRP(false, true, false);
    else FDX_LRP(false, false, false);
  }
#undef FDX_LRP
  check_launch("logreg_pass");
}

void launch_logreg_pass_fp8(const uint8_t* X, int64_t row_begin, int64_t row_end, const float* w,
                            const float* class_w, const int* done, int hessian, int row_sub,
                            float x_scale, float* partial, int nblocks, hipStream_t stream, const SmoteView* sv,
                            int row_phase, bool fisher, RowHole hole, const NewtonFuse* nf) {
  // fp8 rows store features * x_scale for columns < 30; the bias (col 30) and label (col 31)
  // are stored unscaled.  sv, row_phase, fisher: as launch_logreg_pass.
  if (row_sub < 1) row_sub = 1;
  if (row_phase < 0 || row_phase >= row_sub) throw std::runtime_error("logreg_pass_fp8: row_phase out of range");
  if (fisher && hessian > 0) throw std::runtime_error("logreg_pass_fp8: the curvature sum is a gradient-pass output");
  const SmoteView v = checked_view(sv, row_begin, row_end);
  check_hole(hole, row_begin, v.parents != nullptr ? v.n_real : row_end);
  const bool virt = v.parents != nullptr;
  const int hs = hessian > 0 ? hessian : 1;
  const NewtonFuse nfa = checked_fuse(nf, nblocks, fisher, done);
#define FDX_LRP8(H, V, F)                                                                                       \
  logreg_pass_fp8w_kernel<H, V, F><<<nblocks, kThreads, 0, stream>>>(X, row_begin, row_end, w, class_w, done,   \
                                                                     x_scale, 30, hs, row_sub, row_phase, partial, v, hole, \
                                                                     SgdFuse{}, nfa)
  if (hessian > 0) {
    if (virt) FDX_LRP8(true, true, false);
    else FDX_LRP8(true, false, false);
  } else if (fisher) {
    if (virt) FDX_LRP8(false, true, true);
    else FDX_LRP8(false, false, true);
  } else {
    if (virt) FDX_LRP8(false, true, false);
    else FDX_LRP8(false, false, false);
  }
#undef FDX_LRP8
  check_launch("logreg_pass_fp8");
}

// One SGD step in ONE launch (single process): minibatch `row_phase` of `row_sub` through the
// FISH pass whose blocks add their fixed-point sums into acc[36] and whose last block applies the
// update (sgd_fused_tail).  acc and ticket must be zero before the first step (they are left zero).
void launch_sgd_pass_fused(const void* X, int fp8, float x_scale, int64_t row_end, float* w32, const float* class_w,
                           int* done, int row_sub, int row_phase, int nblocks, const SmoteView* sv, RowHole hole,
                           unsigned long long* acc, unsigned int* ticket, double* state, const double* aff,
                           const SgdArgs& a, hipStream_t stream) {
  if (row_sub < 1 || row_phase < 0 || row_phase >= row_sub) throw std::runtime_error("sgd_pass_fused: bad phase");
  const SmoteView v = checked_view(sv, 0, row_end);
  check_hole(hole, 0, v.parents != nullptr ? v.n_real : row_end);
  SgdFuse fz;
  fz.acc = acc;
  fz.ticket = ticket;
  fz.st = state;
  fz.w32 = w32;
  fz.done = done;
  fz.aff = aff;
  fz.a = a;
  const bool virt = v.parents != nullptr;
  if (fp8) {
    const uint8_t* X8 = static_cast<const uint8_t*>(X);
    if (virt)
      logreg_pass_fp8w_kernel<false, true, true, true><<<nblocks, kThreads, 0, stream>>>(
          X8, 0, row_end, w32, class_w, done, x_scale, 30, 1, row_sub, row_phase, nullptr, v, hole, fz, NewtonFuse{});
    else
      logreg_pass_fp8w_kernel<false, false, true, true><<<nblocks, kThreads, 0, stream>>>(
          X8, 0, row_end, w32, class_w, done, x_scale, 30, 1, row_sub, row_phase, nullptr, v, hole, fz, NewtonFuse{});
  } else {
    if (virt)
      logreg_pass_kernel<false, true, true, true><<<nblocks, kThreads, 0, stream>>>(
          X, 0, row_end, w32, class_w, done, 1, row_sub, row_phase, nullptr, v, hole, fz, NewtonFuse{});
    else
      logreg_pass_kernel<false, false, true, true><<<nblocks, kThreads, 0, stream>>>(
          X, 0, row_end, w32, class_w, done, 1, row_sub, row_phase, nullptr, v, hole, fz, NewtonFuse{});
  }
  check_launch("sgd_pass_fused");
}

void launch_logreg_reduce(const float* partial, int nblocks, int ncols, double* out,
                          const int* done, hipStream_t stream) {
  // ncols = 64 for gradient-only passes (SGD), kLRPartStride when the Hessian was accumulated.
  logreg_reduce_kernel<<<(ncols + kRedCols - 1) / kRedCols, 1024, 0, stream>>>(partial, nblocks, ncols, out, done);
  check_launch("logreg_reduce");
}

void launch_newton_update(const double* red, double* state, float* w32, int* done, int d,
                          double C, double tol, int max_iter, int fit_intercept, int phase_start,
                          const double* aff, hipStream_t stream, int* done_host, int seq) {
  if (d + (fit_intercept ? 1 : 0) == 31)  // 30 features + intercept: the specialised stream
    newton_update_kernel<31><<<1, 64, 0, stream>>>(red, state, w32, done, d, C, tol, max_iter, fit_intercept,
                                                   phase_start, aff, nullptr, done_host, seq);
  else
    newton_update_kernel<0><<<1, 64, 0, stream>>>(red, state, w32, done, d, C, tol, max_iter, fit_intercept,
                                                  phase_start, aff, nullptr, done_host, seq);
  check_launch("newton_update");
}

void launch_newton_update_stamped(const double* red, double* state, float* w32, int* done, double C,
                                  const double* aff, unsigned long long* stamps, hipStream_t stream) {
  newton_update_kernel<31, true><<<1, 64, 0, stream>>>(red, state, w32, done, 30, C, 0.0, 1 << 30, 1, 0, aff,
                                                       stamps);
  check_launch("newton_update_stamped");
}

void launch_logreg_init(const LRInitArgs& a, double* state, float* w32, float* class_w, int* done,
                        const double* aff, hipStream_t stream, const double* w0_dev,
                        unsigned long long* persist_ws) {
  logreg_init_kernel<<<1, 64, 0, stream>>>(a, state, w32, class_w, done, aff, w0_dev, persist_ws);
  check_launch("logreg_init");
}

void launch_logreg_export(const double* state, double* host_dev, hipStream_t stream, long long seq) {
  logreg_export_kernel<<<1, 64, 0, stream>>>(state, host_dev, seq);
  check_launch("logreg_export");
}

void launch_logreg_fold(const double* state, const double* aff, float* w32, hipStream_t stream) {
  logreg_fold_kernel<<<1, 64, 0, stream>>>(state, aff, w32);
  check_launch("logreg_fold");
}

void launch_sgd_step(const float* partial, int nblocks, double* state, float* w32, int* done, const double* aff,
                     const SgdArgs& a, hipStream_t stream) {
  sgd_step_kernel<<<1, kSgdGroups * kSgdSlots, 0, stream>>>(partial, nblocks, state, w32, done, aff, a);
  check_launch("sgd_step");
}

void launch_sgd_update(const double* red, double* state, float* w32, int* done, const double* aff,
                       const SgdArgs& a, hipStream_t stream) {
  sgd_update_kernel<<<1, 64, 0, stream>>>(red, state, w32, done, aff, a);
  check_launch("sgd_update");
}

void launch_sgd_pass_sums(const void* X, int fp8, float x_scale, int64_t row_end, const float* w32,
                          const float* class_w, const int* done, int row_sub, int row_phase, int nblocks,
                          const SmoteView* sv, RowHole hole, unsigned long long* acc, unsigned int* ticket,
                          long long* sums, const double* aff, hipStream_t stream) {
  if (row_sub < 1 || row_phase < 0 || row_phase >= row_sub) throw std::runtime_error("sgd_pass_sums: bad phase");
  if (sums == nullptr || acc == nullptr || ticket == nullptr) throw std::runtime_error("sgd_pass_sums: null buffer");
  const SmoteView v = checked_view(sv, 0, row_end);
  check_hole(hole, 0, v.parents != nullptr ? v.n_real : row_end);
  SgdFuse fz;
  fz.acc = acc;
  fz.ticket = ticket;
  fz.aff = aff;
  fz.sums = sums;
  const bool virt = v.parents != nullptr;
  float* w = const_cast<float*>(w32);
  if (fp8) {
    const uint8_t* X8 = static_cast<const uint8_t*>(X);
    if (virt)
      logreg_pass_fp8w_kernel<false, true, true, true><<<nblocks, kThreads, 0, stream>>>(
          X8, 0, row_end, w, class_w, done, x_scale, 30, 1, row_sub, row_phase, nullptr, v, hole, fz, NewtonFuse{});
    else
      logreg_pass_fp8w_kernel<false, false, true, true><<<nblocks, kThreads, 0, stream>>>(
          X8, 0, row_end, w, class_w, done, x_scale, 30, 1, row_sub, row_phase, nullptr, v, hole, fz, NewtonFuse{});
  } else {
    if (virt)
      logreg_pass_kernel<false, true, true, true><<<nblocks, kThreads, 0, stream>>>(
          X, 0, row_end, w, class_w, done, 1, row_sub, row_phase, nullptr, v, hole, fz, NewtonFuse{});
    else
      logreg_pass_kernel<false, false, true, true><<<nblocks, kThreads, 0, stream>>>(
          X, 0, row_end, w, class_w, done, 1, row_sub, row_phase, nullptr, v, hole, fz, NewtonFuse{});
  }
  check_launch("sgd_pass_sums");
}

void launch_sgd_update_fixed(const long long* sums, double* state, float* w32, int* done, const double* aff,
                             const SgdArgs& a, hipStream_t stream) {
  sgd_update_fixed_kernel<<<1, 64, 0, stream>>>(sums, state, w32, done, aff, a);
  check_launch("sgd_update_fixed");
}

int sgd_full_blocks() {
  static int blocks = 0;
  if (blocks == 0) {
    int dev = 0, cus = 256;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess)
      cus = prop.multiProcessorCount;
    blocks = 2 * cus;
  }
  return blocks;
}

SgdConstants sgd_constants() {
  return {kSgdReplicas, kSgdGroups, kSgdLoads, kPersistWaves, kPersistReplicas, (double)kSynQ, (double)kSynQL};
}

int sgd_persist_blocks(int grid_blocks) {
  static int capacity = -1;
  if (capacity < 0) {
    int dev = 0, cus = 0, occ = 0;
    capacity = 0;
    if (hipGetDevice(&dev) == hipSuccess) {
      hipDeviceProp_t prop;
      if (hipGetDeviceProperties(&prop, dev) == hipSuccess) cus = prop.multiProcessorCount;
      int o1 = 0, o2 = 0;
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&o1, sgd_persist_kernel<false, true>, kPersistThreads, 0) ==
              hipSuccess &&
          hipOccupancyMaxActiveBlocksPerMultiprocessor(&o2, sgd_persist_kernel<true, true>, kPersistThreads, 0) ==
              hipSuccess)
        occ = o1 < o2 ? o1 : o2;
      // one block per CU whatever the query says (8 waves = 2 per SIMD: the 256-VGPR budget the
      // persistent step needs for its prefetched pick and tile across the barrier)
      capacity = cus * (occ >= 1 ? 1 : 0);
    }
  }
  if (grid_blocks < 1) return 0;
  const int blocks = (grid_blocks * kWaves + kPersistWaves - 1) / kPersistWaves;
  return blocks <= capacity ? blocks : 0;
}

int launch_sgd_persist(const void* X, int fp8, float x_scale, int64_t row_end, const float* class_w,
                       const SmoteView* sv, RowHole hole, const SgdPersistArgs& a, hipStream_t stream) {
  if (a.nb < 1 || a.epochs < 1 || a.epochs > kSgdMaxEpochs || a.s0 < 0 || a.s1 > a.estart[a.epochs] || a.s0 >= a.s1)
    throw std::runtime_error("sgd_persist: bad schedule");
  if (a.Gw < kWaves || a.Gw % kWaves != 0) throw std::runtime_error("sgd_persist: bad pass grid");
  if (a.ws == nullptr || a.st == nullptr || a.w32 == nullptr || a.done == nullptr)
    throw std::runtime_error("sgd_persist: null buffer");
  const int blocks = sgd_persist_blocks((int)(a.Gw / kWaves));
  if (blocks == 0) throw std::runtime_error("sgd_persist: the grid cannot be resident (launch per step)");
  const SmoteView v = checked_view(sv, 0, row_end);
  check_hole(hole, 0, v.parents != nullptr ? v.n_real : row_end);
  const bool virt = v.parents != nullptr;
  static const int depth = [] {  // lab switch: FDX_SGD_PERSIST_CFG=1 -> one stored tile in flight
    const char* e = std::getenv("FDX_SGD_PERSIST_CFG");
    return (e != nullptr && e[0] == '1') ? 1 : 2;
  }();
  // FDX_SGD_COOP=1: hipLaunchCooperativeKernel, which checks the grid against the occupancy query
  // at launch (hipErrorCooperativeLaunchTooLarge -> the caller runs per step).  Off by default: the
  // grid is already sized from that query (sgd_persist_blocks), so the check never refuses it, and
  // it cost ~30 us per fit at the bench shape (medians 1.097 vs 1.067 ms, profiles/r6_a); run-time
  // co-residency is covered by the bounded barrier + recovery launch either way.
  static const bool coop = [] {
    const char* e = std::getenv("FDX_SGD_COOP");
    return e != nullptr && e[0] == '1';
  }();
  const void* kern = nullptr;
  if (fp8) {  // fp8 tiles are half the bytes: its pass keeps two tiles in flight in the same registers
    kern = virt ? (const void*)sgd_persist_kernel<true, true, 16, 2, 2> : (const void*)sgd_persist_kernel<true, false, 16, 2, 2>;
  } else if (depth == 1) {
    kern = virt ? (const void*)sgd_persist_kernel<false, true, 16, 2, 1> : (const void*)sgd_persist_kernel<false, false, 16, 2, 1>;
  } else {
    kern = virt ? (const void*)sgd_persist_kernel<false, true, 16, 2, 2> : (const void*)sgd_persist_kernel<false, false, 16, 2, 2>;
  }
  // barrier shards, accumulator sets, fault word: zero; the initial state: backed up (stream-ordered)
  if (!a.prepped) {  // else logreg_init did it (stream-ordered in front of this launch)
    sgd_persist_prep_kernel<<<1, 256, 0, stream>>>(a.ws, a.st, a.w32, a.done);
    check_launch("sgd_persist_prep");
  }
  SgdPersistArgs pa = a;
  void* args[] = {(void*)&X, (void*)&row_end, (void*)&x_scale, (void*)&class_w, (void*)&v, (void*)&hole,
                  (void*)&pa};
  hipError_t e = coop ? hipLaunchCooperativeKernel(kern, dim3(blocks), dim3(kPersistThreads), args, 0, stream)
                      : hipLaunchKernel(kern, dim3(blocks), dim3(kPersistThreads), args, 0, stream);
  if (e != hipSuccess) {
    (void)hipGetLastError();  // clear the sticky launch error
    if (e == hipErrorCooperativeLaunchTooLarge) return 1;  // the prep kernel alone is harmless
    throw std::runtime_error(std::string("sgd_persist: launch failed: ") + hipGetErrorString(e));
  }
#define FDX_SGDR(F, V) sgd_recover_kernel<F, V><<<1, kPersistThreads, 0, stream>>>(X, row_end, x_scale, class_w, v, hole, a)
  if (fp8) {
    if (virt) FDX_SGDR(true, true);
    else FDX_SGDR(true, false);
  } else {
    if (virt) FDX_SGDR(false, true);
    else FDX_SGDR(false, false);
  }
#undef FDX_SGDR
  check_launch("sgd_recover");
  return 0;
}

}  // namespace fdx
