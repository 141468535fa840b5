// K8 knn_topk: the k-nearest-neighbour search inside SMOTE.
//
// Reference behaviour being replaced: imblearn SMOTE(k_neighbors=5) fits
// NearestNeighbors(n_neighbors=6) on the minority rows and drops each row's self match
// (train_model.py:65-66,91-92; preprocess.py:43-44).
//
// MI355X mapping: distance ranking via score(c, q) = q.c - 0.5 ||c||^2 (argmax score == argmin
// squared L2).  A workgroup owns 32 queries; each of its 4 waves sweeps every 4th 32-candidate
// tile.  The 32x32 score tile is one chain of 16 v_mfma_f32_32x32x2_f32 (exact fp32, a k-ordered
// fmaf chain, so rankings match an fp32 CPU oracle) with the accumulator pre-loaded with
// -0.5||c||^2.  Candidates sit on the MFMA row axis, so each lane holds 16 scores of ONE query
// (its column) and keeps a sorted top-k of (score, index) in registers with static indices
// (insertion network); the n x n distance matrix never exists.  Lane pairs (l, l^32) and then
// the 4 waves merge their lists through LDS.  Ties break on the smaller candidate index.
// K-index layout: MFMA step s, slot h <-> feature 16h + s, so each lane's operand for all 16
// steps is 16 CONTIGUOUS floats of one row (four 16 B loads).
#include <cmath>
#include <string>
#include <type_traits>

#include "common.h"
#include "launchers.h"
#include "scaler_finalize.h"

namespace fdx {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = 4;
constexpr int kMaxK = 8;
constexpr float kNegBig = -3.0e38f;
constexpr int kQFlush = 4;  // flush a wave's queues once any lane holds this many (2 / 8 / 12 measured
                             // slower at both bench shapes: profiles/r4_l/knn_flush*.json)

__device__ __forceinline__ bool better(float s, int i, float s2, int i2) {
  return s > s2 || (s == s2 && i < i2);
}

template <int K>
__device__ __forceinline__ void topk_insert(float (&bs)[K], int (&bi)[K], float s, int i) {
  if (!better(s, i, bs[K - 1], bi[K - 1])) return;
  bs[K - 1] = s;
  bi[K - 1] = i;
#pragma unroll
  for (int k = K - 1; k > 0; --k) {
    if (better(bs[k], bi[k], bs[k - 1], bi[k - 1])) {
      const float ts = bs[k]; bs[k] = bs[k - 1]; bs[k - 1] = ts;
      const int ti = bi[k]; bi[k] = bi[k - 1]; bi[k - 1] = ti;
    }
  }
}

// Rows for the score GEMM, padded to 32 floats.  Feature columns 0..29 are copied; the
// squared-norm term rides in column 30 so that one MFMA chain yields the whole score:
//   candidate: [c_0..c_29, -0.5 ||c||^2, 0]      (padding rows: [0.., -3e38, 0] -> never chosen)
//   query:     [q_0..q_29, 1, 0]                  (padding rows: zeros)
// so  score(c, q) = q.c - 0.5 ||c||^2  with no norm loads and a zero-initialised accumulator.
// role 2 (queries == candidates, the SMOTE self-search): one read of X writes both operands,
// candidates to `out` and queries to `outq`.  P != nullptr (candidate roles): the same launch also
// writes the bf16 SMOTE parents of smote_parents_kernel (smote.hip), bit for bit.
// chl / qhl / tmax (role 2 only, nullable): the hi/lo bf16 split of both operands in the same
// launch -- knn_split_kernel's role 2 (candidates, fragment order, per-tile norm bound) and role 1
// (queries, row order) on the values this thread just wrote, bitwise the same -- so the self-search
// of the bf16x3 engines needs no split launches.
// RAW (knn_prep_raw_kernel, the fused minority chain): X holds RAW padded minority rows (the
// scaler pass's xraw: features, zeros, bias, label) and every feature is standardized as it is
// read, z = (x - mean32) * inv32 -- scale_cast_kernel's subtract-then-multiply, so everything
// below sees the bits the gather + scale_cast launch used to write.  st: [4][32] floats in LDS,
// mean32 | inv32 | (float)(1 / aff[32 + c]) | (float)aff[c] (the parents' map, as computed below).
__device__ __forceinline__ void split_row(const float (&x)[32], uint32_t (&h)[16], uint32_t (&l)[16]);
template <bool RAW>
__device__ __forceinline__ float4 prep_load(const float4* __restrict__ p, int k, const float* st, int d) {
#pragma clang fp contract(off)
  float4 v = p[k];
  if constexpr (RAW) {
    const int c = 4 * k;
    if (c < d) v.x = (v.x - st[c]) * st[32 + c];
    if (c + 1 < d) v.y = (v.y - st[c + 1]) * st[32 + c + 1];
    if (c + 2 < d) v.z = (v.z - st[c + 2]) * st[32 + c + 2];
    if (c + 3 < d) v.w = (v.w - st[c + 3]) * st[32 + c + 3];
  }
  return v;
}
template <bool RAW>
__device__ __forceinline__ void knn_prep_body(const float* __restrict__ X, int m, int m_pad, int role,
                                              float* __restrict__ out, float* __restrict__ outq,
                                              const double* __restrict__ aff, uint16_t* __restrict__ P,
                                              uint4* __restrict__ chl, uint4* __restrict__ qhl,
                                              float* __restrict__ tmax, const float* st, int d) {
#pragma clang fp contract(off)  // the parents' mul-then-add must match smote_parents_kernel
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (chl != nullptr) {  // the fused split (blockDim 256, m_pad % 32 == 0: whole tiles per wave half)
    const bool ok = r < m_pad;
    float x[32];
    if (ok && r < m) {
      const float4* p = reinterpret_cast<const float4*>(X + (int64_t)r * kCols);
      float s = 0.0f;
#pragma unroll
      for (int k = 0; k < kCols / 4; ++k) {
        float4 v = prep_load<RAW>(p, k, st, d);
        if (k == kCols / 4 - 1) {
          s = fmaf(v.x, v.x, s); s = fmaf(v.y, v.y, s);
          v.z = 0.0f; v.w = 0.0f;
        } else {
          s = fmaf(v.x, v.x, s); s = fmaf(v.y, v.y, s); s = fmaf(v.z, v.z, s); s = fmaf(v.w, v.w, s);
        }
        x[4 * k] = v.x; x[4 * k + 1] = v.y; x[4 * k + 2] = v.z; x[4 * k + 3] = v.w;
      }
      x[30] = -0.5f * s;  // the candidate row; the query row has 1 there
    } else {
#pragma unroll
      for (int k = 0; k < 32; ++k) x[k] = 0.0f;
      x[30] = -3.0e38f;  // padding candidate
    }
    uint32_t h[16], l[16];
    split_row(x, h, l);
    if (ok) {
      const int64_t tb = (int64_t)(r >> 5) * 256 + (r & 31);
#pragma unroll
      for (int v = 0; v < 8; ++v) {
        const int k = v & 3;
        const uint4 c = v < 4 ? make_uint4(h[4 * k], h[4 * k + 1], h[4 * k + 2], h[4 * k + 3])
                              : make_uint4(l[4 * k], l[4 * k + 1], l[4 * k + 2], l[4 * k + 3]);
        chl[tb + (v >> 1) * 64 + (v & 1) * 32] = c;
      }
    }
    float n2 = (ok && x[30] > -1.0e37f) ? -2.0f * x[30] : 0.0f;
#pragma unroll
    for (int o = 1; o < 32; o <<= 1) n2 = fmaxf(n2, __shfl_xor(n2, o, kWave));
    if (ok && (r & 31) == 0) tmax[r >> 5] = sqrtf(n2) * 1.0001f;
    x[30] = (ok && r < m) ? 1.0f : 0.0f;  // the query row (padding queries: zeros)
    split_row(x, h, l);
    if (ok) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        qhl[(int64_t)r * 8 + k] = make_uint4(h[4 * k], h[4 * k + 1], h[4 * k + 2], h[4 * k + 3]);
        qhl[(int64_t)r * 8 + 4 + k] = make_uint4(l[4 * k], l[4 * k + 1], l[4 * k + 2], l[4 * k + 3]);
      }
    }
  }
  if (r >= m_pad) return;
  float4* o = reinterpret_cast<float4*>(out + (int64_t)r * kCols);
  float4* oq = role == 2 ? reinterpret_cast<float4*>(outq + (int64_t)r * kCols) : nullptr;
  if (r >= m) {
#pragma unroll
    for (int k = 0; k < kCols / 4; ++k) {
      o[k] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (oq) oq[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (role != 1) out[(int64_t)r * kCols + 30] = -3.0e38f;
    return;
  }
  const float4* p = reinterpret_cast<const float4*>(X + (int64_t)r * kCols);
  uint2* pp = P ? reinterpret_cast<uint2*>(P + (int64_t)r * kCols) : nullptr;
  float s = 0.0f;
#pragma unroll
  for (int k = 0; k < kCols / 4; ++k) {
    float4 v = prep_load<RAW>(p, k, st, d);
    if (pp) {
      float4 u = v;
      if constexpr (RAW) {
        const int c = 4 * k;
        u.x = u.x * st[64 + c] + st[96 + c];
        u.y = u.y * st[64 + c + 1] + st[96 + c + 1];
        if (c + 2 < kBiasCol) {
          u.z = u.z * st[64 + c + 2] + st[96 + c + 2];
          u.w = u.w * st[64 + c + 3] + st[96 + c + 3];
        }
      } else if (aff != nullptr) {
        const int c = 4 * k;
        u.x = u.x * (float)(1.0 / aff[32 + c]) + (float)aff[c];
        u.y = u.y * (float)(1.0 / aff[32 + c + 1]) + (float)aff[c + 1];
        if (c + 2 < kBiasCol) {
          u.z = u.z * (float)(1.0 / aff[32 + c + 2]) + (float)aff[c + 2];
          u.w = u.w * (float)(1.0 / aff[32 + c + 3]) + (float)aff[c + 3];
        }
      }
      pp[k] = make_uint2(pack_bf16x2(u.x, u.y), pack_bf16x2(u.z, u.w));
    }
    if (k == kCols / 4 - 1) {  // columns 28..31: keep 28, 29; 30 = norm term / 1, 31 = 0
      s = fmaf(v.x, v.x, s); s = fmaf(v.y, v.y, s);
      v.z = 0.0f; v.w = 0.0f;
    } else {
      s = fmaf(v.x, v.x, s); s = fmaf(v.y, v.y, s); s = fmaf(v.z, v.z, s); s = fmaf(v.w, v.w, s);
    }
    o[k] = v;
    if (oq) oq[k] = v;
  }
  out[(int64_t)r * kCols + 30] = role == 1 ? 1.0f : -0.5f * s;
  if (oq) outq[(int64_t)r * kCols + 30] = 1.0f;
}


__global__ void knn_prep_kernel(const float* __restrict__ X, int m, int m_pad, int role,
                                float* __restrict__ out, float* __restrict__ outq,
                                const double* __restrict__ aff, uint16_t* __restrict__ P,
                                uint4* __restrict__ chl = nullptr, uint4* __restrict__ qhl = nullptr,
                                float* __restrict__ tmax = nullptr) {
  knn_prep_body<false>(X, m, m_pad, role, out, outq, aff, P, chl, qhl, tmax, nullptr, 0);
}

// The self-search prep (role 2) of the fused minority chain: raw minority rows in, and the scaler
// finalize folded in.  st.nparts > 0: every block recomputes the statistics of its 32 columns
// from the level-1 partials (scaler_finalize_col: scaler_finalize_kernel's own arithmetic) in its
// prologue -- no finalize launch in front of the prep -- and block 0 writes the ScalerStats
// outputs.  st.nparts == 0: mean32 / inv32 / aff are read from a finalize launch's outputs.
__global__ __launch_bounds__(256) void knn_prep_raw_kernel(const float* __restrict__ X, int m, int m_pad,
                                                           float* __restrict__ out, float* __restrict__ outq,
                                                           uint16_t* __restrict__ P, uint4* __restrict__ chl,
                                                           uint4* __restrict__ qhl, float* __restrict__ tmax,
                                                           KnnRawStats st) {
  __shared__ float sst[4 * 32];
  if (threadIdx.x < 32) {
    const int c = threadIdx.x;
    float mu, inv;
    double ac, ai;
    if (st.nparts > 0) {
      const ScalerCol o = scaler_finalize_col(st.sums, st.n, st.pivot, st.d, st.colscale, st.nparts, c);
      mu = o.mean32; inv = o.inv32; ac = o.aff_c; ai = o.aff_inv;
      if (blockIdx.x == 0) {
        st.mean64[c] = o.mean; st.var64[c] = o.var; st.scale64[c] = o.scale;
        st.mean32[c] = mu; st.inv32[c] = inv;
        st.aff[c] = ac; st.aff[32 + c] = ai;
      }
    } else {
      mu = st.mean32[c]; inv = st.inv32[c]; ac = st.aff[c]; ai = st.aff[32 + c];
    }
    sst[c] = mu;
    sst[32 + c] = inv;
    sst[64 + c] = (float)(1.0 / ai);
    sst[96 + c] = (float)ac;
  }
  __syncthreads();
  knn_prep_body<true>(X, m, m_pad, 2, out, outq, nullptr, P, chl, qhl, tmax, sst, st.d);
}

// Q: [mq_pad][32] query rows and C: [mc_pad][32] candidate rows, both from knn_prep_kernel.
// Query row q is candidate row (self_offset + q) when self_offset >= 0 (self excluded).
//
// One wave per workgroup: blockIdx.x owns 32 queries, blockIdx.y a contiguous slice of the
// candidate tiles (the per-slice lists are merged by knn_merge_kernel).  Per 32-candidate tile:
//   * 16 v_mfma_f32_32x32x2_f32 give lane (j, h) the scores of query j against the 16 candidate
//     rows of half h (exact fp32: score = q.c - 0.5||c||^2, the norm term is column 30);
//   * every score >= the lane's threshold is appended to a per-lane LDS queue (a wave-uniform
//     branch per accumulator row skips the rows no lane passes);
//   * once any lane holds kQFlush entries the queues are inserted into the per-lane top-k
//     (exact score-then-index order, self/padding excluded) and the threshold becomes the k-th
//     best of the UNION of the two half-lists of the query (lanes j and j+32), which is a valid
//     filter for both halves and about twice as tight.
template <int K, int QF = kQFlush>
__global__ __launch_bounds__(kWave) void knn_topk_kernel(const float* __restrict__ Q, int mq,
                                                         const float* __restrict__ C,
                                                         int mc_pad, int mc,
                                                         int64_t self_offset,
                                                         int* __restrict__ out_idx,
                                                         float* __restrict__ out_score) {
  const int lane = threadIdx.x;
  const int h = lane >> 5, j = lane & 31;
  const int q0 = blockIdx.x * 32;
  const int qg = q0 + j;  // this lane's query (column of the score tile)
  const int64_t self_c = self_offset >= 0 ? self_offset + qg : -1;
  float bq[16];
  {
    const float4* p = reinterpret_cast<const float4*>(Q + (int64_t)qg * kCols + 16 * h);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float4 v = p[k];
      bq[4 * k] = v.x; bq[4 * k + 1] = v.y; bq[4 * k + 2] = v.z; bq[4 * k + 3] = v.w;
    }
  }
  float bs[K];
  int bi[K];
#pragma unroll
  for (int k = 0; k < K; ++k) { bs[k] = kNegBig; bi[k] = 0x7fffffff; }
  // padding queries (qg >= mq: zero rows, every score equal) never pass the filter: a lane that
  // appended every candidate made its wave the slowest of the grid (r5_r: 17k minority rows)
  float thr = qg < mq ? kNegBig : __builtin_inff();

  // Per-lane queue, [slot][lane]: same-slot stores of a wave hit 64 distinct banks (the last
  // slot is spare: kept from the select-and-store form's dump slot).
  constexpr int kCap = QF - 1 + 16 + 1;
  __shared__ int2 qent[kCap * kWave];  // (score bits, candidate index) at [slot * 64 + lane]
  int qn = 0;
  auto flush = [&]() {
    for (int e = 0; __any(e < qn); ++e) {
      if (e < qn) {
        const int2 v = qent[e * kWave + lane];
        const int ci = v.y;
        if (ci != self_c && ci < mc) topk_insert<K>(bs, bi, __int_as_float(v.x), ci);
      }
    }
    qn = 0;
    // k-th best of the union of this lane's and its partner's (other half) sorted lists
    float ps[K];
#pragma unroll
    for (int k = 0; k < K; ++k) ps[k] = __shfl_xor(bs[k], 32, kWave);
    int ia = 0, ib = 0;
    float kth = kNegBig;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      float a = kNegBig, b = kNegBig;
#pragma unroll
      for (int u = 0; u < K; ++u) { if (u == ia) a = bs[u]; if (u == ib) b = ps[u]; }
      const bool ta = a >= b;
      kth = ta ? a : b;
      ia += ta ? 1 : 0;
      ib += ta ? 0 : 1;
    }
    thr = qg < mq ? kth : __builtin_inff();
  };
  const int all_tiles = mc_pad / 32;
  const int t_lo = (int)(((int64_t)all_tiles * blockIdx.y) / gridDim.y);
  const int t_hi = (int)(((int64_t)all_tiles * (blockIdx.y + 1)) / gridDim.y);
  // register double buffer: the next tile's 16 floats per lane (L2-resident) are in flight
  // while the current tile's MFMA chain and filter run
  float4 cv[4];
  auto fetch = [&](int t, float4 (&a)[4]) {
    const float4* p = reinterpret_cast<const float4*>(C + (int64_t)(t * 32 + j) * kCols + 16 * h);
#pragma unroll
    for (int k = 0; k < 4; ++k) a[k] = p[k];
  };
  if (t_lo < t_hi) fetch(t_lo, cv);
  for (int t = t_lo; t < t_hi; ++t) {
    const int c0 = t * 32;
    float ac[16];
    f32x16_t acc = {};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      ac[4 * k] = cv[k].x; ac[4 * k + 1] = cv[k].y; ac[4 * k + 2] = cv[k].z; ac[4 * k + 3] = cv[k].w;
    }
    if (t + 1 < t_hi) fetch(t + 1, cv);
#pragma unroll
    for (int s = 0; s < 16; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ac[s], bq[s], acc, 0, 0, 0);
    // quad maxima first (rows 4q .. 4q+3 = 4 consecutive candidates), then the tile's
    float m4[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) m4[q] = fmaxf(fmaxf(acc[4 * q], acc[4 * q + 1]), fmaxf(acc[4 * q + 2], acc[4 * q + 3]));
    const float mx = fmaxf(fmaxf(m4[0], m4[1]), fmaxf(m4[2], m4[3]));
    if (!__any(mx >= thr)) continue;
    const int cbase = c0 + 4 * h;
    // Append: a wave-uniform branch per passing quad, then per accumulator row of it, skips the rows
    // no lane passes (usually all but one or two once the lists are full); the passing lanes store
    // under their exec mask.  The per-row select-and-store of every row (dump slot for non-passing
    // lanes) was ~110 of the ~135 VALU instructions per tile whenever ANY lane passed (r5_n PMC).
    int qe = qn * kWave + lane;                     // element of this lane's next free slot
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (!__any(m4[q] >= thr)) continue;
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int r = 4 * q + rr;
        const bool pass = acc[r] >= thr;
        if (__any(pass)) {
          if (pass) {
            qent[qe] = make_int2(__float_as_int(acc[r]), cbase + rr + 8 * q);
            qe += kWave;
          }
        }
      }
    }
    qn = (qe - lane) / kWave;
    if (__any(qn >= QF)) flush();
  }
  flush();
  // merge with the other half (same query, other candidate rows); lanes h == 0 write
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const float s2 = __shfl_xor(bs[k], 32, kWave);
    const int i2 = __shfl_xor(bi[k], 32, kWave);
    if (h == 0) topk_insert<K>(bs, bi, s2, i2);
  }
  if (h == 0 && qg < mq) {
    // gridDim.y > 1: partial list of this slice at [blockIdx.y][q][k] of the workspace
    const int64_t o = ((int64_t)blockIdx.y * mq + qg) * K;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      out_idx[o + k] = bi[k];
      if (out_score) out_score[o + k] = bs[k];
    }
  }
}

// ---- bf16x3: the approximate score of the collect engines --------------------------------------
// The fp32 MFMA chain above is 16 x v_mfma_f32_32x32x2_f32 = 1024 SIMD cycles per 32x32 tile
// (profiles/r1_s31: 206 us of the bench step at 13.6k minority rows).  The engines below split
// every prepped row x = hi + lo (two bf16 rows) and score a tile as hi.hi + hi.lo + lo.hi on
// v_mfma_f32_32x32x16_bf16 (6 MFMAs = 192 cycles), |approx - exact| <= 2^-16 sum|q_f c_f| (the
// omitted lo.lo term, the split residuals and fp32 accumulation).  That approximate score only
// FILTERS, with a margin that covers the error; what passes is re-scored exactly in fp32.

__device__ __forceinline__ void split_row(const float (&x)[32], uint32_t (&h)[16], uint32_t (&l)[16]) {
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const float a = x[2 * k], b = x[2 * k + 1];
    const uint32_t ph = pack_bf16x2(a, b);
    h[k] = ph;
    l[k] = pack_bf16x2(a - bf16lo(ph), b - bf16hi(ph));
  }
}

// hi/lo bf16 split of prepped rows: hl[r] = 8 x uint4 (hi cols 0..31, then lo cols 0..31);
// role 0 (candidates) also writes tmax[r / 32] = max feature norm over the 32-row tile; role 2 = role 0
// with hl in the fragment order the collect kernels stream (below); role 1 (queries): rows only.
__global__ __launch_bounds__(256) void knn_split_kernel(const float* __restrict__ Xp, int m_pad, int role,
                                                        uint4* __restrict__ hl, float* __restrict__ tmax) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  const bool ok = r < m_pad;
  float x[32];
  const float4* p = reinterpret_cast<const float4*>(Xp + (int64_t)(ok ? r : 0) * kCols);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float4 v = p[k];
    x[4 * k] = v.x; x[4 * k + 1] = v.y; x[4 * k + 2] = v.z; x[4 * k + 3] = v.w;
  }
  uint32_t h[16], l[16];
  split_row(x, h, l);
  if (ok && role == 2) {
    // fragment order: tile r / 32 as [u 0..3][lane 64] uint4, lane (half hh, row j) of load u
    // holding chunk 2u + hh of row j (chunks 0..3 hi, 4..7 lo) -- each of the tile loop's four
    // loads is one contiguous 1 KiB per wave instead of 16 B pieces of 32 rows
    const int64_t tb = (int64_t)(r >> 5) * 256 + (r & 31);
#pragma unroll
    for (int v = 0; v < 8; ++v) {
      const int k = v & 3;
      const uint4 c = v < 4 ? make_uint4(h[4 * k], h[4 * k + 1], h[4 * k + 2], h[4 * k + 3])
                            : make_uint4(l[4 * k], l[4 * k + 1], l[4 * k + 2], l[4 * k + 3]);
      hl[tb + (v >> 1) * 64 + (v & 1) * 32] = c;
    }
  } else if (ok) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      hl[(int64_t)r * 8 + k] = make_uint4(h[4 * k], h[4 * k + 1], h[4 * k + 2], h[4 * k + 3]);
      hl[(int64_t)r * 8 + 4 + k] = make_uint4(l[4 * k], l[4 * k + 1], l[4 * k + 2], l[4 * k + 3]);
    }
  }
  if (role == 0 || role == 2) {
    // candidate rows carry -0.5 ||c||^2 in column 30 (padding rows: -3e38 -> norm 0)
    float n2 = (ok && x[30] > -1.0e37f) ? -2.0f * x[30] : 0.0f;
#pragma unroll
    for (int o = 1; o < 32; o <<= 1) n2 = fmaxf(n2, __shfl_xor(n2, o, kWave));
    if (ok && (r & 31) == 0) tmax[r >> 5] = sqrtf(n2) * 1.0001f;
  }
}

// ---- bf16x3 collect + exact re-rank (two phases) ---------------------------------------------
// The fp32 engine runs the top-k on the critical path of every tile: its chain costs 1024 MFMA
// cycles per 32x32 tile plus the filter's VALU (serial per wave: ~200 us at 13.6k minority rows,
// profiles/r4_g).  Here phase 1 (knn_collect_kernel) never touches fp32 candidate rows: per tile it
// runs the 6 bf16 MFMAs of the bf16x3 score and a max test, and a passing candidate only APPENDS its
// index to a per-lane global list.  The running threshold is the k-th best LOWER bound approx - m of
// the union of the query's two half-lists, where m = 2^-14 (||q|| tmax + 0.5 tmax^2) >= 4x the bf16x3
// error bound 2^-16 sum|q_f c_f| (above; fp32 accumulation of the 96 products and the exact fmaf
// chain add < 0.6 x 2^-16 more); a candidate is appended when its UPPER bound approx + m reaches it.
// Since k distinct candidates have exact >= lower bound >= thr, the exact k-th best s_k >= thr
// at every moment, so every candidate with exact >= s_k (upper bound >= s_k >= thr) is on a list.
// Phase 2 (knn_rerank_kernel, 8 lanes per query) re-scores the listed candidates exactly (one
// k-ordered fp32 fmaf chain over columns 0..31) and keeps the top-k (ties -> smaller index):
// the exact fp32 ranking.  A full lane list is compacted in place first: an entry (lower bound
// lb) whose upper bound -- at most lb + 2 m_max, m_max the largest margin the lane has used -- is
// below the current threshold cannot reach s_k and is dropped.  A list still full after that
// sends its query to a brute-force exact scan in phase 2 (correct, slow: r5_q measured the config-5
// shard, 17k x 17k, at 0.67 ms before the compaction).
constexpr int kListCap = 64;
constexpr int kSeedTiles = 2;             // seed candidates per slice > 0: 64
constexpr float kMarginScale = 0x1p-14f;  // m = 2^-14 (||q|| tmax + 0.5 tmax^2): >= 4x the error bound

template <int K>
__global__ __launch_bounds__(kWave) void knn_collect_kernel(const float* __restrict__ Q, const uint4* __restrict__ Qhl,
                                                            const uint4* __restrict__ Chl,
                                                            const float* __restrict__ tmax, int mq, int mc_pad, int mc,
                                                            int64_t self_offset, int2* __restrict__ lists,
                                                            int* __restrict__ counts) {
  const int lane = threadIdx.x;
  const int h = lane >> 5, j = lane & 31;
  const int qg = blockIdx.x * 32 + j;
  const int64_t self_c = self_offset >= 0 ? self_offset + qg : -1;
  float qn;
  {  // ||q|| over the 30 feature columns: half h sums columns 16h .. 16h + 15
    const float4* p = reinterpret_cast<const float4*>(Q + (int64_t)qg * kCols + 16 * h);
    float s2 = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float4 v = p[k];
      s2 = fmaf(v.x, v.x, s2);
      s2 = fmaf(v.y, v.y, s2);
      if (h == 0 || k < 3) {  // columns 30, 31 (query 1 / 0) are not features
        s2 = fmaf(v.z, v.z, s2);
        s2 = fmaf(v.w, v.w, s2);
      }
    }
    s2 += __shfl_xor(s2, 32, kWave);
    qn = sqrtf(s2) * 1.0001f;
  }
  const uint4* qr = Qhl + (int64_t)qg * 8;
  const bf16x8_t qh0 = __builtin_bit_cast(bf16x8_t, qr[h]), qh1 = __builtin_bit_cast(bf16x8_t, qr[2 + h]);
  const bf16x8_t ql0 = __builtin_bit_cast(bf16x8_t, qr[4 + h]), ql1 = __builtin_bit_cast(bf16x8_t, qr[6 + h]);
  float bs[K];
  int bi[K];
#pragma unroll
  for (int k = 0; k < K; ++k) { bs[k] = kNegBig; bi[k] = 0x7fffffff; }
  // padding queries (qg >= mq: zero rows, every score equal) never pass the filter: a lane that
  // appended every candidate made its wave the slowest of the grid (r5_r: 17k minority rows)
  float thr = qg < mq ? kNegBig : __builtin_inff();
  float mgmax = 0.0f;  // the largest margin this lane has used (list compaction bound)
  constexpr int kCap = kQFlush - 1 + 16 + 1;
  __shared__ int2 qent[kCap * kWave];  // (lower-bound bits, candidate index) at [slot * 64 + lane]
  int qc = 0, cnt = 0;
  const int64_t lbase = (int64_t)(blockIdx.y * gridDim.x + blockIdx.x) * kListCap * kWave + lane;
  auto union_thr = [&]() {  // k-th best lower bound of the union of this lane's and its partner's lists
    float ps[K];
#pragma unroll
    for (int k = 0; k < K; ++k) ps[k] = __shfl_xor(bs[k], 32, kWave);
    int ia = 0, ib = 0;
    float kth = kNegBig;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      float a = kNegBig, b = kNegBig;
#pragma unroll
      for (int u = 0; u < K; ++u) { if (u == ia) a = bs[u]; if (u == ib) b = ps[u]; }
      const bool ta = a >= b;
      kth = ta ? a : b;
      ia += ta ? 1 : 0;
      ib += ta ? 0 : 1;
    }
    thr = qg < mq ? kth : __builtin_inff();
  };
  auto flush = [&]() {
    for (int e = 0; __any(e < qc); ++e) {
      if (e < qc) {
        const int2 v = qent[e * kWave + lane];
        const int ci = v.y;
        if (ci != self_c && ci < mc) {
          if (cnt == kListCap) {  // full: drop the entries that can no longer reach s_k (rare path)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this lane's list stores have landed
            int w = 0;
            for (int e2 = 0; e2 < kListCap; ++e2) {
              const int2 o = lists[lbase + (int64_t)e2 * kWave];
              if (__int_as_float(o.x) + 2.0f * mgmax >= thr) lists[lbase + (int64_t)(w++) * kWave] = o;
            }
            cnt = w;
          }
          if (cnt < kListCap) lists[lbase + (int64_t)cnt * kWave] = v;
          ++cnt;
          topk_insert<K>(bs, bi, __int_as_float(v.x), ci);
        }
      }
    }
    qc = 0;
    union_thr();
  };
  const int all_tiles = mc_pad / 32;
  const int t_lo = (int)(((int64_t)all_tiles * blockIdx.y) / gridDim.y);
  const int t_hi = (int)(((int64_t)all_tiles * (blockIdx.y + 1)) / gridDim.y);
  // Chl in the fragment order of knn_split role 2: each of a tile's four loads is one contiguous
  // 1 KiB per wave (lane (h, j) of load u holds chunk 2u + h of row j -- the same registers as the
  // row layout's p[h], p[2 + h], p[4 + h], p[6 + h]) instead of 32 rows' 16-byte pieces
  auto fetch = [&](int t, uint4 (&a)[4], float& tmv) {
    const uint4* p = Chl + (int64_t)t * 256 + lane;
    a[0] = p[0]; a[1] = p[64]; a[2] = p[128]; a[3] = p[192];
    tmv = tmax[t];
  };
  auto approx = [&](const uint4 (&c)[4]) -> f32x16_t {
    const bf16x8_t ch0 = __builtin_bit_cast(bf16x8_t, c[0]), ch1 = __builtin_bit_cast(bf16x8_t, c[1]);
    const bf16x8_t cl0 = __builtin_bit_cast(bf16x8_t, c[2]), cl1 = __builtin_bit_cast(bf16x8_t, c[3]);
    f32x16_t acc = {};
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(cl0, qh0, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(cl1, qh1, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ch0, ql0, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ch1, ql1, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ch0, qh0, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ch1, qh1, acc, 0, 0, 0);
    return acc;
  };
  // Seed (slices > 0): the lower bounds of the first kSeedTiles tiles of the candidate set -- slice
  // 0's, so distinct from this slice's candidates -- fill the top-k before the slice starts.  They
  // are never appended (slice 0 lists them), but the threshold they give is valid (k distinct
  // candidates with exact >= lower bound >= thr) and spares every slice its fill phase: with
  // thr = -inf the first tile appends all 16 candidates of every lane (r5_j: 62 list entries per
  // query and slice at 13.6k x 13.6k, 4 slices, a 124 us re-rank).
  if (blockIdx.y > 0) {
    const int ns0 = (int)((int64_t)all_tiles / gridDim.y);  // slice 0's tile count
    const int nseed = ns0 < kSeedTiles ? ns0 : kSeedTiles;
    for (int t = 0; t < nseed; ++t) {
      uint4 c[4];
      float tm;
      fetch(t, c, tm);
      const f32x16_t acc = approx(c);
      const float mg = kMarginScale * fmaf(qn, tm, 0.5f * tm * tm);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int ci = t * 32 + 4 * h + (r & 3) + 8 * (r >> 2);
        if (ci != self_c && ci < mc) topk_insert<K>(bs, bi, acc[r] - mg, ci);
      }
    }
    union_thr();
  }
  // The filter of one scored tile (knn_topk_kernel's quad-then-row uniform-skip append).
  auto filter = [&](int t, const f32x16_t& acc, float tm) {
    const float mg = kMarginScale * fmaf(qn, tm, 0.5f * tm * tm);
    mgmax = fmaxf(mgmax, mg);
    const float cut = thr - mg;  // upper bound approx + mg >= thr
    float m4[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) m4[q] = fmaxf(fmaxf(acc[4 * q], acc[4 * q + 1]), fmaxf(acc[4 * q + 2], acc[4 * q + 3]));
    const float mx = fmaxf(fmaxf(m4[0], m4[1]), fmaxf(m4[2], m4[3]));
    if (!__any(mx >= cut)) return;
    const int cbase = t * 32 + 4 * h;
    int qe = qc * kWave + lane;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (!__any(m4[q] >= cut)) continue;
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int r = 4 * q + rr;
        const bool pass = acc[r] >= cut;
        if (__any(pass)) {
          if (pass) {
            qent[qe] = make_int2(__float_as_int(acc[r] - mg), cbase + rr + 8 * q);
            qe += kWave;
          }
        }
      }
    }
    qc = (qe - lane) / kWave;
    if (__any(qc >= kQFlush)) flush();
  };
  // Tiles in PAIRS: the two tiles' 6-MFMA chains are interleaved (independent accumulators), so one
  // chain's result latency is covered by the other's issue -- at ~1.7 waves per SIMD a lone chain's
  // latency was exposed on every tile.  The next pair's loads are in flight meanwhile.
  uint4 ca[4], cb[4];
  float tma = 0.0f, tmb = 0.0f;
  if (t_lo < t_hi) fetch(t_lo, ca, tma);
  if (t_lo + 1 < t_hi) fetch(t_lo + 1, cb, tmb);
  for (int t = t_lo; t < t_hi; t += 2) {
    const bool two = t + 1 < t_hi;  // wave-uniform
    f32x16_t acc0 = {}, acc1 = {};
    {
      const bf16x8_t ah0 = __builtin_bit_cast(bf16x8_t, ca[0]), ah1 = __builtin_bit_cast(bf16x8_t, ca[1]);
      const bf16x8_t al0 = __builtin_bit_cast(bf16x8_t, ca[2]), al1 = __builtin_bit_cast(bf16x8_t, ca[3]);
      const bf16x8_t bh0 = __builtin_bit_cast(bf16x8_t, cb[0]), bh1 = __builtin_bit_cast(bf16x8_t, cb[1]);
      const bf16x8_t bl0 = __builtin_bit_cast(bf16x8_t, cb[2]), bl1 = __builtin_bit_cast(bf16x8_t, cb[3]);
      // approx()'s order per tile (bitwise the same sums), the two chains alternating
      acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al0, qh0, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bl0, qh0, acc1, 0, 0, 0);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al1, qh1, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bl1, qh1, acc1, 0, 0, 0);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah0, ql0, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bh0, ql0, acc1, 0, 0, 0);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah1, ql1, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bh1, ql1, acc1, 0, 0, 0);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah0, qh0, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bh0, qh0, acc1, 0, 0, 0);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah1, qh1, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bh1, qh1, acc1, 0, 0, 0);
    }
    const float ta = tma, tb = tmb;
    if (t + 2 < t_hi) fetch(t + 2, ca, tma);  // the next pair
    if (t + 3 < t_hi) fetch(t + 3, cb, tmb);
    filter(t, acc0, ta);
    if (two) filter(t + 1, acc1, tb);
  }
  flush();
  // counts holds three planes of gridDim.x * gridDim.y * 64 ints: the list length, then this lane's
  // final threshold (the union's k-th best lower bound) and largest margin -- the re-rank skips
  // every entry whose upper bound cannot reach the best of the slices' final thresholds
  const int64_t ci0 = (int64_t)(blockIdx.y * gridDim.x + blockIdx.x) * kWave + lane;
  const int64_t plane = (int64_t)gridDim.x * gridDim.y * kWave;
  counts[ci0] = cnt;
  counts[plane + ci0] = __float_as_int(thr);
  counts[2 * plane + ci0] = __float_as_int(mgmax);
}

// Phase 2: 8 lanes per query (lane l takes every 8th listed candidate), exact re-score, per-lane
// top-k, then a 3-round butterfly merge of the 8 sorted lists (knn_merge_kernel's merge).
template <int K>
__global__ __launch_bounds__(256) void knn_rerank_kernel(const float* __restrict__ Q, const float* __restrict__ C,
                                                         int mq, int mc, int qblocks, int nsplit, int64_t self_offset,
                                                         const int2* __restrict__ lists,
                                                         const int* __restrict__ counts, int* __restrict__ out_idx,
                                                         float* __restrict__ out_score) {
  const int gl = blockIdx.x * 256 + threadIdx.x;
  const int q = gl >> 3, l = gl & 7;
  const bool live = q < mq;
  const int qq = live ? q : 0;
  const int blk = qq >> 5, j = qq & 31;
  const int64_t self_c = self_offset >= 0 ? self_offset + qq : -1;
  float qv[kCols];
  {
    const float4* p = reinterpret_cast<const float4*>(Q + (int64_t)qq * kCols);
#pragma unroll
    for (int k = 0; k < kCols / 4; ++k) {
      const float4 v = p[k];
      qv[4 * k] = v.x; qv[4 * k + 1] = v.y; qv[4 * k + 2] = v.z; qv[4 * k + 3] = v.w;
    }
  }
  auto exact = [&](int ci) -> float {  // the exact score: one fmaf chain, columns 0..31 in order
    const float4* c = reinterpret_cast<const float4*>(C + (int64_t)ci * kCols);
    float acc = 0.0f;
#pragma unroll
    for (int k = 0; k < kCols / 4; ++k) {
      const float4 v = c[k];
      acc = fmaf(qv[4 * k], v.x, acc);
      acc = fmaf(qv[4 * k + 1], v.y, acc);
      acc = fmaf(qv[4 * k + 2], v.z, acc);
      acc = fmaf(qv[4 * k + 3], v.w, acc);
    }
    return acc;
  };
  float bs[K];
  int bi[K];
#pragma unroll
  for (int k = 0; k < K; ++k) { bs[k] = kNegBig; bi[k] = 0x7fffffff; }
  if (live) {
    bool over = false;
    const int64_t plane = (int64_t)nsplit * qblocks * kWave;
    float T = kNegBig;  // the best slice threshold: a lower bound of the exact k-th best s_k
    for (int s = 0; s < nsplit; ++s) {
#pragma unroll
      for (int h = 0; h < 2; ++h) over |= counts[((int64_t)s * qblocks + blk) * kWave + j + 32 * h] > kListCap;
      T = fmaxf(T, __int_as_float(counts[plane + ((int64_t)s * qblocks + blk) * kWave + j]));
    }
    if (!over) {
      for (int s = 0; s < nsplit; ++s) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int64_t cb = ((int64_t)s * qblocks + blk) * kWave + j + 32 * h;
          const int n = counts[cb];
          // an entry's upper bound is at most lb + 2 m_max; below T <= s_k it cannot be in the top-k
          // (not even on a tie), so its fp32 row is never gathered
          const float skip = T - 2.0f * __int_as_float(counts[2 * plane + cb]);
          const int2* li = lists + ((int64_t)s * qblocks + blk) * kListCap * kWave + j + 32 * h;
          for (int e = l; e < n; e += 8) {
            const int2 v = li[(int64_t)e * kWave];
            if (__int_as_float(v.x) < skip) continue;
            topk_insert<K>(bs, bi, exact(v.y), v.y);
          }
        }
      }
    } else {  // a list overflowed: exact scan of every candidate
      for (int ci = l; ci < mc; ci += 8)
        if (ci != self_c) topk_insert<K>(bs, bi, exact(ci), ci);
    }
  }
#pragma unroll
  for (int off = 1; off < 8; off <<= 1) {
    float os[K];
    int oi[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      os[k] = __shfl_xor(bs[k], off, kWave);
      oi[k] = __shfl_xor(bi[k], off, kWave);
    }
    float ns[K];
    int ni[K];
    int ia = 0, ib = 0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      float a = kNegBig, b = kNegBig;
      int ai = 0x7fffffff, bj = 0x7fffffff;
#pragma unroll
      for (int u = 0; u < K; ++u) {
        if (u == ia) { a = bs[u]; ai = bi[u]; }
        if (u == ib) { b = os[u]; bj = oi[u]; }
      }
      const bool ta = !better(b, bj, a, ai);
      ns[k] = ta ? a : b;
      ni[k] = ta ? ai : bj;
      ia += ta ? 1 : 0;
      ib += ta ? 0 : 1;
    }
#pragma unroll
    for (int k = 0; k < K; ++k) { bs[k] = ns[k]; bi[k] = ni[k]; }
  }
  if (live && l == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      out_idx[(int64_t)q * K + k] = bi[k];
      if (out_score) out_score[(int64_t)q * K + k] = bs[k];
    }
  }
}

// ---- bf16x3 two-pass collect: a threshold that is final from the first tile -------------------
// knn_collect_kernel's per-tile cost is its RUNNING threshold (any-tests, LDS queue, flush with a
// top-k insert per entry, seeds, compaction), and a streamed top-k appends ~k ln(n / k) candidates
// per query whatever the tuning.  Here the 6-MFMA score runs twice and nothing else does:
//   pass 1 (knn_groupmax_kernel): a lane pair (j, j + 32) holds a query's scores of the candidates
//     c mod 32 = 4h + (r & 3) + 8 (r >> 2) in accumulator register r of half h -- 32 groups -- and
//     keeps the running maximum of each (self masked, padding scores -3e38), plus the largest margin;
//   knn_threshold_kernel: per query, v_K = the K-th largest of the 32 group maxima (elementwise max
//     over the slices first), M = the largest margin of any slice, T = v_K - M.  The K groups' best
//     candidates are K DISTINCT candidates with exact >= approx - m >= v_K - M = T, so the exact
//     k-th best s_k >= T: knn_collect_kernel's argument with a threshold that never moves;
//   pass 2 (knn_filter_kernel): appends (approx - m, index) when approx + m >= T.  Every candidate
//     with exact >= s_k has approx + m >= exact >= T, so it is listed, in knn_collect_kernel's
//     lists / counts layout with T in the threshold plane and M in the margin plane (a listed entry
//     has lb = approx - m >= T - 2 m >= T - 2 M: knn_rerank_kernel's skip would keep it).
//     A lane list past kListCap is counted, not stored: the re-rank's exact scan answers the query;
//   knn_rerank_sparse_kernel: knn_rerank_kernel's exact re-score and ordering, 32 lanes per query.
// gmax: [nsplit][qblocks][17][64] floats, rows 0..15 the lane's group maxima, row 16 its margin.
__device__ __forceinline__ float knn_query_norm(const float* __restrict__ Q, int qg, int h) {
  // 1.0001 ||q|| over the 30 feature columns (knn_collect_kernel's: half h sums columns 16h .. 16h + 15)
  const float4* p = reinterpret_cast<const float4*>(Q + (int64_t)qg * kCols + 16 * h);
  float s2 = 0.0f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float4 v = p[k];
    s2 = fmaf(v.x, v.x, s2);
    s2 = fmaf(v.y, v.y, s2);
    if (h == 0 || k < 3) {  // columns 30, 31 (query 1 / 0) are not features
      s2 = fmaf(v.z, v.z, s2);
      s2 = fmaf(v.w, v.w, s2);
    }
  }
  s2 += __shfl_xor(s2, 32, kWave);
  return sqrtf(s2) * 1.0001f;
}

// max(a, b) of two non-NaN floats as one v_med3_f32(a, b, +inf): fmaxf costs a canonicalizing
// v_max_f32 x, x on every operand the compiler cannot prove quiet -- an MFMA result, a loop-carried
// maximum -- which tripled the passes' VALU count per tile
__device__ __forceinline__ float knn_max(float a, float b) { return __builtin_amdgcn_fmed3f(a, b, __builtin_inff()); }

// The tile loop both passes share.  A wave scores every candidate tile against TWO query blocks
// (2 x and 2 x + 1): the tile's 4 KiB of operands, fetched once, feed both 6-MFMA chains, which are
// interleaved as knn_collect_kernel interleaves two tiles' (independent accumulators; per block
// bitwise its sums).  That halves the bytes a pass pulls through L2 (740 MB at 13.6k x 13.6k with one
// block per wave); on its own it measured neutral, the unconditional prefetch and knn_max above
// gave the passes their last 10 % (profiles/pr4_knn_twopass).  Two tiles are in flight;
// use(t, acc of block 0, acc of block 1, tmax[t]).
struct KnnQFrag {
  bf16x8_t h0, h1, l0, l1;
};

__device__ __forceinline__ KnnQFrag knn_load_qfrag(const uint4* __restrict__ Qhl, int qg, int h) {
  const uint4* qr = Qhl + (int64_t)qg * 8;
  return {__builtin_bit_cast(bf16x8_t, qr[h]), __builtin_bit_cast(bf16x8_t, qr[2 + h]),
          __builtin_bit_cast(bf16x8_t, qr[4 + h]), __builtin_bit_cast(bf16x8_t, qr[6 + h])};
}

template <typename F>
__device__ __forceinline__ void knn_stream_tiles(const KnnQFrag& qa, const KnnQFrag& qb,
                                                 const uint4* __restrict__ Chl, const float* __restrict__ tmax,
                                                 int lane, int t_lo, int t_hi, F&& use) {
  auto fetch = [&](int t, uint4 (&a)[4], float& tmv) {
    const uint4* p = Chl + (int64_t)t * 256 + lane;
    a[0] = p[0]; a[1] = p[64]; a[2] = p[128]; a[3] = p[192];
    tmv = tmax[t];
  };
  auto score = [&](const uint4 (&c)[4], f32x16_t& acc0, f32x16_t& acc1) {
    const bf16x8_t ch0 = __builtin_bit_cast(bf16x8_t, c[0]), ch1 = __builtin_bit_cast(bf16x8_t, c[1]);
    const bf16x8_t cl0 = __builtin_bit_cast(bf16x8_t, c[2]), cl1 = __builtin_bit_cast(bf16x8_t, c[3]);
    acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(cl0, qa.h0, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(cl0, qb.h0, acc1, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(cl1, qa.h1, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(cl1, qb.h1, acc1, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ch0, qa.l0, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ch0, qb.l0, acc1, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ch1, qa.l1, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ch1, qb.l1, acc1, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ch0, qa.h0, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ch0, qb.h0, acc1, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ch1, qa.h1, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ch1, qb.h1, acc1, 0, 0, 0);
  };
  if (t_lo >= t_hi) return;  // a slice with no tile
  // Every prefetch is issued unconditionally, past the end clamped to the slice's last tile (fetched
  // again, never used): with the loads behind a branch the compiler cannot count them and waits for
  // ALL outstanding loads, the just-issued prefetch included, in front of every tile.
  const int last = t_hi - 1;
  uint4 ca[4], cb[4];
  float tma, tmb;
  fetch(t_lo, ca, tma);
  fetch(t_lo + 1 < t_hi ? t_lo + 1 : last, cb, tmb);
  for (int t = t_lo; t < t_hi; t += 2) {
    {
      f32x16_t acc0 = {}, acc1 = {};
      score(ca, acc0, acc1);
      const float tm = tma;
      fetch(t + 2 < t_hi ? t + 2 : last, ca, tma);
      use(t, acc0, acc1, tm);
    }
    {
      f32x16_t acc0 = {}, acc1 = {};
      score(cb, acc0, acc1);
      const float tm = tmb;
      fetch(t + 3 < t_hi ? t + 3 : last, cb, tmb);
      if (t + 1 < t_hi) use(t + 1, acc0, acc1, tm);  // wave-uniform
    }
  }
}

// grid ((qblocks + 1) / 2, nsplit); an odd last block is scored twice and written once
__global__ __launch_bounds__(kWave) void knn_groupmax_kernel(const float* __restrict__ Q,
                                                             const uint4* __restrict__ Qhl,
                                                             const uint4* __restrict__ Chl,
                                                             const float* __restrict__ tmax, int qblocks, int mc_pad,
                                                             int64_t self_offset, float* __restrict__ gmax) {
  const int lane = threadIdx.x;
  const int h = lane >> 5, j = lane & 31;
  const int b0 = 2 * blockIdx.x;
  const bool has1 = b0 + 1 < qblocks;  // wave-uniform
  const int b1 = has1 ? b0 + 1 : b0;
  const float qn0 = knn_query_norm(Q, b0 * 32 + j, h), qn1 = knn_query_norm(Q, b1 * 32 + j, h);
  const KnnQFrag qa = knn_load_qfrag(Qhl, b0 * 32 + j, h), qb = knn_load_qfrag(Qhl, b1 * 32 + j, h);
  // block b's self candidates self_offset + 32 b .. + 31 lie in tile ts + (b - b0) and, when
  // self_offset is no multiple of 32, the tile after it; sr = the lane's self row relative to that tile
  const int ts = self_offset >= 0 ? (int)((self_offset + b0 * 32) >> 5) : -4;
  const int sr = self_offset >= 0 ? (int)((self_offset + b0 * 32) & 31) + j : -64;
  const int d1 = b1 - b0;
  float m0[16], m1[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) m0[r] = m1[r] = kNegBig;
  float tmm = 0.0f;  // the margin grows with the tile's norm bound: the largest bound gives the largest margin
  const int all_tiles = mc_pad / 32;
  const int t_lo = (int)(((int64_t)all_tiles * blockIdx.y) / gridDim.y);
  const int t_hi = (int)(((int64_t)all_tiles * (blockIdx.y + 1)) / gridDim.y);
  auto take = [&](float (&m)[16], const f32x16_t& acc, int dt) {  // dt = t - the block's first self tile
    if (dt == 0 || dt == 1) {  // wave-uniform: the self candidate stays out of the maxima
      const int rs = sr - 32 * dt;
#pragma unroll
      for (int r = 0; r < 16; ++r) m[r] = knn_max(m[r], 4 * h + (r & 3) + 8 * (r >> 2) == rs ? kNegBig : acc[r]);
    } else {
#pragma unroll
      for (int r = 0; r < 16; ++r) m[r] = knn_max(m[r], acc[r]);
    }
  };
  knn_stream_tiles(qa, qb, Chl, tmax, lane, t_lo, t_hi,
                   [&](int t, const f32x16_t& acc0, const f32x16_t& acc1, float tm) {
                     tmm = fmaxf(tmm, tm);
                     take(m0, acc0, t - ts);
                     take(m1, acc1, t - ts - d1);
                   });
  float* o0 = gmax + (int64_t)(blockIdx.y * qblocks + b0) * 17 * kWave + lane;
#pragma unroll
  for (int r = 0; r < 16; ++r) o0[r * kWave] = m0[r];
  o0[16 * kWave] = kMarginScale * fmaf(qn0, tmm, 0.5f * tmm * tmm);
  if (has1) {
    float* o1 = o0 + 17 * kWave;
#pragma unroll
    for (int r = 0; r < 16; ++r) o1[r * kWave] = m1[r];
    o1[16 * kWave] = kMarginScale * fmaf(qn1, tmm, 0.5f * tmm * tmm);
  }
}

// One wave per query block, the lanes as in the passes: thr[q] = T, thr[mq_pad + q] = M.
template <int K>
__global__ __launch_bounds__(kWave) void knn_threshold_kernel(const float* __restrict__ gmax, int nsplit, int mq,
                                                              float* __restrict__ thr) {
  const int lane = threadIdx.x;
  const int qg = blockIdx.x * 32 + (lane & 31);
  float v[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) v[r] = kNegBig;
  float M = 0.0f;
  for (int s = 0; s < nsplit; ++s) {
    const float* g = gmax + (int64_t)(s * gridDim.x + blockIdx.x) * 17 * kWave + lane;
#pragma unroll
    for (int r = 0; r < 16; ++r) v[r] = fmaxf(v[r], g[r * kWave]);
    M = fmaxf(M, g[16 * kWave]);
  }
  float bs[K];  // this half's K largest group maxima, descending
#pragma unroll
  for (int k = 0; k < K; ++k) bs[k] = kNegBig;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    float x = v[r];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const float hi = fmaxf(bs[k], x);
      x = fminf(bs[k], x);
      bs[k] = hi;
    }
  }
  // the K-th largest of the union with the partner's (other half's) K largest
  float ps[K];
#pragma unroll
  for (int k = 0; k < K; ++k) ps[k] = __shfl_xor(bs[k], 32, kWave);
  int ia = 0, ib = 0;
  float kth = kNegBig;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    float a = kNegBig, b = kNegBig;
#pragma unroll
    for (int u = 0; u < K; ++u) { if (u == ia) a = bs[u]; if (u == ib) b = ps[u]; }
    const bool ta = a >= b;
    kth = ta ? a : b;
    ia += ta ? 1 : 0;
    ib += ta ? 0 : 1;
  }
  if (lane < 32) {
    thr[qg] = qg < mq ? kth - M : __builtin_inff();  // a padding query lists nothing
    thr[(int64_t)gridDim.x * 32 + qg] = M;
  }
}

// grid ((qblocks + 1) / 2, nsplit), as pass 1
__global__ __launch_bounds__(kWave) void knn_filter_kernel(const float* __restrict__ Q, const uint4* __restrict__ Qhl,
                                                           const uint4* __restrict__ Chl,
                                                           const float* __restrict__ tmax,
                                                           const float* __restrict__ thr, int qblocks, int mc_pad,
                                                           int mc, int64_t self_offset, int2* __restrict__ lists,
                                                           int* __restrict__ counts) {
  const int lane = threadIdx.x;
  const int h = lane >> 5, j = lane & 31;
  const int b0 = 2 * blockIdx.x;
  const bool has1 = b0 + 1 < qblocks;  // wave-uniform
  const int b1 = has1 ? b0 + 1 : b0;
  const int qg0 = b0 * 32 + j, qg1 = b1 * 32 + j;
  const int64_t self0 = self_offset >= 0 ? self_offset + qg0 : -1, self1 = self_offset >= 0 ? self_offset + qg1 : -1;
  const float qn0 = knn_query_norm(Q, qg0, h), qn1 = knn_query_norm(Q, qg1, h);
  const KnnQFrag qa = knn_load_qfrag(Qhl, qg0, h), qb = knn_load_qfrag(Qhl, qg1, h);
  const int64_t mq_pad = (int64_t)qblocks * 32;
  const float T0 = thr[qg0], M0 = thr[mq_pad + qg0];
  const float T1 = has1 ? thr[qg1] : __builtin_inff(), M1 = thr[mq_pad + qg1];  // the duplicate block lists nothing
  int cnt0 = 0, cnt1 = 0;
  const int64_t lbase0 = (int64_t)(blockIdx.y * qblocks + b0) * kListCap * kWave + lane;
  const int64_t lbase1 = lbase0 + (int64_t)kListCap * kWave;
  const int all_tiles = mc_pad / 32;
  const int t_lo = (int)(((int64_t)all_tiles * blockIdx.y) / gridDim.y);
  const int t_hi = (int)(((int64_t)all_tiles * (blockIdx.y + 1)) / gridDim.y);
  auto filter = [&](int t, const f32x16_t& acc, float tm, float qn, float T, int64_t self_c, int64_t lbase, int& cnt) {
    const float mg = kMarginScale * fmaf(qn, tm, 0.5f * tm * tm);
    const float cut = T - mg;  // upper bound approx + mg >= T
    float m4[4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
      m4[q] = knn_max(knn_max(acc[4 * q], acc[4 * q + 1]), knn_max(acc[4 * q + 2], acc[4 * q + 3]));
    const float mx = knn_max(knn_max(m4[0], m4[1]), knn_max(m4[2], m4[3]));
    if (!__any(mx >= cut)) return;
    const int cbase = t * 32 + 4 * h;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (!__any(m4[q] >= cut)) continue;
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int ci = cbase + rr + 8 * q;
        if (acc[4 * q + rr] >= cut && ci != self_c && ci < mc) {
          if (cnt < kListCap) lists[lbase + (int64_t)cnt * kWave] = make_int2(__float_as_int(acc[4 * q + rr] - mg), ci);
          ++cnt;  // past the cap: counted only (the re-rank scans this query exactly)
        }
      }
    }
  };
  knn_stream_tiles(qa, qb, Chl, tmax, lane, t_lo, t_hi,
                   [&](int t, const f32x16_t& acc0, const f32x16_t& acc1, float tm) {
                     filter(t, acc0, tm, qn0, T0, self0, lbase0, cnt0);
                     filter(t, acc1, tm, qn1, T1, self1, lbase1, cnt1);
                   });
  const int64_t ci0 = (int64_t)(blockIdx.y * qblocks + b0) * kWave + lane;
  const int64_t plane = (int64_t)qblocks * gridDim.y * kWave;
  counts[ci0] = cnt0;
  counts[plane + ci0] = __float_as_int(T0);
  counts[2 * plane + ci0] = __float_as_int(M0);
  if (has1) {
    counts[ci0 + kWave] = cnt1;
    counts[plane + ci0 + kWave] = __float_as_int(T1);
    counts[2 * plane + ci0 + kWave] = __float_as_int(M1);
  }
}

// The re-rank for the two-pass lists: the same exact re-score and ordering as knn_rerank_kernel, so
// the same result bit for bit, but 32 lanes per query, lane l taking the lane lists l, l + 32, ..
// of the query's 2 nsplit (slice, half) lists.  The fixed threshold leaves ~5.6 entries per query
// spread over 18-28 lists, nearly all empty: knn_rerank_kernel's 8 lanes read the lists' counts one
// after the other, a chain of dependent loads that kept it at 41 us whatever the lists held
// (profiles/pr4_knn_twopass).  No skip test: every listed entry has an upper bound >= T.
template <int K>
__global__ __launch_bounds__(256) void knn_rerank_sparse_kernel(const float* __restrict__ Q,
                                                                const float* __restrict__ C, int mq, int mc,
                                                                int qblocks, int nsplit, int64_t self_offset,
                                                                const int2* __restrict__ lists,
                                                                const int* __restrict__ counts,
                                                                int* __restrict__ out_idx,
                                                                float* __restrict__ out_score) {
  const int gl = blockIdx.x * 256 + threadIdx.x;
  const int q = gl >> 5, l = gl & 31;
  const bool live = q < mq;
  const int qq = live ? q : 0;
  const int blk = qq >> 5, j = qq & 31;
  const int64_t self_c = self_offset >= 0 ? self_offset + qq : -1;
  const float4* qp = reinterpret_cast<const float4*>(Q + (int64_t)qq * kCols);
  auto exact = [&](int ci) -> float {  // knn_rerank_kernel's re-score: columns 0..31 in order
    const float4* c = reinterpret_cast<const float4*>(C + (int64_t)ci * kCols);
    float acc = 0.0f;
#pragma unroll
    for (int k = 0; k < kCols / 4; ++k) {
      const float4 v = c[k], w = qp[k];
      acc = fmaf(w.x, v.x, acc);
      acc = fmaf(w.y, v.y, acc);
      acc = fmaf(w.z, v.z, acc);
      acc = fmaf(w.w, v.w, acc);
    }
    return acc;
  };
  float bs[K];
  int bi[K];
#pragma unroll
  for (int k = 0; k < K; ++k) { bs[k] = kNegBig; bi[k] = 0x7fffffff; }
  bool over = false;
  if (live) {
    for (int u = l; u < 2 * nsplit; u += 32) {
      const int64_t lb = (int64_t)(u >> 1) * qblocks + blk;
      const int lane = j + 32 * (u & 1);
      const int n = counts[lb * kWave + lane];
      over |= n > kListCap;
      const int2* li = lists + lb * kListCap * kWave + lane;
      for (int e = 0; e < (n < kListCap ? n : kListCap); ++e) {
        const int ci = li[(int64_t)e * kWave].y;
        topk_insert<K>(bs, bi, exact(ci), ci);
      }
    }
  }
  // a list of the query overflowed (any of its 32 lanes saw it): exact scan of every candidate
  const uint64_t ob = __ballot(over);
  if (live && ((ob >> (threadIdx.x & 32)) & 0xffffffffull) != 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) { bs[k] = kNegBig; bi[k] = 0x7fffffff; }
    for (int ci = l; ci < mc; ci += 32)
      if (ci != self_c) topk_insert<K>(bs, bi, exact(ci), ci);
  }
#pragma unroll
  for (int off = 1; off < 32; off <<= 1) {  // knn_rerank_kernel's butterfly merge, five rounds
    float os[K];
    int oi[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      os[k] = __shfl_xor(bs[k], off, kWave);
      oi[k] = __shfl_xor(bi[k], off, kWave);
    }
    float ns[K];
    int ni[K];
    int ia = 0, ib = 0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      float a = kNegBig, b = kNegBig;
      int ai = 0x7fffffff, bj = 0x7fffffff;
#pragma unroll
      for (int u = 0; u < K; ++u) {
        if (u == ia) { a = bs[u]; ai = bi[u]; }
        if (u == ib) { b = os[u]; bj = oi[u]; }
      }
      const bool ta = !better(b, bj, a, ai);
      ns[k] = ta ? a : b;
      ni[k] = ta ? ai : bj;
      ia += ta ? 1 : 0;
      ib += ta ? 0 : 1;
    }
#pragma unroll
    for (int k = 0; k < K; ++k) { bs[k] = ns[k]; bi[k] = ni[k]; }
  }
  if (live && l == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      out_idx[(int64_t)q * K + k] = bi[k];
      if (out_score) out_score[(int64_t)q * K + k] = bs[k];
    }
  }
}

// ---- bf16x3f: the two passes, the threshold and the re-rank of bf16x3t in ONE launch -----------
// Nothing bf16x3t hands from stage to stage has to leave the CU: a query block's threshold needs only
// that block's group maxima, its re-rank only its own lists.  One workgroup of W waves owns the pair of
// query blocks 2 x, 2 x + 1; wave y streams tile slice y (t_lo = tiles y / W) in both passes.
//   phase 1: knn_groupmax_kernel's maxima in registers, then an LDS integer max per (block, group
//     register, lane) on the order-preserving integer image of the float (a maximum is order-free;
//     no score is -0, the accumulators start at +0) and on the bits of the slice's largest tile bound
//     (>= 0; the margin is monotone in it, so the margin of the largest bound IS the largest margin);
//   phase 2: every wave computes T and M of its lanes' queries with knn_threshold_kernel's arithmetic;
//   phase 3: knn_filter_kernel's test and early outs; a survivor's index goes to its query's LDS list
//     (one counter per query; past the cap counted, not stored);
//   phase 4: 16 lanes per query re-score the listed candidates with knn_rerank_sparse_kernel's chain
//     and merge; a query over the cap scans every candidate exactly.
// The order (score, then index) is total, so neither W nor the order of the appends shows in the result.
// Every wave reaches all three block barriers: nothing returns early, a wave with no tile (more waves
// than tiles) or of the duplicate odd block only has nothing to contribute between them.
// LDS: 8 KiB of maxima + 64 counters + 64 * cap list entries (dynamic).
constexpr int kFusedMaxWaves = 12;  // 3 per SIMD: 168 VGPRs each (16 would leave 128 and spill)
constexpr int kFusedListCap = 64;
constexpr int kFusedMaxCap = 128;
constexpr int kFusedLanes = 16;  // lanes per query in the re-rank

__device__ __forceinline__ int knn_ord(float f) {  // order-preserving float -> int, its own inverse
  const int b = __float_as_int(f);
  return b ^ ((b >> 31) & 0x7fffffff);
}
__device__ __forceinline__ float knn_unord(int i) { return __int_as_float(i ^ ((i >> 31) & 0x7fffffff)); }

// The lane index read afresh (v_mbcnt), opaque to the compiler: what depends only on it (row
// addresses, the self candidates' registers) is then computed where it is used, not ahead of phase 1
// and carried through the phase's tile loop, which alone fills the 168 registers of a 12-wave
// workgroup: carried values went to scratch.
__device__ __forceinline__ int knn_lane_again() {
  int lane;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane));
  return lane;
}

template <int K>
__global__ __launch_bounds__(kFusedMaxWaves* kWave) void knn_twopass_fused_kernel(
    const float* __restrict__ Q, const uint4* __restrict__ Qhl, const float* __restrict__ C,
    const uint4* __restrict__ Chl, const float* __restrict__ tmax, int qblocks, int mq, int mc_pad, int mc,
    int64_t self_offset, int cap, int* __restrict__ out_idx, float* __restrict__ out_score,
    uint8_t* __restrict__ scanned) {
  __shared__ int s_max[2 * 16 * kWave];  // [block][register][lane], knn_ord of the maxima
  __shared__ int s_cnt[2 * 32];          // [block][query]
  __shared__ int s_tmm;
  extern __shared__ int s_list[];        // [block][query][cap] candidate indices
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), W = blockDim.x >> 6;
  const int b0 = 2 * blockIdx.x;
  const bool has1 = b0 + 1 < qblocks;  // block-uniform
  const int b1 = has1 ? b0 + 1 : b0;
  for (int i = threadIdx.x; i < 2 * 16 * kWave; i += blockDim.x) s_max[i] = knn_ord(kNegBig);
  if (threadIdx.x < 2 * 32) s_cnt[threadIdx.x] = 0;
  if (threadIdx.x == 0) s_tmm = 0;
  __syncthreads();
  const int all_tiles = mc_pad / 32;
  const int t_lo = (int)(((int64_t)all_tiles * wave) / W);
  const int t_hi = (int)(((int64_t)all_tiles * (wave + 1)) / W);
  KnnQFrag qa, qb;
  // ---- phase 1: group maxima (knn_groupmax_kernel) ----
  {
    const int lane = threadIdx.x & (kWave - 1);
    const int h = lane >> 5, j = lane & 31;
    qa = knn_load_qfrag(Qhl, b0 * 32 + j, h);
    qb = knn_load_qfrag(Qhl, b1 * 32 + j, h);
    const int ts = self_offset >= 0 ? (int)((self_offset + b0 * 32) >> 5) : -4;
    const int sr0 = self_offset >= 0 ? (int)((self_offset + b0 * 32) & 31) : -64;  // + j: the lane's self row
    const int d1 = b1 - b0;
    float m0[16], m1[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) m0[r] = m1[r] = kNegBig;
    float tmm = 0.0f;
    auto take = [&](float (&m)[16], const f32x16_t& acc, int dt) {
      if (dt == 0 || dt == 1) {  // wave-uniform: the self candidate stays out of the maxima
        const int ln = knn_lane_again();
        const int rs = sr0 + (ln & 31) - 32 * dt - 4 * (ln >> 5);  // register (r & 3) + 8 (r >> 2) of half h
#pragma unroll
        for (int r = 0; r < 16; ++r) m[r] = knn_max(m[r], (r & 3) + 8 * (r >> 2) == rs ? kNegBig : acc[r]);
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) m[r] = knn_max(m[r], acc[r]);
      }
    };
    knn_stream_tiles(qa, qb, Chl, tmax, lane, t_lo, t_hi,
                     [&](int t, const f32x16_t& acc0, const f32x16_t& acc1, float tm) {
                       tmm = fmaxf(tmm, tm);
                       take(m0, acc0, t - ts);
                       take(m1, acc1, t - ts - d1);
                     });
    const int ln = knn_lane_again();
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      atomicMax(&s_max[r * kWave + ln], knn_ord(m0[r]));
      atomicMax(&s_max[(16 + r) * kWave + ln], knn_ord(m1[r]));
    }
    if (ln == 0) atomicMax(&s_tmm, __float_as_int(tmm));
  }
  __syncthreads();
  // ---- phase 2: T and M of this lane's two queries (knn_threshold_kernel) ----
  const int lane = knn_lane_again();
  const int h = lane >> 5, j = lane & 31;
  const int qg0 = b0 * 32 + j, qg1 = b1 * 32 + j;
  const float tmm_all = __int_as_float(s_tmm);
  const float qn0 = knn_query_norm(Q, qg0, h), qn1 = knn_query_norm(Q, qg1, h);
  auto threshold = [&](int blk, float qn, bool real, float& T, float& M) {
    float bs[K];  // this half's K largest group maxima, descending
#pragma unroll
    for (int k = 0; k < K; ++k) bs[k] = kNegBig;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float x = knn_unord(s_max[(blk * 16 + r) * kWave + lane]);
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const float hi = fmaxf(bs[k], x);
        x = fminf(bs[k], x);
        bs[k] = hi;
      }
    }
    float ps[K];
#pragma unroll
    for (int k = 0; k < K; ++k) ps[k] = __shfl_xor(bs[k], 32, kWave);
    int ia = 0, ib = 0;
    float kth = kNegBig;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      float a = kNegBig, b = kNegBig;
#pragma unroll
      for (int u = 0; u < K; ++u) { if (u == ia) a = bs[u]; if (u == ib) b = ps[u]; }
      const bool ta = a >= b;
      kth = ta ? a : b;
      ia += ta ? 1 : 0;
      ib += ta ? 0 : 1;
    }
    kth = __shfl(kth, j, kWave);  // the value knn_threshold_kernel stores: half 0's
    M = kMarginScale * fmaf(qn, tmm_all, 0.5f * tmm_all * tmm_all);
    T = real ? kth - M : __builtin_inff();  // a padding query, and the duplicate block, list nothing
  };
  float T0, M0, T1, M1;
  threshold(0, qn0, qg0 < mq, T0, M0);
  threshold(1, qn1, has1 && qg1 < mq, T1, M1);
  // ---- phase 3: the filter (knn_filter_kernel), survivors to the queries' LDS lists ----
  {
    const int64_t self0 = self_offset >= 0 ? self_offset + qg0 : -1, self1 = self_offset >= 0 ? self_offset + qg1 : -1;
    auto filter = [&](int t, const f32x16_t& acc, float tm, float qn, float T, int64_t self_c, int qi) {
      const float mg = kMarginScale * fmaf(qn, tm, 0.5f * tm * tm);
      const float cut = T - mg;  // upper bound approx + mg >= T
      float m4[4];
#pragma unroll
      for (int q = 0; q < 4; ++q)
        m4[q] = knn_max(knn_max(acc[4 * q], acc[4 * q + 1]), knn_max(acc[4 * q + 2], acc[4 * q + 3]));
      const float mx = knn_max(knn_max(m4[0], m4[1]), knn_max(m4[2], m4[3]));
      if (!__any(mx >= cut)) return;
      const int cbase = t * 32 + 4 * h;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (!__any(m4[q] >= cut)) continue;
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          const int ci = cbase + rr + 8 * q;
          if (acc[4 * q + rr] >= cut && ci != self_c && ci < mc) {
            const int pos = atomicAdd(&s_cnt[qi], 1);
            if (pos < cap) s_list[qi * cap + pos] = ci;  // past the cap: counted only (exact scan below)
          }
        }
      }
    };
    knn_stream_tiles(qa, qb, Chl, tmax, lane, t_lo, t_hi,
                     [&](int t, const f32x16_t& acc0, const f32x16_t& acc1, float tm) {
                       filter(t, acc0, tm, qn0, T0, self0, j);
                       filter(t, acc1, tm, qn1, T1, self1, 32 + j);
                     });
  }
  __syncthreads();
  // ---- phase 4: exact re-rank (knn_rerank_sparse_kernel), kFusedLanes lanes per query ----
  constexpr int kQPW = kWave / kFusedLanes;  // queries a wave re-ranks at a time
  for (int g = wave; g < 2 * 32 / kQPW; g += W) {  // wave-uniform trip count
    const int qi = g * kQPW + lane / kFusedLanes, l = lane & (kFusedLanes - 1);
    const int q = (b0 + (qi >> 5)) * 32 + (qi & 31);
    const bool live = (qi < 32 || has1) && q < mq;
    const int qq = live ? q : 0;
    const int64_t self_c = self_offset >= 0 ? self_offset + qq : -1;
    const float4* qp = reinterpret_cast<const float4*>(Q + (int64_t)qq * kCols);
    auto exact = [&](int ci) -> float {  // knn_rerank_kernel's re-score: columns 0..31 in order
      const float4* c = reinterpret_cast<const float4*>(C + (int64_t)ci * kCols);
      float acc = 0.0f;
#pragma unroll
      for (int k = 0; k < kCols / 4; ++k) {
        const float4 v = c[k], w = qp[k];
        acc = fmaf(w.x, v.x, acc);
        acc = fmaf(w.y, v.y, acc);
        acc = fmaf(w.z, v.z, acc);
        acc = fmaf(w.w, v.w, acc);
      }
      return acc;
    };
    float bs[K];
    int bi[K];
#pragma unroll
    for (int k = 0; k < K; ++k) { bs[k] = kNegBig; bi[k] = 0x7fffffff; }
    const int n = s_cnt[qi];
    const bool over = live && n > cap;  // the same on all lanes of the query
    if (live && !over) {
      for (int e = l; e < n; e += kFusedLanes) {
        const int ci = s_list[qi * cap + e];
        topk_insert<K>(bs, bi, exact(ci), ci);
      }
    }
    if (over) {  // the list overflowed: exact scan of every candidate
      for (int ci = l; ci < mc; ci += kFusedLanes)
        if (ci != self_c) topk_insert<K>(bs, bi, exact(ci), ci);
    }
#pragma unroll
    for (int off = 1; off < kFusedLanes; off <<= 1) {  // knn_rerank_kernel's butterfly merge
      float os[K];
      int oi[K];
#pragma unroll
      for (int k = 0; k < K; ++k) {
        os[k] = __shfl_xor(bs[k], off, kWave);
        oi[k] = __shfl_xor(bi[k], off, kWave);
      }
      float ns[K];
      int ni[K];
      int ia = 0, ib = 0;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        float a = kNegBig, b = kNegBig;
        int ai = 0x7fffffff, bj = 0x7fffffff;
#pragma unroll
        for (int u = 0; u < K; ++u) {
          if (u == ia) { a = bs[u]; ai = bi[u]; }
          if (u == ib) { b = os[u]; bj = oi[u]; }
        }
        const bool ta = !better(b, bj, a, ai);
        ns[k] = ta ? a : b;
        ni[k] = ta ? ai : bj;
        ia += ta ? 1 : 0;
        ib += ta ? 0 : 1;
      }
#pragma unroll
      for (int k = 0; k < K; ++k) { bs[k] = ns[k]; bi[k] = ni[k]; }
    }
    if (live && l == 0) {
#pragma unroll
      for (int k = 0; k < K; ++k) {
        out_idx[(int64_t)q * K + k] = bi[k];
        if (out_score) out_score[(int64_t)q * K + k] = bs[k];
      }
      if (scanned) scanned[q] = over ? 1 : 0;
    }
  }
}

// Merge the per-slice top-k lists of every query (same ordering: score desc, index asc).
// lps (a power of two >= nsplit, <= 64) lanes per query: lane s loads slice s's sorted list, then
// log2(lps) butterfly rounds merge lists pairwise through shuffles (a static-index merge of two
// sorted K-lists).  The order is total (candidate indices are unique across slices), so the
// result equals sequential insertion -- but 13.6k queries x 9 slices take ~4 us instead of the
// ~30 us of one thread walking all slices of a query.
template <int K>
__global__ __launch_bounds__(256) void knn_merge_kernel(const float* __restrict__ ps, const int* __restrict__ pi,
                                                        int nsplit, int lps_log2, int mq, int* __restrict__ out_idx,
                                                        float* __restrict__ out_score) {
  const int gl = blockIdx.x * 256 + threadIdx.x;
  const int q = gl >> lps_log2, sl = gl & ((1 << lps_log2) - 1);
  float bs[K];
  int bi[K];
#pragma unroll
  for (int k = 0; k < K; ++k) { bs[k] = kNegBig; bi[k] = 0x7fffffff; }
  if (q < mq && sl < nsplit) {
    const int64_t o = ((int64_t)sl * mq + q) * K;
#pragma unroll
    for (int k = 0; k < K; ++k) { bs[k] = ps[o + k]; bi[k] = pi[o + k]; }
  }
  for (int off = 1; off < (1 << lps_log2); off <<= 1) {
    float os[K];
    int oi[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      os[k] = __shfl_xor(bs[k], off, kWave);
      oi[k] = __shfl_xor(bi[k], off, kWave);
    }
    float ns[K];
    int ni[K];
    int ia = 0, ib = 0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      float a = kNegBig, b = kNegBig;
      int ai = 0x7fffffff, bj = 0x7fffffff;
#pragma unroll
      for (int u = 0; u < K; ++u) {
        if (u == ia) { a = bs[u]; ai = bi[u]; }
        if (u == ib) { b = os[u]; bj = oi[u]; }
      }
      const bool ta = !better(b, bj, a, ai);
      ns[k] = ta ? a : b;
      ni[k] = ta ? ai : bj;
      ia += ta ? 1 : 0;
      ib += ta ? 0 : 1;
    }
#pragma unroll
    for (int k = 0; k < K; ++k) { bs[k] = ns[k]; bi[k] = ni[k]; }
  }
  if (sl == 0 && q < mq) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      out_idx[(int64_t)q * K + k] = bi[k];
      if (out_score) out_score[(int64_t)q * K + k] = bs[k];
    }
  }
}

}  // namespace

int merge_log2(int nsplit) {
  if (nsplit > kWave) throw std::runtime_error("knn merge: at most 64 candidate slices");
  int l = 0;
  while ((1 << l) < nsplit) ++l;
  return l;
}

unsigned merge_blocks(int mq, int nsplit) {
  return (unsigned)(((int64_t)mq << merge_log2(nsplit)) + 255) / 256;
}

// The list length k is a template parameter of the kernels: f(std::integral_constant<int, k>) for the
// run-time k, so a launcher writes its launches once, as a generic lambda.
template <typename F>
void with_k(int k, const char* who, F&& f) {
  switch (k) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 5: return f(std::integral_constant<int, 5>{});
    case 6: return f(std::integral_constant<int, 6>{});
    case 7: return f(std::integral_constant<int, 7>{});
    case 8: return f(std::integral_constant<int, 8>{});
    default: throw std::runtime_error(std::string(who) + ": k must be in [1, 8]");
  }
}

void launch_knn_prep(const float* X, int m, int m_pad, int role, float* out, float* outq,
                     const double* aff, uint16_t* P, hipStream_t stream, void* chl, void* qhl, float* tmax) {
  if (role < 0 || role > 2 || (role == 2) != (outq != nullptr) || (role == 1 && P != nullptr))
    throw std::invalid_argument("knn_prep: role 2 needs outq (and only it); parents need a candidate role");
  if ((chl != nullptr || qhl != nullptr || tmax != nullptr) &&
      (role != 2 || chl == nullptr || qhl == nullptr || tmax == nullptr || m_pad % 32 != 0))
    throw std::invalid_argument("knn_prep: the fused split needs role 2, all three outputs and m_pad % 32 == 0");
  knn_prep_kernel<<<(m_pad + 255) / 256, 256, 0, stream>>>(X, m, m_pad, role, out, outq, aff, P,
                                                            static_cast<uint4*>(chl), static_cast<uint4*>(qhl), tmax);
  check_launch("knn_prep");
}

void launch_knn_prep_raw(const float* Xraw, int m, int m_pad, float* out, float* outq, uint16_t* P,
                         const KnnRawStats& st, hipStream_t stream, void* chl, void* qhl, float* tmax) {
  if (Xraw == nullptr || out == nullptr || outq == nullptr || m < 0 || m_pad < m)
    throw std::invalid_argument("knn_prep_raw: rows and both operand outputs");
  if ((chl != nullptr || qhl != nullptr || tmax != nullptr) &&
      (chl == nullptr || qhl == nullptr || tmax == nullptr || m_pad % 32 != 0))
    throw std::invalid_argument("knn_prep_raw: the fused split needs all three outputs and m_pad % 32 == 0");
  if (st.d < 1 || st.d > kCols - 2 || st.nparts < 0 || st.nparts > 128 || st.mean32 == nullptr ||
      st.inv32 == nullptr || st.aff == nullptr ||
      (st.nparts > 0 && (st.sums == nullptr || st.pivot == nullptr || st.mean64 == nullptr || st.var64 == nullptr ||
                         st.scale64 == nullptr)))
    throw std::invalid_argument("knn_prep_raw: bad statistics block");
  knn_prep_raw_kernel<<<(m_pad + 255) / 256, 256, 0, stream>>>(Xraw, m, m_pad, out, outq, P, static_cast<uint4*>(chl),
                                                                static_cast<uint4*>(qhl), tmax, st);
  check_launch("knn_prep_raw");
}

int knn_splits(int mq_pad, int mc_pad) {
  // Candidate slices restart their top-k lists (fill cost), so use the fewest slices that fill
  // the resident capacity (one-wave workgroups) with the best whole-round balance.
  static const int cap = resident_cap(knn_topk_kernel<5>, kWave);
  const int qblocks = mq_pad / 32, tiles = mc_pad / 32;
  int max_s = tiles / 8;
  if (max_s > 32) max_s = 32;
  if (max_s < 1) max_s = 1;
  int best = 1;
  double best_eff = -1.0;
  for (int s = 1; s <= max_s; ++s) {
    const double blocks = (double)qblocks * s;
    const double rounds = std::ceil(blocks / cap);
    double eff = blocks / (rounds * cap);            // occupancy of the resident slots over all rounds
    eff -= 0.004 * (s - 1);                          // fill cost of every extra slice
    if (eff > best_eff + 1e-9) { best_eff = eff; best = s; }
  }
  return best;
}

void launch_knn_split(const float* Xp, int m_pad, int role, uint4* hl, float* tmax, hipStream_t stream) {
  knn_split_kernel<<<(m_pad + 255) / 256, 256, 0, stream>>>(Xp, m_pad, role, hl, tmax);
  check_launch("knn_split");
}

int knn3r_list_cap() { return kListCap; }

int knn3r_splits(int mq_pad, int mc_pad) {
  // Six slices (fewer on small candidate sets: >= 16 tiles each).  Round 5 measured 4 best (r5_o:
  // every slice adds its own list entries and re-rank work); with the fragment-order fetch, the
  // re-rank's final-threshold skip and the seeded slices, 6 edges it (profiles/r6_knn
  // slice_sweep.json: 0.162 vs 0.170 ms at DP=1, 0.485 vs 0.491 at the DP=8 rank; 2, 3, 5, 8 slower).
  (void)mq_pad;
  const int tiles = mc_pad / 32;
  int s = tiles / 16;
  if (s > 6) s = 6;
  if (s < 1) s = 1;
  return s;
}

void launch_knn_topk3r(const float* Q, const void* Qhl, int mq_pad, int mq, const float* C, const void* Chl,
                       const float* tmax, int mc_pad, int mc, int64_t self_offset, int k, int* out_idx,
                       float* out_score, int* lists, int* counts, int nsplit, hipStream_t stream) {
  int2* lists2 = reinterpret_cast<int2*>(lists);  // [.. ][cap][64] (lower bound, index) pairs
  if (mq_pad % 32 != 0 || mc_pad % 32 != 0) throw std::runtime_error("knn_topk3r: pads must be x32");
  if (mq > mq_pad || mc > mc_pad || nsplit < 1 || lists == nullptr || counts == nullptr)
    throw std::runtime_error("knn_topk3r: bad shapes or missing list workspaces");
  const dim3 grid(mq_pad / 32, nsplit);
  const uint4* qh = reinterpret_cast<const uint4*>(Qhl);
  const uint4* chl = reinterpret_cast<const uint4*>(Chl);
  const unsigned rblocks = (unsigned)(((int64_t)mq * 8 + 255) / 256);
  with_k(k, "knn_topk3r", [&](auto kk) {
    constexpr int K = decltype(kk)::value;
    knn_collect_kernel<K><<<grid, kWave, 0, stream>>>(Q, qh, chl, tmax, mq, mc_pad, mc, self_offset, lists2, counts);
    knn_rerank_kernel<K><<<rblocks, 256, 0, stream>>>(Q, C, mq, mc, mq_pad / 32, nsplit, self_offset, lists2, counts,
                                                      out_idx, out_score);
  });
  check_launch("knn_topk3r");
}

int knn3t_splits(int mq_pad, int mc_pad) {
  // No slice has a fill phase, so slices cost only their prologue and their gmax / counts rows: as
  // many as fill the resident one-wave workgroups of the passes in one round (156 / 130 VGPRs: 3 waves
  // per SIMD, 3072 on the card -> 14 slices at 13.6k queries), >= 8 tiles each, <= 16 (the list
  // workspace grows with every slice).  profiles/pr4_knn_twopass/lab_sweep.json: 14 is the fastest of
  // 4 / 6 / 8 / 9 / 12 / 14 / 16 at both bench shapes; 16 needs a second round and loses 10 %.
  static const int cap = resident_cap(knn_filter_kernel, kWave);
  const int waves = (mq_pad / 32 + 1) / 2, tiles = mc_pad / 32;  // a wave scores two query blocks
  int s = cap / (waves > 0 ? waves : 1);
  if (s > 16) s = 16;
  if (s > tiles / 8) s = tiles / 8;
  if (s < 1) s = 1;
  return s;
}

void launch_knn_topk3t(const float* Q, const void* Qhl, int mq_pad, int mq, const float* C, const void* Chl,
                       const float* tmax, int mc_pad, int mc, int64_t self_offset, int k, int* out_idx,
                       float* out_score, int* lists, int* counts, float* gmax, float* thr, int nsplit,
                       hipStream_t stream) {
  int2* lists2 = reinterpret_cast<int2*>(lists);
  if (mq_pad % 32 != 0 || mc_pad % 32 != 0) throw std::runtime_error("knn_topk3t: pads must be x32");
  if (mq > mq_pad || mc > mc_pad || nsplit < 1 || lists == nullptr || counts == nullptr || gmax == nullptr ||
      thr == nullptr)
    throw std::runtime_error("knn_topk3t: bad shapes or missing workspaces");
  const int qblocks = mq_pad / 32;
  const dim3 grid((qblocks + 1) / 2, nsplit);  // a wave scores two query blocks
  const uint4* qh = reinterpret_cast<const uint4*>(Qhl);
  const uint4* chl = reinterpret_cast<const uint4*>(Chl);
  const unsigned rblocks = (unsigned)(((int64_t)mq * 32 + 255) / 256);  // 32 lanes per query
  knn_groupmax_kernel<<<grid, kWave, 0, stream>>>(Q, qh, chl, tmax, qblocks, mc_pad, self_offset, gmax);
  with_k(k, "knn_topk3t", [&](auto kk) {
    constexpr int K = decltype(kk)::value;
    knn_threshold_kernel<K><<<qblocks, kWave, 0, stream>>>(gmax, nsplit, mq, thr);
    knn_filter_kernel<<<grid, kWave, 0, stream>>>(Q, qh, chl, tmax, thr, qblocks, mc_pad, mc, self_offset, lists2,
                                                  counts);
    knn_rerank_sparse_kernel<K><<<rblocks, 256, 0, stream>>>(Q, C, mq, mc, qblocks, nsplit, self_offset, lists2,
                                                             counts, out_idx, out_score);
  });
  check_launch("knn_topk3t");
}

int knn3f_list_cap() { return kFusedListCap; }
int knn3f_max_waves() { return kFusedMaxWaves; }

int knn3f_waves(int mq_pad, int mc_pad) {
  // The waves of ONE workgroup share a CU, so W is bounded by what a CU holds of this kernel (the
  // occupancy query below: registers and LDS: 12) and by the tiles (>= 8 each, as knn3t_splits).
  // Of those, 8 = two per SIMD: alone the 13.6k self-search is fastest with 12 (0.108 ms the whole
  // call against 0.115 with 8, 0.118 with 10: lab_sweep.json), but 12 waves of 164 VGPRs need an
  // EMPTY CU, and in the fit the SMOTE bucket sort runs beside the search and its waves sit on
  // every CU: the trace has the 12-wave kernel at 125 us there against ~90 alone.  Two waves per
  // SIMD leave a third of the register file to the neighbour.  The plain bench, alternating, three
  // runs each (waves_in_bench.jsonl): medians 0.858 / 0.858 / 0.864 ms per step with 8, 0.873 /
  // 0.876 / 0.872 with 12, 0.879 / 0.879 / 0.874 with 10, the parent's 0.892 / 0.887 / 0.891
  // (profiles/pr5_knn_fused).
  static const int fit = [] {
    for (int w = kFusedMaxWaves; w > 1; --w) {
      int occ = 0;
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, knn_twopass_fused_kernel<5>, w * kWave,
                                                       (size_t)2 * 32 * kFusedListCap * sizeof(int)) == hipSuccess &&
          occ >= 1)
        return w;
    }
    return 1;
  }();
  (void)mq_pad;
  const int tiles = mc_pad / 32;
  int w = fit < 8 ? fit : 8;
  if (w > tiles / 8) w = tiles / 8;
  if (w < 1) w = 1;
  return w;
}

void launch_knn_topk3f(const float* Q, const void* Qhl, int mq_pad, int mq, const float* C, const void* Chl,
                       const float* tmax, int mc_pad, int mc, int64_t self_offset, int k, int* out_idx,
                       float* out_score, uint8_t* scanned, int waves, int cap, hipStream_t stream) {
  if (mq_pad % 32 != 0 || mc_pad % 32 != 0) throw std::runtime_error("knn_topk3f: pads must be x32");
  if (mq > mq_pad || mc > mc_pad || waves < 1 || waves > kFusedMaxWaves || cap < 1 || cap > kFusedMaxCap)
    throw std::runtime_error("knn_topk3f: bad shapes, waves not in [1, 12] or list cap not in [1, 128]");
  const int qblocks = mq_pad / 32;
  const uint4* qh = reinterpret_cast<const uint4*>(Qhl);
  const uint4* chl = reinterpret_cast<const uint4*>(Chl);
  with_k(k, "knn_topk3f", [&](auto kk) {
    constexpr int K = decltype(kk)::value;
    knn_twopass_fused_kernel<K><<<(qblocks + 1) / 2, waves * kWave, (size_t)2 * 32 * cap * sizeof(int), stream>>>(
        Q, qh, C, chl, tmax, qblocks, mq, mc_pad, mc, self_offset, cap, out_idx, out_score, scanned);
  });
  check_launch("knn_topk3f");
}

void launch_knn_topk(const float* Q, int mq_pad, int mq, const float* C,
                     int mc_pad, int mc, int64_t self_offset, int k, int* out_idx,
                     float* out_score, float* ws_score, int* ws_idx, int nsplit, hipStream_t stream) {
  if (mq_pad % 32 != 0 || mc_pad % 32 != 0) throw std::runtime_error("knn_topk: pads must be x32");
  if (nsplit < 1) nsplit = 1;
  if (nsplit > 1 && (ws_score == nullptr || ws_idx == nullptr))
    throw std::runtime_error("knn_topk: split search needs the [nsplit][mq][k] workspaces");
  const dim3 grid(mq_pad / 32, nsplit);
  int* oi = nsplit > 1 ? ws_idx : out_idx;
  float* os = nsplit > 1 ? ws_score : out_score;
  with_k(k, "knn_topk", [&](auto kk) {
    constexpr int K = decltype(kk)::value;
    knn_topk_kernel<K><<<grid, kWave, 0, stream>>>(Q, mq, C, mc_pad, mc, self_offset, oi, os);
    if (nsplit > 1)
      knn_merge_kernel<K><<<merge_blocks(mq, nsplit), 256, 0, stream>>>(ws_score, ws_idx, nsplit, merge_log2(nsplit),
                                                                        mq, out_idx, out_score);
  });
  check_launch("knn_topk");
}

}  // namespace fdx
