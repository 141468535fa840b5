// SHAP interaction values of the GBDT family's margin (log-odds): xgboost's
// predict(pred_interactions=True) and shap.TreeExplainer(model).shap_interaction_values, with NO
// background set.  The game is treeshap_path.hip's: v_t(S) is the EXPVALUE recursion over the node
// covers stored in the model, and a NaN in x follows the node's learned default direction.
//
// Per-leaf form: leaf L with value v and the DISTINCT split features M on its path (m = |M|), the
// merged per-feature z_j and o_j exactly as in treeshap_path.hip.  For i != j in M
//     Phi_ij += v (o_i - z_i) (o_j - z_j) sum_s w2(s, m) c_s,   w2(s, m) = s! (m - s - 2)! / (2 (m - 1)!),
// c_s the coefficient of y^s in prod_{k in M, k != i, j} (z_k + o_k y): m - 2 <= 3 linear factors,
// every c_s a sum of non-negative products.  Features off the path are dummies.  The leaf's
// ordinary Shapley values phi_i are treeshap_path.hip's, and the diagonal is
//     Phi_ii = phi_i - sum_{j != i} Phi_ij,
// so the matrix is symmetric, every row sums to phi_i and the whole matrix to margin(x) - f0.
//
// MI355X mapping: one workgroup per explained row; x's direction bits per tree go to LDS once;
// threads run over (tree, leaf) pairs in tree-major order; all of a leaf's work is straight-line
// code on registers (at most 5 phi terms and 10 pair terms).  A private column per thread, as in
// treeshap_path.hip, would take d * d * 256 * 4 B = 900 KiB at d = 30, so the sums are FIXED-POINT
// int64 cells in LDS instead: one per feature (phi_i) and one per unordered pair i < j,
// d (d + 1) / 2 <= 465 cells, added with 64-bit LDS integer atomics (as treecover.hip adds its
// covers).  Integer addition is order-free: no float atomics, results bitwise reproducible and
// equal between the LDS-resident and the streamed path.  All 256 threads share the one set of
// cells: a replica per wave, joined by an integer sum, measured no faster -- 0.128 ms either way
// for 1000 rows x 100 random trees x depth 5 x d = 30, and 0.110 ms either way when every split
// sits on 4 of the 30 columns and all threads meet on 10 cells
// (profiles/treeshap_interactions/README.md).
//
// Scale: with Vmax = max |leaf| <= 2^e (e from the host), a pair term is at most Vmax / 2 and a
// phi term at most Vmax in magnitude, and a cell receives at most 2048 * 32 = 2^16 terms, so units
// of 2^(e - 46) keep every sum below 2^62.  Each fp32 term is converted with one llrint (absolute
// error at most 2^(e - 47)); the accumulation adds none, and the diagonal is formed in integers.
//
// The heap layout, the direction bits, the path merge, the weight sums and the fixed-order margin
// sum are the family's: tree_explain.h.
#include "launchers.h"
#include "tree_explain.h"

namespace fdx {
namespace {

// The per-tree constants go to LDS only while a workgroup's LDS stays within 31 KiB: five
// workgroups then share a CU's 160 KiB, as many as the depth-5 kernel's registers allow, and the
// resident form costs the same as the streamed one.  Beyond that it lowers the occupancy and
// loses: 100 trees at d = 30 (55 KiB, two workgroups per CU) took 0.175 ms resident against
// 0.128 ms streamed for 1000 rows (profiles/treeshap_interactions/README.md).
constexpr int kTILdsBytes = 32768 - 1024;
constexpr int kTIFracBits = 46;

typedef unsigned long long ti_u64;

__device__ __forceinline__ void ti_add(ti_u64* cell, float term, double up) {
  const long long q = llrint((double)term * up);
  if (q != 0) atomicAdd(cell, (ti_u64)q);  // two's complement: the unsigned add is the signed one
}

// One leaf: heap node 2^D + l of a tree with split features ft [2^D - 1], child fractions fr
// [2^(D+1)] (indexed by heap node) and x's direction bits xb; adds the leaf's Shapley values into
// cells acc[f] and its pair terms into acc[d + b (b - 1) / 2 + a], a < b.
template <int D>
__device__ __forceinline__ void leaf_interactions(int l, float v, uint32_t xb, const int* __restrict__ ft,
                                                  const float* __restrict__ fr, const float* __restrict__ wtab,
                                                  const float* __restrict__ w2tab, int d, double up,
                                                  ti_u64* __restrict__ acc) {
  int fs[D], m;
  float z[D], o[D];
  if (leaf_path<D>(l, xb, ft, fr, fs, z, o, m) || m == 0) return;
  float df[D];  // o_i - z_i
#pragma unroll
  for (int i = 0; i < D; ++i) df[i] = o[i] - z[i];
#pragma unroll
  for (int i = 0; i < D; ++i) {
    if (fs[i] < 0) continue;
    // w[s] = 0 for s >= m, where c[s] = 0 too
    ti_add(acc + fs[i], v * df[i] * excluded_weight<D, D>(z, o, wtab + m * 6, i), up);
  }
  if constexpr (D >= 2) {
    if (m < 2) return;
    const float* w2 = w2tab + m * 6;  // w2[s] = 0 for s >= m - 1, as c[s]
#pragma unroll
    for (int i = 0; i < D; ++i) {
#pragma unroll
      for (int j = i + 1; j < D; ++j) {
        if (fs[i] < 0 || fs[j] < 0) continue;
        const float W = excluded_weight<D, D - 1>(z, o, w2, i, j);
        const int a = fs[i] < fs[j] ? fs[i] : fs[j], b = fs[i] < fs[j] ? fs[j] : fs[i];
        ti_add(acc + d + ((b * (b - 1)) >> 1) + a, v * df[i] * df[j] * W, up);
      }
    }
  }
}

template <int D, bool TREE_LDS>
__global__ __launch_bounds__(kTreeThreads) void treeshap_interact_kernel(
    const float* __restrict__ Xs, int ldx, int d, const int* __restrict__ feat, const float* __restrict__ thr,
    const float* __restrict__ leaf, const float* __restrict__ frac, const uint8_t* __restrict__ dleft, int T,
    float base_margin, float f0, int e2, double* __restrict__ inter, float* __restrict__ phi,
    float* __restrict__ fx_out, float* __restrict__ f0_out) {
  constexpr int NI = (1 << D) - 1, NL = 1 << D;
  // dynamic LDS: int64 cells [d (d + 1) / 2] | x's direction bits [T]
  // | (TREE_LDS) leaves [T][NL], split features [T][NI], child fractions [T][2 NL]
  extern __shared__ __attribute__((aligned(16))) unsigned char ti_dyn[];
  const int ncell = (d * (d + 1)) >> 1;
  ti_u64* acc = reinterpret_cast<ti_u64*>(ti_dyn);
  uint32_t* xw = reinterpret_cast<uint32_t*>(acc + ncell);
  __shared__ float xs[32];
  __shared__ float wtab[36];
  __shared__ float w2tab[36];  // [m][s], m = 2 .. 5, s < m - 1: s! (m - s - 2)! / (2 (m - 1)!)
  __shared__ float red[kTreeThreads / kWave];
  __shared__ long long diag[32];
  const int e = blockIdx.x, tid = threadIdx.x;
  if (tid < 32) xs[tid] = tid < d ? Xs[(int64_t)e * ldx + tid] : 0.0f;
  fill_shapley_weights(wtab);
  if (tid < 36) {
    const int m = tid / 6, s = tid % 6;
    w2tab[tid] = (m >= 2 && s < m - 1) ? shap_fact(s) * shap_fact(m - s - 2) / (2.0f * shap_fact(m - 1)) : 0.0f;
  }
  for (int i = tid; i < ncell; i += kTreeThreads) acc[i] = 0ull;
  const TreeConsts tc = stage_tree_consts<D, TREE_LDS, true>(reinterpret_cast<float*>(xw + T), leaf, feat, frac, T);
  __syncthreads();
  stage_direction_bits<NI>(xs, feat, thr, dleft, T, xw);
  __syncthreads();
  const double up = ldexp(1.0, kTIFracBits - e2), down = ldexp(1.0, e2 - kTIFracBits);
  const int npairs = T * NL;
  for (int p = tid; p < npairs; p += kTreeThreads) {
    const int t = p >> D, l = p & (NL - 1);
    leaf_interactions<D>(l, tc.leaf[p], xw[t], tc.feat + t * NI, tc.frac + t * 2 * NL, wtab, w2tab, d, up, acc);
  }
  block_margin_sum<D>(xw, tc.leaf, T, base_margin, f0, red, fx_out + e, f0_out + e);
  const long long* cells = reinterpret_cast<const long long*>(acc);
  if (tid < d) {  // Phi_ii = phi_i - sum_{j != i} Phi_ij, exact in integers
    long long s = cells[tid];
    for (int j = 0; j < d; ++j) {
      if (j == tid) continue;
      const int a = j < tid ? j : tid, b = j < tid ? tid : j;
      s -= cells[d + ((b * (b - 1)) >> 1) + a];
    }
    diag[tid] = s;
    phi[(int64_t)e * d + tid] = (float)((double)cells[tid] * down);
  }
  __syncthreads();
  double* out = inter + (int64_t)e * d * d;
  for (int idx = tid; idx < d * d; idx += kTreeThreads) {
    const int i = idx / d, j = idx - i * d;
    const int a = i < j ? i : j, b = i < j ? j : i;
    const long long q = i == j ? diag[i] : cells[d + ((b * (b - 1)) >> 1) + a];
    out[idx] = (double)q * down;  // one cell feeds [i, j] and [j, i]: symmetric bit for bit
  }
}

size_t ti_base_bytes(int d, int ntrees) {
  return (size_t)(d * (d + 1) / 2) * sizeof(ti_u64) + (size_t)ntrees * sizeof(uint32_t);
}
size_t ti_tree_bytes(int ntrees, int depth) { return (size_t)ntrees * ((4 << depth) - 1) * sizeof(float); }

}  // namespace

bool treeshap_interactions_trees_in_lds(int d, int ntrees, int depth) {
  return ti_base_bytes(d, ntrees) + ti_tree_bytes(ntrees, depth) <= (size_t)kTILdsBytes;
}

void launch_treeshap_interactions(const float* Xs, int ldx, int n_expl, int d, const int* feat, const float* thr,
                                  const float* leaf, const float* frac, const uint8_t* dleft, int ntrees,
                                  int depth, float base_margin, float f0, int leaf_exp, bool stream_trees,
                                  double* inter, float* phi, float* fx_out, float* f0_out, hipStream_t stream) {
  check_tree_args("treeshap_interactions", d, ldx, depth, ntrees);
  if (leaf_exp < -160 || leaf_exp > 128)
    throw std::runtime_error("treeshap_interactions: leaf exponent outside fp32's range");
  if (n_expl <= 0) return;
  const bool in_lds = !stream_trees && treeshap_interactions_trees_in_lds(d, ntrees, depth);
  const size_t lds = ti_base_bytes(d, ntrees) + (in_lds ? ti_tree_bytes(ntrees, depth) : 0);
  dispatch_depth(depth, in_lds, [&](auto D, auto LL) {
    treeshap_interact_kernel<decltype(D)::value, decltype(LL)::value><<<n_expl, kTreeThreads, lds, stream>>>(
        Xs, ldx, d, feat, thr, leaf, frac, dleft, ntrees, base_margin, f0, leaf_exp, inter, phi, fx_out, f0_out);
  });
  check_launch("treeshap_interactions");
}

}  // namespace fdx
