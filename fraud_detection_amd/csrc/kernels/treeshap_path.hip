// Path-dependent TreeSHAP for the GBDT family: exact SHAP values of the ensemble's margin
// (log-odds) with NO background set -- xgboost's predict(pred_contribs=True) and
// shap.TreeExplainer(model) without data.  The node covers stored in the model (treecover.hip)
// take the background's place, and a NaN in x follows the node's learned default direction.
//
// Game: v_t(S) is the EXPVALUE recursion -- at a split node on feature f follow x's direction when
// f is in S, else average the children with weights cover[child] / cover[node] (a split node of
// cover 0 weighs them 1/2 and 1/2; a pass-through node goes left).  phi(x) = sum_t Shapley(v_t),
// f0 = base_margin + sum_t v_t(empty set), sum_f phi = margin(x) - f0.
//
// Per-leaf form: leaf L with value v and the DISTINCT split features M on its path (m = |M| <=
// depth; a leaf to the right of a pass-through node is unreachable and skipped).  For j in M,
// z_j = the product of the path's edge fractions at the nodes that split on j and o_j = 1 iff x
// goes the path's way at all of them.  The leaf's game is v prod_{j in S} o_j prod_{j in M\S} z_j
// and its Shapley value for i in M is
//     v (o_i - z_i) sum_s w(s, m) c_s,    w(s, m) = s! (m - s - 1)! / m!,
// c_s the coefficient of y^s in prod_{j in M, j != i} (z_j + o_j y): m - 1 linear factors
// multiplied out in registers.  Every c_s is a sum of non-negative products, so the inner sum
// has no cancellation.
//
// MI355X mapping (treeshap.hip's, without its divergent walk): one workgroup per explained row;
// x's direction bits per tree go to LDS once (honouring default_left); threads run over (tree,
// leaf) pairs in tree-major order -- a wave covers 64 / 2^depth whole trees, so the per-tree
// constants are near-uniform reads -- and every thread adds into ITS OWN column of an LDS phi
// table; a fixed-order reduce gives the per-feature sums: no atomics, bitwise deterministic.  The
// per-tree constants (split features, leaves, per-child fp32 fractions frac[t][k] = cover[k] /
// cover[parent], computed by the host in fp64 and rounded once) sit in LDS when they fit next to
// the phi table and stream from L2 when they do not.  All of a leaf's work is straight-line code
// on registers: the loops over the depth are unrolled at compile time and a repeated feature is
// merged with selects.
#include "common.h"
#include "launchers.h"

namespace fdx {
namespace {

constexpr int kTPThreads = 256;
constexpr int kTPMaxTrees = 2048;
constexpr int kTPMaxDepth = 5;
constexpr int kTPLdsBytes = 65536 - 1024;

__device__ __forceinline__ float tp_fact(int n) {
  float r = 1.0f;
  for (int i = 2; i <= n; ++i) r *= (float)i;
  return r;
}

template <int D>
__device__ __forceinline__ float tp_tree_margin(uint32_t bits, const float* __restrict__ lf) {
  int node = 1;
#pragma unroll
  for (int l = 0; l < D; ++l) node = (node << 1) | (int)((bits >> node) & 1u);
  return lf[node - (1 << D)];
}

// One leaf: heap node 2^D + l of a tree with split features ft [2^D - 1], child fractions fr
// [2^(D+1)] (indexed by heap node) and x's direction bits xb; adds the leaf's Shapley values into
// the thread's phi column ph (stride kTPThreads per feature).
template <int D>
__device__ __forceinline__ void leaf_shapley(int l, float v, uint32_t xb, const int* __restrict__ ft,
                                             const float* __restrict__ fr, const float* __restrict__ wtab,
                                             float* __restrict__ ph) {
  const int heap = (1 << D) + l;
  int fs[D];
  float z[D], o[D];
  bool dead = false;
  int m = 0;
#pragma unroll
  for (int j = 0; j < D; ++j) {
    const int k = heap >> (D - j);      // the path's node at level j
    const int c = heap >> (D - j - 1);  // and the child it continues to
    const int f = ft[k - 1];
    const int dir = c & 1;
    fs[j] = -1;
    z[j] = 1.0f;
    o[j] = 0.0f;
    if (f < 0) {
      dead = dead || dir != 0;  // right of a pass-through node: no row gets here
    } else {
      const float e = fr[c];
      const float ag = (int)((xb >> k) & 1u) == dir ? 1.0f : 0.0f;
      bool found = false;
#pragma unroll
      for (int i = 0; i < j; ++i) {
        if (fs[i] == f) {  // the feature is on the path already: one merged factor
          z[i] *= e;
          o[i] *= ag;
          found = true;
        }
      }
      if (!found) {
        fs[j] = f;
        z[j] = e;
        o[j] = ag;
        ++m;
      }
    }
  }
  if (dead || m == 0) return;
  const float* w = wtab + m * 6;
#pragma unroll
  for (int i = 0; i < D; ++i) {
    if (fs[i] < 0) continue;
    // c[s]: coefficient of y^s in prod_{j != i} (z_j + o_j y); an empty slot is the factor 1
    float c[D];
    c[0] = 1.0f;
#pragma unroll
    for (int s = 1; s < D; ++s) c[s] = 0.0f;
#pragma unroll
    for (int j = 0; j < D; ++j) {
      if (j == i) continue;
#pragma unroll
      for (int s = D - 1; s >= 1; --s) c[s] = c[s] * z[j] + c[s - 1] * o[j];
      c[0] = c[0] * z[j];
    }
    float W = 0.0f;
#pragma unroll
    for (int s = 0; s < D; ++s) W += w[s] * c[s];  // w[s] = 0 for s >= m, where c[s] = 0 too
    ph[fs[i] * kTPThreads] += v * (o[i] - z[i]) * W;
  }
}

template <int D, bool TREE_LDS>
__global__ __launch_bounds__(kTPThreads) void treeshap_path_kernel(
    const float* __restrict__ Xs, int ldx, int d, const int* __restrict__ feat, const float* __restrict__ thr,
    const float* __restrict__ leaf, const float* __restrict__ frac, const uint8_t* __restrict__ dleft, int T,
    float base_margin, float f0, float* __restrict__ phi, float* __restrict__ fx_out, float* __restrict__ f0_out) {
  constexpr int NI = (1 << D) - 1, NL = 1 << D;
  // dynamic LDS: phi table [d][kTPThreads] | x's direction bits [T] | (TREE_LDS) leaves [T][NL],
  // split features [T][NI], child fractions [T][2 NL]
  extern __shared__ __attribute__((aligned(16))) float tp_dyn[];
  float* ph = tp_dyn;
  uint32_t* xw = reinterpret_cast<uint32_t*>(tp_dyn + d * kTPThreads);
  float* lfs = reinterpret_cast<float*>(xw + T);
  int* fts = reinterpret_cast<int*>(lfs + (TREE_LDS ? T * NL : 0));
  float* frs = reinterpret_cast<float*>(fts + (TREE_LDS ? T * NI : 0));
  __shared__ float xs[32];
  __shared__ float wtab[36];  // [m][s], m = 1 .. 5, s < m: s! (m - s - 1)! / m!
  __shared__ float red[kTPThreads / kWave];
  const int e = blockIdx.x, tid = threadIdx.x;
  if (tid < 32) xs[tid] = tid < d ? Xs[(int64_t)e * ldx + tid] : 0.0f;
  if (tid < 36) {
    const int m = tid / 6, s = tid % 6;
    wtab[tid] = (m >= 1 && s < m) ? tp_fact(s) * tp_fact(m - s - 1) / tp_fact(m) : 0.0f;
  }
  for (int i = tid; i < d * kTPThreads; i += kTPThreads) ph[i] = 0.0f;
  if constexpr (TREE_LDS) {
    for (int i = tid; i < T * NL; i += kTPThreads) lfs[i] = leaf[i];
    for (int i = tid; i < T * NI; i += kTPThreads) fts[i] = feat[i];
    for (int i = tid; i < T * 2 * NL; i += kTPThreads) frs[i] = frac[i];
  }
  __syncthreads();
  // x's direction bits per tree (bit n + 1: internal node n sends x right; a NaN goes left where
  // the node's default_left byte is set; pass-through: left)
  for (int t = tid; t < T; t += kTPThreads) {
    uint32_t m = 0;
    for (int n = 0; n < NI; ++n) {
      const int f = feat[t * NI + n];
      if (f >= 0) {
        const float x = xs[f];
        const bool nan_left = x != x && dleft != nullptr && dleft[t * NI + n] != 0;
        if (!(x < thr[t * NI + n]) && !nan_left) m |= 2u << n;
      }
    }
    xw[t] = m;
  }
  __syncthreads();
  const float* LF = TREE_LDS ? lfs : leaf;
  const int* FT = TREE_LDS ? fts : feat;
  const float* FR = TREE_LDS ? frs : frac;
  const int npairs = T * NL;
  for (int p = tid; p < npairs; p += kTPThreads) {
    const int t = p >> D, l = p & (NL - 1);
    leaf_shapley<D>(l, LF[p], xw[t], FT + t * NI, FR + t * 2 * NL, wtab, ph + tid);
  }
  // f(x): this thread's trees, then a fixed-order block sum (tree order within a thread)
  float mx = 0.0f;
  for (int t = tid; t < T; t += kTPThreads) mx += tp_tree_margin<D>(xw[t], LF + t * NL);
  mx = wave_sum(mx);
  if (lane_id() == 0) red[wave_id()] = mx;
  __syncthreads();
  // phi[f] = the sum over the table's 256 columns: 8 threads per feature, 32 columns each
  const int f = tid >> 3, part = tid & 7;
  float s = 0.0f;
  if (f < d) {
    const float* row = ph + f * kTPThreads + part * 32;
#pragma unroll 8
    for (int i = 0; i < 32; ++i) s += row[i];
  }
  s = group_sum<8>(s);
  if (part == 0 && f < d) phi[(int64_t)e * d + f] = s;
  if (tid == 0) {
    float m = base_margin;
    for (int w = 0; w < kTPThreads / kWave; ++w) m += red[w];
    fx_out[e] = m;
    f0_out[e] = f0;
  }
}

size_t tp_base_words(int d, int ntrees) { return (size_t)d * kTPThreads + ntrees; }
size_t tp_tree_words(int ntrees, int depth) { return (size_t)ntrees * ((4 << depth) - 1); }

}  // namespace

bool treeshap_path_trees_in_lds(int d, int ntrees, int depth) {
  return (tp_base_words(d, ntrees) + tp_tree_words(ntrees, depth)) * sizeof(float) <= (size_t)kTPLdsBytes;
}

void launch_treeshap_path(const float* Xs, int ldx, int n_expl, int d, const int* feat, const float* thr,
                          const float* leaf, const float* frac, const uint8_t* dleft, int ntrees, int depth,
                          float base_margin, float f0, float* phi, float* fx_out, float* f0_out,
                          hipStream_t stream) {
  if (d < 1 || d > 30) throw std::runtime_error("treeshap_path: 1 <= d <= 30");
  if (ldx < d) throw std::runtime_error("treeshap_path: row stride below the feature count");
  if (depth < 1 || depth > kTPMaxDepth) throw std::runtime_error("treeshap_path: depth must be in [1, 5]");
  if (ntrees < 1 || ntrees > kTPMaxTrees) throw std::runtime_error("treeshap_path: 1 <= trees <= 2048");
  if (n_expl <= 0) return;
  const bool in_lds = treeshap_path_trees_in_lds(d, ntrees, depth);
  const size_t lds = (tp_base_words(d, ntrees) + (in_lds ? tp_tree_words(ntrees, depth) : 0)) * sizeof(float);
#define FDX_TP(D_, LL)                                                                                   \
  treeshap_path_kernel<D_, LL><<<n_expl, kTPThreads, lds, stream>>>(Xs, ldx, d, feat, thr, leaf, frac,    \
                                                                    dleft, ntrees, base_margin, f0, phi,  \
                                                                    fx_out, f0_out)
#define FDX_TP_D(D_)                          \
  do {                                        \
    if (in_lds) FDX_TP(D_, true);             \
    else FDX_TP(D_, false);                   \
  } while (0)
  switch (depth) {
    case 1: FDX_TP_D(1); break;
    case 2: FDX_TP_D(2); break;
    case 3: FDX_TP_D(3); break;
    case 4: FDX_TP_D(4); break;
    default: FDX_TP_D(5); break;
  }
#undef FDX_TP_D
#undef FDX_TP
  check_launch("treeshap_path");
}

}  // namespace fdx
