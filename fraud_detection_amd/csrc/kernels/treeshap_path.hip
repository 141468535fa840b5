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
//
// The heap layout, the direction bits, the path merge, the weight sum and the fixed-order sums are
// the family's: tree_explain.h.
#include "launchers.h"
#include "tree_explain.h"

namespace fdx {
namespace {

constexpr int kTPLdsBytes = 65536 - 1024;

// One leaf: heap node 2^D + l of a tree with split features ft [2^D - 1], child fractions fr
// [2^(D+1)] (indexed by heap node) and x's direction bits xb; adds the leaf's Shapley values into
// the thread's phi column ph (stride kTreeThreads per feature).
template <int D>
__device__ __forceinline__ void leaf_shapley(int l, float v, uint32_t xb, const int* __restrict__ ft,
                                             const float* __restrict__ fr, const float* __restrict__ wtab,
                                             float* __restrict__ ph) {
  int fs[D], m;
  float z[D], o[D];
  if (leaf_path<D>(l, xb, ft, fr, fs, z, o, m) || m == 0) return;
  const float* w = wtab + m * 6;  // w[s] = 0 for s >= m, where c[s] = 0 too
#pragma unroll
  for (int i = 0; i < D; ++i) {
    if (fs[i] < 0) continue;
    const float W = excluded_weight<D, D>(z, o, w, i);
    ph[fs[i] * kTreeThreads] += v * (o[i] - z[i]) * W;
  }
}

template <int D, bool TREE_LDS>
__global__ __launch_bounds__(kTreeThreads) void treeshap_path_kernel(
    const float* __restrict__ Xs, int ldx, int d, const int* __restrict__ feat, const float* __restrict__ thr,
    const float* __restrict__ leaf, const float* __restrict__ frac, const uint8_t* __restrict__ dleft, int T,
    float base_margin, float f0, float* __restrict__ phi, float* __restrict__ fx_out, float* __restrict__ f0_out) {
  constexpr int NI = (1 << D) - 1, NL = 1 << D;
  // dynamic LDS: phi table [d][kTreeThreads] | x's direction bits [T] | (TREE_LDS) leaves [T][NL],
  // split features [T][NI], child fractions [T][2 NL]
  extern __shared__ __attribute__((aligned(16))) float tp_dyn[];
  float* ph = tp_dyn;
  uint32_t* xw = reinterpret_cast<uint32_t*>(tp_dyn + d * kTreeThreads);
  __shared__ float xs[32];
  __shared__ float wtab[36];
  __shared__ float red[kTreeThreads / kWave];
  const int e = blockIdx.x, tid = threadIdx.x;
  if (tid < 32) xs[tid] = tid < d ? Xs[(int64_t)e * ldx + tid] : 0.0f;
  fill_shapley_weights(wtab);
  for (int i = tid; i < d * kTreeThreads; i += kTreeThreads) ph[i] = 0.0f;
  const TreeConsts tc = stage_tree_consts<D, TREE_LDS, true>(reinterpret_cast<float*>(xw + T), leaf, feat, frac, T);
  __syncthreads();
  stage_direction_bits<NI>(xs, feat, thr, dleft, T, xw);
  __syncthreads();
  const int npairs = T * NL;
  for (int p = tid; p < npairs; p += kTreeThreads) {
    const int t = p >> D, l = p & (NL - 1);
    leaf_shapley<D>(l, tc.leaf[p], xw[t], tc.feat + t * NI, tc.frac + t * 2 * NL, wtab, ph + tid);
  }
  block_margin_sum<D>(xw, tc.leaf, T, base_margin, f0, red, fx_out + e, f0_out + e);
  const float s = phi_table_sum(ph, d);
  if ((tid & 7) == 0 && (tid >> 3) < d) phi[(int64_t)e * d + (tid >> 3)] = s;
}

size_t tp_base_words(int d, int ntrees) { return (size_t)d * kTreeThreads + ntrees; }
size_t tp_tree_words(int ntrees, int depth) { return (size_t)ntrees * ((4 << depth) - 1); }

}  // namespace

bool treeshap_path_trees_in_lds(int d, int ntrees, int depth) {
  return (tp_base_words(d, ntrees) + tp_tree_words(ntrees, depth)) * sizeof(float) <= (size_t)kTPLdsBytes;
}

void launch_treeshap_path(const float* Xs, int ldx, int n_expl, int d, const int* feat, const float* thr,
                          const float* leaf, const float* frac, const uint8_t* dleft, int ntrees, int depth,
                          float base_margin, float f0, float* phi, float* fx_out, float* f0_out,
                          hipStream_t stream) {
  check_tree_args("treeshap_path", d, ldx, depth, ntrees);
  if (n_expl <= 0) return;
  const bool in_lds = treeshap_path_trees_in_lds(d, ntrees, depth);
  const size_t lds = (tp_base_words(d, ntrees) + (in_lds ? tp_tree_words(ntrees, depth) : 0)) * sizeof(float);
  dispatch_depth(depth, in_lds, [&](auto D, auto LL) {
    treeshap_path_kernel<decltype(D)::value, decltype(LL)::value><<<n_expl, kTreeThreads, lds, stream>>>(
        Xs, ldx, d, feat, thr, leaf, frac, dleft, ntrees, base_margin, f0, phi, fx_out, f0_out);
  });
  check_launch("treeshap_path");
}

}  // namespace fdx
