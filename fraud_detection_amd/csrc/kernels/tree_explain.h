// The tree explainer family's shared device code: treeshap.hip (interventional TreeSHAP),
// treeshap_path.hip (path-dependent TreeSHAP), treeshap_interact.hip (SHAP interaction values)
// and the tree kernel of kernelshap.hip.  Every piece below has this one definition, so what the
// kernels promise one another -- fx bit for bit equal between them, the same game (z_j, o_j, dead
// leaves, NaN routing) in the path and the interactions kernel -- holds by construction.
//
// What holds for the whole family:
// - A tree is a complete binary heap of depth D <= 5, nodes 1-based: node k has children 2k and
//   2k + 1, leaf l is heap node 2^D + l.  feat / thr / default_left are [T][2^D - 1] over the
//   internal nodes (index k - 1), leaf is [T][2^D]; feat < 0 marks a pass-through node, which
//   every row leaves to the left.
// - A row's directions in one tree are ONE 32-bit word: bit k is set where heap node k sends the
//   row right ("not less than the threshold"), so the 31 internal nodes of a depth-5 tree fit and
//   a walk is two VALU operations per level.
// - One workgroup of 256 threads per explained row (kernelshap.hip: per row and coalition part);
//   x's words go to LDS once per workgroup; rows are the scaler's 32 padded fp32 columns, d <= 30.
// - Sums run in a fixed order -- per-thread columns or integer cells, never float atomics -- so
//   every output is bitwise reproducible.
// - The per-tree constants sit in LDS when they fit next to the kernel's accumulators and stream
//   from L2 when they do not; each kernel file states its own limit.
#pragma once
#include <stdexcept>
#include <string>
#include <type_traits>

#include "common.h"

namespace fdx {

constexpr int kTreeThreads = 256;
constexpr int kTreeMaxTrees = 2048;
constexpr int kTreeMaxDepth = 5;
constexpr int kTreeMaxFeatures = 30;

// ---- Shapley weights -----------------------------------------------------------------------
__device__ __forceinline__ float shap_fact(int n) {
  float r = 1.0f;
  for (int i = 2; i <= n; ++i) r *= (float)i;
  return r;
}

// wtab[m][s] = s! (m - s - 1)! / m! for m = 1 .. 5, s < m, and 0 elsewhere: the Shapley weight of
// a coalition of s among m players.  Threads 0 .. 35 fill the [6][6] table.
__device__ __forceinline__ void fill_shapley_weights(float* wtab) {
  const int tid = threadIdx.x;
  if (tid < 36) {
    const int m = tid / 6, s = tid % 6;
    wtab[tid] = (m >= 1 && s < m) ? shap_fact(s) * shap_fact(m - s - 1) / shap_fact(m) : 0.0f;
  }
}

// ---- the walk --------------------------------------------------------------------------------
// Leaf index reached from the direction bits (bit k: heap node k goes right).
template <int D>
__device__ __forceinline__ int tree_leaf(uint32_t bits) {
  int node = 1;
#pragma unroll
  for (int l = 0; l < D; ++l) node = (node << 1) | (int)((bits >> node) & 1u);
  return node - (1 << D);
}

template <int D>
__device__ __forceinline__ float tree_margin(uint32_t bits, const float* __restrict__ lf) {
  return lf[tree_leaf<D>(bits)];
}

// Direction bits of the row xs in one tree (feat / thr / dleft point at the tree's NI internal
// nodes).  A NaN goes left where the node's default_left byte is set and right otherwise;
// dleft == nullptr: no default directions, the comparison alone.
template <int NI>
__device__ __forceinline__ uint32_t direction_bits(const float* xs, const int* __restrict__ feat,
                                                   const float* __restrict__ thr,
                                                   const uint8_t* __restrict__ dleft) {
  uint32_t m = 0;
  for (int n = 0; n < NI; ++n) {
    const int f = feat[n];
    if (f >= 0) {
      const float x = xs[f];
      const bool nan_left = x != x && dleft != nullptr && dleft[n] != 0;
      if (!(x < thr[n]) && !nan_left) m |= 2u << n;
    }
  }
  return m;
}

// The workgroup's row in all T trees, into xw [T].  The caller synchronises before reading xw.
template <int NI>
__device__ __forceinline__ void stage_direction_bits(const float* xs, const int* __restrict__ feat,
                                                     const float* __restrict__ thr,
                                                     const uint8_t* __restrict__ dleft, int T, uint32_t* xw) {
  for (int t = threadIdx.x; t < T; t += kTreeThreads)
    xw[t] = direction_bits<NI>(xs, feat + t * NI, thr + t * NI, dleft != nullptr ? dleft + t * NI : nullptr);
}

// ---- per-tree constants ------------------------------------------------------------------------
struct TreeConsts {
  const float* leaf;  // [T][2^D]
  const int* feat;    // [T][2^D - 1]
  const float* frac;  // [T][2^(D+1)] child fractions by heap node (path-dependent game), or null
};

// IN_LDS: copy leaves [T][NL], split features [T][NI] and (FRAC) fractions [T][2 NL]
// to `lds` in this order and return the copies; otherwise return the global arrays.  The caller
// synchronises before the first read.
template <int D, bool IN_LDS, bool FRAC>
__device__ __forceinline__ TreeConsts stage_tree_consts(float* lds, const float* __restrict__ leaf,
                                                            const int* __restrict__ feat,
                                                            const float* __restrict__ frac, int T) {
  constexpr int NI = (1 << D) - 1, NL = 1 << D;
  if constexpr (IN_LDS) {
    float* lfs = lds;
    int* fts = reinterpret_cast<int*>(lfs + T * NL);
    float* frs = reinterpret_cast<float*>(fts + T * NI);
    const int tid = threadIdx.x;
    for (int i = tid; i < T * NL; i += kTreeThreads) lfs[i] = leaf[i];
    for (int i = tid; i < T * NI; i += kTreeThreads) fts[i] = feat[i];
    if constexpr (FRAC) {
      for (int i = tid; i < T * 2 * NL; i += kTreeThreads) frs[i] = frac[i];
    }
    return TreeConsts{lfs, fts, FRAC ? frs : nullptr};
  } else {
    return TreeConsts{leaf, feat, frac};
  }
}

// ---- the path-dependent game, per leaf -----------------------------------------------------------
// Leaf l (heap node 2^D + l) of a tree with split features ft [2^D - 1], child fractions fr
// [2^(D+1)] (fr[c] = cover[c] / cover[parent of c]) and x's direction bits xb.  The DISTINCT split
// features on the leaf's path are merged into slots: fs[i] the feature (-1: empty slot, the
// factor 1), z[i] the product of the path's edge fractions at the nodes that split on it, o[i] = 1
// iff x goes the path's way at all of them; m the number of slots in use.  Returns `dead`: the
// leaf lies to the right of a pass-through node and no row reaches it.  The results are plain
// arrays of the caller's, not a struct: filled through a struct, treeshap_interact_kernel<4, false>
// took 74 VGPRs instead of 72 and lost a wave per SIMD (profiles/tree_explain_shared).
template <int D>
__device__ __forceinline__ bool leaf_path(int l, uint32_t xb, const int* __restrict__ ft, const float* __restrict__ fr,
                                          int (&fs)[D], float (&z)[D], float (&o)[D], int& m) {
  const int heap = (1 << D) + l;
  bool dead = false;
  m = 0;
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
  return dead;
}

// sum_s w[s] c_s, c_s the coefficient of y^s in prod_k (z_k + o_k y) over the D slots other than
// i and j (j = -1: other than i alone); NC = the number of coefficients, D less the excluded slots
// plus one.  An empty slot is the factor 1; every c_s is a sum of non-negative products, so the
// sum has no cancellation.  w[s] = 0 wherever c_s = 0 for want of factors.
template <int D, int NC>
__device__ __forceinline__ float excluded_weight(const float (&z)[D], const float (&o)[D],
                                                 const float* __restrict__ w, int i, int j = -1) {
  float c[NC];
  c[0] = 1.0f;
#pragma unroll
  for (int s = 1; s < NC; ++s) c[s] = 0.0f;
#pragma unroll
  for (int k = 0; k < D; ++k) {
    if (k == i || k == j) continue;
#pragma unroll
    for (int s = NC - 1; s >= 1; --s) c[s] = c[s] * z[k] + c[s - 1] * o[k];
    c[0] = c[0] * z[k];
  }
  float W = 0.0f;
#pragma unroll
  for (int s = 0; s < NC; ++s) W += w[s] * c[s];
  return W;
}

// ---- block sums ------------------------------------------------------------------------------------
// f(x) = base_margin + the sum of the trees' leaves, in a fixed order: thread tid adds its trees
// tid, tid + 256, ..., wave_sum joins the lanes, thread 0 adds the waves' sums to base_margin in
// wave order and writes *fx_out and *f0_out.  Contains one __syncthreads(), which also orders the
// workgroup's earlier LDS writes before whatever follows the call.
template <int D>
__device__ __forceinline__ void block_margin_sum(const uint32_t* xw, const float* leaf, int T, float base_margin,
                                                 float f0, float* red, float* __restrict__ fx_out,
                                                 float* __restrict__ f0_out) {
  float mx = 0.0f;
  for (int t = threadIdx.x; t < T; t += kTreeThreads) mx += tree_margin<D>(xw[t], leaf + (t << D));
  mx = wave_sum(mx);
  if (lane_id() == 0) red[wave_id()] = mx;
  __syncthreads();
  if (threadIdx.x == 0) {
    float m = base_margin;
    for (int w = 0; w < kTreeThreads / kWave; ++w) m += red[w];
    *fx_out = m;
    *f0_out = f0;
  }
}

// Column sum of the phi table ph [d][256] (one column per thread): 8 threads per feature, 32
// columns each, joined in a fixed order.  Valid in the threads with (tid & 7) == 0 and
// tid >> 3 < d, for feature tid >> 3.
__device__ __forceinline__ float phi_table_sum(const float* ph, int d) {
  const int f = threadIdx.x >> 3, part = threadIdx.x & 7;
  float s = 0.0f;
  if (f < d) {
    const float* row = ph + f * kTreeThreads + part * 32;
#pragma unroll 8
    for (int i = 0; i < 32; ++i) s += row[i];
  }
  return group_sum<8>(s);
}

// ---- host side -----------------------------------------------------------------------------------
// The launchers' shared argument checks; `name` starts every message.
inline void check_tree_args(const char* name, int d, int ldx, int depth, int ntrees) {
  const std::string n(name);
  if (d < 1 || d > kTreeMaxFeatures) throw std::runtime_error(n + ": 1 <= d <= 30");
  if (ldx < d) throw std::runtime_error(n + ": row stride below the feature count");
  if (depth < 1 || depth > kTreeMaxDepth) throw std::runtime_error(n + ": depth must be in [1, 5]");
  if (ntrees < 1 || ntrees > kTreeMaxTrees) throw std::runtime_error(n + ": 1 <= trees <= 2048");
}

// Calls f(std::integral_constant<int, depth>{}, std::bool_constant<flag>{}): the kernels take the
// depth and whether the per-tree constants are in LDS as template arguments.
template <typename F>
inline void dispatch_depth(int depth, bool flag, F&& f) {
  auto with_depth = [&](auto D) {
    if (flag) f(D, std::true_type{});
    else f(D, std::false_type{});
  };
  switch (depth) {
    case 1: with_depth(std::integral_constant<int, 1>{}); break;
    case 2: with_depth(std::integral_constant<int, 2>{}); break;
    case 3: with_depth(std::integral_constant<int, 3>{}); break;
    case 4: with_depth(std::integral_constant<int, 4>{}); break;
    default: with_depth(std::integral_constant<int, 5>{}); break;
  }
}

}  // namespace fdx
