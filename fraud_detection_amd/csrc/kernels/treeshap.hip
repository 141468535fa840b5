// K7b interventional TreeSHAP for the GBDT family: exact SHAP values of the ensemble's margin
// (log-odds) against a background set, per explanation.
//
// Reference behaviour: shap.TreeExplainer(model, data=background, feature_perturbation=
// "interventional", model_output="raw") on the XGBClassifier the reference trains
// (train_model.py:95-113; the explainer family of explain_model.py:24-27 for trees).  The
// model-agnostic KernelSHAP path (kernelshap.hip, tree kernel) samples 2042 coalitions and walks
// every tree once per (coalition, background row); this computes the same attributions exactly,
// with no coalition sampling, in O(reachable leaves) per (background row, tree).
//
// For one explained row x and one background row z the hybrid game v(S) = f(x_S, z_~S) of a tree
// is a sum over leaves of v_L 1[A_L in S, B_L disjoint from S], where A_L (B_L) are the features
// whose split sends the path the way x (z) goes while z (x) goes the other way.  The Shapley
// value of such a term is v_L (a-1)! b! / (a+b)! for i in A_L and -v_L a! (b-1)! / (a+b)! for i
// in B_L (a = |A_L|, b = |B_L|).  A depth-first walk follows the x- and z-branches at nodes where
// they differ (a feature already in A or B is forced to its side), so it visits only the leaves
// some hybrid reaches -- 1 to a few per (z, tree) in practice, at most 2^depth.
// phi(x) = mean over z of the per-z values; sum(phi) = margin(x) - mean_z margin(z) exactly.
//
// MI355X mapping: one workgroup per explanation; x's direction bits per tree go to LDS once,
// the background rows' bits (per tree, precomputed per design) stream from L2; each thread owns
// (tree, background row) pairs in tree-major order (neighbouring threads share a tree: uniform
// feat / leaf reads) and accumulates into ITS OWN column of an LDS phi table, so there are no
// atomics and the final per-feature sums run in a fixed order: bitwise deterministic.  The
// walk is a compile-time recursion over the depth with two call sites per level (2^D inlined
// leaf handlers).  Measured (profiles/r2_s3u): 0.82-0.87 ms per 1000 explanations x 100 trees x
// 100 background rows (3.5e7 values/s, 17x the sampled tree KernelSHAP and exact); the cost is
// branch divergence -- a wave walks the union of its 64 lanes' paths through the ~3,900-
// instruction inlined tree -- not LDS or global latency (staging the split features in LDS and
// no-return LDS atomics both measured flat).  A divergence-free variant with lanes over leaves
// (reachability of all 2^D leaves tested with bit masks per background row) measured slower,
// 1.36-1.42 ms: it tests every leaf where the walk visits only reachable ones.
//
// The heap layout, the direction bits, the walk and the fixed-order sums are the family's:
// tree_explain.h.
#include "launchers.h"
#include "tree_explain.h"

namespace fdx {
namespace {

struct LeafCtx {
  const float* lf;    // this tree's leaves
  float* ph;          // LDS phi table [feature][kTreeThreads] (this thread's column at + tid)
  const float* wp;    // [6][6] weights
  const float* wn;
};

template <int D, int L>
__device__ __forceinline__ void walk_pairs(int k, uint32_t A, uint32_t B, uint32_t xb, uint32_t zb,
                                           const int* __restrict__ ft, const LeafCtx& c) {
  if constexpr (L == D) {
    if ((A | B) == 0u) return;  // x and z reach this leaf together: no attribution
    const float v = c.lf[k - (1 << D)];
    const int a = __popc(A), b = __popc(B);
    const float pw = v * c.wp[a * 6 + b], nw = v * c.wn[a * 6 + b];
    for (uint32_t m = A; m; m &= m - 1u) c.ph[(__ffs(m) - 1) * kTreeThreads] += pw;
    for (uint32_t m = B; m; m &= m - 1u) c.ph[(__ffs(m) - 1) * kTreeThreads] -= nw;
  } else {
    const int f = ft[k - 1];
    int c1 = 2 * k, c2 = 0;
    uint32_t A1 = A, B2 = B;
    if (f >= 0) {
      const int dx = (int)((xb >> k) & 1u), dz = (int)((zb >> k) & 1u);
      const uint32_t bit = 1u << f;
      if (dx == dz || (A & bit)) {
        c1 = 2 * k + dx;
      } else if (B & bit) {
        c1 = 2 * k + dz;
      } else {  // the hybrids split here: x's side puts f in A, z's side puts f in B
        c1 = 2 * k + dx;
        A1 = A | bit;
        c2 = 2 * k + dz;
        B2 = B | bit;
      }
    }
    walk_pairs<D, L + 1>(c1, A1, B, xb, zb, ft, c);
    if (c2) walk_pairs<D, L + 1>(c2, A, B2, xb, zb, ft, c);
  }
}

template <int D, bool LEAF_LDS>
__global__ __launch_bounds__(kTreeThreads) void treeshap_kernel(
    const float* __restrict__ Xs, int ldx, int d, const int* __restrict__ feat, const float* __restrict__ thr,
    const float* __restrict__ leaf, int T, float base_margin, const uint32_t* __restrict__ bw, int bw_ld,
    int n_bg, float f0, float* __restrict__ phi, float* __restrict__ fx_out, float* __restrict__ f0_out) {
  constexpr int NI = (1 << D) - 1, NL = 1 << D;
  // dynamic LDS: phi table [d][kTreeThreads] | x's direction bits [T] | (LEAF_LDS) leaves [T][NL]
  // and split features [T][NI] -- the walk reads one feature per level on a dependent chain,
  // an L2 round trip each from global memory
  extern __shared__ __attribute__((aligned(16))) float dyn[];
  float* ph = dyn;
  uint32_t* xw = reinterpret_cast<uint32_t*>(dyn + d * kTreeThreads);
  __shared__ float xs[32];
  __shared__ float wtab[2][36];
  __shared__ float red[kTreeThreads / kWave];
  const int e = blockIdx.x, tid = threadIdx.x;
  if (tid < 32) xs[tid] = tid < d ? Xs[(int64_t)e * ldx + tid] : 0.0f;
  // Shapley weights of a leaf term with a = |A|, b = |B| (a + b <= depth): positive (features in
  // A) (a-1)! b! / (a+b)!, negative (features in B) a! (b-1)! / (a+b)!
  if (tid < 36) {
    const int a = tid / 6, b = tid % 6;
    const float den = shap_fact(a + b);
    wtab[0][tid] = (a >= 1) ? shap_fact(a - 1) * shap_fact(b) / den : 0.0f;
    wtab[1][tid] = (b >= 1) ? shap_fact(a) * shap_fact(b - 1) / den : 0.0f;
  }
  for (int i = tid; i < d * kTreeThreads; i += kTreeThreads) ph[i] = 0.0f;
  const TreeConsts tc = stage_tree_consts<D, LEAF_LDS, false>(reinterpret_cast<float*>(xw + T), leaf, feat, nullptr, T);
  __syncthreads();
  stage_direction_bits<NI>(xs, feat, thr, nullptr, T, xw);
  __syncthreads();
  LeafCtx c{nullptr, ph + tid, wtab[0], wtab[1]};
  const int npairs = T * n_bg;
  // (tree, background) pairs in tree-major order; the next pair's background bits are loaded
  // while this pair is walked
  int p = tid;
  uint32_t zb_next = 0;
  if (p < npairs) zb_next = bw[(int64_t)(p / n_bg) * bw_ld + (p % n_bg)];
  for (; p < npairs; p += kTreeThreads) {
    const int t = p / n_bg;
    const uint32_t zb = zb_next;
    const int pn = p + kTreeThreads;
    if (pn < npairs) zb_next = bw[(int64_t)(pn / n_bg) * bw_ld + (pn % n_bg)];
    c.lf = tc.leaf + t * NL;
    walk_pairs<D, 0>(1, 0u, 0u, xw[t], zb, tc.feat + t * NI, c);
  }
  block_margin_sum<D>(xw, tc.leaf, T, base_margin, f0, red, fx_out + e, f0_out + e);
  // phi[f] = (sum over the table's 256 columns) / n_bg
  const float s = phi_table_sum(ph, d);
  if ((tid & 7) == 0 && (tid >> 3) < d) phi[(int64_t)e * d + (tid >> 3)] = s / (float)n_bg;
}

}  // namespace

void launch_treeshap(const float* Xs, int ldx, int n_expl, int d, const int* feat, const float* thr,
                     const float* leaf, int ntrees, int depth, float base_margin, const uint32_t* bw, int bw_ld,
                     int n_bg, float f0, float* phi, float* fx_out, float* f0_out, hipStream_t stream) {
  check_tree_args("treeshap", d, ldx, depth, ntrees);
  if (n_bg < 1 || bw_ld < n_bg) throw std::runtime_error("treeshap: bad background");
  if (n_expl <= 0) return;
  // leaves + split features in LDS when they fit next to the phi table (<= 64 KB in total)
  const size_t base_words = (size_t)d * kTreeThreads + ntrees;
  const size_t tree_words = (size_t)ntrees * (2 << depth);
  const bool lds_leaves = (base_words + tree_words) * sizeof(float) <= 65536 - 1024;
  const size_t lds = (base_words + (lds_leaves ? tree_words : 0)) * sizeof(float);
  dispatch_depth(depth, lds_leaves, [&](auto D, auto in_lds) {
    treeshap_kernel<decltype(D)::value, decltype(in_lds)::value><<<n_expl, kTreeThreads, lds, stream>>>(
        Xs, ldx, d, feat, thr, leaf, ntrees, base_margin, bw, bw_ld, n_bg, f0, phi, fx_out, f0_out);
  });
  check_launch("treeshap");
}

}  // namespace fdx
