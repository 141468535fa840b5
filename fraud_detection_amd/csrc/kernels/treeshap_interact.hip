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
#include "common.h"
#include "launchers.h"

namespace fdx {
namespace {

constexpr int kTIThreads = 256;
constexpr int kTIMaxTrees = 2048;
constexpr int kTIMaxDepth = 5;
// The per-tree constants go to LDS only while a workgroup's LDS stays within 31 KiB: five
// workgroups then share a CU's 160 KiB, as many as the depth-5 kernel's registers allow, and the
// resident form costs the same as the streamed one.  Beyond that it lowers the occupancy and
// loses: 100 trees at d = 30 (55 KiB, two workgroups per CU) took 0.175 ms resident against
// 0.128 ms streamed for 1000 rows (profiles/treeshap_interactions/README.md).
constexpr int kTILdsBytes = 32768 - 1024;
constexpr int kTIFracBits = 46;

typedef unsigned long long ti_u64;

__device__ __forceinline__ float ti_fact(int n) {
  float r = 1.0f;
  for (int i = 2; i <= n; ++i) r *= (float)i;
  return r;
}

template <int D>
__device__ __forceinline__ float ti_tree_margin(uint32_t bits, const float* __restrict__ lf) {
  int node = 1;
#pragma unroll
  for (int l = 0; l < D; ++l) node = (node << 1) | (int)((bits >> node) & 1u);
  return lf[node - (1 << D)];
}

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
  float df[D];  // o_i - z_i
#pragma unroll
  for (int i = 0; i < D; ++i) df[i] = o[i] - z[i];
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
    ti_add(acc + fs[i], v * df[i] * W, up);
  }
  if constexpr (D >= 2) {
    if (m < 2) return;
    const float* w2 = w2tab + m * 6;
#pragma unroll
    for (int i = 0; i < D; ++i) {
#pragma unroll
      for (int j = i + 1; j < D; ++j) {
        if (fs[i] < 0 || fs[j] < 0) continue;
        // c[s]: coefficient of y^s in prod_{k != i, j} (z_k + o_k y), D - 2 factors
        float c[D - 1];
        c[0] = 1.0f;
#pragma unroll
        for (int s = 1; s < D - 1; ++s) c[s] = 0.0f;
#pragma unroll
        for (int k = 0; k < D; ++k) {
          if (k == i || k == j) continue;
#pragma unroll
          for (int s = D - 2; s >= 1; --s) c[s] = c[s] * z[k] + c[s - 1] * o[k];
          c[0] = c[0] * z[k];
        }
        float W = 0.0f;
#pragma unroll
        for (int s = 0; s < D - 1; ++s) W += w2[s] * c[s];  // w2[s] = 0 for s >= m - 1, as c[s]
        const int a = fs[i] < fs[j] ? fs[i] : fs[j], b = fs[i] < fs[j] ? fs[j] : fs[i];
        ti_add(acc + d + ((b * (b - 1)) >> 1) + a, v * df[i] * df[j] * W, up);
      }
    }
  }
}

template <int D, bool TREE_LDS>
__global__ __launch_bounds__(kTIThreads) void treeshap_interact_kernel(
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
  float* lfs = reinterpret_cast<float*>(xw + T);
  int* fts = reinterpret_cast<int*>(lfs + (TREE_LDS ? T * NL : 0));
  float* frs = reinterpret_cast<float*>(fts + (TREE_LDS ? T * NI : 0));
  __shared__ float xs[32];
  __shared__ float wtab[36];   // [m][s], m = 1 .. 5, s < m: s! (m - s - 1)! / m!
  __shared__ float w2tab[36];  // [m][s], m = 2 .. 5, s < m - 1: s! (m - s - 2)! / (2 (m - 1)!)
  __shared__ float red[kTIThreads / kWave];
  __shared__ long long diag[32];
  const int e = blockIdx.x, tid = threadIdx.x;
  if (tid < 32) xs[tid] = tid < d ? Xs[(int64_t)e * ldx + tid] : 0.0f;
  if (tid < 36) {
    const int m = tid / 6, s = tid % 6;
    wtab[tid] = (m >= 1 && s < m) ? ti_fact(s) * ti_fact(m - s - 1) / ti_fact(m) : 0.0f;
    w2tab[tid] = (m >= 2 && s < m - 1) ? ti_fact(s) * ti_fact(m - s - 2) / (2.0f * ti_fact(m - 1)) : 0.0f;
  }
  for (int i = tid; i < ncell; i += kTIThreads) acc[i] = 0ull;
  if constexpr (TREE_LDS) {
    for (int i = tid; i < T * NL; i += kTIThreads) lfs[i] = leaf[i];
    for (int i = tid; i < T * NI; i += kTIThreads) fts[i] = feat[i];
    for (int i = tid; i < T * 2 * NL; i += kTIThreads) frs[i] = frac[i];
  }
  __syncthreads();
  // x's direction bits per tree (bit n + 1: internal node n sends x right; a NaN goes left where
  // the node's default_left byte is set; pass-through: left)
  for (int t = tid; t < T; t += kTIThreads) {
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
  const double up = ldexp(1.0, kTIFracBits - e2), down = ldexp(1.0, e2 - kTIFracBits);
  const int npairs = T * NL;
  for (int p = tid; p < npairs; p += kTIThreads) {
    const int t = p >> D, l = p & (NL - 1);
    leaf_interactions<D>(l, LF[p], xw[t], FT + t * NI, FR + t * 2 * NL, wtab, w2tab, d, up, acc);
  }
  // f(x): this thread's trees, then a fixed-order block sum (treeshap_path.hip's, bit for bit)
  float mx = 0.0f;
  for (int t = tid; t < T; t += kTIThreads) mx += ti_tree_margin<D>(xw[t], LF + t * NL);
  mx = wave_sum(mx);
  if (lane_id() == 0) red[wave_id()] = mx;
  __syncthreads();
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
  for (int idx = tid; idx < d * d; idx += kTIThreads) {
    const int i = idx / d, j = idx - i * d;
    const int a = i < j ? i : j, b = i < j ? j : i;
    const long long q = i == j ? diag[i] : cells[d + ((b * (b - 1)) >> 1) + a];
    out[idx] = (double)q * down;  // one cell feeds [i, j] and [j, i]: symmetric bit for bit
  }
  if (tid == 0) {
    float m = base_margin;
    for (int w = 0; w < kTIThreads / kWave; ++w) m += red[w];
    fx_out[e] = m;
    f0_out[e] = f0;
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
  if (d < 1 || d > 30) throw std::runtime_error("treeshap_interactions: 1 <= d <= 30");
  if (ldx < d) throw std::runtime_error("treeshap_interactions: row stride below the feature count");
  if (depth < 1 || depth > kTIMaxDepth) throw std::runtime_error("treeshap_interactions: depth must be in [1, 5]");
  if (ntrees < 1 || ntrees > kTIMaxTrees) throw std::runtime_error("treeshap_interactions: 1 <= trees <= 2048");
  if (leaf_exp < -160 || leaf_exp > 128)
    throw std::runtime_error("treeshap_interactions: leaf exponent outside fp32's range");
  if (n_expl <= 0) return;
  const bool in_lds = !stream_trees && treeshap_interactions_trees_in_lds(d, ntrees, depth);
  const size_t lds = ti_base_bytes(d, ntrees) + (in_lds ? ti_tree_bytes(ntrees, depth) : 0);
#define FDX_TI(D_, LL)                                                                                      \
  treeshap_interact_kernel<D_, LL><<<n_expl, kTIThreads, lds, stream>>>(                                    \
      Xs, ldx, d, feat, thr, leaf, frac, dleft, ntrees, base_margin, f0, leaf_exp, inter, phi, fx_out, f0_out)
#define FDX_TI_D(D_)                          \
  do {                                        \
    if (in_lds) FDX_TI(D_, true);             \
    else FDX_TI(D_, false);                   \
  } while (0)
  switch (depth) {
    case 1: FDX_TI_D(1); break;
    case 2: FDX_TI_D(2); break;
    case 3: FDX_TI_D(3); break;
    case 4: FDX_TI_D(4); break;
    default: FDX_TI_D(5); break;
  }
#undef FDX_TI_D
#undef FDX_TI
  check_launch("treeshap_interactions");
}

}  // namespace fdx
