// Node covers of a tree ensemble over a set of fp32 rows: cover[t][k] for heap node k = 1 ..
// 2^(D+1) - 1 of tree t (index 0 unused and 0), the quantity xgboost stores per node as sum_hess
// and path-dependent TreeSHAP (treeshap_path.hip) weighs a node's children by.
//
//   kind 0 "count":    rows that reach the node
//   kind 1 "hessian":  sum over those rows of h_q = llrint(p (1 - p) 2^30), p = sigmoid((double)m),
//                      m the fp32 margin of the row BEFORE tree t: float(base_margin) plus the leaves
//                      of trees 0 .. t-1 added in tree order in fp32 -- gbdt_predict's value for
//                      n_trees = t.  The sigmoid is the gradient kernels' fp64 expression.
//
// Both are int64 sums: order-free, bitwise reproducible, no float atomics anywhere.  Routing is
// gbdt_predict's (right iff !(x < thr); a NaN goes left iff the node's dleft byte is set; a
// pass-through node, feat -1, goes left).  Only leaves are accumulated; tree_cover_finalize_kernel
// makes every internal node the exact integer sum of its two children.
//
// MI355X mapping: one thread per row, the row in LDS (dynamic feature index without scratch), the
// running margin in a register, trees in sequence.  A launch covers one CHUNK of trees: their
// nodes and an int64 accumulator [chunk][2^D] sit in LDS for the block's whole life, the block
// strides over row tiles and flushes its non-zero sums once with 64-bit global atomics.  When the
// ensemble needs several chunks the launcher runs them in tree order and the hessian kind carries
// every row's margin from chunk to chunk in a caller-provided fp32 workspace, so the LDS sums
// never flush more than once per block and chunk.  Every row issues its own 64-bit LDS atomic;
// lanes that meet on one leaf serialise, and that is accepted: adding one wave-reduced value when
// a wave's 64 rows agree on the leaf measured slower on random rows (0.89 against 0.76 ms for 1M
// rows x 100 trees, counts) and no faster on identical ones (profiles/treeshap_path/README.md).
#include "common.h"
#include "launchers.h"

namespace fdx {
namespace {

constexpr int kCovThreads = 256;
constexpr int kCovMaxFeat = 30;
constexpr int kCovDefaultLeft = 0x100;
constexpr int kCovLdsBytes = 32768 - 1024;  // trees + accumulators of a chunk (rows take 31 KiB more)
constexpr double kCovScale = 1073741824.0;  // 2^30

__host__ __device__ constexpr int cov_tree_bytes(int depth) {
  // per tree: feat words + thresholds (2 (2^D - 1) floats), leaves (2^D floats), int64 sums (2^D)
  return (2 * ((1 << depth) - 1) + (1 << depth)) * 4 + (1 << depth) * 8;
}

template <bool HESS>
__global__ __launch_bounds__(kCovThreads) void tree_cover_kernel(
    const float* __restrict__ X, int64_t n, int ld, int d, const int* __restrict__ feat,
    const float* __restrict__ thr, const float* __restrict__ leaf, const uint8_t* __restrict__ dleft, int t0,
    int nt, int depth, float base_margin, const float* margin_in, float* margin_out,  // may be one buffer
    unsigned long long* __restrict__ out) {
  __shared__ float xr[kCovThreads][kCovMaxFeat + 1];
  extern __shared__ __attribute__((aligned(16))) unsigned char cov_dyn[];
  const int ni = (1 << depth) - 1, nl = 1 << depth;
  const int per_tree = 2 * ni + nl;
  unsigned long long* acc = reinterpret_cast<unsigned long long*>(cov_dyn);  // [nt][nl]
  float* tl = reinterpret_cast<float*>(acc + (size_t)nt * nl);               // [nt][per_tree]
  const int tid = threadIdx.x;
  for (int i = tid; i < nt * nl; i += kCovThreads) acc[i] = 0ull;
  for (int i = tid; i < nt * ni; i += kCovThreads) {
    const int t = i / ni, k = i % ni;
    int fw = feat[(int64_t)(t0 + t) * ni + k];
    if (dleft != nullptr && fw >= 0 && dleft[(int64_t)(t0 + t) * ni + k] != 0) fw |= kCovDefaultLeft;
    tl[t * per_tree + k] = __int_as_float(fw);
    tl[t * per_tree + ni + k] = thr[(int64_t)(t0 + t) * ni + k];
  }
  for (int i = tid; i < nt * nl; i += kCovThreads) {
    const int t = i / nl, k = i % nl;
    tl[t * per_tree + 2 * ni + k] = leaf[(int64_t)(t0 + t) * nl + k];
  }
  __syncthreads();
  const int64_t ntiles = (n + kCovThreads - 1) / kCovThreads;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t r = tile * kCovThreads + tid;
    const bool ok = r < n;
    // a thread reads and writes its own row of xr only: no barrier between tiles
    for (int j = 0; j < d; ++j) xr[tid][j] = ok ? X[r * ld + j] : 0.0f;
    float m = 0.0f;
    if constexpr (HESS) m = (margin_in != nullptr && ok) ? margin_in[r] : base_margin;
    for (int t = 0; t < nt; ++t) {
      const float* T = tl + t * per_tree;
      int node = 0;
      for (int l = 0; l < depth; ++l) {
        const int fw = __float_as_int(T[node]);
        bool right = false;
        if (fw >= 0) {
          const float x = xr[tid][fw & 0xff];
          right = !(x < T[ni + node]) && !(x != x && (fw & kCovDefaultLeft) != 0);
        }
        node = 2 * node + 1 + (right ? 1 : 0);
      }
      const int lf = node - ni;
      unsigned long long v = ok ? 1ull : 0ull;
      if constexpr (HESS) {
        if (ok) {
          const double p = 1.0 / (1.0 + exp(-(double)m));
          v = (unsigned long long)llrint(p * (1.0 - p) * kCovScale);
        }
        m += T[2 * ni + lf];
      }
      if (v != 0ull) atomicAdd(acc + t * nl + lf, v);  // rows past n carry v = 0
    }
    if constexpr (HESS) {
      if (margin_out != nullptr && ok) margin_out[r] = m;
    }
  }
  __syncthreads();
  // one order-free integer flush per block: leaf l of tree t0 + t is heap node 2^D + l
  for (int i = tid; i < nt * nl; i += kCovThreads) {
    const unsigned long long s = acc[i];
    if (s != 0ull) atomicAdd(out + (int64_t)(t0 + i / nl) * (2 * nl) + nl + (i % nl), s);
  }
}

// internal node k = its two children, bottom up; slot 0 stays 0.  One thread per tree.
__global__ void tree_cover_finalize_kernel(unsigned long long* __restrict__ out, int ntrees, int depth) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= ntrees) return;
  const int nl = 1 << depth;
  unsigned long long* c = out + (int64_t)t * (2 * nl);
  for (int k = nl - 1; k >= 1; --k) c[k] = c[2 * k] + c[2 * k + 1];
  c[0] = 0ull;
}

}  // namespace

int tree_cover_chunk_trees(int depth) {
  if (depth < 1 || depth > 8) throw std::runtime_error("tree_cover: depth must be in [1, 8]");
  return kCovLdsBytes / cov_tree_bytes(depth);
}

void launch_tree_cover(const float* X, int64_t n, int ld, int d, const int* feat, const float* thr,
                       const float* leaf, const uint8_t* dleft, int ntrees, int depth, float base_margin,
                       int kind, float* margin_ws, int64_t* cover, hipStream_t stream) {
  if (depth < 1 || depth > 8) throw std::runtime_error("tree_cover: depth must be in [1, 8]");
  if (d < 1 || d > kCovMaxFeat) throw std::runtime_error("tree_cover: at most 30 features");
  if (ld < d) throw std::runtime_error("tree_cover: row stride below the feature count");
  if (ntrees < 1) throw std::runtime_error("tree_cover: at least one tree");
  if (n < 0) throw std::runtime_error("tree_cover: negative row count");
  if (kind != 0 && kind != 1) throw std::runtime_error("tree_cover: kind must be 0 (count) or 1 (hessian)");
  const int chunk = tree_cover_chunk_trees(depth);
  const bool chunked = ntrees > chunk;
  if (kind == 1 && chunked && n > 0 && margin_ws == nullptr)
    throw std::runtime_error("tree_cover: the hessian kind over several tree chunks needs a margin workspace");
  const int nl = 1 << depth;
  auto* out = reinterpret_cast<unsigned long long*>(cover);
  if (hipMemsetAsync(out, 0, (size_t)ntrees * 2 * nl * sizeof(unsigned long long), stream) != hipSuccess)
    throw std::runtime_error("tree_cover: clearing the cover table failed");
  if (n == 0) return;
  const int grid = capped_grid(n, kCovThreads, 2 * device_cu_count());
  for (int t0 = 0; t0 < ntrees; t0 += chunk) {
    const int nt = ntrees - t0 < chunk ? ntrees - t0 : chunk;
    const size_t lds = (size_t)nt * cov_tree_bytes(depth);
    if (kind == 1) {
      tree_cover_kernel<true><<<grid, kCovThreads, lds, stream>>>(
          X, n, ld, d, feat, thr, leaf, dleft, t0, nt, depth, base_margin, t0 > 0 ? margin_ws : nullptr,
          (chunked && t0 + nt < ntrees) ? margin_ws : nullptr, out);
    } else {
      tree_cover_kernel<false><<<grid, kCovThreads, lds, stream>>>(X, n, ld, d, feat, thr, leaf, dleft, t0, nt,
                                                                   depth, base_margin, nullptr, nullptr, out);
    }
    check_launch("tree_cover");
  }
  tree_cover_finalize_kernel<<<(ntrees + 255) / 256, 256, 0, stream>>>(out, ntrees, depth);
  check_launch("tree_cover_finalize");
}

}  // namespace fdx
