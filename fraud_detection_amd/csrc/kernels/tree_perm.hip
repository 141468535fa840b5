// Permutation feature importance of the GBDT margin: the margins of every row with ONE feature
// taken from another row.  Column j = (feature f_j, repeat r_j) gives row i the value
// Xs[donor_j(i)][f_j], donor_j the keyed Feistel permutation of the rows with stream id
// 32 r_j + f_j (feistel_perm.h), and leaves everything else as observed; out[j][i] is that row's
// margin.  f_j = -1 substitutes nothing: the baseline.  The metric kernels (AUC, average precision,
// log-loss) then score each column; ops/perm_importance.py drives both.
//
// A row's directions in a tree are one 32-bit word (tree_explain.h).  Replacing feature f only
// changes the bits of the nodes that split on f, so per (row, tree) the word is computed ONCE, and
// per (tree, column) the host's mask word fmask[t][f] (the heap-node bits of the nodes on f) says
// what to do: 0 -- the tree has no node on f, every column of that kind adds the row's own leaf,
// found once per (row, tree); otherwise the walk takes, at heap node k, the donor comparison
// !(v < thr[t][k]) (a NaN v goes left where default_left is set) when bit k of the mask is set and
// the row's own bit when it is not.  No per-level feature gather, no permuted copy of the table.
//
// MI355X mapping (tree_pd.hip's): a workgroup of 4 waves takes 64 rows x 64 columns; lane = row, and
// wave w owns the 16 consecutive columns 16 w .. 16 w + 15 of the tile as 16 fp32 accumulators.  Its
// 16 donor values are one gathered global read each, kept in registers for the whole kernel.  The
// accumulators start at base_margin and take the leaves in tree order, so out[j] equals
// gbdt_predict on the explicitly permuted table bit for bit whatever the chunking.  Trees go
// through LDS in chunks of 32: leaves, thresholds, default_left bytes, the block's direction words
// [32][64] (direction_bits, wave w the trees w, w + 4, ..) and the tile's mask words [32][64].  The
// column's feature is wave-uniform, so the mask word is a broadcast read made scalar and the branch
// on it is wave-uniform; the direction word is a conflict-free read (lane = consecutive address);
// threshold, default_left and leaf are gathers inside one tree's 2^D consecutive words: distinct
// addresses fall on distinct banks and equal ones broadcast.  34 KiB of LDS at depth 5: four
// workgroups per CU.  The output is column-major [ncols][n]: lanes write consecutive addresses and a
// column is a contiguous score vector.  No atomics: every output element has one writer.
#include "feistel_perm.h"
#include "launchers.h"
#include "tree_explain.h"

namespace fdx {
namespace {

constexpr int kPermRows = 64;                                  // rows per workgroup: one per lane
constexpr int kPermWaves = kTreeThreads / kWave;               // 4
constexpr int kPermColsPerThread = 16;                         // accumulators per thread
constexpr int kPermCols = kPermWaves * kPermColsPerThread;     // columns per workgroup
constexpr int kPermChunk = 32;                                 // trees per LDS chunk
static_assert(kPermRows == kWave, "lane = row");

// DL: the ensemble has default directions (dleft != nullptr)
template <int D, bool DL>
__global__ __launch_bounds__(kTreeThreads) void tree_perm_kernel(
    const float* __restrict__ Xs, int64_t n, int ldx, int d, const int* __restrict__ feat,
    const float* __restrict__ thr, const float* __restrict__ leaf, const uint8_t* __restrict__ dleft,
    const uint32_t* __restrict__ fmask, int T, float base_margin, const int* __restrict__ col_feat,
    const int* __restrict__ col_rep, int ncols, uint32_t seed, float* __restrict__ out) {
  constexpr int NI = (1 << D) - 1, NL = 1 << D;
  __shared__ float xs[kPermRows][kCols + 1];       // + 1: lanes read one column of 64 rows
  __shared__ uint32_t xw[kPermChunk][kPermRows];   // the rows' direction words
  __shared__ uint32_t cm[kPermChunk][kPermCols];   // fmask[t][f_j] of the tile's columns
  __shared__ float lf[kPermChunk * NL];
  __shared__ float th[kPermChunk * NI];
  __shared__ uint8_t dl[DL ? kPermChunk * NI : 1];
  const int tid = threadIdx.x, lane = lane_id();
  const int w = __builtin_amdgcn_readfirstlane(wave_id());
  const int64_t r0 = (int64_t)blockIdx.x * kPermRows;
  const int c0 = blockIdx.y * kPermCols;
  const int64_t r = r0 + lane;
  const bool ok = r < n;

  for (int i = tid; i < kPermRows * kCols; i += kTreeThreads) {
    const int row = i / kCols, col = i % kCols;
    const int64_t rr = r0 + row;
    xs[row][col] = (rr < n && col < d) ? Xs[rr * ldx + col] : 0.0f;
  }
  // the wave's donor values: column j of row r reads feature f_j of row donor_j(r)
  float v[kPermColsPerThread], acc[kPermColsPerThread];
#pragma unroll
  for (int j = 0; j < kPermColsPerThread; ++j) {
    const int col = c0 + w * kPermColsPerThread + j;  // wave-uniform
    acc[j] = base_margin;
    v[j] = 0.0f;
    const int f = col < ncols ? col_feat[col] : -1;
    if (f >= 0 && f < d) {
      FeistelPerm P;
      P.init((uint64_t)n, seed, 32u * (uint32_t)col_rep[col] + (uint32_t)f);
      if (ok) v[j] = Xs[(int64_t)P.apply((uint64_t)r) * ldx + f];
    }
  }

  for (int t0 = 0; t0 < T; t0 += kPermChunk) {
    const int nt = min(kPermChunk, T - t0);
    __syncthreads();  // xs is written; the previous chunk is read
    for (int i = tid; i < nt * NL; i += kTreeThreads) lf[i] = leaf[(int64_t)t0 * NL + i];
    for (int i = tid; i < nt * NI; i += kTreeThreads) {
      th[i] = thr[(int64_t)t0 * NI + i];
      if constexpr (DL) dl[i] = dleft[(int64_t)t0 * NI + i];
    }
    for (int i = tid; i < nt * kPermCols; i += kTreeThreads) {
      const int t = i / kPermCols, col = c0 + i % kPermCols;
      const int f = col < ncols ? col_feat[col] : -1;  // a column past the list walks like the baseline
      cm[t][i % kPermCols] = (f >= 0 && f < d) ? fmask[(int64_t)(t0 + t) * kCols + f] : 0u;
    }
    for (int t = w; t < nt; t += kPermWaves) {
      const int64_t tt = t0 + t;
      xw[t][lane] = direction_bits<NI>(xs[lane], feat + tt * NI, thr + tt * NI, DL ? dleft + tt * NI : nullptr);
    }
    __syncthreads();
    for (int t = 0; t < nt; ++t) {
      const uint32_t b = xw[t][lane];
      const float* l = lf + t * NL;
      const float* tht = th + t * NI;  // heap node k at k - 1
      [[maybe_unused]] const uint8_t* dlt = dl + t * NI;
      const float own = l[tree_leaf<D>(b)];
      const uint32_t* cmt = cm[t] + w * kPermColsPerThread;
#pragma unroll
      for (int j = 0; j < kPermColsPerThread; ++j) {
        const uint32_t m = __builtin_amdgcn_readfirstlane(cmt[j]);
        if (m == 0u) {  // no node on the column's feature
          acc[j] += own;
        } else {
          const float x = v[j];
          int node = 1;
#pragma unroll
          for (int lv = 0; lv < D; ++lv) {
            bool right = !(x < tht[node - 1]);
            if constexpr (DL) right = right && !(x != x && dlt[node - 1] != 0);
            const uint32_t bit = ((m >> node) & 1u) ? (uint32_t)right : ((b >> node) & 1u);
            node = (node << 1) | (int)bit;
          }
          acc[j] += l[node - NL];
        }
      }
    }
  }

  if (ok) {
#pragma unroll
    for (int j = 0; j < kPermColsPerThread; ++j) {
      const int col = c0 + w * kPermColsPerThread + j;  // wave-uniform
      if (col >= ncols) break;
      out[(int64_t)col * n + r] = acc[j];
    }
  }
}

}  // namespace

int tree_perm_rows_per_block() { return kPermRows; }
int tree_perm_chunk_trees() { return kPermChunk; }
int tree_perm_cols_per_block() { return kPermCols; }

void launch_tree_perm(const float* Xs, int64_t n, int ldx, int d, const int* feat, const float* thr,
                      const float* leaf, const uint8_t* dleft, const uint32_t* fmask, int ntrees, int depth,
                      float base_margin, const int* col_feat, const int* col_rep, int ncols, uint32_t seed,
                      float* out, hipStream_t stream) {
  check_tree_args("tree_perm", d, ldx, depth, ntrees);
  if (n < 0) throw std::runtime_error("tree_perm: negative row count");
  if (ncols < 1 || ncols > kTreePermMaxCols) throw std::runtime_error("tree_perm: 1 <= columns <= 2^20");
  if (fmask == nullptr || col_feat == nullptr || col_rep == nullptr || out == nullptr)
    throw std::runtime_error("tree_perm: null argument");
  if (n == 0) return;
  if (Xs == nullptr) throw std::runtime_error("tree_perm: null rows");
  const int64_t row_tiles = (n + kPermRows - 1) / kPermRows;
  if (row_tiles > 2147483647ll) throw std::runtime_error("tree_perm: too many rows for one launch");
  const dim3 grid((unsigned)row_tiles, (unsigned)((ncols + kPermCols - 1) / kPermCols));
  dispatch_depth(depth, dleft != nullptr, [&](auto D, auto DL) {
    tree_perm_kernel<decltype(D)::value, decltype(DL)::value><<<grid, kTreeThreads, 0, stream>>>(
        Xs, n, ldx, d, feat, thr, leaf, dleft, fmask, ntrees, base_margin, col_feat, col_rep, ncols, seed, out);
  });
  check_launch("tree_perm");
}

}  // namespace fdx
