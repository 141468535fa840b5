// Partial dependence and ICE curves of the GBDT margin (log-odds): the global counterpart of the
// tree explainers.  For one feature f (or a pair) and every CELL of its grid -- the intervals
// between the ensemble's distinct thresholds on f, plus one cell for "missing" where the model has
// learned default directions -- ice[i][c] is the margin of row i with f placed in cell c and every
// other feature as observed, and pd_q[c] = sum_i llrint((double)ice[i][c] * 2^30) the brute-force
// partial dependence as an exact integer (models/explainers.py has the definitions and the oracle).
//
// A row's directions in a tree are one 32-bit word (tree_explain.h).  Moving f across its cells only
// changes the bits of the nodes that split on f, so per (row, tree) the word is computed ONCE,
// cleared at those nodes (mask[t]) and, per cell, OR-ed with the bits the cell sets there
// (word_a[t][ca] | word_b[t][cb], built by the host): one OR, the register walk tree_leaf<D> and one
// leaf read per (row, tree, cell), against a full walk with three LDS reads per level when the
// table is predicted once per cell.  A tree without a node on f (mask 0) is walked once per row.
//
// MI355X mapping: a workgroup of 4 waves takes 64 rows x 64 cells; lane = row, and wave w owns the
// 16 consecutive cells 16 w .. 16 w + 15 of the tile as 16 fp32 accumulators in registers.  The
// accumulators start at base_margin and take the leaves in tree order, so ice equals gbdt_predict
// on the modified row bit for bit whatever the chunking.  Trees go through LDS in chunks of 32:
// their leaves, the block's premasked direction words [32][64] (built by direction_bits, wave w
// the trees w, w + 4, ..: feat / thr / default_left are wave-uniform reads) and the tile's combined
// override words [32][64].  In the inner loop the direction word is a conflict-free read (lane =
// consecutive address), the override word a broadcast and the leaf a gather inside 2^D consecutive
// floats: no bank conflicts.  29 KiB of LDS at depth 5: five workgroups per CU.
//
// pd_q: every lane rounds its row's value to an integer, the wave adds its 64 rows with shuffles
// and lane 0 issues ONE 64-bit integer atomic per cell and workgroup (a cell belongs to one wave of
// the block).  Integer sums are order free: bitwise reproducible, no float atomics.  ice is written
// only when asked for, 16 consecutive floats per lane.
#include "launchers.h"
#include "tree_explain.h"

namespace fdx {
namespace {

constexpr int kPdRows = 64;                                // rows per workgroup: one per lane
constexpr int kPdWaves = kTreeThreads / kWave;             // 4
constexpr int kPdCellsPerThread = 16;                      // accumulators per thread
constexpr int kPdCells = kPdWaves * kPdCellsPerThread;     // cells per workgroup
constexpr int kPdChunk = 32;                               // trees per LDS chunk
constexpr double kPdScale = 1073741824.0;                  // 2^30
static_assert(kPdRows == kWave, "lane = row");

template <int D>
__global__ __launch_bounds__(kTreeThreads) void tree_pd_kernel(
    const float* __restrict__ Xs, int64_t n, int ldx, int d, const int* __restrict__ feat,
    const float* __restrict__ thr, const float* __restrict__ leaf, const uint8_t* __restrict__ dleft,
    const uint32_t* __restrict__ mask, const uint32_t* __restrict__ word_a, int cells_a,
    const uint32_t* __restrict__ word_b, int cells_b, int T, float base_margin,
    unsigned long long* __restrict__ pd_q, float* __restrict__ ice) {
  constexpr int NI = (1 << D) - 1, NL = 1 << D;
  __shared__ float xs[kPdRows][kCols + 1];       // + 1: lanes read one column of 64 rows
  __shared__ uint32_t xw[kPdChunk][kPdRows];     // direction words, cleared at the overridden nodes
  __shared__ uint32_t ov[kPdChunk][kPdCells];    // what the tile's cells set at those nodes
  __shared__ float lf[kPdChunk * NL];
  __shared__ uint32_t mk[kPdChunk];
  const int tid = threadIdx.x, lane = lane_id();
  const int w = __builtin_amdgcn_readfirstlane(wave_id());
  const int64_t r0 = (int64_t)blockIdx.x * kPdRows;
  const int C = cells_a * cells_b;
  const int c0 = blockIdx.y * kPdCells;

  for (int i = tid; i < kPdRows * kCols; i += kTreeThreads) {
    const int row = i / kCols, col = i % kCols;
    const int64_t r = r0 + row;
    xs[row][col] = (r < n && col < d) ? Xs[r * ldx + col] : 0.0f;
  }
  float acc[kPdCellsPerThread];
#pragma unroll
  for (int j = 0; j < kPdCellsPerThread; ++j) acc[j] = base_margin;

  for (int t0 = 0; t0 < T; t0 += kPdChunk) {
    const int nt = min(kPdChunk, T - t0);
    __syncthreads();  // xs is written; the previous chunk is read
    for (int i = tid; i < nt * NL; i += kTreeThreads) lf[i] = leaf[(int64_t)t0 * NL + i];
    if (tid < nt) mk[tid] = mask[t0 + tid];
    for (int i = tid; i < nt * kPdCells; i += kTreeThreads) {
      const int t = i / kPdCells, j = i % kPdCells;
      const int cell = c0 + j;
      uint32_t u = 0;  // a cell past the grid walks like cell "nothing set" and is never stored
      if (cell < C) {
        const int ca = cell / cells_b, cb = cell - ca * cells_b;
        u = word_a[(int64_t)(t0 + t) * cells_a + ca];
        if (word_b != nullptr) u |= word_b[(int64_t)(t0 + t) * cells_b + cb];
      }
      ov[t][j] = u;
    }
    for (int t = w; t < nt; t += kPdWaves) {
      const int64_t tt = t0 + t;
      const uint32_t bits =
          direction_bits<NI>(xs[lane], feat + tt * NI, thr + tt * NI, dleft != nullptr ? dleft + tt * NI : nullptr);
      xw[t][lane] = bits & ~mask[tt];
    }
    __syncthreads();
    for (int t = 0; t < nt; ++t) {
      const uint32_t b = xw[t][lane];
      const float* l = lf + t * NL;
      if (__builtin_amdgcn_readfirstlane(mk[t]) == 0u) {  // no node on the features: one walk per row
        const float v = l[tree_leaf<D>(b)];
#pragma unroll
        for (int j = 0; j < kPdCellsPerThread; ++j) acc[j] += v;
      } else {
        const uint32_t* o = ov[t] + w * kPdCellsPerThread;
#pragma unroll
        for (int j = 0; j < kPdCellsPerThread; ++j) acc[j] += l[tree_leaf<D>(b | o[j])];
      }
    }
  }

  const int64_t r = r0 + lane;
  const bool ok = r < n;
#pragma unroll
  for (int j = 0; j < kPdCellsPerThread; ++j) {
    const int cell = c0 + w * kPdCellsPerThread + j;  // wave-uniform
    if (cell >= C) break;
    long long q = ok ? llrint((double)acc[j] * kPdScale) : 0ll;
    q = wave_sum(q);
    if (lane == 0 && q != 0ll) atomicAdd(pd_q + cell, (unsigned long long)q);
    if (ice != nullptr && ok) ice[r * C + cell] = acc[j];
  }
}

}  // namespace

int tree_pd_rows_per_block() { return kPdRows; }
int tree_pd_chunk_trees() { return kPdChunk; }
int tree_pd_cells_per_block() { return kPdCells; }

void launch_tree_pd(const float* Xs, int64_t n, int ldx, int d, const int* feat, const float* thr,
                    const float* leaf, const uint8_t* dleft, const uint32_t* mask, const uint32_t* word_a,
                    int cells_a, const uint32_t* word_b, int cells_b, int ntrees, int depth, float base_margin,
                    int64_t* pd_q, float* ice, hipStream_t stream) {
  check_tree_args("tree_pd", d, ldx, depth, ntrees);
  if (n < 0) throw std::runtime_error("tree_pd: negative row count");
  if (cells_a < 1 || cells_b < 1 || (int64_t)cells_a * cells_b > kTreePdMaxCells)
    throw std::runtime_error("tree_pd: 1 <= cells <= 65536");
  if (word_b == nullptr && cells_b != 1) throw std::runtime_error("tree_pd: cells_b without word_b");
  if (mask == nullptr || word_a == nullptr || pd_q == nullptr) throw std::runtime_error("tree_pd: null argument");
  const int C = cells_a * cells_b;
  if (hipMemsetAsync(pd_q, 0, (size_t)C * sizeof(int64_t), stream) != hipSuccess)
    throw std::runtime_error("tree_pd: clearing the sums failed");
  if (n == 0) return;
  const int64_t row_tiles = (n + kPdRows - 1) / kPdRows;
  if (row_tiles > 2147483647ll) throw std::runtime_error("tree_pd: too many rows for one launch");
  const dim3 grid((unsigned)row_tiles, (unsigned)((C + kPdCells - 1) / kPdCells));
  auto* out = reinterpret_cast<unsigned long long*>(pd_q);
  dispatch_depth(depth, false, [&](auto D, auto) {
    tree_pd_kernel<decltype(D)::value><<<grid, kTreeThreads, 0, stream>>>(
        Xs, n, ldx, d, feat, thr, leaf, dleft, mask, word_a, cells_a, word_b, cells_b, ntrees, base_margin, out, ice);
  });
  check_launch("tree_pd");
}

}  // namespace fdx
