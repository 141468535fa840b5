// One column of the scaler finalize: mean / var / scale from (possibly all-reduced) shifted sums.
// Shared by scaler_finalize_kernel (scaler.hip) and the fused k-NN prep (knn.hip), which
// recomputes the statistics in every block's prologue instead of waiting for a finalize launch:
// one body, so both give the same bits.  Keep it free of fp-contract pragmas (the callers' own
// pragmas do not reach into it).
#pragma once
#include "common.h"

namespace fdx {

struct ScalerCol {
  double mean, var, scale;  // [c] of mean64 / var64 / scale64
  float mean32, inv32;
  double aff_c, aff_inv;    // aff[c], aff[32 + c]
};

// sums: [nparts][64] rows (shifted sums | shifted squares), summed here in order; n < 0: the row
// count rides in slot 31.  colscale (nullable): fp8 rows store v = s * k, folded into aff.
__device__ __forceinline__ ScalerCol scaler_finalize_col(const double* __restrict__ sums, double n,
                                                         const float* __restrict__ pivot, int d,
                                                         const float* __restrict__ colscale, int nparts,
                                                         int c) {
  // nparts > 1: `sums` holds the first-level reduce's [nparts][64] rows, summed here in order
  // (the order of the second-level reduce launch this replaces: bit-identical sums)
  double s1 = 0.0, s2 = 0.0, sn = 0.0;
  for (int p = 0; p < nparts; ++p) {
    s1 += sums[64 * p + c];
    s2 += sums[64 * p + 32 + c];
    sn += sums[64 * p + kCols - 1];
  }
  // n < 0: the (all-reduced) row count rides in the unused slot sums[31] (one collective for the
  // sums and the count, and no host round trip for n)
  if (n < 0.0) n = sn;
  ScalerCol o;
  if (c < d) {
    const double m = s1 / n;
    const double mean = (double)pivot[c] + m;
    double var = s2 / n - m * m;
    if (var < 0.0) var = 0.0;
    const double eps = 2.220446049250313e-16;
    const double ub = n * eps * var + (n * mean * eps) * (n * mean * eps);
    const double scale = (var <= ub) ? 1.0 : sqrt(var);
    o.mean = mean;
    o.var = var;
    o.scale = scale;
    o.mean32 = (float)mean;
    o.inv32 = (float)(1.0 / scale);
    // mean - pivot, without the cancellation of (pivot + m) - pivot; fp8 rows store v = s * k
    // (colscale), so z = (s - m) / scale = (v - k m) * (1 / (scale k))
    const double k = colscale ? (double)colscale[c] : 1.0;
    o.aff_c = m * k;
    o.aff_inv = 1.0 / scale / k;
  } else {
    o.mean = 0.0; o.var = 0.0; o.scale = 1.0;
    o.mean32 = 0.0f; o.inv32 = 0.0f;
    o.aff_c = 0.0;
    o.aff_inv = 1.0;
  }
  return o;
}

}  // namespace fdx
