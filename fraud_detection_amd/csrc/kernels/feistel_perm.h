// A keyed, stateless pseudo-random permutation of [0, n): 4 Feistel rounds over half-words of
// h = (b + 1) >> 1 bits (2^b >= n, b >= 2) with murmur3's fmix32 as the round function, and cycle
// walking (apply the network again while the value is >= n; a bijection of [0, 2^(2h)) restricted
// this way is a bijection of [0, n), after fewer than 4 rounds on average).  Every element is
// evaluated on its own in registers, ~60 integer operations, so a permuted column needs no sort,
// no index array and no state.  Keys: key[k] = fmix32(seed ^ fmix32(0x9E3779B9 (2 c + 1) + k)) for
// the stream id c.  The construction is split.hip's class permutation on another domain;
// ops/reference_gbdt.py permutation_donors is the numpy oracle of this header.
#pragma once
#include "common.h"

namespace fdx {

__device__ __forceinline__ uint32_t feistel_fmix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x85ebca6bu;
  x ^= x >> 13;
  x *= 0xc2b2ae35u;
  x ^= x >> 16;
  return x;
}

struct FeistelPerm {
  uint64_t n;     // domain size, >= 1
  uint32_t mask;  // half-word mask (h bits)
  int h;
  uint32_t key[4];

  __device__ __forceinline__ void init(uint64_t n_, uint32_t seed, uint32_t stream) {
    n = n_;
    int b = 2;
    while (b < 64 && (1ull << b) < n_) ++b;  // 2^b >= n
    h = (b + 1) >> 1;
    mask = (h >= 32) ? 0xffffffffu : ((1u << h) - 1u);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      key[i] = feistel_fmix32(seed ^ feistel_fmix32(0x9E3779B9u * (2u * stream + 1u) + (uint32_t)i));
  }

  // the image of x < n
  __device__ __forceinline__ uint64_t apply(uint64_t x) const {
    do {
      uint32_t L = (uint32_t)(x >> h), R = (uint32_t)x & mask;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const uint32_t t = L ^ (feistel_fmix32(R ^ key[i]) & mask);
        L = R;
        R = t;
      }
      x = ((uint64_t)L << h) | R;
    } while (x >= n);
    return x;
  }
};

}  // namespace fdx
