// Philox4x32-10 (Salmon et al., "Parallel Random Numbers: As Easy as 1, 2, 3"):
// the counter-based generator of the walks (sampler.hip, ppr_topk.hip,
// n2v.hip).  The four output words depend on (key, counter) only; the CPU twin
// is oracle/'s orc_philox.
#pragma once
#include "common.h"

namespace ps {

__device__ __forceinline__ uint4 philox10(uint64_t key, uint4 c) {
  uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    uint64_t p0 = (uint64_t)0xD2511F53u * c.x;
    uint64_t p1 = (uint64_t)0xCD9E8D57u * c.z;
    uint32_t n0 = (uint32_t)(p1 >> 32) ^ c.y ^ k0;
    uint32_t n2 = (uint32_t)(p0 >> 32) ^ c.w ^ k1;
    c = make_uint4(n0, (uint32_t)p1, n2, (uint32_t)p0);
    if (r < 9) {
      k0 += 0x9E3779B9u;
      k1 += 0xBB67AE85u;
    }
  }
  return c;
}

}  // namespace ps
