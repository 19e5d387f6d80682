// What the host entry (rank_host.cpp) and the device entry (rank.hip) of
// sedx_average_precision share: the sort key, the sizes that fix the
// summation order, the argument checks and the per-thread message.  Plain
// C++ (rank_host.cpp also builds without HIP, under the sanitizers).
#ifndef SEDX_RANK_H
#define SEDX_RANK_H

#include <stdint.h>

#include "../../include/sedx.h"

#if defined(__HIPCC__)
#define SEDX_RANK_HD __host__ __device__ inline
#else
#define SEDX_RANK_HD inline
#endif

namespace sedx {

// keys one workgroup handles per radix pass (sedx_rank_tile): 256 threads, 4
// wavefronts of 16 rounds of 64 keys
constexpr int64_t RANK_TILE = 4096;
// the float64 sum of the terms: a fixed tree over RANK_SUM_CHUNK consecutive
// terms, the same tree over RANK_SUM_CHUNK consecutive chunk sums, then the
// second-level sums in ascending order (include/sedx.h)
constexpr int RANK_SUM_CHUNK = 64;
// classes are ranked in groups of at most RANK_GROUP_ELEMS / M (at least one)
constexpr int64_t RANK_GROUP_ELEMS = int64_t(1) << 22;

// Order-preserving key of a float32 bit pattern, complemented: ascending keys
// are descending scores.  -0.0 folds into +0.0; denormals keep their bits.
SEDX_RANK_HD uint32_t rank_key(uint32_t bits) {
  if ((bits & 0x7fffffffu) == 0) bits = 0;
  const uint32_t asc = (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
  return ~asc;
}
SEDX_RANK_HD uint32_t rank_key_bits(uint32_t key) {   // the score's bit pattern back
  const uint32_t asc = ~key;
  return (asc & 0x80000000u) ? (asc & 0x7fffffffu) : ~asc;
}
SEDX_RANK_HD bool rank_nonfinite(uint32_t bits) { return (bits & 0x7f800000u) == 0x7f800000u; }

// one term of the sum; tp_prev = tp_{k-1} (0 for the first threshold)
SEDX_RANK_HD double rank_term(int32_t tp, int32_t tp_prev, int32_t n, int64_t P) {
  return ((double)(tp - tp_prev) / (double)P) * ((double)tp / (double)n);
}

// rank_host.cpp: 1 <= M < 2^31, 1 <= C <= 65535, and the message of the
// handle-free average-precision entry points (sedx_last_error(NULL))
sedx_status rank_check(int64_t M, int64_t C);
sedx_status rank_fail(const char* fmt, ...);
const char* rank_error();
void rank_error_clear();

}  // namespace sedx
#endif
