// Geometry and arithmetic that conv_f16.hip, the host packer (weights.cpp) and
// the host-side checks (tests/native/f16_pack_driver.cpp) share: the operand
// rounding q, the LDS images of the halo and of the weights, and the MFMA
// row -> pixel maps.  Plain C++, usable on host and device.
#pragma once
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define SEDX_F16_HD __host__ __device__ inline
#else
#define SEDX_F16_HD inline
#endif

namespace sedx {

// q(v), SEDX_PRECISION_F16's operand rounding, as fp16 bits: clamp to
// +-65504, round to nearest even with gradual underflow in the rounding
// itself, then every result below 2^-14 in magnitude (zeros and subnormals
// of either sign) becomes +0.  Integer arithmetic only: the host's answer
// does not depend on the compiler's _Float16 support.  (NaN stays a NaN; no
// weight is one.)
inline uint16_t f16_q_bits(float v) {
  uint32_t u;
  std::memcpy(&u, &v, 4);
  const uint16_t sign = (uint16_t)((u >> 16) & 0x8000u);
  const uint32_t a = u & 0x7FFFFFFFu;
  if (a > 0x7F800000u) return 0x7E00;
  if (a >= 0x477FE000u) return sign | 0x7BFF;   // |v| >= 65504: the clamp
  const int e = (int)(a >> 23) - 127;           // unbiased exponent of |v|
  if (e < -25) return 0;                        // below half the smallest subnormal
  uint32_t man = (a & 0x7FFFFFu) | 0x800000u;   // 24-bit significand
  // bits to drop: 13 for a normal result, more below 2^-14 (gradual underflow)
  const int drop = e >= -14 ? 13 : 13 + (-14 - e);
  const uint32_t half = 1u << (drop - 1), rest = man & ((1u << drop) - 1);
  uint32_t m = man >> drop;
  if (rest > half || (rest == half && (m & 1u))) ++m;
  // m counts units of 2^(max(e, -14) - 10): the implicit bit adds one exponent step
  const uint32_t bits = e >= -14 ? ((uint32_t)(e + 14) << 10) + m : m;   // (e + 15 - 1) << 10 + (1.m)
  if ((bits & 0x7C00u) == 0) return 0;          // the flush: |q| < 2^-14 -> +0
  return sign | (uint16_t)bits;
}

// ---- LDS images ---------------------------------------------------------------
// Halo: one record per pixel position, F16_REC_U4 16-byte slots: [k 0-7 | k 8-15 | pad].
// A lane of the A fragment (MFMA row r = lane & 31, k half h = lane >> 5) reads
// slot position * 3 + h.  ds_read_b128 is served in 4 groups of 16 lanes, a
// group conflict-free when its 16 slots are distinct mod 16 (64 banks of 4 B);
// h is constant in a group and 3 is odd, so that is: the group's 16 positions
// are distinct mod 16 — what the row stride CSP is chosen for, per shape.
constexpr int F16_REC_U4 = 3;

// output tile: BM pixels x BN channels (8 waves of 64 x 64)
SEDX_F16_HD constexpr int f16_bm(int BN) { return BN == 64 ? 512 : 256; }

// halo row stride in positions (>= F + 2), by (F, pooled epilogue)
SEDX_F16_HD constexpr int f16_csp(int F, bool pool) {
  return pool ? (F == 64 ? 72 : F == 32 ? 40 : 24) : (F == 64 ? 66 : F == 32 ? 34 : F == 16 ? 32 : 12);
}

// MFMA row R (0 .. BM-1 of the block tile) -> (t_local, f).  pool: R = 4 q + e,
// a 2x2 pool group in one lane's accumulator registers 4g .. 4g+3.  F == 8
// un-pooled: 32 rows = 4 t x 8 f, arranged so that the ds_read_b128 lane
// groups each hold two whole t rows and a lane's registers {0-3,12-15} and
// {4-11} are one t each (the frequency mean stays in-lane).
SEDX_F16_HD void f16_rowmap(int F, bool pool, int R, int& tl, int& f) {
  if (pool) {
    const int q = R >> 2, e = R & 3;
    const int tp = q / (F / 2), fp = q % (F / 2);
    tl = 2 * tp + (e >> 1);
    f = 2 * fp + (e & 1);
  } else if (F == 8) {
    const int r = R & 31, half = r >> 4, q = (r >> 2) & 3;
    const int tq = half ? ((0x3021 >> (4 * q)) & 0xF) : ((0x2130 >> (4 * q)) & 0xF);
    tl = 4 * (R >> 5) + tq;
    f = (r & 3) + 4 * half;
  } else {
    tl = R / F;
    f = R % F;
  }
}

// the 16-byte LDS slot that the A-fragment lane of row R and k half h reads for tap (0, 0); tap (ky, kx) adds
// (ky * CSP + kx) * F16_REC_U4
SEDX_F16_HD int f16_aslot(int F, bool pool, int R, int h) {
  int tl = 0, f = 0;
  f16_rowmap(F, pool, R, tl, f);
  return (tl * f16_csp(F, pool) + f) * F16_REC_U4 + h;
}

// Weights: per (n-tile, 16-channel chunk, tap) BN records of 2 slots (32 B, no
// pad): k half c of output channel n sits in slot 2 n + (c ^ ((n >> 3) & 1)).
// A B-fragment lane (n = lane & 31 of its 32-column tile, h = lane >> 5) reads
// f16_wslot(n, h); in every 16-lane group each n mod 8 occurs twice, once
// with bit 3 set and once clear, so the 16 slots are distinct mod 16.
SEDX_F16_HD constexpr int f16_wslot(int n, int c) { return 2 * n + (c ^ ((n >> 3) & 1)); }

// where pack_f16 puts weight (o, i, tap), in fp16 elements:
// [N/BN][K/16][taps][BN][2 slots x 8]
inline size_t f16_pack_index(int K, int taps, int BN, int o, int i, int tap) {
  const int n = o % BN, k = i % 16;
  return ((((size_t)(o / BN) * (K / 16) + i / 16) * taps + tap) * BN) * 16 + (size_t)f16_wslot(n, k / 8) * 8 + k % 8;
}

}  // namespace sedx
