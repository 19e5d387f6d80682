// Host entry of the average-precision ranking (sedx_average_precision): per
// class a stable sort of the keys rank.hip sorts, the same integer curve and
// the same float64 sum in the same order (rank.h, include/sedx.h), so `ap` is
// bit-identical to the device entry's and `info` / the curve are equal.
// Plain C++: also built without HIP under the sanitizers (make asan-rank).
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "rank.h"

namespace sedx {

namespace {
thread_local std::string g_rank_error;

// The documented order: RANK_SUM_CHUNK consecutive values by the fixed tree
// (a[j] += a[j + off] for off = 32, 16, ..., 1: what a wavefront's shuffle-down
// reduction computes in lane 0), missing values as +0.0.
double tree_sum(const double* v, int64_t n) {
  double a[RANK_SUM_CHUNK];
  for (int j = 0; j < RANK_SUM_CHUNK; ++j) a[j] = j < n ? v[j] : 0.0;
  for (int off = RANK_SUM_CHUNK / 2; off >= 1; off >>= 1)
    for (int j = 0; j < off; ++j) a[j] += a[j + off];
  return a[0];
}

std::vector<double> tree_level(const std::vector<double>& in) {
  const int64_t n = (int64_t)in.size();
  std::vector<double> out((size_t)((n + RANK_SUM_CHUNK - 1) / RANK_SUM_CHUNK));
  for (int64_t q = 0; q < (int64_t)out.size(); ++q)
    out[q] = tree_sum(in.data() + q * RANK_SUM_CHUNK, std::min<int64_t>(RANK_SUM_CHUNK, n - q * RANK_SUM_CHUNK));
  return out;
}
}  // namespace

const char* rank_error() { return g_rank_error.empty() ? nullptr : g_rank_error.c_str(); }
void rank_error_clear() { g_rank_error.clear(); }

sedx_status rank_fail(const char* fmt, ...) {
  char buf[256];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_rank_error = buf;
  return SEDX_EINVAL;
}

sedx_status rank_check(int64_t M, int64_t C) {
  if (M < 1 || M >= (int64_t(1) << 31))
    return rank_fail("average precision: M = %lld samples, 1 <= M < 2^31 is required", (long long)M);
  if (C < 1 || C > 65535)
    return rank_fail("average precision: C = %lld classes, 1 <= C <= 65535 is required", (long long)C);
  return SEDX_OK;
}

}  // namespace sedx

extern "C" int64_t sedx_rank_tile(void) { return sedx::RANK_TILE; }

extern "C" sedx_status sedx_average_precision(const float* h_scores, const uint8_t* h_target, int64_t M, int64_t C,
                                              double* h_ap, int64_t* h_info, float* h_thr, int32_t* h_tp,
                                              int32_t* h_n) {
  using namespace sedx;
  const sedx_status chk = rank_check(M, C);
  if (chk != SEDX_OK) return chk;
  if (!h_scores || !h_target || !h_ap || !h_info) return rank_fail("average precision: null argument");
  const bool curve = h_thr && h_tp && h_n;
  if (!curve && (h_thr || h_tp || h_n))
    return rank_fail("average precision: the curve needs thr, tp and n together (or none of them)");
  int64_t bad_total = 0, bad_class = -1;
  std::vector<uint64_t> v((size_t)M);               // key << 1 | label
  std::vector<int32_t> tp, n;
  std::vector<double> terms;
  for (int64_t c = 0; c < C; ++c) {
    int64_t nonfinite = 0, P = 0;
    for (int64_t i = 0; i < M; ++i) {
      uint32_t bits;
      std::memcpy(&bits, h_scores + i * C + c, 4);
      nonfinite += rank_nonfinite(bits);
      const uint64_t y = h_target[i * C + c] != 0;
      P += (int64_t)y;
      v[(size_t)i] = ((uint64_t)rank_key(bits) << 1) | y;
    }
    h_info[c * 3 + 0] = P;
    h_info[c * 3 + 2] = nonfinite;
    if (nonfinite) {                                // no curve, K = 0, AP = NaN
      h_info[c * 3 + 1] = 0;
      h_ap[c] = std::numeric_limits<double>::quiet_NaN();
      bad_total += nonfinite;
      if (bad_class < 0) bad_class = c;
      continue;
    }
    std::stable_sort(v.begin(), v.end(), [](uint64_t a, uint64_t b) { return (a >> 1) < (b >> 1); });
    tp.clear();
    n.clear();
    int32_t run = 0;
    for (int64_t i = 0; i < M; ++i) {
      run += (int32_t)(v[(size_t)i] & 1);
      if (i == M - 1 || (v[(size_t)i] >> 1) != (v[(size_t)i + 1] >> 1)) {
        if (curve) {
          const uint32_t bits = rank_key_bits((uint32_t)(v[(size_t)i] >> 1));
          std::memcpy(h_thr + c * M + (int64_t)tp.size(), &bits, 4);
          h_tp[c * M + (int64_t)tp.size()] = run;
          h_n[c * M + (int64_t)tp.size()] = (int32_t)(i + 1);
        }
        tp.push_back(run);
        n.push_back((int32_t)(i + 1));
      }
    }
    const int64_t K = (int64_t)tp.size();
    h_info[c * 3 + 1] = K;
    if (P == 0) {
      h_ap[c] = std::numeric_limits<double>::quiet_NaN();
      continue;
    }
    terms.resize((size_t)K);
    for (int64_t k = 0; k < K; ++k) terms[(size_t)k] = rank_term(tp[(size_t)k], k ? tp[(size_t)k - 1] : 0, n[(size_t)k], P);
    const std::vector<double> second = tree_level(tree_level(terms));
    double sum = 0.0;
    for (double s : second) sum += s;
    h_ap[c] = sum;
  }
  if (bad_total)
    return rank_fail("average precision: %lld non-finite score(s), the first in class %lld (its AP is NaN; info[:, 2] "
                     "counts them per class)", (long long)bad_total, (long long)bad_class);
  return SEDX_OK;
}
