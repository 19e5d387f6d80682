// Host-side segment-based counts for threshold calibration: the quirk-exact
// host state machine (sedx_events, vad.cpp) per (clip, class, variant), events
// rasterised onto the segment grid and counted against the target masks.
// The bit-for-bit mirror of segment_counts_kernel (calib.hip).
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/sedx.h"
#include "rank.h"

namespace sedx {

namespace {
thread_local std::string g_segment_error;
}

// message of the handle-free segment-count entry points (sedx_last_error(NULL))
const char* segment_error() { return g_segment_error.empty() ? nullptr : g_segment_error.c_str(); }

sedx_status segment_fail(const char* fmt, ...) {
  char buf[256];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_segment_error = buf;
  rank_error_clear();   // sedx_last_error(NULL) reports the latest failure of either family
  return SEDX_EINVAL;
}

// the shape limits shared by the host and the device entry point
sedx_status segment_counts_check(int64_t n_clips, int64_t T, int64_t C, int64_t segment_frames, int64_t V) {
  if (n_clips < 0 || T < 0 || C <= 0) return segment_fail("segment counts: n_clips >= 0, T >= 0 and C >= 1 are required");
  if (segment_frames < 1) return segment_fail("segment counts: segment_frames = %lld, must be >= 1", (long long)segment_frames);
  if (V < 1 || V > 64) return segment_fail("segment counts: V = %lld variants, 1..64 are supported", (long long)V);
  if ((T + segment_frames - 1) / segment_frames > 64)
    return segment_fail("segment counts: T = %lld at %lld frames per segment is %lld segments, at most 64 fit the mask",
                        (long long)T, (long long)segment_frames, (long long)((T + segment_frames - 1) / segment_frames));
  return SEDX_OK;
}

}  // namespace sedx

extern "C" sedx_status sedx_segment_counts(const float* h_x, int64_t n_clips, int64_t T, int64_t C,
                                           const uint64_t* h_target, int64_t segment_frames, int64_t V,
                                           const double* high, const double* low, const int64_t* n_smooth,
                                           const int64_t* n_salt, int64_t* h_counts) {
  using namespace sedx;
  const sedx_status chk = segment_counts_check(n_clips, T, C, segment_frames, V);
  if (chk != SEDX_OK) return chk;
  if (!high || !low || !n_smooth || !n_salt || !h_counts || (n_clips > 0 && (!h_x || !h_target)))
    return segment_fail("segment counts: null argument");
  for (int64_t i = 0; i < V * C * 4; ++i) h_counts[i] = 0;
  const int64_t S = (T + segment_frames - 1) / segment_frames;
  const uint64_t smask = S >= 64 ? ~0ull : ((1ull << S) - 1);
  const int64_t cap = T / 2 + 2;                    // a series has at most T / 2 + 1 runs
  std::vector<float> x((size_t)(T > 0 ? T : 1));   // never a null pointer (T = 0)
  std::vector<int32_t> ev((size_t)cap * 4);
  for (int64_t n = 0; n < n_clips; ++n)
    for (int64_t k = 0; k < C; ++k) {
      for (int64_t t = 0; t < T; ++t) x[t] = h_x[(n * T + t) * C + k];
      const uint64_t ref = h_target[n * C + k] & smask;
      for (int64_t v = 0; v < V; ++v) {
        int64_t* out = h_counts + (v * C + k) * 4;
        int64_t n_ev = 0;
        const sedx_status st = sedx_events(x.data(), 1, T, 1, high + v * C + k, low + v * C + k, 1, n_smooth + k,
                                           n_salt + k, ev.data(), cap, &n_ev);
        if (st != SEDX_OK) {                        // the reference's IndexError
          out[3] += 1;
          continue;
        }
        uint64_t est = 0;
        for (int64_t e = 0; e < n_ev; ++e) {
          const int64_t b = ev[4 * e + 2], f = ev[4 * e + 3];
          const int64_t s0 = b / segment_frames, s1 = (f + segment_frames - 1) / segment_frames;
          if (s1 > s0 && s0 < 64) {
            const int64_t len = s1 - s0;
            est |= (len >= 64 ? ~0ull : ((1ull << len) - 1)) << s0;
          }
        }
        est &= smask;
        out[0] += __builtin_popcountll(est & ref);
        out[1] += __builtin_popcountll(est & ~ref);
        out[2] += __builtin_popcountll(ref & ~est);
      }
    }
  return SEDX_OK;
}
