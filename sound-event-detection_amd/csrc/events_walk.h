// Device helpers shared by events.hip and calib.hip: the streaming state
// machine of the reference's list stages (find_bgn_fin_pairs -> second
// threshold -> smooth(1) -> smooth(n_smooth) -> remove_salt_noise,
// utils/vad.py:108-199) over a series' on / below bitmaps, one wavefront per
// series.  The quirks are listed at the top of events.hip.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

namespace sedx {
namespace evwalk {

// Streaming state of one series: the find_bgn_fin_pairs run tracker and the
// two smoothers (utils/vad.py:158-183).  Resumable across frame chunks.
struct SeriesState {
  bool ok, in_run, pending, first, s1_any, s2_any;
  int64_t rs, re, pb, pe, s1_mem, s1_pre, s2_mem, s2_pre;
};

__device__ __forceinline__ void series_init(SeriesState& st) {
  st.ok = true;
  st.in_run = st.pending = st.s1_any = st.s2_any = false;
  st.first = true;
  st.rs = st.re = st.pb = st.pe = st.s1_mem = st.s1_pre = st.s2_mem = st.s2_pre = 0;
}

template <typename Emit>
__device__ __forceinline__ void final_out(int64_t b, int64_t f, int64_t n_salt, Emit& emit) {
  if (f - b <= n_salt) return;                     // remove_salt_noise vad.py:186-199
  emit(b, f);
}

template <typename Emit>                           // smooth(n_smooth)
__device__ __forceinline__ void push2(SeriesState& st, int64_t b, int64_t f, int64_t n_smooth,
                                      int64_t n_salt, Emit& emit) {
  if (!st.s2_any) {
    st.s2_any = true;
    st.s2_mem = b;
  } else if (!(b - st.s2_pre <= n_smooth)) {
    final_out(st.s2_mem, st.s2_pre, n_salt, emit);
    st.s2_mem = b;
  }
  st.s2_pre = f;
}

template <typename Emit>                           // smooth(n_smooth=1) of the 2nd threshold
__device__ __forceinline__ void push1(SeriesState& st, int64_t b, int64_t f, int64_t n_smooth,
                                      int64_t n_salt, Emit& emit) {
  if (!st.s1_any) {
    st.s1_any = true;
    st.s1_mem = b;
  } else if (!(b - st.s1_pre <= 1)) {
    push2(st, st.s1_mem, st.s1_pre, n_smooth, n_salt, emit);
    st.s1_mem = b;
  }
  st.s1_pre = f;
}

__device__ __forceinline__ uint64_t ev_uniform(uint64_t v) {
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  return ((uint64_t)hi << 32) | lo;
}

// below-bitmap scans: last set bit <= b (or -1), first set bit >= f (or T)
struct BelowMask {
  const uint64_t* m;
  int64_t W, T;
  __device__ int64_t prev_set(int64_t b) const {
    int64_t w = b >> 6;
    uint64_t bits = ev_uniform(m[w]) & (~0ull >> (63 - (b & 63)));
    while (true) {
      if (bits) return w * 64 + 63 - __builtin_clzll(bits);
      if (--w < 0) return -1;
      bits = ev_uniform(m[w]);
    }
  }
  __device__ int64_t next_set(int64_t f) const {
    int64_t w = f >> 6;
    if (w >= W) return T;
    uint64_t bits = ev_uniform(m[w]) & (~0ull << (f & 63));
    while (true) {
      if (bits) return w * 64 + __builtin_ctzll(bits);
      if (++w >= W) return T;
      bits = ev_uniform(m[w]);
    }
  }
};

template <typename Emit>
__device__ __forceinline__ void push_pair_m(SeriesState& st, const BelowMask& bm, int64_t T, int64_t b,
                                            int64_t f, bool use_lo, int64_t n_smooth, int64_t n_salt,
                                            Emit& emit) {
  if (!use_lo) {
    push2(st, b, f, n_smooth, n_salt, emit);
    return;
  }
  // activity_detection_with_second_thres vad.py:139-151: walk left from b
  // while x >= low (x[b] read first: b == T is the reference's IndexError),
  // right from f until x < low or T
  if (b >= T || f > T) {
    st.ok = false;
    return;
  }
  b = bm.prev_set(b);
  if (f < T) f = bm.next_set(f);
  push1(st, b + 1, f, n_smooth, n_salt, emit);
}

// Runs of the on-bitmap om[W] (wave-uniform scalar code, ctz over words)
// through the reference's list stages; emit(bgn, fin) per surviving event.
// Returns false where the reference raises IndexError (st.ok == false).
template <typename Emit>
__device__ __forceinline__ bool walk_runs(const uint64_t* om, const BelowMask& bm, int64_t W, int64_t T,
                                          bool use_lo, int64_t ns, int64_t nsalt, Emit& emit) {
  SeriesState st;
  series_init(st);
  int64_t w = 0;
  uint64_t cur = W > 0 ? ev_uniform(om[0]) : 0;     // on-bits of word w not yet consumed
  while (st.ok) {
    while (!cur && ++w < W) cur = ev_uniform(om[w]);
    if (!cur) break;
    const int64_t rs = w * 64 + __builtin_ctzll(cur);
    // run end: first off bit after rs
    uint64_t off = ~ev_uniform(om[w]) & (~0ull << (rs & 63));
    int64_t we = w;
    while (!off && ++we < W) off = ~ev_uniform(om[we]);
    const int64_t re1 = off ? we * 64 + __builtin_ctzll(off) : W * 64;   // one past the run
    const int64_t re = (re1 < T ? re1 : T) - 1;
    // find_bgn_fin_pairs vad.py:115-121: a completed run is held until the
    // next one shows it was not the last
    if (st.pending) push_pair_m(st, bm, T, st.pb, st.pe + 1, use_lo, ns, nsalt, emit);
    st.pb = st.first ? rs : rs + 1;
    st.pe = re;
    st.pending = true;
    st.first = false;
    if (re1 >= W * 64) break;
    w = re1 >> 6;
    cur = ev_uniform(om[w]) & (~0ull << (re1 & 63));
  }
  if (st.ok && st.pending) push_pair_m(st, bm, T, st.pb, st.pe, use_lo, ns, nsalt, emit);  // fin = locts[-1]
  if (st.ok && use_lo && st.s1_any) push2(st, st.s1_mem, st.s1_pre, ns, nsalt, emit);
  if (st.ok && st.s2_any) final_out(st.s2_mem, st.s2_pre, nsalt, emit);
  return st.ok;
}

}  // namespace evwalk
}  // namespace sedx
