// Average precision as a ranking problem (pytorch/evaluate.py:24,76 call
// sklearn.metrics.average_precision_score): a per-class segmented radix sort
// of the scores and the precision-recall curve in integers over it.  The
// definition, the P = 0 and non-finite rules: include/sedx.h.
//
// Per group of classes (the workspace holds RANK_GROUP_ELEMS / M classes):
//   keys     scores [M][C] / target [M][C] -> key [g][M], label [g][M] through
//            an LDS tile (reads coalesced along the classes, writes along the
//            samples); key = rank_key (rank.h): ascending keys are descending
//            scores.  Non-finite scores are counted per class (integer
//            atomics).
//   sort     LSD radix, 8 bits x 4 passes, each pass: per-tile histogram
//            (RANK_TILE keys per workgroup, LDS integer atomics), exclusive
//            scan over (digit, tile), stable scatter.  A key's slot inside its
//            tile comes from lane order only: wavefront w takes the keys
//            [1024 w, 1024 (w + 1)) of the tile in 16 rounds of 64, a round's
//            lanes with equal digits find each other with 8 ballots, a lane's
//            slot is the wavefront's running count of the digit plus the
//            popcount of the lower matching lanes, and the highest matching
//            lane advances the count.  No slot is claimed with an atomic.  All
//            counters are 32-bit (M < 2^31).
//   curve    run ends key[i] != key[i + 1] (and i = M - 1), inclusive scan of
//            the labels and the index: (t_k, tp_k, n_k) compacted per class.
//   sum      float64, in ONE order that depends on nothing but k:
//            term_k = ((double)(tp_k - tp_{k-1}) / (double)P) * ((double)tp_k / (double)n_k);
//            64 consecutive terms (k = 64 q .. 64 q + 63, missing ones +0.0)
//            by the tree a[j] += a[j + off], off = 32, 16, 8, 4, 2, 1 (a
//            wavefront's shuffle-down reduction); 64 consecutive such sums by
//            the same tree; the resulting sums (one per 4096 terms) added in
//            ascending order starting from +0.0.  rank_host.cpp does the same.
// No float atomics anywhere.
#include "rank.h"
#include "sedx_internal.h"

namespace sedx {

namespace {

constexpr int RK_THREADS = 256;
constexpr int RK_WAVES = RK_THREADS / 64;
constexpr int RK_ROUNDS = (int)(RANK_TILE / RK_THREADS);      // rounds of 64 keys per wavefront
constexpr int RK_PER_WAVE = RK_ROUNDS * 64;
constexpr int RK_PER_THREAD = (int)(RANK_TILE / RK_THREADS);  // curve pass: consecutive elements per thread
constexpr int KP_ROWS = 64, KP_COLS = 64;                     // key pass tile: samples x classes
static_assert(RANK_TILE == (int64_t)RANK_SUM_CHUNK * RANK_SUM_CHUNK, "one workgroup sums one second-level chunk");

struct RankTotals {
  int64_t K, P;   // K = 0 for a class with a non-finite score
};

__device__ __forceinline__ void rk_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// grid (ceil(M / 64), ceil(G / 64)); classes c0 .. c0 + G - 1 of the call
__global__ __launch_bounds__(RK_THREADS) void rank_keys_kernel(const float* __restrict__ scores,
                                                               const uint8_t* __restrict__ target, int64_t M,
                                                               int64_t C, int64_t c0, int64_t G, int64_t stride,
                                                               uint32_t* __restrict__ keys,
                                                               uint8_t* __restrict__ labels,
                                                               unsigned long long* __restrict__ info) {
  __shared__ uint32_t tk[KP_ROWS * (KP_COLS + 1)];
  __shared__ uint8_t tl[KP_ROWS * (KP_COLS + 1)];
  const int64_t m0 = (int64_t)blockIdx.x * KP_ROWS, g0 = (int64_t)blockIdx.y * KP_COLS;
  const int cw = (int)(G - g0 < KP_COLS ? G - g0 : KP_COLS);
  const int rows = (int)(M - m0 < KP_ROWS ? M - m0 : KP_ROWS);
  const int ld = cw | 1;
  for (int e = threadIdx.x; e < rows * cw; e += RK_THREADS) {
    const int r = e / cw, c = e - r * cw;
    const int64_t src = (m0 + r) * C + c0 + g0 + c;
    tk[r * ld + c] = __float_as_uint(scores[src]);
    tl[r * ld + c] = target[src] != 0;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < cw * KP_ROWS; e += RK_THREADS) {   // whole wavefronts: c is wave-uniform
    const int c = e >> 6, r = e & 63;
    const bool ok = r < rows;
    const uint32_t bits = ok ? tk[r * ld + c] : 0u;
    if (ok) {
      keys[(g0 + c) * stride + m0 + r] = rank_key(bits);
      labels[(g0 + c) * stride + m0 + r] = tl[r * ld + c];
    }
    const unsigned long long bad = __ballot(ok && rank_nonfinite(bits));
    if (bad && r == 0) atomicAdd(&info[(c0 + g0 + c) * 3 + 2], (unsigned long long)__builtin_popcountll(bad));
  }
}

// grid (ntiles, G): hist[g][digit][tile]
__global__ __launch_bounds__(RK_THREADS) void rank_hist_kernel(const uint32_t* __restrict__ keys, int64_t M,
                                                               int64_t stride, int shift, int64_t ntiles,
                                                               uint32_t* __restrict__ hist) {
  __shared__ uint32_t h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  const int64_t tile = blockIdx.x, g = blockIdx.y;
  const uint32_t* k = keys + g * stride;
  const int64_t i0 = tile * RANK_TILE;
  for (int r = 0; r < RK_ROUNDS; ++r) {
    const int64_t i = i0 + r * RK_THREADS + threadIdx.x;
    if (i < M) atomicAdd(&h[(k[i] >> shift) & 255u], 1u);
  }
  __syncthreads();
  hist[(g * 256 + threadIdx.x) * ntiles + tile] = h[threadIdx.x];
}

// grid (G): exclusive scan of one class's [digit][tile] counts in that order, in place
__global__ __launch_bounds__(256) void rank_scan_kernel(uint32_t* __restrict__ hist, int64_t ntiles) {
  __shared__ uint32_t tot[256];
  uint32_t* row = hist + ((int64_t)blockIdx.x * 256 + threadIdx.x) * ntiles;
  uint32_t s = 0;
  for (int64_t t = 0; t < ntiles; ++t) s += row[t];
  tot[threadIdx.x] = s;
  __syncthreads();
  uint32_t base = 0;
  for (int j = 0; j < (int)threadIdx.x; ++j) base += tot[j];
  for (int64_t t = 0; t < ntiles; ++t) {
    const uint32_t v = row[t];
    row[t] = base;
    base += v;
  }
}

// grid (ntiles, G): the stable scatter of one pass (see the file comment)
__global__ __launch_bounds__(RK_THREADS) void rank_scatter_kernel(const uint32_t* __restrict__ kin,
                                                                  const uint8_t* __restrict__ lin,
                                                                  uint32_t* __restrict__ kout,
                                                                  uint8_t* __restrict__ lout, int64_t M,
                                                                  int64_t stride, int shift, int64_t ntiles,
                                                                  const uint32_t* __restrict__ base) {
  __shared__ uint32_t wh[RK_WAVES][256];
  __shared__ uint32_t tb[256];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t tile = blockIdx.x, g = blockIdx.y;
#pragma unroll
  for (int w = 0; w < RK_WAVES; ++w) wh[w][threadIdx.x] = 0;
  tb[threadIdx.x] = base[(g * 256 + threadIdx.x) * ntiles + tile];
  __syncthreads();

  const uint32_t* ki = kin + g * stride;
  const uint8_t* li = lin + g * stride;
  const int64_t i0 = tile * RANK_TILE + (int64_t)wave * RK_PER_WAVE;
  const unsigned long long lower = (1ull << lane) - 1ull;
  uint32_t key[RK_ROUNDS], off[RK_ROUNDS];
  uint8_t lab[RK_ROUNDS];
#pragma unroll
  for (int r = 0; r < RK_ROUNDS; ++r) {
    const int64_t i = i0 + r * 64 + lane;
    const bool ok = i < M;
    key[r] = ok ? ki[i] : 0xffffffffu;
    lab[r] = ok ? li[i] : (uint8_t)0;
    const uint32_t d = (key[r] >> shift) & 255u;
    unsigned long long match = __ballot(ok);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (d >> b) & 1u;
      const unsigned long long bal = __ballot(ok && bit);
      match &= bit ? bal : ~bal;
    }
    const uint32_t pre = ok ? wh[wave][d] : 0u;
    rk_wave_sync();
    if (ok && (match >> lane) == 1ull) wh[wave][d] = pre + (uint32_t)__builtin_popcountll(match);
    rk_wave_sync();
    off[r] = pre + (uint32_t)__builtin_popcountll(match & lower);
  }
  __syncthreads();
  {   // digit threadIdx.x: exclusive over the wavefronts
    uint32_t run = 0;
#pragma unroll
    for (int w = 0; w < RK_WAVES; ++w) {
      const uint32_t t = wh[w][threadIdx.x];
      wh[w][threadIdx.x] = run;
      run += t;
    }
  }
  __syncthreads();
  uint32_t* ko = kout + g * stride;
  uint8_t* lo = lout + g * stride;
#pragma unroll
  for (int r = 0; r < RK_ROUNDS; ++r) {
    const int64_t i = i0 + r * 64 + lane;
    if (i < M) {
      const uint32_t d = (key[r] >> shift) & 255u;
      const int64_t dest = (int64_t)tb[d] + wh[wave][d] + off[r];
      if (dest < M) {   // always true for consistent counts
        ko[dest] = key[r];
        lo[dest] = lab[r];
      }
    }
  }
}

__device__ __forceinline__ uint32_t rk_wave_incl(uint32_t v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = __shfl_up(v, o);
    if (lane >= o) v += t;
  }
  return v;
}

// exclusive prefix of (a, b) over the workgroup's threads; tot = the workgroup's sums
__device__ __forceinline__ void rk_block_excl2(uint32_t a, uint32_t b, uint32_t& ea, uint32_t& eb, uint32_t& ta,
                                               uint32_t& tb_) {
  __shared__ uint32_t wa[RK_WAVES], wb[RK_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t ia = rk_wave_incl(a, lane), ib = rk_wave_incl(b, lane);
  if (lane == 63) {
    wa[wave] = ia;
    wb[wave] = ib;
  }
  __syncthreads();
  ea = ia - a;
  eb = ib - b;
  ta = 0;
  tb_ = 0;
#pragma unroll
  for (int w = 0; w < RK_WAVES; ++w) {
    if (w < wave) {
      ea += wa[w];
      eb += wb[w];
    }
    ta += wa[w];
    tb_ += wb[w];
  }
}

// this thread's RK_PER_THREAD consecutive elements of the tile: run ends and label sum
__device__ __forceinline__ void rk_thread_counts(const uint32_t* k, const uint8_t* l, int64_t i0, int64_t M,
                                                 uint32_t& ends, uint32_t& lsum) {
  ends = 0;
  lsum = 0;
  for (int j = 0; j < RK_PER_THREAD; ++j) {
    const int64_t i = i0 + j;
    if (i < M) {
      ends += (i == M - 1 || k[i + 1] != k[i]) ? 1u : 0u;
      lsum += l[i];
    }
  }
}

// grid (ntiles, G): part[g][tile] = (run ends, positives) of the tile
__global__ __launch_bounds__(RK_THREADS) void rank_curve_count_kernel(const uint32_t* __restrict__ keys,
                                                                      const uint8_t* __restrict__ labels, int64_t M,
                                                                      int64_t stride, int64_t ntiles,
                                                                      uint2* __restrict__ part) {
  const int64_t tile = blockIdx.x, g = blockIdx.y;
  uint32_t ends, lsum, ea, eb, ta, tb_;
  rk_thread_counts(keys + g * stride, labels + g * stride, tile * RANK_TILE + (int64_t)threadIdx.x * RK_PER_THREAD, M,
                   ends, lsum);
  rk_block_excl2(ends, lsum, ea, eb, ta, tb_);
  if (threadIdx.x == 0) part[g * ntiles + tile] = make_uint2(ta, tb_);
}

// grid (G): exclusive scan of part over the tiles, in place; totals -> tot[g], info (P, K)
__global__ __launch_bounds__(256) void rank_curve_scan_kernel(uint2* __restrict__ part, int64_t ntiles, int64_t c0,
                                                              RankTotals* __restrict__ tot,
                                                              int64_t* __restrict__ info) {
  __shared__ uint32_t sa[256], sb[256];
  const int64_t g = blockIdx.x;
  uint2* p = part + g * ntiles;
  const int64_t per = (ntiles + 255) / 256;
  const int64_t t0 = (int64_t)threadIdx.x * per, t1 = t0 + per < ntiles ? t0 + per : ntiles;
  uint32_t a = 0, b = 0;
  for (int64_t t = t0; t < t1; ++t) {
    a += p[t].x;
    b += p[t].y;
  }
  sa[threadIdx.x] = a;
  sb[threadIdx.x] = b;
  __syncthreads();
  uint32_t ba = 0, bb = 0;
  for (int j = 0; j < (int)threadIdx.x; ++j) {
    ba += sa[j];
    bb += sb[j];
  }
  for (int64_t t = t0; t < t1; ++t) {
    const uint2 v = p[t];
    p[t] = make_uint2(ba, bb);
    ba += v.x;
    bb += v.y;
  }
  if (threadIdx.x == 255) {   // its running sums are the totals (t1 <= ntiles for every thread)
    int64_t* inf = info + (c0 + g) * 3;
    const bool bad = inf[2] != 0;
    tot[g].K = bad ? 0 : (int64_t)ba;
    tot[g].P = (int64_t)bb;
    inf[0] = (int64_t)bb;
    inf[1] = bad ? 0 : (int64_t)ba;
  }
}

// grid (ntiles, G): (tp_k, n_k) compacted per class, and the caller's curve
__global__ __launch_bounds__(RK_THREADS) void rank_curve_write_kernel(const uint32_t* __restrict__ keys,
                                                                      const uint8_t* __restrict__ labels, int64_t M,
                                                                      int64_t stride, int64_t ntiles,
                                                                      const uint2* __restrict__ part,
                                                                      const RankTotals* __restrict__ tot, int64_t c0,
                                                                      int32_t* __restrict__ ctp,
                                                                      int32_t* __restrict__ cn,
                                                                      float* __restrict__ o_thr,
                                                                      int32_t* __restrict__ o_tp,
                                                                      int32_t* __restrict__ o_n) {
  const int64_t tile = blockIdx.x, g = blockIdx.y;
  const uint32_t* k = keys + g * stride;
  const uint8_t* l = labels + g * stride;
  const int64_t i0 = tile * RANK_TILE + (int64_t)threadIdx.x * RK_PER_THREAD;
  uint32_t ends, lsum, ea, eb, ta, tb_;
  rk_thread_counts(k, l, i0, M, ends, lsum);
  rk_block_excl2(ends, lsum, ea, eb, ta, tb_);
  const uint2 base = part[g * ntiles + tile];
  int64_t kk = (int64_t)base.x + ea;
  int32_t tp = (int32_t)(base.y + eb);
  const bool user = o_thr != nullptr && tot[g].K != 0;   // K = 0: a non-finite score, no curve
  for (int j = 0; j < RK_PER_THREAD; ++j) {
    const int64_t i = i0 + j;
    if (i >= M) break;
    tp += l[i];
    if (i == M - 1 || k[i + 1] != k[i]) {
      if (kk < M) {   // always true: at most one run end per element
        ctp[g * stride + kk] = tp;
        cn[g * stride + kk] = (int32_t)(i + 1);
        if (user) {
          o_thr[(c0 + g) * M + kk] = __uint_as_float(rank_key_bits(k[i]));
          o_tp[(c0 + g) * M + kk] = tp;
          o_n[(c0 + g) * M + kk] = (int32_t)(i + 1);
        }
      }
      ++kk;
    }
  }
}

__device__ __forceinline__ double rk_tree(double t) {
#pragma unroll
  for (int off = RANK_SUM_CHUNK / 2; off >= 1; off >>= 1) t += __shfl_down(t, off);
  return t;   // lane 0 holds the tree's sum
}

// grid (ntiles, G): s2[g][blk] = the second-level sum of terms 4096 blk .. 4096 blk + 4095
__global__ __launch_bounds__(RK_THREADS) void rank_terms_kernel(const int32_t* __restrict__ ctp,
                                                                const int32_t* __restrict__ cn, int64_t stride,
                                                                int64_t ntiles, const RankTotals* __restrict__ tot,
                                                                double* __restrict__ s2) {
  __shared__ double cs[RANK_SUM_CHUNK];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t blk = blockIdx.x, g = blockIdx.y;
  const int64_t K = tot[g].K, P = tot[g].P;
  if (blk * RANK_TILE >= K || P == 0) {   // workgroup-uniform
    if (threadIdx.x == 0) s2[g * ntiles + blk] = 0.0;
    return;
  }
  const int32_t* tp = ctp + g * stride;
  const int32_t* n = cn + g * stride;
  constexpr int CHUNKS_PER_WAVE = RANK_SUM_CHUNK / RK_WAVES;
  for (int q = 0; q < CHUNKS_PER_WAVE; ++q) {
    const int chunk = wave * CHUNKS_PER_WAVE + q;
    const int64_t kk = blk * RANK_TILE + (int64_t)chunk * RANK_SUM_CHUNK + lane;
    double t = 0.0;
    if (kk < K) t = rank_term(tp[kk], kk ? tp[kk - 1] : 0, n[kk], P);
    t = rk_tree(t);
    if (lane == 0) cs[chunk] = t;
  }
  __syncthreads();
  if (wave == 0) {
    const double t = rk_tree(cs[lane]);
    if (lane == 0) s2[g * ntiles + blk] = t;
  }
}

// one thread per class: the second-level sums in ascending order
__global__ __launch_bounds__(64) void rank_final_kernel(const double* __restrict__ s2, int64_t ntiles, int64_t G,
                                                        int64_t c0, const RankTotals* __restrict__ tot,
                                                        double* __restrict__ ap) {
  const int64_t g = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (g >= G) return;
  const int64_t K = tot[g].K, P = tot[g].P;
  if (K == 0 || P == 0) {
    ap[c0 + g] = __longlong_as_double(0x7ff8000000000000ll);
    return;
  }
  const int64_t nb = (K + RANK_TILE - 1) / RANK_TILE;
  double sum = 0.0;
  for (int64_t b = 0; b < nb; ++b) sum += s2[g * ntiles + b];
  ap[c0 + g] = sum;
}

struct RankLayout {
  int64_t gmax, stride, ntiles;
  size_t keys_a, keys_b, lab_a, lab_b, cn, hist, part, tot, s2, bytes;
};

// keys_b doubles as the compacted tp once the sort has ended in keys_a
RankLayout rank_layout(int64_t M, int64_t C) {
  RankLayout l;
  l.gmax = std::max<int64_t>(1, std::min<int64_t>(C, RANK_GROUP_ELEMS / M));
  l.stride = (M + 63) / 64 * 64;
  l.ntiles = (M + RANK_TILE - 1) / RANK_TILE;
  size_t o = 0;
  auto take = [&o](int64_t bytes) {
    const size_t at = o;
    o += align256(bytes);
    return at;
  };
  l.keys_a = take(l.gmax * l.stride * 4);
  l.keys_b = take(l.gmax * l.stride * 4);
  l.lab_a = take(l.gmax * l.stride);
  l.lab_b = take(l.gmax * l.stride);
  l.cn = take(l.gmax * l.stride * 4);
  l.hist = take(l.gmax * 256 * l.ntiles * 4);
  l.part = take(l.gmax * l.ntiles * 8);
  l.tot = take(l.gmax * (int64_t)sizeof(RankTotals));
  l.s2 = take(l.gmax * l.ntiles * 8);
  l.bytes = o;
  return l;
}

template <typename K, typename... A>
bool rk_launch(K kern, dim3 grid, int threads, hipStream_t s, A... args) {
  if (!launch_info(reinterpret_cast<const void*>(kern), threads, 0).ok) return false;
  hipLaunchKernelGGL(kern, grid, dim3(threads), 0, s, args...);
  return true;
}

}  // namespace

}  // namespace sedx

extern "C" sedx_status sedx_average_precision_workspace_size(int64_t M, int64_t C, size_t* bytes) {
  using namespace sedx;
  const sedx_status chk = rank_check(M, C);
  if (chk != SEDX_OK) return chk;
  if (!bytes) return rank_fail("average precision: null argument");
  *bytes = rank_layout(M, C).bytes;
  return SEDX_OK;
}

extern "C" sedx_status sedx_average_precision_device(const float* d_scores, const uint8_t* d_target, int64_t M,
                                                     int64_t C, double* d_ap, int64_t* d_info, float* d_thr,
                                                     int32_t* d_tp, int32_t* d_n, void* d_workspace,
                                                     size_t workspace_bytes, void* stream) {
  using namespace sedx;
  const sedx_status chk = rank_check(M, C);
  if (chk != SEDX_OK) return chk;
  if (!d_scores || !d_target || !d_ap || !d_info) return rank_fail("average precision: null argument");
  const bool curve = d_thr && d_tp && d_n;
  if (!curve && (d_thr || d_tp || d_n))
    return rank_fail("average precision: the curve needs thr, tp and n together (or none of them)");
  const RankLayout l = rank_layout(M, C);
  if (!d_workspace || workspace_bytes < l.bytes)
    return rank_fail("average precision: workspace too small: %zu < %zu bytes", workspace_bytes, l.bytes);
  hipStream_t s = static_cast<hipStream_t>(stream);
  char* p = static_cast<char*>(d_workspace);
  uint32_t* keys[2] = {reinterpret_cast<uint32_t*>(p + l.keys_a), reinterpret_cast<uint32_t*>(p + l.keys_b)};
  uint8_t* labs[2] = {reinterpret_cast<uint8_t*>(p + l.lab_a), reinterpret_cast<uint8_t*>(p + l.lab_b)};
  int32_t* cn = reinterpret_cast<int32_t*>(p + l.cn);
  uint32_t* hist = reinterpret_cast<uint32_t*>(p + l.hist);
  uint2* part = reinterpret_cast<uint2*>(p + l.part);
  RankTotals* tot = reinterpret_cast<RankTotals*>(p + l.tot);
  double* s2 = reinterpret_cast<double*>(p + l.s2);
  // the non-finite counts are accumulated; everything else is overwritten
  if (hipMemsetAsync(d_info, 0, (size_t)C * 3 * sizeof(int64_t), s) != hipSuccess) return SEDX_EHIP;
  const unsigned nt = (unsigned)l.ntiles;
  bool ok = true;
  for (int64_t c0 = 0; c0 < C && ok; c0 += l.gmax) {
    const int64_t G = std::min<int64_t>(l.gmax, C - c0);
    const dim3 tiles(nt, (unsigned)G);
    ok = ok && rk_launch(rank_keys_kernel, dim3((unsigned)((M + KP_ROWS - 1) / KP_ROWS), (unsigned)((G + KP_COLS - 1) / KP_COLS)),
                         RK_THREADS, s, d_scores, d_target, M, C, c0, G, l.stride, keys[0], labs[0],
                         reinterpret_cast<unsigned long long*>(d_info));
    for (int pass = 0; pass < 4 && ok; ++pass) {
      const int in = pass & 1, out = in ^ 1, shift = 8 * pass;
      ok = ok && rk_launch(rank_hist_kernel, tiles, RK_THREADS, s, (const uint32_t*)keys[in], M, l.stride, shift,
                           l.ntiles, hist);
      ok = ok && rk_launch(rank_scan_kernel, dim3((unsigned)G), 256, s, hist, l.ntiles);
      ok = ok && rk_launch(rank_scatter_kernel, tiles, RK_THREADS, s, (const uint32_t*)keys[in],
                           (const uint8_t*)labs[in], keys[out], labs[out], M, l.stride, shift, l.ntiles,
                           (const uint32_t*)hist);
    }
    int32_t* ctp = reinterpret_cast<int32_t*>(keys[1]);   // four passes: the sorted keys are in keys[0]
    ok = ok && rk_launch(rank_curve_count_kernel, tiles, RK_THREADS, s, (const uint32_t*)keys[0],
                         (const uint8_t*)labs[0], M, l.stride, l.ntiles, part);
    ok = ok && rk_launch(rank_curve_scan_kernel, dim3((unsigned)G), 256, s, part, l.ntiles, c0, tot, d_info);
    ok = ok && rk_launch(rank_curve_write_kernel, tiles, RK_THREADS, s, (const uint32_t*)keys[0],
                         (const uint8_t*)labs[0], M, l.stride, l.ntiles, (const uint2*)part, (const RankTotals*)tot,
                         c0, ctp, cn, curve ? d_thr : (float*)nullptr, curve ? d_tp : (int32_t*)nullptr,
                         curve ? d_n : (int32_t*)nullptr);
    ok = ok && rk_launch(rank_terms_kernel, tiles, RK_THREADS, s, (const int32_t*)ctp, (const int32_t*)cn, l.stride,
                         l.ntiles, (const RankTotals*)tot, s2);
    ok = ok && rk_launch(rank_final_kernel, dim3((unsigned)((G + 63) / 64)), 64, s, (const double*)s2, l.ntiles, G,
                         c0, (const RankTotals*)tot, d_ap);
  }
  if (take_launch_error() != hipSuccess || !ok) return SEDX_EHIP;
  return hipGetLastError() == hipSuccess ? SEDX_OK : SEDX_EHIP;
}
