// Probe: does an out-of-range buffer_load_dword / _dwordx4 ... offen lds
// (raw buffer, voffset >= num_records) write zeros into LDS, and does soffset
// take part in the range check?  The F(4,3) Winograd halo staging
// (csrc/conv_wino43.hip) relies on the zero fill for pixels outside the clip.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>

__global__ void probe(const float* src, int nbytes, int soff_bytes, unsigned* out) {
  __shared__ unsigned sm[2048];
  const int l = threadIdx.x;
  for (int i = l; i < 2048; i += 64) sm[i] = 0xDEADBEEFu;
  __syncthreads();
  __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc((void*)src, 0, nbytes, 0x00020000);
  // lanes 0..31 in range, 32..47 far out (0x80000000), 48..63 just past the end
  unsigned vo = l < 32 ? 4u * l : (l < 48 ? 0x80000000u : (unsigned)nbytes + 4u * (l - 48));
  const unsigned m0a = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(__attribute__((address_space(3))) unsigned*)sm);
  const unsigned m0b = m0a + 256 * 4;
  const int so = __builtin_amdgcn_readfirstlane(soff_bytes);
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dword %0, %1, %3 offen offset:4 lds" ::"v"(vo), "s"(r), "s"(m0a), "s"(so) : "memory");
  unsigned vo4 = l < 32 ? 16u * l : (l < 48 ? 0x80000000u : (unsigned)nbytes + 16u * (l - 48));
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %1, %3 offen lds" ::"v"(vo4), "s"(r), "s"(m0b), "s"(so) : "memory");
  asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
  for (int i = l; i < 512; i += 64) out[i] = sm[i];
}

// The planar halo piece of block 1 (conv_wino43.hip, PL): one dwordx4 piece of
// 64 lanes x 16 bytes whose M0 is 8 (mod 16) — planes 1 and 3 of a halo slot,
// plane stride 770 dwords — with in-range lanes, lanes at 0x80000000 and
// lanes just past num_records in one instruction and a non-zero soffset; then
// ds_read_b64 at ODD dword addresses on it (where a patch would start with the
// image written at M0 exactly: correct values, but see time_reads below — the
// kernel writes the image one dword further instead).  out[0..255]: the piece
// as plain dword reads; out[256..383]: lane l's ds_read_b64 at dword 2 + 4 l + 3.
__global__ void probe_planar(const float* src, int nbytes, int soff_bytes, unsigned* out) {
  __shared__ __attribute__((aligned(16))) unsigned sm[1024];
  const int l = threadIdx.x;
  for (int i = l; i < 1024; i += 64) sm[i] = 0xDEADBEEFu;
  __syncthreads();
  // the resource covers soff_bytes + nbytes: lanes 0..39 in range, 40..51 at 0x80000000, 52..63 past the end
  __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc((void*)src, 0, soff_bytes + nbytes, 0x00020000);
  const unsigned vo = l < 40 ? 16u * l : (l < 52 ? 0x80000000u : (unsigned)(soff_bytes + nbytes) + 16u * (l - 52));
  const unsigned base = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned*)sm;
  const unsigned m0 = __builtin_amdgcn_readfirstlane(base + 2 * 4);   // 8 (mod 16)
  const int so = __builtin_amdgcn_readfirstlane(soff_bytes);
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %1, %3 offen lds" ::"v"(vo), "s"(r), "s"(m0), "s"(so) : "memory");
  asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
  for (int i = l; i < 256; i += 64) out[i] = sm[2 + i];
  typedef unsigned u2v __attribute__((ext_vector_type(2)));
  u2v x;
  const unsigned a = base + 4 * (2 + 4 * (l & 62) + 3);   // odd dword address
  asm volatile("ds_read_b64 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(x) : "v"(a) : "memory");
  out[256 + 2 * l] = x[0];
  out[256 + 2 * l + 1] = x[1];
}

static int run_planar(const float* d) {
  unsigned* o;
  hipMalloc(&o, 384 * 4);
  int bad = 0;
  for (int so : {0, 1024}) {
    hipLaunchKernelGGL(probe_planar, dim3(1), dim3(64), 0, 0, d, 40 * 16, so, o);
    std::vector<unsigned> r(384);
    hipMemcpy(r.data(), o, 384 * 4, hipMemcpyDeviceToHost);
    int bad_data = 0, bad_zero = 0, bad_read = 0;
    // expected image: dword i of the piece = src[so / 4 + i] (= so / 4 + i + 1) for i < 160, else 0
    auto want = [&](int i) -> unsigned {
      const float v = (float)(so / 4 + i + 1);
      return i < 160 ? *reinterpret_cast<const unsigned*>(&v) : 0u;
    };
    for (int i = 0; i < 256; ++i) (i < 160 ? bad_data : bad_zero) += r[i] != want(i);
    for (int l = 0; l < 64; ++l)
      for (int q = 0; q < 2; ++q) {
        const int i = 4 * (l & 62) + 3 + q;   // dword of the piece
        bad_read += r[256 + 2 * l + q] != (i < 256 ? want(i) : 0xDEADBEEFu);
      }
    printf("planar piece, M0 = 8 (mod 16), soffset %d: in-range dwords wrong %d, out-of-range dwords not zero %d, "
           "odd-address ds_read_b64 words wrong %d\n", so, bad_data, bad_zero, bad_read);
    printf("  piece dwords 156..163: ");
    for (int i = 156; i < 164; ++i) printf("%g ", *reinterpret_cast<float*>(&r[i]));
    printf("\n");
    bad += bad_data + bad_zero + bad_read;
  }
  hipFree(o);
  return bad;
}

// The same piece with M0 = 4 and 12 (mod 16): dword-aligned only (the image one dword further, so that
// column -1 of a row lands on an even dword).  out[0..259]: sm[0..259].
__global__ void probe_m0_dword(const float* src, int nbytes, int m0_dwords, unsigned* out) {
  __shared__ __attribute__((aligned(16))) unsigned sm[1024];
  const int l = threadIdx.x;
  for (int i = l; i < 1024; i += 64) sm[i] = 0xDEADBEEFu;
  __syncthreads();
  __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc((void*)src, 0, nbytes, 0x00020000);
  const unsigned vo = l < 40 ? 16u * l : 0x80000000u;
  const unsigned base = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned*)sm;
  const unsigned m0 = __builtin_amdgcn_readfirstlane(base + 4 * m0_dwords);
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %1, %3 offen lds" ::"v"(vo), "s"(r), "s"(m0), "s"(0) : "memory");
  asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
  for (int i = l; i < 260; i += 64) out[i] = sm[i];
}

// Cost of the patch reads: 12 waves (the conv's workgroup), each lane 3 x ds_read_b64 per round at
// the conv's addresses — plane (lane >> 4) x 770 dwords + 4 (lane & 15) + shift — for shift 0 (8-byte
// aligned) and an odd shift.  out[wave] = cycles of `rounds` rounds.
__global__ void time_reads(int shift, int rounds, unsigned long long* out, unsigned* sink) {
  __shared__ __attribute__((aligned(16))) unsigned sm[4 * 770 + 64];
  for (int i = threadIdx.x; i < 4 * 770 + 64; i += blockDim.x) sm[i] = i;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const unsigned a = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned*)sm +
                     4 * ((lane >> 4) * 770 + 4 * (lane & 15) + shift);
  typedef unsigned u2v __attribute__((ext_vector_type(2)));
  unsigned acc = 0;
  const unsigned long long t0 = __builtin_amdgcn_s_memtime();
  for (int r = 0; r < rounds; ++r) {
    u2v x, y, z;
    asm volatile("ds_read_b64 %0, %3\n\tds_read_b64 %1, %3 offset:8\n\tds_read_b64 %2, %3 offset:16\n\ts_waitcnt lgkmcnt(0)"
                 : "=v"(x), "=v"(y), "=v"(z) : "v"(a) : "memory");
    acc += x[0] ^ y[1] ^ z[0];
  }
  const unsigned long long t1 = __builtin_amdgcn_s_memtime();
  if (lane == 0) out[threadIdx.x >> 6] = t1 - t0;
  if (acc == 0x12345678u) sink[0] = acc;
}

static int run_shift(const float* d) {
  unsigned* o;
  hipMalloc(&o, 260 * 4);
  int bad_total = 0;
  for (int sh : {1, 3}) {
    hipLaunchKernelGGL(probe_m0_dword, dim3(1), dim3(64), 0, 0, d, 40 * 16, sh, o);
    std::vector<unsigned> r(260);
    hipMemcpy(r.data(), o, 260 * 4, hipMemcpyDeviceToHost);
    int bad = 0;
    for (int i = 0; i < 256; ++i) {
      const float v = (float)(i + 1);
      bad += r[sh + i] != (i < 160 ? *reinterpret_cast<const unsigned*>(&v) : 0u);
    }
    for (int i = 0; i < sh; ++i) bad += r[i] != 0xDEADBEEFu;
    bad += r[sh + 256] != 0xDEADBEEFu;
    printf("dwordx4 piece, M0 = %d (mod 16): dwords wrong %d; sm[0..7] as float / hex:", 4 * sh, bad);
    for (int i = 0; i < 8; ++i) printf(" %g/%08x", *reinterpret_cast<float*>(&r[i]), r[i]);
    printf("\n");
    bad_total += bad;
  }
  hipFree(o);
  unsigned long long* t;
  unsigned* sink;
  hipMalloc(&t, 12 * 8);
  hipMalloc(&sink, 4);
  for (int pass = 0; pass < 2; ++pass)
    for (int sh : {0, 3, 1, 2}) {
      const int rounds = 2000;
      hipLaunchKernelGGL(time_reads, dim3(1), dim3(768), 0, 0, sh, rounds, t, sink);
      unsigned long long h[12];
      hipMemcpy(h, t, sizeof(h), hipMemcpyDeviceToHost);
      double s = 0;
      for (int w = 0; w < 12; ++w) s += (double)h[w];
      if (pass) printf("ds_read_b64 x 3 per round, 12 waves, dword shift %d: %.1f cycles per round per wave\n", sh, s / 12 / rounds);
    }
  hipFree(t);
  hipFree(sink);
  return bad_total;
}

int main() {
  const int n = 4096;
  std::vector<float> h(n);
  for (int i = 0; i < n; ++i) h[i] = (float)(i + 1);
  float* d;
  unsigned* o;
  hipMalloc(&d, n * 4 + 4096);
  hipMemcpy(d, h.data(), n * 4, hipMemcpyHostToDevice);
  hipMemset((char*)d + n * 4, 0x7f, 4096);   // bytes past num_records are NOT zero
  hipMalloc(&o, 512 * 4);
  for (int so : {0, 64}) {
    hipLaunchKernelGGL(probe, dim3(1), dim3(64), 0, 0, d, 256 * 4, so, o);
    std::vector<unsigned> r(512);
    hipMemcpy(r.data(), o, 512 * 4, hipMemcpyDeviceToHost);
    printf("soffset %d\n dword: ", so);
    int bad = 0;
    for (int l = 0; l < 64; ++l) {
      const float v = *reinterpret_cast<float*>(&r[l]);
      printf("%g%s", v, l % 16 == 15 ? "\n        " : " ");
      if (l >= 32 && r[l] != 0) ++bad;
    }
    printf("\n dwordx4 (first dword of each lane): ");
    for (int l = 0; l < 64; ++l) {
      const float v = *reinterpret_cast<float*>(&r[256 + 4 * l]);
      printf("%g%s", v, l % 16 == 15 ? "\n        " : " ");
      if (l >= 32) for (int q = 0; q < 4; ++q) bad += r[256 + 4 * l + q] != 0;
    }
    printf("\n out-of-range lanes not zero: %d\n", bad);
  }
  const int bad_planar = run_planar(d);
  run_shift(d);   // (reported, not part of the exit status: a question, not a reliance)
  hipFree(d);
  hipFree(o);
  return bad_planar ? 1 : 0;
}
