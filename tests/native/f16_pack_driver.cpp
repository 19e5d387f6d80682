// The host side of SEDX_PRECISION_F16 under ASan + UBSan, stand-alone: pack_f16 (weights.cpp) on seeded weights with
// the rounding's edge values planted in them, and the LDS slots that conv_f16.hip's fragment reads address
// (f16_geom.h), and prepare_weights with the fp16 packs beside the DevWeights regions.  The packs and slots are written
// as raw files into the directory given as argv[1]; tests/test_f16_cpu.py
// un-swizzles the packs by the layout weights.h documents and enumerates the slots per ds_read_b128 lane group.
//   w_<N>_<K>_<BN>.f32   the weights [N][K][9] as given to pack_f16
//   pk_<N>_<K>_<BN>.u16  pack_f16's image
//   lds.txt              one line per fragment read: "A|B F BN pool wave tile tap" and the 64 lanes' slots
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "host_check.h"

using namespace sedx;

// a whole synthetic state_dict of model m (random tensors, positive variances, a consistent windowed DFT and mel table)
static Params synth_params(const Model& m, uint32_t seed) {
  Params P;
  std::mt19937 rng(seed);
  std::normal_distribution<float> nd(0.f, 0.1f);
  for (const auto& kv : expected_params(m)) {
    Tensor t;
    t.shape = kv.second;
    size_t n = 1;
    for (int64_t d : t.shape) n *= (size_t)d;
    t.data.resize(n);
    const std::string& key = kv.first;
    const bool var = key.size() > 11 && key.compare(key.size() - 11, 11, "running_var") == 0;
    for (auto& v : t.data) v = var ? std::fabs(nd(rng)) + 0.5f : nd(rng);
    P[key] = std::move(t);
  }
  const int N = m.cfg.window_size, K = N / 2 + 1;
  auto& wr = P.at("spectrogram_extractor.stft.conv_real.weight").data;
  auto& wi = P.at("spectrogram_extractor.stft.conv_imag.weight").data;
  const double pi = 3.14159265358979323846;
  for (int k = 0; k < K; ++k)
    for (int n = 0; n < N; ++n) {
      const double win = 0.5 - 0.5 * std::cos(2.0 * pi * n / N), ang = 2.0 * pi * ((int64_t)k * n % N) / N;
      wr[(size_t)k * N + n] = (float)(std::cos(ang) * win);
      wi[(size_t)k * N + n] = (float)(-std::sin(ang) * win);
    }
  auto& mel = P.at("logmel_extractor.melW").data;
  const double step = (K - 1) / 65.0;
  for (int k = 0; k < K; ++k)
    for (int b = 0; b < 64; ++b) {
      const double v = 1.0 - std::fabs(k - (b + 1) * step) / step;
      mel[(size_t)k * 64 + b] = v > 0 ? (float)v : 0.f;
    }
  return P;
}

// prepare_weights with and without the fp16 packs: the same DevWeights regions either way, one aux region per packed
// conv layer (n_packed of them), 256-byte aligned, inside the image, overlapping nothing, bound with the others, and
// block 1's conv2 pack equal to pack_f16 of the folded weight after its one rounding to fp32
static void check_prepare(int model_type, int n_packed) {
  const Model m = model_of(model_type);
  const Params P = synth_params(m, 300 + model_type);
  DevWeights W0, W1;
  WeightBlob b0, b1;
  GammaGeom gg;
  std::string err;
  F16Weights f;
  CHECK(prepare_weights(m, P, &W0, &b0, &gg, &err) == SEDX_OK, "model %d: %s", model_type, err.c_str());
  CHECK(prepare_weights(m, P, &W1, &b1, &gg, &err, &f) == SEDX_OK, "model %d with f16: %s", model_type, err.c_str());
  CHECK(b0.aux.empty() && (int)b1.aux.size() == n_packed, "model %d: %zu / %zu aux regions", model_type, b0.aux.size(),
        b1.aux.size());
  CHECK(b0.regions.size() == b1.regions.size(), "model %d: the DevWeights regions changed", model_type);
  size_t aux_bytes = 0;
  for (const auto& r : b1.aux) {
    CHECK(r.off % 256 == 0 && r.bytes > 0 && r.off + r.bytes <= b1.image.size(), "aux region at %zu", r.off);
    aux_bytes += (r.bytes + 255) & ~size_t(255);
    for (const auto& q : b1.regions) CHECK(r.off + r.bytes <= q.off || q.off + q.bytes <= r.off, "aux overlaps a region");
    for (const auto& q : b1.aux) CHECK(&q == &r || r.off + r.bytes <= q.off || q.off + q.bytes <= r.off, "aux overlap");
  }
  CHECK(b1.image.size() == b0.image.size() + aux_bytes, "image %zu != %zu + %zu", b1.image.size(), b0.image.size(), aux_bytes);
  for (int i = 0; i < 8; ++i) CHECK(f.w[i] == nullptr, "f16 pointer %d set before bind", i);
  b1.bind(b1.image.data());
  int set = 0;
  for (int i = 0; i < 8; ++i) set += f.w[i] != nullptr;
  CHECK(set == n_packed && f.w[0] == nullptr && (f.w[1] != nullptr) == (n_packed > 0), "model %d: %d f16 pointers",
        model_type, set);
  for (const auto& r : b1.aux) CHECK(*r.dst == b1.image.data() + r.off, "bind");
  for (size_t i = 0; i < b0.regions.size(); ++i)
    CHECK(b0.regions[i].bytes == b1.regions[i].bytes &&
              std::memcmp(b0.image.data() + b0.regions[i].off, b1.image.data() + b1.regions[i].off, b0.regions[i].bytes) == 0,
          "region %zu differs with the f16 packs", i);
  if (!n_packed) return;   // (the VGGish trunk has no conv_block1)
  // block 1's conv2
  const auto& wt = P.at("conv_block1.conv2.weight").data;
  std::vector<float> wff((size_t)64 * 64 * 9);
  for (int o = 0; o < 64; ++o) {
    const double sc = (double)P.at("conv_block1.bn2.weight").data[o] /
                      std::sqrt((double)P.at("conv_block1.bn2.running_var").data[o] + 1e-5);
    for (int q = 0; q < 64 * 9; ++q) wff[(size_t)o * 576 + q] = (float)(wt[(size_t)o * 576 + q] * sc);
  }
  const std::vector<uint16_t> want = pack_f16(wff.data(), 64, 64, 9, 64);
  if (f.w[1]) CHECK(std::memcmp(f.w[1], want.data(), want.size() * 2) == 0, "model %d: block 1 conv2's fp16 pack", model_type);
}

static bool dump(const std::string& path, const void* p, size_t bytes) {
  FILE* f = std::fopen(path.c_str(), "wb");
  if (!f) return false;
  const bool ok = std::fwrite(p, 1, bytes, f) == bytes;
  return std::fclose(f) == 0 && ok;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::printf("usage: f16_pack_driver <output directory>\n");
    return 2;
  }
  const std::string dir = argv[1];
  const float inf = std::numeric_limits<float>::infinity();
  const float edge[] = {
      65504.f, -65504.f, 65519.99f, 65520.f, -65520.f, 1e6f, -3e38f, inf, -inf, 65503.99f, 65488.f /* tie below the clamp */,
      1.f + std::ldexp(1.f, -11), 1.f + 3 * std::ldexp(1.f, -11), -(1.f + std::ldexp(1.f, -11)), 2049.f, 2051.f,   // exact ties
      std::ldexp(1.f, -14) * (1.f - std::ldexp(1.f, -12)), -std::ldexp(1.f, -14) * (1.f - std::ldexp(1.f, -12)),
      std::ldexp(1.f, -14) * (1.f - std::ldexp(1.f, -11)) /* a tie that rounds up to 2^-14 */,
      std::ldexp(1.f, -14) * (1.f - std::ldexp(1.f, -10)) /* the largest subnormal */, std::ldexp(1.f, -14),
      -std::ldexp(1.f, -14), std::ldexp(1.f, -15), -std::ldexp(1.f, -15), 3e-6f, std::ldexp(1.f, -24), std::ldexp(1.f, -25),
      std::ldexp(1.5f, -25), 1e-40f, -1e-40f, 0.f, -0.f};
  const int n_edge = (int)(sizeof(edge) / sizeof(edge[0]));
  const int shapes[3][3] = {{64, 64, 64}, {128, 64, 128}, {512, 256, 128}};
  for (const auto& sh : shapes) {
    const int N = sh[0], K = sh[1], BN = sh[2];
    std::vector<float> w((size_t)N * K * 9);
    uint32_t st = 12345u + (uint32_t)N * 7 + (uint32_t)K;
    for (size_t i = 0; i < w.size(); ++i) {
      st = st * 1664525u + 1013904223u;
      const float u = (float)(st >> 8) * (1.0f / 16777216.0f) - 0.5f;   // [-0.5, 0.5)
      // a folded conv weight's range, with every 7th value small enough to meet the subnormal range
      w[i] = i % 7 == 3 ? u * 2e-4f : u * 0.2f;
    }
    // the edge values, spread so that every slot, swizzle phase and tap holds some
    for (size_t j = 0; j < w.size() / 97; ++j) w[j * 97] = edge[j % n_edge];
    const std::vector<uint16_t> pk = pack_f16(w.data(), N, K, 9, BN);
    CHECK(pk.size() == w.size(), "pack size %zu for %zu weights", pk.size(), w.size());
    // every weight at its documented index, and every element of the image written exactly once
    std::vector<char> seen(pk.size(), 0);
    for (int o = 0; o < N; ++o)
      for (int i = 0; i < K; ++i)
        for (int t = 0; t < 9; ++t) {
          const size_t at = f16_pack_index(K, 9, BN, o, i, t);
          CHECK(at < pk.size() && !seen[at], "index (%d, %d, %d)", o, i, t);
          if (at < pk.size()) {
            seen[at] = 1;
            CHECK(pk[at] == f16_q_bits(w[((size_t)o * K + i) * 9 + t]), "value (%d, %d, %d)", o, i, t);
          }
        }
    const std::string tag = std::to_string(N) + "_" + std::to_string(K) + "_" + std::to_string(BN);
    CHECK(dump(dir + "/w_" + tag + ".f32", w.data(), w.size() * 4), "write w_%s", tag.c_str());
    CHECK(dump(dir + "/pk_" + tag + ".u16", pk.data(), pk.size() * 2), "write pk_%s", tag.c_str());
  }

  // the kernel's instantiations: (F, BN, pooled epilogue); the frequency-mean epilogue reads as the un-pooled F = 8
  const int inst[6][3] = {{64, 64, 1}, {32, 128, 0}, {32, 128, 1}, {16, 128, 0}, {16, 128, 1}, {8, 128, 0}};
  FILE* f = std::fopen((dir + "/lds.txt").c_str(), "w");
  CHECK(f != nullptr, "open lds.txt");
  for (const auto& in : inst) {
    if (!f) break;
    const int F = in[0], BN = in[1];
    const bool pool = in[2] != 0;
    const int BM = f16_bm(BN), TT = BM / F, CSP = f16_csp(F, pool), waves_n = BN / 64, WM = BM / (8 / waves_n);
    CHECK(CSP >= F + 2, "row stride %d below the halo's %d columns", CSP, F + 2);
    const int a_slots = (TT + 2) * CSP * F16_REC_U4, w_slots = 3 * BN * 2;
    for (int wave = 0; wave < 8; ++wave) {
      const int wm = wave / waves_n, wn = wave % waves_n;
      for (int tile = 0; tile < 2; ++tile)
        for (int tap = 0; tap < 9; ++tap) {
          std::fprintf(f, "A %d %d %d %d %d %d", F, BN, (int)pool, wave, tile, tap);
          for (int lane = 0; lane < 64; ++lane) {
            const int slot = f16_aslot(F, pool, wm * WM + tile * 32 + (lane & 31), lane >> 5) +
                             ((tap / 3) * CSP + tap % 3) * F16_REC_U4;
            CHECK(slot >= 0 && slot < a_slots, "A slot %d outside the halo image of %d", slot, a_slots);
            std::fprintf(f, " %d", slot);
          }
          std::fprintf(f, "\nB %d %d %d %d %d %d", F, BN, (int)pool, wave, tile, tap);
          for (int lane = 0; lane < 64; ++lane) {
            const int slot = f16_wslot(wn * 64 + tile * 32 + (lane & 31), lane >> 5) + (tap % 3) * BN * 2;
            CHECK(slot >= 0 && slot < w_slots, "B slot %d outside the stage image of %d", slot, w_slots);
            std::fprintf(f, " %d", slot);
          }
          std::fprintf(f, "\n");
        }
    }
  }
  if (f) CHECK(std::fclose(f) == 0, "close lds.txt");

  check_prepare(SEDX_MODEL_GRU_FRAMEATT, 7);      // the 9-layer trunk: block 1's conv2 and blocks 2-4
  check_prepare(SEDX_MODEL_GRU14_FRAMEATT, 6);    // the 14-layer trunk: up to block 4's conv1
  check_prepare(SEDX_MODEL_VGGISH_FRAMEATT, 0);   // no packed layer
  return host_check::finish("f16_pack_driver");
}
