// Host side of the ragged windowed driver under AddressSanitizer + UBSan (make asan-ragged): ragged_geometry,
// ragged_layout and ragged_tables swept over random lists of clip lengths, durations, overlap values and chunk
// sizes.  Every clip against window_geometry on that clip alone; every table read back the way the kernels
// address it (the frontend's item rows stay inside their clip, the merge's clip rows / off / src / div entries
// inside their tables, windows and frames inside the clip's items); the table regions inside the upload; the
// refusals, by clip index.  No GPU, no preload.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "host_check.h"

using namespace sedx;

static sedx_window_spec spec_of(int sd, int overlap, double ov) {
  sedx_window_spec s{};
  s.driver = SEDX_DRIVER_PREDICT, s.overlap = overlap, s.sample_duration = sd, s.vote = 0;
  s.overlap_value = ov, s.audio_duration = 0.0;
  return s;
}

static void check_case(const Model& m, const std::vector<int64_t>& len, const std::vector<double>* dur,
                       const sedx_window_spec& sp, int64_t per_forward, std::mt19937_64& rng) {
  const int64_t n = (int64_t)len.size();
  RaggedGeom rg;
  const char* why = ragged_geometry(m, len.data(), n, &sp, dur ? dur->data() : nullptr, &rg);
  // alone: every clip by window_geometry
  bool any_refused = false;
  std::vector<WinGeom> alone((size_t)n);
  for (int64_t c = 0; c < n; ++c) {
    sedx_window_spec s1 = sp;
    s1.audio_duration = dur && (*dur)[c] > 0 ? (*dur)[c] : 0.0;
    const bool refused = window_geometry(m, len[c], &s1, true, &alone[c]) != nullptr ||
                         len[c] < (int64_t)sp.sample_duration * m.cfg.sample_rate;
    if (refused && !any_refused) {
      char want[32];
      snprintf(want, sizeof(want), "clip %lld:", (long long)c);
      CHECK(why && std::strstr(why, want) == why, "first refused clip %lld: %s", (long long)c, why ? why : "accepted");
    }
    any_refused = any_refused || refused;
  }
  CHECK((why != nullptr) == any_refused, "refusal: %s", why ? why : "accepted");
  if (why) return;
  const int C = m.cfg.classes_num;
  CHECK((int64_t)rg.n_win.size() == n && (int64_t)rg.frame_off.size() == n + 1 && rg.frame_off[0] == 0 &&
            rg.item_off[0] == 0, "sizes");
  for (int64_t c = 0; c < n; ++c) {
    CHECK(rg.n_win[c] == alone[c].n_win && rg.frame_off[c + 1] - rg.frame_off[c] == alone[c].plan.N &&
              rg.item_off[c + 1] - rg.item_off[c] == alone[c].n_win && rg.full_len == alone[c].full_len,
          "clip %lld against window_geometry alone", (long long)c);
    const MergePlan& p = rg.plans[rg.plan_of[c]];
    CHECK(p.N == alone[c].plan.N && p.off == alone[c].plan.off && p.src == alone[c].plan.src &&
              p.div == alone[c].plan.div && p.win_base == alone[c].plan.win_base,
          "clip %lld's shared plan is not its own", (long long)c);
    CHECK(rg.g.out_frames == alone[c].groups[0].g.out_frames && rg.g.T == alone[c].groups[0].g.T, "item geometry");
  }
  const RaggedLayout l = ragged_layout(m, Tuning{}, rg, per_forward);
  CHECK(l.items == rg.item_off[n] && l.chunk >= 1 && l.chunk <= l.items && (per_forward <= 0 || l.chunk <= per_forward),
        "chunk %lld of %lld items", (long long)l.chunk, (long long)l.items);
  CHECK(l.fw * 4 >= l.model_bytes && l.clipwise >= l.fw + (size_t)l.items * rg.g.out_frames * C &&
            l.tables >= l.clipwise + (size_t)l.chunk * C && l.total_bytes == l.tables * 4 + l.table_bytes,
        "the area's order");
  const size_t ends[5][2] = {{l.t_item, sizeof(ItemRow) * (size_t)l.items},
                             {l.t_clip, sizeof(RaggedClipRow) * (size_t)(n + 1)},
                             {l.t_off, 4 * l.n_off},
                             {l.t_src, 8 * l.n_src},
                             {l.t_div, 4 * l.n_off}};
  for (int i = 0; i < 5; ++i) {
    CHECK(ends[i][0] % 256 == 0 && ends[i][0] + ends[i][1] <= l.table_bytes, "table %d outside the upload", i);
    if (i) CHECK(ends[i - 1][0] + ends[i - 1][1] <= ends[i][0], "table %d overlaps table %d", i, i - 1);
  }
  // clips back to back at random (odd) offsets
  std::vector<int64_t> clip_off((size_t)n + 1);
  clip_off[0] = (int64_t)(rng() % 7);
  for (int64_t c = 0; c < n; ++c) clip_off[c + 1] = clip_off[c] + len[c];
  std::vector<char> blob;
  ragged_tables(rg, l, clip_off.data(), &blob);
  CHECK(blob.size() == l.table_bytes, "blob size");
  if (blob.size() != l.table_bytes) return;
  const ItemRow* item = reinterpret_cast<const ItemRow*>(blob.data() + l.t_item);
  const RaggedClipRow* crow = reinterpret_cast<const RaggedClipRow*>(blob.data() + l.t_clip);
  const int32_t* off = reinterpret_cast<const int32_t*>(blob.data() + l.t_off);
  const int32_t* src = reinterpret_cast<const int32_t*>(blob.data() + l.t_src);
  const int32_t* div = reinterpret_cast<const int32_t*>(blob.data() + l.t_div);
  CHECK(crow[n].frame0 == rg.frame_off[n], "the closing clip row");
  for (int64_t c = 0; c < n; ++c) {
    const RaggedClipRow r = crow[c];
    CHECK(r.frame0 == rg.frame_off[c] && r.item0 == rg.item_off[c] && crow[c + 1].frame0 > r.frame0, "clip row %lld",
          (long long)c);
    const int64_t N = crow[c + 1].frame0 - r.frame0;
    bool ok = r.off0 >= 0 && (size_t)r.off0 + (size_t)N + 1 <= l.n_off && r.src0 >= 0 && (size_t)r.src0 <= l.n_src;
    CHECK(ok, "clip %lld's table bases", (long long)c);
    if (!ok) continue;
    for (int64_t f = 0; f < N && ok; ++f) {
      const int32_t j0 = off[r.off0 + f], j1 = off[r.off0 + f + 1];
      ok = ok && j0 >= 0 && j0 < j1 && (size_t)r.src0 + (size_t)j1 <= l.n_src && div[r.off0 + f] >= 1;
      for (int32_t j = j0; j < j1 && ok; ++j) {
        const int32_t w = src[2 * (r.src0 + j)], t = src[2 * (r.src0 + j) + 1];
        ok = w >= 0 && w < rg.n_win[c] && t >= 0 && t < rg.g.out_frames;
      }
    }
    CHECK(ok, "clip %lld: a merge table entry out of range", (long long)c);
    for (int32_t w = 0; w < rg.n_win[c]; ++w) {
      const ItemRow it = item[r.item0 + w];
      const int64_t st = alone[c].loop.start[w];
      CHECK(it.avail >= 0 && it.avail <= rg.full_len && it.src >= clip_off[c] && it.src + it.avail <= clip_off[c + 1],
            "clip %lld window %d reads outside its clip", (long long)c, w);
      CHECK(it.avail == std::min<int64_t>(rg.full_len, std::max<int64_t>(0, len[c] - st)) &&
                (it.avail == 0 || it.src == clip_off[c] + st), "clip %lld window %d: source", (long long)c, w);
    }
  }
}

static void check_refusals(const Model& m) {
  RaggedGeom rg;
  const int64_t len[3] = {80000, 79999, 112001};
  sedx_window_spec sp = spec_of(5, 1, 1.0);
  const char* why = ragged_geometry(m, len, 3, &sp, nullptr, &rg);
  CHECK(why && std::strstr(why, "clip 1:") == why, "a 79,999-sample clip in the middle: %s", why ? why : "accepted");
  CHECK(!ragged_geometry(m, len, 1, &sp, nullptr, &rg) && rg.n_win[0] == 1, "one clip");
  CHECK(ragged_geometry(m, len, 0, &sp, nullptr, &rg) && ragged_geometry(m, nullptr, 3, &sp, nullptr, &rg) &&
            ragged_geometry(m, len, 1, nullptr, nullptr, &rg), "no clips / null arrays");
  sp.driver = SEDX_DRIVER_MAIN_STRONG;
  CHECK(ragged_geometry(m, len, 1, &sp, nullptr, &rg), "main_strong");
  sp = spec_of(5, 1, 1.0), sp.vote = 1;
  CHECK(ragged_geometry(m, len, 1, &sp, nullptr, &rg), "vote");
  sp = spec_of(5, 1, 1.0), sp.audio_duration = 5.0;
  CHECK(ragged_geometry(m, len, 1, &sp, nullptr, &rg), "audio_duration in the spec");
  sp = spec_of(5, 1, 0.001);   // int(100 * overlap_value) == 0: avg_merge raises
  why = ragged_geometry(m, len, 1, &sp, nullptr, &rg);
  CHECK(why && std::strstr(why, "clip 0:") == why, "a zero merge step: %s", why ? why : "accepted");
}

int main() {
  std::mt19937_64 rng(20240611);
  const Model models[3] = {model_of(SEDX_MODEL_GRU_FRAMEATT), model_of(SEDX_MODEL_TRANSFORMER_FRAMEATT),
                           model_of(SEDX_MODEL_GRU_FRAMEATT, 25, 512, SEDX_FEATURE_LOGMEL, true)};
  check_refusals(models[0]);
  check_refusals(models[1]);
  const double ovs[4] = {1.0, 0.5, 2.0, 0.37};
  for (int it = 0; it < 160; ++it) {
    const Model& m = models[it % 3];
    const int sr = m.cfg.sample_rate;
    const int sd = 1 + (int)(rng() % 6);
    const int64_t n = 1 + (int64_t)(rng() % 9);
    std::vector<int64_t> len((size_t)n);
    std::vector<double> dur((size_t)n);
    for (int64_t c = 0; c < n; ++c) {
      // mostly runnable clips of sd .. sd + 20 s, odd lengths; now and then a short one
      len[c] = (int64_t)sd * sr + (int64_t)(rng() % ((uint64_t)20 * sr));
      if (rng() % 23 == 0) len[c] = (int64_t)(rng() % ((uint64_t)sd * sr));
      // loop bounds a little off the decoded length, some running past the samples
      dur[c] = rng() % 3 ? 0.0 : (double)len[c] / sr + ((double)(rng() % 2000) - 1000.0) / 1000.0;
    }
    const sedx_window_spec sp = spec_of(sd, (int)(rng() % 2), ovs[rng() % 4]);
    const int64_t per = (int64_t)(rng() % 4 == 0 ? 0 : 1 + rng() % 12);
    check_case(m, len, rng() % 2 ? &dur : nullptr, sp, per, rng);
  }
  return host_check::finish("ragged_driver");
}
