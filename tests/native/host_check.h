// What the host sanitizer drivers (asan_driver, deep14_driver, conformer14_driver, cnn14_driver, vggish_driver)
// share: CHECK and the failure count with its exit code, a Model from a model type, and the region predicates.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../sound-event-detection_amd/csrc/plan.h"
#include "../../sound-event-detection_amd/csrc/weights.h"

namespace host_check {
inline int failures = 0;
// "<driver>: clean" and 0, or the failure count and 1: what main returns
inline int finish(const char* driver) {
  if (failures) std::printf("%s: %d failures\n", driver, failures);
  else std::printf("%s: clean\n", driver);
  return failures ? 1 : 0;
}
}  // namespace host_check

#define CHECK(cond, ...)                               \
  do {                                                 \
    if (!(cond)) {                                     \
      ++host_check::failures;                          \
      std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
      std::printf(__VA_ARGS__);                        \
      std::printf("\n");                               \
    }                                                  \
  } while (0)

// the model of a 16 kHz configuration (k32: the 32 kHz preset: window 1024, hop 320)
inline sedx::Model model_of(int type, int classes = 25, int window = 512, int feature = SEDX_FEATURE_LOGMEL, bool k32 = false) {
  sedx_config cfg{};
  cfg.model_type = type;
  cfg.feature_type = feature;
  cfg.sample_rate = k32 ? 32000 : 16000, cfg.window_size = k32 ? 1024 : window, cfg.hop_size = k32 ? 320 : 160;
  cfg.mel_bins = 64, cfg.fmin = 50.f, cfg.fmax = k32 ? 14000.f : 7000.f, cfg.classes_num = classes;
  sedx::Model m;
  if (!sedx::make_model(cfg, &m)) {
    std::printf("FAIL make_model(%d)\n", type);
    std::exit(1);
  }
  return m;
}

inline bool disjoint(const sedx::Region& a, const sedx::Region& b) {
  return a.floats == 0 || b.floats == 0 || a.off + a.floats <= b.off || b.off + b.floats <= a.off;
}
inline bool inside(const sedx::Region& a, const sedx::Region& outer) {
  return a.off >= outer.off && a.off + a.floats <= outer.off + outer.floats;
}

struct Span {
  const char* name;
  size_t off, floats;   // float units
};
inline Span span(const char* name, const sedx::Region& r) { return Span{name, r.off, r.floats}; }
// every span 256-byte aligned and inside [lo, hi) floats, no two overlapping
inline void check_spans(const std::vector<Span>& v, size_t lo, size_t hi, const char* what) {
  for (size_t i = 0; i < v.size(); ++i) {
    CHECK(v[i].off * 4 % 256 == 0, "%s: %s at float %zu is not 256-byte aligned", what, v[i].name, v[i].off);
    CHECK(v[i].off >= lo && v[i].off + v[i].floats <= hi, "%s: %s [%zu, +%zu) outside [%zu, %zu)", what, v[i].name,
          v[i].off, v[i].floats, lo, hi);
    for (size_t j = 0; j < i; ++j)
      CHECK(v[i].off + v[i].floats <= v[j].off || v[j].off + v[j].floats <= v[i].off, "%s: %s overlaps %s", what,
            v[i].name, v[j].name);
  }
}
