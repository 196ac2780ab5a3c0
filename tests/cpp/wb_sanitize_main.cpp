// The wideband channelizer's host weight builder (fmx_wb_design.cpp) under
// ASan + UBSan: every configuration of tests/test_wb_design.py's weight test
// through fmx_wb_weights, the error cases, and the edges of the geometry
// (D = 2 and 128, 4 and 28 taps per phase).  Built by the test with
// fmx_design.cpp (firdes_kaiser); prints one JSON line.
#include <cmath>
#include <cstdio>
#include <vector>

#include "fmx.h"

int main() {
  const int dsp = 240000;
  int calls = 0, bad = 0;
  double sum = 0.0;
  const int geo[][2] = {{10, 0}, {25, 0}, {100, 0}, {2, 4}, {2, 28}, {128, 4}, {128, 28}, {45, 20}, {3, 7}};
  for (const auto &g : geo) {
    for (int fmt = 0; fmt < 2; ++fmt) {
      fmx_wb_config cfg = {g[0] * dsp, dsp, fmt, g[1], 4096};
      const int fs = cfg.wide_rate;
      const int freqs[] = {0, 123457 % (fs / 2), -fs / 2 + 1, fs / 2, -fs / 2, 1, -1};
      for (int f : freqs) {
        const int n = fmx_wb_weights(&cfg, f, nullptr, 0);
        if (n <= 0) {
          ++bad;
          continue;
        }
        std::vector<float> w(n);
        if (fmx_wb_weights(&cfg, f, w.data(), n) != n) ++bad;
        for (float v : w) {
          if (!std::isfinite(v)) ++bad;
          sum += v;
        }
        ++calls;
      }
    }
  }
  // rejected before anything is built
  const fmx_wb_config wrong[] = {{2400001, dsp, 0, 0, 4096}, {dsp, dsp, 0, 0, 4096},   {129 * dsp, dsp, 0, 0, 4096},
                                 {2400000, dsp, 0, 3, 4096}, {2400000, dsp, 0, 29, 4096}, {2400000, dsp, 2, 0, 4096},
                                 {2400000, 0, 0, 0, 4096},   {2400000, dsp, 0, 0, 0}};
  int rejected = 0;
  for (const auto &c : wrong)
    if (fmx_wb_weights(&c, 0, nullptr, 0) < 0) ++rejected;
  fmx_wb_config ok = {2400000, dsp, 1, 0, 4096};
  if (fmx_wb_weights(&ok, 1200001, nullptr, 0) < 0) ++rejected;
  if (fmx_wb_weights(&ok, -1200001, nullptr, 0) < 0) ++rejected;
  if (fmx_wb_weights(nullptr, 0, nullptr, 0) < 0) ++rejected;
  std::printf("{\"calls\": %d, \"bad\": %d, \"rejected\": %d, \"sum\": %.9g}\n", calls, bad, rejected, sum);
  return bad ? 1 : 0;
}
