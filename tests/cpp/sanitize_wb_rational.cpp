// The rational-rate channelizer's host design (fmx_wb_design.cpp: fmx_wb_ratio,
// fmx_wb_weights_rational, fmx_wb_rational_geometry) under ASan + UBSan: every
// phase of the ratios people's receivers produce and of the geometry's edges
// (Q = 16, D = 2 and 128, 4 and 28 taps per phase) into heap blocks of exactly
// the size each call asks for, and the rejected ratios.  Built by the test
// with fmx_design.cpp (firdes_kaiser); prints one JSON line.
#include <cmath>
#include <cstdio>
#include <vector>

#include "fmx.h"

int main() {
  int calls = 0, bad = 0, tiles = 0;
  double sum = 0.0;
  // wide_rate, dsp_rate, taps_per_phase
  const int geo[][3] = {{20000000, 240000, 0}, {10000000, 240000, 0}, {2048000, 240000, 0}, {2000000, 240000, 0},
                        {600000, 240000, 12},  {10000000, 256000, 0}, {2400000, 240000, 0}, {33, 16, 4},
                        {1023, 8, 28},       {2, 1, 4},             {128, 1, 28}};
  for (const auto &g : geo) {
    for (int fmt = 0; fmt < 2; ++fmt) {
      fmx_wb_config cfg = {g[0], g[1], fmt, g[2], 4096};
      int P = 0, Q = 0, taps = 0;
      if (fmx_wb_ratio(&cfg, &P, &Q, &taps) != FMX_OK) {
        // 625 / 16 and 1023 / 8 at int16: one tile's window exceeds the LDS budget
        if (!(fmt == 1 && (g[1] == 256000 || g[0] == 1023))) ++bad;
        continue;
      }
      const int fs = cfg.wide_rate;
      const int freqs[] = {0, 123457 % (fs / 2 + 1), -fs / 2 + (fs > 2 ? 1 : 0), fs / 2};
      for (int f : freqs)
        for (int r = 0; r < Q; ++r) {
          const int n = fmx_wb_weights_rational(&cfg, f, r, nullptr, 0);
          if (n <= 0 || n > 2 * taps) {
            ++bad;
            continue;
          }
          std::vector<float> w(n);
          if (fmx_wb_weights_rational(&cfg, f, r, w.data(), n) != n) ++bad;
          for (float v : w) {
            if (!std::isfinite(v)) ++bad;
            sum += v;
          }
          ++calls;
        }
      const int outs[] = {Q, 16 * Q, 4095 - 4095 % Q};
      for (int n_out : outs) {
        const int need = fmx_wb_rational_geometry(&cfg, n_out, nullptr, 0);
        if (need < 6) {
          ++bad;
          continue;
        }
        std::vector<int> geo_out(need);
        if (fmx_wb_rational_geometry(&cfg, n_out, geo_out.data(), need) != need) ++bad;
        if (need != 6 + 4 * geo_out[4]) ++bad;
        tiles += geo_out[4];
        // one int short: the count comes back and nothing is written
        std::vector<int> small(need - 1, -7);
        if (fmx_wb_rational_geometry(&cfg, n_out, small.data(), need - 1) != need) ++bad;
        for (int v : small)
          if (v != -7) ++bad;
      }
      if (fmx_wb_weights_rational(&cfg, 0, Q, nullptr, 0) >= 0 || fmx_wb_weights_rational(&cfg, 0, -1, nullptr, 0) >= 0) ++bad;
      if (Q > 1 && fmx_wb_rational_geometry(&cfg, Q + 1, nullptr, 0) >= 0) ++bad;
      if (fmx_wb_rational_geometry(&cfg, 0, nullptr, 0) >= 0 || fmx_wb_rational_geometry(&cfg, 4096 + Q, nullptr, 0) >= 0) ++bad;
    }
  }
  // rejected before anything is built
  const fmx_wb_config wrong[] = {{2400001, 240000, 0, 0, 4096}, {240000, 240000, 0, 0, 4096}, {129 * 240000, 240000, 0, 0, 4096},
                                 {2049, 16, 0, 0, 4096},        {31, 16, 0, 0, 4096},         {100, 34, 0, 0, 4096},
                                 {35, 17, 0, 0, 4096},          {2000000, 240000, 0, 3, 4096}, {2000000, 240000, 0, 29, 4096},
                                 {2000000, 240000, 2, 0, 4096}, {2000000, 0, 0, 0, 4096},     {0, 240000, 0, 0, 4096},
                                 {2000000, 240000, 0, 0, 0},    {10000000, 256000, 1, 0, 4096}};
  int rejected = 0;
  for (const auto &c : wrong)
    if (fmx_wb_ratio(&c, nullptr, nullptr, nullptr) == FMX_E_INVALID) ++rejected;
  fmx_wb_config ok = {2000000, 240000, 1, 0, 4096};
  if (fmx_wb_weights_rational(&ok, 1000001, 0, nullptr, 0) < 0) ++rejected;
  if (fmx_wb_weights_rational(&ok, -1000001, 0, nullptr, 0) < 0) ++rejected;
  if (fmx_wb_ratio(nullptr, nullptr, nullptr, nullptr) < 0) ++rejected;
  std::printf("{\"calls\": %d, \"bad\": %d, \"rejected\": %d, \"tiles\": %d, \"sum\": %.9g}\n", calls, bad, rejected, tiles, sum);
  return bad ? 1 : 0;
}
