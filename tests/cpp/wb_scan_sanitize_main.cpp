// The band scan's host-only entry points (fmx_wb_scan_points, fmx_scan_peaks
// in fmx_wb_design.cpp) under ASan + UBSan: plans at the edges of their
// conditions with output buffers of exactly cap elements, the rejections, and
// the peak picker on heap arrays of exactly n values with every spacing.
// Built by tests/test_wb_scan.py with fmx_design.cpp; prints one JSON line.
#include <climits>
#include <cstdio>
#include <vector>

#include "fmx.h"

int main() {
  int bad = 0, rejected = 0, peaks = 0;
  const int dsp = 240000;
  const fmx_wb_scan_config ok[] = {{{2400000, dsp, 1, 0, 4096}, -1100000, 100000, 23},
                                   {{2400000, dsp, 0, 0, 4096}, -1200000, 1, 8192},
                                   {{2400000, dsp, 0, 0, 4096}, 1200000 - 8191, 1, 8192},
                                   {{128 * dsp, dsp, 1, 28, 64}, -15360000, 30720000, 2},
                                   {{2 * dsp, dsp, 1, 4, 5}, 240000, 1, 1}};
  for (const auto &c : ok) {
    for (int cap : {0, 1, c.n_points - 1, c.n_points, c.n_points + 5}) {
      std::vector<int> f(cap > 0 ? cap : 0, INT_MIN);
      if (fmx_wb_scan_points(&c, cap > 0 ? f.data() : nullptr, cap) != c.n_points) ++bad;
      for (int k = 0; k < cap; ++k) {
        const bool written = k < c.n_points;
        if (written ? f[k] != c.start_hz + k * c.step_hz : f[k] != INT_MIN) ++bad;
      }
    }
  }
  const fmx_wb_scan_config wrong[] = {{{2400000, dsp, 1, 0, 4096}, 0, 0, 5},        {{2400000, dsp, 1, 0, 4096}, 0, -1, 5},
                                      {{2400000, dsp, 1, 0, 4096}, 0, 1, 0},        {{2400000, dsp, 1, 0, 4096}, 0, 1, 8193},
                                      {{2400000, dsp, 1, 0, 4096}, -1200001, 1, 2}, {{2400000, dsp, 1, 0, 4096}, 1200000, 1, 2},
                                      {{2400000, dsp, 1, 0, 4096}, INT_MAX, INT_MAX, 8192},
                                      {{2400000, dsp, 1, 0, 4096}, INT_MIN, 1, 1},  {{dsp, dsp, 1, 0, 4096}, 0, 1, 1},
                                      {{2400000, dsp, 1, 3, 4096}, 0, 1, 1},        {{2400000, dsp, 2, 0, 4096}, 0, 1, 1}};
  for (const auto &c : wrong)
    if (fmx_wb_scan_points(&c, nullptr, 0) < 0) ++rejected;
  if (fmx_wb_scan_points(nullptr, nullptr, 0) < 0) ++rejected;
  for (int n = 0; n <= 40; ++n) {
    std::vector<double> v(n);
    unsigned s = 12345u + n;
    for (double &x : v) {
      s = s * 1664525u + 1013904223u;
      x = -60.0 + (s >> 24) % 7 * 5.0; // many ties
    }
    for (int sp : {0, 1, 2, 39, 40, 41, INT_MAX}) {
      for (int cap : {0, 1, n}) {
        std::vector<int> idx(cap, -7);
        const int k = fmx_scan_peaks(n ? v.data() : nullptr, n, -45.0, sp, cap ? idx.data() : nullptr, cap);
        if (k < 0 || k > n) ++bad;
        for (int j = 0; j < cap; ++j) {
          if (j < k ? (idx[j] < 0 || idx[j] >= n || (j && idx[j] <= idx[j - 1])) : idx[j] != -7) ++bad;
        }
        peaks += k;
      }
    }
  }
  if (fmx_scan_peaks(nullptr, 3, 0.0, 1, nullptr, 0) < 0) ++rejected;
  if (fmx_scan_peaks(nullptr, -1, 0.0, 1, nullptr, 0) < 0) ++rejected;
  std::printf("{\"bad\": %d, \"rejected\": %d, \"peaks\": %d}\n", bad, rejected, peaks);
  return bad ? 1 : 0;
}
