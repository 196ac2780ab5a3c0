// fmx_iq_estimate (fmx_wb_design.cpp, fmx_iqc.h) under ASan + UBSan: both
// formats at their extreme values (the int64 sums of a million full-scale
// int16 samples), buffers of exactly n samples on the heap, n = 1, the
// degenerate inputs and the refused arguments.  Built by the test with
// fmx_design.cpp (fmx_wb_design.cpp's other entries need firdes_kaiser);
// prints one JSON line.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "fmx.h"

int main() {
  int calls = 0, bad = 0;
  double sum = 0.0;
  fmx_iq_correction p;
  const long sizes[] = {1, 2, 7, 4097, 1000000};
  for (long n : sizes) {
    // int16: the extremes alternate, so every product reaches 2^30 in magnitude
    std::vector<int16_t> s(2 * n);
    for (long i = 0; i < n; ++i) {
      s[2 * i] = (i & 1) ? 32767 : -32768;
      s[2 * i + 1] = (i & 2) ? -32768 : 32767;
    }
    if (fmx_iq_estimate(s.data(), FMX_WB_S16, n, &p) != FMX_OK) ++bad;
    if (!(std::isfinite(p.dc_i) && std::isfinite(p.dc_q) && p.gain > 0.0 && std::isfinite(p.cross))) ++bad;
    sum += p.gain;
    ++calls;
    std::vector<uint8_t> b(2 * n);
    for (long i = 0; i < n; ++i) {
      b[2 * i] = (i % 3) ? 255 : 0;
      b[2 * i + 1] = static_cast<uint8_t>(37 * i);
    }
    if (fmx_iq_estimate(b.data(), FMX_WB_U8, n, &p) != FMX_OK) ++bad;
    if (!(std::isfinite(p.dc_i) && std::isfinite(p.dc_q) && p.gain > 0.0 && std::isfinite(p.cross))) ++bad;
    sum += p.gain;
    ++calls;
  }
  // all samples equal: no variance, gain 1 and cross 0, the DC exact
  std::vector<uint8_t> flat(2 * 100, 255);
  if (fmx_iq_estimate(flat.data(), FMX_WB_U8, 100, &p) != FMX_OK || p.gain != 1.0 || p.cross != 0.0 || p.dc_i != 1.0 ||
      p.dc_q != 1.0)
    ++bad;
  ++calls;
  int rejected = 0;
  rejected += fmx_iq_estimate(flat.data(), FMX_WB_U8, 0, &p) == FMX_E_INVALID;
  rejected += fmx_iq_estimate(flat.data(), FMX_WB_U8, -5, &p) == FMX_E_INVALID;
  rejected += fmx_iq_estimate(flat.data(), 2, 100, &p) == FMX_E_INVALID;
  rejected += fmx_iq_estimate(nullptr, FMX_WB_U8, 100, &p) == FMX_E_INVALID;
  rejected += fmx_iq_estimate(flat.data(), FMX_WB_U8, 100, nullptr) == FMX_E_INVALID;
  std::printf("{\"calls\": %d, \"bad\": %d, \"rejected\": %d, \"sum\": %.17g}\n", calls, bad, rejected, sum);
  return bad ? 1 : 0;
}
