// fmx_wb_design.cpp -- host-side design of the wideband channelizer
// (fmx_wb_*): geometry of one fmx_wb_config and the per-channel weight rows
// the kernel k_wb multiplies with.  Host-only C++: it
// compiles stand-alone with g++ beside fmx_design.cpp (firdes_kaiser).
//
// Channel weights W[k] = 2 fc h[k] exp(+j 2 pi f k / Fs), h = firdes_kaiser(L,
// fc, 80 dB) as ComplexDecimator::init designs it (liquid_primitives.cpp:
// 370-403) with fc = min(0.45 / D, 0.45) -- without the reference's lower
// clamp at 0.01, which above D = 45 would make the pass band wider than the
// output rate.  The phase comes from the integer (f k mod Fs) / Fs turns.
#include "fmx_internal.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace fmx {

static constexpr double kTwoPi = 6.283185307179586476925286766559;

// IEEE binary16 (round to nearest even) of a double already within range
static uint16_t wb_f16_bits(double v) {
  const uint16_t sign = std::signbit(v) ? 0x8000u : 0u;
  const double a = std::fabs(v);
  if (a == 0.0) return sign;
  int e;
  std::frexp(a, &e); // a = m 2^e, m in [0.5, 1)
  // spacing of the binary16 grid at a: 2^(e - 11), at least 2^-24 (subnormals)
  const int q = std::max(e - 11, -24);
  const double r = std::nearbyint(std::ldexp(a, -q)); // ties to even
  if (r == 0.0) return sign;
  const double back = std::ldexp(r, q);
  if (back >= 65520.0) return sign | 0x7C00u;
  int e2;
  std::frexp(back, &e2); // a carry may have moved it one binade up
  if (e2 - 1 < -14) return sign | static_cast<uint16_t>(std::ldexp(back, 24)); // subnormal
  const uint32_t mant = static_cast<uint32_t>(std::ldexp(back, 11 - e2)) - 0x400u; // 10 bits
  return sign | static_cast<uint16_t>(((e2 - 1 + 15) << 10) + mant);
}
static double wb_f16_value(uint16_t h) {
  const int e = (h >> 10) & 31;
  const double m = h & 0x3FFu;
  const double v = e == 0 ? std::ldexp(m, -24) : std::ldexp(m + 1024.0, e - 25);
  return (h & 0x8000u) ? -v : v;
}

int wb_plan(const fmx_wb_config &cfg, WbPlan *p, std::string *err) {
  auto fail = [&](const char *m) {
    if (err) *err = m;
    return FMX_E_INVALID;
  };
  if (cfg.dsp_rate <= 0 || cfg.wide_rate <= 0) return fail("fmx_wb: rates must be positive");
  if (cfg.wide_rate % cfg.dsp_rate != 0) return fail("fmx_wb: wide_rate must be an integer multiple of dsp_rate");
  const int D = cfg.wide_rate / cfg.dsp_rate;
  if (D < 2 || D > 128) return fail("fmx_wb: wide_rate / dsp_rate must be 2..128");
  const int tpp = cfg.taps_per_phase == 0 ? (D >= 8 ? 28 : (D >= 4 ? 20 : 12)) : cfg.taps_per_phase;
  if (tpp < 4 || tpp > 28) return fail("fmx_wb: taps_per_phase must be 0 or 4..28");
  if (cfg.format != FMX_WB_U8 && cfg.format != FMX_WB_S16) return fail("fmx_wb: unknown sample format");
  if (cfg.block < 1) return fail("fmx_wb: block must be at least 1");
  p->D = D;
  p->tpp = tpp;
  p->L = D * tpp;
  p->Lp = (p->L + 31) & ~31;
  p->fs = cfg.wide_rate;
  p->format = cfg.format;
  p->block = cfg.block;
  p->fc = std::min(0.45f / static_cast<float>(D), 0.45f);
  std::vector<float> h(p->L);
  firdes_kaiser(static_cast<unsigned>(p->L), p->fc, 80.0f, 0.0f, h.data());
  const double scale = static_cast<double>(2.0f * p->fc); // firdecim's scale, a float product as the reference's
  p->g.resize(p->L);
  double gmax = 0.0;
  for (int k = 0; k < p->L; ++k) {
    p->g[k] = scale * static_cast<double>(h[k]);
    gmax = std::max(gmax, std::fabs(p->g[k]));
  }
  if (!(gmax > 0.0)) return fail("fmx_wb: degenerate filter");
  // the largest |W| lands in [2^13, 2^14): both components stay below f16's
  // 65504, and a tap 2^-12 of the largest still has its lo half on f16's grid
  p->sexp = 13 - std::ilogb(gmax);
  return FMX_OK;
}

bool wb_freq_ok(const WbPlan &p, int freq_hz) {
  return 2 * static_cast<int64_t>(freq_hz) <= p.fs && 2 * static_cast<int64_t>(freq_hz) >= -static_cast<int64_t>(p.fs);
}

uint32_t wb_freq_mod(const WbPlan &p, int freq_hz) {
  int64_t m = static_cast<int64_t>(freq_hz) % p.fs;
  if (m < 0) m += p.fs;
  return static_cast<uint32_t>(m);
}

void wb_weight_rows(const WbPlan &p, int freq_hz, uint16_t *rows) {
  std::memset(rows, 0, sizeof(uint16_t) * 4 * p.Lp);
  const int64_t fm = wb_freq_mod(p, freq_hz);
  for (int k = 0; k < p.L; ++k) {
    const int64_t turns = (fm * k) % p.fs; // (f k mod Fs) / Fs turns, exact
    const double ph = kTwoPi * static_cast<double>(turns) / static_cast<double>(p.fs);
    const double w[2] = {std::ldexp(p.g[k] * std::cos(ph), p.sexp), std::ldexp(p.g[k] * std::sin(ph), p.sexp)};
    const int kk = p.Lp - 1 - k;
    for (int c = 0; c < 2; ++c) {
      const uint16_t hi = wb_f16_bits(w[c]);
      rows[(2 * c) * p.Lp + kk] = hi;
      rows[(2 * c + 1) * p.Lp + kk] = wb_f16_bits(w[c] - wb_f16_value(hi));
    }
  }
}

void wb_rows_to_taps(const WbPlan &p, const uint16_t *rows, float *out) {
  for (int k = 0; k < p.L; ++k) {
    const int kk = p.Lp - 1 - k;
    for (int c = 0; c < 2; ++c)
      out[2 * k + c] = static_cast<float>(
          std::ldexp(wb_f16_value(rows[(2 * c) * p.Lp + kk]) + wb_f16_value(rows[(2 * c + 1) * p.Lp + kk]), -p.sexp));
  }
}

int wb_scan_plan(const fmx_wb_scan_config &cfg, WbPlan *p, std::string *err) {
  auto fail = [&](const char *m) {
    if (err) *err = m;
    return FMX_E_INVALID;
  };
  const int rc = wb_plan(cfg.wb, p, err);
  if (rc != FMX_OK) return rc;
  if (cfg.step_hz < 1) return fail("fmx_wb_scan: step_hz must be at least 1");
  if (cfg.n_points < 1 || cfg.n_points > 8192) return fail("fmx_wb_scan: n_points must be 1..8192");
  const int64_t last = static_cast<int64_t>(cfg.start_hz) + static_cast<int64_t>(cfg.n_points - 1) * cfg.step_hz;
  if (2 * static_cast<int64_t>(cfg.start_hz) < -static_cast<int64_t>(p->fs) || 2 * last > p->fs)
    return fail("fmx_wb_scan: a point lies outside +- wide_rate / 2");
  return FMX_OK;
}

// The capture bank's work list (k_wbb): one group
// {capture, first channel, channels 1..16} per 16 channels of a capture, in
// channel order, none for an empty capture.  Returns the group count G, or
// FMX_E_INVALID for a bad table, FMX_E_CAPACITY for one of more than 65 535
// groups, or -G when out is NULL or cap < G (then nothing is written).
int wbb_groups(const int *first_channel, int n_captures, int *out, int cap) {
  if (!first_channel || n_captures < 1 || n_captures > FMX_WBB_CAPTURES_MAX || first_channel[0] != 0) return FMX_E_INVALID;
  int64_t G = 0;
  for (int s = 0; s < n_captures; ++s) {
    const int64_t n = static_cast<int64_t>(first_channel[s + 1]) - first_channel[s];
    if (n < 0) return FMX_E_INVALID;
    G += (n + 15) / 16;
  }
  if (G > FMX_WBB_GROUPS_MAX) return FMX_E_CAPACITY;
  if (G > 0 && (!out || cap < G)) return -static_cast<int>(G);
  int g = 0;
  for (int s = 0; s < n_captures; ++s)
    for (int c = first_channel[s]; c < first_channel[s + 1]; c += 16) {
      out[3 * g] = s;
      out[3 * g + 1] = c;
      out[3 * g + 2] = std::min(16, first_channel[s + 1] - c);
      ++g;
    }
  return g;
}

} // namespace fmx

extern "C" int fmx_wb_bank_groups(const int *first_channel, int n_captures, int *out, int cap) {
  return fmx::wbb_groups(first_channel, n_captures, out, cap);
}

extern "C" int fmx_wb_scan_points(const fmx_wb_scan_config *cfg, int *freq_hz, int cap) {
  if (!cfg) return FMX_E_INVALID;
  fmx::WbPlan p;
  const int rc = fmx::wb_scan_plan(*cfg, &p, nullptr);
  if (rc != FMX_OK) return rc;
  for (int k = 0; freq_hz && k < cfg->n_points && k < cap; ++k) freq_hz[k] = cfg->start_hz + k * cfg->step_hz;
  return cfg->n_points;
}

extern "C" int fmx_scan_peaks(const double *dbfs, int n, double min_dbfs, int min_spacing, int *idx, int cap) {
  if (n < 0 || min_spacing < 0 || (n > 0 && !dbfs)) return FMX_E_INVALID;
  int count = 0;
  for (int p = 0; p < n; ++p) {
    bool peak = dbfs[p] >= min_dbfs;
    for (int q = std::max(0, p - min_spacing); peak && q < p; ++q) peak = dbfs[p] > dbfs[q];
    for (int q = p + 1; peak && q < n && q - p <= min_spacing; ++q) peak = dbfs[p] >= dbfs[q];
    if (!peak) continue;
    if (idx && count < cap) idx[count] = p;
    ++count;
  }
  return count;
}

extern "C" int fmx_wb_weights(const fmx_wb_config *cfg, int freq_hz, float *out, int cap) {
  if (!cfg) return FMX_E_INVALID;
  fmx::WbPlan p;
  int rc = fmx::wb_plan(*cfg, &p, nullptr);
  if (rc != FMX_OK) return rc;
  if (!fmx::wb_freq_ok(p, freq_hz)) return FMX_E_INVALID;
  if (!out || cap < 2 * p.L) return 2 * p.L;
  std::vector<uint16_t> rows(static_cast<size_t>(4) * p.Lp);
  fmx::wb_weight_rows(p, freq_hz, rows.data());
  fmx::wb_rows_to_taps(p, rows.data(), out);
  return 2 * p.L;
}
