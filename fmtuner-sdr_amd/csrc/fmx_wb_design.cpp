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

// SR + j SI = sum_k W[k] of one channel, from the rows the kernel multiplies
// (hi + lo of every entry, units of W * 2^sexp): the corrected kernels'
// per-channel DC constant
void wb_tap_sums(const WbPlan &p, const uint16_t *rows, float *out2) {
  for (int c = 0; c < 2; ++c) {
    double s = 0.0;
    for (int k = 0; k < p.L; ++k) {
      const int kk = p.Lp - 1 - k;
      s += wb_f16_value(rows[(2 * c) * p.Lp + kk]) + wb_f16_value(rows[(2 * c + 1) * p.Lp + kk]);
    }
    out2[c] = static_cast<float>(s);
  }
}

// ---- rational rates ----
// wide_rate / dsp_rate = P / Q in lowest terms.  The prototype is designed at
// the up-sampled rate Q Fs: Lup = P tpp taps, fc = min(0.45 / P, 0.45), gain
// Q 2 fc.  Output n = Q m + r uses the taps h[Q j + b_r] on x[m P + a_r - j],
// r P = Q a_r + b_r: Q integer channelizers of decimation P.  With Q = 1 every
// number below is wb_plan's.
int wbr_plan(const fmx_wb_config &cfg, WbrPlan *p, std::string *err, bool taps) {
  auto fail = [&](const char *m) {
    if (err) *err = m;
    return FMX_E_INVALID;
  };
  if (cfg.dsp_rate <= 0 || cfg.wide_rate <= 0) return fail("fmx_wb: rates must be positive");
  int g = cfg.wide_rate, t = cfg.dsp_rate;
  while (t != 0) {
    const int u = g % t;
    g = t;
    t = u;
  }
  const int P = cfg.wide_rate / g, Q = cfg.dsp_rate / g;
  if (Q > FMX_WBR_QMAX) return fail("fmx_wb: wide_rate / dsp_rate = P / Q in lowest terms needs Q <= 16");
  if (P < 2 * Q || P > 128 * Q) return fail("fmx_wb: wide_rate / dsp_rate must be 2..128");
  const int tpp = cfg.taps_per_phase == 0 ? (P >= 8 * Q ? 28 : (P >= 4 * Q ? 20 : 12)) : cfg.taps_per_phase;
  if (tpp < 4 || tpp > 28) return fail("fmx_wb: taps_per_phase must be 0 or 4..28");
  if (cfg.format != FMX_WB_U8 && cfg.format != FMX_WB_S16) return fail("fmx_wb: unknown sample format");
  if (cfg.block < 1) return fail("fmx_wb: block must be at least 1");
  p->P = P;
  p->Q = Q;
  p->tpp = tpp;
  p->Lup = P * tpp;
  p->fs = cfg.wide_rate;
  p->format = cfg.format;
  p->block = cfg.block;
  p->Lh = 0;
  for (int r = 0; r < Q; ++r) {
    p->a[r] = r * P / Q;
    p->b[r] = r * P % Q;
    p->Lr[r] = (p->Lup - p->b[r] + Q - 1) / Q;
    p->Lh = std::max(p->Lh, p->Lr[r]);
  }
  p->Lp = (p->Lh + 31) & ~31;
  // one tile's window: 16 outputs P samples apart, the last phase's offset, Lp taps
  const int window = (wbr_window(P, p->a[Q - 1], p->Lp, 0, 0) + 7) & ~7;
  if (static_cast<long>(window) * (cfg.format == FMX_WB_S16 ? 8 : 4) > kWbLdsMax)
    return fail(cfg.format == FMX_WB_S16
                    ? "fmx_wb: one tile's window (15 P + a_{Q-1} + Lp int16 samples of 8 bytes) exceeds 80 KB of LDS"
                    : "fmx_wb: one tile's window (15 P + a_{Q-1} + Lp u8 samples of 4 bytes) exceeds 80 KB of LDS");
  p->fc = std::min(0.45f / static_cast<float>(P), 0.45f);
  if (!taps) return FMX_OK;
  std::vector<float> h(p->Lup);
  firdes_kaiser(static_cast<unsigned>(p->Lup), p->fc, 80.0f, 0.0f, h.data());
  const double scale = static_cast<double>(Q) * static_cast<double>(2.0f * p->fc);
  p->g.resize(p->Lup);
  // every k = Q j + b_r belongs to exactly one phase (b_r runs through all
  // residues): the largest |W| over every phase is the largest |g|
  double gmax = 0.0;
  for (int k = 0; k < p->Lup; ++k) {
    p->g[k] = scale * static_cast<double>(h[k]);
    gmax = std::max(gmax, std::fabs(p->g[k]));
  }
  if (!(gmax > 0.0)) return fail("fmx_wb: degenerate filter");
  p->sexp = 13 - std::ilogb(gmax);
  return FMX_OK;
}

void wbr_weight_rows(const WbrPlan &p, int freq_hz, uint16_t *rows) {
  std::memset(rows, 0, sizeof(uint16_t) * 4 * p.Lp * p.Q);
  int64_t fm = static_cast<int64_t>(freq_hz) % p.fs;
  if (fm < 0) fm += p.fs;
  for (int r = 0; r < p.Q; ++r) {
    uint16_t *rr = rows + static_cast<size_t>(4) * p.Lp * r;
    for (int j = 0; j < p.Lr[r]; ++j) {
      const double gk = p.g[p.Q * j + p.b[r]];
      const int64_t turns = (fm * j) % p.fs; // (f j mod Fs) / Fs turns, exact
      const double ph = kTwoPi * static_cast<double>(turns) / static_cast<double>(p.fs);
      const double w[2] = {std::ldexp(gk * std::cos(ph), p.sexp), std::ldexp(gk * std::sin(ph), p.sexp)};
      const int kk = p.Lp - 1 - j;
      for (int c = 0; c < 2; ++c) {
        const uint16_t hi = wb_f16_bits(w[c]);
        rr[(2 * c) * p.Lp + kk] = hi;
        rr[(2 * c + 1) * p.Lp + kk] = wb_f16_bits(w[c] - wb_f16_value(hi));
      }
    }
  }
}

void wbr_rows_to_taps(const WbrPlan &p, const uint16_t *rows, int phase, float *out) {
  const uint16_t *rr = rows + static_cast<size_t>(4) * p.Lp * phase;
  for (int j = 0; j < p.Lr[phase]; ++j) {
    const int kk = p.Lp - 1 - j;
    for (int c = 0; c < 2; ++c)
      out[2 * j + c] = static_cast<float>(
          std::ldexp(wb_f16_value(rr[(2 * c) * p.Lp + kk]) + wb_f16_value(rr[(2 * c + 1) * p.Lp + kk]), -p.sexp));
  }
}

int wbr_tiles(int P, int Q, int a_last, int Lp, int s16, int n_out) {
  const long cap = kWbLdsMax / (s16 ? 8 : 4); // samples of the window
  const long M = (n_out / Q + 15) / 16;       // blocks of 16 outputs per phase
  int nt = 0;
  // nt consecutive tiles span at most 1 + ceil((nt - 1) / Q) blocks (a workgroup starting at the last phase)
  for (int k = 1; k <= kWbNtMax && k <= M * Q; ++k) {
    const int span = 1 + (k - 1 + Q - 1) / Q;
    if (((static_cast<long>(wbr_window(P, a_last, Lp, 0, span - 1)) + 7) & ~7L) > cap) break;
    nt = k;
  }
  return nt;
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

// The bank scan's work list (k_bscan): one entry
// {capture, first point, points 1..64} per 64 points of a capture (a workgroup's
// four waves of 16), in point order, none for an empty capture.  Returns and
// errors as wbb_groups.
int bscan_groups(const int *first_point, int n_captures, int *out, int cap) {
  if (!first_point || n_captures < 1 || n_captures > FMX_WBB_CAPTURES_MAX || first_point[0] != 0) return FMX_E_INVALID;
  int64_t G = 0;
  for (int s = 0; s < n_captures; ++s) {
    const int64_t n = static_cast<int64_t>(first_point[s + 1]) - first_point[s];
    if (n < 0) return FMX_E_INVALID;
    G += (n + 63) / 64;
  }
  if (G > FMX_WBB_GROUPS_MAX) return FMX_E_CAPACITY;
  if (G > 0 && (!out || cap < G)) return -static_cast<int>(G);
  int g = 0;
  for (int s = 0; s < n_captures; ++s)
    for (int64_t c = first_point[s]; c < first_point[s + 1]; c += 64) {
      out[3 * g] = s;
      out[3 * g + 1] = static_cast<int>(c);
      out[3 * g + 2] = static_cast<int>(std::min<int64_t>(64, first_point[s + 1] - c));
      ++g;
    }
  return g;
}

} // namespace fmx

extern "C" int fmx_wb_bank_scan_groups(const int *first_point, int n_captures, int *out, int cap) {
  return fmx::bscan_groups(first_point, n_captures, out, cap);
}

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

extern "C" int fmx_iq_estimate(const void *h_raw, int format, long n_samples, fmx_iq_correction *out) {
  if (!h_raw || !out || n_samples <= 0 || (format != FMX_WB_U8 && format != FMX_WB_S16)) return FMX_E_INVALID;
  long long s[5] = {0, 0, 0, 0, 0};
  for (long i = 0; i < n_samples; ++i) {
    long long vi, vq;
    if (format == FMX_WB_S16) {
      vi = static_cast<const int16_t *>(h_raw)[2 * i];
      vq = static_cast<const int16_t *>(h_raw)[2 * i + 1];
    } else {
      vi = 2 * static_cast<int>(static_cast<const uint8_t *>(h_raw)[2 * i]) - 255;
      vq = 2 * static_cast<int>(static_cast<const uint8_t *>(h_raw)[2 * i + 1]) - 255;
    }
    s[0] += vi;
    s[1] += vq;
    s[2] += vi * vi;
    s[3] += vq * vq;
    s[4] += vi * vq;
  }
  FmxIqcBlock b{};
  fmx_iqc_finish(s, n_samples, 1.0, format == FMX_WB_S16 ? 32768.0 : 255.0, &b);
  *out = b.x;
  return FMX_OK;
}

extern "C" int fmx_wb_ratio(const fmx_wb_config *cfg, int *P, int *Q, int *taps) {
  if (!cfg) return FMX_E_INVALID;
  fmx::WbrPlan p;
  const int rc = fmx::wbr_plan(*cfg, &p, nullptr, false);
  if (rc != FMX_OK) return rc;
  if (P) *P = p.P;
  if (Q) *Q = p.Q;
  if (taps) *taps = p.Lh;
  return FMX_OK;
}

extern "C" int fmx_wb_weights_rational(const fmx_wb_config *cfg, int freq_hz, int phase, float *out, int cap) {
  if (!cfg) return FMX_E_INVALID;
  fmx::WbrPlan p;
  const int rc = fmx::wbr_plan(*cfg, &p, nullptr);
  if (rc != FMX_OK) return rc;
  if (phase < 0 || phase >= p.Q) return FMX_E_INVALID;
  if (2 * static_cast<int64_t>(freq_hz) > p.fs || 2 * static_cast<int64_t>(freq_hz) < -static_cast<int64_t>(p.fs))
    return FMX_E_INVALID;
  const int n = 2 * p.Lr[phase];
  if (!out || cap < n) return n;
  std::vector<uint16_t> rows(static_cast<size_t>(4) * p.Lp * p.Q);
  fmx::wbr_weight_rows(p, freq_hz, rows.data());
  fmx::wbr_rows_to_taps(p, rows.data(), phase, out);
  return n;
}

extern "C" int fmx_wb_rational_geometry(const fmx_wb_config *cfg, int n_out, int *out, int cap) {
  if (!cfg) return FMX_E_INVALID;
  fmx::WbrPlan p;
  const int rc = fmx::wbr_plan(*cfg, &p, nullptr, false);
  if (rc != FMX_OK) return rc;
  if (n_out < 1 || n_out % p.Q != 0 || n_out > p.block) return FMX_E_INVALID;
  const int s16 = p.format == FMX_WB_S16;
  const int nt = fmx::wbr_tiles(p.P, p.Q, p.a[p.Q - 1], p.Lp, s16, n_out);
  if (nt < 1) return FMX_E_INVALID;
  const int ntiles = (n_out / p.Q + 15) / 16 * p.Q;
  const int need = 6 + 4 * ntiles;
  if (!out || cap < need) return need;
  int wmax = 0;
  for (int T = 0; T < ntiles; ++T) {
    // the workgroup's frame and the tile's place in it, from the functions k_wbr itself calls
    const fmx::WbrGroup wg = fmx::wbr_group(T / nt, nt, ntiles, p.P, p.Q, p.a[p.Q - 1], p.Lp);
    const int r = T % p.Q;
    wmax = std::max(wmax, wg.window);
    int *o = out + 6 + 4 * T;
    o[0] = r;
    o[1] = p.a[r];
    o[2] = fmx::wbr_tile_offset(p.P, p.Q, p.a[r], T, wg.mb0);
    o[3] = wg.window;
  }
  out[0] = nt;
  out[1] = wmax;
  out[2] = ((wmax + 7) & ~7) * (s16 ? 8 : 4);
  out[3] = (ntiles + nt - 1) / nt;
  out[4] = ntiles;
  out[5] = p.Lp;
  return need;
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
