// fmx_synth_band.cpp -- the synthetic FM band on the host (fmx.h; definition in
// fmx_synth_band.h): what the band calls refuse, the
// content config, and fmx_synth_band_host, which takes every residue
// turn(f, i) straight from the definition (a 64-bit product and remainder per
// tone and sample).  Plain C++17, no HIP.
#include <cmath>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "fmx_synth_band.h"

namespace fmx {

void synth_band_content(const fmx_synth_band_config &cfg, fmx_synth_config *out) {
  std::memset(out, 0, sizeof(*out));
  out->iq_rate = cfg.wide_rate;
  out->kind = cfg.kind;
  out->amplitude = 1.0f;
  out->noise_std = 0.0f;
  out->seed_base = cfg.seed_base;
  out->max_offset_hz = cfg.max_offset_hz;
  out->rds_level = cfg.rds_level;
  out->n_bits = cfg.n_bits;
  out->level_spread_db = 0.0f;
}

static int refuse(const char *who, const char *what, std::string *err) {
  if (err) *err = std::string(who) + ": " + what;
  return FMX_E_INVALID;
}

static const char *config_refused(const fmx_synth_band_config &c) {
  if (c.wide_rate < FMX_SB_RATE_MIN || c.wide_rate > FMX_SB_RATE_MAX) return "wide_rate must be 480000..30720000";
  if (c.format != FMX_WB_U8 && c.format != FMX_WB_S16) return "format must be FMX_WB_U8 or FMX_WB_S16";
  if (c.kind < FMX_SYNTH_MONO || c.kind > FMX_SYNTH_STEREO_RDS) return "kind must be 0, 1 or 2";
  if (c.max_offset_hz < 0 || 2 * static_cast<int64_t>(c.max_offset_hz) > c.wide_rate)
    return "max_offset_hz must be 0..wide_rate / 2";
  if (!std::isfinite(c.rds_level)) return "rds_level is not finite";
  if (!(std::isfinite(c.noise_std) && c.noise_std >= 0.0f)) return "noise_std must be finite and >= 0";
  if (c.kind == FMX_SYNTH_STEREO_RDS && (c.n_bits < 104 || c.n_bits > FMX_SB_NBITS_MAX))
    return "kind 2 needs 104 <= n_bits <= 2^24";
  return nullptr;
}

int synth_band_check(const char *who, const fmx_synth_band_config *cfg, int n_captures, const int *first_station,
                     const fmx_synth_station *stations, const fmx_synth_frontend *frontends, const uint8_t *h_bits,
                     std::string *err) {
  if (!cfg || !first_station) return refuse(who, "null argument", err);
  if (const char *bad = config_refused(*cfg)) return refuse(who, bad, err);
  if (n_captures < 1 || n_captures > FMX_SB_CAPTURES_MAX) return refuse(who, "n_captures must be 1..1024", err);
  bool ok = first_station[0] == 0;
  for (int s = 0; ok && s < n_captures; ++s) ok = first_station[s + 1] >= first_station[s];
  if (!ok) return refuse(who, "first_station must start at 0 and not decrease", err);
  const int G = first_station[n_captures];
  if (G > FMX_SB_STATIONS_MAX) return refuse(who, "the captures' stations must be 0..8192 in all", err);
  if (G > 0 && !stations) return refuse(who, "null station table", err);
  if (G > 0 && cfg->kind == FMX_SYNTH_STEREO_RDS && !h_bits) return refuse(who, "kind 2 needs the RDS bit table", err);
  for (int g = 0; g < G; ++g) {
    const int64_t f = stations[g].freq_hz;
    if (2 * ((f < 0 ? -f : f) + cfg->max_offset_hz) > cfg->wide_rate) {
      if (err) *err = std::string(who) + ": station " + std::to_string(g) + ": |freq_hz| + max_offset_hz exceeds wide_rate / 2";
      return FMX_E_INVALID;
    }
    if (!(std::isfinite(stations[g].amplitude) && stations[g].amplitude >= 0.0f)) {
      if (err) *err = std::string(who) + ": station " + std::to_string(g) + ": amplitude must be finite and >= 0";
      return FMX_E_INVALID;
    }
  }
  if (frontends)
    for (int s = 0; s < n_captures; ++s) {
      const fmx_synth_frontend &f = frontends[s];
      if (!(std::isfinite(f.dc_i) && std::isfinite(f.dc_q) && std::isfinite(f.q_gain) && std::isfinite(f.q_cross))) {
        if (err) *err = std::string(who) + ": front end " + std::to_string(s) + " is not finite";
        return FMX_E_INVALID;
      }
      if (!(f.q_gain > 0.0)) {
        if (err) *err = std::string(who) + ": front end " + std::to_string(s) + ": q_gain must be > 0";
        return FMX_E_INVALID;
      }
    }
  return FMX_OK;
}

int synth_band_window(const char *who, int64_t sample0, int n_samples, size_t wide_stride, std::string *err) {
  if (sample0 < 0) return refuse(who, "sample0 must be >= 0", err);
  if (n_samples < 0) return refuse(who, "n_samples must be >= 0", err);
  if (sample0 > FMX_SB_SAMPLE_END - n_samples) return refuse(who, "sample0 + n_samples exceeds 2^40", err);
  if (wide_stride < static_cast<size_t>(n_samples)) return refuse(who, "wide_stride is less than n_samples", err);
  return FMX_OK;
}

} // namespace fmx

using namespace fmx;

namespace {
thread_local std::string t_err;

// one sample of capture s: stations [g0, g1) of st, residues from the definition
template <typename T>
void host_sample(const fmx_synth_band_config &cfg, const fmx_sb_station *st, int g0, int g1, const uint8_t *bits,
                 const double *fe, uint64_t nbase, double krds, int64_t i, T *out2) {
  const int64_t fs = cfg.wide_rate;
  const double fsd = static_cast<double>(fs);
  const uint64_t im = static_cast<uint64_t>(i % fs);
  double vi = 0.0, vq = 0.0;
  for (int g = g0; g < g1; ++g) {
    const fmx_sb_station &q = st[g];
    uint32_t r[FMX_SB_RES];
    for (int m = 0; m < FMX_SB_R57; ++m) r[m] = static_cast<uint32_t>((q.fm[m] * im) % static_cast<uint64_t>(fs));
    double rds = 0.0;
    r[FMX_SB_R57] = 0;
    if (cfg.kind == FMX_SYNTH_STEREO_RDS) {
      const int64_t nr = i + q.rds_off;
      const int64_t h = (2375 * nr) / fs;
      const int bit = bits[static_cast<size_t>(g) * cfg.n_bits + static_cast<size_t>((h >> 1) % cfg.n_bits)];
      rds = fmx_sb_rds_sign(bit, static_cast<int>(h & 1));
      r[FMX_SB_R57] = static_cast<uint32_t>((q.fm[FMX_SB_R57] * static_cast<uint64_t>(nr % fs)) % static_cast<uint64_t>(fs));
    }
    fmx_sb_add(q.amp, fmx_sb_phi(cfg.kind, q.k, q.c0, q.ph, r, fsd, rds, krds), &vi, &vq);
  }
  if (cfg.noise_std > 0.0f) fmx_sb_noise(static_cast<double>(cfg.noise_std), nbase, i, &vi, &vq);
  fmx_sb_frontend(fe, &vi, &vq);
  if (sizeof(T) == 2) {
    out2[0] = static_cast<T>(fmx_sb_quant_s16(vi));
    out2[1] = static_cast<T>(fmx_sb_quant_s16(vq));
  } else {
    out2[0] = static_cast<T>(fmx_sb_quant_u8(vi));
    out2[1] = static_cast<T>(fmx_sb_quant_u8(vq));
  }
}
} // namespace

extern "C" {

const char *fmx_synth_band_error(void) { return t_err.c_str(); }

int fmx_synth_band_tile(void) { return SB_TILE; }

int fmx_synth_band_content(const fmx_synth_band_config *cfg, fmx_synth_config *out) {
  if (!cfg || !out) return refuse("fmx_synth_band_content", "null argument", &t_err);
  synth_band_content(*cfg, out);
  return FMX_OK;
}

int fmx_synth_band_host(const fmx_synth_band_config *cfg, uint32_t ch0, int n_captures, const int *first_station,
                        const fmx_synth_station *stations, const fmx_synth_frontend *frontends, int64_t sample0,
                        int n_samples, const uint8_t *h_bits, void *h_out, size_t wide_stride, int threads) {
  const char *who = "fmx_synth_band_host";
  int rc = synth_band_check(who, cfg, n_captures, first_station, stations, frontends, h_bits, &t_err);
  if (rc != FMX_OK) return rc;
  if ((rc = synth_band_window(who, sample0, n_samples, wide_stride, &t_err)) != FMX_OK) return rc;
  if (n_samples == 0) return FMX_OK;
  if (!h_out) return refuse(who, "null output", &t_err);
  fmx_synth_config content;
  synth_band_content(*cfg, &content);
  const int G = first_station[n_captures];
  std::vector<fmx_sb_station> st(static_cast<size_t>(G));
  for (int g = 0; g < G; ++g)
    fmx_sb_derive(&content, ch0 + static_cast<uint32_t>(g), stations[g].freq_hz, stations[g].amplitude, &st[g]);
  const double krds = fmx_sb_krds(cfg->rds_level);
  // work items: runs of 256 samples of one capture, dealt to the threads in turn
  const int runs = (n_samples + 255) / 256;
  const long items = static_cast<long>(runs) * n_captures;
  if (threads < 1) threads = 1;
  if (threads > items) threads = static_cast<int>(items);
  auto work = [&](int t) {
    for (long it = t; it < items; it += threads) {
      const int s = static_cast<int>(it / runs), run = static_cast<int>(it % runs);
      const int n0 = run * 256, n1 = n0 + 256 < n_samples ? n0 + 256 : n_samples;
      const double ident[4] = {0.0, 0.0, 1.0, 0.0};
      const double fe[4] = {frontends ? frontends[s].dc_i : ident[0], frontends ? frontends[s].dc_q : ident[1],
                            frontends ? frontends[s].q_gain : ident[2], frontends ? frontends[s].q_cross : ident[3]};
      const uint64_t nbase = fmx_sb_noise_base(cfg->seed_base, s);
      const size_t row = static_cast<size_t>(s) * wide_stride;
      for (int n = n0; n < n1; ++n) {
        const size_t cell = 2 * (row + static_cast<size_t>(n));
        if (cfg->format == FMX_WB_S16)
          host_sample(*cfg, st.data(), first_station[s], first_station[s + 1], h_bits, fe, nbase, krds, sample0 + n,
                      static_cast<int16_t *>(h_out) + cell);
        else
          host_sample(*cfg, st.data(), first_station[s], first_station[s + 1], h_bits, fe, nbase, krds, sample0 + n,
                      static_cast<uint8_t *>(h_out) + cell);
      }
    }
  };
  std::vector<std::thread> th;
  for (int t = 1; t < threads; ++t) th.emplace_back(work, t);
  work(0);
  for (auto &x : th) x.join();
  return FMX_OK;
}

} // extern "C"
