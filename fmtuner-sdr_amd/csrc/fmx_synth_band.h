// fmx_synth_band.h -- synthetic FM band: wide captures of many stations
// (host + device).
//
// A band is n_captures captures of one rate Fs and one format; capture s holds
// the stations [first_station[s], first_station[s + 1]).  Station g's content
// is channel ch0 + g of fmx_synth.h's generator at iq_rate = Fs, and the sample
// at the absolute index i is
//
//   turn(f, i) = ((f mod Fs)(i mod Fs)) mod Fs          exact integer, >= 0
//   A(f, i)    = 2 pi turn(f, i) / Fs
//   Isin(a, f, ph) = (75000 a / f)(cos ph - cos(A(f, i) + ph))
//   Icos(a, f, ph) = (75000 a / f)(sin(A(f, i) + ph) - sin ph)
//   PHI  = fmx_synth_fm_phase's sum, term for term, of these
//   phi  = A(freq_hz + f_off, i) + PHI
//   (I, Q) += amplitude (cos phi, sin phi)     stations in ascending order
//   noise, front end (I + dc_i, q_gain Q + q_cross I + dc_q), rint, clamp
//
// all in double.  The build has -ffp-contract=off on both sides, so the host
// and the device run the same IEEE operations on the same integers: they
// differ only by the ulps of sin / cos and of fmx_gauss's float functions.
// Everything that touches a double is in this header and shared; what differs
// is how the integer residues turn(f, i) are reached: the host takes them
// from the definition (fmx_synth_band.cpp), the kernel steps them
// (fmx_synth_band.inc).
#ifndef FMX_SYNTH_BAND_H
#define FMX_SYNTH_BAND_H

#include <math.h>
#include <stdint.h>

#include "fmx_synth.h"

#define FMX_SB_CAPTURES_MAX 1024
#define FMX_SB_STATIONS_MAX 8192
#define FMX_SB_RATE_MIN 480000
#define FMX_SB_RATE_MAX 30720000
#define FMX_SB_NBITS_MAX (1 << 24)
#define FMX_SB_SAMPLE_END (1ll << 40)
#define FMX_SB_TONES 7 /* stereo: L+R (2), the four L-R side tones, the pilot; mono uses the first 2 */
#define FMX_SB_RES 9   /* residues of a station: carrier, the tones, 57 kHz on the RDS clock */
#define FMX_SB_R57 8
#define FMX_SB_TWO_PI 6.283185307179586

/* A station as the generator reads it, derived once (fmx_sb_derive).  The
 * first 23 members are doubles; the kernel's staging copies them as such. */
typedef struct {
  double k[FMX_SB_TONES];  /* 75000 a / f                                              */
  double c0[FMX_SB_TONES]; /* cos ph of an Isin tone, sin ph of an Icos tone             */
  double ph[FMX_SB_TONES];
  double amp;
  double pad;
  int64_t rds_off;          /* RDS bit-clock offset, samples                            */
  uint32_t fm[FMX_SB_RES];  /* f mod Fs, non-negative: [0] carrier, [1..7] tones, [8] 57 kHz */
  uint32_t pad2;
} fmx_sb_station;
#define FMX_SB_STATION_DOUBLES 23

FMX_HD uint32_t fmx_sb_fmod(int64_t f, int64_t fs) {
  int64_t r = f % fs;
  return (uint32_t)(r < 0 ? r + fs : r);
}

/* station g = channel ch0 + g of the content config; content->iq_rate is Fs */
FMX_HD void fmx_sb_derive(const fmx_synth_cfg *content, uint32_t ch, int freq_hz, float amplitude, fmx_sb_station *o) {
  const fmx_synth_chan c = fmx_synth_channel(content, ch);
  const int64_t fs = content->iq_rate;
  const double al = (double)c.a_l, ar = (double)c.a_r, pl = (double)c.ph_l, pr = (double)c.ph_r;
  double a[FMX_SB_TONES], ph[FMX_SB_TONES];
  int64_t f[FMX_SB_TONES];
  int icos[FMX_SB_TONES];
  for (int j = 0; j < FMX_SB_TONES; ++j) {
    a[j] = 0.0;
    ph[j] = 0.0;
    f[j] = 1;
    icos[j] = 0;
  }
  if (content->kind == FMX_SYNTH_MONO) {
    a[0] = al, f[0] = c.f_l, ph[0] = pl;
    a[1] = ar, f[1] = c.f_r, ph[1] = pr;
  } else {
    a[0] = 0.45 * al, f[0] = c.f_l, ph[0] = pl;
    a[1] = 0.45 * ar, f[1] = c.f_r, ph[1] = pr;
    a[2] = 0.225 * al, f[2] = (int64_t)c.f_l - 38000, ph[2] = pl, icos[2] = 1;
    a[3] = 0.225 * al, f[3] = (int64_t)c.f_l + 38000, ph[3] = pl, icos[3] = 1;
    a[4] = 0.225 * ar, f[4] = (int64_t)c.f_r - 38000, ph[4] = pr, icos[4] = 1;
    a[5] = 0.225 * ar, f[5] = (int64_t)c.f_r + 38000, ph[5] = pr, icos[5] = 1;
    a[6] = 0.09, f[6] = 19000, ph[6] = 0.0;
  }
  for (int j = 0; j < FMX_SB_TONES; ++j) {
    o->k[j] = 75000.0 * a[j] / (double)f[j];
    o->c0[j] = icos[j] ? sin(ph[j]) : cos(ph[j]);
    o->ph[j] = ph[j];
    o->fm[1 + j] = fmx_sb_fmod(f[j], fs);
  }
  o->amp = (double)amplitude;
  o->pad = 0.0;
  o->rds_off = c.rds_off;
  o->fm[0] = fmx_sb_fmod((int64_t)freq_hz + c.f_off, fs);
  o->fm[FMX_SB_R57] = fmx_sb_fmod(57000, fs);
  o->pad2 = 0;
}

FMX_HD double fmx_sb_angle(uint32_t r, double fs) { return FMX_SB_TWO_PI * (double)r / fs; }
/* (75000 rds_level / 57000), the RDS term's scale */
FMX_HD double fmx_sb_krds(float rds_level) { return 75000.0 * (double)rds_level / 57000.0; }

/* PHI after tone j (0 .. 6, or 0 .. 1 of a mono station) from PHI before it;
 * r: the tone's residue turn(f, i).  The order and the signs are
 * fmx_synth_fm_phase's: Isin, Isin, Icos, -Icos, -Icos, Icos, Isin. */
FMX_HD double fmx_sb_tone(int j, double p, double k, double c0, double ph, uint32_t r, double fs) {
  const double ang = fmx_sb_angle(r, fs) + ph;
  if (j >= 2 && j <= 5) {
    const double v = k * (sin(ang) - c0);
    return (j == 3 || j == 4) ? p - v : p + v;
  }
  return p + k * (c0 - cos(ang));
}
/* the RDS term: sgn the symbol sign +-1, r57 the 57 kHz residue on i + rds_off */
FMX_HD double fmx_sb_rds_term(double sgn, double krds, uint32_t r57, double fs) {
  return sgn * krds * (1.0 - cos(fmx_sb_angle(r57, fs)));
}

/* phi of one station from its residues r[FMX_SB_RES] (turn(f, i) of fm[], the
 * 57 kHz one on i + rds_off).  rds: 0 none, else the symbol sign +-1. */
FMX_HD double fmx_sb_phi(int kind, const double *k, const double *c0, const double *ph, const uint32_t *r, double fs,
                         double rds, double krds) {
  double p = 0.0;
  const int nt = kind == FMX_SYNTH_MONO ? 2 : FMX_SB_TONES;
  for (int j = 0; j < nt; ++j) p = fmx_sb_tone(j, p, k[j], c0[j], ph[j], r[1 + j], fs);
  if (rds != 0.0) p += fmx_sb_rds_term(rds, krds, r[FMX_SB_R57], fs);
  return fmx_sb_angle(r[0], fs) + p;
}

/* the symbol sign of half-bit h with the encoded bit `bit` */
FMX_HD double fmx_sb_rds_sign(int bit, int h_odd) { return (bit ? 1.0 : -1.0) * (h_odd ? -1.0 : 1.0); }

FMX_HD void fmx_sb_add(double amp, double phi, double *i, double *q) {
  double s, c;
#if defined(__HIP_DEVICE_COMPILE__)
  sincos(phi, &s, &c);
#else
  s = sin(phi);
  c = cos(phi);
#endif
  *i += amp * c;
  *q += amp * s;
}

FMX_HD uint64_t fmx_sb_noise_base(uint32_t seed_base, int s) {
  return fmx_splitmix64(((uint64_t)seed_base << 32) ^ (uint64_t)s ^ 0xBA4Dull);
}
FMX_HD void fmx_sb_noise(double noise_std, uint64_t base, int64_t i, double *vi, double *vq) {
  const uint64_t key = base + 2ull * (uint64_t)i;
  *vi += noise_std * (double)fmx_gauss(key);
  *vq += noise_std * (double)fmx_gauss(key + 1ull);
}

/* front end fe = {dc_i, dc_q, q_gain, q_cross} */
FMX_HD void fmx_sb_frontend(const double *fe, double *vi, double *vq) {
  const double i = *vi, q = *vq;
  *vi = i + fe[0];
  *vq = fe[2] * q + fe[3] * i + fe[1];
}

FMX_HD uint8_t fmx_sb_quant_u8(double v) {
  double x = rint(127.5 * v + 127.5);
  x = x < 0.0 ? 0.0 : (x > 255.0 ? 255.0 : x);
  return (uint8_t)x;
}
FMX_HD int16_t fmx_sb_quant_s16(double v) {
  double x = rint(32768.0 * v);
  x = x < -32768.0 ? -32768.0 : (x > 32767.0 ? 32767.0 : x);
  return (int16_t)x;
}

#ifdef __cplusplus
#include <string>
namespace fmx {

// samples per workgroup of k_synth_band: 256 threads, thread t owns t + 256 q
constexpr int SB_Q = 4;
constexpr int SB_TILE = 256 * SB_Q;

// What fmx_synth_band_host and fmx_synth_band_create refuse (fmx_synth_band.cpp):
// FMX_OK, or FMX_E_INVALID with *err = who + the condition.  bits_needed: the
// call needs the bit table of a kind-2 band with stations.
int synth_band_check(const char *who, const fmx_synth_band_config *cfg, int n_captures, const int *first_station,
                     const fmx_synth_station *stations, const fmx_synth_frontend *frontends, const uint8_t *h_bits,
                     std::string *err);
// a call's window: sample0 >= 0, n_samples >= 0, sample0 + n_samples <= 2^40, wide_stride >= n_samples
int synth_band_window(const char *who, int64_t sample0, int n_samples, size_t wide_stride, std::string *err);
void synth_band_content(const fmx_synth_band_config &cfg, fmx_synth_config *out);

struct SbArgs {
  void *out;          // [S][wide_stride] samples, interleaved I/Q
  size_t wide_stride; // samples
  int n;              // samples of each row this call writes
  int64_t sample0;
  const fmx_sb_station *st; // [stations]
  const int *first;         // [S + 1]
  const uint8_t *bits;      // [stations][n_bits] or NULL
  const double *fe;         // [S][4]
  int S, fs, kind, n_bits, s16;
  uint32_t seed_base;
  double noise_std, krds;
  double inv_fs, inv_2nb; // 1 / Fs, 1 / (2 n_bits)
  uint32_t im0;           // sample0 mod Fs
  uint32_t rstep_q, rstep_r; // quotient and remainder of 2375 * 256 / Fs
  int wide_store;         // every row starts at twice the element's alignment: one store per sample
};
int launch_synth_band(const SbArgs &a, void *stream); // k_synth_band (fmx_synth_band.inc)

} // namespace fmx
#endif

#endif
