// The synthetic FM band's host side (fmx_synth_band.cpp: fmx_synth_band_host,
// fmx_synth_band_content and what they refuse) under ASan + UBSan: random bands
// of both formats and all three kinds, the output buffers heap blocks of
// exactly n_captures x wide_stride samples at ragged strides, the tables heap
// blocks of exactly the entries a call reads; each band once whole and once
// cut in two, which must give the same bytes, and its padding untouched.
// Built by the test with fmx_synth_band.cpp alone; prints one JSON line.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "fmx.h"

static uint32_t rnd(uint32_t &s) { // xorshift32
  s ^= s << 13;
  s ^= s >> 17;
  s ^= s << 5;
  return s;
}

int main() {
  int calls = 0, bad = 0, rejected = 0;
  long samples = 0;
  uint32_t seed = 3030u;
  const int rates[] = {480000, 2048000, 2400000, 10000000, 30720000};
  for (int round = 0; round < 60; ++round) {
    fmx_synth_band_config cfg{};
    cfg.wide_rate = rates[rnd(seed) % 5];
    cfg.format = (int)(rnd(seed) % 2);
    cfg.kind = (int)(rnd(seed) % 3);
    cfg.seed_base = rnd(seed);
    cfg.max_offset_hz = (int)(rnd(seed) % 5001);
    cfg.rds_level = 0.05f;
    cfg.n_bits = 104 + (int)(rnd(seed) % 300);
    cfg.noise_std = (round & 1) ? 0.01f : 0.0f;
    const int S = round == 0 ? 1024 : 1 + (int)(rnd(seed) % 5);
    std::vector<int> first(S + 1, 0); // exactly S + 1 ints
    for (int s = 0; s < S; ++s) first[s + 1] = first[s] + (round == 0 ? (s % 97 == 0) : (int)(rnd(seed) % 4));
    const int G = first[S];
    std::vector<fmx_synth_station> st(G); // exactly G stations
    const int span = cfg.wide_rate / 2 - cfg.max_offset_hz;
    for (int g = 0; g < G; ++g) {
      st[g].freq_hz = (int)(rnd(seed) % (2u * (unsigned)span + 1u)) - span; // the edges included
      st[g].amplitude = 0.05f + 0.1f * (float)(rnd(seed) % 8);
    }
    if (G > 0 && round == 1) st[0].freq_hz = span;
    if (G > 1 && round == 1) st[1].freq_hz = -span;
    std::vector<fmx_synth_frontend> fe(S);
    for (int s = 0; s < S; ++s) fe[s] = {0.01 * (s % 3), -0.02, 1.0 + 0.02 * (s % 4), 0.03 * (s % 2)};
    std::vector<uint8_t> bits((size_t)G * cfg.n_bits); // exactly [G][n_bits]
    for (auto &b : bits) b = (uint8_t)(rnd(seed) & 1u);
    const int n = round == 0 ? 3 : 1 + (int)(rnd(seed) % 700);
    const size_t stride = (size_t)n + rnd(seed) % 7;
    const int64_t sample0 = (round % 3 == 0) ? 0 : (round % 3 == 1) ? ((int64_t)1 << 40) - n : ((int64_t)1 << 33) + rnd(seed);
    const size_t esz = cfg.format == FMX_WB_S16 ? 2 : 1;
    const size_t cells = (size_t)S * stride * 2;
    std::vector<uint8_t> whole(cells * esz, 0x55), cut(cells * esz, 0x55); // exactly S x stride samples
    const uint8_t *bp = (cfg.kind == 2 && G > 0) ? bits.data() : nullptr;
    const fmx_synth_frontend *fp = (round % 4 == 3) ? nullptr : fe.data();
    const int threads = 1 + (int)(rnd(seed) % 5);
    if (fmx_synth_band_host(&cfg, 7u + round, S, first.data(), G ? st.data() : nullptr, fp, sample0, n, bp, whole.data(),
                            stride, threads) != FMX_OK) {
      ++bad;
      continue;
    }
    const int n1 = (int)(rnd(seed) % (unsigned)(n + 1)); // 0 .. n: an empty call is legal
    int rc = fmx_synth_band_host(&cfg, 7u + round, S, first.data(), G ? st.data() : nullptr, fp, sample0, n1, bp, cut.data(),
                                 stride, 1);
    if (rc == FMX_OK && n > n1)
      rc = fmx_synth_band_host(&cfg, 7u + round, S, first.data(), G ? st.data() : nullptr, fp, sample0 + n1, n - n1, bp,
                               cut.data() + 2 * esz * (size_t)n1, stride, 3);
    // the second call's rows start n1 samples into a block that ends with the last row's stride:
    // its last row may use n - n1 + (stride - n) cells and no more
    if (rc != FMX_OK || std::memcmp(whole.data(), cut.data(), whole.size()) != 0) ++bad;
    for (int s = 0; s < S; ++s)
      for (size_t c = 2 * esz * ((size_t)s * stride + n); c < 2 * esz * ((size_t)s + 1) * stride; ++c)
        if (whole[c] != 0x55) ++bad;
    fmx_synth_config content;
    if (fmx_synth_band_content(&cfg, &content) != FMX_OK || content.iq_rate != cfg.wide_rate || content.amplitude != 1.0f) ++bad;
    samples += (long)n * S;
    ++calls;
  }

  // refused calls: nothing is read past a table or written
  fmx_synth_band_config ok{};
  ok.wide_rate = 2400000;
  ok.format = FMX_WB_S16;
  ok.kind = 1;
  ok.max_offset_hz = 5000;
  ok.rds_level = 0.05f;
  ok.n_bits = 208;
  const int f01[] = {0, 1}, f12[] = {1, 2}, f_dec[] = {0, 1, 0}, f_big[] = {0, 8193};
  std::vector<int> many(1026, 0);
  const fmx_synth_station one[] = {{100000, 0.1f}}, edge[] = {{1195001, 0.1f}}, neg[] = {{0, -0.1f}};
  const fmx_synth_station nan_a[] = {{0, std::numeric_limits<float>::quiet_NaN()}};
  std::vector<fmx_synth_station> lots(8193, fmx_synth_station{0, 0.1f});
  const fmx_synth_frontend g0[] = {{0, 0, 0, 0}}, inf_dc[] = {{std::numeric_limits<double>::infinity(), 0, 1, 0}};
  std::vector<int16_t> out(2 * 8, (int16_t)-7); // exactly 8 samples
  std::vector<uint8_t> b208(208, 0);
  auto R = [&](const fmx_synth_band_config *c, int S, const int *first, const fmx_synth_station *st,
               const fmx_synth_frontend *fe, int64_t s0, int n, const uint8_t *bits, void *o, size_t stride) {
    if (fmx_synth_band_host(c, 0, S, first, st, fe, s0, n, bits, o, stride, 2) == FMX_E_INVALID &&
        std::strncmp(fmx_synth_band_error(), "fmx_synth_band_host: ", 21) == 0)
      ++rejected;
  };
  R(nullptr, 1, f01, one, nullptr, 0, 8, nullptr, out.data(), 8);
  R(&ok, 1, nullptr, one, nullptr, 0, 8, nullptr, out.data(), 8);
  R(&ok, 1, f01, nullptr, nullptr, 0, 8, nullptr, out.data(), 8);
  R(&ok, 1, f01, one, nullptr, 0, 8, nullptr, nullptr, 8);
  R(&ok, 1, f12, one, nullptr, 0, 8, nullptr, out.data(), 8);
  R(&ok, 2, f_dec, one, nullptr, 0, 8, nullptr, out.data(), 8);
  R(&ok, 0, f01, one, nullptr, 0, 8, nullptr, out.data(), 8);
  R(&ok, 1025, many.data(), one, nullptr, 0, 8, nullptr, out.data(), 8);
  R(&ok, 1, f_big, lots.data(), nullptr, 0, 8, nullptr, out.data(), 8);
  R(&ok, 1, f01, edge, nullptr, 0, 8, nullptr, out.data(), 8);
  R(&ok, 1, f01, neg, nullptr, 0, 8, nullptr, out.data(), 8);
  R(&ok, 1, f01, nan_a, nullptr, 0, 8, nullptr, out.data(), 8);
  R(&ok, 1, f01, one, g0, 0, 8, nullptr, out.data(), 8);
  R(&ok, 1, f01, one, inf_dc, 0, 8, nullptr, out.data(), 8);
  fmx_synth_band_config c = ok;
  c.format = 2;
  R(&c, 1, f01, one, nullptr, 0, 8, nullptr, out.data(), 8);
  c = ok, c.wide_rate = 479999;
  R(&c, 1, f01, one, nullptr, 0, 8, nullptr, out.data(), 8);
  c = ok, c.wide_rate = 30720001;
  R(&c, 1, f01, one, nullptr, 0, 8, nullptr, out.data(), 8);
  c = ok, c.kind = 2, c.n_bits = 103;
  R(&c, 1, f01, one, nullptr, 0, 8, b208.data(), out.data(), 8);
  c = ok, c.kind = 2;
  R(&c, 1, f01, one, nullptr, 0, 8, nullptr, out.data(), 8);
  R(&ok, 1, f01, one, nullptr, 0, 9, nullptr, out.data(), 8);
  R(&ok, 1, f01, one, nullptr, -1, 8, nullptr, out.data(), 8);
  R(&ok, 1, f01, one, nullptr, ((int64_t)1 << 40) - 7, 8, nullptr, out.data(), 8);
  for (int16_t v : out)
    if (v != -7) ++bad;
  if (fmx_synth_band_content(nullptr, nullptr) != FMX_E_INVALID) ++bad;
  std::printf("{\"calls\": %d, \"bad\": %d, \"rejected\": %d, \"samples\": %ld, \"tile\": %d}\n", calls, bad, rejected, samples,
              fmx_synth_band_tile());
  return bad ? 1 : 0;
}
