// The bank scan's work list (fmx_wb_design.cpp: fmx_wb_bank_scan_groups) under
// ASan + UBSan: random and malformed point tables, the output buffers heap
// blocks of exactly the entries each call asks for, every entry checked
// against the definition (one entry per 64 points of a capture, none for an
// empty one).  Built by the test with fmx_wb_design.cpp and fmx_design.cpp;
// prints one JSON line.
#include <climits>
#include <cstdint>
#include <cstdio>
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
  long entries = 0;
  uint32_t seed = 2828u;
  const int sizes[] = {0, 0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 1000};
  for (int round = 0; round < 400; ++round) {
    int S = 1 + (int)(rnd(seed) % 48);
    if (round == 0) S = 1024; // the limit
    std::vector<int> first(S + 1, 0); // exactly S + 1 ints
    for (int s = 0; s < S; ++s) first[s + 1] = first[s] + (round == 1 ? 0 : sizes[rnd(seed) % 13]);
    const int G = -fmx_wb_bank_scan_groups(first.data(), S, nullptr, 0); // the count, negated (0 for no work)
    if (G < 0) {
      ++bad;
      continue;
    }
    long want = 0;
    for (int s = 0; s < S; ++s) want += (first[s + 1] - first[s] + 63) / 64;
    if (G != want) ++bad;
    std::vector<int> out((size_t)3 * G, -7); // exactly G entries
    if (fmx_wb_bank_scan_groups(first.data(), S, G ? out.data() : nullptr, G) != G) ++bad;
    int g = 0;
    for (int s = 0; s < S; ++s)
      for (int p = first[s]; p < first[s + 1]; p += 64, ++g) {
        const int n = first[s + 1] - p < 64 ? first[s + 1] - p : 64;
        if (g >= G || out[3 * g] != s || out[3 * g + 1] != p || out[3 * g + 2] != n) ++bad;
      }
    if (g != G) ++bad;
    entries += G;
    if (G > 0) { // one entry short: the count comes back negated and nothing is written
      std::vector<int> small((size_t)3 * (G - 1), -7);
      if (fmx_wb_bank_scan_groups(first.data(), S, G > 1 ? small.data() : nullptr, G - 1) != -G) ++bad;
      for (int v : small)
        if (v != -7) ++bad;
    }
    ++calls;
  }
  // malformed tables: refused before anything is read past the table or written
  int out3[3] = {-7, -7, -7};
  const int f_start[] = {1, 2}, f_dec[] = {0, 5, 4}, f_one[] = {0}, f_neg[] = {0, -1};
  const int f_wide[] = {0, INT_MAX}, f_wrap[] = {0, INT_MAX, INT_MIN};
  std::vector<int> many(1026, 0);
  if (fmx_wb_bank_scan_groups(f_start, 1, out3, 1) == FMX_E_INVALID) ++rejected;
  if (fmx_wb_bank_scan_groups(f_dec, 2, out3, 1) == FMX_E_INVALID) ++rejected;
  if (fmx_wb_bank_scan_groups(f_one, 0, out3, 1) == FMX_E_INVALID) ++rejected;
  if (fmx_wb_bank_scan_groups(f_one, -1, out3, 1) == FMX_E_INVALID) ++rejected;
  if (fmx_wb_bank_scan_groups(f_neg, 1, out3, 1) == FMX_E_INVALID) ++rejected;
  if (fmx_wb_bank_scan_groups(many.data(), 1025, out3, 1) == FMX_E_INVALID) ++rejected;
  if (fmx_wb_bank_scan_groups(nullptr, 1, out3, 1) == FMX_E_INVALID) ++rejected;
  if (fmx_wb_bank_scan_groups(f_wrap, 2, out3, 1) == FMX_E_INVALID) ++rejected;
  if (fmx_wb_bank_scan_groups(f_wide, 1, out3, 1) == FMX_E_CAPACITY) ++rejected; // more entries than the grid has rows
  for (int v : out3)
    if (v != -7) ++bad;
  std::printf("{\"calls\": %d, \"bad\": %d, \"rejected\": %d, \"entries\": %ld}\n", calls, bad, rejected, entries);
  return bad ? 1 : 0;
}
