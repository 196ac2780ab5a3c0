// The capture bank's host work-list builder (fmx_wb_bank_groups,
// fmx_wb_design.cpp) under ASan + UBSan: tables at the limits -- 1 and 1024
// captures, every capture empty, one channel each, a single capture of
// 65 535 groups' worth of channels and one channel more, counts around the
// multiples of 16 -- into heap buffers of exactly `cap` groups, so that one
// entry written past G is an error the sanitizer reports.  Built by
// tests/test_wb_bank.py with fmx_wb_design.cpp and fmx_design.cpp; prints one
// JSON line.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fmx.h"

static int bad = 0, calls = 0, rejected = 0;
static long groups_total = 0;

// the table's groups into a buffer of exactly the count the function asks for, checked entry by entry
static void run(const std::vector<int> &counts) {
  const int S = (int)counts.size();
  std::vector<int> first(S + 1, 0);
  for (int s = 0; s < S; ++s) first[s + 1] = first[s] + counts[s];
  const int need = fmx_wb_bank_groups(first.data(), S, nullptr, 0);
  long want = 0;
  for (int c : counts) want += (c + 15) / 16;
  ++calls;
  if (want == 0) {
    if (need != 0) ++bad;
    return;
  }
  if (need != -want) {
    ++bad;
    return;
  }
  // one entry too few: refused with nothing written
  if (want > 1) {
    int *small = static_cast<int *>(std::malloc(sizeof(int) * 3 * (want - 1)));
    if (fmx_wb_bank_groups(first.data(), S, small, (int)want - 1) != -want) ++bad;
    std::free(small);
  }
  int *out = static_cast<int *>(std::malloc(sizeof(int) * 3 * want));
  const int G = fmx_wb_bank_groups(first.data(), S, out, (int)want);
  if (G != want) ++bad;
  long g = 0;
  for (int s = 0; s < S && G == want; ++s)
    for (int c = first[s]; c < first[s + 1]; c += 16, ++g) {
      const int n = first[s + 1] - c < 16 ? first[s + 1] - c : 16;
      if (out[3 * g] != s || out[3 * g + 1] != c || out[3 * g + 2] != n) ++bad;
    }
  if (g != want && G == want) ++bad;
  groups_total += want;
  std::free(out);
}

int main() {
  run({17, 0, 5, 16, 1});
  run({1});
  run({0});
  run({16});
  run({15, 17, 31, 32, 33});
  run(std::vector<int>(1024, 0));
  run(std::vector<int>(1024, 1));
  run(std::vector<int>(1024, 16));
  run(std::vector<int>(1024, 17));
  run({65535 * 16});                    // the most groups there may be
  run({65535 * 16 - 15});
  {
    std::vector<int> c(1024, 63 * 16);  // 64 512 groups
    c[1023] += 1023 * 16;               // 65 535
    run(c);
  }
  // refused tables
  auto refused = [&](const std::vector<int> &first, int S) {
    std::vector<int> out(3 * 8);
    if (fmx_wb_bank_groups(first.empty() ? nullptr : first.data(), S, out.data(), 8) < 0) ++rejected;
    else ++bad;
  };
  refused({1, 2}, 1);                   // first[0] != 0
  refused({0, 5, 4}, 2);                // decreasing
  refused({0}, 0);                      // no capture
  refused(std::vector<int>(1026, 0), 1025);
  refused({}, 1);                       // null table
  refused({0, 65535 * 16 + 1}, 1);      // one group too many
  refused({0, -1}, 1);
  std::printf("{\"calls\": %d, \"bad\": %d, \"rejected\": %d, \"groups\": %ld}\n", calls, bad, rejected, groups_total);
  return bad ? 1 : 0;
}
