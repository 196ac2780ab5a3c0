// fmx_xdr_signal_line under ASan + UBSan (built by tests/test_wb_signal.py with
// fmtuner-sdr_amd/csrc/fmx_host.cpp, -fsanitize=address,undefined
// -fno-sanitize-recover=all): levels across and far outside [0, 120], NaN and
// infinities, every mode, extreme cci / aci, into heap buffers of exactly
// `cap` bytes for every cap from 0 to past the line's length -- a write past
// cap is a heap overflow the sanitizer reports.  Prints one JSON line.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../include/fmx.h"

int main() {
  const float inf = std::numeric_limits<float>::infinity();
  std::vector<float> levels = {-inf, -1e30f, -3.0f, -0.04f, 0.0f, 0.04f, 0.05f, 0.45f, 42.25f, 99.96f,
                               119.96f, 120.0f, 120.04f, 500.0f, 1e30f, inf, std::nanf("")};
  for (int k = 0; k <= 1200; ++k) levels.push_back(0.1f * static_cast<float>(k) + 0.05f);
  const int ints[] = {-1, 0, 100, std::numeric_limits<int>::max(), std::numeric_limits<int>::min()};
  long lines = 0, refused = 0, bytes = 0;
  for (float lv : levels)
    for (int mode = 0; mode < 4; ++mode)
      for (int ci : ints) {
        char ref[64];
        const int n = fmx_xdr_signal_line(lv, mode & 1, mode >> 1, ci, ci / 3, ref, sizeof(ref));
        if (n < 4 || ref[0] != 'S' || ref[n - 1] != '\n' || ref[n] != '\0' || std::strlen(ref) != static_cast<size_t>(n)) {
          std::printf("{\"error\": \"bad line\", \"n\": %d}\n", n);
          return 1;
        }
        double v = -1.0;
        if (std::sscanf(ref + 2, "%lf", &v) != 1 || v < 0.0 || v > 120.0) {
          std::printf("{\"error\": \"level out of range\"}\n");
          return 1;
        }
        for (int cap = 0; cap <= n + 2; ++cap) {
          std::vector<char> buf(static_cast<size_t>(cap)); // exactly cap bytes on the heap
          const int rc = fmx_xdr_signal_line(lv, mode & 1, mode >> 1, ci, ci / 3, cap ? buf.data() : nullptr, cap);
          if (cap < n + 1 ? rc != -(n + 1) : (rc != n || std::memcmp(buf.data(), ref, static_cast<size_t>(n) + 1) != 0)) {
            std::printf("{\"error\": \"return convention\", \"cap\": %d, \"rc\": %d, \"n\": %d}\n", cap, rc, n);
            return 1;
          }
          refused += rc < 0;
        }
        ++lines;
        bytes += n;
      }
  std::printf("{\"lines\": %ld, \"refused\": %ld, \"bytes\": %ld}\n", lines, refused, bytes);
  return 0;
}
