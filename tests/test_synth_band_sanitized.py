"""The synthetic FM band's host side (fmx_synth_band.cpp) under ASan + UBSan in
a stand-alone program, tests/cpp/sanitize_synth_band.cpp: host code only,
nothing is loaded into Python and nothing is preloaded.  Its output buffers
are heap blocks of exactly n_captures x wide_stride samples at ragged strides,
and it makes every refused call of test_synth_band.py."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_synth_band_host_sanitized(tmp_path):
    exe = str(tmp_path / "sanitize_synth_band")
    csrc = os.path.join(ROOT, "fmtuner-sdr_amd", "csrc")
    cmd = ["g++", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-g", "-O1", "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-o", exe,
           os.path.join(ROOT, "tests", "cpp", "sanitize_synth_band.cpp"), os.path.join(csrc, "fmx_synth_band.cpp"),
           "-lpthread"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:], r.stdout[-400:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    out = json.loads(r.stdout)
    assert out["bad"] == 0 and out["calls"] == 60 and out["rejected"] == 22 and out["samples"] > 10000
    assert out["tile"] > 0 and out["tile"] % 256 == 0
