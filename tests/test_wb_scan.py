"""The band scan's host side (fmx_wb_scan_points, fmx_scan_peaks) and its
float64 restatement tests/wb_scan_ref.py, on the CPU: the level mapping pinned
to the reference's computeSignalLevel, the plan's conditions, the peak
picker's known answers, and the band of the end-to-end tests -- the scan of
one capture finds exactly its four stations."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle as O
import wb_ref as R
import wb_scan_ref as S

# the plan of the band: 23 points at 100 kHz from -1.1 MHz, measured at 240 kHz
BAND_START, BAND_STEP, BAND_POINTS = -1_100_000, 100_000, 23
BAND_SCAN_CALLS = (0, 1, 5)


@functools.lru_cache(maxsize=None)
def band_levels(fmx):
    """float64 P_p [3][23] of calls 0, 1 and 5 of the band capture, and the capture."""
    raw = R.band_capture(fmx)
    per = 2 * R.BAND_N * R.BAND_D
    freqs = S.points(BAND_START, BAND_STEP, BAND_POINTS)
    tpp = R.tpp_rule(R.BAND_D)
    pw = np.stack([S.powers(raw[per * i:per * (i + 1)], R.S16, R.BAND_D, tpp, R.BAND_FS, freqs, R.BAND_N)
                   for i in BAND_SCAN_CALLS])
    return pw, raw


@pytest.mark.parametrize("params", [S.DEFAULT_PARAMS, (20, 0.5, 3.0, -80.0, -12.0), (0, 0.5, 0.0, -20.0, -40.0),
                                    (0, 0.5, -4.0, -10.0, -5.0)])
@pytest.mark.parametrize("sigma", [2.0, 30.0, 140.0])
def test_level_mapping_is_the_reference_signal_level(params, sigma):
    """u8 IQ made of pairs b, 255 - b (I and Q each), so that the mean is
    exactly 127.5 and the reference's mean removal does nothing: the record
    wb_scan_ref forms from mean |x|^2 is computeSignalLevel's.  dbfs and
    compensated dbfs to 1e-9, level120 to 1e-4 (one f32 conversion), the clip
    ratios exact.  The parameter sets include an inverted floor / ceil (the
    safeCeil clamp) and one that clamps the level to 0."""
    rng = np.random.default_rng(int(sigma))
    b = np.clip(127.5 + rng.normal(0, sigma, 2 * 3000), 0, 255).astype(np.uint8)  # I, Q of the even samples
    iq = np.empty(4 * 3000, np.uint8)
    iq[0::4], iq[1::4] = b[0::2], b[1::2]
    iq[2::4], iq[3::4] = 255 - b[0::2], 255 - b[1::2]
    x = R.normalise(iq, R.U8)
    got = S.record(np.mean(np.abs(x) ** 2), params)
    got["hard_clip_ratio"], got["near_clip_ratio"] = S.clip_ratios(iq, R.U8)
    refs = [O.signal_level(iq, *params)] + ([O.ref_signal_level(iq, *params)] if O.ref_available() else [])
    for want in refs:
        assert abs(got["dbfs"] - want["dbfs"]) < 1e-9
        assert abs(got["compensated_dbfs"] - want["compensated_dbfs"]) < 1e-9
        assert abs(got["level120"] - want["level120"]) <= 1e-4
        assert got["hard_clip_ratio"] == want["hard_clip_ratio"]
        assert got["near_clip_ratio"] == want["near_clip_ratio"]
    if params[3] == -10.0 and sigma == 2.0:
        assert got["level120"] == 0.0  # a clamped level is among the cases
    if sigma == 140.0:
        assert got["hard_clip_ratio"] > 0.1


def test_int16_clip_ratio_is_judged_by_the_top_byte():
    """b <= 1 is v <= -32257, b >= 254 v >= 32256, b <= 8 v <= -30465, b >= 247 v >= 30464."""
    v = np.array([-32257, 0, -32256, 0, 0, 32256, 0, 32255, -30465, 0, -30464, 0, 0, 30464, 0, 30463, 5, 5,
                  -32768, 32767], np.int16)  # hard: samples 0, 2, 9; near: those and 1, 3, 4, 6
    assert S.clip_ratios(v, R.S16) == (3 / 10.0, 7 / 10.0)


def test_scan_points(fmx):
    cfg = fmx.make_wb_scan_config(2_400_000, 240_000, fmx.FMX_WB_S16, 0, 4096, -1_100_000, 100_000, 23)
    f = fmx.wb_scan_points(cfg)
    assert f == [-1_100_000 + 100_000 * p for p in range(23)]
    L = fmx.lib()
    buf = (C.c_int * 4)(7, 7, 7, 7)
    assert L.fmx_wb_scan_points(C.byref(cfg), buf, 3) == 23 and list(buf) == f[:3] + [7]  # at most cap are written
    edge = fmx.make_wb_scan_config(start_hz=-1_200_000, step_hz=1, n_points=1)
    assert fmx.wb_scan_points(edge) == [-1_200_000]
    assert fmx.wb_scan_points(fmx.make_wb_scan_config(start_hz=1_200_000 - 8191, step_hz=1, n_points=8192))[-1] == 1_200_000
    bad = dict(step0=dict(step_hz=0), none=dict(n_points=0), many=dict(n_points=8193, step_hz=1),
               low=dict(start_hz=-1_200_001), high=dict(start_hz=-1_000_000, step_hz=100_000, n_points=24),
               high1=dict(start_hz=1_200_001 - 22, step_hz=1, n_points=23),
               d1=dict(wide_rate=240_000), tpp3=dict(taps_per_phase=3), fmt2=dict(format=2))
    for name, kw in bad.items():
        assert L.fmx_wb_scan_points(C.byref(fmx.make_wb_scan_config(**kw)), None, 0) == -1, name
    assert L.fmx_wb_scan_points(None, None, 0) == -1


def test_scan_peaks_known_answers(fmx):
    pk = fmx.scan_peaks
    assert pk([], -40.0, 1) == []
    assert pk([-10.0], -40.0, 3) == [0]
    assert pk([-50.0], -40.0, 3) == []
    assert pk([-10, -20, -30, -20, -10], -40.0, 1) == [0, 4]               # peaks at both ends
    assert pk([-30, -10, -10, -30], -40.0, 1) == [1]                       # a tie goes to the lowest index
    assert pk([-10, -10, -10, -10], -40.0, 1) == [0]
    assert pk([-10, -10, -10, -10], -40.0, 0) == [0, 1, 2, 3]              # no spacing: the threshold alone
    assert pk([-30, -10, -20, -9, -30, -12, -30], -40.0, 1) == [1, 3, 5]
    assert pk([-30, -10, -20, -9, -30, -12, -30], -40.0, 2) == [3]         # -12 has -9 two to its left
    assert pk([-30, -10, -20, -9, -30, -12, -30], -40.0, 100) == [3]
    assert pk([-30, -10, -20, -9, -30, -12, -30], -9.5, 1) == [3]          # the threshold
    assert pk([-30, -10, -20, -9, -30, -12, -30], -9.0, 1) == [3]          # at the threshold counts
    L = fmx.lib()
    v = (C.c_double * 7)(-30, -10, -20, -9, -30, -12, -30)
    idx = (C.c_int * 3)(77, 77, 77)
    assert L.fmx_scan_peaks(v, 7, -40.0, 1, idx, 2) == 3 and list(idx) == [1, 3, 77]  # cap below the count
    assert L.fmx_scan_peaks(v, 7, -40.0, 1, None, 0) == 3
    assert L.fmx_scan_peaks(v, 0, -40.0, 1, idx, 3) == 0
    assert L.fmx_scan_peaks(v, -1, -40.0, 1, idx, 3) == -1 and L.fmx_scan_peaks(v, 7, -40.0, -1, idx, 3) == -1
    assert L.fmx_scan_peaks(None, 7, -40.0, 1, idx, 3) == -1


def test_band_scan_finds_the_stations(fmx):
    """wb_ref.band_capture, calls 0, 1 and 5 of 4096 outputs, 23 points from
    -1.1 MHz at 100 kHz (D = 10, tpp 28): fmx_scan_peaks(dbfs, -40, 1) on the
    float64 levels returns exactly BAND_FREQ, each peak at least 1 dB above
    both neighbours (the margins are 1.95 - 2.5 dB; the stations read -14.4 /
    -22.3 / -16.0 / -28.4 dBFS, the strongest point not next to a station
    -49 dBFS).  On a 50 or 25 kHz grid the filter is wider than the step and
    the margin falls to 0.03 dB: not asserted there."""
    pw, _ = band_levels(fmx)
    freqs = fmx.wb_scan_points(fmx.make_wb_scan_config(R.BAND_FS, R.BAND_DSP, fmx.FMX_WB_S16, 0, R.BAND_N,
                                                       BAND_START, BAND_STEP, BAND_POINTS))
    want = [freqs.index(f) for f in R.BAND_FREQ]
    for k in range(len(BAND_SCAN_CALLS)):
        dbfs = [S.record(p)["dbfs"] for p in pw[k]]
        print("call", BAND_SCAN_CALLS[k], [round(v, 2) for v in dbfs])
        peaks = fmx.scan_peaks(dbfs, -40.0, 1)
        assert [freqs[i] for i in peaks] == list(R.BAND_FREQ), (k, peaks)
        for i in want:
            assert dbfs[i] - max(dbfs[i - 1], dbfs[i + 1]) >= 1.0, (k, i, dbfs[i - 1:i + 2])
        rest = [v for i, v in enumerate(dbfs) if all(abs(i - j) > 1 for j in want)]
        assert max(rest) < -45.0, (k, max(rest))


def test_scan_host_entry_points_sanitized(tmp_path):
    """fmx_wb_scan_points and fmx_scan_peaks (fmx_wb_design.cpp, with
    fmx_design.cpp's firdes_kaiser) under ASan + UBSan in a stand-alone
    program: host code only, nothing is loaded into Python."""
    import json
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "wb_scan_sanitize")
    csrc = os.path.join(root, "fmtuner-sdr_amd", "csrc")
    cmd = ["g++", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-g", "-O1", "-I" + os.path.join(root, "include"), "-I" + csrc, "-o", exe,
           os.path.join(root, "tests", "cpp", "wb_scan_sanitize_main.cpp"), os.path.join(csrc, "fmx_wb_design.cpp"),
           os.path.join(csrc, "fmx_design.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-4000:])
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    assert rec["bad"] == 0 and rec["rejected"] == 14 and rec["peaks"] > 0, rec
