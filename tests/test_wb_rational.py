"""The rational-rate channelizer on the CPU (fmx_wb_create_rational, DESIGN.md
section 23; the GPU side is tests/test_gpu_wb_rational.py):

  1. tests/wb_rational_ref.py, the float64 restatement every GPU comparison
     uses: the factored form against the defining sum, against tests/wb_ref.py
     at Q = 1, and against a tone (the definition is a resampler);
  2. fmx_wb_ratio: the accepted and the refused ratios;
  3. fmx_wb_weights_rational (the kernel's f16 hi + lo tables read back, every
     phase) against float64;
  4. fmx_wb_rational_geometry, the kernel's tiling: for every legal ratio no
     fragment read leaves its workgroup's window, LDS stays within 80 KB and
     the tiles cover every output exactly once;
  5. header and binding carry every name; the ABI version is still 13;
  6. the code object's metadata: k_wbr's instances, no scratch or spills;
  7. every call refuses a NULL object without touching a device;
  8. the host design under ASan + UBSan, as a stand-alone program."""
import ctypes as C
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest

import wb_rational_ref as RR
import wb_ref as R
from test_resources import _kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DSP = 240_000
NAMES = ("fmx_wb_create_rational", "fmx_wb_ratio", "fmx_wb_weights_rational", "fmx_wb_rational_geometry")
LDS_MAX = 80 * 1024


@pytest.mark.parametrize("P,Q", [(25, 3), (250, 3), (5, 2), (128, 15)])
def test_factored_form_against_the_defining_sum(P, Q):
    """channelize (Q integer channelizers interleaved) against direct (the
    defining sum, term by term), a tuned channel and a first index of 777 and
    of 2^40 + 12 345: |d| < 1e-12 at outputs of every phase, the filter filling
    and full."""
    tpp = RR.tpp_rule(P, Q)
    Fs = P * DSP // Q  # 2 MS/s, 20 MS/s, 600 kS/s, 2.048 MS/s
    assert Fs * Q == P * DSP
    M = tpp + 9
    rng = np.random.default_rng(P)
    x = rng.uniform(-1, 1, M * P) + 1j * rng.uniform(-1, 1, M * P)
    for s0, f in ((777, -123_457 % (Fs // 2)), ((1 << 40) + 12_345, -(Fs // 2) + 1)):
        y = RR.channelize(x, P, Q, tpp, Fs, [0, f], sample0=s0)
        assert y.shape == (2, M * Q)
        for n in list(range(2 * Q + 1)) + [tpp * Q - 1, tpp * Q, M * Q - Q - 1, M * Q - 1]:
            assert abs(y[1, n] - RR.direct(x, P, Q, tpp, Fs, f, n, s0)) < 1e-12, (P, Q, n)
            assert abs(y[0, n] - RR.direct(x, P, Q, tpp, Fs, 0, n, s0)) < 1e-12, (P, Q, n)


@pytest.mark.parametrize("D,tpp", [(10, 28), (25, 12), (100, 28)])
def test_q1_is_the_integer_channelizer(D, tpp):
    Fs = D * DSP
    rng = np.random.default_rng(D)
    x = rng.uniform(-1, 1, 64 * D) + 1j * rng.uniform(-1, 1, 64 * D)
    freqs = [0, 123_457, -Fs // 2 + 1]
    s0 = (1 << 40) + 12_345
    d = RR.channelize(x, D, 1, tpp, Fs, freqs, sample0=s0) - R.channelize(x, D, tpp, Fs, freqs, sample0=s0)
    assert np.max(np.abs(d)) < 1e-12


@pytest.mark.parametrize("P,Q,Fs", [(10, 1, 2_400_000), (25, 3, 2_000_000), (128, 15, 2_048_000)])
def test_a_tone_comes_out_resampled(P, Q, Fs):
    """A unit tone at f_c + delta comes out as the tone at delta sampled at
    n P / Q, delayed by the prototype's (Lup - 1) / (2 Q) wide samples: the
    definition is a resampler, not merely self-consistent.  Bar 1.5e-4: the
    80 dB design's ripple is 1e-4."""
    tpp, fc_hz = 28, 300_000
    M = 3 * tpp
    i = np.arange(M * P, dtype=np.int64)
    Lup = P * tpp
    for delta in (0, 30_000, -75_000):
        turns = (((fc_hz + delta) % Fs) * i) % Fs
        x = np.exp(2j * np.pi * turns / Fs)
        y = RR.channelize(x, P, Q, tpp, Fs, [fc_hz])[0]
        n = np.arange(tpp * Q + Q, M * Q)  # the filter has filled
        want = np.exp(2j * np.pi * delta * (n * P / Q - (Lup - 1) / (2.0 * Q)) / Fs)
        err = float(np.max(np.abs(y[n] - want)))
        print(f"tone P/Q = {P}/{Q} delta {delta}: max |d| = {err:.3g}")
        assert err < 1.5e-4, (P, Q, delta, err)


def _ratio(fmx, wide, dsp=DSP, fmt=0, tpp=0, block=4096):
    cfg = fmx.make_wb_config(wide, dsp, fmt, tpp, block)
    P, Q, taps = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    rc = fmx.lib().fmx_wb_ratio(C.byref(cfg), C.byref(P), C.byref(Q), C.byref(taps))
    return rc, P.value, Q.value, taps.value


def test_ratio_accepts_and_refuses(fmx):
    for wide, want in ((20_000_000, (250, 3)), (10_000_000, (125, 3)), (2_048_000, (128, 15)), (600_000, (5, 2)),
                       (2_400_000, (10, 1))):
        for fmt in (0, 1):
            rc, P, Q, taps = _ratio(fmx, wide, fmt=fmt)
            assert (rc, P, Q) == (0, *want), (wide, rc, P, Q)
            assert taps == max(L for _, _, L in RR.phases(P, Q, RR.tpp_rule(P, Q)))
            assert fmx.wb_ratio(fmx.make_wb_config(wide, DSP, fmt, 0, 4096)) == (P, Q, taps)
    assert _ratio(fmx, 2_400_001) == (-1, -1, -1, -1)            # 2 400 001 / 240 000: Q = 240 000
    assert _ratio(fmx, 129 * DSP)[0] == -1                      # D > 128
    assert _ratio(fmx, 128 * DSP + 1_000)[0] == -1              # 3085 / 24: Q > 16
    assert _ratio(fmx, 2049, dsp=16)[0] == -1                   # D = 128.06
    assert _ratio(fmx, 2048, dsp=16)[0] == 0                    # D = 128
    assert _ratio(fmx, 31, dsp=16)[0] == -1                     # D = 1.94
    assert _ratio(fmx, 32, dsp=16)[:3] == (0, 2, 1)             # D = 2
    assert _ratio(fmx, DSP)[0] == -1                            # D = 1
    assert _ratio(fmx, 35, dsp=17)[0] == -1                     # Q = 17
    assert _ratio(fmx, 10_000_000, dsp=256_000, fmt=1)[0] == -1  # 625 / 16: an int16 tile's window is 88 640 bytes
    assert _ratio(fmx, 10_000_000, dsp=256_000, fmt=0)[:3] == (0, 625, 16)
    assert _ratio(fmx, 2_000_000, tpp=3)[0] == -1 and _ratio(fmx, 2_000_000, tpp=29)[0] == -1
    assert _ratio(fmx, 2_000_000, fmt=2)[0] == -1 and _ratio(fmx, 2_000_000, block=0)[0] == -1
    assert fmx.lib().fmx_wb_ratio(None, None, None, None) == -1
    # the integer entry keeps refusing what it refused
    cfg = fmx.make_wb_config(2_000_000, DSP, 0, 0, 4096)
    assert fmx.lib().fmx_wb_weights(C.byref(cfg), 0, None, 0) == -1


@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("Fs", [2_000_000, 20_000_000])
def test_rational_weight_tables_against_float64(fmx, Fs, fmt):
    """Every phase's W_r[j] read back from the f16 hi + lo rows: error per tap
    <= 2^-21 of the largest tap of any phase (one scale serves all phases),
    test_weight_tables_against_float64's bar."""
    P, Q = RR.ratio(Fs, DSP)
    tpp = RR.tpp_rule(P, Q)
    wcfg = fmx.make_wb_config(Fs, DSP, fmt, 0, 4096)
    for f in (0, 123_457, -Fs // 2 + 1):
        want = [RR.weights(P, Q, tpp, Fs, f, r) for r in range(Q)]
        top = max(np.max(np.abs(w)) for w in want)
        for r in range(Q):
            got = fmx.wb_weights_rational(wcfg, f, r).astype(np.complex128)
            assert got.shape == want[r].shape == (RR.phases(P, Q, tpp)[r][2],)
            err = np.abs(got - want[r])
            assert np.max(err) <= top * 2.0 ** -21, (Fs, fmt, f, r, np.max(err) / top)
            big = np.abs(want[r]) >= top * 2.0 ** -12
            assert np.max(err[big] / np.abs(want[r][big])) <= 2.0 ** -18, (Fs, fmt, f, r)
    L = fmx.lib()
    assert L.fmx_wb_weights_rational(C.byref(wcfg), 0, Q, None, 0) == -1
    assert L.fmx_wb_weights_rational(C.byref(wcfg), Fs // 2 + 1, 0, None, 0) == -1


def test_q1_weights_are_the_integer_tables(fmx):
    wcfg = fmx.make_wb_config(2_400_000, DSP, 1, 0, 4096)
    for f in (0, 123_457, -1_199_999):
        assert np.array_equal(fmx.wb_weights_rational(wcfg, f, 0), fmx.wb_weights(wcfg, f))


def _legal_ratios():
    return [(P, Q) for Q in range(1, 17) for P in range(2 * Q, min(128 * Q, 640) + 1) if math.gcd(P, Q) == 1]


def test_geometry_keeps_every_fragment_inside_its_window(fmx):
    """For every legal (P, Q) with Q <= 16 and P <= 640, both formats, at
    n_out = Q, 16 Q and the largest multiple of Q up to 4095: the last fragment
    read of every tile (column 15, lane group 3, last K step: the window's 8
    last elements of Lp from offset + 15 P on) ends inside its workgroup's
    window, that window fits the launch's LDS, LDS <= 80 KB, every tile's
    offset is what the kernel computes (16 (mb - mb0) P + a_r), and the tiles'
    outputs (16 mb + col) Q + r, col < 16, cover 0 .. n_out - 1 exactly once."""
    L = fmx.lib()
    checked = refused = 0
    for P, Q in _legal_ratios():
        for fmt in (0, 1):
            cfg = fmx.make_wb_config(P * 16_000, Q * 16_000, fmt, 0, 4096)
            if L.fmx_wb_ratio(C.byref(cfg), None, None, None) != 0:
                refused += 1
                assert L.fmx_wb_rational_geometry(C.byref(cfg), Q, None, 0) == -1
                continue
            for n_out in (Q, 16 * Q, 4095 - 4095 % Q):
                g = fmx.wb_rational_geometry(cfg, n_out)
                t = g["tile"]
                nt, Lp, M = g["nt"], g["Lp"], n_out // Q
                assert 1 <= nt <= 16 and Lp % 32 == 0 and g["tiles"] == len(t) == -(-M // 16) * Q
                assert g["workgroups"] == -(-len(t) // nt)
                assert g["lds_bytes"] <= LDS_MAX and g["lds_bytes"] >= g["window"] * (8 if fmt else 4)
                T = np.arange(len(t))
                r, mb, mb0 = T % Q, T // Q, (T // nt * nt) // Q
                assert np.array_equal(t[:, 0], r) and np.array_equal(t[:, 1], r * P // Q)
                assert np.array_equal(t[:, 2], 16 * (mb - mb0) * P + t[:, 1])
                last = t[:, 2] + 15 * P + (Lp - 32) + 8 * 3 + 8  # one past the last element read
                assert np.all(last <= t[:, 3]) and np.all(t[:, 3] <= g["window"]) and np.all(t[:, 2] >= 0), (P, Q, fmt, n_out)
                n = ((16 * mb[:, None] + np.arange(16)[None, :]) * Q + r[:, None]).ravel()
                n = n[n < n_out]
                assert len(n) == n_out and np.array_equal(np.sort(n), np.arange(n_out)), (P, Q, n_out)
                checked += 1
    assert checked > 3 * 2 * 1000 and refused > 0, (checked, refused)
    # n_out must be a multiple of Q and within the block
    cfg = fmx.make_wb_config(2_000_000, DSP, 0, 0, 4096)
    for n_out in (0, 1, 4, 4097, 4098):
        assert L.fmx_wb_rational_geometry(C.byref(cfg), n_out, None, 0) == -1
    assert L.fmx_wb_rational_geometry(None, 3, None, 0) == -1


def test_geometry_of_the_receivers_people_own(fmx):
    """20 MS/s int16 is the tightest: one tile per workgroup (two would need
    82 016 bytes); u8 takes ten."""
    g = fmx.wb_rational_geometry(fmx.make_wb_config(20_000_000, DSP, 1, 0, 4096), 4092)
    assert (g["nt"], g["Lp"], g["window"], g["lds_bytes"]) == (1, 2336, 15 * 250 + 166 + 2336, 50_048)
    g = fmx.wb_rational_geometry(fmx.make_wb_config(20_000_000, DSP, 0, 0, 4096), 4092)
    assert g["nt"] == 10 and g["lds_bytes"] <= LDS_MAX


def test_names_and_abi_version(fmx):
    with open(os.path.join(ROOT, "include", "fmx.h")) as fh:
        header = fh.read()
    L = fmx.lib()
    for name in NAMES:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert getattr(L, name).argtypes is not None, name
    assert re.search(r"^#define FMX_ABI_VERSION 13$", header, re.M)
    for fn in ("wb_ratio", "wb_weights_rational", "wb_rational_geometry"):
        assert callable(getattr(fmx, fn)), fn
    import inspect
    assert inspect.signature(fmx.Wideband.__init__).parameters["rational"].default is False


def test_code_object_metadata(tmp_path):
    """k_wbr's four instances (int16 / u8 x P even / odd) and k_wbr_hist's two:
    no scratch, no spills, no AGPRs, VGPRs no more than k_wb's (112 int16, 104
    u8; built: 112 / 110 and 104 / 102)."""
    ks = _kernels(tmp_path)
    pick = lambda pat: {k: v for k, v in ks.items() if re.search(pat, k)}  # noqa: E731
    wbr, hist = pick(r"\d+k_wbrI"), pick(r"\d+k_wbr_histI")
    assert (len(wbr), len(hist)) == (4, 2), (sorted(wbr), sorted(hist))
    assert len(pick(r"\d+k_wbr")) == 6
    for name, f in {**wbr, **hist}.items():
        print(name, f)
        assert f.get("private_segment_fixed_size", 0) == 0, (name, f)
        assert f.get("vgpr_spill_count", 0) == 0 and f.get("sgpr_spill_count", 0) == 0, (name, f)
        assert f.get("agpr_count", 0) == 0, (name, f)
    for name, f in wbr.items():
        s16 = "k_wbrILb1E" in name  # the first template argument
        assert f.get("vgpr_count", 0) <= (112 if s16 else 104), (name, f)


def test_null_object_calls_need_no_gpu(fmx):
    L = fmx.lib()
    wb = C.c_void_p(1)
    cfg = fmx.make_wb_config(2_000_000, DSP, 0, 0, 4096)
    f = (C.c_int * 1)(0)
    assert L.fmx_wb_create_rational(None, C.byref(cfg), f, 1, C.byref(wb)) == -1 and not wb.value
    assert L.fmx_wb_create(None, C.byref(cfg), f, 1, C.byref(wb)) == -1
    out = fmx.BlockOut(None, 0, None, None, 0, None, None, None, None, None, 0, None, None, None)
    assert L.fmx_wb_destroy(None) == -1 and L.fmx_wb_set_freq(None, 0, 0) == -1 and L.fmx_wb_reset(None, 0) == -1
    assert L.fmx_wb_process(None, None, 3, None, 3) == -1
    assert L.fmx_wb_process_block(None, None, 3, C.byref(out)) == -1
    assert L.fmx_wb_signal(None, None) == -1 and L.fmx_wb_signal_reset(None, -1) == -1
    assert L.fmx_wb_set_signal_params(None, 0, 0.5, -4.0, -55.0, -19.0) == -1


def test_rational_design_sanitized(tmp_path):
    """fmx_wb_ratio, fmx_wb_weights_rational and fmx_wb_rational_geometry
    (fmx_wb_design.cpp + fmx_design.cpp's firdes_kaiser) under ASan + UBSan in
    a stand-alone program: host code only, nothing is loaded into Python."""
    exe = str(tmp_path / "sanitize_wb_rational")
    csrc = os.path.join(ROOT, "fmtuner-sdr_amd", "csrc")
    cmd = ["g++", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-g", "-O1", "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-o", exe,
           os.path.join(ROOT, "tests", "cpp", "sanitize_wb_rational.cpp"), os.path.join(csrc, "fmx_wb_design.cpp"),
           os.path.join(csrc, "fmx_design.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:], r.stdout[-400:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    out = json.loads(r.stdout)
    # 11 ratios x 2 formats less the two int16 refusals; 4 frequencies x Q phases each
    q = [3, 3, 15, 3, 2, 16, 1, 16, 8, 1, 1]
    assert out["bad"] == 0 and out["calls"] == 4 * (2 * sum(q) - 16 - 8) and out["rejected"] == 17 and out["tiles"] > 0
    assert np.isfinite(out["sum"])
