"""The wideband channelizer's yardstick, design and test input on the CPU
(fmx_wb_*; the GPU side is tests/test_gpu_wideband.py):

  1. tests/wb_ref.py, the float64 restatement every GPU comparison uses,
     against the oracle's ComplexDecimator at f = 0;
  2. fmx_wb_weights (the kernel's f16 hi + lo tables read back) against
     2 fc h[k] e^{j 2 pi f k / Fs} in float64;
  3. configuration errors, rejected before any device is touched;
  4. the end-to-end band (four stations in one capture) is an input the oracle
     decides the same way under ten times the GPU channelizer's error;
  5. the host weight builder under ASan + UBSan, as a stand-alone program."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import gpu_harness as H
import rds_wave as W
import wb_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DSP = 240_000

# The GPU channelizer's error relative to its output, RMS over a station's
# row of the band (tests/test_gpu_wideband.py::test_band_receiver_end_to_end,
# "wb_band_rows" in the parity log, profiles/wb_parity_errors.jsonl): 1.6e-7,
# 2.6e-7, 1.6e-7 and 1.9e-7 for the four stations.  The perturbation below is
# ten times the worst.
WB_REL_RMS_GPU = 2.65e-7


@pytest.mark.parametrize("D,tpp", [(10, 28), (25, 12), (40, 28), (45, 20)])
def test_float64_restatement_against_the_oracle_decimator(oracle, D, tpp):
    """The oracle sums in f32, the restatement in float64: max |d| <= 1e-6
    (measured <= 3.7e-7).  Up to D = 45 the reference's lower clamp of the
    cut-off at 0.01 does not bind, so both design the same filter.  Guards the
    yardstick, not the product."""
    n = 600
    raw = np.random.default_rng(D).integers(0, 256, 2 * n * D, dtype=np.uint8)
    L = oracle.lib()
    dec = L.oracle_decim_create(D, tpp, 80.0)
    out = np.zeros(2 * n, np.float32)
    pos = 0
    for k in (1, 37, n - 38):  # cut anywhere: the oracle object streams
        x = np.ascontiguousarray(raw[2 * D * pos:2 * D * (pos + k)])
        assert L.oracle_decim_execute_complex(dec, x.ctypes.data, k * D, out[2 * pos:].ctypes.data, k) == k
        pos += k
    L.oracle_decim_destroy(dec)
    x = R.normalise(raw, R.U8)
    y = R.channelize(x, D, tpp, D * DSP, [0])[0]
    assert np.max(np.abs(y - out.view(np.complex64))) <= 1e-6
    # the block evaluation against the formula term by term, tuned and with a large first index
    s0, f = (1 << 40) + 12_345, -123_457
    yt = R.channelize(x, D, tpp, D * DSP, [f], sample0=s0)[0]
    for k in (0, 1, tpp, n - 1):
        assert abs(yt[k] - R.direct(x, D, tpp, D * DSP, f, k, s0)) < 1e-12


@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("D", [10, 25, 100])
def test_weight_tables_against_float64(fmx, D, fmt):
    """W[k] read back from the f16 hi + lo rows: error per tap <= 2^-21 of the
    largest tap (a 22-bit pair with one guard bit).  Scale: the rows hold W *
    2^s with the largest |W| 2^s in [2^13, 2^14), so a tap down to 2^-12 of
    the largest still has its lo half on f16's grid (spacing 2^-24 against a
    hi of at least 2): for those taps the error stays below 2^-18 of the tap
    itself -- a flushed lo half would leave up to 2^-12."""
    Fs = D * DSP
    wcfg = fmx.make_wb_config(Fs, DSP, fmt, 0, 4096)
    for f in (0, 123_457, -Fs // 2 + 1, Fs // 2):
        got = fmx.wb_weights(wcfg, f).astype(np.complex128)
        want = R.weights(D, R.tpp_rule(D), Fs, f)
        assert got.shape == want.shape == (D * R.tpp_rule(D),)
        err, top = np.abs(got - want), np.max(np.abs(want))
        assert np.max(err) <= top * 2.0 ** -21, (D, fmt, f, np.max(err) / top)
        big = np.abs(want) >= top * 2.0 ** -12
        assert big.sum() > len(want) // 2
        assert np.max(err[big] / np.abs(want[big])) <= 2.0 ** -18, (D, fmt, f)
        assert np.all(np.abs(got[np.abs(want) > top * 2.0 ** -30]) > 0)


def test_invalid_wideband_config_rejected_before_device(fmx):
    L = fmx.lib()

    def rc(wide=2_400_000, dsp=DSP, fmt=0, tpp=0, block=4096, f=0):
        cfg = fmx.make_wb_config(wide, dsp, fmt, tpp, block)
        return L.fmx_wb_weights(ctypes.byref(cfg), f, None, 0)

    assert rc() == 2 * 280 and rc(tpp=4) == 2 * 40 and rc(wide=128 * DSP, tpp=28) == 2 * 128 * 28
    assert rc(wide=2_400_001) == -1       # no multiple of dsp_rate
    assert rc(wide=DSP) == -1             # D = 1
    assert rc(wide=129 * DSP) == -1       # D > 128
    assert rc(tpp=3) == -1 and rc(tpp=29) == -1
    assert rc(fmt=2) == -1
    assert rc(f=1_200_000) > 0 and rc(f=-1_200_000) > 0
    assert rc(f=1_200_001) == -1 and rc(f=-1_200_001) == -1  # |f| > Fs / 2
    # fmx_wb_create needs a handle: without one nothing is created
    wb = ctypes.c_void_p(1)
    cfg = fmx.make_wb_config()
    f = (ctypes.c_int * 1)(0)
    assert L.fmx_wb_create(None, ctypes.byref(cfg), f, 1, ctypes.byref(wb)) == -1 and not wb.value


def test_band_input_is_stable_under_ten_times_the_gpu_error(fmx, oracle):
    """The composite of the GPU end-to-end test through the float64
    channelizer and the oracle's objects: every group with an error-free block
    A carries PI 0x1000 + station, and neither the groups nor the stereo flags
    of any call change when the channelizer's rows are perturbed by complex
    Gaussian noise of ten times the GPU channelizer's relative RMS error
    (WB_REL_RMS_GPU, two seeds).  Amplitudes found unsuitable on the way: the
    fourth station at 0.10 (its acquisition flips under 1e-5)."""
    raw = R.band_capture(fmx)
    ref = R.band_reference(raw)
    assert WB_REL_RMS_GPU > 0
    noise = 10.0 * WB_REL_RMS_GPU
    jobs = [(c, s) for c in range(4) for s in (None, 1, 2)]
    res = dict(zip(jobs, W.pmap(
        lambda j: R.oracle_chain(H, oracle, ref[j[0]].astype(np.complex64), noise if j[1] else 0.0, j[1] or 0),
        jobs)))
    for c in range(4):
        base = res[(c, None)]
        groups = [g for r in base for g in r["groups"]]
        assert len(groups) >= 2, (c, groups)
        for g in groups:
            if (g[4] >> 6) == 0:
                assert g[0] == 0x1000 + R.BAND_CH0 + c, (c, g)
        assert base[-1]["stereo"] == 1, c
        for s in (1, 2):
            got = res[(c, s)]
            assert [r["groups"] for r in got] == [r["groups"] for r in base], (c, s)
            assert [r["stereo"] for r in got] == [r["stereo"] for r in base], (c, s)
    rms = lambda v: float(np.sqrt(np.mean(np.abs(v[R.BAND_HEAD:]) ** 2)))  # noqa: E731
    assert rms(ref[4]) < rms(ref[3]) / 50.0


def test_weight_builder_sanitized(tmp_path):
    """fmx_wb_design.cpp (+ fmx_design.cpp's firdes_kaiser) under ASan + UBSan
    in a stand-alone program: host code only, nothing is loaded into Python."""
    exe = str(tmp_path / "wb_sanitize")
    csrc = os.path.join(ROOT, "fmtuner-sdr_amd", "csrc")
    cmd = ["g++", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-g", "-O1", "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-o", exe,
           os.path.join(ROOT, "tests", "cpp", "wb_sanitize_main.cpp"), os.path.join(csrc, "fmx_wb_design.cpp"),
           os.path.join(csrc, "fmx_design.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    out = json.loads(r.stdout)
    assert out["bad"] == 0 and out["calls"] == 9 * 2 * 7 and out["rejected"] == 11 and np.isfinite(out["sum"])
