"""DC-offset and IQ-imbalance correction of wide captures on the CPU
(fmx_wb_set_iq_correction, fmx_iq_estimate; the GPU side
is tests/test_gpu_wb_iqcorr.py):

  1. fmx_iq_estimate against tests/wb_iq_ref.py's estimator (exact integer
     sums, then a dozen double operations: 1e-12 relative), the degenerate
     inputs and the refused arguments;
  2. the correction does what it is for, on the float64 reference alone: the
     image of an FM station, 27 dB down in the impaired capture, falls below
     -45 dB with the estimate of the same samples;
  3. the code object's metadata of the new kernels;
  4. header and binding carry every name; the calls refuse a NULL object
     without touching a device;
  5. the host estimator under ASan + UBSan, as a stand-alone program."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import wb_iq_ref as Q
import wb_ref as R
from test_resources import LLVM, _kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fmx_wb_set_iq_correction", "fmx_wb_iq_correction", "fmx_wb_scan_set_iq_correction",
         "fmx_wb_scan_iq_correction", "fmx_iq_estimate")
FMTS = [R.U8, R.S16]
IMAGE_BEFORE_DB = (-29.0, -25.0)  # the uncorrected image of impaired_capture
IMAGE_AFTER_DB = -45.0            # at most, corrected


def _random_raw(fmt, n, seed, plant=None):
    """Noise of about a third of full scale; plant = (dc_i, dc_q, q_gain, skew) in units of x / radians."""
    rng = np.random.default_rng(seed)
    i, q = rng.normal(size=n) * 0.3, rng.normal(size=n) * 0.3
    if plant:
        dc_i, dc_q, g, sk = plant
        q = g * (q * np.cos(sk) + i * np.sin(sk)) + dc_q
        i = i + dc_i
    raw = np.empty(2 * n, np.uint8 if fmt == R.U8 else np.int16)
    if fmt == R.U8:
        raw[0::2], raw[1::2] = (np.clip(np.rint(v * 127.5 + 127.5), 0, 255) for v in (i, q))
    else:
        raw[0::2], raw[1::2] = (np.clip(np.rint(v * 32768.0), -32768, 32767) for v in (i, q))
    return raw


def _close(got, want, tol=1e-12):
    return all(abs(g - w) <= tol * max(abs(w), 1e-300) or g == w for g, w in zip(got, want))


@pytest.mark.parametrize("fmt", FMTS)
def test_estimate_against_the_reference(fmx, fmt):
    """Random buffers of 1, 2, 4097 and 50 000 samples, with and without
    planted imbalance: every field within 1e-12 relative of wb_iq_ref.estimate."""
    for n, plant in ((50_000, None), (50_000, (0.03, -0.02, 1.1, 0.08)), (4097, (-0.1, 0.05, 0.9, -0.05)),
                     (2, None), (1, None)):
        raw = _random_raw(fmt, n, 11 + n, plant)
        got = fmx.iq_estimate(raw, fmt)
        want, _ = Q.estimate(raw, fmt)
        assert _close(got, want), (fmt, n, plant, got, want)
    # the planted front end is found: gain and cross of its inverse within the noise of 50 000 samples
    raw = _random_raw(fmt, 50_000, 3, (0.03, -0.02, 1.1, 0.08))
    dc_i, dc_q, gain, cross = fmx.iq_estimate(raw, fmt)
    assert abs(dc_i - 0.03) < 5e-3 and abs(dc_q + 0.02) < 5e-3
    assert abs(gain - 1.0 / (1.1 * np.cos(0.08))) < 0.02 and abs(cross + np.tan(0.08)) < 0.02


@pytest.mark.parametrize("fmt", FMTS)
def test_estimate_degenerate_inputs(fmx, fmt):
    """All samples equal (no variance), Q a multiple of I (no independent Q
    component) and Q constant: gain 1, cross 0; the DC still comes out."""
    n = 1000
    dt = np.uint8 if fmt == R.U8 else np.int16
    flat = np.full(2 * n, 77, dt)
    dc = (2 * 77 - 255) / 255.0 if fmt == R.U8 else 77 / 32768.0
    assert fmx.iq_estimate(flat, fmt) == (dc, dc, 1.0, 0.0)
    rng = np.random.default_rng(5)
    i = rng.integers(-40, 41, n)
    # the raw value of byte b is v = 2 b - 255: b = i + 128 is v = 2 i + 1, and b = 3 i + 129 is 3 v
    triple = (i + 128, 3 * i + 129) if fmt == R.U8 else (i, 3 * i)
    const = (i + 128, np.full(n, 128)) if fmt == R.U8 else (i, np.zeros(n, np.int64))
    for vi, vq in (triple, const):
        raw = np.empty(2 * n, dt)
        raw[0::2], raw[1::2] = vi, vq
        got = fmx.iq_estimate(raw, fmt)
        want, _ = Q.estimate(raw, fmt)
        assert got[2:] == (1.0, 0.0) and want[2:] == (1.0, 0.0), (fmt, got, want)
        assert _close(got, want)


def test_estimate_refuses(fmx):
    L = fmx.lib()
    raw = np.zeros(8, np.int16)
    out = fmx.IqCorrection()
    p = raw.ctypes.data_as(C.c_void_p)
    assert L.fmx_iq_estimate(p, 1, 0, C.byref(out)) == -1 and L.fmx_iq_estimate(p, 1, -3, C.byref(out)) == -1
    assert L.fmx_iq_estimate(p, 2, 4, C.byref(out)) == -1 and L.fmx_iq_estimate(p, -1, 4, C.byref(out)) == -1
    assert L.fmx_iq_estimate(None, 1, 4, C.byref(out)) == -1 and L.fmx_iq_estimate(p, 1, 4, None) == -1
    assert L.fmx_iq_estimate(p, 1, 4, C.byref(out)) == 0


def test_reference_smoothing_and_identity():
    """The reference's own pieces: alpha = 1 forgets the state, the first call
    initialises it, and correct() with the identity is the identity."""
    a, b = _random_raw(R.S16, 500, 1, (0.1, 0.0, 1.2, 0.1)), _random_raw(R.S16, 500, 2)
    pa, sa = Q.estimate(a, R.S16)
    pb, _ = Q.estimate(b, R.S16)
    assert _close(Q.estimate(b, R.S16, sa, 1.0)[0], pb, 1e-12)  # m + 1 (c - m) is c up to rounding
    pm, sm = Q.estimate(b, R.S16, sa, 0.25)
    assert pa[0] > pm[0] > pb[0]
    assert np.allclose(sm, [x + 0.25 * (y - x) for x, y in zip(sa, Q.estimate(b, R.S16)[1])], rtol=1e-15)
    x = np.array([0.25 - 0.5j, -1 + 1j])
    assert np.array_equal(Q.correct(x, Q.IDENTITY), x)
    # the correction undoes a front end exactly when handed its inverse
    sk = 0.07
    y = (x.real + 0.02) + 1j * (1.06 * (x.imag * np.cos(sk) + x.real * np.sin(sk)) - 0.015)
    assert np.max(np.abs(Q.correct(y, (0.02, -0.015, 1.0 / (1.06 * np.cos(sk)), -np.tan(sk))) - x)) < 1e-15


def image_rejection_reference(fmt):
    """(uncorrected, corrected with the estimate of the same samples) image
    ratio in dB of impaired_capture through the float64 channelizer, D = 10,
    channels at +300 kHz and -300 kHz."""
    raw = Q.impaired_capture(fmt)
    p, _ = Q.estimate(raw, fmt)
    freqs = [Q.CAP_STATION_HZ, -Q.CAP_STATION_HZ]
    x = R.normalise(raw, fmt)
    before = R.channelize(x, 10, 28, Q.CAP_FS, freqs)
    after = R.channelize(Q.correct(x, p), 10, 28, Q.CAP_FS, freqs)
    return Q.image_ratio_db(before), Q.image_ratio_db(after), p


@pytest.mark.parametrize("fmt", FMTS)
def test_correction_rejects_the_image_on_the_reference(fmt):
    """Uncorrected the image lies between -29 and -25 dB; corrected with the
    estimate of the same 96 000 samples at most -45 dB.  Reference's figures
    (mean |y|^2 over the rows' 9600 outputs): u8 -26.82 -> -49.99 dB, int16
    -26.83 -> -51.74 dB; the estimate is within 2e-4 of the front end's inverse
    (the noise of 96 000 samples: u8 gain 0.945767 against 0.945700)."""
    before, after, p = image_rejection_reference(fmt)
    print(f"image fmt {fmt}: before {before:.2f} dB, after {after:.2f} dB, p {p}, true {Q.CAP_TRUE}")
    assert IMAGE_BEFORE_DB[0] <= before <= IMAGE_BEFORE_DB[1], before
    assert after <= IMAGE_AFTER_DB, after
    assert max(abs(a - b) for a, b in zip(p, Q.CAP_TRUE)) < 2e-4, (p, Q.CAP_TRUE)


def test_code_object_metadata(tmp_path):
    """k_wb_iqc and k_wb_scan_iqc (int16 / u8 x D even / odd each), the
    estimator k_iqc_sums (u8, int16), k_iqc_finish and k_iqc_fixed: no
    scratch, no spills, no AGPRs; every corrected instance in the occupancy
    class of its uncorrected counterpart (512 // VGPRs equal; k_wb is at
    112 / 104, so <= 128); the estimator has static LDS only (160 bytes).
    Built: k_wb_iqc 120 (int16) / 112 (u8) against k_wb's 112 / 104;
    k_wb_scan_iqc 144 / 128 against k_wb_scan's 142 / 126; k_iqc_sums 56 / 62."""
    ks = _kernels(tmp_path)
    pick = lambda pat: {k: v for k, v in ks.items() if re.search(pat, k)}  # noqa: E731
    wb, scan = pick(r"8k_wb_iqcILb[01]ELb[01]E"), pick(r"13k_wb_scan_iqcILb[01]ELb[01]E")
    sums, one = pick(r"10k_iqc_sumsI[sh]E"), pick(r"(12k_iqc_finishE|11k_iqc_fixedE)")
    assert (len(wb), len(scan), len(sums), len(one)) == (4, 4, 2, 2), (sorted(wb), sorted(scan), sorted(sums), sorted(one))
    # .agpr_count opens a kernel's entry in the notes; its .name follows in the same entry
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", str(tmp_path / "k.co")], check=True,
                           capture_output=True, text=True).stdout
    agprs = {m.group(2): int(m.group(1))
             for m in re.finditer(r"- \.agpr_count:\s+(\d+)\n(?:(?!\s+- \.agpr_count).*\n)*?\s+\.name:\s+(\S+)", notes)}
    for name, f in {**wb, **scan, **sums, **one}.items():
        print(name, f, "agprs", agprs.get(name))
        assert agprs.get(name) == 0, (name, agprs.get(name))
        assert f.get("private_segment_fixed_size", 0) == 0, (name, f)
        assert f.get("vgpr_spill_count", 0) == 0 and f.get("sgpr_spill_count", 0) == 0, (name, f)
        assert f.get("agpr_count", 0) == 0, (name, f)
    for name, f in {**wb, **scan}.items():
        twin = name.replace("8k_wb_iqcI", "4k_wbI").replace("13k_wb_scan_iqcI", "9k_wb_scanI")
        twin = re.sub(r"PK11FmxIqcBlockPKf$", "", twin)
        assert twin in ks and twin != name, (name, twin)
        assert 512 // f["vgpr_count"] == 512 // ks[twin]["vgpr_count"], (name, f, ks[twin])
    for f in wb.values():
        assert f["vgpr_count"] <= 128
    for name, f in sums.items():
        assert f.get("group_segment_fixed_size", 0) <= 160, (name, f)


def test_names_struct_and_abi_version(fmx):
    with open(os.path.join(ROOT, "include", "fmx.h")) as fh:
        header = fh.read()
    L = fmx.lib()
    for name in NAMES:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert getattr(L, name).argtypes is not None, name
    assert re.search(r"^#define FMX_ABI_VERSION 13$", header, re.M)
    assert re.search(r"typedef struct \{ double dc_i, dc_q, gain, cross; \} fmx_iq_correction;", header)
    assert re.search(r"enum \{ FMX_IQC_OFF = 0, FMX_IQC_FIXED = 1, FMX_IQC_AUTO = 2 \};", header)
    assert C.sizeof(fmx.IqCorrection) == 32
    assert [n for n, _ in fmx.IqCorrection._fields_] == ["dc_i", "dc_q", "gain", "cross"]
    assert (fmx.FMX_IQC_OFF, fmx.FMX_IQC_FIXED, fmx.FMX_IQC_AUTO) == (0, 1, 2)
    for cls in (fmx.Wideband, fmx.WidebandScan):
        assert callable(cls.set_iq_correction) and callable(cls.iq_correction)
    assert callable(fmx.iq_estimate)


def test_estimator_sanitized(tmp_path):
    """fmx_iq_estimate (fmx_wb_design.cpp + fmx_iqc.h) under ASan + UBSan in a
    stand-alone program: host code only, nothing is loaded into Python."""
    exe = str(tmp_path / "sanitize_iq_estimate")
    csrc = os.path.join(ROOT, "fmtuner-sdr_amd", "csrc")
    cmd = ["g++", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-g", "-O1", "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-o", exe,
           os.path.join(ROOT, "tests", "cpp", "sanitize_iq_estimate.cpp"), os.path.join(csrc, "fmx_wb_design.cpp"),
           os.path.join(csrc, "fmx_design.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:], r.stdout[-400:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    out = json.loads(r.stdout)
    assert out["bad"] == 0 and out["calls"] == 11 and out["rejected"] == 5 and np.isfinite(out["sum"])


def test_null_object_calls_need_no_gpu(fmx):
    L = fmx.lib()
    p = fmx.IqCorrection(0.0, 0.0, 1.0, 0.0)
    assert L.fmx_wb_set_iq_correction(None, fmx.FMX_IQC_FIXED, C.byref(p), 0.0) == -1
    assert L.fmx_wb_iq_correction(None, C.byref(p)) == -1
    assert L.fmx_wb_scan_set_iq_correction(None, fmx.FMX_IQC_AUTO, None, 0.5) == -1
    assert L.fmx_wb_scan_iq_correction(None, C.byref(p)) == -1
