"""The band receiver's RF level without a GPU (fmx_wb_signal and its helpers,
DESIGN.md section 21): the XDR "S" line formatter, the NULL-object returns,
the binding's names, the ABI version and k_wb_level's resources.

fmx_xdr_signal_line is XDRServer::updateSignal + buildSignalLine
(xdr_server.cpp:368-397).  The float32 restatement below is its only pin:
oracle/refdrv/xdr_driver.cpp drops the server's S lines, so no fixture of the
reference's own output exists for them."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from test_resources import _find, _kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def s_line(level, stereo, forced_mono, cci, aci):
    """updateSignal's tenths in float32 (clamp, x 10, round half away from
    zero), buildSignalLine's mode letter and one-decimal text."""
    lv = np.float32(level)
    lv = np.float32(0.0) if lv < np.float32(0.0) else (np.float32(120.0) if lv > np.float32(120.0) else lv)
    t = np.float32(lv * np.float32(10.0))
    deci = int(np.floor(np.float64(t) + 0.5))  # t >= 0: half away from zero; exact in double
    mode = ("S" if stereo else "M") if forced_mono else ("s" if stereo else "m")
    return "S%s%.1f,%d,%d\n" % (mode, deci / 10.0, cci, aci)


def call(fmx, level, stereo=0, forced_mono=0, cci=-1, aci=-1, cap=64):
    buf = C.create_string_buffer(b"\xaa" * 64, 64)
    rc = fmx.lib().fmx_xdr_signal_line(C.c_float(level), stereo, forced_mono, cci, aci, buf, cap)
    return rc, buf.raw


@pytest.mark.parametrize("stereo,forced,letter", [(0, 0, "m"), (1, 0, "s"), (0, 1, "M"), (1, 1, "S")])
def test_mode_letters(fmx, stereo, forced, letter):
    rc, raw = call(fmx, 57.3, stereo, forced)
    want = s_line(57.3, stereo, forced, -1, -1)
    assert want == "S" + letter + "57.3,-1,-1\n"
    assert rc == len(want) and raw[:rc + 1] == want.encode() + b"\0"
    assert fmx.xdr_signal_line(57.3, bool(stereo), bool(forced)) == want


@pytest.mark.parametrize("level", [-3.0, -0.04, 0.0, 0.04, 0.05, 33.333, 99.96, 119.96, 120.0, 120.04, 500.0, 1e30, -1e30])
def test_clamp_and_rounding(fmx, level):
    rc, raw = call(fmx, level)
    want = s_line(level, 0, 0, -1, -1)
    assert rc == len(want) and raw[:rc] == want.encode(), (level, raw[:rc], want)
    v = float(want[2:].split(",")[0])
    assert 0.0 <= v <= 120.0


def test_halves_round_in_float(fmx):
    """42.25 x 10 is 422.5 exactly: away from zero, 42.3 (half-even would give
    42.2).  float32(0.45) lies below 0.45, its float product with 10 is 4.5
    exactly (5 tenths); the same product in double stays below 4.5 (4
    tenths)."""
    assert np.float32(42.25) * np.float32(10.0) == np.float32(422.5)
    assert call(fmx, 42.25)[1].startswith(b"Sm42.3,-1,-1\n\0")
    x = np.float32(0.45)
    assert float(x) < 0.45 and np.float32(x * np.float32(10.0)) == np.float32(4.5) and float(x) * 10.0 < 4.5
    assert s_line(x, 0, 0, -1, -1) == "Sm0.5,-1,-1\n"
    assert call(fmx, float(x))[1].startswith(b"Sm0.5,-1,-1\n\0")
    for lv in (0.05, 0.15, 0.25, 7.75, 61.35, 119.95):  # more values at or beside a half
        rc, raw = call(fmx, lv)
        assert raw[:rc] == s_line(lv, 0, 0, -1, -1).encode(), lv


def test_cci_aci_and_small_buffer(fmx):
    rc, raw = call(fmx, 88.8, 1, 0, 37, 4)
    assert raw[:rc + 1] == b"Ss88.8,37,4\n\0" == s_line(88.8, 1, 0, 37, 4).encode() + b"\0"
    rc, raw = call(fmx, 5.0, 0, 1, 0, 100)
    assert raw[:rc + 1] == b"SM5.0,0,100\n\0"
    # too small: -(bytes needed + 1), nothing written; the line and its NUL need len + 1
    n = len("Ss88.8,37,4\n")
    for cap in (0, 1, n):
        rc, raw = call(fmx, 88.8, 1, 0, 37, 4, cap=cap)
        assert rc == -(n + 1) and raw == b"\xaa" * 64, (cap, rc)
    rc, raw = call(fmx, 88.8, 1, 0, 37, 4, cap=n + 1)
    assert rc == n and raw[n + 1:] == b"\xaa" * (63 - n)
    assert fmx.lib().fmx_xdr_signal_line(C.c_float(1.0), 0, 0, -1, -1, None, 64) == -(len("Sm1.0,-1,-1\n") + 1)


def test_null_object_is_invalid_without_a_gpu(fmx):
    L = fmx.lib()
    lv = (fmx.SignalLevel * 2)()
    assert L.fmx_wb_signal(None, C.cast(lv, C.c_void_p)) == -1
    assert L.fmx_wb_signal(None, None) == -1
    assert L.fmx_wb_set_signal_params(None, 0, 0.5, -4.0, -55.0, -19.0) == -1
    assert L.fmx_wb_signal_reset(None, -1) == -1 and L.fmx_wb_signal_reset(None, 0) == -1


def test_binding_and_header_carry_the_names(fmx):
    L = fmx.lib()
    for name in ("fmx_wb_signal", "fmx_wb_set_signal_params", "fmx_wb_signal_reset", "fmx_xdr_signal_line"):
        f = getattr(L, name)
        assert f.argtypes is not None and f.restype is C.c_int, name
    for name in ("signal", "set_signal_params", "signal_reset"):
        assert callable(getattr(fmx.Wideband, name)), name
    assert callable(fmx.xdr_signal_line)
    with open(os.path.join(ROOT, "include", "fmx.h")) as f:
        text = f.read()
    assert re.search(r"#define FMX_ABI_VERSION 13\b", text)
    for name in ("fmx_wb_signal", "fmx_wb_set_signal_params", "fmx_wb_signal_reset", "fmx_xdr_signal_line"):
        assert re.search(r"\bint " + name + r"\(", text), name


def test_signal_line_sanitized(tmp_path):
    """tests/cpp/sanitize_signal_line.cpp, a stand-alone program, built from
    source with fmx_host.cpp under ASan + UBSan and run directly: every level
    class, mode and cap, into heap buffers of exactly cap bytes."""
    exe = str(tmp_path / "sanitize_signal_line")
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-g", "-O1", "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "sanitize_signal_line.cpp"),
                    os.path.join(ROOT, "fmtuner-sdr_amd", "csrc", "fmx_host.cpp")], check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    out = json.loads(r.stdout)
    assert out["lines"] == (17 + 1201) * 4 * 5 and out["refused"] > out["lines"] and out["bytes"] > 0, out


def test_level_kernel_budget(tmp_path):
    """k_wb_level: three instances (16-, 8- and 4-byte loads), a handful of
    registers, its 32 bytes of LDS (four doubles) and no scratch."""
    hits = _find(_kernels(tmp_path), r"10k_wb_levelILi(16|8|4)EEEvNS_11WbLevelArgs")
    assert len(hits) == 3, sorted(hits)
    for name, f in hits.items():
        assert f.get("vgpr_count", 0) <= 64 and f.get("agpr_count", 0) == 0, (name, f)
        assert f.get("vgpr_spill_count", 0) == 0 and f.get("sgpr_spill_count", 0) == 0, (name, f)
        assert f.get("private_segment_fixed_size", 0) == 0 and f.get("group_segment_fixed_size", 0) == 32, (name, f)
