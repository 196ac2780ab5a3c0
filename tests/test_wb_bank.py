"""The capture bank on the CPU (fmx_wb_bank_*; the GPU
side is tests/test_gpu_wb_bank.py):

  1. fmx_wb_bank_groups, the kernel's work list: the groups of a table with a
     ragged, an empty, a short, a full and a one-channel capture; refused
     tables; a too-small cap;
  2. every entry point refuses a NULL object without touching a device;
  3. header and binding carry every name; the ABI version is still 13;
  4. the code object's metadata: the kernel instances, no scratch or spills,
     k_wbb's registers, k_wbb_level's LDS;
  5. the work-list builder under ASan + UBSan, as a stand-alone program."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np

from test_resources import _kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fmx_wb_bank_create", "fmx_wb_bank_destroy", "fmx_wb_bank_set_freq", "fmx_wb_bank_reset",
         "fmx_wb_bank_process", "fmx_wb_bank_process_block", "fmx_wb_bank_signal", "fmx_wb_bank_set_signal_params",
         "fmx_wb_bank_signal_reset", "fmx_wb_bank_groups")


def _groups(L, first, n, cap, out=None):
    t = (C.c_int * max(len(first), 1))(*first)
    buf = (C.c_int * (3 * max(cap, 1)))() if out is None else out
    return L.fmx_wb_bank_groups(t, n, buf, cap), buf


def test_groups_of_a_ragged_table(fmx):
    first = np.concatenate([[0], np.cumsum([17, 0, 5, 16, 1])]).tolist()
    want = [(0, 0, 16), (0, 16, 1), (2, 17, 5), (3, 22, 16), (4, 38, 1)]
    assert fmx.wb_bank_groups(first) == want
    g, buf = _groups(fmx.lib(), first, 5, 5)
    assert g == 5 and [tuple(buf[3 * k:3 * k + 3]) for k in range(5)] == want
    assert fmx.wb_bank_groups([0, 0, 0]) == []          # every capture empty: no work
    assert fmx.wb_bank_groups([0, 32]) == [(0, 0, 16), (0, 16, 16)]


def test_invalid_tables_and_small_cap(fmx):
    L = fmx.lib()
    assert _groups(L, [1, 2], 1, 8)[0] < 0              # first[0] != 0
    assert _groups(L, [0, 5, 4], 2, 8)[0] < 0           # decreasing
    assert _groups(L, [0], 0, 8)[0] < 0                 # no capture
    assert _groups(L, [0] * 1026, 1025, 8)[0] < 0       # more than 1024 captures
    assert _groups(L, [0] * 1025, 1024, 8)[0] == 0      # 1024 are legal
    assert L.fmx_wb_bank_groups(None, 1, None, 0) == -1
    assert _groups(L, [0, 65535 * 16 + 1], 1, 8)[0] == -4  # more groups than the grid has rows
    # a too-small cap: the needed count negated, nothing written
    first = [0, 17, 17, 22, 38, 39]
    buf = (C.c_int * 15)(*([-7] * 15))
    assert _groups(L, first, 5, 4, buf)[0] == -5
    assert list(buf) == [-7] * 15
    t = (C.c_int * 6)(*first)
    assert L.fmx_wb_bank_groups(t, 5, None, 0) == -5


def test_null_object_calls_need_no_gpu(fmx):
    L = fmx.lib()
    one = (C.c_int * 2)(0, 1)
    f = (C.c_int * 1)(0)
    bank = C.c_void_p(1)
    cfg = fmx.make_wb_config()
    assert L.fmx_wb_bank_create(None, C.byref(cfg), 1, one, f, C.byref(bank)) == -1 and not bank.value
    out = fmx.BlockOut(None, 0, None, None, 0, None, None, None, None, None, 0, None, None, None)
    assert L.fmx_wb_bank_destroy(None) == -1
    assert L.fmx_wb_bank_set_freq(None, 0, 0) == -1
    assert L.fmx_wb_bank_reset(None, -1, 0) == -1
    assert L.fmx_wb_bank_process(None, None, 0, 0, None, 0) == -1
    assert L.fmx_wb_bank_process_block(None, None, 0, 0, C.byref(out)) == -1
    assert L.fmx_wb_bank_signal(None, None) == -1
    assert L.fmx_wb_bank_set_signal_params(None, -1, 0, 0.5, -4.0, -55.0, -19.0) == -1
    assert L.fmx_wb_bank_signal_reset(None, -1) == -1


def test_names_and_abi_version(fmx):
    with open(os.path.join(ROOT, "include", "fmx.h")) as fh:
        header = fh.read()
    L = fmx.lib()
    for name in NAMES:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert getattr(L, name).argtypes is not None, name
    assert re.search(r"^#define FMX_ABI_VERSION 13$", header, re.M)
    for attr in ("process", "process_block", "signal", "set_freq", "reset", "set_signal_params", "signal_reset", "close"):
        assert callable(getattr(fmx.WidebandBank, attr)), attr
    assert callable(fmx.wb_bank_groups)


def test_code_object_metadata(tmp_path):
    ks = _kernels(tmp_path)
    pick = lambda pat: {k: v for k, v in ks.items() if re.search(pat, k)}  # noqa: E731
    wbb, hist, clip, level = pick(r"\d+k_wbbI"), pick(r"\d+k_wbb_histI"), pick(r"\d+k_wbb_clipI"), pick(r"\d+k_wbb_levelI")
    assert (len(wbb), len(hist), len(clip), len(level)) == (4, 2, 2, 3), (sorted(wbb), sorted(hist), sorted(clip), sorted(level))
    every = pick(r"\d+k_wbb")
    assert len(every) == 4 + 2 + 2 + 3 + 2, sorted(every)  # and the two one-thread state kernels
    for name, f in every.items():
        assert f.get("private_segment_fixed_size", 0) == 0, (name, f)
        assert f.get("vgpr_spill_count", 0) == 0 and f.get("sgpr_spill_count", 0) == 0, (name, f)
    for name, f in wbb.items():
        assert f.get("vgpr_count", 0) + f.get("agpr_count", 0) <= 256, (name, f)
    for name, f in level.items():
        assert f.get("group_segment_fixed_size") == 32, (name, f)


def test_group_builder_sanitized(tmp_path):
    """fmx_wb_bank_groups (fmx_wb_design.cpp) under ASan + UBSan in a
    stand-alone program: host code only, nothing is loaded into Python.  Its
    output buffers are heap blocks of exactly cap groups."""
    exe = str(tmp_path / "sanitize_wb_bank")
    csrc = os.path.join(ROOT, "fmtuner-sdr_amd", "csrc")
    cmd = ["g++", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-g", "-O1", "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-o", exe,
           os.path.join(ROOT, "tests", "cpp", "sanitize_wb_bank.cpp"), os.path.join(csrc, "fmx_wb_design.cpp"),
           os.path.join(csrc, "fmx_design.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    out = json.loads(r.stdout)
    assert out["bad"] == 0 and out["calls"] == 12 and out["rejected"] == 7 and out["groups"] > 3 * 65535
