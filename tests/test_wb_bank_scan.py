"""The band scan over a capture bank (fmx_wb_bank_scan_*)
without a GPU:
  1. the header, the ABI history and the binding name the six symbols;
  2. every call with a NULL object returns FMX_E_INVALID;
  3. fmx_wb_bank_scan_groups against a Python restatement over random tables
     (empty captures, counts of exactly 64 and 65, 1024 captures), the
     cap-too-small convention and the refused tables;
  4. the code object's metadata: k_bscan's four instances and k_bscan_level,
     no scratch, no spills, no AGPRs, no static LDS, k_bscan <= 170 VGPRs
     (three waves per SIMD: one more than the two workgroups per CU its 80 KB
     of LDS allow, so registers never set the occupancy), k_bscan_level <= 64;
     the sibling tests' kernel counts hold and no new name matches their
     patterns;
  5. the float64 reference on its own: capture s reads row s."""
import ctypes as C
import inspect
import os
import re

import numpy as np

import wb_bank_scan_ref as B
import wb_ref as R
from test_resources import _kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fmx_wb_bank_scan_create", "fmx_wb_bank_scan_destroy", "fmx_wb_bank_scan_set_signal_params",
         "fmx_wb_bank_scan_reset", "fmx_wb_bank_scan_process", "fmx_wb_bank_scan_groups")


def test_header_and_binding(fmx):
    with open(os.path.join(ROOT, "include", "fmx.h")) as fh:
        header = fh.read()
    L = fmx.lib()
    for name in NAMES:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert getattr(L, name).argtypes is not None, name
    assert re.search(r"^#define FMX_ABI_VERSION 13$", header, re.M)
    assert "fmx_wb_bank_scan_create" in header.split("#define FMX_ABI_VERSION")[0]  # the ABI history names it
    assert list(inspect.signature(fmx.WidebandBankScan.__init__).parameters) == ["self", "handle", "wcfg",
                                                                                 "freqs_per_capture"]
    assert list(inspect.signature(fmx.WidebandBankScan.process).parameters) == ["self", "d_wide", "wide_stride",
                                                                                "n_out", "d_level"]
    assert inspect.signature(fmx.WidebandBankScan.set_signal_params).parameters["capture"].default == -1
    assert inspect.signature(fmx.WidebandBankScan.reset).parameters["capture"].default == -1
    assert callable(fmx.WidebandBankScan.close) and callable(fmx.wb_bank_scan_groups)


def test_null_object_calls_need_no_gpu(fmx):
    L = fmx.lib()
    one = (C.c_int * 2)(0, 1)
    f = (C.c_int * 1)(0)
    obj = C.c_void_p(1)
    cfg = fmx.make_wb_config()
    assert L.fmx_wb_bank_scan_create(None, C.byref(cfg), 1, one, f, C.byref(obj)) == -1 and not obj.value
    assert L.fmx_wb_bank_scan_destroy(None) == -1
    assert L.fmx_wb_bank_scan_set_signal_params(None, -1, 0, 0.5, -4.0, -55.0, -19.0) == -1
    assert L.fmx_wb_bank_scan_reset(None, -1) == -1
    assert L.fmx_wb_bank_scan_process(None, None, 0, 64, None) == -1


def _groups(L, first, n, cap, out=None):
    t = (C.c_int * max(len(first), 1))(*first)
    buf = (C.c_int * (3 * max(cap, 1)))() if out is None else out
    return L.fmx_wb_bank_scan_groups(t, n, buf, cap), buf


def test_work_list_against_a_restatement(fmx):
    L = fmx.lib()
    rng = np.random.default_rng(28)
    tables = [[19, 0, 70], [64], [65], [0, 64, 0, 65, 1], [0] * 1024, [1] * 1024, [8192], [63, 128, 129]]
    for _ in range(300):
        S = int(rng.integers(1, 40))
        tables.append(rng.choice([0, 0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 200], S).tolist())
    for counts in tables:
        first = B.first_point([[0] * c for c in counts])
        want = B.groups(first)
        assert all(1 <= g[2] <= 64 for g in want)
        assert fmx.wb_bank_scan_groups(first) == want, counts
        g, buf = _groups(L, first, len(counts), len(want))  # a buffer of exactly G entries
        assert g == len(want) and [tuple(buf[3 * k:3 * k + 3]) for k in range(g)] == want, counts
    assert fmx.wb_bank_scan_groups([0, 19, 19, 89]) == [(0, 0, 19), (2, 19, 64), (2, 83, 6)]
    assert fmx.wb_bank_scan_groups([0, 0, 0]) == []  # every capture empty: no work


def test_refused_tables_and_small_cap(fmx):
    L = fmx.lib()
    assert _groups(L, [1, 2], 1, 8)[0] == -1             # first_point[0] != 0
    assert _groups(L, [0, 5, 4], 2, 8)[0] == -1          # decreasing
    assert _groups(L, [0], 0, 8)[0] == -1                # no capture
    assert _groups(L, [0] * 1026, 1025, 8)[0] == -1      # more than 1024 captures
    assert _groups(L, [0] * 1025, 1024, 8)[0] == 0       # 1024 are legal
    assert L.fmx_wb_bank_scan_groups(None, 1, None, 0) == -1
    # a too-small cap: the needed count negated, nothing written
    first = [0, 19, 19, 89, 153, 154]
    buf = (C.c_int * 15)(*([-7] * 15))
    assert _groups(L, first, 5, 4, buf)[0] == -5
    assert list(buf) == [-7] * 15
    t = (C.c_int * 6)(*first)
    assert L.fmx_wb_bank_scan_groups(t, 5, None, 0) == -5


def test_code_object_metadata(tmp_path):
    ks = _kernels(tmp_path)
    pick = lambda pat: {k: v for k, v in ks.items() if re.search(pat, k)}  # noqa: E731
    main, level = pick(r"7k_bscanILb[01]ELb[01]E"), pick(r"13k_bscan_levelE")
    assert (len(main), len(level)) == (4, 1), (sorted(main), sorted(level))
    assert len(pick(r"k_bscan")) == 5, sorted(pick(r"k_bscan"))
    for name, f in {**main, **level}.items():
        print(name, f)
        assert "BscanArgs" in name, name
        assert f.get("private_segment_fixed_size", 0) == 0, (name, f)
        assert f.get("vgpr_spill_count", 0) == 0 and f.get("sgpr_spill_count", 0) == 0, (name, f)
        assert f.get("agpr_count", 0) == 0, (name, f)
        assert f.get("group_segment_fixed_size", 0) == 0, (name, f)  # k_bscan's LDS is dynamic
    for name, f in main.items():
        assert 0 < f.get("vgpr_count", 0) <= 170, (name, f)
    for name, f in level.items():
        assert 0 < f.get("vgpr_count", 0) <= 64, (name, f)
    # what the sibling tests count is what it was, and the new names match none of their patterns
    assert len(pick(r"\d+k_wbb")) == 13 and len(pick(r"\d+k_wbr")) == 6 and len(pick(r"k_bank_iqc")) == 8
    assert len(pick(r"k_rbank")) == 6 and len(pick(r"9k_wb_scanILb[01]ELb[01]E.*WbScanArgs")) == 4
    assert pick(r"8k_wb_iqcI") and pick(r"13k_wb_scan_iqcI")
    for pat in (r"\d+k_wbb", r"\d+k_wbr", r"k_bank_iqc", r"k_rbank", r"k_wb_scan", r"WbScanArgs", r"8k_wb_iqcI",
                r"13k_wb_scan_iqcI"):
        assert not [k for k in {**main, **level} if re.search(pat, k)], pat


def test_reference_reads_each_captures_own_row():
    """Three u8 captures at D = 10, each a tone 7 kHz off one of its 9 points
    (another point per capture) over noise: the reference's strongest point of
    a capture is that capture's tone, and the points of the other captures'
    tones read at least 20 dB lower there."""
    D, tpp, dsp, n_out = 10, 28, 240_000, 160
    Fs = D * dsp
    freqs = [[-800_000 + 200_000 * p for p in range(9)]] * 3
    tone_at = (1, 4, 7)
    rng = np.random.default_rng(5)
    i = np.arange(n_out * D, dtype=np.int64)
    rows = []
    for s in range(3):
        x = (1e-3 / np.sqrt(2.0)) * (rng.normal(size=i.size) + 1j * rng.normal(size=i.size))
        turns = (((freqs[s][tone_at[s]] + 7_000) % Fs) * i) % Fs
        x += 0.3 * np.exp(2j * np.pi * turns / Fs)
        raw = np.empty(2 * i.size, np.uint8)
        raw[0::2] = np.clip(np.rint(x.real * 127.5 + 127.5), 0, 255)
        raw[1::2] = np.clip(np.rint(x.imag * 127.5 + 127.5), 0, 255)
        rows.append(raw)
    rec = B.scan_call(rows, R.U8, D, tpp, Fs, freqs, n_out)
    assert len(rec) == 27
    first = B.first_point(freqs)
    for s in range(3):
        db = np.array([r["dbfs"] for r in rec[first[s]:first[s + 1]]])
        assert int(np.argmax(db)) == tone_at[s], (s, db)
        for o in range(3):
            if o != s:
                assert db[tone_at[s]] - db[tone_at[o]] >= 20.0, (s, o, db)
