"""The capture bank at rational rates on the CPU (fmx_wb_bank_create_rational,
DESIGN.md section 27; the GPU side is tests/test_gpu_wb_bank_rational.py):

  1. header and binding carry the new name; the ABI version is still 13;
     WidebandBank's `rational` defaults to False;
  2. every bank call refuses a NULL object without touching a device;
  3. the code object's metadata: k_rbank's four instances (int16 / u8 x P
     even / odd) and k_rbank_hist's two, no scratch, no spills, no AGPRs,
     VGPRs within k_wbr's class (<= 112 int16, <= 104 u8; built: 112 / 110 and
     104 / 102, k_wbr's own figures); the counts the sibling tests assert (13 k_wbb*, 6 k_wbr*,
     8 k_bank_iqc*) still hold and no new name matches their patterns.

No host helper was added outside the HIP translation units (the sample-count
arithmetic sits beside wb_consumed in fmx_capi.cpp), so there is no new
stand-alone sanitizer program."""
import ctypes as C
import inspect
import os
import re

from test_resources import _kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DSP = 240_000


def test_names_and_abi_version(fmx):
    with open(os.path.join(ROOT, "include", "fmx.h")) as fh:
        header = fh.read()
    L = fmx.lib()
    assert re.search(r"\bint fmx_wb_bank_create_rational\(", header)
    assert L.fmx_wb_bank_create_rational.argtypes is not None
    assert L.fmx_wb_bank_create_rational.argtypes == L.fmx_wb_bank_create.argtypes
    assert re.search(r"^#define FMX_ABI_VERSION 13$", header, re.M)
    assert "fmx_wb_bank_create_rational" in header.split("#define FMX_ABI_VERSION")[0]  # the ABI history names it
    assert inspect.signature(fmx.WidebandBank.__init__).parameters["rational"].default is False
    assert callable(fmx.WidebandBank.consumed)


def test_null_object_calls_need_no_gpu(fmx):
    L = fmx.lib()
    one = (C.c_int * 2)(0, 1)
    f = (C.c_int * 1)(0)
    bank = C.c_void_p(1)
    cfg = fmx.make_wb_config(2_048_000, DSP, 0, 0, 4096)
    assert L.fmx_wb_bank_create_rational(None, C.byref(cfg), 1, one, f, C.byref(bank)) == -1 and not bank.value
    out = fmx.BlockOut(None, 0, None, None, 0, None, None, None, None, None, 0, None, None, None)
    assert L.fmx_wb_bank_destroy(None) == -1
    assert L.fmx_wb_bank_set_freq(None, 0, 0) == -1
    assert L.fmx_wb_bank_reset(None, -1, 0) == -1
    assert L.fmx_wb_bank_process(None, None, 0, 15, None, 15) == -1
    assert L.fmx_wb_bank_process_block(None, None, 0, 15, C.byref(out)) == -1
    assert L.fmx_wb_bank_signal(None, None) == -1
    assert L.fmx_wb_bank_set_signal_params(None, -1, 0, 0.5, -4.0, -55.0, -19.0) == -1
    assert L.fmx_wb_bank_signal_reset(None, -1) == -1
    assert L.fmx_wb_bank_set_iq_correction(None, -1, 0, None, 0.0) == -1
    assert L.fmx_wb_bank_iq_correction(None, 0, None) == -1


def test_code_object_metadata(tmp_path):
    ks = _kernels(tmp_path)
    pick = lambda pat: {k: v for k, v in ks.items() if re.search(pat, k)}  # noqa: E731
    main, hist = pick(r"7k_rbankILb[01]ELb[01]E"), pick(r"12k_rbank_histI[sh]E")
    assert (len(main), len(hist)) == (4, 2), (sorted(main), sorted(hist))
    assert len(pick(r"k_rbank")) == 6
    for name, f in {**main, **hist}.items():
        print(name, f)
        assert f.get("private_segment_fixed_size", 0) == 0, (name, f)
        assert f.get("vgpr_spill_count", 0) == 0 and f.get("sgpr_spill_count", 0) == 0, (name, f)
        assert f.get("agpr_count", 0) == 0, (name, f)
    for name, f in main.items():
        s16 = "k_rbankILb1E" in name  # the first template argument
        assert f.get("vgpr_count", 0) <= (112 if s16 else 104), (name, f)
        twin = pick(name.split("EE")[0].replace("7k_rbankI", "5k_wbrI") + "EE")
        assert len(twin) == 1, (name, sorted(twin))
        assert 512 // f["vgpr_count"] == 512 // next(iter(twin.values()))["vgpr_count"], (name, f, twin)
    # what the sibling tests count is what it was, and the new names match none of their patterns
    assert len(pick(r"\d+k_wbb")) == 13 and len(pick(r"\d+k_wbr")) == 6 and len(pick(r"k_bank_iqc")) == 8
    for pat in (r"\d+k_wbb", r"\d+k_wbr", r"k_bank_iqc", r"\d+k_wbb.*iqc", r"\d+k_wbr.*iqc", r"8k_wb_iqcI", r"13k_wb_scan_iqcI"):
        assert not [k for k in {**main, **hist} if re.search(pat, k)], pat
