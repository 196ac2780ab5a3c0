"""DC-offset and IQ-imbalance correction per capture of the band scan over a
capture bank (fmx_wb_bank_scan_set_iq_correction,
fmx_wb_bank_scan_iq_correction) without a GPU; the GPU
side is tests/test_gpu_wb_bank_scan_iqcorr.py:

  1. header, ABI history and binding carry the two symbols; both calls with a
     NULL object return FMX_E_INVALID without touching a device;
  2. the code object's metadata: k_scan_bank_iqc's four instances have no
     scratch, no spills, no AGPRs, no static LDS and at most 170 VGPRs
     (k_bscan's bar: three waves per SIMD is all two workgroups of LDS allow),
     and what the sibling tests count is what it was;
  3. the condition the GPU ghost test rests on, on the float64 reference
     alone: three captures behind three different front ends, each scanned
     over 13 points; uncorrected, fmx_scan_peaks finds at least one ghost per
     capture, corrected with the estimate of the read's own samples exactly
     the stations."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import wb_bank_scan_iq_ref as BQ
import wb_iq_ref as Q
import wb_ref as R
import wb_scan_ref as S
from test_resources import _kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fmx_wb_bank_scan_set_iq_correction", "fmx_wb_bank_scan_iq_correction")


def test_header_and_binding(fmx):
    with open(os.path.join(ROOT, "include", "fmx.h")) as fh:
        header = fh.read()
    L = fmx.lib()
    for name in NAMES:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert getattr(L, name).argtypes is not None, name
        assert name in header.split("#define FMX_ABI_VERSION")[0], name  # the ABI history names it
    assert re.search(r"^#define FMX_ABI_VERSION 13$", header, re.M)
    sig = inspect.signature(fmx.WidebandBankScan.set_iq_correction).parameters
    assert list(sig) == ["self", "mode", "fixed", "alpha", "capture"]
    assert (sig["fixed"].default, sig["alpha"].default, sig["capture"].default) == (None, 0.0, -1)
    assert list(inspect.signature(fmx.WidebandBankScan.iq_correction).parameters) == ["self", "capture"]
    # mirrors WidebandBank
    assert list(sig) == list(inspect.signature(fmx.WidebandBank.set_iq_correction).parameters)


def test_null_object_calls_need_no_gpu(fmx):
    L = fmx.lib()
    p = fmx.IqCorrection(0.0, 0.0, 1.0, 0.0)
    assert L.fmx_wb_bank_scan_set_iq_correction(None, -1, fmx.FMX_IQC_FIXED, C.byref(p), 0.0) == -1
    assert L.fmx_wb_bank_scan_set_iq_correction(None, 0, fmx.FMX_IQC_AUTO, None, 0.5) == -1
    assert L.fmx_wb_bank_scan_iq_correction(None, 0, C.byref(p)) == -1


def test_code_object_metadata(tmp_path):
    """Built: k_scan_bank_iqc 144 VGPRs (int16) / 128 (u8) against k_bscan's
    142 / 126 and k_wb_scan_iqc's 144 / 128: 512 // VGPRs is 3 / 4 for both,
    so the corrected read runs in k_bscan's occupancy class."""
    ks = _kernels(tmp_path)
    pick = lambda pat: {k: v for k, v in ks.items() if re.search(pat, k)}  # noqa: E731
    main = pick(r"15k_scan_bank_iqcILb[01]ELb[01]E")
    assert len(main) == 4 and len(pick(r"k_scan_bank_iqc")) == 4, sorted(pick(r"k_scan_bank_iqc"))
    plain = pick(r"7k_bscanILb[01]ELb[01]E")
    for name, f in main.items():
        twin = name.replace("15k_scan_bank_iqcI", "7k_bscanI").split("PK11FmxIqcBlock")[0]
        print(name, f, "waves by VGPRs", 512 // f["vgpr_count"], "k_bscan's", 512 // plain[twin]["vgpr_count"])
        assert "BscanArgs" in name and "FmxIqcBlock" in name and "WbbIqcMode" in name, name
        assert f.get("private_segment_fixed_size", 0) == 0, (name, f)
        assert f.get("vgpr_spill_count", 0) == 0 and f.get("sgpr_spill_count", 0) == 0, (name, f)
        assert f.get("agpr_count", 0) == 0, (name, f)
        assert f.get("group_segment_fixed_size", 0) == 0, (name, f)  # the LDS is dynamic
        assert 0 < f.get("vgpr_count", 0) <= 170, (name, f)
    # what the sibling tests count is what it was: the estimator and the set are the bank's, not new instances
    assert len(pick(r"k_bscan")) == 5 and len(pick(r"k_bank_iqc")) == 8 and len(pick(r"k_rbank")) == 6
    assert len(pick(r"\d+k_wbb")) == 13 and len(pick(r"\d+k_wbr")) == 6
    for pat in (r"k_bscan", r"k_bank_iqc", r"k_rbank", r"k_wb_scan", r"\d+k_wbb", r"\d+k_wbr"):
        assert not [k for k in main if re.search(pat, k)], pat


@pytest.mark.parametrize("fmt", [R.U8, R.S16])
def test_reference_scan_finds_ghosts_per_front_end(fmx, fmt):
    """D = 10, tpp 28, 13 points from -600 to +600 kHz, one read of 2048
    outputs, fmx_scan_peaks at -45 dBFS with spacing 1.  Capture 0 is
    impaired_capture; capture 1 (seed 25) one station of 0.4 at -500 kHz, Q
    gain 0.95, skew -3 degrees, DC (-0.012, +0.025); capture 2 (seed 26)
    stations 0.35 at +200 kHz and 0.2 at +500 kHz, Q gain 1.08, skew -5
    degrees, DC (+0.030, +0.010).  Uncorrected peaks {-300k, 0, +300k},
    {-500k, 0, +500k}, {-500k, +200k, +500k}; corrected with each capture's
    own estimate exactly the stations.  Both formats: the weakest counted
    ghost reads -41.3 dBFS, the highest corrected non-station point -55.9."""
    D, tpp, n = BQ.GHOST_D, BQ.GHOST_TPP, BQ.GHOST_N_OUT
    rows = BQ.ghost_rows(fmt)
    assert np.array_equal(BQ.impaired(fmt, **BQ.FRONT_ENDS[0]), rows[0])  # the parameterised form is impaired_capture's
    grid = S.points(BQ.GHOST_START, BQ.GHOST_STEP, BQ.GHOST_POINTS)
    freqs = [grid] * 3
    ps, _ = BQ.estimates(rows, fmt, D, n, [None] * 3, [1.0] * 3)
    off = BQ.scan_call(rows, fmt, D, tpp, Q.CAP_FS, freqs, n, [Q.IDENTITY] * 3)
    auto = BQ.scan_call(rows, fmt, D, tpp, Q.CAP_FS, freqs, n, ps)
    assert len(off) == len(auto) == 39
    weakest_ghost, highest_other = 0.0, -200.0
    for s in range(3):
        db_off = [r["dbfs"] for r in off[13 * s:13 * s + 13]]
        db_auto = [r["dbfs"] for r in auto[13 * s:13 * s + 13]]
        peaks = lambda db: [grid[i] for i in fmx.scan_peaks(db, BQ.GHOST_THRESHOLD_DBFS, BQ.GHOST_SPACING)]  # noqa: E731
        print(f"fmt {fmt} capture {s} off ", np.round(db_off, 1), peaks(db_off))
        print(f"fmt {fmt} capture {s} auto", np.round(db_auto, 1), peaks(db_auto), ps[s])
        assert peaks(db_off) == BQ.GHOSTS[s], (s, peaks(db_off))
        assert len(set(peaks(db_off)) - set(BQ.STATIONS[s])) >= 1, s  # at least one ghost
        assert peaks(db_auto) == BQ.STATIONS[s], (s, peaks(db_auto))
        weakest_ghost = min([weakest_ghost] + [db_off[grid.index(f)] for f in BQ.GHOSTS[s] if f not in BQ.STATIONS[s]])
        highest_other = max([highest_other] + [d for f, d in zip(grid, db_auto)
                                               if all(abs(f - st) > BQ.GHOST_STEP for st in BQ.STATIONS[s])])
    print(f"fmt {fmt}: weakest counted ghost {weakest_ghost:.1f} dBFS, highest corrected point away from a station "
          f"{highest_other:.1f} dBFS")
    assert weakest_ghost > BQ.GHOST_THRESHOLD_DBFS + 2.0 and highest_other < BQ.GHOST_THRESHOLD_DBFS - 5.0
    assert len({p for p in ps}) == 3  # three front ends, three estimates
