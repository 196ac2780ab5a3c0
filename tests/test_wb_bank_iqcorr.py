"""The capture bank's DC-offset and IQ-imbalance correction on the CPU
(fmx_wb_bank_set_iq_correction, fmx_wb_bank_iq_correction; DESIGN.md section
26; the GPU side is tests/test_gpu_wb_bank_iqcorr.py):

  1. header and binding carry the two names; the ABI version is still 13; the
     two WidebandBank methods exist;
  2. the calls refuse a NULL object without touching a device;
  3. the code object's metadata of the new kernels."""
import ctypes as C
import os
import re
import subprocess

from test_resources import LLVM, _kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fmx_wb_bank_set_iq_correction", "fmx_wb_bank_iq_correction")


def test_names_and_abi_version(fmx):
    with open(os.path.join(ROOT, "include", "fmx.h")) as fh:
        header = fh.read()
    L = fmx.lib()
    for name in NAMES:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert getattr(L, name).argtypes is not None, name
    assert re.search(r"^#define FMX_ABI_VERSION 13$", header, re.M)
    assert callable(fmx.WidebandBank.set_iq_correction) and callable(fmx.WidebandBank.iq_correction)


def test_null_object_calls_need_no_gpu(fmx):
    L = fmx.lib()
    p = fmx.IqCorrection(0.0, 0.0, 1.0, 0.0)
    assert L.fmx_wb_bank_set_iq_correction(None, -1, fmx.FMX_IQC_FIXED, C.byref(p), 0.0) == -1
    assert L.fmx_wb_bank_set_iq_correction(None, 0, fmx.FMX_IQC_AUTO, None, 0.5) == -1
    assert L.fmx_wb_bank_iq_correction(None, 0, C.byref(p)) == -1


def test_code_object_metadata(tmp_path):
    """k_bank_iqc (int16 / u8 x D even / odd), the estimator k_bank_iqc_sums
    (u8, int16), k_bank_iqc_finish and k_bank_iqc_set: no scratch, no spills,
    no AGPRs; every k_bank_iqc instance in the occupancy class of its k_wbb
    twin (512 // VGPRs equal, <= 128); the estimator has k_iqc_sums' static LDS
    (160 bytes) and no more.  No new name matches the patterns by which
    tests/test_wb_bank.py and tests/test_wb_rational.py count their kernels.
    Built: k_bank_iqc 120 (int16) / 112 (u8) against k_wbb's 112 / 104 and
    k_wb_iqc's 120 / 112; k_bank_iqc_sums 56 (int16) / 62 (u8), k_iqc_sums' own
    figures; k_bank_iqc_finish 56, k_bank_iqc_set 28."""
    ks = _kernels(tmp_path)
    pick = lambda pat: {k: v for k, v in ks.items() if re.search(pat, k)}  # noqa: E731
    main, sums = pick(r"10k_bank_iqcILb[01]ELb[01]E"), pick(r"15k_bank_iqc_sumsI[sh]E")
    one = pick(r"(17k_bank_iqc_finishE|14k_bank_iqc_setE)")
    assert (len(main), len(sums), len(one)) == (4, 2, 2), (sorted(main), sorted(sums), sorted(one))
    assert len(pick(r"k_bank_iqc")) == 8
    assert not pick(r"\d+k_wbb.*iqc") and not pick(r"\d+k_wbr.*iqc")
    # .agpr_count opens a kernel's entry in the notes; its .name follows in the same entry
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", str(tmp_path / "k.co")], check=True,
                           capture_output=True, text=True).stdout
    agprs = {m.group(2): int(m.group(1))
             for m in re.finditer(r"- \.agpr_count:\s+(\d+)\n(?:(?!\s+- \.agpr_count).*\n)*?\s+\.name:\s+(\S+)", notes)}
    for name, f in {**main, **sums, **one}.items():
        print(name, f, "agprs", agprs.get(name))
        assert agprs.get(name) == 0, (name, agprs.get(name))
        assert f.get("private_segment_fixed_size", 0) == 0, (name, f)
        assert f.get("vgpr_spill_count", 0) == 0 and f.get("sgpr_spill_count", 0) == 0, (name, f)
        assert f.get("agpr_count", 0) == 0, (name, f)
    for name, f in main.items():
        twin = re.sub(r"PK11FmxIqcBlockPKNS_10WbbIqcModeEPKf$", "", name.replace("10k_bank_iqcI", "5k_wbbI"))
        assert twin in ks and twin != name, (name, twin)
        assert 512 // f["vgpr_count"] == 512 // ks[twin]["vgpr_count"], (name, f, ks[twin])
        assert f["vgpr_count"] <= 128, (name, f)
    for name, f in sums.items():
        assert f.get("group_segment_fixed_size", 0) <= 160, (name, f)
