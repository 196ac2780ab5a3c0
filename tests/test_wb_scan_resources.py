"""Register and scratch budget of the band scan's kernels (CPU: reads the
gfx950 code object's metadata out of fmtuner-sdr_amd/libfmx.so, as
tests/test_resources.py does).  k_wb_scan holds the accumulators of four
tiles per wave (64 VGPRs) beside the weight and sample fragments: at most 256
VGPRs and no scratch, so that the two workgroups per CU its 80 KB of dynamic
LDS allow are resident."""
from test_resources import _find, _kernels


def test_scan_kernel_budget(tmp_path):
    ks = _kernels(tmp_path)
    hits = _find(ks, r"9k_wb_scanILb[01]ELb[01]EEEvNS_10WbScanArgs")
    assert len(hits) == 4, sorted(hits)  # int16 / u8 x even / odd D
    for name, f in hits.items():
        assert f.get("vgpr_count", 0) + f.get("agpr_count", 0) <= 256, (name, f)
        assert f.get("vgpr_spill_count", 0) == 0 and f.get("sgpr_spill_count", 0) == 0, (name, f)
        assert f.get("private_segment_fixed_size", 0) == 0 and f.get("group_segment_fixed_size", 0) == 0, (name, f)
    for pat in (r"14k_wb_scan_clipI[sh]EEvNS_10WbScanArgs", r"15k_wb_scan_levelENS_10WbScanArgs"):
        for name, f in _find(ks, pat).items():
            assert f.get("vgpr_count", 0) <= 64 and f.get("private_segment_fixed_size", 0) == 0, (name, f)
