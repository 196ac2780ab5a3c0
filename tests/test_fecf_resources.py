"""Register and LDS budget of k_fecf, the fast front end on complex-float rows
(fmx_wb_process_block) -- CPU: reads the gfx950 code
object's metadata out of fmtuner-sdr_amd/libfmx.so, as tests/test_resources.py
does.

k_fecf holds a subset of k_fe8's LDS regions (the four IQ images, yb, the IQ
FIR history, the shared words: no decimator window, no tap windows, no landing
area), so its LDS at launch is at most that of k_fe8<10, 28, false>, the front
end of a 2.4 MS/s process_block step, with no margin.  A kernel's static LDS
is in the code object; the dynamic part a launch adds is not (k_fe8's LDS is
all dynamic, its metadata says 0), so the library reports what its launchers
pass (fmx_diag_lds_bytes) and the sums are compared."""
import test_resources as TR


def _one(ks, pat):
    hits = TR._find(ks, pat)
    assert len(hits) == 1, sorted(hits)
    return next(iter(hits.items()))


def test_fecf_registers_scratch_and_lds(tmp_path, fmx):
    ks = TR._kernels(tmp_path)
    name, f = _one(ks, r"6k_fecfENS_6FeArgs")
    assert f.get("vgpr_count", 0) + f.get("agpr_count", 0) <= 256, (name, f)
    assert f.get("vgpr_spill_count", 0) == 0 and f.get("sgpr_spill_count", 0) == 0, (name, f)
    assert f.get("private_segment_fixed_size", 0) == 0, (name, f)
    name8, f8 = _one(ks, r"k_fe8ILi10ELi28ELb0E")
    L = fmx.lib()
    dyn, dyn8 = L.fmx_diag_lds_bytes(1), L.fmx_diag_lds_bytes(0)
    assert dyn >= 0 and dyn8 > 0 and L.fmx_diag_lds_bytes(2) < 0
    lds = f.get("group_segment_fixed_size", 0) + dyn
    lds8 = f8.get("group_segment_fixed_size", 0) + dyn8
    print("k_fecf", f, "dynamic", dyn, "| k_fe8<10,28,false>", f8, "dynamic", dyn8)
    assert 0 < lds <= lds8, (lds, lds8)
