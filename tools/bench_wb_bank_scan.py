#!/usr/bin/env python3
"""Times the band scan over a capture bank against what a user with several
captures does without it, in one process, on one handle --

  A  one fmx_wb_bank_scan object of S captures: one fmx_wb_bank_scan_process
     per read (k_wbb_clip -> k_bscan -> k_bscan_level, three launches whatever
     S is);
  B  S fmx_wb_scan objects: S fmx_wb_scan_process calls per read (3 S
     launches), each on its capture's row.

Both arms run interleaved: --warmup reads per arm, then --reps repetitions that
alternate a train of --train reads per arm; the host clock stops at fmx_sync;
per-read time = train time / reads; median and min-max over the repetitions.

Cases, 4096 outputs per read (17.07 ms of signal at 240 kHz):
  dongles  u8, D = 10 (2.4 MS/s), S = 16 captures of 23 points at 100 kHz;
  bands    int16, D = 100 (24 MS/s), S = 4 captures of 205 points at 100 kHz
           (DESIGN.md section 19's band case, times four).

Writes one JSON document (default profiles/wb_bank_scan.json) and exits
non-zero when, in either case, A's median is above B's (A launches strictly
less for the same arithmetic) or a read of A is not faster than real time.  The
ratio is reported, not gated.  Needs a GPU."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fmtuner-sdr_amd"))

DSP = 240_000
N_OUT = 4096
TPP = 28
WB_LDS_MAX, WB_SCAN_NT = 80 * 1024, 4  # fmx_wb_core.inc


def _stats(ms):
    import numpy as np
    ms = np.sort(np.array(ms))
    return dict(median=float(np.median(ms)), min=float(ms[0]), max=float(ms[-1]))


def _tiling(D, s16, n_out):
    """k_bscan's tiles per workgroup, workgroups per entry and dynamic LDS bytes (wb_scan_tiles and its kin)."""
    Lp = (D * TPP + 31) & ~31
    fit = ((WB_LDS_MAX // (8 if s16 else 4) - 8 - Lp) // D + 1) // 16
    nt = min(fit, WB_SCAN_NT)
    window = (16 * nt - 1) * D + Lp
    return dict(tiles_per_workgroup=nt, workgroups_per_entry=(n_out - TPP + 16 * nt - 1) // (16 * nt),
                lds_bytes=((window + 7) & ~7) * (8 if s16 else 4))


def _check(torch, lev, points):
    import numpy as np
    rec = lev.cpu().numpy().view(np.dtype([("level120", "<f4"), ("smoothed", "<f4"), ("dbfs", "<f8"), ("cdb", "<f8"),
                                           ("hard", "<f8"), ("near", "<f8")]))
    assert rec.size == points and np.isfinite(rec["dbfs"]).all() and (rec["dbfs"] > -100.0).all()
    return rec


def run_case(fmx, torch, name, fmt, D, S, Pn, start, step, warmup, reps, train):
    Fs, n = D * DSP, N_OUT
    s16 = fmt == "s16"
    code = fmx.FMX_WB_S16 if s16 else fmx.FMX_WB_U8
    freqs = [start + i * step for i in range(Pn)]
    wcfg = fmx.make_wb_config(Fs, DSP, code, TPP, n)
    g = torch.Generator(device="cpu").manual_seed(1)
    if s16:
        raw = torch.randint(-32768, 32768, (S, 2 * n * D), generator=g, dtype=torch.int32).to(torch.int16).to("cuda")
    else:
        raw = torch.randint(0, 256, (S, 2 * n * D), generator=g, dtype=torch.int32).to(torch.uint8).to("cuda")
    row_bytes = raw.element_size() * 2 * n * D
    h = fmx.Handle(fmx.make_config(iq_rate=DSP, dsp_rate=DSP), 1)
    bank = fmx.WidebandBankScan(h, wcfg, [freqs] * S)
    singles = [fmx.WidebandScan(h, fmx.make_wb_scan_config(Fs, DSP, code, TPP, n, start, step, Pn)) for _ in range(S)]
    levA = torch.zeros(S * Pn * 40, dtype=torch.uint8, device="cuda")
    levB = torch.zeros(S * Pn * 40, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def read_a():
        bank.process(raw.data_ptr(), n * D, n, levA.data_ptr())

    def read_b():
        for s in range(S):
            singles[s].process(raw.data_ptr() + s * row_bytes, n, levB.data_ptr() + 40 * Pn * s)

    arms = {"A_bank_scan": read_a, "B_one_scan_object_per_capture": read_b}

    def run_train(fn, k):
        h.sync()
        t0 = time.perf_counter()
        for _ in range(k):
            fn()
        h.sync()
        return (time.perf_counter() - t0) * 1e3 / k

    for fn in arms.values():
        run_train(fn, warmup)
    ms = {k: [] for k in arms}
    for _ in range(reps):
        for k, fn in arms.items():
            ms[k].append(run_train(fn, train))
    a, b = _check(torch, levA, S * Pn), _check(torch, levB, S * Pn)
    # both arms made the same reads of the same rows: the records, smoothed levels included, agree bit for bit
    same = a.tobytes() == b.tobytes()
    bank.close()
    for sc in singles:
        sc.close()
    h.close()
    signal_ms = n / DSP * 1e3
    res = dict(case=name, format=fmt, D=D, wide_rate=Fs, taps=D * TPP, captures=S, points_per_capture=Pn,
               points=S * Pn, start_hz=start, step_hz=step, n_out=n, warmup=warmup, reps=reps, reads_per_train=train,
               signal_ms=signal_ms, launches_per_read=dict(A_bank_scan=3, B_one_scan_object_per_capture=3 * S),
               k_bscan=dict(grid_y_entries=S * ((Pn + 63) // 64), **_tiling(D, s16, n)),
               records_equal_the_single_objects=bool(same))
    for k in arms:
        st = _stats(ms[k])
        res[k] = dict(ms_per_read=st, times_real_time=signal_ms / st["median"])
    ma, mb = res["A_bank_scan"]["ms_per_read"], res["B_one_scan_object_per_capture"]["ms_per_read"]
    res["A_over_B"] = ma["median"] / mb["median"]
    res["A_over_B_inside_the_arms_spread"] = bool(ma["min"] <= mb["max"] and mb["min"] <= ma["max"])
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--train", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wb_bank_scan.json"))
    a = ap.parse_args()
    if a.reps < 10:
        ap.error("--reps must be at least 10")
    import torch
    import fmx
    if not torch.cuda.is_available():
        sys.exit("bench_wb_bank_scan: no GPU")
    cases = [run_case(fmx, torch, "dongles_16x23pt_2.4MSps_u8", "u8", 10, 16, 23, -1_100_000, 100_000, a.warmup, a.reps,
                      a.train),
             run_case(fmx, torch, "bands_4x205pt_24MSps_s16", "s16", 100, 4, 205, -10_200_000, 100_000, a.warmup, a.reps,
                      a.train)]
    doc = dict(tool="tools/bench_wb_bank_scan.py", library=fmx.build_info(), device=torch.cuda.get_device_name(0),
               cases=cases)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))
    for c in cases:
        if not c["records_equal_the_single_objects"]:
            sys.exit(f"bench_wb_bank_scan: the arms' records differ in case {c['case']}")
        if c["A_over_B"] > 1.0:
            sys.exit(f"bench_wb_bank_scan: the bank scan is slower than one scan object per capture in case {c['case']}")
        if c["A_bank_scan"]["times_real_time"] <= 1.0:
            sys.exit(f"bench_wb_bank_scan: the bank scan is slower than real time in case {c['case']}")


if __name__ == "__main__":
    main()
