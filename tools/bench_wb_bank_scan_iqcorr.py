#!/usr/bin/env python3
"""Times the bank scan's DC / IQ-imbalance correction per capture (DESIGN.md
section 29) against the uncorrected bank scan and against what a user with
several impaired front ends did without it, in one process, on one handle --

  OFF      one fmx_wb_bank_scan object, every capture in FMX_IQC_OFF: k_wbb_clip
           -> k_bscan -> k_bscan_level, three launches per read;
  AUTO     one fmx_wb_bank_scan object, every capture in FMX_IQC_AUTO:
           k_bank_iqc_sums -> k_bank_iqc_finish -> k_wbb_clip -> k_scan_bank_iqc
           -> k_bscan_level, five launches per read whatever S is;
  SINGLES  S fmx_wb_scan objects, each in FMX_IQC_AUTO on its capture's row:
           5 S launches per read.

The arms run interleaved: --warmup reads per arm, then --reps repetitions that
alternate a train of --train reads per arm, the opening arm rotating from one
repetition to the next; the host clock stops at fmx_sync;
per-read time = train time / reads; median and min-max over the repetitions.
Kernel times are not traced: these are host times of queued reads.

Case, 4096 outputs per read (17.07 ms of signal at 240 kHz): u8, D = 10
(2.4 MS/s), S = 16 captures of 23 points at 100 kHz (DESIGN.md section 28's
first case).

Writes one JSON document (default profiles/wb_bank_scan_iqcorr.json) and exits
non-zero when AUTO's median is not below SINGLES' of the same run, when a read
of AUTO is not faster than real time, or when AUTO's records or read-backs
differ from the single objects' in a bit (both arms made the same reads of the
same rows).  AUTO / OFF is reported, not gated.  Needs a GPU."""
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


def _stats(ms):
    import numpy as np
    ms = np.sort(np.array(ms))
    return dict(median=float(np.median(ms)), min=float(ms[0]), max=float(ms[-1]))


def _records(lev, points):
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
    off = fmx.WidebandBankScan(h, wcfg, [freqs] * S)
    auto = fmx.WidebandBankScan(h, wcfg, [freqs] * S)
    auto.set_iq_correction(fmx.FMX_IQC_AUTO)
    singles = [fmx.WidebandScan(h, fmx.make_wb_scan_config(Fs, DSP, code, TPP, n, start, step, Pn)) for _ in range(S)]
    for sc in singles:
        sc.set_iq_correction(fmx.FMX_IQC_AUTO)
    lev = {k: torch.zeros(S * Pn * 40, dtype=torch.uint8, device="cuda") for k in ("OFF", "AUTO", "SINGLES")}
    torch.cuda.synchronize()

    def read_off():
        off.process(raw.data_ptr(), n * D, n, lev["OFF"].data_ptr())

    def read_auto():
        auto.process(raw.data_ptr(), n * D, n, lev["AUTO"].data_ptr())

    def read_singles():
        for s in range(S):
            singles[s].process(raw.data_ptr() + s * row_bytes, n, lev["SINGLES"].data_ptr() + 40 * Pn * s)

    arms = {"OFF": read_off, "AUTO": read_auto, "SINGLES": read_singles}

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
    order = list(arms)
    for r in range(reps):  # the arm that opens a repetition rotates: no arm always follows the long SINGLES train
        for k in order[r % 3:] + order[:r % 3]:
            ms[k].append(run_train(arms[k], train))
    rec = {k: _records(lev[k], S * Pn) for k in arms}
    # AUTO and SINGLES made the same reads of the same rows in the same mode: records and read-backs agree bit for bit
    same_records = rec["AUTO"].tobytes() == rec["SINGLES"].tobytes()
    back_auto = [auto.iq_correction(s) for s in range(S)]
    back_singles = [sc.iq_correction() for sc in singles]
    same_back = back_auto == back_singles
    corrected_differs = rec["AUTO"]["dbfs"].tobytes() != rec["OFF"]["dbfs"].tobytes()
    off.close()
    auto.close()
    for sc in singles:
        sc.close()
    h.close()
    signal_ms = n / DSP * 1e3
    res = dict(case=name, format=fmt, D=D, wide_rate=Fs, taps=D * TPP, captures=S, points_per_capture=Pn,
               points=S * Pn, start_hz=start, step_hz=step, n_out=n, warmup=warmup, reps=reps, reads_per_train=train,
               signal_ms=signal_ms, launches_per_read=dict(OFF=3, AUTO=5, SINGLES=5 * S),
               kernel_times_traced=False,
               auto_records_equal_the_single_objects=bool(same_records),
               auto_read_backs_equal_the_single_objects=bool(same_back),
               auto_records_differ_from_off=bool(corrected_differs),
               read_back_capture_0=list(back_auto[0]))
    for k in arms:
        st = _stats(ms[k])
        res[k] = dict(ms_per_read=st, times_real_time=signal_ms / st["median"])
    res["AUTO_over_SINGLES"] = res["AUTO"]["ms_per_read"]["median"] / res["SINGLES"]["ms_per_read"]["median"]
    res["AUTO_over_OFF"] = res["AUTO"]["ms_per_read"]["median"] / res["OFF"]["ms_per_read"]["median"]
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--train", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wb_bank_scan_iqcorr.json"))
    a = ap.parse_args()
    if a.reps < 10:
        ap.error("--reps must be at least 10")
    import torch
    import fmx
    if not torch.cuda.is_available():
        sys.exit("bench_wb_bank_scan_iqcorr: no GPU")
    cases = [run_case(fmx, torch, "dongles_16x23pt_2.4MSps_u8", "u8", 10, 16, 23, -1_100_000, 100_000, a.warmup, a.reps,
                      a.train)]
    doc = dict(tool="tools/bench_wb_bank_scan_iqcorr.py", library=fmx.build_info(), device=torch.cuda.get_device_name(0),
               cases=cases)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))
    for c in cases:
        if not (c["auto_records_equal_the_single_objects"] and c["auto_read_backs_equal_the_single_objects"]):
            sys.exit(f"bench_wb_bank_scan_iqcorr: AUTO's records or read-backs differ from the single objects' in case {c['case']}")
        if c["AUTO_over_SINGLES"] >= 1.0:
            sys.exit(f"bench_wb_bank_scan_iqcorr: the corrected bank scan is not faster than one corrected scan object per "
                     f"capture in case {c['case']}")
        if c["AUTO"]["times_real_time"] <= 1.0:
            sys.exit(f"bench_wb_bank_scan_iqcorr: the corrected bank scan is slower than real time in case {c['case']}")


if __name__ == "__main__":
    main()
