#!/usr/bin/env python3
"""Times fmx_wb_scan_process (the band scan, kernels k_wb_scan_clip + k_wb_scan
+ k_wb_scan_level) against the only other route to the same levels,
fmx_wb_process on one channel per scan point (before any reduction of its
rows), in one process: warm-up, then --reps repetitions that alternate a
train of --train scan calls and a train of channelizer calls, each train
ending in fmx_sync.  The calls run on the handle's own stream, which the ABI
does not hand out, so the clock is the host's around the synchronised train;
per-call time = train time / calls.  Median and spread over the repetitions.

Cases: the band of tools/bench_channelizer.py -- int16, D = 100 (24 MS/s), 28
taps per phase, 205 points at 100 kHz, 4096 outputs per call -- and a fine scan
of 820 points at 25 kHz.  A 4096-output block is 17.07 ms of signal.

The MFMA floor is bench_channelizer's: (point groups of 16) x (output tiles of
16) x (K steps of 32 taps) x 12 MFMAs, one per 16 cycles per SIMD.

Writes one JSON document (default profiles/wb_scan.json) and exits non-zero
when the scan's median is above the channelizer's on the same points, or a
case is not faster than real time.  Needs a GPU."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fmtuner-sdr_amd"))

DSP = 240_000
N_OUT = 4096
D, TPP = 100, 28
MFMA_CYCLES = 16  # v_mfma_f32_16x16x32_f16, back to back on one SIMD


def _stats(ms):
    import numpy as np
    ms = np.sort(np.array(ms))
    return dict(median=float(np.median(ms)), min=float(ms[0]), max=float(ms[-1]), p10=float(ms[len(ms) // 10]),
                p90=float(ms[(9 * len(ms)) // 10]))


def run_case(fmx, torch, name, points, step, warmup, reps, train):
    Fs = D * DSP
    start = -int((points - 1) * step / 2)
    scfg = fmx.make_wb_scan_config(Fs, DSP, fmx.FMX_WB_S16, TPP, N_OUT, start, step, points)
    freqs = fmx.wb_scan_points(scfg)
    h = fmx.Handle(fmx.make_config(iq_rate=DSP, dsp_rate=DSP), points)
    sc = fmx.WidebandScan(h, scfg)
    wb = fmx.Wideband(h, scfg.wb, freqs)
    dev = torch.device("cuda")
    g = torch.Generator(device="cpu").manual_seed(1)
    raw = torch.randint(-32768, 32768, (2 * N_OUT * D,), generator=g, dtype=torch.int32).to(torch.int16).to(dev)
    rows = torch.zeros((points, 2 * N_OUT), dtype=torch.float32, device=dev)
    lev = torch.zeros((points, 5), dtype=torch.float64, device=dev)  # 40-byte records
    torch.cuda.synchronize()
    arms = {"scan": lambda: sc.process(raw.data_ptr(), N_OUT, lev.data_ptr()),
            "channelizer": lambda: wb.process(raw.data_ptr(), N_OUT, rows.data_ptr(), N_OUT)}
    for f in arms.values():
        for _ in range(warmup):
            f()
    h.sync()
    ms = {k: [] for k in arms}
    for _ in range(reps):
        for k, f in arms.items():
            h.sync()
            t0 = time.perf_counter()
            for _ in range(train):
                f()
            h.sync()
            ms[k].append((time.perf_counter() - t0) * 1e3 / train)
    assert bool(torch.isfinite(rows).all()) and bool(torch.isfinite(lev[:, 1:]).all())
    sc.close()
    wb.close()
    h.close()
    props = torch.cuda.get_device_properties(0)
    cus, mhz = props.multi_processor_count, props.clock_rate / 1e3 if hasattr(props, "clock_rate") else 2400.0
    L = D * TPP
    signal_ms = N_OUT / DSP * 1e3
    floor = {"scan": (N_OUT - TPP + 15) // 16, "channelizer": N_OUT // 16}
    res = dict(case=name, format="s16", D=D, wide_rate=Fs, taps=L, points=points, step_hz=step, n_out=N_OUT,
               warmup=warmup, reps=reps, calls_per_train=train, signal_ms=signal_ms, compute_units=cus, clock_mhz=mhz)
    for k in arms:
        st = _stats(ms[k])
        mfma = ((points + 15) // 16) * floor[k] * ((L + 31) // 32) * 12
        floor_ms = mfma * MFMA_CYCLES / (cus * 4) / (mhz * 1e3)
        res[k] = dict(ms_per_call=st, times_real_time=signal_ms / st["median"], mfma_issued=mfma,
                      mfma_floor_ms=floor_ms, fraction_of_mfma_floor=floor_ms / st["median"])
    res["scan_over_channelizer"] = res["scan"]["ms_per_call"]["median"] / res["channelizer"]["ms_per_call"]["median"]
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--train", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wb_scan.json"))
    a = ap.parse_args()
    if a.reps < 10:
        ap.error("--reps must be at least 10")
    import torch
    import fmx
    if not torch.cuda.is_available():
        sys.exit("bench_scan: no GPU")
    cases = [run_case(fmx, torch, "band_24MSps_205pt_100kHz", 205, 100_000, a.warmup, a.reps, a.train),
             run_case(fmx, torch, "fine_24MSps_820pt_25kHz", 820, 25_000, a.warmup, a.reps, a.train)]
    doc = dict(tool="tools/bench_scan.py", library=fmx.build_info(), device=torch.cuda.get_device_name(0), cases=cases)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))
    bad = [c["case"] for c in cases if c["scan_over_channelizer"] > 1.0]
    slow = [c["case"] for c in cases if c["scan"]["times_real_time"] <= 1.0]
    if bad:
        sys.exit(f"bench_scan: the scan is slower than the channelizer on the same points: {bad}")
    if slow:
        sys.exit(f"bench_scan: slower than real time: {slow}")


if __name__ == "__main__":
    main()
