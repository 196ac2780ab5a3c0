#!/usr/bin/env python3
"""Times fmx_wb_process alone (the wideband channelizer, kernels k_wb +
k_wb_hist): warm-up calls, then --calls timed ones; median and spread.  The
calls run on the handle's own stream, which the ABI does not hand out, so no
HIP event can be recorded on it from outside: the clock is the host's around
work that ends in fmx_sync -- each call alone on an idle stream (an upper
bound: launch and completion latency included), and a train of calls back to
back (the per-call time a streaming receiver sees).

Cases: the band -- int16, D = 100 (24 MS/s), 28 taps per phase, 205 channels
at 100 kHz spacing, 4096 outputs per call -- and the same call at D = 10 with
5 channels.  A 4096-sample block is 4096 / 240 000 s = 17.07 ms of signal.

The MFMA floor is the time the MFMAs the kernel issues would take if every
SIMD issued one v_mfma_f32_16x16x32_f16 every 16 cycles: (channel groups of
16) x (output tiles of 16) x (K steps of 32 taps) x 12 MFMAs (s16: four
chains x hi*hi, hi*lo, lo*hi) over CUs x 4 SIMDs at the device's clock.

Writes one JSON document (default profiles/wb_channelizer.json) and exits
non-zero when the band case is not faster than real time.  Needs a GPU."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fmtuner-sdr_amd"))

DSP = 240_000
N_OUT = 4096
MFMA_CYCLES = 16  # v_mfma_f32_16x16x32_f16, back to back on one SIMD


def run_case(fmx, torch, name, D, channels, warmup, calls):
    import numpy as np
    Fs = D * DSP
    freqs = [int((k - (channels - 1) / 2) * 100_000) for k in range(channels)]
    assert max(abs(f) for f in freqs) <= Fs // 2
    h = fmx.Handle(fmx.make_config(iq_rate=DSP, dsp_rate=DSP), channels)
    wb = fmx.Wideband(h, fmx.make_wb_config(Fs, DSP, fmx.FMX_WB_S16, 28, N_OUT), freqs)
    dev = torch.device("cuda")
    g = torch.Generator(device="cpu").manual_seed(1)
    raw = torch.randint(-32768, 32768, (2 * N_OUT * D,), generator=g, dtype=torch.int32).to(torch.int16).to(dev)
    out = torch.zeros((channels, 2 * N_OUT), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    for _ in range(warmup):
        wb.process(raw.data_ptr(), N_OUT, out.data_ptr(), N_OUT)
    h.sync()
    # the handle's stage stream is not torch's: time with host clocks around a
    # synchronised call and, for the device time, with the stream idle before
    # each call -- a call is two kernels back to back, so the synchronised wall
    # time bounds it from above (launch + completion latency included)
    import time
    ms = []
    for _ in range(calls):
        h.sync()
        t0 = time.perf_counter()
        wb.process(raw.data_ptr(), N_OUT, out.data_ptr(), N_OUT)
        h.sync()
        ms.append((time.perf_counter() - t0) * 1e3)
    # a back-to-back train: per-call time with the launch latency overlapped
    h.sync()
    t0 = time.perf_counter()
    for _ in range(calls):
        wb.process(raw.data_ptr(), N_OUT, out.data_ptr(), N_OUT)
    h.sync()
    train = (time.perf_counter() - t0) * 1e3 / calls
    assert bool(torch.isfinite(out).all())
    wb.close()
    h.close()
    ms = np.sort(np.array(ms))
    props = torch.cuda.get_device_properties(0)
    cus, mhz = props.multi_processor_count, props.clock_rate / 1e3 if hasattr(props, "clock_rate") else 2400.0
    L = D * 28
    mfma = ((channels + 15) // 16) * (N_OUT // 16) * ((L + 31) // 32) * 12
    floor_ms = mfma * MFMA_CYCLES / (cus * 4) / (mhz * 1e3)
    signal_ms = N_OUT / DSP * 1e3
    return dict(case=name, format="s16", D=D, wide_rate=Fs, taps=L, channels=channels, n_out=N_OUT,
                warmup=warmup, calls=calls,
                ms_per_call_synchronised=dict(median=float(np.median(ms)), min=float(ms[0]), max=float(ms[-1]),
                                              p10=float(ms[len(ms) // 10]), p90=float(ms[(9 * len(ms)) // 10])),
                ms_per_call_back_to_back=train,
                signal_ms=signal_ms, times_real_time=signal_ms / train,
                times_real_time_synchronised=signal_ms / float(np.median(ms)),
                mfma_issued=mfma, mfma_floor_ms=floor_ms, fraction_of_mfma_floor=floor_ms / train,
                compute_units=cus, clock_mhz=mhz)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wb_channelizer.json"))
    a = ap.parse_args()
    if a.calls < 50:
        ap.error("--calls must be at least 50")
    import torch
    import fmx
    if not torch.cuda.is_available():
        sys.exit("bench_channelizer: no GPU")
    cases = [run_case(fmx, torch, "band_24MSps_205ch", 100, 205, a.warmup, a.calls),
             run_case(fmx, torch, "slice_2.4MSps_5ch", 10, 5, a.warmup, a.calls)]
    doc = dict(tool="tools/bench_channelizer.py", library=fmx.build_info(), device=torch.cuda.get_device_name(0),
               cases=cases)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))
    if cases[0]["times_real_time"] <= 1.0:
        sys.exit("bench_channelizer: the band case is slower than real time")


if __name__ == "__main__":
    main()
