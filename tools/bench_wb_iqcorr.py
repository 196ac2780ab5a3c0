#!/usr/bin/env python3
"""Times fmx_wb_process with the DC / IQ-imbalance correction in AUTO
(fmx_wb_set_iq_correction; kernels k_iqc_sums, k_iqc_finish and k_wb_iqc,
DESIGN.md section 24) beside the same object with the correction OFF (k_wb),
in one run with the two arms interleaved call by call, so that clock and
thermal state are shared.  The clock is the host's around work that ends in
fmx_sync (tools/bench_channelizer.py says why): each call alone on an idle
stream, and trains of calls back to back.

Case: 205 channels of a 24 MS/s u8 capture (D = 100), 4096 outputs per call:
409 600 raw samples, 17.07 ms of signal.  Writes one JSON document (default
profiles/wb_iqcorr.json) with both arms' times and AUTO's ratio to OFF (a
figure, not a gate); exits non-zero when an AUTO call is not faster than real
time.  Needs a GPU."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fmtuner-sdr_amd"))

DSP = 240_000
WIDE, D, CHANNELS, N_OUT = 24_000_000, 100, 205, 4096
TRAINS = 5


class Arm:
    def __init__(self, fmx, torch, name, mode, raw):
        self.name, self.mode = name, mode
        wcfg = fmx.make_wb_config(WIDE, DSP, fmx.FMX_WB_U8, 28, N_OUT)
        freqs = [int((k - (CHANNELS - 1) / 2) * 100_000) for k in range(CHANNELS)]
        self.h = fmx.Handle(fmx.make_config(iq_rate=DSP, dsp_rate=DSP), CHANNELS)
        self.wb = fmx.Wideband(self.h, wcfg, freqs)
        if mode != fmx.FMX_IQC_OFF:
            self.wb.set_iq_correction(mode, None, 0.0)
        self.raw = raw
        self.out = torch.zeros((CHANNELS, 2 * N_OUT), dtype=torch.float32, device="cuda")
        self.ms, self.trains = [], []

    def call(self):
        self.wb.process(self.raw.data_ptr(), N_OUT, self.out.data_ptr(), N_OUT)

    def timed_call(self):
        self.h.sync()
        t0 = time.perf_counter()
        self.call()
        self.h.sync()
        self.ms.append((time.perf_counter() - t0) * 1e3)

    def timed_train(self, calls):
        self.h.sync()
        t0 = time.perf_counter()
        for _ in range(calls):
            self.call()
        self.h.sync()
        self.trains.append((time.perf_counter() - t0) * 1e3 / calls)

    def result(self, torch, warmup, calls):
        import numpy as np
        assert bool(torch.isfinite(self.out).all())
        ms, tr = np.sort(np.array(self.ms)), np.sort(np.array(self.trains))
        signal_ms = N_OUT / DSP * 1e3
        train = float(np.median(tr))
        return dict(arm=self.name, parameters=list(self.wb.iq_correction()), format="u8", wide_rate=WIDE, D=D,
                    channels=CHANNELS, n_out=N_OUT, wide_samples_per_call=N_OUT * D, warmup=warmup, calls=calls,
                    ms_per_call_synchronised=dict(median=float(np.median(ms)), min=float(ms[0]), max=float(ms[-1]),
                                                  p10=float(ms[len(ms) // 10]), p90=float(ms[(9 * len(ms)) // 10])),
                    ms_per_call_back_to_back=dict(median=train, min=float(tr[0]), max=float(tr[-1]), trains=len(tr)),
                    signal_ms=signal_ms, times_real_time=signal_ms / train,
                    times_real_time_synchronised=signal_ms / float(np.median(ms)))

    def close(self):
        self.wb.close()
        self.h.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wb_iqcorr.json"))
    a = ap.parse_args()
    if a.calls < 50:
        ap.error("--calls must be at least 50")
    import torch
    import fmx
    if not torch.cuda.is_available():
        sys.exit("bench_wb_iqcorr: no GPU")
    g = torch.Generator(device="cpu").manual_seed(1)
    raw = torch.randint(0, 256, (2 * N_OUT * D,), generator=g, dtype=torch.int32).to(torch.uint8).to("cuda")
    arms = [Arm(fmx, torch, "off", fmx.FMX_IQC_OFF, raw), Arm(fmx, torch, "auto", fmx.FMX_IQC_AUTO, raw)]
    torch.cuda.synchronize()
    for _ in range(a.warmup):
        for c in arms:
            c.call()
    for c in arms:
        c.h.sync()
    for _ in range(a.calls):  # interleaved call by call
        for c in arms:
            c.timed_call()
    for _ in range(TRAINS):   # and train by train
        for c in arms:
            c.timed_train(a.calls // TRAINS)
    res = [c.result(torch, a.warmup, a.calls) for c in arms]
    for c in arms:
        c.close()
    off, auto = res
    ratio = dict(back_to_back=auto["ms_per_call_back_to_back"]["median"] / off["ms_per_call_back_to_back"]["median"],
                 synchronised=auto["ms_per_call_synchronised"]["median"] / off["ms_per_call_synchronised"]["median"])
    doc = dict(tool="tools/bench_wb_iqcorr.py", library=fmx.build_info(), device=torch.cuda.get_device_name(0), arms=res,
               auto_over_off=ratio)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))
    if auto["times_real_time"] <= 1.0:
        sys.exit("bench_wb_iqcorr: an AUTO call is slower than real time")


if __name__ == "__main__":
    main()
