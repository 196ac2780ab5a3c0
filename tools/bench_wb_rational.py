#!/usr/bin/env python3
"""Times fmx_wb_process on rational-rate objects (fmx_wb_create_rational,
kernels k_wbr + k_wbr_hist) beside k_wb's band case, in
one run with the cases interleaved call by call, so that clock and thermal
state are shared.  The clock is the host's around work that ends in fmx_sync
(tools/bench_channelizer.py says why): each call alone on an idle stream, and
trains of calls back to back.

Cases:
  hackrf_20MSps_205ch   u8, 250 / 3, 205 channels across the capture, 4092 outputs per call
  hackrf_20MSps_205ch_s16  the same as int16: one tile per workgroup (DESIGN.md section 23's LDS table)
  rtl_2.048MSps_5ch     u8, 128 / 15, 5 channels, 4095 outputs per call
  band_24MSps_205ch_u8  u8, D = 100 through fmx_wb_create (k_wb), 205 channels, 4096 outputs per call

A call of n outputs is n / 240 000 s of signal (4092: 17.05 ms).  Writes one
JSON document (default profiles/wb_rational.json) with each case's times and
the rational cases' ratio to k_wb's band per output; exits non-zero when a
case is not faster than real time.  Needs a GPU."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fmtuner-sdr_amd"))

DSP = 240_000
TRAINS = 5


class Case:
    def __init__(self, fmx, torch, name, wide_rate, channels, n_out, rational, s16=False):
        self.name, self.wide_rate, self.channels, self.n_out, self.rational = name, wide_rate, channels, n_out, rational
        self.s16 = s16
        wcfg = fmx.make_wb_config(wide_rate, DSP, fmx.FMX_WB_S16 if s16 else fmx.FMX_WB_U8, 28, 4096)
        self.P, self.Q, self.taps = fmx.wb_ratio(wcfg)
        assert n_out % self.Q == 0 and (rational or self.Q == 1)
        # 100 kHz spacing, less where the capture is narrower than the channels' span (20 MS/s: 97 087 Hz)
        step = min(100_000, wide_rate // (channels + 1))
        freqs = [int((k - (channels - 1) / 2) * step) for k in range(channels)]
        assert max(abs(f) for f in freqs) <= wide_rate // 2
        self.h = fmx.Handle(fmx.make_config(iq_rate=DSP, dsp_rate=DSP), channels)
        self.wb = fmx.Wideband(self.h, wcfg, freqs, rational=rational)
        self.n_in = n_out // self.Q * self.P
        g = torch.Generator(device="cpu").manual_seed(1)
        if s16:
            self.raw = torch.randint(-32768, 32768, (2 * self.n_in,), generator=g, dtype=torch.int32).to(torch.int16).to("cuda")
        else:
            self.raw = torch.randint(0, 256, (2 * self.n_in,), generator=g, dtype=torch.int32).to(torch.uint8).to("cuda")
        self.out = torch.zeros((channels, 2 * n_out), dtype=torch.float32, device="cuda")
        self.ms, self.trains = [], []

    def call(self):
        self.wb.process(self.raw.data_ptr(), self.n_out, self.out.data_ptr(), self.n_out)

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
        signal_ms = self.n_out / DSP * 1e3
        train = float(np.median(tr))
        return dict(case=self.name, format="s16" if self.s16 else "u8", kernel="k_wbr" if self.rational and self.Q > 1 else "k_wb",
                    wide_rate=self.wide_rate, P=self.P, Q=self.Q, taps_per_phase_row=self.taps, channels=self.channels,
                    n_out=self.n_out, wide_samples_per_call=self.n_in, warmup=warmup, calls=calls,
                    ms_per_call_synchronised=dict(median=float(np.median(ms)), min=float(ms[0]), max=float(ms[-1]),
                                                  p10=float(ms[len(ms) // 10]), p90=float(ms[(9 * len(ms)) // 10])),
                    ms_per_call_back_to_back=dict(median=train, min=float(tr[0]), max=float(tr[-1]), trains=len(tr)),
                    signal_ms=signal_ms, times_real_time=signal_ms / train,
                    times_real_time_synchronised=signal_ms / float(np.median(ms)),
                    us_per_output_and_channel=train * 1e3 / (self.n_out * self.channels))

    def close(self):
        self.wb.close()
        self.h.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wb_rational.json"))
    a = ap.parse_args()
    if a.calls < 50:
        ap.error("--calls must be at least 50")
    import torch
    import fmx
    if not torch.cuda.is_available():
        sys.exit("bench_wb_rational: no GPU")
    cases = [Case(fmx, torch, "hackrf_20MSps_205ch", 20_000_000, 205, 4092, True),
             Case(fmx, torch, "rtl_2.048MSps_5ch", 2_048_000, 5, 4095, True),
             Case(fmx, torch, "band_24MSps_205ch_u8", 24_000_000, 205, 4096, False),
             Case(fmx, torch, "hackrf_20MSps_205ch_s16", 20_000_000, 205, 4092, True, s16=True)]
    torch.cuda.synchronize()
    for _ in range(a.warmup):
        for c in cases:
            c.call()
    for c in cases:
        c.h.sync()
    for _ in range(a.calls):  # interleaved call by call
        for c in cases:
            c.timed_call()
    for _ in range(TRAINS):   # and train by train
        for c in cases:
            c.timed_train(a.calls // TRAINS)
    res = [c.result(torch, a.warmup, a.calls) for c in cases]
    for c in cases:
        c.close()
    band = res[2]["us_per_output_and_channel"]
    for r in res[:2] + res[3:]:
        r["per_output_time_relative_to_k_wb_band"] = r["us_per_output_and_channel"] / band
    doc = dict(tool="tools/bench_wb_rational.py", library=fmx.build_info(), device=torch.cuda.get_device_name(0), cases=res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))
    slow = [r["case"] for r in res if r["times_real_time"] <= 1.0]
    if slow:
        sys.exit("bench_wb_rational: slower than real time: " + ", ".join(slow))


if __name__ == "__main__":
    main()
