#!/usr/bin/env python3
"""Times fmx_wb_bank_process on a bank of fmx_wb_bank_create_rational (kernels
k_rbank and k_rbank_hist) beside what a user does
without it: one handle and one fmx_wb_create_rational object per capture
(k_wbr and k_wbr_hist, once per capture).  One run per case, the two arms
interleaved call by call and train by train, so that clock and thermal state
are shared; the clock is the host's around work that ends in fmx_sync of every
handle of the arm (tools/bench_wb_bank_iqcorr.py's scheme): each call alone on
idle streams, and trains of calls back to back.

Cases: sixteen u8 captures at 2.048 MS/s (128 / 15: RTL dongles at their stock
rate), five stations each, 4095 outputs per call -- 34 944 raw samples per
capture, 17.06 ms of signal; and four int16 captures at 20 MS/s (250 / 3) of
50 stations, 4095 outputs per call -- 341 250 raw samples per capture.
Writes one JSON document (default profiles/wb_bank_rational.json) with the
arms' times and the bank's ratio to the objects (a figure, not a gate); exits
non-zero when a bank call is not faster than real time or its rows differ
from the objects'.  Needs a GPU."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fmtuner-sdr_amd"))

DSP = 240_000
N_OUT = 4095
TRAINS = 5
CASES = [dict(name="sixteen_dongles_2048k", wide=2_048_000, fmt="u8", captures=16, channels=5, step=400_000),
         dict(name="four_hackrf_20M", wide=20_000_000, fmt="s16", captures=4, channels=50, step=200_000)]


class Arm:
    """call: what one call queues; handles: synchronised around it."""

    def __init__(self, name, handles, objects, call, out):
        self.name, self.handles, self.objects, self.call, self.out = name, handles, objects, call, out
        self.ms, self.trains = [], []

    def sync(self):
        for h in self.handles:
            h.sync()

    def timed_call(self):
        self.sync()
        t0 = time.perf_counter()
        self.call()
        self.sync()
        self.ms.append((time.perf_counter() - t0) * 1e3)

    def timed_train(self, calls):
        self.sync()
        t0 = time.perf_counter()
        for _ in range(calls):
            self.call()
        self.sync()
        self.trains.append((time.perf_counter() - t0) * 1e3 / calls)

    def result(self, torch, warmup, calls):
        import numpy as np
        assert bool(torch.isfinite(self.out).all())
        ms, tr = np.sort(np.array(self.ms)), np.sort(np.array(self.trains))
        signal_ms = N_OUT / DSP * 1e3
        train = float(np.median(tr))
        return dict(arm=self.name, warmup=warmup, calls=calls,
                    ms_per_call_synchronised=dict(median=float(np.median(ms)), min=float(ms[0]), max=float(ms[-1]),
                                                  p10=float(ms[len(ms) // 10]), p90=float(ms[(9 * len(ms)) // 10])),
                    ms_per_call_back_to_back=dict(median=train, min=float(tr[0]), max=float(tr[-1]), trains=len(tr)),
                    signal_ms=signal_ms, times_real_time=signal_ms / train,
                    times_real_time_synchronised=signal_ms / float(np.median(ms)))


def run_case(fmx, torch, k, warmup, calls):
    S, Cn = k["captures"], k["channels"]
    s16 = k["fmt"] == "s16"
    wcfg = fmx.make_wb_config(k["wide"], DSP, fmx.FMX_WB_S16 if s16 else fmx.FMX_WB_U8, 0, N_OUT)
    P, Q, _ = fmx.wb_ratio(wcfg)
    assert N_OUT % Q == 0
    n_in = N_OUT // Q * P
    g = torch.Generator(device="cpu").manual_seed(1)
    if s16:
        raw = torch.randint(-32768, 32768, (S, 2 * n_in), generator=g, dtype=torch.int32).to(torch.int16).to("cuda")
    else:
        raw = torch.randint(0, 256, (S, 2 * n_in), generator=g, dtype=torch.int32).to(torch.uint8).to("cuda")
    freqs = [-int((Cn - 1) * k["step"] / 2) + i * k["step"] for i in range(Cn)]
    new_out = lambda: torch.zeros((S * Cn, 2 * N_OUT), dtype=torch.float32, device="cuda")  # noqa: E731

    h = fmx.Handle(fmx.make_config(iq_rate=DSP, dsp_rate=DSP), S * Cn)
    bank = fmx.WidebandBank(h, wcfg, [freqs] * S, rational=True)
    bout = new_out()
    arm_b = Arm("bank", [h], [bank], lambda: bank.process(raw.data_ptr(), n_in, N_OUT, bout.data_ptr(), N_OUT), bout)

    hs = [fmx.Handle(fmx.make_config(iq_rate=DSP, dsp_rate=DSP), Cn) for _ in range(S)]
    wbs = [fmx.Wideband(hh, wcfg, freqs, rational=True) for hh in hs]
    sout = new_out()
    row, orow = raw.element_size() * 2 * n_in, 4 * Cn * 2 * N_OUT

    def singles():
        for s, wb in enumerate(wbs):
            wb.process(raw.data_ptr() + s * row, N_OUT, sout.data_ptr() + s * orow, N_OUT)

    arm_s = Arm("objects", hs, wbs, singles, sout)
    arms = [arm_b, arm_s]
    torch.cuda.synchronize()
    for _ in range(warmup):
        for c in arms:
            c.call()
    for c in arms:
        c.sync()
    for _ in range(calls):  # interleaved call by call
        for c in arms:
            c.timed_call()
    for _ in range(TRAINS):  # and train by train
        for c in arms:
            c.timed_train(calls // TRAINS)
    res = [c.result(torch, warmup, calls) for c in arms]
    same = bool(torch.equal(bout, sout))  # every arm has made the same number of calls from the same start
    for c in arms:
        for o in c.objects:
            o.close()
        for hh in c.handles:
            hh.close()
    b, s = res
    return dict(case=k["name"], format=k["fmt"], wide_rate=k["wide"], P=P, Q=Q, captures=S, channels_per_capture=Cn,
                n_out=N_OUT, wide_samples_per_capture=n_in, arms=res,
                bank_over_objects=dict(
                    back_to_back=b["ms_per_call_back_to_back"]["median"] / s["ms_per_call_back_to_back"]["median"],
                    synchronised=b["ms_per_call_synchronised"]["median"] / s["ms_per_call_synchronised"]["median"]),
                bank_rows_equal_the_objects=same)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wb_bank_rational.json"))
    a = ap.parse_args()
    if a.calls < 50:
        ap.error("--calls must be at least 50")
    import torch
    import fmx
    if not torch.cuda.is_available():
        sys.exit("bench_wb_bank_rational: no GPU")
    cases = [run_case(fmx, torch, k, a.warmup, a.calls) for k in CASES]
    doc = dict(tool="tools/bench_wb_bank_rational.py", library=fmx.build_info(), device=torch.cuda.get_device_name(0),
               cases=cases)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))
    for c in cases:
        if not c["bank_rows_equal_the_objects"]:
            sys.exit(f"bench_wb_bank_rational: {c['case']}: the bank's rows differ from the objects'")
        if c["arms"][0]["times_real_time"] <= 1.0:
            sys.exit(f"bench_wb_bank_rational: {c['case']}: a bank call is slower than real time")


if __name__ == "__main__":
    main()
