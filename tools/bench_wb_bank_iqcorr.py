#!/usr/bin/env python3
"""Times fmx_wb_bank_process with every capture's DC / IQ-imbalance correction
in AUTO (fmx_wb_bank_set_iq_correction; kernels k_bank_iqc_sums,
k_bank_iqc_finish and k_bank_iqc) beside the same bank
with every capture in OFF (k_wbb) and beside what a user does without the
bank's correction: one handle and one fmx_wb object in AUTO per capture
(k_iqc_sums, k_iqc_finish and k_wb_iqc, sixteen times).  One run, the three
arms interleaved call by call and train by train, so that clock and thermal
state are shared; the clock is the host's around work that ends in fmx_sync
of every handle of the arm (tools/bench_wb_iqcorr.py's scheme): each call
alone on idle streams, and trains of calls back to back.

Case: section 22's dongles -- sixteen u8 captures of 5 channels, 2.4 MS/s
(D = 10), 4096 outputs per call: 40 960 raw samples per capture, 17.07 ms of
signal.  Writes one JSON document (default profiles/wb_bank_iqcorr.json) with
the arms' times, AUTO's ratio to OFF and the bank's ratio to the sixteen
objects (figures, not gates); exits non-zero when an AUTO bank call is not
faster than real time.  Needs a GPU."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fmtuner-sdr_amd"))

DSP = 240_000
WIDE, D, CAPTURES, CHANNELS, STEP, N_OUT = 2_400_000, 10, 16, 5, 400_000, 4096
TRAINS = 5


class Arm:
    """calls: what one call queues; handles: synchronised around it; readback() -> capture 0's parameters."""

    def __init__(self, name, handles, call, readback, out):
        self.name, self.handles, self.call, self.readback, self.out = name, handles, call, readback, out
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
        return dict(arm=self.name, parameters_capture_0=list(self.readback()), format="u8", wide_rate=WIDE, D=D,
                    captures=CAPTURES, channels_per_capture=CHANNELS, n_out=N_OUT, wide_samples_per_capture=N_OUT * D,
                    warmup=warmup, calls=calls,
                    ms_per_call_synchronised=dict(median=float(np.median(ms)), min=float(ms[0]), max=float(ms[-1]),
                                                  p10=float(ms[len(ms) // 10]), p90=float(ms[(9 * len(ms)) // 10])),
                    ms_per_call_back_to_back=dict(median=train, min=float(tr[0]), max=float(tr[-1]), trains=len(tr)),
                    signal_ms=signal_ms, times_real_time=signal_ms / train,
                    times_real_time_synchronised=signal_ms / float(np.median(ms)))


def bank_arm(fmx, torch, name, mode, raw, wcfg, freqs):
    h = fmx.Handle(fmx.make_config(iq_rate=DSP, dsp_rate=DSP), CAPTURES * CHANNELS)
    bank = fmx.WidebandBank(h, wcfg, [freqs] * CAPTURES)
    if mode != fmx.FMX_IQC_OFF:
        bank.set_iq_correction(mode, None, 0.0)
    out = torch.zeros((CAPTURES * CHANNELS, 2 * N_OUT), dtype=torch.float32, device="cuda")
    arm = Arm(name, [h], lambda: bank.process(raw.data_ptr(), N_OUT * D, N_OUT, out.data_ptr(), N_OUT),
              lambda: bank.iq_correction(0), out)
    arm.objects = [bank]
    return arm


def singles_arm(fmx, torch, name, mode, raw, wcfg, freqs):
    hs = [fmx.Handle(fmx.make_config(iq_rate=DSP, dsp_rate=DSP), CHANNELS) for _ in range(CAPTURES)]
    wbs = [fmx.Wideband(h, wcfg, freqs) for h in hs]
    for wb in wbs:
        wb.set_iq_correction(mode, None, 0.0)
    out = torch.zeros((CAPTURES * CHANNELS, 2 * N_OUT), dtype=torch.float32, device="cuda")
    row, orow = raw.element_size() * 2 * N_OUT * D, 4 * CHANNELS * 2 * N_OUT

    def call():
        for s, wb in enumerate(wbs):
            wb.process(raw.data_ptr() + s * row, N_OUT, out.data_ptr() + s * orow, N_OUT)

    arm = Arm(name, hs, call, wbs[0].iq_correction, out)
    arm.objects = wbs
    return arm


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wb_bank_iqcorr.json"))
    a = ap.parse_args()
    if a.calls < 50:
        ap.error("--calls must be at least 50")
    import torch
    import fmx
    if not torch.cuda.is_available():
        sys.exit("bench_wb_bank_iqcorr: no GPU")
    g = torch.Generator(device="cpu").manual_seed(1)
    raw = torch.randint(0, 256, (CAPTURES, 2 * N_OUT * D), generator=g, dtype=torch.int32).to(torch.uint8).to("cuda")
    wcfg = fmx.make_wb_config(WIDE, DSP, fmx.FMX_WB_U8, 28, N_OUT)
    freqs = [-int((CHANNELS - 1) * STEP / 2) + i * STEP for i in range(CHANNELS)]
    arms = [bank_arm(fmx, torch, "bank_off", fmx.FMX_IQC_OFF, raw, wcfg, freqs),
            bank_arm(fmx, torch, "bank_auto", fmx.FMX_IQC_AUTO, raw, wcfg, freqs),
            singles_arm(fmx, torch, "sixteen_objects_auto", fmx.FMX_IQC_AUTO, raw, wcfg, freqs)]
    torch.cuda.synchronize()
    for _ in range(a.warmup):
        for c in arms:
            c.call()
    for c in arms:
        c.sync()
    for _ in range(a.calls):  # interleaved call by call
        for c in arms:
            c.timed_call()
    for _ in range(TRAINS):   # and train by train
        for c in arms:
            c.timed_train(a.calls // TRAINS)
    res = [c.result(torch, a.warmup, a.calls) for c in arms]
    same = bool(torch.equal(arms[1].out, arms[2].out))  # the bank's rows are the sixteen objects'
    for c in arms:
        for o in c.objects:
            o.close()
        for h in c.handles:
            h.close()
    off, auto, singles = res
    over = lambda x, y: dict(back_to_back=x["ms_per_call_back_to_back"]["median"] / y["ms_per_call_back_to_back"]["median"],  # noqa: E731
                             synchronised=x["ms_per_call_synchronised"]["median"] / y["ms_per_call_synchronised"]["median"])
    doc = dict(tool="tools/bench_wb_bank_iqcorr.py", library=fmx.build_info(), device=torch.cuda.get_device_name(0), arms=res,
               auto_over_off=over(auto, off), bank_over_sixteen_objects=over(auto, singles),
               bank_rows_equal_the_objects=same)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))
    if not same:
        sys.exit("bench_wb_bank_iqcorr: the bank's rows differ from the sixteen objects'")
    if auto["times_real_time"] <= 1.0:
        sys.exit("bench_wb_bank_iqcorr: an AUTO bank call is slower than real time")


if __name__ == "__main__":
    main()
