#!/usr/bin/env python3
"""Times the synthetic FM band generator (fmx_synth_band_generate, kernel
k_synth_band), three cases in one process --

  a  one int16 capture at 24 MS/s, 52 stereo + RDS stations of amplitude 0.03
     every 400 kHz, n = 409 600 samples per call (17.07 ms of signal): the band
     tools/bench_band_receiver.py --band receives;
  b  sixteen u8 captures at 2.048 MS/s with 5 stations each, n = 34 944 (17.06
     ms): a bank of dongles;
  c  case a's first 25 600 samples through fmx_synth_band_host on 16 threads,
     scaled to the full length: the only route that existed before.

Device cases: warm-up calls, then --reps trains of --train calls, each train
ending in one fmx_sync; the calls run on the handle's own stream, so the clock
is the host's around the synchronised train and per-call time = train time /
calls.  Successive calls advance sample0, as a stream does.  Case c: --host-reps
calls.  Median and min-max per case, and each case's ratio to real time
(reported, not gated).

Writes one JSON document (default profiles/synth_band.json) and exits non-zero
unless case a's device median is below case c's scaled host time.  Needs a GPU."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fmtuner-sdr_amd"))

A_RATE, A_N, A_STATIONS, A_STEP, A_AMP = 24_000_000, 409_600, 52, 400_000, 0.03
B_RATE, B_N, B_CAPTURES, B_PER = 2_048_000, 34_944, 16, 5
C_N, C_THREADS = 25_600, 16


def _stats(ms):
    import numpy as np
    ms = np.sort(np.array(ms))
    return dict(median=float(np.median(ms)), min=float(ms[0]), max=float(ms[-1]))


def a_stations():
    f0 = -(A_STATIONS - 1) * A_STEP // 2
    return [(f0 + k * A_STEP, A_AMP) for k in range(A_STATIONS)]


def b_captures():
    return [[(-800_000 + 400_000 * k, 0.1) for k in range(B_PER)] for _ in range(B_CAPTURES)]


def device_case(fmx, torch, h, name, cfg, captures, n, warmup, reps, train):
    s16 = cfg.format == fmx.FMX_WB_S16
    band = fmx.SynthBand(h, cfg, 0, captures)
    out = torch.zeros((len(captures), 2 * n), dtype=torch.int16 if s16 else torch.uint8, device="cuda")
    torch.cuda.synchronize()
    pos = [0]

    def run_train(k):
        h.sync()
        t0 = time.perf_counter()
        for _ in range(k):
            band.generate(pos[0], n, out.data_ptr(), n)
            pos[0] += n
        h.sync()
        return (time.perf_counter() - t0) * 1e3 / k

    run_train(warmup)
    ms = [run_train(train) for _ in range(reps)]
    # the last call's samples against the host's, 2048 of them: the timed kernel is the tested one
    import numpy as np
    got = out.cpu().numpy().reshape(len(captures), n, 2)[:, :2048]
    want = fmx.synth_band_host(cfg, 0, captures, pos[0] - n, 2048, bits=band.bits, threads=C_THREADS)
    worst = int(np.abs(got.astype(np.int64) - want.astype(np.int64)).max())
    band.close()
    if worst > 1:
        sys.exit(f"bench_synth_band: case {name}: the device differs from the host by {worst} LSB")
    st = _stats(ms)
    signal_ms = n / cfg.wide_rate * 1e3
    return dict(case=name, wide_rate=cfg.wide_rate, format="s16" if s16 else "u8", kind=cfg.kind,
                captures=len(captures), stations=sum(len(c) for c in captures), n_samples=n, signal_ms=signal_ms,
                warmup=warmup, reps=reps, calls_per_train=train, ms_per_call=st,
                times_real_time=signal_ms / st["median"],
                station_samples_per_us=sum(len(c) for c in captures) * n / (st["median"] * 1e3),
                max_lsb_from_host_2048_samples=worst)


def host_case(fmx, cfg, captures, reps):
    bits = fmx.synth_band_bits(cfg, 0, sum(len(c) for c in captures))[1]
    ms = []
    for k in range(reps):
        t0 = time.perf_counter()
        fmx.synth_band_host(cfg, 0, captures, k * C_N, C_N, bits=bits, threads=C_THREADS)
        ms.append((time.perf_counter() - t0) * 1e3)
    st = _stats(ms)
    scale = A_N / C_N
    signal_ms = A_N / cfg.wide_rate * 1e3
    return dict(case="c_host_16_threads_scaled", wide_rate=cfg.wide_rate, format="s16", kind=cfg.kind, captures=1,
                stations=len(captures[0]), n_samples_timed=C_N, threads=C_THREADS, cpus=os.cpu_count(), scaled_to=A_N,
                reps=reps, ms_per_call_timed=st, ms_per_call=dict(median=st["median"] * scale, min=st["min"] * scale,
                                                                  max=st["max"] * scale),
                signal_ms=signal_ms, times_real_time=signal_ms / (st["median"] * scale))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--train", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "synth_band.json"))
    a = ap.parse_args()
    if a.reps < 10:
        ap.error("--reps must be at least 10")
    import torch
    import fmx
    if not torch.cuda.is_available():
        sys.exit("bench_synth_band: no GPU")
    h = fmx.Handle(fmx.make_config(iq_rate=240_000, dsp_rate=240_000, block=4096), 1)
    cfg_a = fmx.make_synth_band(wide_rate=A_RATE, format=fmx.FMX_WB_S16, kind=2, n_bits=8192)
    cfg_b = fmx.make_synth_band(wide_rate=B_RATE, format=fmx.FMX_WB_U8, kind=2, n_bits=8192, noise_std=0.01)
    cases = [device_case(fmx, torch, h, "a_24MSps_s16_52_stations", cfg_a, [a_stations()], A_N, a.warmup, a.reps, a.train),
             device_case(fmx, torch, h, "b_16x2.048MSps_u8_5_stations", cfg_b, b_captures(), B_N, a.warmup, a.reps, a.train),
             host_case(fmx, cfg_a, [a_stations()], a.host_reps)]
    h.close()
    doc = dict(tool="tools/bench_synth_band.py", library=fmx.build_info(), device=torch.cuda.get_device_name(0),
               tile=fmx.synth_band_tile(), cases=cases,
               device_a_over_host_c=cases[0]["ms_per_call"]["median"] / cases[2]["ms_per_call"]["median"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))
    if doc["device_a_over_host_c"] >= 1.0:
        sys.exit("bench_synth_band: the device is not faster than the host route in case a")


if __name__ == "__main__":
    main()
