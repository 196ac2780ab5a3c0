#!/usr/bin/env python3
"""Times the band receiver: one wide IQ capture in, every station's audio,
stereo state and RDS groups out, three ways in one process --

  A  fmx_wb_process_block (k_wb -> k_fecf -> k_pilot | k_rs -> k_rds | k_pll |
     k_bits -> k_audio on the pipelined step's four streams);
  B  the same call with FMX_DIAG_FE_GENERIC (k_frontend on the rows instead of
     k_fecf / k_pilot / k_rs);
  C  the route before that call existed: fmx_wb_process -> fmx_demod ->
     fmx_stereo -> fmx_afpost -> fmx_rds, five stage calls on one stream.

Warm-up calls per arm, then --reps repetitions that alternate a train of
--train calls per arm, each train ending in one fmx_sync.  The calls run on
the handle's own streams, which the ABI does not hand out, so the clock is the
host's around the synchronised train; per-call time = train time / calls.
Median and min-max over the repetitions, plus fmx_kernel_times of a train of
arm A (k_wb is not timed).

Cases: the band of tools/bench_channelizer.py -- int16, D = 100 (24 MS/s), 28
taps per phase, 205 channels at 100 kHz, 4096 outputs per call (17.07 ms of
signal), stereo + RDS -- and a slice: D = 10 (2.4 MS/s), 5 channels.

Writes one JSON document (default profiles/wb_receiver.json) and exits
non-zero when, in the band case, A's median is not below C's or A is not
faster than real time.  The slice is reported, not gated: five channels are
launch latency.

--signal times a fourth arm instead of B, alternating with A and C in the same
scheme --

  A+S  arm A's call followed by fmx_wb_signal (k_wb_scan_clip and k_wb_level
       behind the call's front end on the stage stream): every station's RF
       level with its audio, three rotating record arrays;

writes profiles/wb_receiver_signal.json by default and exits non-zero when, in
the band case, the A+S median is not below C's or A+S is not faster than real
time.  The A+S / A ratio is reported with both arms' min-max, not gated.

--band times, instead of B, arms A and C a second time on a band with stations
in it: the 205-channel case's capture is then tools/bench_synth_band.py's case
(a) -- 52 stereo + RDS stations of amplitude 0.03 on every fourth channel --
generated on the GPU by fmx_synth_band_generate as BAND_BLOCKS consecutive
blocks, which the band arms read in turn (one seam per BAND_BLOCKS calls), so
pilot PLLs lock, k_bits finds block sync and groups are written.  A soak of
BAND_BLOCKS calls of arm A then counts the RDS groups and stereo flags seen.
Writes profiles/wb_receiver_band.json by default; the band arms are reported
beside the noise-capture ones, not gated.
Needs a GPU."""
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
GS = 8
BAND_BLOCKS = 64      # consecutive 17.07 ms blocks of the generated band (1.09 s of signal)
BAND_AMPLITUDE = 0.03


def _stats(ms):
    import numpy as np
    ms = np.sort(np.array(ms))
    return dict(median=float(np.median(ms)), min=float(ms[0]), max=float(ms[-1]))


def run_case(fmx, torch, name, D, channels, step, warmup, reps, train, signal=False, band=False):
    Fs, C, n = D * DSP, channels, N_OUT
    freqs = [-int((C - 1) * step / 2) + i * step for i in range(C)]
    h = fmx.Handle(fmx.make_config(iq_rate=DSP, dsp_rate=DSP, block=n), C)
    wb = fmx.Wideband(h, fmx.make_wb_config(Fs, DSP, fmx.FMX_WB_S16, TPP, n), freqs)
    dev = torch.device("cuda")
    g = torch.Generator(device="cpu").manual_seed(1)
    raw = torch.randint(-32768, 32768, (2 * n * D,), generator=g, dtype=torch.int32).to(torch.int16).to(dev)
    f = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)  # noqa: E731
    z = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)  # noqa: E731
    # three rotating output sets of the one-call arms, as bench.py rotates them
    T = dict(pl=f(3, C, n), pr=f(3, C, n), clip=f(3, C), cnt=z(3, C), st=z(3, C), pil=z(3, C), ind=z(3, C),
             gcnt=z(3, C), grp=z(3, C, GS, 4))
    outs = [fmx.BlockOut(None, 0, T["pl"][k].data_ptr(), T["pr"][k].data_ptr(), n, T["cnt"][k].data_ptr(),
                         T["st"][k].data_ptr(), T["pil"][k].data_ptr(), T["clip"][k].data_ptr(),
                         T["grp"][k].data_ptr(), GS, T["gcnt"][k].data_ptr(), None, T["ind"][k].data_ptr())
            for k in range(3)]
    # the stage chain's buffers
    bb, mpx, lf, rf, sl, sr = f(C, 2 * n), f(C, n), f(C, n), f(C, n), f(C, n), f(C, n)
    s_st, s_pil, s_cnt, s_gcnt, s_grp = z(C), z(C), z(C), z(C), z(C, GS, 4)
    lev = torch.zeros((3, C * 40), dtype=torch.uint8, device=dev)  # fmx_signal_level records, rotating with the sets
    ring = None
    if band:  # stations on every fourth channel, BAND_BLOCKS consecutive blocks of them
        bcfg = fmx.make_synth_band(wide_rate=Fs, format=fmx.FMX_WB_S16, kind=2, n_bits=8192)
        sb = fmx.SynthBand(h, bcfg, 0, [[(fq, BAND_AMPLITUDE) for fq in freqs[::4]]])
        ring = torch.zeros((BAND_BLOCKS, 2 * n * D), dtype=torch.int16, device=dev)
        for k in range(BAND_BLOCKS):
            sb.generate(k * n * D, n * D, ring[k].data_ptr(), n * D)
        h.sync()
        sb.close()
    torch.cuda.synchronize()
    calls = [0]
    band_calls = [0]

    def band_block():
        band_calls[0] += 1
        return ring[(band_calls[0] - 1) % BAND_BLOCKS].data_ptr()

    def one_call_band():
        wb.process_block(band_block(), n, outs[calls[0] % 3])
        calls[0] += 1

    def stage_chain_band():
        stage_chain(band_block())

    def one_call():
        wb.process_block(raw.data_ptr(), n, outs[calls[0] % 3])
        calls[0] += 1

    def one_call_and_signal():
        k = calls[0] % 3
        one_call()
        wb.signal(lev[k].data_ptr())

    def stage_chain(src=None):
        wb.process(raw.data_ptr() if src is None else src, n, bb.data_ptr(), n)
        h.demod(bb.data_ptr(), 2 * n, n, mpx.data_ptr(), n)
        h.stereo(mpx.data_ptr(), n, n, lf.data_ptr(), rf.data_ptr(), n, s_st.data_ptr(), s_pil.data_ptr())
        h.afpost(lf.data_ptr(), rf.data_ptr(), n, n, sl.data_ptr(), sr.data_ptr(), n, n, s_cnt.data_ptr())
        h.rds(mpx.data_ptr(), n, n, s_grp.data_ptr(), GS, s_gcnt.data_ptr())

    arms = {"A_one_call": (0, one_call), "B_one_call_generic_front_end": (1, one_call), "C_stage_calls": (0, stage_chain)}
    if signal:
        arms = {"A_one_call": (0, one_call), "AS_one_call_and_signal": (0, one_call_and_signal),
                "C_stage_calls": (0, stage_chain)}

    if band:
        arms = {"A_one_call": (0, one_call), "A_one_call_band": (0, one_call_band), "C_stage_calls": (0, stage_chain),
                "C_stage_calls_band": (0, stage_chain_band)}

    def run_train(generic, fn, k):
        h.diag_set(fmx.FMX_DIAG_FE_GENERIC, generic)
        h.sync()
        t0 = time.perf_counter()
        for _ in range(k):
            fn()
        h.sync()
        return (time.perf_counter() - t0) * 1e3 / k

    for generic, fn in arms.values():
        run_train(generic, fn, warmup)
    ms = {k: [] for k in arms}
    for _ in range(reps):
        for k, (generic, fn) in arms.items():
            ms[k].append(run_train(generic, fn, train))
    h.diag_set(fmx.FMX_DIAG_FE_GENERIC, 0)
    h.timing_enable(True)
    run_train(0, one_call, train)
    kt = h.kernel_times()
    kt_band = None
    if band:  # the same train on the band: fmx_kernel_times accumulates, so the difference is the band's
        run_train(0, one_call_band, train)
        kt2 = h.kernel_times()
        kt_band = {k: (kt2[k][0] - kt[k][0], kt2[k][1] - kt[k][1]) for k in kt}
    h.timing_enable(False)
    assert bool(torch.isfinite(T["pl"]).all()) and bool(torch.isfinite(sl).all())
    assert int(T["cnt"].min()) > 0 and int(s_cnt.min()) > 0
    if signal:
        import numpy as np
        rec = lev.cpu().numpy().view(np.dtype([("level120", "<f4"), ("smoothed", "<f4"), ("dbfs", "<f8"), ("cdb", "<f8"),
                                               ("hard", "<f8"), ("near", "<f8")]))
        assert np.isfinite(rec["dbfs"]).all() and (rec["dbfs"] > -100.0).all() and (rec["hard"] > 0.0).all()
    soak = None
    if band:  # the lock paths: BAND_BLOCKS consecutive blocks from the reset state, outputs read after every call
        h.reset()
        wb.reset()
        groups = stereo = 0
        per_station = torch.zeros(C, dtype=torch.int64)
        for k in range(BAND_BLOCKS):
            wb.process_block(ring[k].data_ptr(), n, outs[0])
            h.sync()
            g = T["gcnt"][0].cpu().to(torch.int64)
            per_station += g
            groups += int(g.sum())
            stereo += int(T["st"][0].sum())
        on = per_station[::4]
        soak = dict(calls=BAND_BLOCKS, stations=len(freqs[::4]), rds_groups=groups, stereo_flags=stereo,
                    stations_with_groups=int((on > 0).sum()), groups_on_empty_channels=int(groups - int(on.sum())),
                    stereo_flags_last_call=int(T["st"][0].sum()))
    wb.close()
    h.close()
    signal_ms = n / DSP * 1e3
    res = dict(case=name, format="s16", D=D, wide_rate=Fs, taps=D * TPP, channels=C, step_hz=step, n_out=n,
               stereo=1, rds=1, warmup=warmup, reps=reps, calls_per_train=train, signal_ms=signal_ms)
    for k in arms:
        st = _stats(ms[k])
        res[k] = dict(ms_per_call=st, times_real_time=signal_ms / st["median"])
    res["A_over_C"] = res["A_one_call"]["ms_per_call"]["median"] / res["C_stage_calls"]["ms_per_call"]["median"]
    if band:
        res["band"] = dict(stations=len(freqs[::4]), amplitude=BAND_AMPLITUDE, kind=2, blocks=BAND_BLOCKS, soak=soak)
        res["A_band_over_A"] = (res["A_one_call_band"]["ms_per_call"]["median"] /
                                res["A_one_call"]["ms_per_call"]["median"])
        res["C_band_over_C"] = (res["C_stage_calls_band"]["ms_per_call"]["median"] /
                                res["C_stage_calls"]["ms_per_call"]["median"])
    elif signal:
        res["AS_over_A"] = (res["AS_one_call_and_signal"]["ms_per_call"]["median"] /
                            res["A_one_call"]["ms_per_call"]["median"])
        res["AS_over_C"] = (res["AS_one_call_and_signal"]["ms_per_call"]["median"] /
                            res["C_stage_calls"]["ms_per_call"]["median"])
    else:
        res["A_over_B"] = (res["A_one_call"]["ms_per_call"]["median"] /
                           res["B_one_call_generic_front_end"]["ms_per_call"]["median"])
    res["kernel_ms_per_launch_arm_A"] = {k: (v[0] / v[1] if v[1] else None) for k, v in kt.items()}
    res["kernel_launches_arm_A"] = {k: v[1] for k, v in kt.items()}
    if kt_band:
        res["kernel_ms_per_launch_arm_A_band"] = {k: (v[0] / v[1] if v[1] else None) for k, v in kt_band.items()}
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--train", type=int, default=10)
    ap.add_argument("--signal", action="store_true", help="time arm A+S (the call followed by fmx_wb_signal) instead of B")
    ap.add_argument("--band", action="store_true",
                    help="time arms A and C on a generated band of 52 stations as well, instead of B")
    ap.add_argument("--out", default=None, help="default profiles/wb_receiver.json (wb_receiver_signal.json with --signal, "
                                                "wb_receiver_band.json with --band)")
    a = ap.parse_args()
    if a.band and a.signal:
        ap.error("--band and --signal are separate runs")
    if a.out is None:
        name = "wb_receiver_band.json" if a.band else "wb_receiver_signal.json" if a.signal else "wb_receiver.json"
        a.out = os.path.join(ROOT, "profiles", name)
    if a.reps < 10:
        ap.error("--reps must be at least 10")
    import torch
    import fmx
    if not torch.cuda.is_available():
        sys.exit("bench_band_receiver: no GPU")
    cases = [run_case(fmx, torch, "band_24MSps_205ch_100kHz", 100, 205, 100_000, a.warmup, a.reps, a.train, a.signal,
                      a.band),
             run_case(fmx, torch, "slice_2.4MSps_5ch", 10, 5, 400_000, a.warmup, a.reps, a.train, a.signal)]
    doc = dict(tool="tools/bench_band_receiver.py", library=fmx.build_info(), device=torch.cuda.get_device_name(0),
               cases=cases)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))
    band = cases[0]
    if band["A_over_C"] >= 1.0:
        sys.exit("bench_band_receiver: the one call is not faster than the five stage calls in the band case")
    if band["A_one_call"]["times_real_time"] <= 1.0:
        sys.exit("bench_band_receiver: the band case is slower than real time")
    if a.signal:
        if band["AS_over_C"] >= 1.0:
            sys.exit("bench_band_receiver: the call with fmx_wb_signal is not faster than the five stage calls in the band case")
        if band["AS_one_call_and_signal"]["times_real_time"] <= 1.0:
            sys.exit("bench_band_receiver: the band case with fmx_wb_signal is slower than real time")


if __name__ == "__main__":
    main()
