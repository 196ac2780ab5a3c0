#!/usr/bin/env python3
"""Times the capture bank against what a user with several captures does
without it, in one process --

  A  one handle of S * Cs channels and one bank of S captures: one
     fmx_wb_bank_process_block + fmx_wb_bank_signal per block (k_wbb ->
     k_wbb_hist -> k_fecf -> k_wbb_clip -> k_wbb_level on the stage stream, the
     unchanged step behind it at S * Cs channels);
  B  S handles of Cs channels, each with its own fmx_wb object: S x
     (fmx_wb_process_block + fmx_wb_signal) per block, one sync over all
     handles at the train's end.

tools/bench_band_receiver.py's scheme: warm-up calls per arm, then --reps
repetitions that alternate a train of --train blocks per arm, each train ending
in one synchronisation (of every handle of the arm); the clock is the host's
around the synchronised train, per-block time = train time / blocks; median
and min-max over the repetitions, plus fmx_kernel_times of a train of arm A
(the channelizer and level kernels are not timed).

Cases, 4096 outputs per block (17.07 ms of signal at 240 kHz), stereo + RDS:
  dongles  u8, D = 10 (2.4 MS/s), S = 16 captures of 5 channels;
  bands    int16, D = 100 (24 MS/s), S = 4 captures of 205 channels.

Writes one JSON document (default profiles/wb_bank.json) and exits non-zero
when, in the dongle case, A's median is not below B's, or when A is not faster
than real time in either case.  The band case's A / B is reported, not gated:
four handles' sixteen streams may overlap on the device.  Needs a GPU."""
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


def _stats(ms):
    import numpy as np
    ms = np.sort(np.array(ms))
    return dict(median=float(np.median(ms)), min=float(ms[0]), max=float(ms[-1]))


class Outputs:
    """Three rotating output sets and level-record arrays of one handle, as bench.py rotates them."""

    def __init__(self, fmx, torch, C, n):
        dev = torch.device("cuda")
        f = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)  # noqa: E731
        z = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)  # noqa: E731
        self.T = T = dict(pl=f(3, C, n), pr=f(3, C, n), clip=f(3, C), cnt=z(3, C), st=z(3, C), pil=z(3, C), ind=z(3, C),
                          gcnt=z(3, C), grp=z(3, C, GS, 4))
        self.outs = [fmx.BlockOut(None, 0, T["pl"][k].data_ptr(), T["pr"][k].data_ptr(), n, T["cnt"][k].data_ptr(),
                                  T["st"][k].data_ptr(), T["pil"][k].data_ptr(), T["clip"][k].data_ptr(),
                                  T["grp"][k].data_ptr(), GS, T["gcnt"][k].data_ptr(), None, T["ind"][k].data_ptr())
                     for k in range(3)]
        self.lev = torch.zeros((3, C * 40), dtype=torch.uint8, device=dev)

    def check(self, torch):
        import numpy as np
        assert bool(torch.isfinite(self.T["pl"]).all()) and int(self.T["cnt"].min()) > 0
        rec = self.lev.cpu().numpy().view(np.dtype([("level120", "<f4"), ("smoothed", "<f4"), ("dbfs", "<f8"),
                                                    ("cdb", "<f8"), ("hard", "<f8"), ("near", "<f8")]))
        assert np.isfinite(rec["dbfs"]).all() and (rec["dbfs"] > -100.0).all()


def run_case(fmx, torch, name, fmt, D, S, Cs, step, warmup, reps, train):
    Fs, n = D * DSP, N_OUT
    s16 = fmt == "s16"
    freqs = [-int((Cs - 1) * step / 2) + i * step for i in range(Cs)]
    wcfg = fmx.make_wb_config(Fs, DSP, fmx.FMX_WB_S16 if s16 else fmx.FMX_WB_U8, TPP, n)
    hcfg = fmx.make_config(iq_rate=DSP, dsp_rate=DSP, block=n)
    g = torch.Generator(device="cpu").manual_seed(1)
    if s16:
        raw = torch.randint(-32768, 32768, (S, 2 * n * D), generator=g, dtype=torch.int32).to(torch.int16).to("cuda")
    else:
        raw = torch.randint(0, 256, (S, 2 * n * D), generator=g, dtype=torch.int32).to(torch.uint8).to("cuda")
    row_bytes = raw.element_size() * 2 * n * D
    # arm A
    hA = fmx.Handle(hcfg, S * Cs)
    bank = fmx.WidebandBank(hA, wcfg, [freqs] * S)
    oA = Outputs(fmx, torch, S * Cs, n)
    # arm B
    hB = [fmx.Handle(hcfg, Cs) for _ in range(S)]
    wB = [fmx.Wideband(h, wcfg, freqs) for h in hB]
    oB = [Outputs(fmx, torch, Cs, n) for _ in range(S)]
    torch.cuda.synchronize()
    blocks = [0, 0]

    def block_a():
        k = blocks[0] % 3
        bank.process_block(raw.data_ptr(), n * D, n, oA.outs[k])
        bank.signal(oA.lev[k].data_ptr())
        blocks[0] += 1

    def block_b():
        k = blocks[1] % 3
        for s in range(S):
            wB[s].process_block(raw.data_ptr() + s * row_bytes, n, oB[s].outs[k])
            wB[s].signal(oB[s].lev[k].data_ptr())
        blocks[1] += 1

    arms = {"A_bank": (block_a, [hA]), "B_one_handle_per_capture": (block_b, hB)}

    def run_train(fn, handles, k):
        for h in handles:
            h.sync()
        t0 = time.perf_counter()
        for _ in range(k):
            fn()
        for h in handles:
            h.sync()
        return (time.perf_counter() - t0) * 1e3 / k

    for fn, hs in arms.values():
        run_train(fn, hs, warmup)
    ms = {k: [] for k in arms}
    for _ in range(reps):
        for k, (fn, hs) in arms.items():
            ms[k].append(run_train(fn, hs, train))
    hA.timing_enable(True)
    run_train(block_a, [hA], train)
    kt = hA.kernel_times()
    hA.timing_enable(False)
    oA.check(torch)
    for o in oB:
        o.check(torch)
    bank.close()
    hA.close()
    for w, h in zip(wB, hB):
        w.close()
        h.close()
    signal_ms = n / DSP * 1e3
    res = dict(case=name, format=fmt, D=D, wide_rate=Fs, taps=D * TPP, captures=S, channels_per_capture=Cs,
               channels=S * Cs, step_hz=step, n_out=n, stereo=1, rds=1, warmup=warmup, reps=reps, blocks_per_train=train,
               signal_ms=signal_ms)
    for k in arms:
        st = _stats(ms[k])
        res[k] = dict(ms_per_block=st, times_real_time=signal_ms / st["median"])
    a, b = res["A_bank"]["ms_per_block"], res["B_one_handle_per_capture"]["ms_per_block"]
    res["A_over_B"] = a["median"] / b["median"]
    res["A_over_B_inside_the_arms_spread"] = bool(a["min"] <= b["max"] and b["min"] <= a["max"])
    res["kernel_ms_per_launch_arm_A"] = {k: (v[0] / v[1] if v[1] else None) for k, v in kt.items()}
    res["kernel_launches_arm_A"] = {k: v[1] for k, v in kt.items()}
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--train", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wb_bank.json"))
    a = ap.parse_args()
    if a.reps < 10:
        ap.error("--reps must be at least 10")
    import torch
    import fmx
    if not torch.cuda.is_available():
        sys.exit("bench_wb_bank: no GPU")
    cases = [run_case(fmx, torch, "dongles_16x5ch_2.4MSps_u8", "u8", 10, 16, 5, 400_000, a.warmup, a.reps, a.train),
             run_case(fmx, torch, "bands_4x205ch_24MSps_s16", "s16", 100, 4, 205, 100_000, a.warmup, a.reps, a.train)]
    doc = dict(tool="tools/bench_wb_bank.py", library=fmx.build_info(), device=torch.cuda.get_device_name(0), cases=cases)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))
    dongles, bands = cases
    if dongles["A_over_B"] >= 1.0:
        sys.exit("bench_wb_bank: the bank is not faster than one handle per capture in the dongle case")
    for c in cases:
        if c["A_bank"]["times_real_time"] <= 1.0:
            sys.exit(f"bench_wb_bank: the bank is slower than real time in case {c['case']}")


if __name__ == "__main__":
    main()
