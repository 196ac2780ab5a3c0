#!/usr/bin/env python3
"""SHA-256 of the raw output bytes of the wideband family (fmx_wb_process,
the rational object, the capture bank, the band scan and the level records)
on seeded inputs, one digest per case: two builds of the library compute the
same thing exactly when their lists are equal.  The library is the one FMX_LIB
names (default: fmtuner-sdr_amd/libfmx.so); run it once per library, each in a
process of its own:

    FMX_LIB=.../libfmx_base.so python tools/wb_digest.py --out base.json
    python tools/wb_digest.py --out new.json

Cases (every one well under a second):
  wb       u8 / int16, D = 10, 25, 100 (even window, odd window, a tile count
           the LDS budget limits), 17 channels (a ragged group of one), 300
           outputs in calls of 37 and 263 (a partial, then a full history);
           correction OFF, FIXED and AUTO; at D = 10 also the input offset by
           one sample, by half a sample (no whole-sample loads) and a sample
           counter above 2^40
  wbr      the rational cases of tests/test_gpu_wb_rational.py, 17 channels,
           16 Q 2 + Q outputs in two calls
  bank     three captures of 17, 0 and 5 channels, calls of 37 and 263
  scan     70 points (a ragged last group, a second blockIdx.y), D = 10, 25,
           100, correction OFF and FIXED: the scan's level records
  signal   fmx_wb_signal and fmx_wb_bank_signal at an odd n over rows whose
           base is 16-, 8- and 4-byte aligned (the level kernel's three load
           widths)
Prints one JSON document {"library": ..., "digests": {case: hex}}.  Needs a GPU."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fmtuner-sdr_amd"))

DSP = 240_000
NCH = 17
SIZES = (37, 263)
FIXED = (0.013, -0.021, 1.07, -0.045)  # dc_i, dc_q, gain, cross
RATIONAL = [(2_000_000, "u8", 28), (2_000_000, "s16", 28), (20_000_000, "s16", 28), (2_048_000, "u8", 28),
            (600_000, "u8", 12)]
LEVEL_BYTES = 40  # fmx_signal_level


def raw_samples(fmt, n, seed):
    rng = np.random.default_rng(seed)
    if fmt == "u8":
        return rng.integers(0, 256, 2 * n, dtype=np.uint8)
    return rng.integers(-32768, 32768, 2 * n).astype(np.int16)


def freqs(Fs, n, seed=5):
    rng = np.random.default_rng(seed)
    base = [0, 1, -1, 123_457, -Fs // 2 + 1, Fs // 2]
    return (base + [int(v) for v in rng.integers(-Fs // 2, Fs // 2, n)])[:n]


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.cpu().numpy().tobytes())
    return h.hexdigest()


class Run:
    def __init__(self, fmx, torch):
        self.fmx, self.torch, self.out = fmx, torch, {}
        self.FMT = {"u8": fmx.FMX_WB_U8, "s16": fmx.FMX_WB_S16}

    def upload(self, raw, off=0):
        """raw at byte offset `off` of a 256-byte aligned allocation -> (tensor, address)"""
        t = self.torch.zeros(off + raw.nbytes + 64, dtype=self.torch.uint8, device="cuda")
        t[off:off + raw.nbytes] = self.torch.from_numpy(raw.view(np.uint8).copy()).cuda()
        return t, t.data_ptr() + off

    def handle(self, n):
        return self.fmx.Handle(self.fmx.make_config(iq_rate=DSP, dsp_rate=DSP), max(n, 1))

    def wb(self, name, fmt, D, off=0, sample0=None, mode=None):
        fmx, torch = self.fmx, self.torch
        Fs, total = D * DSP, sum(SIZES)
        h = self.handle(NCH)
        w = fmx.Wideband(h, fmx.make_wb_config(Fs, DSP, self.FMT[fmt], 28, max(SIZES)), freqs(Fs, NCH))
        if sample0 is not None:
            w.reset(sample0)
        if mode == "fixed":
            w.set_iq_correction(fmx.FMX_IQC_FIXED, FIXED)
        elif mode == "auto":
            w.set_iq_correction(fmx.FMX_IQC_AUTO, None, 0.25)
        raw = raw_samples(fmt, total * D, 100 + D)
        keep, d_raw = self.upload(raw, off)
        per = 2 * raw.itemsize
        rows = torch.zeros((len(SIZES), NCH, 2 * max(SIZES)), dtype=torch.float32, device="cuda")
        pos = 0
        for i, n in enumerate(SIZES):
            w.process(d_raw + per * D * pos, n, rows[i].data_ptr(), max(SIZES))
            pos += n
        h.sync()
        self.out[name] = sha(rows)
        w.close()
        h.close()

    def wbr(self, Fs, fmt, tpp):
        fmx, torch = self.fmx, self.torch
        P, Q, _ = fmx.wb_ratio(fmx.make_wb_config(Fs, DSP, self.FMT[fmt], tpp, 4096))
        sizes = (Q, 32 * Q)  # one output per phase, then 16 Q 2
        wcfg = fmx.make_wb_config(Fs, DSP, self.FMT[fmt], tpp, max(sizes))
        h = self.handle(NCH)
        w = fmx.Wideband(h, wcfg, freqs(Fs, NCH), rational=True)
        raw = raw_samples(fmt, sum(sizes) // Q * P, 200 + P)
        keep, d_raw = self.upload(raw)
        per = 2 * raw.itemsize
        rows = torch.zeros((len(sizes), NCH, 2 * max(sizes)), dtype=torch.float32, device="cuda")
        pos = 0
        for i, n in enumerate(sizes):
            w.process(d_raw + per * pos, n, rows[i].data_ptr(), max(sizes))
            pos += n // Q * P
        h.sync()
        self.out[f"wbr-{P}_{Q}-{fmt}-tpp{tpp}"] = sha(rows)
        w.close()
        h.close()

    def bank(self, fmt, D, signal=False):
        """three captures of 17, 0 and 5 channels; signal: the bank's records
        at the odd n = 37 over rows of the three alignments instead of the rows"""
        fmx, torch = self.fmx, self.torch
        Fs, total = D * DSP, sum(SIZES)
        owned = [freqs(Fs, 17, 7), [], freqs(Fs, 5, 8)]
        C = 22
        h = self.handle(C)
        b = fmx.WidebandBank(h, fmx.make_wb_config(Fs, DSP, self.FMT[fmt], 28, max(SIZES)), owned)
        wide_stride = total * D + 3
        raw = raw_samples(fmt, 3 * wide_stride, 300 + D)
        keep, d_raw = self.upload(raw)
        per = 2 * raw.itemsize
        if not signal:
            rows = torch.zeros((len(SIZES), C, 2 * max(SIZES)), dtype=torch.float32, device="cuda")
            pos = 0
            for i, n in enumerate(SIZES):
                b.process(d_raw + per * D * pos, wide_stride, n, rows[i].data_ptr(), max(SIZES))
                pos += n
            h.sync()
            self.out[f"bank-{fmt}-D{D}"] = sha(rows)
        else:
            self.records(f"bank_signal-{fmt}-D{D}", h, C,
                         lambda d_rows, stride: b.process(d_raw, wide_stride, SIZES[0], d_rows, stride), b.signal)
        b.close()
        h.close()

    def records(self, name, h, C, process, signal):
        """process into rows whose base is 16-, 8- and 4-byte aligned, then the level records of each call"""
        torch = self.torch
        for align, stride in ((16, 38), (8, 39), (4, 39)):
            buf = torch.zeros(4 + 2 * stride * C + 8, dtype=torch.float32, device="cuda")
            d_rows = buf.data_ptr() + (0 if align == 16 else align)
            assert d_rows % align == 0 and (align == 16 or d_rows % (2 * align))
            lev = torch.zeros(C * LEVEL_BYTES, dtype=torch.uint8, device="cuda")
            process(d_rows, stride)
            signal(lev.data_ptr())
            h.sync()
            self.out[f"{name}-rows{align}"] = sha(lev)

    def wb_signal(self, fmt, D):
        fmx = self.fmx
        Fs, n = D * DSP, SIZES[0]  # odd
        h = self.handle(NCH)
        w = fmx.Wideband(h, fmx.make_wb_config(Fs, DSP, self.FMT[fmt], 28, max(SIZES)), freqs(Fs, NCH))
        keep, d_raw = self.upload(raw_samples(fmt, n * D, 400 + D))
        self.records(f"wb_signal-{fmt}-D{D}", h, NCH, lambda d_rows, stride: w.process(d_raw, n, d_rows, stride),
                     w.signal)
        w.close()
        h.close()

    def scan(self, fmt, D, mode):
        fmx, torch = self.fmx, self.torch
        Fs, n_out, points = D * DSP, 301, 70
        step = Fs // 80
        scfg = fmx.make_wb_scan_config(Fs, DSP, self.FMT[fmt], 28, n_out, -35 * step, step, points)
        h = self.handle(1)
        s = fmx.WidebandScan(h, scfg)
        if mode == "fixed":
            s.set_iq_correction(fmx.FMX_IQC_FIXED, FIXED)
        keep, d_raw = self.upload(raw_samples(fmt, n_out * D, 500 + D))
        lev = torch.zeros((2, points * LEVEL_BYTES), dtype=torch.uint8, device="cuda")
        for i in range(2):  # the second read moves the smoothers
            s.process(d_raw, n_out, lev[i].data_ptr())
        h.sync()
        self.out[f"scan-{fmt}-D{D}-{mode}"] = sha(lev)
        s.close()
        h.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="also write the document to this file")
    a = ap.parse_args()
    import torch
    import fmx
    if not torch.cuda.is_available():
        sys.exit("wb_digest: no GPU")
    r = Run(fmx, torch)
    for fmt in ("u8", "s16"):
        per = 2 if fmt == "u8" else 4  # bytes per wide sample
        for D in (10, 25, 100):
            for mode in ("off", "fixed", "auto"):
                r.wb(f"wb-{fmt}-D{D}-{mode}", fmt, D, mode=None if mode == "off" else mode)
            r.bank(fmt, D)
            for mode in ("off", "fixed"):
                r.scan(fmt, D, mode)
        for mode in ("off", "fixed"):
            r.wb(f"wb-{fmt}-D10-{mode}-offset_one_sample", fmt, 10, off=per, mode=None if mode == "off" else mode)
            r.wb(f"wb-{fmt}-D10-{mode}-offset_half_sample", fmt, 10, off=per // 2, mode=None if mode == "off" else mode)
            r.wb(f"wb-{fmt}-D10-{mode}-counter_2_40", fmt, 10, sample0=(1 << 40) + 12_345,
                 mode=None if mode == "off" else mode)
        r.wb_signal(fmt, 10)
        r.bank(fmt, 10, signal=True)
    for case in RATIONAL:
        r.wbr(*case)
    doc = dict(tool="tools/wb_digest.py", library=fmx.build_info(), device=torch.cuda.get_device_name(0), digests=r.out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
