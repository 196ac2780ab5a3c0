"""The rational-rate channelizer on the GPU (fmx_wb_create_rational, kernels
k_wbr and k_wbr_hist): wide_rate / dsp_rate = P / Q,
against the float64 restatement tests/wb_rational_ref.py (pinned on the CPU by
tests/test_wb_rational.py).  Row comparisons hold test_gpu_wideband's WB_TOL
(max |d| < 1e-5, fmx_decimate's bar: the arithmetic is the same); level records
hold test_gpu_wb_signal's bars; the end-to-end band holds test_gpu_parity's.

Cases: 25 / 3 (2 MS/s; P odd, every fragment read element by element) as u8
and int16; 250 / 3 int16 (20 MS/s; a_r = 0, 83, 166 of mixed parity, one tile
per workgroup); 128 / 15 u8 (2.048 MS/s; 15 phases); 5 / 2 u8 at 12 taps per
phase (Lp = 32: one K step).  Calls are Q x (341, 111, 1, 6, 342, 32) outputs:
more than one workgroup, ragged last blocks of 16, a call of one output per
phase.
Achieved (profiles/wb_rational_parity_errors.jsonl): rows, worst channel's
max |d|: 25/3 u8 2.3e-7, int16 3.7e-7, 250/3 int16 2.4e-7, 128/15 u8 3.6e-7,
5/2 u8 3.2e-7; at a first index of 2^40 + 12 345 3.6e-7, retuned 3.0e-7; level
records rms / dB / level120 1.4e-8 / 1.0e-6 / 7.6e-6; the band's worst channel
MPX max 5.9e-6 / RMS 4.6e-7, PCM max 1.0e-5 / RMS 1.1e-6 on either front end."""
import ctypes as C
import functools

import numpy as np
import pytest

import gpu_harness as H
import rds_wave as W
import wb_rational_ref as RR
import wb_ref as R
import wb_scan_ref as S
from test_gpu_wb_receiver import check_channel, oracle_cut
from test_gpu_wb_signal import REC, compare, quantise
from test_gpu_wideband import SIZES as INT_SIZES
from test_gpu_wideband import WB_TOL, _freqs, _log, _raw, run_wb

pytestmark = pytest.mark.gpu

DSP = 240_000
NCH = 19
FMT = {"u8": R.U8, "s16": R.S16}
MULT = (341, 111, 1, 6, 342, 32)  # x Q outputs per call
CASES = [(2_000_000, "u8", 28), (2_000_000, "s16", 28), (20_000_000, "s16", 28), (2_048_000, "u8", 28),
         (600_000, "u8", 12)]
IDS = ["25_3-u8", "25_3-s16", "250_3-s16", "128_15-u8", "5_2-u8-tpp12"]


def run_wbr(fmx, torch, wcfg, freqs, raw, sizes, sample0=None, retunes=None, in_off=0, pad=0):
    """test_gpu_wideband.run_wb for a rational object: a call of n outputs
    consumes n P / Q wide samples.  -> complex64 [len(freqs)][sum(sizes)]."""
    P, Q = RR.ratio(wcfg.wide_rate, wcfg.dsp_rate)
    Cn = len(freqs)
    h = fmx.Handle(fmx.make_config(iq_rate=DSP, dsp_rate=DSP), Cn)
    wb = fmx.Wideband(h, wcfg, freqs, rational=True)
    if sample0 is not None:
        wb.reset(sample0)
    dev = torch.device("cuda")
    t = torch.full((in_off + raw.nbytes + 64,), H.SENTINEL_BYTE, dtype=torch.uint8, device=dev)
    t[in_off:in_off + raw.nbytes] = torch.from_numpy(raw.view(np.uint8).copy()).to(dev)
    per = 2 * raw.itemsize  # bytes per wide sample
    stride = max(sizes) + pad
    G = H.Guarded(torch, "f32", Cn, 2 * stride, off=1 if pad else 0, tail=21 if pad else 0)
    rows, pos = [], 0
    for i, n in enumerate(sizes):
        assert n % Q == 0
        for (c, f) in (retunes or {}).get(i, []):
            wb.set_freq(c, f)
        if pad:
            G.fill()
            torch.cuda.synchronize()
        wb.process(t.data_ptr() + in_off + per * pos, n, G.ptr, stride)
        h.sync()
        raw_out = G.raw()
        if pad:
            G.check(2 * n, ("call", i, n), raw_out)
        rows.append(G.view(raw_out, np.float32)[:, :2 * n].copy().view(np.complex64))
        pos += n // Q * P
    wb.close()
    h.close()
    return np.concatenate(rows, axis=1)


def _sizes(Q):
    return [Q * m for m in MULT]


@functools.lru_cache(maxsize=None)
def _stream(Fs, fmt, tpp):
    """Raw full-scale noise, frequencies and float64 rows of one case."""
    P, Q = RR.ratio(Fs, DSP)
    raw = _raw(FMT[fmt], sum(MULT) * P, 300 + P + Q)
    raw.setflags(write=False)
    freqs = _freqs(Fs)
    return raw, freqs, RR.channelize(R.normalise(raw, FMT[fmt]), P, Q, tpp, Fs, freqs)


_gpu_rows = {}


def _ragged(fmx, torch, Fs, fmt, tpp):
    """The ragged-call GPU run of _stream(Fs, fmt, tpp), once per session."""
    key = (Fs, fmt, tpp)
    if key not in _gpu_rows:
        raw, freqs, _ = _stream(*key)
        Q = RR.ratio(Fs, DSP)[1]
        wcfg = fmx.make_wb_config(Fs, DSP, FMT[fmt], tpp, max(_sizes(Q)))
        _gpu_rows[key] = run_wbr(fmx, torch, wcfg, freqs, raw, _sizes(Q))
    return _gpu_rows[key]


@pytest.mark.parametrize("Fs,fmt,tpp", CASES, ids=IDS)
def test_rows_against_float64(fmx, torch_cuda, Fs, fmt, tpp):
    """19 channels (0, +-1 Hz, 123 457, -Fs/2 + 1, Fs/2 and 13 random ones) of
    full-scale noise in calls of Q x (341, 111, 1, 6, 342, 32) outputs:
    max |d| < 1e-5 against float64 per channel."""
    _, freqs, ref = _stream(Fs, fmt, tpp)
    got = _ragged(fmx, torch_cuda, Fs, fmt, tpp)
    assert got.shape == ref.shape
    P, Q = RR.ratio(Fs, DSP)
    worst = 0.0
    for c in range(NCH):
        st = _log(f"wbr_{P}_{Q}_{fmt}_f{freqs[c]}", c, got[c] - ref[c], ref[c])
        worst = max(worst, st["wb_max"])
    print(f"wbr rows {P}/{Q} {fmt}: worst max |d| = {worst:.3g}")
    assert worst < WB_TOL, worst


@pytest.mark.parametrize("Fs,fmt,tpp", CASES, ids=IDS)
def test_rows_do_not_depend_on_the_call_split(fmx, torch_cuda, Fs, fmt, tpp):
    """The same stream in one call of 833 Q outputs and in the ragged calls, and
    the ragged calls again on a fresh object: bit-identical rows."""
    raw, freqs, _ = _stream(Fs, fmt, tpp)
    Q = RR.ratio(Fs, DSP)[1]
    ragged = _ragged(fmx, torch_cuda, Fs, fmt, tpp)
    one = run_wbr(fmx, torch_cuda, fmx.make_wb_config(Fs, DSP, FMT[fmt], tpp, sum(_sizes(Q))), freqs, raw,
                  [sum(_sizes(Q))])
    again = run_wbr(fmx, torch_cuda, fmx.make_wb_config(Fs, DSP, FMT[fmt], tpp, max(_sizes(Q))), freqs, raw, _sizes(Q))
    assert np.array_equal(ragged.view(np.uint32), one.view(np.uint32))
    assert np.array_equal(ragged.view(np.uint32), again.view(np.uint32))


def test_sample_counter_above_2_40_and_retune(fmx, torch_cuda):
    """25 / 3 int16: fmx_wb_reset(2^40 + 12 345) against float64 evaluated at
    that index, then fmx_wb_set_freq on channels 3 and 17 between calls (Q rows
    staged each): from that call on their rows are those of a float64 channel
    that was always at the new frequency, and every other channel is
    bit-identical to the run without the retune."""
    Fs, s0 = 2_000_000, (1 << 40) + 12_345
    P, Q = 25, 3
    sizes = [Q * 341, Q * 111, Q * 259]
    raw, freqs, _ = _stream(Fs, "s16", 28)
    raw = raw[:2 * P * sum(sizes) // Q]
    wcfg = fmx.make_wb_config(Fs, DSP, fmx.FMX_WB_S16, 28, max(sizes))
    new = {3: -654_321, 17: Fs // 2}
    plain = run_wbr(fmx, torch_cuda, wcfg, freqs, raw, sizes, sample0=s0)
    tuned = run_wbr(fmx, torch_cuda, wcfg, freqs, raw, sizes, sample0=s0, retunes={1: list(new.items())})
    x = R.normalise(raw, R.S16)
    ref = RR.channelize(x, P, Q, 28, Fs, freqs, sample0=s0)
    worst = max(_log("wbr_counter_2_40", c, plain[c] - ref[c], ref[c])["wb_max"] for c in range(NCH))
    assert worst < WB_TOL, worst
    wrong = RR.channelize(x, P, Q, 28, Fs, freqs, sample0=s0 & 0xFFFFFFFF)
    assert np.max(np.abs(wrong[3] - ref[3])) > 0.1  # the check can tell a 32-bit counter
    ref_new = RR.channelize(x, P, Q, 28, Fs, [new[3], new[17]], sample0=s0)
    for j, c in enumerate((3, 17)):
        assert np.array_equal(tuned[c, :sizes[0]].view(np.uint32), plain[c, :sizes[0]].view(np.uint32))
        d = tuned[c, sizes[0]:] - ref_new[j, sizes[0]:]
        assert _log("wbr_retuned", c, d, ref_new[j])["wb_max"] < WB_TOL
    others = [c for c in range(NCH) if c not in new]
    assert np.array_equal(tuned[others].view(np.uint32), plain[others].view(np.uint32))


@pytest.mark.parametrize("Fs,fmt,in_off", [(2_000_000, "u8", 1), (2_000_000, "s16", 2), (20_000_000, "s16", 2)],
                         ids=["25_3-u8", "25_3-s16", "250_3-s16"])
def test_caller_geometry(fmx, torch_cuda, Fs, fmt, in_off):
    """Input one element off its sample alignment (the loads go element by
    element), output rows of stride block + 3 at a base that is only 4-byte
    aligned: the guard cells stay intact and the rows are bit-identical to the
    dense run."""
    raw, freqs, _ = _stream(Fs, fmt, 28)
    Q = RR.ratio(Fs, DSP)[1]
    wcfg = fmx.make_wb_config(Fs, DSP, FMT[fmt], 28, max(_sizes(Q)))
    got = run_wbr(fmx, torch_cuda, wcfg, freqs, raw, _sizes(Q), in_off=in_off, pad=3)
    assert np.array_equal(got.view(np.uint32), _ragged(fmx, torch_cuda, Fs, fmt, 28).view(np.uint32))


def test_refusals(fmx, torch_cuda):
    torch = torch_cuda
    L = fmx.lib()
    h = fmx.Handle(fmx.make_config(iq_rate=DSP, dsp_rate=DSP), 2)
    wcfg = fmx.make_wb_config(2_000_000, DSP, fmx.FMX_WB_S16, 0, 64)
    f = (C.c_int * 2)(0, 1000)
    w = C.c_void_p()
    assert L.fmx_wb_create(h.h, C.byref(wcfg), f, 2, C.byref(w)) == -1 and not w.value  # still no multiple
    assert b"integer multiple" in L.fmx_last_error(h.h)
    one = (C.c_int * 2)(0, 2)
    assert L.fmx_wb_bank_create(h.h, C.byref(wcfg), 1, one, f, C.byref(w)) == -1 and not w.value
    bad = fmx.make_wb_config(2_400_001, DSP, fmx.FMX_WB_S16, 0, 64)
    assert L.fmx_wb_create_rational(h.h, C.byref(bad), f, 2, C.byref(w)) == -1 and not w.value
    assert b"Q <= 16" in L.fmx_last_error(h.h)
    wb = fmx.Wideband(h, wcfg, [0, 1000], rational=True)
    buf = torch.zeros(4 * 66 * 9, dtype=torch.int16, device="cuda")
    out = torch.zeros((2, 2 * 66), dtype=torch.float32, device="cuda")
    for n in (1, 2, 62):
        assert L.fmx_wb_process(wb.w, buf.data_ptr(), n, out.data_ptr(), 66) == -1  # no multiple of Q = 3
        assert b"Q = 3" in L.fmx_last_error(h.h)
    assert L.fmx_wb_process(wb.w, buf.data_ptr(), 66, out.data_ptr(), 66) == -4  # FMX_E_CAPACITY: block is 64
    assert L.fmx_wb_process(wb.w, buf.data_ptr(), 63, out.data_ptr(), 62) == -1  # out_stride < n_out
    assert L.fmx_wb_set_freq(wb.w, 2, 0) == -1 and L.fmx_wb_set_freq(wb.w, 0, 1_000_001) == -1
    wb.process(buf.data_ptr(), 0, out.data_ptr(), 66)
    wb.process(buf.data_ptr(), 63, out.data_ptr(), 66)  # block need not be a multiple of Q
    h.sync()
    wb.close()
    h.close()


def test_q1_is_the_integer_object(fmx, torch_cuda):
    """2.4 MS/s int16 (10 / 1) through fmx_wb_create_rational: every row bit for
    bit fmx_wb_create's, ragged calls that are no multiple of anything."""
    Fs = 2_400_000
    raw = _raw(R.S16, sum(INT_SIZES) * 10, 77)
    freqs = _freqs(Fs)
    wcfg = fmx.make_wb_config(Fs, DSP, fmx.FMX_WB_S16, 28, 4096)
    a = run_wb(fmx, torch_cuda, wcfg, freqs, raw, INT_SIZES)
    b = run_wbr(fmx, torch_cuda, wcfg, freqs, raw, INT_SIZES)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


L_FS, L_P, L_Q, L_TPP = 2_000_000, 25, 3, 28
L_FREQS, L_AMPS = (0, 123_457, -900_000, 600_000), (0.3, 0.1, 0.03)
L_SIZES = [L_Q * 341, L_Q * 111, L_Q * 342]


@functools.lru_cache(maxsize=None)
def _level_input(fmt):
    """The level test's raw capture and its float64 rows."""
    Fs, P = L_FS, L_P
    n_in = sum(L_SIZES) // L_Q * P
    rng = np.random.default_rng(9)
    i = np.arange(n_in, dtype=np.int64)
    x = 1e-3 * (rng.normal(size=n_in) + 1j * rng.normal(size=n_in))
    for f, a in zip(L_FREQS, L_AMPS):
        x += a * np.exp(2j * np.pi * (((f % Fs) * i) % Fs) / Fs)
    raw = quantise(x, fmt)
    lo, hi, nlo, nhi = (0, 255, 8, 247) if fmt == "u8" else (-32768, 32767, -30720 + 100, 30464 + 200)
    base = 2 * (341 * P + 100)  # inside the second call
    for k in range(7):
        raw[base + 34 * k + (k & 1)] = hi if k % 3 else lo
    for k in range(5):
        raw[base + 1000 + 18 * k + (k & 1)] = nhi if k & 1 else nlo
    return raw, RR.channelize(R.normalise(raw, FMT[fmt]), P, L_Q, L_TPP, Fs, list(L_FREQS))


@pytest.mark.parametrize("fmt", ["u8", "s16"])
def test_level_records(fmx, oracle, torch_cuda, fmt):
    """25 / 3: tones of 0.3 / 0.1 / 0.03 at three channels and an empty fourth,
    noise of RMS 1e-3, and clipped samples planted in the raw input (7 hard, 5
    more near, all inside the second call); fmx_wb_signal behind each
    fmx_wb_process call of Q x (341, 111, 342) outputs into rows of an odd
    stride: every record within test_gpu_wb_signal's bars against float64, the
    clip ratios exact over the call's n P / Q raw samples."""
    torch = torch_cuda
    Fs, P, Q, tpp, freqs, sizes = L_FS, L_P, L_Q, L_TPP, L_FREQS, L_SIZES
    raw, y = _level_input(fmt)
    dev = torch.device("cuda")
    Cn = len(freqs)
    h = fmx.Handle(fmx.make_config(iq_rate=DSP, dsp_rate=DSP), Cn)
    wb = fmx.Wideband(h, fmx.make_wb_config(Fs, DSP, FMT[fmt], tpp, max(sizes)), list(freqs), rational=True)
    G = H.Guarded(torch, "i32", 1, Cn, off=2, tail=21, cell=10)
    d_raw = torch.from_numpy(raw.view(np.uint8).copy()).to(dev)
    stride = max(sizes) + 3
    rows = torch.zeros(1 + 2 * stride * Cn + 7, dtype=torch.float32, device=dev)
    pos = opos = 0
    for k, n in enumerate(sizes):
        G.fill()
        torch.cuda.synchronize()
        wb.process(d_raw.data_ptr() + 2 * raw.itemsize * pos, n, rows.data_ptr() + 4, stride)
        wb.signal(G.ptr)
        h.sync()
        got_raw = G.raw()
        G.check(Cn, ("call", k, n), got_raw)
        got = G.view(got_raw)[0][:10 * Cn].copy().view(REC)
        m = n // Q * P
        hard, near = S.clip_ratios(raw[2 * pos:2 * (pos + m)], FMT[fmt])
        pw = np.mean(np.abs(y[:, opos:opos + n]) ** 2, axis=1)
        want = [dict(S.record(p), hard_clip_ratio=hard, near_clip_ratio=near) for p in pw]
        ref_rms = compare(f"wbr_signal_{fmt}_call{k}", got, want)
        # the reference itself: every tuned channel is loud; away from the planted full-scale
        # samples (wideband clicks) the empty one holds the noise and the format's
        # quantisation alone (u8: 1.05e-3 in the channel's 216 kHz)
        assert np.all(ref_rms[:3] >= 1e-2) and (k == 1 or ref_rms[3] < 2e-3), ref_rms
        if k == 1:
            assert round(hard * m) == 7 and round(near * m) == 12, (hard, near, m)
        else:
            assert hard == 0.0 and near == 0.0
        pos += m
        opos += n
    wb.close()
    h.close()


# ---- end to end: four stations in one 2 MS/s capture through fmx_wb_process_block ----
E_FS, E_P, E_Q, E_N, E_CALLS = 2_000_000, 25, 3, 4092, 24
E_FREQ = (-700_000, -300_000, 200_000, 600_000)
GS = 8


@functools.lru_cache(maxsize=None)
def _band():
    """wb_ref.band_capture's stations synthesised at 2 MS/s -> (int16 capture,
    float64 rational rows [4][24 * 4092], the oracle's outputs per station)."""
    import fmx
    import oracle
    n = E_CALLS * E_N // E_Q * E_P
    scfg = fmx.make_synth(iq_rate=E_FS, kind=2, n_bits=8192)
    bits, _ = fmx.synth_rds_bits(scfg, R.BAND_CH0, 4)
    iq = fmx.synth_host(scfg, R.BAND_CH0, 4, 0, n, bits)
    i = np.arange(n, dtype=np.int64)
    x = np.zeros(n, np.complex128)
    for c, (f, a) in enumerate(zip(E_FREQ, R.BAND_AMP)):
        turns = ((f % E_FS) * (i % E_FS)) % E_FS
        x += (a / 0.8) * R.normalise(iq[c], R.U8) * np.exp(2j * np.pi * turns / E_FS)
    raw = quantise(x * 0.9, "s16")
    ref = RR.channelize(R.normalise(raw, R.S16), E_P, E_Q, RR.tpp_rule(E_P, E_Q), E_FS, list(E_FREQ))
    ora = W.pmap(lambda c: oracle_cut(oracle, ref[c].astype(np.complex64), [E_N] * E_CALLS), range(4))
    return raw, ref, ora


@pytest.mark.parametrize("generic", [False, True], ids=["fecf", "generic"])
def test_band_receiver_end_to_end(fmx, oracle, torch_cuda, generic):
    """Stations 700 .. 703 at -700 / -300 / +200 / +600 kHz in one int16 2 MS/s
    capture, 24 calls of 4092 outputs (34 100 wide samples each) through
    fmx_wb_process_block on a 4-channel handle, on k_fecf and under
    FMX_DIAG_FE_GENERIC.  Against the oracle's objects fed the float64 rational
    rows: groups equal call by call with PI 0x1000 + station, stereo flag and
    pilot exact from call 2 on, MPX from output 128 on and PCM from call 2 on
    at test_gpu_parity's bars, for every station."""
    torch = torch_cuda
    raw, ref, ora = _band()
    dev = torch.device("cuda")
    B = 4096
    h = fmx.Handle(fmx.make_config(iq_rate=DSP, dsp_rate=DSP, block=B, bandwidth_hz=-1, deemphasis=1), 4)
    wb = fmx.Wideband(h, fmx.make_wb_config(E_FS, DSP, fmx.FMX_WB_S16, 0, B), list(E_FREQ), rational=True)
    if generic:
        h.diag_set(fmx.FMX_DIAG_FE_GENERIC, 1)
    h.timing_enable(True)
    f = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)  # noqa: E731
    z = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)  # noqa: E731
    T = dict(mpx=f(4, B), pcm_l=f(4, B), pcm_r=f(4, B), clip=f(4), count=z(4), stereo=z(4), pilot=z(4), indicator=z(4),
             gcount=z(4), grp=z(4, GS, 4))
    out = fmx.BlockOut(T["mpx"].data_ptr(), B, T["pcm_l"].data_ptr(), T["pcm_r"].data_ptr(), B, T["count"].data_ptr(),
                       T["stereo"].data_ptr(), T["pilot"].data_ptr(), T["clip"].data_ptr(), T["grp"].data_ptr(), GS,
                       T["gcount"].data_ptr(), None, T["indicator"].data_ptr())
    d_raw = torch.from_numpy(raw).to(dev)
    torch.cuda.synchronize()
    g, per = [], 4 * E_N // E_Q * E_P  # bytes of one call's wide samples
    for i in range(E_CALLS):
        wb.process_block(d_raw.data_ptr() + per * i, E_N, out)
        h.sync()
        r = {k: v.cpu().numpy().copy() for k, v in T.items()}
        r["mpx"] = r["mpx"][:, :E_N].copy()
        r["groups"] = H._groups_of(r["grp"], r["gcount"], GS)
        g.append(r)
    kt = h.kernel_times()
    wb.close()
    h.close()
    assert kt["frontend"][1] == (0 if generic else E_CALLS) and kt["frontend_generic"][1] == (E_CALLS if generic else 0), kt
    sizes = [E_N] * E_CALLS
    ngroups = 0
    for c in range(4):
        ngroups += check_channel("wbr_band_" + ("generic" if generic else "fecf"), c, g, ora[c], sizes,
                                 1.0, pcm_from=2 * E_N, exact_from=2 * E_N,
                                 pi=0x1000 + R.BAND_CH0 + c)
        assert ora[c][-1]["stereo"] == 1, c
    assert ngroups >= 8
