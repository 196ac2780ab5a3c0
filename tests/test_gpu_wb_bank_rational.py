"""The capture bank at rational rates on the GPU (fmx_wb_bank_create_rational,
kernels k_rbank and k_rbank_hist): many wide captures of
one P / Q plan channelized by one launch, each capture behaving as its own
fmx_wb_create_rational object.

Yardsticks: the single rational objects themselves (fmx_wb_process,
fmx_wb_signal, fmx_wb_process_block on objects of fmx_wb_create_rational --
bit for bit), tests/wb_rational_ref.py's float64 channelizer at the
channelizer's bar (max |d| < 1e-5, tests/test_gpu_wideband.py's WB_TOL), and
fmx_wb_bank_create's bank at Q = 1.
Shapes: captures of 17, 0, 5 and 16 channels (a ragged group, an empty capture,
a short group, a full group; 250 / 3 int16: 17, 0 and 1), calls of Q x (40, 1,
21, 6, 32) outputs, wide_stride = block P / Q + 13 with the padding at full
scale, out_stride = block + 3 inside guard cells.  25 / 3 u8 and int16 (P odd:
element path only), 128 / 15 u8 (15 phases, a_r of mixed parity: both paths in
one launch, three workgroups of tiles), 250 / 3 int16 (one tile per workgroup,
the largest LDS image), 5 / 2 u8 at 12 taps per phase (one K step).
Achieved (profiles/wb_bank_rational_parity_errors.jsonl): rows against
float64, worst channel's max |d|: 25/3 u8 2.4e-7, int16 2.6e-7, 128/15 u8
3.1e-7, 250/3 int16 2.7e-7, 5/2 u8 2.6e-7; against the single objects every
comparison is exact."""
import ctypes as C
import functools

import numpy as np
import pytest

import gpu_harness as H
import wb_rational_ref as RR
import wb_ref as R
import wb_scan_ref as S
from test_gpu_wb_bank import CASES as INT_CASES
from test_gpu_wb_bank import LCOUNTS, PAD, PARAMS3, _bits, _collect, _first, _handle, _same_channels
from test_gpu_wb_bank import _inputs as int_inputs
from test_gpu_wb_bank import run_bank as run_int_bank
from test_gpu_wb_rational import E_FREQ, E_FS, E_N, E_P, E_Q
from test_gpu_wb_receiver import KEYS
from test_gpu_wb_signal import REC, _tones, quantise
from test_gpu_wideband import WB_TOL, _freqs, _log, _raw

pytestmark = pytest.mark.gpu

DSP = 240_000
FMT = {"u8": R.U8, "s16": R.S16}
MULT = (40, 1, 21, 6, 32)  # x Q outputs per call
COUNTS = (17, 0, 5, 16)
CASES = {"25_3-u8": dict(Fs=2_000_000, fmt="u8", tpp=28, counts=COUNTS),
         "25_3-s16": dict(Fs=2_000_000, fmt="s16", tpp=28, counts=COUNTS),
         "128_15-u8": dict(Fs=2_048_000, fmt="u8", tpp=28, counts=COUNTS),
         "250_3-s16": dict(Fs=20_000_000, fmt="s16", tpp=28, counts=(17, 0, 1)),
         "5_2-u8-tpp12": dict(Fs=600_000, fmt="u8", tpp=12, counts=COUNTS)}


def _rfreqs(Fs, counts):
    """Per capture: test_gpu_wideband._freqs' list (0, +-1, 123 457, -Fs / 2 + 1, Fs / 2, random ones), rotated."""
    return [_freqs(Fs, n + 6, seed=11 + s)[s % 3:][:n] for s, n in enumerate(counts)]


@functools.lru_cache(maxsize=None)
def _inputs(case):
    """Distinct full-scale noise per capture, the captures' frequencies and float64 rows."""
    k = CASES[case]
    P, Q = RR.ratio(k["Fs"], DSP)
    raws = [_raw(FMT[k["fmt"]], sum(MULT) * P, 500 + 7 * s + P) for s in range(len(k["counts"]))]
    freqs = _rfreqs(k["Fs"], k["counts"])
    ref = [RR.channelize(R.normalise(r, FMT[k["fmt"]]), P, Q, k["tpp"], k["Fs"], f) if f else None
           for r, f in zip(raws, freqs)]
    return raws, freqs, ref


class Wide:
    """test_gpu_wb_bank.Wide at P / Q: per call [S][wide_stride] samples, row s
    holding capture s's n P / Q samples of that call and full-scale padding
    behind them, wide_stride = block P / Q + 13, at byte offset in_off of a
    sentinel-filled allocation."""

    def __init__(self, torch, fmt, P, Q, block, sizes, raws, in_off=0):
        self.sb = 2 if FMT[fmt] == R.U8 else 4
        self.ws = block * P // Q + PAD
        self.S = len(raws)
        dt, full = (np.uint8, 255) if FMT[fmt] == R.U8 else (np.int16, 32767)
        host = np.full((len(sizes), self.S, 2 * self.ws), full, dtype=dt)
        pos = 0
        for i, n in enumerate(sizes):
            m = n // Q * P
            for s, r in enumerate(raws):
                host[i, s, :2 * m] = r[2 * pos:2 * (pos + m)]
            pos += m
        self.t = torch.full((in_off + host.nbytes + 64,), H.SENTINEL_BYTE, dtype=torch.uint8, device="cuda")
        self.t[in_off:in_off + host.nbytes] = torch.from_numpy(host.view(np.uint8).reshape(-1)).to("cuda")
        self.base = self.t.data_ptr() + in_off

    def ptr(self, call, capture=0):
        return self.base + (call * self.S + capture) * self.ws * self.sb


def _plan(Fs, mult):
    P, Q = RR.ratio(Fs, DSP)
    sizes = [Q * m for m in mult]
    return P, Q, sizes, max(sizes)


def run_rbank(fmx, torch, Fs, fmt, tpp, raws, freqs, mult=MULT, sync="end", in_off=0, events=None, levels=(),
              rational=True):
    """The captures through fmx_wb_bank_process on a bank of
    fmx_wb_bank_create_rational, as test_gpu_wb_bank.run_bank runs the integer
    bank.  -> rows complex64 [C][sum(sizes)], records [len(levels)][C]."""
    P, Q, sizes, block = _plan(Fs, mult)
    Cn, stride = sum(len(f) for f in freqs), block + 3
    h = _handle(fmx, Cn, block)
    bank = fmx.WidebandBank(h, fmx.make_wb_config(Fs, DSP, FMT[fmt], tpp, block), freqs, rational=rational)
    assert bank.consumed(block) == block // Q * P
    wide = Wide(torch, fmt, P, Q, block, sizes, raws, in_off)
    G = H.Guarded(torch, "f32", len(sizes) * Cn, 2 * stride, off=1, tail=21)
    lev = torch.zeros((max(len(levels), 1), Cn * 40), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for i, n in enumerate(sizes):
        if events:
            events(i, bank)
        bank.process(wide.ptr(i), wide.ws, n, G.ptr + 4 * i * Cn * 2 * stride, stride)
        if i in levels:
            bank.signal(lev[list(levels).index(i)].data_ptr())
        if sync == "each":
            h.sync()
    h.sync()
    out = _collect(torch, G, lev if levels else None, sizes, Cn, stride)
    bank.close()
    h.close()
    return out


def run_rsingles(fmx, torch, Fs, fmt, tpp, raws, freqs, mult=MULT, events=None, levels=(), params=None):
    """One fmx_wb_create_rational object per non-empty capture, each fed its row
    of the same device input; events(i, s, wb) before call i of capture s.
    -> per capture (rows, records), None for an empty capture."""
    P, Q, sizes, block = _plan(Fs, mult)
    stride = block + 3
    h = _handle(fmx, 1, block)
    wide = Wide(torch, fmt, P, Q, block, sizes, raws)
    out = []
    for s, f in enumerate(freqs):
        if not f:
            out.append(None)
            continue
        wb = fmx.Wideband(h, fmx.make_wb_config(Fs, DSP, FMT[fmt], tpp, block), f, rational=True)
        if params and params.get(s):
            wb.set_signal_params(*params[s])
        G = H.Guarded(torch, "f32", len(sizes) * len(f), 2 * stride, off=1, tail=21)
        lev = torch.zeros((max(len(levels), 1), len(f) * 40), dtype=torch.uint8, device="cuda")
        for i, n in enumerate(sizes):
            if events:
                events(i, s, wb)
            wb.process(wide.ptr(i, s), n, G.ptr + 4 * i * len(f) * 2 * stride, stride)
            if i in levels:
                wb.signal(lev[list(levels).index(i)].data_ptr())
        h.sync()
        out.append(_collect(torch, G, lev if levels else None, sizes, len(f), stride))
        wb.close()
    h.close()
    return out


@pytest.mark.parametrize("case", list(CASES))
def test_rows_equal_the_single_objects(fmx, torch_cuda, case):
    """Distinct full-scale noise per capture, calls of Q x (40, 1, 21, 6, 32)
    outputs, wide_stride = block P / Q + 13 with the padding at full scale,
    out_stride = block + 3 inside intact guard cells: each capture's rows
    torch.equal those of an fmx_wb_create_rational object fed the same device
    row and are within 1e-5 of float64; the whole input once more at an offset
    of one element (loads element by element) gives identical rows."""
    torch = torch_cuda
    k = CASES[case]
    raws, freqs, ref = _inputs(case)
    args = (fmx, torch, k["Fs"], k["fmt"], k["tpp"], raws, freqs)
    rows, _ = run_rbank(*args)
    off_rows, _ = run_rbank(*args, in_off=1 if k["fmt"] == "u8" else 2)
    single = run_rsingles(*args)
    first = _first(k["counts"])
    Q = RR.ratio(k["Fs"], DSP)[1]
    assert rows.shape == (first[-1], Q * sum(MULT))
    worst = 0.0
    for s in range(len(k["counts"])):
        a, b = first[s], first[s + 1]
        if a == b:
            continue
        assert torch.equal(torch.from_numpy(_bits(rows[a:b]).astype(np.int64)),
                           torch.from_numpy(_bits(single[s][0]).astype(np.int64))), (case, s)
        for c in range(a, b):
            st = _log(f"wb_bank_rational_rows_{case}_cap{s}_f{freqs[s][c - a]}", c, rows[c] - ref[s][c - a], ref[s][c - a])
            worst = max(worst, st["wb_max"])
    print(f"rational bank rows {case}: worst max |d| = {worst:.3g}")
    assert worst < WB_TOL, worst
    assert np.array_equal(_bits(rows), _bits(off_rows))


def test_q1_is_the_integer_bank(fmx, torch_cuda):
    """2.4 MS/s u8 (10 / 1) through fmx_wb_bank_create_rational: every row and
    every level record bit for bit fmx_wb_bank_create's, calls that are no
    multiple of anything (40, 1, 333, 17, 512)."""
    case = "u8_D10"
    k = INT_CASES[case]
    raws, freqs, _ = int_inputs(case)
    want = run_int_bank(fmx, torch_cuda, case, raws, freqs, levels=(1, 4))
    got = run_rbank(fmx, torch_cuda, k["D"] * DSP, k["fmt"], 0, raws, freqs, mult=k["sizes"], levels=(1, 4))
    assert np.array_equal(_bits(got[0]), _bits(want[0])) and got[1].tobytes() == want[1].tobytes()
    # and fmx_wb_bank_create itself still refuses a rate that is no multiple
    h = _handle(fmx, 1, 64)
    w, one, f = C.c_void_p(), (C.c_int * 2)(0, 1), (C.c_int * 1)(0)
    cfg = fmx.make_wb_config(2_048_000, DSP, fmx.FMX_WB_U8, 0, 64)
    assert fmx.lib().fmx_wb_bank_create(h.h, C.byref(cfg), 1, one, f, C.byref(w)) == -1 and not w.value
    h.close()


RESET_AT, RESET_CAP, SAMPLE0, RETUNE_TO = 2, 2, 2 ** 40 + 12345, -654_321
EV_CASE = "25_3-u8"


def _bank_events(i, bank):
    if i == RESET_AT:
        bank.reset(RESET_CAP, SAMPLE0)
        bank.set_freq(_first(COUNTS)[3] + 4, RETUNE_TO)


def _single_events(i, s, wb):
    if i == RESET_AT and s == RESET_CAP:
        wb.reset(SAMPLE0)
    if i == RESET_AT and s == 3:
        wb.set_freq(4, RETUNE_TO)


def test_reset_and_retune_per_capture_queued(fmx, torch_cuda):
    """25 / 3 u8.  Between the queued calls 1 and 2, with no sync anywhere
    before the end: fmx_wb_bank_reset(bank, 2, 2^40 + 12 345) and
    fmx_wb_bank_set_freq (Q = 3 phase rows staged) of channel 4 of capture 3.
    The untouched captures and channels stay bit-identical to the undisturbed
    run; the reset capture and the retuned channel equal single rational
    objects given the same calls, and differ from the undisturbed run from
    call 2 on, not before it.  A sync after every call, one sync at the end and
    a fresh bank give identical rows and records."""
    k = CASES[EV_CASE]
    raws, freqs, _ = _inputs(EV_CASE)
    args = (fmx, torch_cuda, k["Fs"], k["fmt"], k["tpp"], raws, freqs)
    plain, _ = run_rbank(*args)
    runs = [run_rbank(*args, sync=sync, events=_bank_events, levels=(1, 4)) for sync in ("each", "end", "end")]
    for rows, recs in runs[1:]:
        assert np.array_equal(_bits(rows), _bits(runs[0][0]))
        assert recs.tobytes() == runs[0][1].tobytes()
    ev = runs[1][0]
    single = run_rsingles(*args, events=_single_events)
    first = _first(COUNTS)
    tuned = first[3] + 4
    same = [c for c in range(first[-1]) if not (first[2] <= c < first[3]) and c != tuned]
    assert np.array_equal(_bits(ev[same]), _bits(plain[same]))
    assert np.array_equal(_bits(ev[first[2]:first[3]]), _bits(single[2][0]))
    assert np.array_equal(_bits(ev[first[3]:first[4]]), _bits(single[3][0]))
    cut = _first(_plan(k["Fs"], MULT)[2])[RESET_AT]
    for c in list(range(first[2], first[3])) + [tuned]:
        assert np.array_equal(_bits(ev[c, :cut]), _bits(plain[c, :cut])), c
        assert not np.array_equal(_bits(ev[c, cut:]), _bits(plain[c, cut:])), c


L_FS, L_FMT, L_TPP = 2_000_000, "u8", 28
L_FREQS = (0, 123_457, -900_000, L_FS // 2, -L_FS // 2 + 1, 600_000)


@functools.lru_cache(maxsize=None)
def _level_inputs():
    """25 / 3 u8: tones (nothing clipped) with noise of its own per capture; in
    capture 1 alone, bytes 0, 1, 8, 9, 247, 254 and 255 planted in the last
    call's n P / Q samples."""
    P, Q, sizes, _ = _plan(L_FS, MULT)
    total = sum(sizes) // Q * P
    raws = [_tones("u8", total, seed=40 + s, fs=L_FS, freqs=L_FREQS[:5]).copy() for s in range(len(LCOUNTS))]
    for r in raws:
        assert S.clip_ratios(r, R.U8) == (0.0, 0.0)
    last = sizes[-1] // Q * P
    base, pos = total - last, 0
    for bv, cnt in ((0, 3), (1, 5), (8, 7), (9, 11), (247, 13), (254, 2), (255, 9)):
        for _ in range(cnt):
            raws[1][2 * (base + 5 + 15 * pos) + (pos & 1)] = bv
            pos += 1
    assert 5 + 15 * pos < last
    rng = np.random.default_rng(3)
    extra = [int(v) for v in rng.integers(-L_FS // 2, L_FS // 2, 11)]
    return raws, [list(L_FREQS), list(L_FREQS[:5]), [], list(L_FREQS) + extra]


def test_levels_equal_the_single_objects(fmx, torch_cuda):
    """Captures of 6, 5, 0 and 17 channels, fmx_wb_bank_signal behind call 1
    (Q outputs) and call 4 (32 Q outputs), capture 3 with signal parameters
    (12, 0.5, -2, -60, -15): every record equals that of an
    fmx_wb_create_rational object given the same calls and parameters, every
    field.  Clipped samples planted in capture 1's last call only: its ratios
    are clip_ratios' counts over that capture's n P / Q raw samples exactly,
    every other record's are 0 -- the full-scale padding behind the rows is
    never counted.  A second fmx_wb_bank_signal without a new call returns
    FMX_E_INVALID."""
    torch = torch_cuda
    lv = (1, 4)
    raws, freqs = _level_inputs()
    P, Q, sizes, _ = _plan(L_FS, MULT)
    first = _first(LCOUNTS)
    scratch = torch.zeros(first[-1] * 40, dtype=torch.uint8, device="cuda")

    def ev(i, bank):
        if i == 0:
            bank.set_signal_params(3, *PARAMS3)
        if i == 2:  # behind call 1's level call: nothing new to measure
            rc = fmx.lib().fmx_wb_bank_signal(bank.b, C.c_void_p(scratch.data_ptr()))
            assert rc == -1 and b"fmx_wb_bank_signal" in fmx.lib().fmx_last_error(bank.handle.h)
    args = (fmx, torch, L_FS, L_FMT, L_TPP, raws, freqs)
    _, recs = run_rbank(*args, events=ev, levels=lv)
    single = run_rsingles(*args, levels=lv, params={3: PARAMS3})
    start = _first([n // Q * P for n in sizes])
    for s in range(len(LCOUNTS)):
        a, b = first[s], first[s + 1]
        if a == b:
            continue
        assert recs[:, a:b].tobytes() == single[s][1].tobytes(), s
        for j, i in enumerate(lv):
            cr = S.clip_ratios(raws[s][2 * start[i]:2 * start[i + 1]], R.U8)
            assert np.all(recs[j]["hard_clip_ratio"][a:b] == cr[0]) and np.all(recs[j]["near_clip_ratio"][a:b] == cr[1])
            assert (cr != (0.0, 0.0)) == (s == 1 and i == 4), (s, i, cr)
            if s == 1 and i == 4:
                m = start[i + 1] - start[i]
                assert m == 32 * P and round(cr[0] * m) == 3 + 5 + 2 + 9 and round(cr[1] * m) == 3 + 5 + 7 + 13 + 2 + 9


# ---- the band receiver: fmx_wb_bank_process_block at 25 / 3 ----
B, GS = 4096, 8
RX_FREQS = [list(E_FREQ), list(E_FREQ)[::-1]]  # capture B's stations tuned in reverse order


@functools.lru_cache(maxsize=None)
def _captures(n_out):
    """Capture A: the first n_out P / Q samples of test_gpu_wb_rational._band's
    int16 2 MS/s four-station capture (the same synthesis; its float64 rows and
    oracle runs are not needed here).  Capture B: A at half amplitude,
    requantised."""
    import fmx
    n = n_out // E_Q * E_P
    scfg = fmx.make_synth(iq_rate=E_FS, kind=2, n_bits=8192)
    bits, _ = fmx.synth_rds_bits(scfg, R.BAND_CH0, 4)
    iq = fmx.synth_host(scfg, R.BAND_CH0, 4, 0, n, bits)
    i = np.arange(n, dtype=np.int64)
    x = np.zeros(n, np.complex128)
    for c, (f, a) in enumerate(zip(E_FREQ, R.BAND_AMP)):
        turns = ((f % E_FS) * (i % E_FS)) % E_FS
        x += (a / 0.8) * R.normalise(iq[c], R.U8) * np.exp(2j * np.pi * turns / E_FS)
    a = quantise(x * 0.9, "s16")
    return a, np.rint(a.astype(np.float64) * 0.5).astype(np.int16)


def run_rx(fmx, torch, raws, freqs, sizes, bank, generic=False):
    """The captures through fmx_wb_bank_process_block on a rational bank (bank:
    [S][whole capture + 13 samples of full scale], a call's d_wide its first
    sample in row 0) or the one capture through fmx_wb_process_block on an
    fmx_wb_create_rational object, a sync behind every call.
    -> per call dicts as test_gpu_wb_receiver.run_rx's."""
    Cn = sum(len(f) for f in freqs)
    dev = torch.device("cuda")
    h = fmx.Handle(fmx.make_config(iq_rate=DSP, dsp_rate=DSP, block=B, bandwidth_hz=-1, deemphasis=1), Cn)
    wcfg = fmx.make_wb_config(E_FS, DSP, fmx.FMX_WB_S16, 0, B)
    obj = fmx.WidebandBank(h, wcfg, freqs, rational=True) if bank else fmx.Wideband(h, wcfg, freqs[0], rational=True)
    if generic:
        h.diag_set(fmx.FMX_DIAG_FE_GENERIC, 1)
    f = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)  # noqa: E731
    z = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)  # noqa: E731
    T = dict(mpx=f(Cn, B), pcm_l=f(Cn, B), pcm_r=f(Cn, B), clip=f(Cn), count=z(Cn), stereo=z(Cn), pilot=z(Cn),
             indicator=z(Cn), gcount=z(Cn), grp=z(Cn, GS, 4))
    out = fmx.BlockOut(T["mpx"].data_ptr(), B, T["pcm_l"].data_ptr(), T["pcm_r"].data_ptr(), B, T["count"].data_ptr(),
                       T["stereo"].data_ptr(), T["pilot"].data_ptr(), T["clip"].data_ptr(), T["grp"].data_ptr(), GS,
                       T["gcount"].data_ptr(), None, T["indicator"].data_ptr())
    total = sum(sizes) // E_Q * E_P
    ws = total + PAD
    host = np.full((len(raws), 2 * ws), 32767, dtype=np.int16)
    for s, r in enumerate(raws):
        host[s, :2 * total] = r[:2 * total]
    d_raw = torch.from_numpy(host).to(dev)
    torch.cuda.synchronize()
    res, pos = [], 0
    for n in sizes:
        if bank:
            obj.process_block(d_raw.data_ptr() + 4 * pos, ws, n, out)
        else:
            obj.process_block(d_raw.data_ptr() + 4 * pos, n, out)
        h.sync()
        pos += n // E_Q * E_P
        r = {key: T[key].cpu().numpy().copy() for key in KEYS}
        r["mpx"] = r["mpx"][:, :n].copy()
        for c in range(Cn):  # cells past a row's logical length are never written
            r["pcm_l"][c, int(r["count"][c]):] = 0.0
            r["pcm_r"][c, int(r["count"][c]):] = 0.0
            r["grp"][c, min(int(r["gcount"][c]), GS):] = 0
        res.append(r)
    obj.close()
    h.close()
    return res


def _rx_equal(fmx, torch, sizes, generic, tag):
    a, b = _captures(sum(sizes))
    g = run_rx(fmx, torch, [a, b], RX_FREQS, sizes, True, generic)
    wb_a = run_rx(fmx, torch, [a], RX_FREQS[:1], sizes, False, generic)
    wb_b = run_rx(fmx, torch, [b], RX_FREQS[1:], sizes, False, generic)
    assert all(int(r["count"].min()) > 0 for r in g if r["mpx"].shape[1] >= 333)
    _same_channels(tag + " 0-3", g, wb_a, slice(0, 4), slice(0, 4))
    _same_channels(tag + " 4-7", g, wb_b, slice(4, 8), slice(0, 4))


@pytest.mark.parametrize("generic", [False, True], ids=["fecf", "generic"])
def test_band_receiver_equals_the_single_objects(fmx, torch_cuda, generic):
    """The 2 MS/s int16 four-station capture of section 23 (A) and A at half
    amplitude, requantised, tuned in reverse order (B) on one 8-channel stereo
    + RDS handle, 6 calls of 4092 outputs (34 100 wide samples of either row):
    channels 0-3 and 4-7 are bit-identical, every output, to two 4-channel
    handles run through fmx_wb_process_block on fmx_wb_create_rational
    objects, on k_fecf and under FMX_DIAG_FE_GENERIC."""
    _rx_equal(fmx, torch_cuda, [E_N] * 6, generic, "generic" if generic else "fecf")


def test_band_receiver_ragged_on_the_generic_front_end(fmx, torch_cuda):
    """Calls of 4092, 1023, 333, 3 and 1029 outputs under FMX_DIAG_FE_GENERIC:
    the 8 channels equal the two 4-channel handles' outputs."""
    _rx_equal(fmx, torch_cuda, [4092, 1023, 333, 3, 1029], True, "ragged")


def test_arguments(fmx, torch_cuda):
    """n_out that is no multiple of Q (the message names Q), wide_stride <
    n P / Q and the IQ-correction calls return FMX_E_INVALID, n > block
    FMX_E_CAPACITY, a refused ratio (10 MS/s to 256 kHz as int16) FMX_E_INVALID
    at creation; each message names its function.  n = 0 is accepted and does
    nothing."""
    torch = torch_cuda
    L = fmx.lib()
    Fs, P, Q, Cn, blk = 2_000_000, 25, 3, 5, 1026
    h = fmx.Handle(fmx.make_config(iq_rate=DSP, dsp_rate=DSP, block=4096), Cn)
    wcfg = fmx.make_wb_config(Fs, DSP, fmx.FMX_WB_S16, 0, blk)
    bank = fmx.WidebandBank(h, wcfg, [[0, 1000], [], [5, -7, 9]], rational=True)
    ws = blk // Q * P
    d = torch.zeros(3 * 2 * ws + 64, dtype=torch.int16, device="cuda")
    rows = torch.full((Cn * 2 * (blk + 1),), 7.0, dtype=torch.float32, device="cuda")
    f = lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda")  # noqa: E731
    pl, pr, cnt = f(Cn, 4096), f(Cn, 4096), torch.zeros(Cn, dtype=torch.int32, device="cuda")
    good = lambda: fmx.BlockOut(None, 0, pl.data_ptr(), pr.data_ptr(), 4096, cnt.data_ptr(), None, None, None, None, 0,  # noqa: E731
                                None, None, None)
    err = lambda: L.fmx_last_error(h.h)  # noqa: E731
    p, r = C.c_void_p(d.data_ptr()), C.c_void_p(rows.data_ptr())
    for n in (1, 2, 1025):
        assert L.fmx_wb_bank_process(bank.b, p, ws, n, r, blk) == -1
        assert b"fmx_wb_bank_process:" in err() and b"Q = 3" in err()
        assert L.fmx_wb_bank_process_block(bank.b, p, ws, n, C.byref(good())) == -1
        assert b"fmx_wb_bank_process_block:" in err() and b"Q = 3" in err()
    assert L.fmx_wb_bank_process(bank.b, p, ws - 1, blk, r, blk) == -1
    assert b"fmx_wb_bank_process:" in err() and b"wide_stride" in err()
    assert L.fmx_wb_bank_process_block(bank.b, p, 1023 // Q * P - 1, 1023, C.byref(good())) == -1
    assert b"fmx_wb_bank_process_block:" in err() and b"wide_stride" in err()
    assert L.fmx_wb_bank_process(bank.b, p, ws + 50, blk + 3, r, blk + 3) == -4
    assert b"fmx_wb_bank_process:" in err()
    assert L.fmx_wb_bank_process_block(bank.b, p, ws + 50, blk + 3, C.byref(good())) == -4
    assert b"fmx_wb_bank_process_block:" in err()
    fixed = fmx.IqCorrection(0.0, 0.0, 1.0, 0.0)
    assert L.fmx_wb_bank_set_iq_correction(bank.b, -1, fmx.FMX_IQC_FIXED, C.byref(fixed), 0.0) == -1
    assert b"fmx_wb_bank_set_iq_correction:" in err()
    assert L.fmx_wb_bank_set_iq_correction(bank.b, 0, fmx.FMX_IQC_OFF, None, 0.0) == -1
    assert L.fmx_wb_bank_iq_correction(bank.b, 0, C.byref(fixed)) == -1 and b"fmx_wb_bank_iq_correction:" in err()
    # n == 0 is accepted and does nothing: no row is written, nothing to measure
    assert L.fmx_wb_bank_process(bank.b, p, 0, 0, None, 0) == 0
    assert L.fmx_wb_bank_process_block(bank.b, p, ws, 0, C.byref(good())) == 0
    h.sync()
    assert bool((rows == 7.0).all())
    sig = torch.zeros(Cn * 40, dtype=torch.uint8, device="cuda")
    assert L.fmx_wb_bank_signal(bank.b, C.c_void_p(sig.data_ptr())) == -1 and b"fmx_wb_bank_signal" in err()
    bank.process_block(d.data_ptr(), ws, 1026, good())  # and a good call runs: block need not be a multiple of 4
    h.sync()
    assert int(cnt.cpu().numpy().min()) > 0
    bank.close()
    # creation: a refused ratio, the table rules
    bad = C.c_void_p(1)
    one, fr = (C.c_int * 2)(0, 1), (C.c_int * 4)(0, 0, 0, 0)
    big = fmx.make_wb_config(10_000_000, 256_000, fmx.FMX_WB_S16, 0, 64)  # 625 / 16: one tile's int16 window exceeds 80 KB
    assert L.fmx_wb_bank_create_rational(h.h, C.byref(big), 1, one, fr, C.byref(bad)) == -1 and not bad.value
    assert b"fmx_wb_bank_create_rational:" in err() and b"80 KB" in err()
    q17 = fmx.make_wb_config(2_400_001, DSP, fmx.FMX_WB_S16, 0, 64)
    assert L.fmx_wb_bank_create_rational(h.h, C.byref(q17), 1, one, fr, C.byref(bad)) == -1
    assert b"fmx_wb_bank_create_rational:" in err() and b"Q <= 16" in err()
    for table, n in (((1, 2), 1), ((0, 3, 2), 2)):
        t = (C.c_int * len(table))(*table)
        assert L.fmx_wb_bank_create_rational(h.h, C.byref(wcfg), n, t, fr, C.byref(bad)) == -1 and not bad.value
        assert b"fmx_wb_bank_create_rational:" in err()
    out_of_band = (C.c_int * 1)(1_000_001)
    assert L.fmx_wb_bank_create_rational(h.h, C.byref(wcfg), 1, one, out_of_band, C.byref(bad)) == -1
    assert b"fmx_wb_bank_create_rational:" in err()
    h.close()
