"""The capture bank's DC-offset and IQ-imbalance correction on the GPU
(fmx_wb_bank_set_iq_correction, fmx_wb_bank_iq_correction; kernels k_bank_iqc,
k_bank_iqc_sums, k_bank_iqc_finish, k_bank_iqc_set):
every capture of a bank behaves as an fmx_wb object given the same
fmx_wb_set_iq_correction calls.

Yardsticks: the single objects themselves (rows, read-back, band receiver and
level records -- bit for bit), tests/wb_iq_ref.py's float64 / int64
restatement at the channelizer's bar (max |d| < 1e-5) and the estimator's
(1e-12 relative), and tests/test_wb_iqcorr.py's image bars.
Shapes: tests/test_gpu_wb_bank.py's bank -- captures of 17, 0, 5 and 16
channels, distinct full-scale noise per capture, wide_stride = block D + 13
with the padding at full scale, out_stride = block + 3 inside guard cells,
block 512, calls of 40, 1, 333, 17 and 512 outputs -- as u8 at D = 10 (tpp 28)
and int16 at D = 5 (odd, tpp 20).
Achieved: see the tests' docstrings (profiles/wb_bank_iqcorr_parity_errors.jsonl)."""
import ctypes as C
import functools

import numpy as np
import pytest

import gpu_harness as H
import wb_iq_ref as Q
import wb_ref as R
import wb_scan_ref as S
from test_gpu_wb_bank import COUNTS, PAD, Wide, _bank_freqs, _bits, _collect, _first, _handle
from test_gpu_wb_iqcorr import EST_TOL, FIXED, WB_TOL, _cut, _log, _rel
from test_gpu_wb_receiver import KEYS
from test_gpu_wb_signal import REC
from test_gpu_wideband import _raw
from test_wb_iqcorr import IMAGE_AFTER_DB, IMAGE_BEFORE_DB, image_rejection_reference

pytestmark = pytest.mark.gpu

DSP = 240_000
FMT = {"u8": R.U8, "s16": R.S16}
SIZES = (40, 1, 333, 17, 512)
BLOCK = 512
CASES = {"u8_D10": dict(fmt="u8", D=10, tpp=28), "s16_D5": dict(fmt="s16", D=5, tpp=20)}
FIRST = _first(COUNTS)
START = _first(SIZES)
ALPHA2 = 0.25
FIXED2 = (-0.01, 0.03, 1.05, 0.02)


def _modes(fmx):
    """Per capture (mode, fixed, alpha): FIXED, AUTO (the empty capture; alpha 0: 1 / 16), AUTO 0.25, OFF."""
    return [(fmx.FMX_IQC_FIXED, FIXED, 0.0), (fmx.FMX_IQC_AUTO, None, 0.0), (fmx.FMX_IQC_AUTO, None, ALPHA2),
            (fmx.FMX_IQC_OFF, None, 0.0)]


@functools.lru_cache(maxsize=None)
def _inputs(case):
    """Distinct full-scale noise per capture and the captures' frequencies."""
    k = CASES[case]
    raws = [_raw(FMT[k["fmt"]], sum(SIZES) * k["D"], 500 + 7 * s + k["D"]) for s in range(len(COUNTS))]
    return raws, _bank_freqs(k["D"] * DSP, COUNTS)


def _wcfg(fmx, case, block=BLOCK):
    k = CASES[case]
    return fmx.make_wb_config(k["D"] * DSP, DSP, FMT[k["fmt"]], k["tpp"], block)


def run_bank(fmx, torch, case, raws, freqs, setup=None, events=None, after=None, in_off=0):
    """tests/test_gpu_wb_bank.py's run_bank with setup(bank) behind the
    bank's creation, events(i, bank) before call i and, when given,
    after(i, bank) behind a sync after call i (without it the calls stay
    queued to the end).  -> rows complex64 [C][sum(SIZES)]."""
    k = CASES[case]
    Cn, stride = sum(len(f) for f in freqs), BLOCK + 3
    h = _handle(fmx, Cn, BLOCK)
    bank = fmx.WidebandBank(h, _wcfg(fmx, case), freqs)
    if setup:
        setup(bank)
    wide = Wide(torch, k["fmt"], k["D"], BLOCK, SIZES, raws, in_off)
    G = H.Guarded(torch, "f32", len(SIZES) * Cn, 2 * stride, off=1, tail=21)
    torch.cuda.synchronize()
    for i, n in enumerate(SIZES):
        if events:
            events(i, bank)
        bank.process(wide.ptr(i), wide.ws, n, G.ptr + 4 * i * Cn * 2 * stride, stride)
        if after:
            h.sync()
            after(i, bank)
    h.sync()
    rows, _ = _collect(torch, G, None, SIZES, Cn, stride)
    bank.close()
    h.close()
    return rows


def run_singles(fmx, torch, case, raws, freqs, setup=None, events=None, after=None):
    """One fmx_wb object per capture, fed its row of the bank's device input;
    an empty capture gets an object of one channel, so that its estimator can
    be followed (its rows are not compared).  setup(s, wb), events(i, s, wb),
    after(i, s, wb) as run_bank's.  -> per capture rows [channels][sum(SIZES)]."""
    k = CASES[case]
    stride = BLOCK + 3
    h = _handle(fmx, 1, BLOCK)
    wide = Wide(torch, k["fmt"], k["D"], BLOCK, SIZES, raws)
    out = []
    for s, f in enumerate(freqs):
        f = f or [0]
        wb = fmx.Wideband(h, _wcfg(fmx, case), f)
        if setup:
            setup(s, wb)
        G = H.Guarded(torch, "f32", len(SIZES) * len(f), 2 * stride, off=1, tail=21)
        for i, n in enumerate(SIZES):
            if events:
                events(i, s, wb)
            wb.process(wide.ptr(i, s), n, G.ptr + 4 * i * len(f) * 2 * stride, stride)
            if after:
                h.sync()
                after(i, s, wb)
        h.sync()
        out.append(_collect(torch, G, None, SIZES, len(f), stride)[0])
        wb.close()
    h.close()
    return out


def _set_bank(modes):
    def setup(bank):
        for s, (mode, fixed, alpha) in enumerate(modes):
            bank.set_iq_correction(mode, fixed, alpha, capture=s)
    return setup


def _set_single(modes):
    return lambda s, wb: wb.set_iq_correction(*modes[s])


def _assert_captures_equal(rows, single, tag):
    for s in range(len(COUNTS)):
        a, b = FIRST[s], FIRST[s + 1]
        if a != b:
            assert np.array_equal(_bits(rows[a:b]), _bits(single[s])), (tag, s)


_shared = {}


def _mixed(fmx, torch, case):
    """The bank in the four modes, a sync and a read-back of every capture after every call; once per case."""
    if case not in _shared:
        raws, freqs = _inputs(case)
        seen = {}

        def after(i, bank):
            for s in range(len(COUNTS)):
                seen[i, s] = bank.iq_correction(s)

        rows = run_bank(fmx, torch, case, raws, freqs, setup=_set_bank(_modes(fmx)), after=after)
        rows.setflags(write=False)
        _shared[case] = (rows, seen)
    return _shared[case]


@pytest.mark.parametrize("case", list(CASES))
def test_equals_the_single_objects(fmx, torch_cuda, case):
    """Captures in FIXED (0.02, -0.015, 0.9457, -0.0699), AUTO (the empty
    one), AUTO with alpha 0.25 and OFF: each capture's rows are bit-identical
    to those of an fmx_wb object in the same mode fed the same device row, and
    fmx_wb_bank_iq_correction(s) after every call == that object's read-back,
    every field.  The bank again with every call left queued to the end, with
    the input base one element off its alignment (one byte / one int16), rows
    of stride block + 3 inside intact guard cells throughout: the same bits."""
    torch = torch_cuda
    raws, freqs = _inputs(case)
    modes = _modes(fmx)
    rows, seen = _mixed(fmx, torch, case)
    want = {}
    single = run_singles(fmx, torch, case, raws, freqs, setup=_set_single(modes),
                         after=lambda i, s, wb: want.__setitem__((i, s), wb.iq_correction()))
    _assert_captures_equal(rows, single, case)
    assert seen == want, [(k, seen[k], want[k]) for k in seen if seen[k] != want[k]][:4]
    assert all(seen[i, 3] == Q.IDENTITY and seen[i, 0] == FIXED for i in range(len(SIZES)))
    assert seen[0, 1] != seen[0, 2] and seen[4, 1] != seen[0, 1]  # each capture its own estimate, and it moves
    skew = run_bank(fmx, torch, case, raws, freqs, setup=_set_bank(modes), in_off=1 if CASES[case]["fmt"] == "u8" else 2)
    assert np.array_equal(_bits(rows), _bits(skew))


@pytest.mark.parametrize("case", list(CASES))
def test_against_float64(fmx, torch_cuda, case):
    """The FIXED capture (17 channels) and the AUTO capture with alpha 0.25 (5
    channels) against wb_iq_ref.rows, the AUTO capture's per-call parameters
    from wb_iq_ref.estimate over that capture's n D samples of each call: max
    |d| < 1e-5; both AUTO captures' read-backs after every call within 1e-12
    relative of the reference estimator (the empty capture's at alpha 1 / 16).
    The padding behind every row is at full scale: one padded sample in a sum
    moves E I^2 by 1e-4 relative at the least.
    Achieved (worst channel's max |d|): u8 D = 10 FIXED 2.4e-7, AUTO 2.0e-7;
    int16 D = 5 FIXED 3.3e-7, AUTO 2.2e-7; the read-backs equal the reference
    estimator's exactly (relative error 0 in every field of every call)."""
    k = CASES[case]
    fmt, D, tpp = FMT[k["fmt"]], k["D"], k["tpp"]
    raws, freqs = _inputs(case)
    rows, seen = _mixed(fmx, torch_cuda, case)
    est = {}
    for s, alpha in ((1, 1.0 / 16.0), (2, ALPHA2)):
        state, est[s] = None, []
        for i, call in enumerate(_cut(raws[s], D, SIZES)):
            p, state = Q.estimate(call, fmt, state, alpha)
            est[s].append(p)
            err = _rel(seen[i, s], p)
            print(f"{case} capture {s} call {i}: {seen[i, s]} rel err {err:.3g}")
            assert err <= EST_TOL, (s, i, seen[i, s], p)
    for s, params, tag in ((0, [FIXED] * len(SIZES), "fixed"), (2, est[2], "auto")):
        ref = Q.rows(_cut(raws[s], D, SIZES), fmt, D, tpp, D * DSP, freqs[s], params)
        worst = 0.0
        for c in range(FIRST[s], FIRST[s + 1]):
            r = ref[c - FIRST[s]]
            worst = max(worst, _log(f"wb_bank_iqcorr_{tag}_{case}_f{freqs[s][c - FIRST[s]]}", c, rows[c] - r, r)["wb_max"])
        print(f"{case} {tag}: worst max |d| = {worst:.3g}")
        assert worst < WB_TOL, (tag, worst)
    plain = R.channelize(R.normalise(raws[0], fmt), D, tpp, D * DSP, freqs[0][:1])
    assert np.max(np.abs(plain[0] - rows[0])) > 0.01  # channel 0 of the FIXED capture sits on the DC term: the check can tell


@pytest.mark.parametrize("case", list(CASES))
def test_off_stays_todays_bank(fmx, torch_cuda, case):
    """A bank never set, one set to OFF (every capture, then one), and one
    set to FIXED and back before its first call: bit-identical rows.  Every
    capture FIXED with (0, 0, 1, 0) runs k_bank_iqc and gives rows equal as
    numbers.  The OFF capture of the mixed bank (k_bank_iqc's uncorrected
    epilogue) has the never-set bank's bits."""
    torch = torch_cuda
    raws, freqs = _inputs(case)
    never = run_bank(fmx, torch, case, raws, freqs)

    def off(bank):
        bank.set_iq_correction(fmx.FMX_IQC_OFF)
        bank.set_iq_correction(fmx.FMX_IQC_OFF, capture=2)

    def there_and_back(bank):
        bank.set_iq_correction(fmx.FMX_IQC_FIXED, FIXED, capture=0)
        bank.set_iq_correction(fmx.FMX_IQC_AUTO, capture=3)
        bank.set_iq_correction(fmx.FMX_IQC_OFF, capture=-1)

    assert np.array_equal(_bits(never), _bits(run_bank(fmx, torch, case, raws, freqs, setup=off)))
    assert np.array_equal(_bits(never), _bits(run_bank(fmx, torch, case, raws, freqs, setup=there_and_back)))
    ident = run_bank(fmx, torch, case, raws, freqs, setup=lambda b: b.set_iq_correction(fmx.FMX_IQC_FIXED, Q.IDENTITY))
    assert np.array_equal(ident, never)
    mixed, _ = _mixed(fmx, torch, case)
    assert np.array_equal(_bits(mixed[FIRST[3]:]), _bits(never[FIRST[3]:]))
    assert not np.array_equal(mixed[:FIRST[1]], never[:FIRST[1]])


SAMPLE0, RETUNE_TO = 12345, -654_321


def test_per_capture_ordering(fmx, torch_cuda):
    """u8, D = 10, every call queued with no sync before the end.  The bank
    starts with capture 0 in AUTO (alpha 0.5) and capture 3 in FIXED.  Before
    call 1 capture 2 is set to FIXED; before call 2 capture 0 is reset to
    sample 12345 and channel 4 of capture 3 is retuned; before call 3 capture
    0 is set to AUTO again; before call 4 capture -1 sets every capture to
    FIXED with other parameters.  Every capture equals a single object given
    the same calls at the same points (the retuned channel included: its tap
    sums were restaged), and against the undisturbed bank each capture
    changes from its own event on, not before, the others staying
    bit-identical.  Then with a sync after every call: the reset keeps capture
    0's estimate (read-back unchanged, the next call smooths on from it) and
    setting AUTO again restarts it, both within 1e-12 of the reference."""
    torch = torch_cuda
    case = "u8_D10"
    raws, freqs = _inputs(case)
    tuned = 4
    base = [(fmx.FMX_IQC_AUTO, None, 0.5), (fmx.FMX_IQC_OFF, None, 0.0), (fmx.FMX_IQC_OFF, None, 0.0),
            (fmx.FMX_IQC_FIXED, FIXED, 0.0)]

    def bank_events(i, bank):
        if i == 1:
            bank.set_iq_correction(fmx.FMX_IQC_FIXED, FIXED, capture=2)
        if i == 2:
            bank.reset(0, SAMPLE0)
            bank.set_freq(FIRST[3] + tuned, RETUNE_TO)
        if i == 3:
            bank.set_iq_correction(fmx.FMX_IQC_AUTO, None, 0.5, capture=0)
        if i == 4:
            bank.set_iq_correction(fmx.FMX_IQC_FIXED, FIXED2)

    def single_events(i, s, wb):
        if i == 1 and s == 2:
            wb.set_iq_correction(fmx.FMX_IQC_FIXED, FIXED)
        if i == 2 and s == 0:
            wb.reset(SAMPLE0)
        if i == 2 and s == 3:
            wb.set_freq(tuned, RETUNE_TO)
        if i == 3 and s == 0:
            wb.set_iq_correction(fmx.FMX_IQC_AUTO, None, 0.5)
        if i == 4:
            wb.set_iq_correction(fmx.FMX_IQC_FIXED, FIXED2)

    plain = run_bank(fmx, torch, case, raws, freqs, setup=_set_bank(base))
    ev = run_bank(fmx, torch, case, raws, freqs, setup=_set_bank(base), events=bank_events)
    single = run_singles(fmx, torch, case, raws, freqs, setup=_set_single(base), events=single_events)
    _assert_captures_equal(ev, single, "events")
    # each capture against the undisturbed bank: the same bits before its first event, others from it on
    rest3 = [c for c in range(FIRST[3], FIRST[4]) if c != FIRST[3] + tuned]
    for chans, call in ((range(FIRST[0], FIRST[1]), 2), (range(FIRST[2], FIRST[3]), 1), ([FIRST[3] + tuned], 2), (rest3, 4)):
        chans, cut = list(chans), START[call]
        assert np.array_equal(_bits(ev[chans, :cut]), _bits(plain[chans, :cut])), call
        for c in chans:
            assert not np.array_equal(_bits(ev[c, cut:]), _bits(plain[c, cut:])), (call, c)
    # the estimate across the reset and the restart
    seen = {}

    def after(i, bank):
        seen[i] = bank.iq_correction(0)

    def events_read(i, bank):
        bank_events(i, bank)
        if i == 2:
            seen["kept"] = bank.iq_correction(0)

    run_bank(fmx, torch, case, raws, freqs, setup=_set_bank(base), events=events_read, after=after)
    calls = _cut(raws[0], CASES[case]["D"], SIZES)
    want, state = [], None
    for i in range(3):
        p, state = Q.estimate(calls[i], R.U8, state, 0.5)
        want.append(p)
    want.append(Q.estimate(calls[3], R.U8)[0])  # the restart: the call's estimate alone
    for i in range(4):
        assert _rel(seen[i], want[i]) <= EST_TOL, (i, seen[i], want[i])
    assert seen["kept"] == seen[1] and seen[4] == FIXED2
    assert _rel(want[2], Q.estimate(calls[2], R.U8)[0]) > 1e-6  # call 2 smoothed on: not its own estimate


def _swapped(raw):
    out = np.empty_like(raw)
    out[0::2], out[1::2] = raw[1::2], raw[0::2]
    return out


@pytest.mark.parametrize("fmt", ["s16", "u8"])
def test_image_rejection_of_two_front_ends(fmx, torch_cuda, fmt):
    """Capture A is impaired_capture, capture B the same samples with I and Q
    swapped (another front end: the station lies at -300 kHz, its image at
    +300 kHz, gain 1.0625 for A's 0.9458, the DC components exchanged), both
    with channels at +300 kHz and -300 kHz, D = 10, one call of 9600 outputs.
    The float64 reference meets tests/test_wb_iqcorr.py's conditions for both
    captures (uncorrected between -29 and -25 dB, corrected at most -45 dB);
    each capture's GPU ratio is within 0.5 dB of its reference, with every
    capture in OFF and with both in AUTO (alpha 0), and the read-backs are the
    reference's estimates (1e-12) and differ.
    Achieved, both captures alike: the reference u8 -26.82 -> -49.99 dB, int16
    -26.83 -> -51.74 dB; the GPU u8 -26.82 -> -49.96 dB, int16 -26.83 ->
    -51.68 dB; the read-backs equal the reference's estimates exactly."""
    torch = torch_cuda
    f = FMT[fmt]
    n, D = Q.CAP_N // 10, 10
    raw_a = Q.impaired_capture(f)
    raw_b = _swapped(raw_a)
    freqs = [Q.CAP_STATION_HZ, -Q.CAP_STATION_HZ]
    before_a, after_a, p_a = image_rejection_reference(f)
    p_b, _ = Q.estimate(raw_b, f)
    x = R.normalise(raw_b, f)
    ratio_b = lambda y: Q.image_ratio_db(y[::-1])  # noqa: E731  B's station is the second channel
    before_b = ratio_b(R.channelize(x, D, 28, Q.CAP_FS, freqs))
    after_b = ratio_b(R.channelize(Q.correct(x, p_b), D, 28, Q.CAP_FS, freqs))
    print(f"reference {fmt}: A {before_a:.2f} -> {after_a:.2f} dB {p_a}; B {before_b:.2f} -> {after_b:.2f} dB {p_b}")
    for before, after in ((before_a, after_a), (before_b, after_b)):
        assert IMAGE_BEFORE_DB[0] <= before <= IMAGE_BEFORE_DB[1] and after <= IMAGE_AFTER_DB, (before, after)
    h = fmx.Handle(fmx.make_config(iq_rate=DSP, dsp_rate=DSP), 4)
    ws = n * D + PAD
    host = np.full((2, 2 * ws), 255 if f == R.U8 else 32767, dtype=raw_a.dtype)
    host[0, :2 * n * D], host[1, :2 * n * D] = raw_a, raw_b
    d_raw = torch.from_numpy(host).to("cuda")
    d_out = torch.zeros((4, 2 * n), dtype=torch.float32, device="cuda")
    got = {}
    for mode in (fmx.FMX_IQC_OFF, fmx.FMX_IQC_AUTO):
        bank = fmx.WidebandBank(h, fmx.make_wb_config(Q.CAP_FS, DSP, f, 28, n), [freqs, freqs])
        bank.set_iq_correction(mode, None, 0.0)
        bank.process(d_raw.data_ptr(), ws, n, d_out.data_ptr(), n)
        par = [bank.iq_correction(s) for s in range(2)]
        y = d_out.cpu().numpy().view(np.complex64).astype(np.complex128)
        got[mode] = (Q.image_ratio_db(y[0:2]), ratio_b(y[2:4]), par)
        bank.close()
    h.close()
    (a0, b0, par0), (a1, b1, par1) = got[fmx.FMX_IQC_OFF], got[fmx.FMX_IQC_AUTO]
    print(f"GPU {fmt}: A {a0:.2f} -> {a1:.2f} dB, B {b0:.2f} -> {b1:.2f} dB")
    assert abs(a0 - before_a) < 0.5 and abs(a1 - after_a) < 0.5, (a0, before_a, a1, after_a)
    assert abs(b0 - before_b) < 0.5 and abs(b1 - after_b) < 0.5, (b0, before_b, b1, after_b)
    assert par0 == [Q.IDENTITY, Q.IDENTITY]
    assert _rel(par1[0], p_a) <= EST_TOL and _rel(par1[1], p_b) <= EST_TOL, (par1, p_a, p_b)
    assert par1[0] != par1[1] and abs(par1[0][2] - par1[1][2]) > 0.1


def _receiver(fmx, torch, Cn, n, make, d_wide, call):
    """A stereo + RDS handle of Cn channels and block n, obj = make(handle);
    call(obj, i, input pointer, BlockOut, level pointer) queues call i of two
    and its level call.  -> per call ({key: host array} as
    tests/test_gpu_wb_receiver.py's run_rx prepares them, records [Cn])."""
    dev = torch.device("cuda")
    h = fmx.Handle(fmx.make_config(iq_rate=DSP, dsp_rate=DSP, block=n, bandwidth_hz=-1, deemphasis=1), Cn)
    obj = make(h)
    GS = 8
    f = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)  # noqa: E731
    z = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)  # noqa: E731
    T = dict(mpx=f(Cn, n), pcm_l=f(Cn, n), pcm_r=f(Cn, n), clip=f(Cn), count=z(Cn), stereo=z(Cn), pilot=z(Cn),
             indicator=z(Cn), gcount=z(Cn), grp=z(Cn, GS, 4))
    lev = torch.zeros(Cn * 40, dtype=torch.uint8, device=dev)
    out = fmx.BlockOut(T["mpx"].data_ptr(), n, T["pcm_l"].data_ptr(), T["pcm_r"].data_ptr(), n, T["count"].data_ptr(),
                       T["stereo"].data_ptr(), T["pilot"].data_ptr(), T["clip"].data_ptr(), T["grp"].data_ptr(), GS,
                       T["gcount"].data_ptr(), None, T["indicator"].data_ptr())
    res = []
    for i in range(2):
        call(obj, i, d_wide, out, lev.data_ptr())
        h.sync()
        r = {key: T[key].cpu().numpy().copy() for key in KEYS}
        for c in range(Cn):  # cells past a row's logical length are never written
            r["pcm_l"][c, int(r["count"][c]):] = 0.0
            r["pcm_r"][c, int(r["count"][c]):] = 0.0
            r["grp"][c, min(int(r["gcount"][c]), GS):] = 0
        res.append((r, lev.cpu().numpy().copy().view(REC)))
    obj.close()
    h.close()
    return res


def test_band_receiver_and_levels(fmx, torch_cuda):
    """Two calls of 1024 through fmx_wb_bank_process_block, each followed by
    fmx_wb_bank_signal: capture A (impaired_capture as int16, three samples of
    call 1 driven to full scale) in FIXED, capture B (A with I and Q swapped)
    in OFF, three stations each on a 6-channel stereo + RDS handle.  Every
    output (MPX, PCM, counts, flags, pilot, clip, groups) and every level
    record equals, bit for bit, those of two 3-channel handles whose fmx_wb
    objects were set the same way and run through fmx_wb_process_block and
    fmx_wb_signal.  The clip ratios are those of each capture's raw samples;
    the corrected capture's image channel reads 40 dB below its station."""
    torch = torch_cuda
    n, D = 1024, 10
    freqs = [Q.CAP_STATION_HZ, -Q.CAP_STATION_HZ, 0]
    raw_a = Q.impaired_capture(R.S16)[:2 * D * 2 * n].copy()
    top = np.argsort(raw_a[2 * D * n::2])[-3:]  # call 1's three largest I: the smallest steps to full scale
    raw_a[2 * (D * n + top)] = 32767
    raws = [raw_a, _swapped(raw_a)]
    ws = 2 * n * D + PAD
    host = np.full((2, 2 * ws), 32767, dtype=np.int16)
    for s in range(2):
        host[s, :4 * n * D] = raws[s]
    d_raw = torch.from_numpy(host).to("cuda")
    wcfg = fmx.make_wb_config(Q.CAP_FS, DSP, fmx.FMX_WB_S16, 0, n)

    def make_bank(h):
        bank = fmx.WidebandBank(h, wcfg, [freqs, freqs])
        bank.set_iq_correction(fmx.FMX_IQC_FIXED, FIXED, capture=0)
        return bank

    def bank_call(bank, i, p, out, lev):
        bank.process_block(p + 4 * D * n * i, ws, n, out)
        bank.signal(lev)

    got = _receiver(fmx, torch, 6, n, make_bank, d_raw.data_ptr(), bank_call)
    for s in range(2):
        def make_wb(h):
            wb = fmx.Wideband(h, wcfg, freqs)
            if s == 0:
                wb.set_iq_correction(fmx.FMX_IQC_FIXED, FIXED)
            return wb

        def wb_call(wb, i, p, out, lev):
            wb.process_block(p + 4 * ws * s + 4 * D * n * i, n, out)
            wb.signal(lev)

        want = _receiver(fmx, torch, 3, n, make_wb, d_raw.data_ptr(), wb_call)
        sl = slice(3 * s, 3 * s + 3)
        for i in range(2):
            bad = [key for key in KEYS if not np.array_equal(_bits(got[i][0][key][sl]), _bits(want[i][0][key]))]
            assert not bad, (s, i, bad)
            assert got[i][1][sl].tobytes() == want[i][1].tobytes(), (s, i)
            hard, near = S.clip_ratios(raws[s][2 * D * n * i:2 * D * n * (i + 1)], R.S16)
            assert np.all(got[i][1]["hard_clip_ratio"][sl] == hard) and np.all(got[i][1]["near_clip_ratio"][sl] == near)
            assert (hard > 0.0) == (i == 1), (s, i, hard)
    assert int(got[1][0]["count"].min()) > 0
    db = got[1][1]["dbfs"]
    # A corrected (image -50 dB, the three planted steps of 0.5 add -46 dB of the station in a channel), B (station at
    # -300 kHz, image -27 dB) not
    assert db[0] - db[1] > 35.0 and db[4] - db[3] < 30.0, db


def test_errors(fmx, torch_cuda):
    """FMX_E_INVALID with the function named: a capture outside
    [-1, n_captures), whatever fmx_wb_set_iq_correction refuses, a NULL h_out,
    capture -1 in the read-back, and an object that is not a bank; alpha 0
    and 1 are legal, and alpha is ignored outside AUTO.  The four calls of the
    single object and the scan still refuse a bank."""
    L = fmx.lib()
    h = fmx.Handle(fmx.make_config(iq_rate=DSP, dsp_rate=DSP), 3)
    err = lambda: L.fmx_last_error(h.h)  # noqa: E731
    p = fmx.IqCorrection(0.0, 0.0, 1.0, 0.0)
    out = fmx.IqCorrection()
    bank = fmx.WidebandBank(h, fmx.make_wb_config(block=64), [[0], [], [1000, -1000]])
    setn, getn = b"fmx_wb_bank_set_iq_correction", b"fmx_wb_bank_iq_correction"
    fn = L.fmx_wb_bank_set_iq_correction
    nan = float("nan")
    for cap in (-2, 3, 1 << 20):
        assert fn(bank.b, cap, fmx.FMX_IQC_AUTO, None, 0.5) == -1 and setn in err(), cap
        assert L.fmx_wb_bank_iq_correction(bank.b, cap, C.byref(out)) == -1 and getn in err(), cap
    assert L.fmx_wb_bank_iq_correction(bank.b, -1, C.byref(out)) == -1 and getn in err()
    assert L.fmx_wb_bank_iq_correction(bank.b, 0, None) == -1 and getn in err()
    for cap in (-1, 0, 1):
        assert fn(bank.b, cap, 3, C.byref(p), 0.5) == -1 and setn in err()
        assert fn(bank.b, cap, -1, C.byref(p), 0.5) == -1
        assert fn(bank.b, cap, fmx.FMX_IQC_AUTO, None, -0.1) == -1 and fn(bank.b, cap, fmx.FMX_IQC_AUTO, None, 1.01) == -1
        assert fn(bank.b, cap, fmx.FMX_IQC_AUTO, None, nan) == -1
        assert fn(bank.b, cap, fmx.FMX_IQC_FIXED, None, 0.0) == -1 and setn in err()
        for bad in ((0.0, 0.0, 0.0, 0.0), (0.0, 0.0, -1.0, 0.0), (nan, 0.0, 1.0, 0.0), (0.0, 0.0, 1.0, float("inf"))):
            assert fn(bank.b, cap, fmx.FMX_IQC_FIXED, C.byref(fmx.IqCorrection(*bad)), 0.0) == -1, bad
    assert all(bank.iq_correction(s) == Q.IDENTITY for s in range(3))  # nothing took effect
    for cap in (-1, 1, 2):
        assert fn(bank.b, cap, fmx.FMX_IQC_AUTO, None, 0.0) == 0 and fn(bank.b, cap, fmx.FMX_IQC_AUTO, None, 1.0) == 0
        assert fn(bank.b, cap, fmx.FMX_IQC_FIXED, C.byref(p), 7.0) == 0  # alpha is ignored outside AUTO
        assert fn(bank.b, cap, fmx.FMX_IQC_OFF, None, 0.0) == 0
    bank.set_iq_correction(fmx.FMX_IQC_FIXED, FIXED, capture=1)  # the empty capture
    assert [bank.iq_correction(s) for s in range(3)] == [Q.IDENTITY, FIXED, Q.IDENTITY]
    # the single object's and the scan's calls on a bank, and the bank's on them
    for name in ("fmx_wb_set_iq_correction", "fmx_wb_scan_set_iq_correction"):
        assert getattr(L, name)(bank.b, fmx.FMX_IQC_AUTO, None, 0.5) == -1 and name.encode() in err()
    for name in ("fmx_wb_iq_correction", "fmx_wb_scan_iq_correction"):
        assert getattr(L, name)(bank.b, C.byref(out)) == -1 and name.encode() in err()
    wb = fmx.Wideband(h, fmx.make_wb_config(block=64), [0, 1000])
    sc = fmx.WidebandScan(h, fmx.make_wb_scan_config(block=64))
    for obj in (wb.w, sc.s):
        assert fn(obj, 0, fmx.FMX_IQC_OFF, None, 0.0) == -1 and setn in err()
        assert L.fmx_wb_bank_iq_correction(obj, 0, C.byref(out)) == -1 and getn in err()
    sc.close()
    wb.close()
    bank.close()
    h.close()
