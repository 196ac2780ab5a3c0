"""The band scan over a capture bank on the GPU (fmx_wb_bank_scan_*, kernels
k_bscan and k_bscan_level with k_wbb_clip and k_wbb_set_params; DESIGN.md
section 28): [S][wide_stride] captures in, one fmx_signal_level record per
scan point of every capture out.

The standard bank is three captures of 19, 0 and 70 points: a ragged second
wave, an empty capture, and a capture of two work-list entries whose 6-point
tail leaves waves 1 to 3 idle.  Capture 0's points are test_gpu_wb_scan.py's
grid (GEO) for its D, capture 2's the same start at a quarter of the step, and
the captures are coloured as that file colours its own: tones 7 kHz off a few
points, other points in each capture, over noise of RMS 1e-3.

Bar of the float64 comparison: |rms - rms_ref| < 1e-5, test_gpu_wb_scan.py's
RMS_TOL (the RMS of a difference cannot exceed its
maximum, and the rows' bar is max |d| < 1e-5).  Everything else is equality:
of bytes with fmx_wb_scan objects, of clip ratios with integer counts."""
import ctypes as C
import functools

import numpy as np
import pytest

import gpu_harness as H
import wb_bank_scan_ref as B
import wb_ref as R
import wb_scan_ref as S
from test_gpu_parity import log_errors
from test_gpu_wb_scan import CLIP_AMP, DSP, FMT, GEO, REC, RMS_TOL, TONE_AMP, TONE_OFF

pytestmark = pytest.mark.gpu

COUNTS = (19, 0, 70)
# the points the tones sit 7 kHz above, per capture (capture 1 has no points: its row carries tones all the same)
TONES = ((2, 5, 10, 12, 17), (1, 3, 8, 11, 15), (4, 21, 38, 47, 66))
ODD = [-612_345, 17, 250_001]  # a fourth capture that is no grid
PARAMS0, PARAMS2 = (12, 0.5, -2.0, -60.0, -15.0), (30, 0.25, 1.5, -70.0, -10.0)
CASES = [(fmt, D) for fmt in ("u8", "s16") for D in (10, 25, 100)]


def _grids(D):
    """(start, step) of each capture's points."""
    _, start, step = GEO[D]
    return [(start, step), (start, step), (start, step // 4)]


def _freqs(D, counts=COUNTS):
    return [S.points(s0, st, n) for (s0, st), n in zip(_grids(D), counts)]


@functools.lru_cache(maxsize=None)
def _row(fmt, D, cap, n_samples, amps=TONE_AMP, scale=1.0):
    """Interleaved raw I/Q of capture cap's coloured row."""
    Fs = D * DSP
    start, step = _grids(D)[cap]
    rng = np.random.default_rng(100 + cap)
    i = np.arange(n_samples, dtype=np.int64)
    x = (1e-3 / np.sqrt(2.0)) * (rng.normal(size=n_samples) + 1j * rng.normal(size=n_samples))
    for p, a in zip(TONES[cap], amps):
        turns = (((start + p * step + TONE_OFF) % Fs) * (i % Fs)) % Fs
        x += a * np.exp(2j * np.pi * turns / Fs)
    x *= scale
    if FMT[fmt] == R.U8:
        raw = np.empty(2 * n_samples, np.uint8)
        q = lambda v: np.clip(np.rint(v * 127.5 + 127.5), 0, 255)  # noqa: E731
    else:
        raw = np.empty(2 * n_samples, np.int16)
        q = lambda v: np.clip(np.rint(v * 32768.0), -32768, 32767)  # noqa: E731
    raw[0::2], raw[1::2] = q(x.real), q(x.imag)
    raw.setflags(write=False)
    return raw


def _wcfg(fmx, fmt, D, block=4096):
    return fmx.make_wb_config(D * DSP, DSP, FMT[fmt], GEO[D][0], block)


def _device_rows(torch, rows, n_samples, pad=0, in_off=0):
    """[S][n_samples + pad] samples on the device, the base in_off elements
    into its allocation; the padding of every row and what lies before the
    base and behind the last row hold full-scale garbage.  -> (tensor, base
    pointer, wide_stride)."""
    dt = rows[0].dtype
    ws = n_samples + pad
    lim = (0, 255) if dt == np.uint8 else (-32768, 32767)
    rng = np.random.default_rng(9)
    host = rng.choice(lim, in_off + 2 * ws * len(rows) + 64).astype(dt)
    for s, r in enumerate(rows):
        host[in_off + 2 * ws * s:in_off + 2 * ws * s + 2 * n_samples] = r[:2 * n_samples]
    t = torch.from_numpy(host).to(torch.device("cuda"))
    return t, t.data_ptr() + in_off * dt.itemsize, ws


def run_bank_scan(fmx, torch, wcfg, freqs, calls, pad=0, in_off=0, events=None, handle=None):
    """calls: [(rows, n_out)], rows[s] capture s's raw samples (at least
    n_out * D).  events: {k: f(object)} queued ahead of call k, with no
    synchronisation in between.  The records live in a sentinel-guarded
    allocation checked after every call.  -> records [len(calls)][points]."""
    h = handle or fmx.Handle(fmx.make_config(iq_rate=DSP, dsp_rate=DSP), 1)
    bs = fmx.WidebandBankScan(h, wcfg, freqs)
    D = wcfg.wide_rate // wcfg.dsp_rate
    P = bs.n_points
    G = H.Guarded(torch, "i32", 1, P, off=2, tail=21, cell=10)
    out = []
    for k, (rows, n_out) in enumerate(calls):
        t, ptr, ws = _device_rows(torch, rows, n_out * D, pad, in_off)
        G.fill()
        torch.cuda.synchronize()
        if events and k in events:
            events[k](bs)
        bs.process(ptr, ws, n_out, G.ptr)
        h.sync()
        got = G.raw()
        G.check(P, ("call", k, n_out), got)
        out.append(G.view(got)[0].copy().view(REC))
        del t
    bs.close()
    if handle is None:
        h.close()
    return np.stack(out)


def _sizes(D):
    tpp = GEO[D][0]
    return ([4096] if D == 10 else []) + [333, tpp + 17, tpp + 1]


def _calls(fmt, D, sizes, **kw):
    """Each call on its own slice of every capture's row."""
    total = sum(sizes) * D
    rows = [_row(fmt, D, s, total, **kw) for s in range(3)]
    per, pos, out = 2 * D, 0, []
    for n in sizes:
        out.append(([r[per * pos:per * (pos + n)] for r in rows], n))
        pos += n
    return out


_gpu = {}


def _standard(fmx, torch, fmt, D):
    """The standard bank's run in _sizes' calls, once per session."""
    if (fmt, D) not in _gpu:
        _gpu[(fmt, D)] = run_bank_scan(fmx, torch, _wcfg(fmx, fmt, D), _freqs(D), _calls(fmt, D, _sizes(D)))
    return _gpu[(fmt, D)]


@pytest.mark.parametrize("fmt,D", CASES)
def test_levels_against_float64(fmx, torch_cuda, fmt, D):
    """Calls of 333, tpp + 17 and tpp + 1 outputs (and one of 4096 at D = 10)
    on slices of their own: every point's |rms - rms_ref| < 1e-5 against
    wb_scan_ref.scan_call on its capture's row; clip ratios equal its
    capture's integer counts; the captures are coloured, so a row or point
    mix-up shows.  Achieved (worst point and call): u8 D = 10 3.9e-8, D = 25 2.5e-8, D = 100
    8.7e-8; s16 D = 10 3.8e-8, D = 25 4.1e-8, D = 100 5.3e-8
    (profiles/wb_bank_scan_parity_errors.jsonl)."""
    tpp = GEO[D][0]
    freqs = _freqs(D)
    first = B.first_point(freqs)
    got = _standard(fmx, torch_cuda, fmt, D)
    worst = 0.0
    for k, (rows, n) in enumerate(_calls(fmt, D, _sizes(D))):
        want = B.scan_call(rows, FMT[fmt], D, tpp, D * DSP, freqs, n)
        assert len(want) == first[-1] == got.shape[1]
        ref_rms = S.rms_of([w["dbfs"] for w in want])
        err = np.abs(S.rms_of(got[k]["dbfs"]) - ref_rms)
        st = dict(bank_scan_rms_err=float(err.max()), point=int(np.argmax(err)), groups_oracle=[])
        log_errors(f"wb_bank_scan_{fmt}_D{D}_n{n}", int(np.argmax(err)), st)
        worst = max(worst, float(err.max()))
        assert err.max() < RMS_TOL, (k, n, st)
        for s in range(3):
            hard, near = S.clip_ratios(rows[s][:2 * n * D], FMT[fmt])
            sl = slice(first[s], first[s + 1])
            assert np.all(got[k]["hard_clip_ratio"][sl] == hard) and np.all(got[k]["near_clip_ratio"][sl] == near), (k, s)
    print("worst rms error", fmt, D, worst)
    # capture s reads row s: its strongest point is its own loudest tone, not another capture's
    d0 = got[0]["dbfs"]
    assert int(np.argmax(d0[first[0]:first[1]])) == TONES[0][0], d0[first[0]:first[1]]
    # capture 2's points lie a quarter step apart: a tone is in the pass band of up to 4 points either side
    assert abs(int(np.argmax(d0[first[2]:first[3]])) - TONES[2][0]) <= 5, d0[first[2]:first[3]]
    # point 8 of the shared grid carries a tone in row 1 and nothing within two steps in row 0
    assert d0[first[0] + TONES[0][0]] - d0[first[0] + TONES[1][2]] > 20.0


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


@pytest.mark.parametrize("fmt,D", CASES)
def test_records_equal_the_single_objects(fmx, torch_cuda, fmt, D):
    """Every capture against an fmx_wb_scan object on the same handle with the
    same plan and grid, fed that capture's row, over three successive calls
    (333, tpp + 17, 333 outputs: the smoothers move): the 40 bytes of every
    record are equal.  A fourth capture that is no grid (-612 345, 17,
    250 001 Hz): each record equals a one-point scan object's."""
    torch = torch_cuda
    tpp, sizes = GEO[D][0], [333, GEO[D][0] + 17, 333]
    freqs = _freqs(D) + [ODD]
    first = B.first_point(freqs)
    calls = [(rows + [rows[0]], n) for rows, n in _calls(fmt, D, sizes)]  # the odd capture reads a copy of row 0
    h = fmx.Handle(fmx.make_config(iq_rate=DSP, dsp_rate=DSP), 1)
    got = run_bank_scan(fmx, torch, _wcfg(fmx, fmt, D), freqs, calls, handle=h)
    # the single objects: (capture, start, step, points)
    plans = [(s, g[0], g[1], COUNTS[s]) for s, g in enumerate(_grids(D)) if COUNTS[s]] + [(3, f, 1, 1) for f in ODD]
    at = {s: first[s] for s in range(4)}
    for cap, start, step, n_pts in plans:
        sc = fmx.WidebandScan(h, fmx.make_wb_scan_config(D * DSP, DSP, FMT[fmt], tpp, 4096, start, step, n_pts))
        lev = torch.zeros(40 * n_pts, dtype=torch.uint8, device="cuda")
        for k, (rows, n) in enumerate(calls):
            t, ptr, _ = _device_rows(torch, [rows[cap]], n * D)
            sc.process(ptr, n, lev.data_ptr())
            h.sync()
            one = lev.cpu().numpy().view(REC)
            assert _bits(one) == _bits(got[k][at[cap]:at[cap] + n_pts]), (cap, start, k)
            del t
        sc.close()
        at[cap] += n_pts
    h.close()
    assert at[3] == first[4]
    assert np.any(got[1]["level120_smoothed"] != got[1]["level120"])  # the smoothers were in play


@pytest.mark.parametrize("fmt,D", [("u8", 10), ("s16", 10), ("u8", 25), ("s16", 100)])
def test_rows_and_geometry(fmx, torch_cuda, fmt, D):
    """wide_stride = n_out * D + 37 with full-scale garbage in every row's
    padding and behind the last row, the base one element into its allocation
    (the element-load path): the records' bits are those of the tight, aligned
    run.  The guard cells around d_level are checked in every run of this file
    (run_bank_scan)."""
    tpp = GEO[D][0]
    for n in (333, tpp + 1):
        calls = _calls(fmt, D, [n])
        tight = run_bank_scan(fmx, torch_cuda, _wcfg(fmx, fmt, D), _freqs(D), calls)
        padded = run_bank_scan(fmx, torch_cuda, _wcfg(fmx, fmt, D), _freqs(D), calls, pad=37)
        skewed = run_bank_scan(fmx, torch_cuda, _wcfg(fmx, fmt, D), _freqs(D), calls, pad=37, in_off=1)
        assert _bits(padded) == _bits(tight), n
        assert _bits(skewed) == _bits(tight), n


def _expected_level(dbfs, params):
    """compensated_dbfs and level120 of a record from its own dbfs (wb_scan_ref.record's formulas)."""
    gain_db, comp, bias, floor_db, ceil_db = params
    comp_db = dbfs - (float(gain_db) * comp) + bias
    norm = (comp_db - floor_db) / (max(ceil_db, floor_db + 1.0) - floor_db)
    return comp_db, np.clip((norm * 120.0).astype(np.float32), np.float32(0.0), np.float32(120.0))


@pytest.mark.parametrize("fmt", ["u8", "s16"])
def test_clip_and_parameters_per_capture(fmx, torch_cuda, fmt):
    """Four calls of 1024 outputs at D = 10; capture 2's row is driven into
    clipping in the first two.  Call 0 runs on the defaults; sets for captures
    0 and 2 are queued ahead of call 1; capture 0 is reset ahead of call 3.  A
    twin object runs the same calls without the reset."""
    D, n = 10, 1024
    scales = ((1.0, 0.25, 0.5, 1.0), (1.0, 1.0, 1.0, 1.0), (2.0, 2.0, 1.0, 0.25))
    calls = [([_row(fmt, D, s, n * D, amps=CLIP_AMP, scale=scales[s][k]) for s in range(3)], n) for k in range(4)]
    freqs = _freqs(D)
    first = B.first_point(freqs)
    sets = lambda bs: (bs.set_signal_params(0, *PARAMS0), bs.set_signal_params(2, *PARAMS2))  # noqa: E731
    got = run_bank_scan(fmx, torch_cuda, _wcfg(fmx, fmt, D, n), freqs, calls,
                        events={1: sets, 3: lambda bs: bs.reset(capture=0)})
    twin = run_bank_scan(fmx, torch_cuda, _wcfg(fmx, fmt, D, n), freqs, calls, events={1: sets})
    c0, c2 = slice(first[0], first[1]), slice(first[2], first[3])
    for k, (rows, _) in enumerate(calls):
        for s, sl in ((0, c0), (2, c2)):
            b = rows[s].astype(np.int64) if FMT[fmt] == R.U8 else (rows[s].astype(np.int64) >> 8) + 128
            lo, hi = np.minimum(b[0::2], b[1::2]), np.maximum(b[0::2], b[1::2])
            hard, near = int(np.count_nonzero((lo <= 1) | (hi >= 254))), int(np.count_nonzero((lo <= 8) | (hi >= 247)))
            assert np.all(got[k]["hard_clip_ratio"][sl] == hard / float(n * D)), (k, s)
            assert np.all(got[k]["near_clip_ratio"][sl] == near / float(n * D)), (k, s)
            # each capture's own set, from the call behind it on
            params = S.DEFAULT_PARAMS if k == 0 else (PARAMS0 if s == 0 else PARAMS2)
            comp, level = _expected_level(got[k]["dbfs"][sl], params)
            assert np.max(np.abs(got[k]["compensated_dbfs"][sl] - comp)) < 1e-9, (k, s)
            assert np.max(np.abs(got[k]["level120"][sl] - level)) < 1e-3, (k, s)
    assert got[0]["hard_clip_ratio"][c2][0] > 0.0 and got[0]["hard_clip_ratio"][c0][0] == 0.0
    assert got[0]["near_clip_ratio"][c2][0] > got[0]["hard_clip_ratio"][c2][0]
    shift = got[1]["compensated_dbfs"] - got[1]["dbfs"]  # -8 dB on capture 0, -6 dB on capture 2
    assert abs(shift[c0][0] + 8.0) < 1e-9 and abs(shift[c2][0] + 6.0) < 1e-9, (shift[c0][0], shift[c2][0])
    # the reset restarted capture 0's smoothers and nobody else's
    assert _bits(got[:3]) == _bits(twin[:3])
    assert np.all(got[3]["level120_smoothed"][c0] == got[3]["level120"][c0])
    assert np.any(twin[3]["level120_smoothed"][c0] != twin[3]["level120"][c0])
    assert _bits(got[3][c2]) == _bits(twin[3][c2])
    assert np.any(got[3]["level120_smoothed"][c2] != got[3]["level120"][c2])


def test_two_fresh_objects_agree_bit_for_bit(fmx, torch_cuda):
    again = run_bank_scan(fmx, torch_cuda, _wcfg(fmx, "s16", 10), _freqs(10), _calls("s16", 10, _sizes(10)))
    assert _bits(again) == _bits(_standard(fmx, torch_cuda, "s16", 10))


def test_errors(fmx, torch_cuda):
    torch = torch_cuda
    L = fmx.lib()
    h = fmx.Handle(fmx.make_config(iq_rate=DSP, dsp_rate=DSP), 1)
    err = lambda: L.fmx_last_error(h.h)  # noqa: E731
    wcfg = fmx.make_wb_config(block=64)  # int16, D = 10, tpp 28
    freqs = [[-100_000, 0, 100_000], [], [50_000]]
    bs = fmx.WidebandBankScan(h, wcfg, freqs)
    assert bs.first_point == [0, 3, 3, 4] and bs.n_points == 4
    buf = torch.zeros(3 * 4 * 65 * 10, dtype=torch.int16, device="cuda")
    out = torch.zeros(40 * 4 + 8, dtype=torch.uint8, device="cuda")
    p, o, ws = buf.data_ptr(), out.data_ptr(), 650
    proc = L.fmx_wb_bank_scan_process
    assert proc(bs.b, p, ws, 28, o) == -1 and b"fmx_wb_bank_scan_process" in err()   # n_out = tpp
    assert proc(bs.b, p, ws, 65, o) == -4 and b"fmx_wb_bank_scan_process" in err()   # block + 1: FMX_E_CAPACITY
    assert proc(bs.b, p, 639, 64, o) == -1 and b"fmx_wb_bank_scan_process" in err() and b"wide_stride" in err()
    assert proc(bs.b, None, ws, 64, o) == -1 and b"fmx_wb_bank_scan_process" in err()
    assert proc(bs.b, p, ws, 64, None) == -1 and b"fmx_wb_bank_scan_process" in err()
    assert proc(bs.b, p, ws, 64, o + 4) == -1 and b"fmx_wb_bank_scan_process" in err() and b"aligned" in err()
    assert L.fmx_wb_bank_scan_set_signal_params(bs.b, 3, 0, 0.5, -4.0, -55.0, -19.0) == -1
    assert b"fmx_wb_bank_scan_set_signal_params" in err()
    assert L.fmx_wb_bank_scan_reset(bs.b, 3) == -1 and b"fmx_wb_bank_scan_reset" in err()
    h.sync()
    assert not out.cpu().numpy().any()  # nothing was written by the refused calls
    bs.process(p, 640, 64, o)           # and a good call runs
    h.sync()
    assert out.cpu().numpy()[:160].any()

    def create(cfg, first, f):
        obj = C.c_void_p(1)
        rc = L.fmx_wb_bank_scan_create(h.h, C.byref(cfg), len(first) - 1, (C.c_int * len(first))(*first),
                                       (C.c_int * max(len(f), 1))(*f), C.byref(obj))
        assert obj.value is None
        return rc
    assert create(wcfg, [0, 1], [1_200_001]) == -1 and b"fmx_wb_bank_scan_create" in err()   # beyond + wide_rate / 2
    assert create(wcfg, [0, 1], [-1_200_001]) == -1 and b"fmx_wb_bank_scan_create" in err()
    assert create(wcfg, [0, 0, 0], []) == -1 and b"fmx_wb_bank_scan_create" in err()         # 0 points in all
    assert create(wcfg, [0, 8000, 8193], [0] * 8193) == -1 and b"fmx_wb_bank_scan_create" in err()
    assert create(wcfg, [0, 2, 1], [0, 0]) == -1 and b"fmx_wb_bank_scan_create" in err()
    assert create(fmx.make_wb_config(block=28), [0, 1], [0]) == -1 and b"fmx_wb_bank_scan_create" in err()
    # the other kinds of object, and the bank scan handed to their calls
    hc = fmx.Handle(fmx.make_config(), 1)
    wb = fmx.Wideband(hc, fmx.make_wb_config(), [0])
    bank = fmx.WidebandBank(hc, fmx.make_wb_config(), [[0]])
    sc = fmx.WidebandScan(hc, fmx.make_wb_scan_config())
    for other in (wb.w, bank.b, sc.s):
        assert proc(other, p, ws, 64, o) == -1
        assert b"fmx_wb_bank_scan_process" in L.fmx_last_error(hc.h)
    fixed = fmx.IqCorrection(0.0, 0.0, 1.0, 0.0)
    got = fmx.IqCorrection()
    refusals = [("fmx_wb_set_iq_correction", (bs.b, fmx.FMX_IQC_FIXED, C.byref(fixed), 0.0)),
                ("fmx_wb_iq_correction", (bs.b, C.byref(got))),
                ("fmx_wb_scan_set_iq_correction", (bs.b, fmx.FMX_IQC_FIXED, C.byref(fixed), 0.0)),
                ("fmx_wb_scan_iq_correction", (bs.b, C.byref(got))),
                ("fmx_wb_bank_set_iq_correction", (bs.b, -1, fmx.FMX_IQC_FIXED, C.byref(fixed), 0.0)),
                ("fmx_wb_bank_iq_correction", (bs.b, 0, C.byref(got)))]
    for name, args in refusals:
        assert getattr(L, name)(*args) == -1, name
        assert name.encode() in err(), (name, err())
    sc.close()
    bank.close()
    wb.close()
    hc.close()
    bs.close()
    h.close()


def test_a_bank_that_tunes_itself(fmx, torch_cuda):
    """Two u8 captures at 2.4 MS/s, each with two of the synthetic plan's
    stereo + RDS stations (stations 700, 701 at -900 and +200 kHz in capture
    0; 702, 703 at -300 and +700 kHz in capture 1), 23 points at 100 kHz per
    capture: one bank-scan call and fmx_scan_peaks(dbfs[slice], -40, 1) per
    capture return exactly that capture's two offsets; a WidebandBank created
    at the found frequencies, through fmx_demod and fmx_rds over the 24 calls,
    decodes on every channel a group whose error-free block A is 0x1000 + 700
    + station."""
    torch = torch_cuda
    n, D, Fs = R.BAND_N, R.BAND_D, R.BAND_FS
    total = R.BAND_CALLS * n * D
    where = [(-900_000, 200_000), (-300_000, 700_000)]
    amps = [(0.30, 0.25), (0.25, 0.30)]
    scfg = fmx.make_synth(iq_rate=Fs, kind=2, n_bits=8192)
    bits, _ = fmx.synth_rds_bits(scfg, R.BAND_CH0, 4)
    iq = fmx.synth_host(scfg, R.BAND_CH0, 4, 0, total, bits)
    i = np.arange(total, dtype=np.int64)
    rows = []
    for s in range(2):
        x = np.zeros(total, np.complex128)
        for j in range(2):
            turns = ((where[s][j] % Fs) * (i % Fs)) % Fs
            x += (amps[s][j] / 0.8) * R.normalise(iq[2 * s + j], R.U8) * np.exp(2j * np.pi * turns / Fs)
        x *= 0.9
        raw = np.empty(2 * total, np.uint8)
        raw[0::2] = np.clip(np.rint(x.real * 127.5 + 127.5), 0, 255)
        raw[1::2] = np.clip(np.rint(x.imag * 127.5 + 127.5), 0, 255)
        rows.append(raw)
    grid = S.points(-1_100_000, 100_000, 23)
    wcfg = fmx.make_wb_config(Fs, R.BAND_DSP, fmx.FMX_WB_U8, 0, n)
    got = run_bank_scan(fmx, torch, wcfg, [grid, grid], [([r[:2 * n * D] for r in rows], n)])[0]
    found = [[grid[k] for k in fmx.scan_peaks(got["dbfs"][23 * s:23 * (s + 1)], -40.0, 1)] for s in range(2)]
    assert found == [list(w) for w in where], found
    # tune the bank to what the scan found
    Cn = 4
    dev = torch.device("cuda")
    h = fmx.Handle(fmx.make_config(bandwidth_hz=-1, deemphasis=1), Cn)
    bank = fmx.WidebandBank(h, wcfg, found)
    d_raw = torch.from_numpy(np.stack(rows)).to(dev)  # [2][2 * total] bytes: wide_stride = total samples
    GS = 8
    bb = torch.zeros((Cn, 2 * n), dtype=torch.float32, device=dev)
    mpx = torch.zeros((Cn, n), dtype=torch.float32, device=dev)
    grp = torch.zeros((Cn, GS, 4), dtype=torch.int32, device=dev)
    gcnt = torch.zeros(Cn, dtype=torch.int32, device=dev)
    groups = [[] for _ in range(Cn)]
    for k in range(R.BAND_CALLS):
        bank.process(d_raw.data_ptr() + 2 * D * n * k, total, n, bb.data_ptr(), n)
        h.demod(bb.data_ptr(), 2 * n, n, mpx.data_ptr(), n)
        h.rds(mpx.data_ptr(), n, n, grp.data_ptr(), GS, gcnt.data_ptr())
        h.sync()
        for c, g in enumerate(H._groups_of(grp.cpu().numpy(), gcnt.cpu().numpy(), GS)):
            groups[c] += g
    bank.close()
    h.close()
    for c in range(Cn):
        good = [g for g in groups[c] if (g[4] >> 6) == 0]
        assert any(g[0] == 0x1000 + R.BAND_CH0 + c for g in good), (c, groups[c])
