"""The bank scan's DC-offset and IQ-imbalance correction on the GPU
(fmx_wb_bank_scan_set_iq_correction, fmx_wb_bank_scan_iq_correction; kernel
k_scan_bank_iqc with the bank's k_bank_iqc_sums, k_bank_iqc_finish and
k_bank_iqc_set): every capture of a bank scan behaves as
an fmx_wb_scan object given the same fmx_wb_scan_set_iq_correction calls.

Yardsticks: the single scan objects themselves (records and read-backs, bit
for bit), tests/wb_bank_scan_iq_ref.py's float64 / int64 restatement at
tests/test_gpu_wb_scan.py's bar (|rms - rms_ref| < 1e-5) and the estimator's
(1e-12 relative), and fmx_scan_peaks on three impaired front ends.
Shapes: tests/test_gpu_wb_bank_scan.py's bank of 19, 0 and 70 points with its
coloured rows and grids, as u8 and int16 at D = 10, 25 (odd, tpp 12) and 100,
in reads of 333, tpp + 17 and tpp + 1 outputs: a ragged wave, an empty
capture, a two-entry capture with idle waves, a one-output read and the odd-D
element path.  d_level lies between guard cells in every run of this file.
Achieved: see the tests' docstrings (profiles/wb_bank_scan_iqcorr_parity_errors.jsonl)."""
import ctypes as C

import numpy as np
import pytest

import gpu_harness as H
import wb_bank_scan_iq_ref as BQ
import wb_bank_scan_ref as B
import wb_iq_ref as Q
import wb_ref as R
import wb_scan_ref as S
from test_gpu_parity import log_errors
from test_gpu_wb_bank_scan import CASES, COUNTS, ODD, _bits, _calls, _device_rows, _freqs, _grids, _wcfg
from test_gpu_wb_iqcorr import EST_TOL, FIXED, _rel
from test_gpu_wb_scan import DSP, FMT, GEO, REC, RMS_TOL

pytestmark = pytest.mark.gpu

ALPHA2 = 0.25
FIXED3 = (-0.01, 0.03, 1.05, 0.02)  # the off-grid capture's


def _sizes(D):
    return [333, GEO[D][0] + 17, GEO[D][0] + 1]


def _modes(fmx):
    """Per capture (mode, fixed, alpha): FIXED, AUTO (the empty capture; alpha 0: 1 / 16), AUTO 0.25, FIXED (off grid)."""
    return [(fmx.FMX_IQC_FIXED, FIXED, 0.0), (fmx.FMX_IQC_AUTO, None, 0.0), (fmx.FMX_IQC_AUTO, None, ALPHA2),
            (fmx.FMX_IQC_FIXED, FIXED3, 0.0)]


def _set_all(modes):
    def setup(bs):
        for s, (mode, fixed, alpha) in enumerate(modes):
            bs.set_iq_correction(mode, fixed, alpha, capture=s)
    return setup


def run_bscan(fmx, torch, wcfg, freqs, calls, events=None, after=None, pad=0, in_off=0, handle=None):
    """calls: [(rows, n_out)], rows[s] capture s's raw samples (at least
    n_out * D).  events: {k: f(object)} queued ahead of read k; after(k,
    object) runs behind a sync after read k -- without it nothing
    synchronises before the last read is queued.  Every read writes a row of
    its own in one guarded allocation (two guard cells between the rows).
    -> records [len(calls)][points]."""
    h = handle or fmx.Handle(fmx.make_config(iq_rate=DSP, dsp_rate=DSP), 1)
    bs = fmx.WidebandBankScan(h, wcfg, freqs)
    D = wcfg.wide_rate // wcfg.dsp_rate
    P = bs.n_points
    G = H.Guarded(torch, "i32", len(calls), P + 2, off=2, tail=21, cell=10)
    inputs = [_device_rows(torch, rows, n_out * D, pad, in_off) for rows, n_out in calls]
    torch.cuda.synchronize()
    for k, (_, n_out) in enumerate(calls):
        if events and k in events:
            events[k](bs)
        bs.process(inputs[k][1], inputs[k][2], n_out, G.ptr + 40 * (P + 2) * k)
        if after:
            h.sync()
            after(k, bs)
    h.sync()
    got = G.raw()
    G.check(P, "bank scan", got)
    out = np.stack([G.view(got)[k][:10 * P].copy().view(REC) for k in range(len(calls))])
    bs.close()
    if handle is None:
        h.close()
    del inputs
    return out


def run_scan_object(fmx, torch, h, fmt, D, start, step, n_pts, calls, setup=None, events=None, after=None):
    """One fmx_wb_scan object on handle h over calls [(row, n_out)], with
    setup(object), events {k: f(object)} and after(k, object) as run_bscan's.
    -> records [len(calls)][n_pts]."""
    sc = fmx.WidebandScan(h, fmx.make_wb_scan_config(D * DSP, DSP, FMT[fmt], GEO[D][0], 4096, start, step, n_pts))
    if setup:
        setup(sc)
    G = H.Guarded(torch, "i32", len(calls), n_pts + 2, off=2, tail=21, cell=10)
    inputs = [_device_rows(torch, [row], n * D) for row, n in calls]
    torch.cuda.synchronize()
    for k, (_, n) in enumerate(calls):
        if events and k in events:
            events[k](sc)
        sc.process(inputs[k][1], n, G.ptr + 40 * (n_pts + 2) * k)
        if after:
            h.sync()
            after(k, sc)
    h.sync()
    got = G.raw()
    G.check(n_pts, "scan object", got)
    out = np.stack([G.view(got)[k][:10 * n_pts].copy().view(REC) for k in range(len(calls))])
    sc.close()
    del inputs
    return out


def _four(fmt, D, sizes):
    """The standard bank's three captures and the off-grid fourth, which reads a copy of row 0."""
    return _freqs(D) + [ODD], [(rows + [rows[0]], n) for rows, n in _calls(fmt, D, sizes)]


_shared = {}


def _run_mixed(fmx, torch, fmt, D, handle=None):
    """The four captures in _modes over _sizes' reads, a sync and a read-back of every capture after every read.
    -> (records [reads][points], {(read, capture): read-back})."""
    freqs, calls = _four(fmt, D, _sizes(D))
    seen = {}

    def after(k, bs):
        for s in range(4):
            seen[k, s] = bs.iq_correction(s)

    got = run_bscan(fmx, torch, _wcfg(fmx, fmt, D), freqs, calls, events={0: _set_all(_modes(fmx))}, after=after,
                    handle=handle)
    got.setflags(write=False)
    return got, seen


def _mixed(fmx, torch, fmt, D):
    """_run_mixed on a handle of its own, once per case."""
    if (fmt, D) not in _shared:
        _shared[fmt, D] = _run_mixed(fmx, torch, fmt, D)
    return _shared[fmt, D]


@pytest.mark.parametrize("fmt,D", CASES)
def test_equals_the_single_objects(fmx, torch_cuda, fmt, D):
    """Capture 0 in FIXED (0.02, -0.015, 0.9457, -0.0699), capture 1 (empty)
    in AUTO with alpha 0, capture 2 in AUTO with alpha 0.25, over three
    successive reads (333, tpp + 17, tpp + 1 outputs: the smoothed moments and
    the level smoothers move): the 40 bytes of every record equal those of an
    fmx_wb_scan object on the same handle with the same plan and grid, set the
    same way and fed the capture's row, and fmx_wb_bank_scan_iq_correction(s)
    after every read equals that object's read-back in all four doubles -- the
    empty capture's that of a one-point object fed its row.  A fourth capture
    at -612 345, 17 and 250 001 Hz in FIXED: each record equals a one-point
    object's."""
    torch = torch_cuda
    freqs, calls = _four(fmt, D, _sizes(D))
    first = B.first_point(freqs)
    modes = _modes(fmx)
    h = fmx.Handle(fmx.make_config(iq_rate=DSP, dsp_rate=DSP), 1)
    got, seen = _run_mixed(fmx, torch, fmt, D, handle=h)
    again, seen_again = _mixed(fmx, torch, fmt, D)  # a fresh object on another handle: the same bits
    assert _bits(again) == _bits(got) and seen_again == seen
    # the single objects: (capture, start, step, points, compared)
    grids = _grids(D)
    plans = [(0, grids[0][0], grids[0][1], COUNTS[0], True), (1, grids[1][0], grids[1][1], 1, False),
             (2, grids[2][0], grids[2][1], COUNTS[2], True)] + [(3, f, 1, 1, True) for f in ODD]
    at = {s: first[s] for s in range(4)}
    for cap, start, step, n_pts, compared in plans:
        want = {}
        one = run_scan_object(fmx, torch, h, fmt, D, start, step, n_pts, [(rows[cap], n) for rows, n in calls],
                              setup=lambda sc: sc.set_iq_correction(*modes[cap]),
                              after=lambda k, sc: want.__setitem__(k, sc.iq_correction()))
        for k in range(len(calls)):
            assert seen[k, cap] == want[k], (cap, k, seen[k, cap], want[k])
            if compared:
                assert _bits(one[k]) == _bits(got[k][at[cap]:at[cap] + n_pts]), (cap, start, k)
        at[cap] += n_pts if compared else 0
    h.close()
    assert at[0] == first[1] and at[2] == first[3] and at[3] == first[4]
    assert all(seen[k, 0] == FIXED and seen[k, 3] == FIXED3 for k in range(3))
    assert seen[0, 1] != seen[0, 2] and seen[2, 1] != seen[0, 1] and seen[2, 2] != seen[0, 2]  # own estimates, and they move
    assert np.any(got[1]["level120_smoothed"] != got[1]["level120"])  # the level smoothers were in play


@pytest.mark.parametrize("fmt,D", CASES)
def test_against_float64(fmx, torch_cuda, fmt, D):
    """The same run against wb_bank_scan_iq_ref.scan_call: capture 0 and the
    off-grid capture with their FIXED parameters, capture 2 with the reference
    estimator's parameters of each read (wb_iq_ref.estimate over the capture's
    n_out D samples, smoothed at 0.25): |rms - rms_ref| < 1e-5 at every point,
    clip ratios equal the rows' integer counts, and both AUTO captures'
    read-backs (the empty capture's at alpha 1 / 16) within 1e-12 relative of
    the reference estimator.
    Achieved (worst point and read): u8 D = 10 7.5e-8, D = 25 2.5e-8, D = 100
    5.3e-8; int16 D = 10 3.2e-8, D = 25 4.8e-8, D = 100 7.4e-8; the read-backs
    equal the reference estimator's exactly (relative error 0 in every field
    of every read) (profiles/wb_bank_scan_iqcorr_parity_errors.jsonl)."""
    tpp = GEO[D][0]
    f = FMT[fmt]
    freqs, calls = _four(fmt, D, _sizes(D))
    first = B.first_point(freqs)
    got, seen = _mixed(fmx, torch_cuda, fmt, D)
    states, alphas = [None] * 4, [1.0, 1.0 / 16.0, ALPHA2, 1.0]
    worst, worst_est = 0.0, 0.0
    for k, (rows, n) in enumerate(calls):
        est, states = BQ.estimates(rows, f, D, n, states, alphas)
        for s in (1, 2):
            err = _rel(seen[k, s], est[s])
            worst_est = max(worst_est, err)
            assert err <= EST_TOL, (s, k, seen[k, s], est[s])
        ps = [FIXED, est[1], est[2], FIXED3]
        want = BQ.scan_call(rows, f, D, tpp, D * DSP, freqs, n, ps)
        assert len(want) == first[-1] == got.shape[1]
        err = np.abs(S.rms_of(got[k]["dbfs"]) - S.rms_of([w["dbfs"] for w in want]))
        st = dict(bank_scan_iqc_rms_err=float(err.max()), point=int(np.argmax(err)), groups_oracle=[])
        log_errors(f"wb_bank_scan_iqcorr_{fmt}_D{D}_n{n}", int(np.argmax(err)), st)
        worst = max(worst, float(err.max()))
        assert err.max() < RMS_TOL, (k, n, st)
        for s in range(4):
            hard, near = S.clip_ratios(rows[s][:2 * n * D], f)
            sl = slice(first[s], first[s + 1])
            assert np.all(got[k]["hard_clip_ratio"][sl] == hard) and np.all(got[k]["near_clip_ratio"][sl] == near), (k, s)
    print(f"worst rms error {fmt} D = {D}: {worst:.3g}; worst read-back error {worst_est:.3g}")
    # the check can tell: uncorrected, capture 0's point at 0 Hz (D = 10: point 9) reads the FIXED set's DC term away
    if D == 10:
        rows, n = calls[0]
        plain = B.scan_call(rows[:3], f, D, tpp, D * DSP, freqs[:3], n)
        assert abs(S.rms_of([plain[9]["dbfs"]])[0] - S.rms_of(got[0]["dbfs"][9:10])[0]) > 100 * RMS_TOL


@pytest.mark.parametrize("fmt,D", CASES)
def test_off_stays_todays_object(fmx, torch_cuda, fmt, D):
    """An object never set, one set to OFF (every capture, then one), one set
    to FIXED and AUTO and back to OFF before its first read: bit-identical
    records everywhere.  One with capture 2 in FIXED and captures 0 and 1 in
    OFF: capture 0 has the uncorrected bits (k_scan_bank_iqc's uncorrected
    epilogue) and capture 2 has not.  FIXED with the identity in every capture
    gives the uncorrected records bit for bit."""
    torch = torch_cuda
    calls = _calls(fmt, D, _sizes(D)[:2])
    freqs = _freqs(D)
    first = B.first_point(freqs)
    run = lambda setup=None: run_bscan(fmx, torch, _wcfg(fmx, fmt, D), freqs, calls,  # noqa: E731
                                       events={0: setup} if setup else None)
    never = run()

    def off(bs):
        bs.set_iq_correction(fmx.FMX_IQC_OFF)
        bs.set_iq_correction(fmx.FMX_IQC_OFF, capture=2)

    def there_and_back(bs):
        bs.set_iq_correction(fmx.FMX_IQC_FIXED, FIXED, capture=0)
        bs.set_iq_correction(fmx.FMX_IQC_AUTO, capture=2)
        bs.set_iq_correction(fmx.FMX_IQC_OFF, capture=-1)

    def one_fixed(bs):
        bs.set_iq_correction(fmx.FMX_IQC_FIXED, FIXED, capture=2)
        bs.set_iq_correction(fmx.FMX_IQC_OFF, capture=0)
        bs.set_iq_correction(fmx.FMX_IQC_OFF, capture=1)

    assert _bits(run(off)) == _bits(never)
    assert _bits(run(there_and_back)) == _bits(never)
    mixed = run(one_fixed)
    c0, c2 = slice(first[0], first[1]), slice(first[2], first[3])
    assert _bits(mixed[:, c0]) == _bits(never[:, c0])
    assert np.any(mixed[:, c2]["dbfs"] != never[:, c2]["dbfs"])
    ident = run(lambda bs: bs.set_iq_correction(fmx.FMX_IQC_FIXED, Q.IDENTITY))
    assert _bits(ident) == _bits(never)


@pytest.mark.parametrize("fmt,D", [("u8", 10), ("s16", 10), ("u8", 25), ("s16", 100)])
def test_rows_and_geometry(fmx, torch_cuda, fmt, D):
    """wide_stride = n_out * D + 37 with full-scale garbage in every row's
    padding and behind the last row, and the base one element into its
    allocation (the element-load path), against the tight, aligned run: the
    same bits with every capture in FIXED, and with every capture in AUTO the
    same read-backs and the same bits -- one padded sample in an estimator's
    sum moves E I^2 by 1e-4 relative at the least."""
    torch = torch_cuda
    tpp = GEO[D][0]
    freqs = _freqs(D)
    for mode, fixed in ((fmx.FMX_IQC_FIXED, FIXED), (fmx.FMX_IQC_AUTO, None)):
        for n in (333, tpp + 1):
            calls = _calls(fmt, D, [n])
            runs = []
            for pad, in_off in ((0, 0), (37, 0), (37, 1)):
                seen = {}
                rec = run_bscan(fmx, torch, _wcfg(fmx, fmt, D), freqs, calls, pad=pad, in_off=in_off,
                                events={0: lambda bs: bs.set_iq_correction(mode, fixed, 0.0)},
                                after=lambda k, bs: seen.update({s: bs.iq_correction(s) for s in range(3)}))
                runs.append((rec, seen))
            for rec, seen in runs[1:]:
                assert _bits(rec) == _bits(runs[0][0]), (mode, n)
                assert seen == runs[0][1], (mode, n, seen, runs[0][1])
            if mode == fmx.FMX_IQC_AUTO:
                for s in range(3):
                    p, _ = Q.estimate(calls[0][0][s][:2 * n * D], FMT[fmt])
                    assert _rel(runs[0][1][s], p) <= EST_TOL, (s, n, runs[0][1][s], p)


@pytest.mark.parametrize("fmt", ["u8", "s16"])
def test_per_capture_ordering(fmx, torch_cuda, fmt):
    """D = 10, four reads of 333 outputs.  Without a sync before the end: the
    object starts with capture 0 in AUTO (alpha 0.5); a FIXED set for capture
    2 queued between reads 0 and 1 changes capture 2 from read 1 on, not read
    0, and no other capture's bits.  Then with a sync after every read:
    setting capture 2 to AUTO again before read 2 restarts its estimate (the
    read-back is that read's own estimate) while capture 0's smoothed sequence
    equals an uninterrupted twin's; fmx_wb_bank_scan_reset and
    fmx_wb_bank_scan_set_signal_params before read 3 leave the estimates alone
    (the read-back before read 3 is read 2's, and read 3 smooths on from it)."""
    torch = torch_cuda
    D, f = 10, FMT[fmt]
    calls = _calls(fmt, D, [333] * 4)
    freqs = _freqs(D)
    first = B.first_point(freqs)
    c2 = slice(first[2], first[3])
    start = lambda bs: (bs.set_iq_correction(fmx.FMX_IQC_AUTO, None, 0.5, capture=0),  # noqa: E731
                        bs.set_iq_correction(fmx.FMX_IQC_AUTO, None, 0.5, capture=2))
    run = lambda events, after=None: run_bscan(fmx, torch, _wcfg(fmx, fmt, D), freqs, calls[:len(events)],  # noqa: E731
                                               events=events, after=after)
    plain = run({0: lambda bs: bs.set_iq_correction(fmx.FMX_IQC_AUTO, None, 0.5, capture=0), 1: lambda bs: None})
    ev = run({0: lambda bs: bs.set_iq_correction(fmx.FMX_IQC_AUTO, None, 0.5, capture=0),
              1: lambda bs: bs.set_iq_correction(fmx.FMX_IQC_FIXED, FIXED, capture=2)})
    assert _bits(ev[0]) == _bits(plain[0])
    assert _bits(ev[1][:first[2]]) == _bits(plain[1][:first[2]])
    assert np.any(ev[1][c2]["dbfs"] != plain[1][c2]["dbfs"])
    # the estimates across a restart, a reset and a parameter set
    seen, twin, kept = {}, {}, {}

    def events3(bs):
        kept["before"] = (bs.iq_correction(0), bs.iq_correction(2))
        bs.reset()
        bs.set_signal_params(2, 12, 0.5, -2.0, -60.0, -15.0)
        kept["after"] = (bs.iq_correction(0), bs.iq_correction(2))

    run({0: start, 1: lambda bs: None, 2: lambda bs: bs.set_iq_correction(fmx.FMX_IQC_AUTO, None, 0.5, capture=2), 3: events3},
        after=lambda k, bs: seen.__setitem__(k, (bs.iq_correction(0), bs.iq_correction(2))))
    run({0: start, 1: lambda bs: None, 2: lambda bs: None, 3: lambda bs: None},
        after=lambda k, bs: twin.__setitem__(k, (bs.iq_correction(0), bs.iq_correction(2))))
    assert [seen[k][0] for k in range(4)] == [twin[k][0] for k in range(4)]
    assert seen[0] == twin[0] and seen[1] == twin[1] and seen[2][1] != twin[2][1]
    assert kept["before"] == kept["after"] == seen[2]
    row2 = [calls[k][0][2][:2 * 333 * D] for k in range(4)]
    own, state = Q.estimate(row2[2], f)
    assert _rel(seen[2][1], own) <= EST_TOL, (seen[2][1], own)        # the restart: read 2's estimate alone
    on, _ = Q.estimate(row2[3], f, state, 0.5)
    assert _rel(seen[3][1], on) <= EST_TOL, (seen[3][1], on)          # the reset kept it: read 3 smooths on
    assert _rel(on, Q.estimate(row2[3], f)[0]) > 1e-6                 # and that differs from read 3's own estimate
    want, state = [], None
    for k in range(4):
        p, state = Q.estimate(calls[k][0][0][:2 * 333 * D], f, state, 0.5)
        assert _rel(seen[k][0], p) <= EST_TOL, (k, seen[k][0], p)


@pytest.mark.parametrize("fmt", ["u8", "s16"])
def test_scan_stops_tuning_ghosts_per_front_end(fmx, torch_cuda, fmt):
    """tests/test_wb_bank_scan_iqcorr.py's three impaired captures, 13 points
    from -600 to +600 kHz each, one read of 2048 outputs: with every capture
    in OFF fmx_scan_peaks(dbfs[slice], -45, 1) returns per capture the
    reference's ghost-laden sets ({-300k, 0, +300k}, {-500k, 0, +500k},
    {-500k, +200k, +500k}), with every capture in AUTO exactly the stations
    ({+300k}, {-500k}, {+200k, +500k}); each capture's read-back is within
    1e-12 relative of the reference estimate of its own samples and differs
    from the other captures'."""
    torch = torch_cuda
    f = FMT[fmt]
    D, tpp, n = BQ.GHOST_D, BQ.GHOST_TPP, BQ.GHOST_N_OUT
    rows = BQ.ghost_rows(f)
    grid = S.points(BQ.GHOST_START, BQ.GHOST_STEP, BQ.GHOST_POINTS)
    wcfg = fmx.make_wb_config(Q.CAP_FS, DSP, f, tpp, n)
    ps, _ = BQ.estimates(rows, f, D, n, [None] * 3, [1.0] * 3)
    peaks = lambda rec, s: [grid[i] for i in fmx.scan_peaks(rec["dbfs"][13 * s:13 * s + 13],  # noqa: E731
                                                            BQ.GHOST_THRESHOLD_DBFS, BQ.GHOST_SPACING)]
    seen = {}
    off = run_bscan(fmx, torch, wcfg, [grid] * 3, [(rows, n)], pad=37,
                    after=lambda k, bs: seen.update(off=[bs.iq_correction(s) for s in range(3)]))[0]
    auto = run_bscan(fmx, torch, wcfg, [grid] * 3, [(rows, n)], pad=37,
                     events={0: lambda bs: bs.set_iq_correction(fmx.FMX_IQC_AUTO)},
                     after=lambda k, bs: seen.update(auto=[bs.iq_correction(s) for s in range(3)]))[0]
    for s in range(3):
        print(f"{fmt} capture {s}: off {peaks(off, s)} auto {peaks(auto, s)} read-back {seen['auto'][s]}")
        assert peaks(off, s) == BQ.GHOSTS[s], (s, peaks(off, s))
        assert peaks(auto, s) == BQ.STATIONS[s], (s, peaks(auto, s))
        assert _rel(seen["auto"][s], ps[s]) <= EST_TOL, (s, seen["auto"][s], ps[s])
    assert seen["off"] == [Q.IDENTITY] * 3
    assert len(set(seen["auto"])) == 3


def test_a_bank_that_tunes_itself_past_the_ghosts(fmx, torch_cuda):
    """tests/test_gpu_wb_bank_scan.py's closed loop behind two impaired front
    ends: two u8 captures at 2.4 MS/s, two of the synthetic plan's stereo +
    RDS stations each (700, 701 at -900 and +200 kHz; 702, 703 at -300 and
    +700 kHz), capture 0 through Q gain 1.06, skew 4 degrees, DC (+0.020,
    -0.015), capture 1 through Q gain 0.95, skew -3 degrees, DC (-0.012,
    +0.025); 23 points at 100 kHz per capture.  One read in AUTO:
    fmx_scan_peaks(dbfs[slice], -40, 1) per capture returns exactly the
    stations' offsets; the same read in OFF returns more peaks than stations
    for at least one capture.  A WidebandBank created at the found
    frequencies, each capture in FIXED with the bank scan's read-back, through
    fmx_demod and fmx_rds over the 24 calls, decodes on every channel a group
    whose error-free block A is 0x1000 + 700 + station."""
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
        fe = BQ.FRONT_ENDS[s]
        rows.append(BQ.front_end(0.9 * x, R.U8, fe["q_gain"], fe["skew_deg"], fe["dc"]))
    grid = S.points(-1_100_000, 100_000, 23)
    wcfg = fmx.make_wb_config(Fs, R.BAND_DSP, fmx.FMX_WB_U8, 0, n)
    read = [([r[:2 * n * D] for r in rows], n)]
    found = lambda rec: [[grid[k] for k in fmx.scan_peaks(rec["dbfs"][23 * s:23 * (s + 1)], -40.0, 1)]  # noqa: E731
                         for s in range(2)]
    par = {}
    auto = run_bscan(fmx, torch, wcfg, [grid, grid], read, events={0: lambda bs: bs.set_iq_correction(fmx.FMX_IQC_AUTO)},
                     after=lambda k, bs: par.update({s: bs.iq_correction(s) for s in range(2)}))[0]
    off = run_bscan(fmx, torch, wcfg, [grid, grid], read)[0]
    print("found in AUTO", found(auto), "in OFF", found(off), "read-backs", par)
    assert found(auto) == [list(w) for w in where], found(auto)
    assert any(len(found(off)[s]) > 2 for s in range(2)), found(off)
    assert par[0] != par[1]
    # tune the bank to what the scan found, correct it with what the scan estimated
    Cn = 4
    dev = torch.device("cuda")
    h = fmx.Handle(fmx.make_config(bandwidth_hz=-1, deemphasis=1), Cn)
    bank = fmx.WidebandBank(h, wcfg, found(auto))
    for s in range(2):
        bank.set_iq_correction(fmx.FMX_IQC_FIXED, par[s], capture=s)
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
    assert [bank.iq_correction(s) for s in range(2)] == [par[0], par[1]]
    bank.close()
    h.close()
    for c in range(Cn):
        good = [g for g in groups[c] if (g[4] >> 6) == 0]
        assert any(g[0] == 0x1000 + R.BAND_CH0 + c for g in good), (c, groups[c])


def test_errors(fmx, torch_cuda):
    """FMX_E_INVALID with the function named: a capture outside
    [-1, n_captures), capture -1 or a NULL h_out in the read-back, a bad mode,
    alpha below 0 or above 1, a NULL fixed in FIXED, gain 0, a NaN field, and
    the two calls handed a wb, a scan and a bank object; alpha 0 and alpha 1
    are legal.  The six existing correction calls still refuse the bank scan."""
    L = fmx.lib()
    h = fmx.Handle(fmx.make_config(iq_rate=DSP, dsp_rate=DSP), 3)
    err = lambda: L.fmx_last_error(h.h)  # noqa: E731
    p = fmx.IqCorrection(0.0, 0.0, 1.0, 0.0)
    out = fmx.IqCorrection()
    bs = fmx.WidebandBankScan(h, fmx.make_wb_config(block=64), [[-100_000, 0, 100_000], [], [50_000]])
    setn, getn = b"fmx_wb_bank_scan_set_iq_correction", b"fmx_wb_bank_scan_iq_correction"
    fn, rd = L.fmx_wb_bank_scan_set_iq_correction, L.fmx_wb_bank_scan_iq_correction
    nan = float("nan")
    for cap in (-2, 3, 1 << 20):
        assert fn(bs.b, cap, fmx.FMX_IQC_AUTO, None, 0.5) == -1 and setn in err(), cap
        assert rd(bs.b, cap, C.byref(out)) == -1 and getn in err(), cap
    assert rd(bs.b, -1, C.byref(out)) == -1 and getn in err()
    assert rd(bs.b, 0, None) == -1 and getn in err()
    for cap in (-1, 0, 1):
        assert fn(bs.b, cap, 3, C.byref(p), 0.5) == -1 and setn in err()
        assert fn(bs.b, cap, -1, C.byref(p), 0.5) == -1 and setn in err()
        assert fn(bs.b, cap, fmx.FMX_IQC_AUTO, None, -0.1) == -1 and setn in err()
        assert fn(bs.b, cap, fmx.FMX_IQC_AUTO, None, 1.01) == -1 and setn in err()
        assert fn(bs.b, cap, fmx.FMX_IQC_AUTO, None, nan) == -1
        assert fn(bs.b, cap, fmx.FMX_IQC_FIXED, None, 0.0) == -1 and setn in err()
        for bad in ((0.0, 0.0, 0.0, 0.0), (0.0, 0.0, -1.0, 0.0), (nan, 0.0, 1.0, 0.0), (0.0, 0.0, 1.0, float("inf"))):
            assert fn(bs.b, cap, fmx.FMX_IQC_FIXED, C.byref(fmx.IqCorrection(*bad)), 0.0) == -1 and setn in err(), bad
    assert all(bs.iq_correction(s) == Q.IDENTITY for s in range(3))  # nothing took effect
    for cap in (-1, 1, 2):
        assert fn(bs.b, cap, fmx.FMX_IQC_AUTO, None, 0.0) == 0 and fn(bs.b, cap, fmx.FMX_IQC_AUTO, None, 1.0) == 0
        assert fn(bs.b, cap, fmx.FMX_IQC_OFF, None, 0.0) == 0
    bs.set_iq_correction(fmx.FMX_IQC_FIXED, FIXED, capture=1)  # the empty capture
    assert [bs.iq_correction(s) for s in range(3)] == [Q.IDENTITY, FIXED, Q.IDENTITY]
    # the other kinds of object handed to the two calls
    wb = fmx.Wideband(h, fmx.make_wb_config(block=64), [0, 1000])
    sc = fmx.WidebandScan(h, fmx.make_wb_scan_config(block=64))
    bank = fmx.WidebandBank(h, fmx.make_wb_config(block=64), [[0]])
    for obj in (wb.w, sc.s, bank.b):
        assert fn(obj, 0, fmx.FMX_IQC_OFF, None, 0.0) == -1 and setn in err()
        assert rd(obj, 0, C.byref(out)) == -1 and getn in err()
    # and the six existing calls handed the bank scan
    refusals = [("fmx_wb_set_iq_correction", (bs.b, fmx.FMX_IQC_FIXED, C.byref(p), 0.0)),
                ("fmx_wb_iq_correction", (bs.b, C.byref(out))),
                ("fmx_wb_scan_set_iq_correction", (bs.b, fmx.FMX_IQC_FIXED, C.byref(p), 0.0)),
                ("fmx_wb_scan_iq_correction", (bs.b, C.byref(out))),
                ("fmx_wb_bank_set_iq_correction", (bs.b, -1, fmx.FMX_IQC_FIXED, C.byref(p), 0.0)),
                ("fmx_wb_bank_iq_correction", (bs.b, 0, C.byref(out)))]
    for name, args in refusals:
        assert getattr(L, name)(*args) == -1, name
        assert name.encode() in err(), (name, err())
    bank.close()
    sc.close()
    wb.close()
    bs.close()
    h.close()
