"""DC-offset and IQ-imbalance correction of wide captures on the GPU
(fmx_wb_set_iq_correction, fmx_wb_scan_set_iq_correction; kernels k_iqc_sums,
k_iqc_finish, k_iqc_fixed, k_wb_iqc, k_wb_scan_iqc)
against the float64 / int64 restatement tests/wb_iq_ref.py.

Rows: max |d| < 1e-5, the bar of every row comparison of the channelizer
(tests/test_gpu_wideband.py).  The estimator's read-back: 1e-12 relative (its
sums are exact integers, the rest a dozen double operations).  Scan records:
tests/test_gpu_wb_scan.py's bars.  Shapes: 19 channels (a full group of 16 and
a ragged one of 3) at section 18's edge frequencies, full-scale noise, u8 and
int16, D = 10 (even, tpp 28) and D = 5 (odd, tpp 20), calls of 341, 111, 1, 6,
342 and 32 outputs against one call of 833."""
import ctypes as C

import numpy as np
import pytest

import gpu_harness as H
import wb_iq_ref as Q
import wb_ref as R
import wb_scan_ref as S
from test_gpu_parity import MPX_MAX_TOL, MPX_RMS_TOL, log_errors
from test_gpu_wb_scan import DB_TOL, LEVEL_TOL, REC, RMS_TOL
from test_gpu_wb_scan import _compare as scan_compare
from test_gpu_wideband import _freqs, _raw
from test_wb_iqcorr import IMAGE_AFTER_DB, IMAGE_BEFORE_DB, image_rejection_reference

pytestmark = pytest.mark.gpu

WB_TOL = 1e-5
EST_TOL = 1e-12
DSP = 240_000
SIZES = (341, 111, 1, 6, 342, 32)
BLOCK = sum(SIZES)  # 833
NCH = 19
TPP = {10: 28, 5: 20}
FMT = {"u8": R.U8, "s16": R.S16}
FIXED = (0.02, -0.015, 0.9457, -0.0699)
SHAPES = [("s16", 10), ("u8", 10), ("s16", 5), ("u8", 5)]


def run(fmx, torch, fmt, D, freqs, raw, sizes, setup=None, before=None, after=None, in_off=0, pad=0, block=BLOCK):
    """raw (interleaved I/Q) through fmx_wb_process in calls of `sizes` outputs
    -> complex64 [len(freqs)][sum(sizes)].  setup(wb) runs once after the
    object is made, before(i, wb) ahead of call i, after(i, wb) behind its
    sync.  in_off: the input's byte offset in its allocation; the output rows
    have a stride of block + pad cells, and with pad every cell outside the
    rows' first n is checked against gpu_harness's sentinel."""
    Cn = len(freqs)
    h = fmx.Handle(fmx.make_config(iq_rate=DSP, dsp_rate=DSP), Cn)  # fmx_wb_process is not bound by the handle's block
    wb = fmx.Wideband(h, fmx.make_wb_config(D * DSP, DSP, FMT[fmt], TPP[D], block), freqs)
    if setup:
        setup(wb)
    dev = torch.device("cuda")
    t = torch.full((in_off + raw.nbytes + 64,), H.SENTINEL_BYTE, dtype=torch.uint8, device=dev)
    t[in_off:in_off + raw.nbytes] = torch.from_numpy(np.ascontiguousarray(raw).view(np.uint8).copy()).to(dev)
    per = 2 * raw.itemsize
    stride = block + pad
    G = H.Guarded(torch, "f32", Cn, 2 * stride, off=1 if pad else 0, tail=21 if pad else 0)
    rows, pos = [], 0
    for i, n in enumerate(sizes):
        if before:
            before(i, wb)
        if pad:
            G.fill()
            torch.cuda.synchronize()
        wb.process(t.data_ptr() + in_off + per * D * pos, n, G.ptr, stride)
        h.sync()
        if after:
            after(i, wb)
        out = G.raw()
        if pad:
            G.check(2 * n, ("call", i, n), out)
        rows.append(G.view(out, np.float32)[:, :2 * n].copy().view(np.complex64))
        pos += n
    wb.close()
    h.close()
    return np.concatenate(rows, axis=1)


def _noise(fmt, D):
    return _raw(FMT[fmt], BLOCK * D, 300 + D)


def _cut(raw, D, sizes):
    out, pos = [], 0
    for n in sizes:
        out.append(raw[2 * D * pos:2 * D * (pos + n)])
        pos += n
    return out


def _bits(a):
    return a.view(np.uint32)


def _rel(got, want):
    return max(abs(g - w) / max(abs(w), 1e-300) if g != w else 0.0 for g, w in zip(got, want))


def _log(tag, c, d, ref):
    st = dict(wb_max=float(np.max(np.abs(d))), wb_rms=float(np.sqrt(np.mean(np.abs(d) ** 2))),
              wb_rel_rms=float(np.sqrt(np.mean(np.abs(d) ** 2) / max(np.mean(np.abs(ref) ** 2), 1e-300))),
              groups_oracle=[])
    log_errors(tag, c, st)
    return st


@pytest.mark.parametrize("fmt,D", SHAPES)
def test_off_is_todays_channelizer(fmx, torch_cuda, fmt, D):
    """An object that never got the call, one set to OFF, and one set to FIXED
    and back to OFF before its first process call: bit-identical rows, and
    within 1e-5 of the uncorrected float64 channelizer.  FIXED with
    (0, 0, 1, 0) runs the corrected kernel and gives rows equal as numbers."""
    raw, freqs = _noise(fmt, D), _freqs(D * DSP)
    never = run(fmx, torch_cuda, fmt, D, freqs, raw, SIZES)
    off = run(fmx, torch_cuda, fmt, D, freqs, raw, SIZES, setup=lambda wb: wb.set_iq_correction(fmx.FMX_IQC_OFF))

    def there_and_back(wb):
        wb.set_iq_correction(fmx.FMX_IQC_FIXED, FIXED)
        wb.set_iq_correction(fmx.FMX_IQC_OFF)

    back = run(fmx, torch_cuda, fmt, D, freqs, raw, SIZES, setup=there_and_back)
    ident = run(fmx, torch_cuda, fmt, D, freqs, raw, SIZES,
                setup=lambda wb: wb.set_iq_correction(fmx.FMX_IQC_FIXED, Q.IDENTITY))
    assert np.array_equal(_bits(never), _bits(off)) and np.array_equal(_bits(never), _bits(back))
    assert np.array_equal(ident, never)
    ref = R.channelize(R.normalise(raw, FMT[fmt]), D, TPP[D], D * DSP, freqs)
    assert np.max(np.abs(never - ref)) < WB_TOL


@pytest.mark.parametrize("fmt,D", SHAPES)
def test_fixed_against_float64(fmx, torch_cuda, fmt, D):
    """FIXED with (0.02, -0.015, 0.9457, -0.0699), the ragged calls: every
    channel's max |d| < 1e-5 against wb_iq_ref.rows (the correction applied to
    the stream from L zeros before its start on).  The single call of 833, a
    fresh object, the input one element off its alignment and rows of stride
    block + 3 inside intact guard cells: bit-identical rows.  The uncorrected
    reference is 0.02 away: the check can tell.
    Achieved (worst channel's max / RMS; profiles/wb_iqcorr_parity_errors.jsonl):
    int16 D = 10 3.4e-7 / 5.1e-8, u8 D = 10 2.3e-7 / 4.3e-8, int16 D = 5
    2.4e-7 / 5.2e-8, u8 D = 5 2.5e-7 / 4.7e-8."""
    raw, freqs = _noise(fmt, D), _freqs(D * DSP)
    fixed = lambda wb: wb.set_iq_correction(fmx.FMX_IQC_FIXED, FIXED)  # noqa: E731
    ragged = run(fmx, torch_cuda, fmt, D, freqs, raw, SIZES, setup=fixed)
    ref = Q.rows(_cut(raw, D, SIZES), FMT[fmt], D, TPP[D], D * DSP, freqs, [FIXED] * len(SIZES))
    assert ragged.shape == ref.shape == (NCH, BLOCK)
    worst = 0.0
    for c in range(NCH):
        worst = max(worst, _log(f"wb_iqcorr_fixed_{fmt}_D{D}_f{freqs[c]}", c, ragged[c] - ref[c], ref[c])["wb_max"])
    print(f"fixed {fmt} D = {D}: worst max |d| = {worst:.3g}")
    assert worst < WB_TOL, worst
    plain = R.channelize(R.normalise(raw, FMT[fmt]), D, TPP[D], D * DSP, freqs)
    assert np.max(np.abs(plain[0] - ref[0])) > 0.01  # channel 0 sits on the DC term
    one = run(fmx, torch_cuda, fmt, D, freqs, raw, [BLOCK], setup=fixed)
    again = run(fmx, torch_cuda, fmt, D, freqs, raw, SIZES, setup=fixed)
    skew = run(fmx, torch_cuda, fmt, D, freqs, raw, SIZES, setup=fixed, in_off=raw.itemsize, pad=3)
    for other in (one, again, skew):
        assert np.array_equal(_bits(ragged), _bits(other))


@pytest.mark.parametrize("fmt", ["s16", "u8"])
def test_auto_follows_the_reference_estimator(fmx, torch_cuda, fmt):
    """AUTO with alpha 0.25, four calls of 341 outputs of impaired_capture:
    fmx_wb_iq_correction after each call equals the reference estimator's
    smoothed result within 1e-12 relative, and the rows agree with the
    reference evaluated with those parameters (max |d| < 1e-5).  Then
    fmx_wb_reset keeps the estimate (the read-back is unchanged, and the next
    call smooths on from it), and setting AUTO again restarts it: the next
    call's parameters are that call's alone."""
    D, n, alpha = 10, 341, 0.25
    freqs = _freqs(D * DSP)
    raw = Q.impaired_capture(FMT[fmt])[:2 * D * n * 6]
    calls = _cut(raw, D, [n] * 6)
    seen = {}

    def before(i, wb):
        if i == 4:
            wb.reset(0)
            seen["kept"] = wb.iq_correction()
        if i == 5:
            wb.set_iq_correction(fmx.FMX_IQC_AUTO, None, alpha)

    def after(i, wb):
        seen[i] = wb.iq_correction()

    got = run(fmx, torch_cuda, fmt, D, freqs, raw, [n] * 6, block=n, before=before, after=after,
              setup=lambda wb: wb.set_iq_correction(fmx.FMX_IQC_AUTO, None, alpha))
    want, state = [], None
    for k in range(5):
        p, state = Q.estimate(calls[k], FMT[fmt], state, alpha)
        want.append(p)
    want.append(Q.estimate(calls[5], FMT[fmt])[0])  # the restart
    for k in range(6):
        err = _rel(seen[k], want[k])
        print(f"auto {fmt} call {k}: {seen[k]} rel err {err:.3g}")
        assert err <= EST_TOL, (k, seen[k], want[k])
    assert seen["kept"] == seen[3]
    assert want[1] != want[0] and _rel(want[5], want[4]) > 1e-6  # the smoothing moved, the restart shows
    ref = Q.rows(calls[:4], FMT[fmt], D, TPP[D], D * DSP, freqs, want[:4])
    worst = 0.0
    for c in range(NCH):
        st = _log(f"wb_iqcorr_auto_{fmt}_f{freqs[c]}", c, got[c, :4 * n] - ref[c], ref[c])
        worst = max(worst, st["wb_max"])
    print(f"auto {fmt}: worst max |d| = {worst:.3g}")
    assert worst < WB_TOL, worst


@pytest.mark.parametrize("fmt", ["s16", "u8"])
def test_image_rejection(fmx, torch_cuda, fmt):
    """impaired_capture, D = 10, channels at +300 kHz and -300 kHz, one call of
    9600 outputs: the reference's own conditions first (uncorrected between
    -29 and -25 dB, corrected at most -45 dB), then the GPU's ratio within
    0.5 dB of the reference's, uncorrected and in AUTO."""
    before, after, _ = image_rejection_reference(FMT[fmt])
    assert IMAGE_BEFORE_DB[0] <= before <= IMAGE_BEFORE_DB[1] and after <= IMAGE_AFTER_DB, (before, after)
    raw = Q.impaired_capture(FMT[fmt])
    n = Q.CAP_N // 10
    freqs = [Q.CAP_STATION_HZ, -Q.CAP_STATION_HZ]
    off = run(fmx, torch_cuda, fmt, 10, freqs, raw, [n], block=n)
    auto = run(fmx, torch_cuda, fmt, 10, freqs, raw, [n], block=n,
               setup=lambda wb: wb.set_iq_correction(fmx.FMX_IQC_AUTO, None, 0.0))
    g0, g1 = Q.image_ratio_db(off.astype(np.complex128)), Q.image_ratio_db(auto.astype(np.complex128))
    print(f"image {fmt}: reference {before:.2f} -> {after:.2f} dB, GPU {g0:.2f} -> {g1:.2f} dB")
    assert abs(g0 - before) < 0.5 and abs(g1 - after) < 0.5, (g0, before, g1, after)


SCAN_START, SCAN_STEP, SCAN_POINTS = -600_000, 100_000, 13


def run_scan(fmx, torch, raw, n_out, mode=None, reads=1, alpha=0.0):
    """`reads` reads of the same int16 capture by one scan object -> (records
    [reads][points], the object's parameters after each read)."""
    h = fmx.Handle(fmx.make_config(iq_rate=DSP, dsp_rate=DSP), 1)
    scfg = fmx.make_wb_scan_config(Q.CAP_FS, DSP, fmx.FMX_WB_S16, 0, n_out, SCAN_START, SCAN_STEP, SCAN_POINTS)
    sc = fmx.WidebandScan(h, scfg)
    if mode is not None:
        sc.set_iq_correction(mode, None, alpha)
    d_raw = torch.from_numpy(np.ascontiguousarray(raw).copy()).to(torch.device("cuda"))
    G = H.Guarded(torch, "i32", 1, SCAN_POINTS, off=2, tail=21, cell=10)
    recs, pars = [], []
    for k in range(reads):
        G.fill()
        torch.cuda.synchronize()
        sc.process(d_raw.data_ptr(), n_out, G.ptr)
        h.sync()
        pars.append(sc.iq_correction())
        got = G.raw()
        G.check(SCAN_POINTS, ("read", k), got)
        recs.append(G.view(got)[0].copy().view(REC))
    sc.close()
    h.close()
    return np.stack(recs), pars


def test_scan_stops_tuning_ghosts(fmx, torch_cuda):
    """13 points from -600 kHz to +600 kHz, one read of impaired_capture as
    int16.  Expected from the construction: station about -9 dBFS, image about
    -36, DC about -35, noise floor below -55.  fmx_scan_peaks(-45 dBFS,
    spacing 1) on the reference's levels, then on the GPU's: uncorrected the
    points -300 kHz, 0 and +300 kHz, in AUTO +300 kHz alone.  The records
    agree with the reference on the corrected samples within
    tests/test_gpu_wb_scan.py's bars, the clip ratios exactly; the read-back
    is the reference's estimate within 1e-12.  A second read of the same
    capture in AUTO gives the first read's records bit for bit (smoothing equal
    moments changes nothing but rounding, and the levels' smoother is fed equal levels)."""
    fmt, D, tpp = R.S16, 10, 28
    raw = Q.impaired_capture(fmt)
    n = Q.CAP_N // D
    freqs = S.points(SCAN_START, SCAN_STEP, SCAN_POINTS)
    p, _ = Q.estimate(raw, fmt)
    want_off = Q.scan_call(raw, fmt, D, tpp, Q.CAP_FS, freqs, n, Q.IDENTITY)
    want_auto = Q.scan_call(raw, fmt, D, tpp, Q.CAP_FS, freqs, n, p)
    peaks = lambda db: [freqs[i] for i in fmx.scan_peaks(db, -45.0, 1)]  # noqa: E731
    ghosts, clean = [-300_000, 0, 300_000], [300_000]
    db_off, db_auto = [w["dbfs"] for w in want_off], [w["dbfs"] for w in want_auto]
    print("reference dBFS off ", np.round(db_off, 2))
    print("reference dBFS auto", np.round(db_auto, 2))
    assert abs(db_off[9] + 9.0) < 0.5 and abs(db_off[3] + 36.0) < 1.5 and abs(db_off[6] + 35.0) < 1.5
    assert max(db_auto[:8] + db_auto[11:]) < -55.0
    assert peaks(db_off) == ghosts and peaks(db_auto) == clean
    got_off, par_off = run_scan(fmx, torch_cuda, raw, n)
    got_auto, par_auto = run_scan(fmx, torch_cuda, raw, n, fmx.FMX_IQC_AUTO, reads=2, alpha=0.5)
    for tag, got, want in (("wb_iqcorr_scan_off", got_off[0], want_off), ("wb_iqcorr_scan_auto", got_auto[0], want_auto)):
        st = scan_compare(tag, got, want)
        assert st["scan_rms_err"] < RMS_TOL, st
        assert st["scan_db_err_loud"] < DB_TOL and st["scan_cdb_err_loud"] < DB_TOL and st["scan_level_err_loud"] < LEVEL_TOL, st
        assert np.all(got["hard_clip_ratio"] == want[0]["hard_clip_ratio"])
        assert np.all(got["near_clip_ratio"] == want[0]["near_clip_ratio"])
    assert par_off[0] == Q.IDENTITY
    assert _rel(par_auto[0], p) <= EST_TOL, (par_auto[0], p)
    assert _rel(par_auto[1], p) <= EST_TOL, (par_auto[1], p)
    assert peaks(got_off[0]["dbfs"]) == ghosts and peaks(got_auto[0]["dbfs"]) == clean
    for f in ("dbfs", "level120", "hard_clip_ratio"):
        assert np.max(np.abs(got_auto[1][f] - got_auto[0][f])) < 1e-6, f


def test_band_receiver_in_fixed_mode(fmx, torch_cuda):
    """Two calls of n = 1024 through fmx_wb_process_block on an object in
    FIXED against fmx_demod of the rows a twin object in the same mode gives
    through fmx_wb_process.  fmx_demod's front end is k_frontend, and a
    process_block call of n >= 1024 takes k_fecf, whose
    MPX differs from k_frontend's in the last bits whatever the rows are.  So
    d_mpx is bit-identical to fmx_demod's where the receiver runs the front
    end fmx_demod runs (FMX_DIAG_FE_GENERIC), and on k_fecf the station's
    channel is within the project's MPX bars (max 3e-4, RMS 1e-5; the two
    other channels hold noise alone once the image and the DC are gone, where
    a discriminator amplifies a last-bit difference without bound: their
    figures are logged, not gated).  fmx_wb_signal behind each call returns
    the records it returns behind the twin's call, bit for bit, and those are
    the ones computed from the twin's rows by section 21's rule (P = mean
    |y|^2, wb_scan_ref.record; tests/test_gpu_wb_signal.py's bars)."""
    torch = torch_cuda
    n, D, fmt = 1024, 10, R.S16
    freqs = [Q.CAP_STATION_HZ, -Q.CAP_STATION_HZ, 0]
    Cn = len(freqs)
    raw = Q.impaired_capture(fmt)[:2 * D * 2 * n]
    dev = torch.device("cuda")
    d_raw = torch.from_numpy(raw.copy()).to(dev)
    f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)  # noqa: E731
    mk = lambda: fmx.Handle(fmx.make_config(iq_rate=DSP, dsp_rate=DSP, block=n, bandwidth_hz=-1, deemphasis=1), Cn)  # noqa: E731
    wcfg = fmx.make_wb_config(Q.CAP_FS, DSP, fmx.FMX_WB_S16, 0, n)
    lev = lambda: torch.zeros(Cn * 40, dtype=torch.uint8, device=dev)  # noqa: E731

    def receiver(generic):
        h = mk()
        wb = fmx.Wideband(h, wcfg, freqs)
        wb.set_iq_correction(fmx.FMX_IQC_FIXED, FIXED)
        if generic:
            h.diag_set(fmx.FMX_DIAG_FE_GENERIC, 1)
        mpx, pl, pr, cnt, lv = f32(Cn, n), f32(Cn, n), f32(Cn, n), torch.zeros(Cn, dtype=torch.int32, device=dev), lev()
        out = fmx.BlockOut(mpx.data_ptr(), n, pl.data_ptr(), pr.data_ptr(), n, cnt.data_ptr(), None, None, None, None, 0,
                           None, None, None)
        res = []
        for k in range(2):
            wb.process_block(d_raw.data_ptr() + 4 * D * n * k, n, out)
            wb.signal(lv.data_ptr())
            h.sync()
            res.append((mpx.cpu().numpy().copy(), lv.cpu().numpy().copy().view(REC)))
        wb.close()
        h.close()
        return res

    def twin():
        h = mk()
        wb = fmx.Wideband(h, wcfg, freqs)
        wb.set_iq_correction(fmx.FMX_IQC_FIXED, FIXED)
        bb, mpx, lv = f32(Cn, 2 * n), f32(Cn, n), lev()
        res = []
        for k in range(2):
            wb.process(d_raw.data_ptr() + 4 * D * n * k, n, bb.data_ptr(), n)
            wb.signal(lv.data_ptr())
            h.demod(bb.data_ptr(), 2 * n, n, mpx.data_ptr(), n)
            h.sync()
            res.append((mpx.cpu().numpy().copy(), lv.cpu().numpy().copy().view(REC),
                        bb.cpu().numpy().copy().view(np.complex64)))
        wb.close()
        h.close()
        return res

    rx, rx_generic, tw = receiver(False), receiver(True), twin()
    for k in range(2):
        d = (rx[k][0] - tw[k][0]).astype(np.float64)
        st = dict(mpx_max_by_channel=[float(v) for v in np.max(np.abs(d), axis=1)],
                  mpx_rms_by_channel=[float(v) for v in np.sqrt(np.mean(d * d, axis=1))],
                  mpx_max_generic=float(np.max(np.abs(rx_generic[k][0] - tw[k][0]))), groups_oracle=[])
        log_errors(f"wb_iqcorr_receiver_call{k}", 0, st)
        # the front end fmx_demod runs: the same rows in, the same bits out
        assert np.array_equal(_bits(rx_generic[k][0]), _bits(tw[k][0])), k
        # k_fecf on the same rows, the station's channel: the project's MPX bars
        assert st["mpx_max_by_channel"][0] < MPX_MAX_TOL and st["mpx_rms_by_channel"][0] < MPX_RMS_TOL, st
    for k in range(2):
        assert rx[k][1].tobytes() == tw[k][1].tobytes() == rx_generic[k][1].tobytes(), k
        pw = np.mean(np.abs(tw[k][2].astype(np.complex128)) ** 2, axis=1)
        hard, near = S.clip_ratios(raw[2 * D * n * k:2 * D * n * (k + 1)], fmt)
        want = [dict(S.record(v), hard_clip_ratio=hard, near_clip_ratio=near) for v in pw]
        got = tw[k][1]
        assert np.max(np.abs(S.rms_of(got["dbfs"]) - S.rms_of([w["dbfs"] for w in want]))) < RMS_TOL
        assert np.max(np.abs(got["level120"] - np.array([w["level120"] for w in want]))) < LEVEL_TOL
        assert np.all(got["hard_clip_ratio"] == hard) and np.all(got["near_clip_ratio"] == near)
    # the rows are the corrected ones: the image channel is far below the station
    assert tw[1][1]["dbfs"][0] - tw[1][1]["dbfs"][1] > 40.0


def test_errors(fmx, torch_cuda):
    """A rational object at Q = 3 and a bank: FMX_E_INVALID with the function
    named; bad mode, alpha < 0 or > 1, NULL `fixed` in FIXED, gain = 0 and NaN:
    FMX_E_INVALID; alpha = 0 and alpha = 1 are legal."""
    L = fmx.lib()
    h = fmx.Handle(fmx.make_config(iq_rate=DSP, dsp_rate=DSP), 2)
    p = fmx.IqCorrection(0.0, 0.0, 1.0, 0.0)
    out = fmx.IqCorrection()
    rat = fmx.Wideband(h, fmx.make_wb_config(2_000_000, DSP, fmx.FMX_WB_U8, 0, 300), [0, 1000], rational=True)
    assert fmx.wb_ratio(rat.cfg)[1] == 3
    assert L.fmx_wb_set_iq_correction(rat.w, fmx.FMX_IQC_FIXED, C.byref(p), 0.0) == -1
    assert b"fmx_wb_set_iq_correction" in L.fmx_last_error(h.h)
    assert L.fmx_wb_iq_correction(rat.w, C.byref(out)) == -1 and b"fmx_wb_iq_correction" in L.fmx_last_error(h.h)
    rat.close()
    bank = fmx.WidebandBank(h, fmx.make_wb_config(block=64), [[0], [1000]])
    for name in ("fmx_wb_set_iq_correction", "fmx_wb_scan_set_iq_correction"):
        assert getattr(L, name)(bank.b, fmx.FMX_IQC_AUTO, None, 0.5) == -1
        assert name.encode() in L.fmx_last_error(h.h)
    for name in ("fmx_wb_iq_correction", "fmx_wb_scan_iq_correction"):
        assert getattr(L, name)(bank.b, C.byref(out)) == -1 and name.encode() in L.fmx_last_error(h.h)
    bank.close()
    wb = fmx.Wideband(h, fmx.make_wb_config(block=64), [0, 1000])
    sc = fmx.WidebandScan(h, fmx.make_wb_scan_config(block=64))
    nan = float("nan")
    for fn, obj in ((L.fmx_wb_set_iq_correction, wb.w), (L.fmx_wb_scan_set_iq_correction, sc.s)):
        name = b"fmx_wb_scan_set_iq_correction" if obj is sc.s else b"fmx_wb_set_iq_correction"
        assert fn(obj, 3, C.byref(p), 0.5) == -1 and name in L.fmx_last_error(h.h)
        assert fn(obj, -1, C.byref(p), 0.5) == -1
        assert fn(obj, fmx.FMX_IQC_AUTO, None, -0.1) == -1 and fn(obj, fmx.FMX_IQC_AUTO, None, 1.01) == -1
        assert fn(obj, fmx.FMX_IQC_AUTO, None, nan) == -1
        assert fn(obj, fmx.FMX_IQC_FIXED, None, 0.0) == -1 and name in L.fmx_last_error(h.h)
        for bad in ((0.0, 0.0, 0.0, 0.0), (0.0, 0.0, -1.0, 0.0), (nan, 0.0, 1.0, 0.0), (0.0, 0.0, 1.0, float("inf"))):
            q = fmx.IqCorrection(*bad)
            assert fn(obj, fmx.FMX_IQC_FIXED, C.byref(q), 0.0) == -1, bad
        assert fn(obj, fmx.FMX_IQC_AUTO, None, 0.0) == 0 and fn(obj, fmx.FMX_IQC_AUTO, None, 1.0) == 0
        assert fn(obj, fmx.FMX_IQC_FIXED, C.byref(p), 7.0) == 0  # alpha is ignored outside AUTO
        assert fn(obj, fmx.FMX_IQC_OFF, None, 0.0) == 0
    # an object and a scan are not each other's
    assert L.fmx_wb_set_iq_correction(sc.s, fmx.FMX_IQC_OFF, None, 0.0) == -1
    assert L.fmx_wb_scan_set_iq_correction(wb.w, fmx.FMX_IQC_OFF, None, 0.0) == -1
    assert L.fmx_wb_iq_correction(wb.w, None) == -1
    assert wb.iq_correction() == Q.IDENTITY and sc.iq_correction() == Q.IDENTITY
    wb.set_iq_correction(fmx.FMX_IQC_FIXED, FIXED)
    assert wb.iq_correction() == FIXED
    sc.close()
    wb.close()
    h.close()
