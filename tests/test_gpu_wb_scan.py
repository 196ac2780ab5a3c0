"""The band scan on the GPU (fmx_wb_scan_*, kernels k_wb_scan, k_wb_scan_clip,
k_wb_scan_level): one wide IQ capture in, one fmx_signal_level record per
scan point out, against the float64 restatement tests/wb_scan_ref.py (itself
pinned to the reference's computeSignalLevel by tests/test_wb_scan.py).

Bar of every level comparison: |rms_gpu - rms_ref| < 1e-5 with rms =
10^(dbfs / 20) - 1e-12.  It follows from fmx_decimate's bar on the rows
(max |d| < 1e-5): the RMS of a difference cannot exceed
its maximum.  At rms_ref >= 1e-3 that is < 0.09 dB and < 0.29 of level120."""
import ctypes as C
import functools

import numpy as np
import pytest

import gpu_harness as H
import wb_ref as R
import wb_scan_ref as S
from test_gpu_parity import log_errors
from test_wb_scan import BAND_POINTS, BAND_SCAN_CALLS, BAND_START, BAND_STEP, band_levels

pytestmark = pytest.mark.gpu

RMS_TOL = 1e-5
DB_TOL, LEVEL_TOL = 0.09, 0.29  # what RMS_TOL comes to at rms_ref >= 1e-3
DSP = 240_000
NP = 19                         # a ragged second group of 16
FMT = {"u8": R.U8, "s16": R.S16}
GEO = {10: (28, -900_000, 100_000), 25: (12, -2_700_000, 300_000), 100: (28, -11_700_000, 1_300_000)}  # D: tpp, start, step
# complex tones 7 kHz above these points (none the mirror image of another, two
# of them -- 2 and 5 -- with nothing on the positive side) and noise of RMS 1e-3
TONE_POINTS, TONE_OFF = (2, 5, 10, 12, 17), 7_000
TONE_AMP = (0.3, 0.1, 0.03, 0.01, 0.003)
CLIP_AMP = (0.45, 0.2, 0.05, 0.01, 0.003)  # the smoother test's capture: twice it clips
PARAMS = (12, 0.5, -2.0, -60.0, -15.0)
REC = np.dtype([("level120", "<f4"), ("level120_smoothed", "<f4"), ("dbfs", "<f8"), ("compensated_dbfs", "<f8"),
                ("hard_clip_ratio", "<f8"), ("near_clip_ratio", "<f8")])
assert REC.itemsize == 40


def _sizes(tpp):
    return [4096, 333, tpp + 17, tpp + 1]


def _scfg(fmx, fmt, D, block=4096, start=None, step=None, n=NP):
    tpp, s0, st = GEO[D]
    return fmx.make_wb_scan_config(D * DSP, DSP, FMT[fmt], tpp, block, s0 if start is None else start,
                                   st if step is None else step, n)


@functools.lru_cache(maxsize=None)
def _capture(fmt, D, n_samples, seed=1, amps=TONE_AMP, scale=1.0):
    """Interleaved raw I/Q of the coloured capture."""
    tpp, start, step = GEO[D]
    Fs = D * DSP
    rng = np.random.default_rng(seed)
    i = np.arange(n_samples, dtype=np.int64)
    x = (1e-3 / np.sqrt(2.0)) * (rng.normal(size=n_samples) + 1j * rng.normal(size=n_samples))
    for p, a in zip(TONE_POINTS, amps):
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


def run_scan(fmx, torch, scfg, calls, params=None, in_off=0, reset_before=()):
    """calls: [(raw, n_out)], each raw array (uint8 / int16, interleaved, at
    least n_out * D samples; what lies behind them is handed to the device
    too) on the device at byte offset in_off of its allocation.  The records
    live in a sentinel-guarded allocation checked after every call.
    -> records [len(calls)][n_points] (numpy, dtype REC)."""
    h = fmx.Handle(fmx.make_config(iq_rate=DSP, dsp_rate=DSP), 1)
    sc = fmx.WidebandScan(h, scfg)
    if params:
        sc.set_signal_params(*params)
    dev = torch.device("cuda")
    P = scfg.n_points
    G = H.Guarded(torch, "i32", 1, P, off=2, tail=21, cell=10)
    out = []
    for k, (raw, n_out) in enumerate(calls):
        if k in reset_before:
            sc.reset()
        t = torch.full((in_off + raw.nbytes + 64,), H.SENTINEL_BYTE, dtype=torch.uint8, device=dev)
        t[in_off:in_off + raw.nbytes] = torch.from_numpy(np.ascontiguousarray(raw).view(np.uint8).copy()).to(dev)
        G.fill()
        torch.cuda.synchronize()
        sc.process(t.data_ptr() + in_off, n_out, G.ptr)
        h.sync()
        got = G.raw()
        G.check(P, ("call", k, n_out), got)
        out.append(G.view(got)[0].copy().view(REC))
        del t
    sc.close()
    h.close()
    return np.stack(out)


def _slices(raw, D, sizes):
    """Each call on its own slice of the stream."""
    per, pos, out = 2 * D, 0, []
    for n in sizes:
        out.append((raw[per * pos:per * (pos + n)], n))
        pos += n
    return out


_gpu = {}


def _levels(fmx, torch, fmt, D):
    """The GPU run of the coloured capture in _sizes' calls, once per session."""
    if (fmt, D) not in _gpu:
        sizes = _sizes(GEO[D][0])
        raw = _capture(fmt, D, sum(sizes) * D)
        _gpu[(fmt, D)] = run_scan(fmx, torch, _scfg(fmx, fmt, D), _slices(raw, D, sizes))
    return _gpu[(fmt, D)]


def _compare(tag, got, want):
    """got: REC [P]; want: wb_scan_ref.scan_call's dicts.  Logs and returns the worst errors."""
    ref_rms = S.rms_of([w["dbfs"] for w in want])
    rms_err = np.abs(S.rms_of(got["dbfs"]) - ref_rms)
    loud = ref_rms >= 1e-3
    db_err = np.abs(got["dbfs"] - np.array([w["dbfs"] for w in want]))
    cdb_err = np.abs(got["compensated_dbfs"] - np.array([w["compensated_dbfs"] for w in want]))
    lv_err = np.abs(got["level120"].astype(np.float64) - np.array([w["level120"] for w in want]))
    st = dict(scan_rms_err=float(rms_err.max()), scan_db_err_loud=float(db_err[loud].max()) if loud.any() else 0.0,
              scan_cdb_err_loud=float(cdb_err[loud].max()) if loud.any() else 0.0,
              scan_level_err_loud=float(lv_err[loud].max()) if loud.any() else 0.0, loud_points=int(loud.sum()),
              groups_oracle=[])
    log_errors(tag, int(np.argmax(rms_err)), st)
    return st


@pytest.mark.parametrize("fmt", ["s16", "u8"])
@pytest.mark.parametrize("D", [10, 25, 100])
def test_levels_against_float64(fmx, oracle, torch_cuda, fmt, D):
    """19 points (a ragged second group) at -900 k / 100 k (D = 10, tpp 28),
    -2.7 M / 300 k (D = 25, tpp 12: an odd D) and -11.7 M / 1.3 M (D = 100,
    tpp 28), the coloured capture, calls of 4096, 333, tpp + 17 and tpp + 1
    outputs on slices of their own: every point's |rms - rms_ref| < 1e-5, and
    < 0.09 dB / 0.29 of level120 where rms_ref >= 1e-3; clip ratios exact.
    Achieved (worst point and call, rms / dB / level120): s16 D = 10 6.5e-8 /
    4.5e-5 / 8.2e-5, D = 25 3.6e-8 / 3.8e-6 / 1.3e-5, D = 100 4.8e-8 / 5.9e-6 /
    2.3e-5; u8 D = 10 3.0e-8 / 1.4e-5 / 4.6e-5, D = 25 5.0e-8 / 5.7e-6 /
    1.9e-5, D = 100 6.7e-8 / 4.2e-6 / 1.1e-5 (profiles/wb_scan_parity_errors.jsonl)."""
    tpp, start, step = GEO[D]
    sizes = _sizes(tpp)
    raw = _capture(fmt, D, sum(sizes) * D)
    got = _levels(fmx, torch_cuda, fmt, D)
    freqs = S.points(start, step, NP)
    sm = [oracle.SignalSmoother() for _ in range(NP)]
    for k, (seg, n) in enumerate(_slices(raw, D, sizes)):
        want = S.scan_call(seg, FMT[fmt], D, tpp, D * DSP, freqs, n)
        st = _compare(f"wb_scan_{fmt}_D{D}_n{n}", got[k], want)
        assert st["scan_rms_err"] < RMS_TOL, (k, st)
        assert st["scan_db_err_loud"] < DB_TOL and st["scan_cdb_err_loud"] < DB_TOL, (k, st)
        assert st["scan_level_err_loud"] < LEVEL_TOL, (k, st)
        assert st["loud_points"] >= 3, st  # the tones above u8's quantisation step at least
        assert np.all(got[k]["hard_clip_ratio"] == want[0]["hard_clip_ratio"])
        assert np.all(got[k]["near_clip_ratio"] == want[0]["near_clip_ratio"])
        for p in range(NP):
            assert abs(float(got[k]["level120_smoothed"][p]) - sm[p](want[p]["level120"])) < LEVEL_TOL, (k, p)
    # the capture is coloured: the check can tell a point mix-up or a conjugate
    d0 = got[0]["dbfs"]
    assert np.argmax(d0) == TONE_POINTS[0] and d0[TONE_POINTS[0]] - d0[NP - 1 - TONE_POINTS[0]] > 20.0


@pytest.mark.parametrize("fmt,D", [("s16", 10), ("u8", 25), ("s16", 100)])
def test_records_do_not_depend_on_the_plan(fmx, torch_cuda, fmt, D):
    """The frequencies shared by the 19-point plan, a 5-point plan (start + 2
    steps, every third point) and a 1-point plan (point 11): bit-identical
    records."""
    tpp, start, step = GEO[D]
    raw = _capture(fmt, D, sum(_sizes(tpp)) * D)
    call = [(raw[:2 * D * 4096], 4096)]
    full = _levels(fmx, torch_cuda, fmt, D)[0]
    five = run_scan(fmx, torch_cuda, _scfg(fmx, fmt, D, start=start + 2 * step, step=3 * step, n=5), call)[0]
    one = run_scan(fmx, torch_cuda, _scfg(fmx, fmt, D, start=start + 11 * step, n=1), call)[0]
    assert five.tobytes() == full[[2, 5, 8, 11, 14]].tobytes()
    assert one.tobytes() == full[[11]].tobytes()


def test_two_fresh_objects_agree_bit_for_bit(fmx, torch_cuda):
    tpp = GEO[10][0]
    sizes = _sizes(tpp)
    raw = _capture("s16", 10, sum(sizes) * 10)
    again = run_scan(fmx, torch_cuda, _scfg(fmx, "s16", 10), _slices(raw, 10, sizes))
    assert again.tobytes() == _levels(fmx, torch_cuda, "s16", 10).tobytes()


@pytest.mark.parametrize("fmt,D", [("u8", 10), ("s16", 10), ("u8", 25), ("s16", 100)])
def test_input_bounds_and_geometry(fmx, torch_cuda, fmt, D):
    """Calls of 333 and tpp + 1 outputs: with full-scale garbage behind the
    n_out * D samples instead of the stream's continuation, and with the input
    one element into its allocation (the element-load path), the records'
    bits are those of the plain call.  The guard cells around d_level are
    checked in every run of this file (run_scan)."""
    tpp = GEO[D][0]
    raw = _capture(fmt, D, sum(_sizes(tpp)) * D)
    rng = np.random.default_rng(9)
    lim = (0, 255) if FMT[fmt] == R.U8 else (-32768, 32767)
    for n in (333, tpp + 1):
        plain = run_scan(fmx, torch_cuda, _scfg(fmx, fmt, D), [(raw[:2 * D * (n + 64)], n)])
        junk = np.concatenate([raw[:2 * D * n], rng.choice(lim, 2 * D * 64).astype(raw.dtype)])
        fenced = run_scan(fmx, torch_cuda, _scfg(fmx, fmt, D), [(junk, n)])
        skewed = run_scan(fmx, torch_cuda, _scfg(fmx, fmt, D), [(junk, n)], in_off=raw.itemsize)
        assert fenced.tobytes() == plain.tobytes(), n
        assert skewed.tobytes() == plain.tobytes(), n


@pytest.mark.parametrize("fmt", ["u8", "s16"])
def test_smoother_parameters_and_clip_ratios(fmx, oracle, torch_cuda, fmt):
    """Three calls of 1024 outputs, the capture scaled by 1, 0.25 and 2 (the
    last clips), non-default signal parameters: level120_smoothed within 0.29
    of the float32 smoother run over the reference's levels, clip ratios exact
    (and non-zero in the third call); after fmx_wb_scan_reset a fourth call of
    the first input gives the first call's records again."""
    D, n = 10, 1024
    tpp, start, step = GEO[D]
    raws = [_capture(fmt, D, n * D, seed=3, amps=CLIP_AMP, scale=s) for s in (1.0, 0.25, 2.0)]
    calls = [(r, n) for r in raws] + [(raws[0], n)]
    got = run_scan(fmx, torch_cuda, _scfg(fmx, fmt, D, block=n), calls, params=PARAMS, reset_before=(3,))
    freqs = S.points(start, step, NP)
    sm = [oracle.SignalSmoother() for _ in range(NP)]
    for k in range(3):
        want = S.scan_call(raws[k], FMT[fmt], D, tpp, D * DSP, freqs, n, PARAMS)
        st = _compare(f"wb_scan_smoother_{fmt}_call{k}", got[k], want)
        assert st["scan_rms_err"] < RMS_TOL and st["scan_level_err_loud"] < LEVEL_TOL, (k, st)
        assert np.all(got[k]["hard_clip_ratio"] == want[0]["hard_clip_ratio"]), k
        assert np.all(got[k]["near_clip_ratio"] == want[0]["near_clip_ratio"]), k
        for p in range(NP):
            s = sm[p](want[p]["level120"])
            assert abs(float(got[k]["level120_smoothed"][p]) - s) < LEVEL_TOL, (k, p, got[k][p], s)
    assert got[2]["hard_clip_ratio"][0] > 0.0 and got[0]["hard_clip_ratio"][0] == 0.0
    assert got[2]["near_clip_ratio"][0] > got[2]["hard_clip_ratio"][0]
    # the smoother moved: the second call's smoothed level lies between the two levels
    p = TONE_POINTS[0]
    assert got[1]["level120"][p] < got[1]["level120_smoothed"][p] < got[0]["level120"][p]
    assert got[3].tobytes() == got[0].tobytes()


def test_errors(fmx, torch_cuda):
    torch = torch_cuda
    L = fmx.lib()
    h = fmx.Handle(fmx.make_config(iq_rate=DSP, dsp_rate=DSP), 1)
    scfg = fmx.make_wb_scan_config(block=64)  # D = 10, tpp 28
    sc = fmx.WidebandScan(h, scfg)
    buf = torch.zeros(4 * 65 * 10, dtype=torch.int16, device="cuda")
    out = torch.zeros(40 * 23, dtype=torch.uint8, device="cuda")
    assert L.fmx_wb_scan_process(sc.s, buf.data_ptr(), 28, out.data_ptr()) == -1   # n_out = tpp: FMX_E_INVALID
    assert b"fmx_wb_scan_process" in L.fmx_last_error(h.h)
    assert L.fmx_wb_scan_process(sc.s, buf.data_ptr(), 65, out.data_ptr()) == -4   # block + 1: FMX_E_CAPACITY
    assert L.fmx_wb_scan_process(sc.s, None, 64, out.data_ptr()) == -1
    assert L.fmx_wb_scan_process(sc.s, buf.data_ptr(), 64, None) == -1
    assert L.fmx_wb_scan_process(None, buf.data_ptr(), 64, out.data_ptr()) == -1
    h.sync()
    assert not out.cpu().numpy().any()  # nothing was written by the refused calls
    sc.process(buf.data_ptr(), 29, out.data_ptr())
    h.sync()
    s = C.c_void_p(1)
    assert L.fmx_wb_scan_create(None, C.byref(scfg), C.byref(s)) == -1 and s.value is None
    s = C.c_void_p(1)
    bad = fmx.make_wb_scan_config(step_hz=0)
    assert L.fmx_wb_scan_create(h.h, C.byref(bad), C.byref(s)) == -1 and s.value is None
    assert b"fmx_wb_scan" in L.fmx_last_error(h.h)
    assert L.fmx_wb_scan_destroy(None) == -1 and L.fmx_wb_scan_reset(None) == -1
    sc.close()
    h.close()


def test_a_receiver_that_tunes_itself(fmx, torch_cuda):
    """The band capture (four stations in one int16 2.4 MS/s capture): the scan
    of call 0 over 23 points at 100 kHz and fmx_scan_peaks(dbfs, -40, 1) give
    BAND_FREQ; three reads (calls 0, 1, 5) formatted by fmx_xdr_scan_line list
    all 23 points within 0.35 of the reference's mean level (0.29 and the
    one-decimal rounding); a Wideband created at the found frequencies,
    through fmx_demod and fmx_rds over the 24 calls, decodes on every channel
    a group whose error-free block A is 0x1000 + 700 + c."""
    torch = torch_cuda
    pw, raw = band_levels(fmx)
    n, D, per = R.BAND_N, R.BAND_D, 2 * R.BAND_N * R.BAND_D
    scfg = fmx.make_wb_scan_config(R.BAND_FS, R.BAND_DSP, fmx.FMX_WB_S16, 0, n, BAND_START, BAND_STEP, BAND_POINTS)
    freqs = fmx.wb_scan_points(scfg)
    got = run_scan(fmx, torch, scfg, [(raw[per * i:per * (i + 1)], n) for i in BAND_SCAN_CALLS])
    found = [freqs[i] for i in fmx.scan_peaks(got[0]["dbfs"], -40.0, 1)]
    assert found == list(R.BAND_FREQ), found
    want = np.array([[S.record(p)["level120"] for p in row] for row in pw])  # [3][23]
    for k in range(3):
        st = dict(scan_rms_err=float(np.max(np.abs(S.rms_of(got[k]["dbfs"]) - np.sqrt(0.5 * pw[k])))),
                  scan_level_err=float(np.max(np.abs(got[k]["level120"] - want[k]))), groups_oracle=[])
        log_errors("wb_scan_band", k, st)
        assert st["scan_rms_err"] < RMS_TOL, st
    line = fmx.xdr_scan_line([f // 1000 for f in freqs], got["level120"].astype(np.float64).sum(axis=0), [3] * len(freqs))
    print(line)
    cells = line[1:].split(",")
    assert line.startswith("U") and len(cells) == BAND_POINTS
    for cell, f, w in zip(cells, freqs, want.mean(axis=0)):
        khz, v = cell.split("=")
        assert int(khz) == f // 1000 and abs(float(v) - w) < 0.35, (cell, f, w)
    # tune to what the scan found
    Cn = len(found)
    dev = torch.device("cuda")
    h = fmx.Handle(fmx.make_config(bandwidth_hz=-1, deemphasis=1), Cn)
    wb = fmx.Wideband(h, fmx.make_wb_config(R.BAND_FS, R.BAND_DSP, fmx.FMX_WB_S16, 0, n), found)
    d_raw = torch.from_numpy(raw.copy()).to(dev)
    GS = 8
    bb = torch.zeros((Cn, 2 * n), dtype=torch.float32, device=dev)
    mpx = torch.zeros((Cn, n), dtype=torch.float32, device=dev)
    grp = torch.zeros((Cn, GS, 4), dtype=torch.int32, device=dev)
    gcnt = torch.zeros(Cn, dtype=torch.int32, device=dev)
    groups = [[] for _ in range(Cn)]
    for i in range(R.BAND_CALLS):
        wb.process(d_raw.data_ptr() + 4 * D * n * i, n, bb.data_ptr(), n)
        h.demod(bb.data_ptr(), 2 * n, n, mpx.data_ptr(), n)
        h.rds(mpx.data_ptr(), n, n, grp.data_ptr(), GS, gcnt.data_ptr())
        h.sync()
        for c, g in enumerate(H._groups_of(grp.cpu().numpy(), gcnt.cpu().numpy(), GS)):
            groups[c] += g
    wb.close()
    h.close()
    for c in range(Cn):
        good = [g for g in groups[c] if (g[4] >> 6) == 0]
        assert any(g[0] == 0x1000 + R.BAND_CH0 + c for g in good), (c, groups[c])
