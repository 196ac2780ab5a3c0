"""The band receiver's RF level on the GPU (fmx_wb_signal, kernel k_wb_level,
DESIGN.md section 21): one fmx_signal_level record per channel of the
channelizer from the rows of the call just queued, against float64 --
tests/wb_ref.py's channelizer over the whole stream since the reset, cut at
the call boundaries, P_c = mean |y|^2 of each slice, tests/wb_scan_ref.py's
record and clip_ratios, oracle.SignalSmoother.

Bars (tests/test_gpu_wb_scan.py's, for its reason: the rows' own bar is
max |d| < 1e-5, and an RMS difference cannot exceed that maximum):
|rms_gpu - rms_ref| < 1e-5 everywhere; < 0.09 dB and < 0.29 of level120 where
rms_ref >= 1e-3; clip ratios equal exactly.
Achieved (worst channel and call, rms / dB / level120;
profiles/wb_signal_parity_errors.jsonl): the six-channel capture int16 1.8e-8 /
7.5e-7 / 7.6e-6, u8 2.1e-8 / 2.4e-6 / 7.6e-6; D = 100 6.7e-8 / 2.8e-6 / 0; the
smoother test 2.0e-8 / 7.4e-7 / 7.6e-6; the band's 12 calls 8.5e-9 / 4.6e-7 /
7.6e-6."""
import ctypes as C
import functools

import numpy as np
import pytest

import gpu_harness as H
import wb_ref as R
import wb_scan_ref as S
from test_gpu_parity import log_errors
from test_gpu_wb_receiver import _capture as band_capture
from test_wb_signal import s_line

pytestmark = pytest.mark.gpu

RMS_TOL = 1e-5
DB_TOL, LEVEL_TOL = 0.09, 0.29  # what RMS_TOL comes to at rms_ref >= 1e-3
DSP, D, FS, TPP, B = 240_000, 10, 2_400_000, 28, 4096
FMT = {"u8": R.U8, "s16": R.S16}
EMPTY = 600_000
FREQS = (0, 123_457, -900_000, FS // 2, -FS // 2 + 1, EMPTY)
AMPS = (0.3, 0.1, 0.03, 0.01, 0.01)  # complex tones at the first five channels
SIZES = (4096, 333, 1, 17, 1028, 4096)
PARAMS = (12, 0.5, -2.0, -60.0, -15.0)
REC = np.dtype([("level120", "<f4"), ("level120_smoothed", "<f4"), ("dbfs", "<f8"), ("compensated_dbfs", "<f8"),
                ("hard_clip_ratio", "<f8"), ("near_clip_ratio", "<f8")])
assert REC.itemsize == 40
KEYS = ("pcm_l", "pcm_r", "count", "stereo", "pilot", "indicator", "clip", "gcount", "grp")


def quantise(x, fmt):
    if FMT[fmt] == R.U8:
        raw = np.empty(2 * len(x), np.uint8)
        q = lambda v: np.clip(np.rint(v * 127.5 + 127.5), 0, 255)  # noqa: E731
    else:
        raw = np.empty(2 * len(x), np.int16)
        q = lambda v: np.clip(np.rint(v * 32768.0), -32768, 32767)  # noqa: E731
    raw[0::2], raw[1::2] = q(x.real), q(x.imag)
    return raw


@functools.lru_cache(maxsize=None)
def _tones(fmt, n_samples, seed=1, scale=1.0, fs=FS, freqs=FREQS[:5], amps=AMPS):
    """Interleaved raw I/Q: complex tones of `amps` at `freqs` plus complex
    noise of RMS 1e-3 per component, times scale."""
    rng = np.random.default_rng(seed)
    i = np.arange(n_samples, dtype=np.int64)
    x = 1e-3 * (rng.normal(size=n_samples) + 1j * rng.normal(size=n_samples))
    for f, a in zip(freqs, amps):
        turns = ((f % fs) * (i % fs)) % fs
        x += a * np.exp(2j * np.pi * turns / fs)
    raw = quantise(x * scale, fmt)
    raw.setflags(write=False)
    return raw


def run_levels(fmx, torch, fmt, freqs, raw, sizes, mode, wide_rate=FS, tpp=0, block=B, events=None, level_cells=None):
    """The stream `raw` through one channelizer in calls of `sizes`, each with
    fmx_wb_signal behind it and a sync behind that.  mode "block":
    fmx_wb_process_block on a stereo + RDS handle of len(freqs) channels;
    "stage": fmx_wb_process into caller rows of an odd stride whose base is
    only 4-byte aligned.  events(i, handle, wideband) runs before call i.  The
    records live in a sentinel-guarded allocation checked after every call.
    -> records [len(sizes)][channels] (numpy, dtype REC)."""
    Cn, Dn = len(freqs), wide_rate // DSP
    dev = torch.device("cuda")
    h = fmx.Handle(fmx.make_config(iq_rate=DSP, dsp_rate=DSP, block=block, bandwidth_hz=-1, deemphasis=1), Cn)
    wb = fmx.Wideband(h, fmx.make_wb_config(wide_rate, DSP, FMT[fmt], tpp, block), list(freqs))
    G = H.Guarded(torch, "i32", 1, Cn if level_cells is None else level_cells, off=2, tail=21, cell=10)
    d_raw = torch.from_numpy(np.ascontiguousarray(raw).view(np.uint8).copy()).to(dev)
    per = 2 * raw.itemsize * Dn  # bytes of one output's wide samples
    if mode == "block":
        f = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)  # noqa: E731
        z = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)  # noqa: E731
        pl, pr, cnt = f(Cn, block), f(Cn, block), z(Cn)
        out = fmx.BlockOut(None, 0, pl.data_ptr(), pr.data_ptr(), block, cnt.data_ptr(), None, None, None, None, 0,
                           None, None, None)
    else:
        stride = block + 3  # odd
        rows = torch.zeros(1 + 2 * stride * Cn + 7, dtype=torch.float32, device=dev)
        d_rows = rows.data_ptr() + 4
        assert stride % 2 == 1 and d_rows % 8 == 4
    torch.cuda.synchronize()
    res, pos = [], 0
    for i, n in enumerate(sizes):
        if events:
            events(i, h, wb)
        G.fill()
        torch.cuda.synchronize()
        if mode == "block":
            wb.process_block(d_raw.data_ptr() + per * pos, n, out)
        else:
            wb.process(d_raw.data_ptr() + per * pos, n, d_rows, stride)
        wb.signal(G.ptr)
        h.sync()
        pos += n
        got = G.raw()
        G.check(Cn, ("call", i, n), got)
        res.append(G.view(got)[0][:10 * Cn].copy().view(REC))
    wb.close()
    h.close()
    return np.stack(res)


def reference(raw, fmt, sizes, freqs=FREQS, params=S.DEFAULT_PARAMS, wide_rate=FS, tpp=TPP):
    """Per call: wb_scan_ref.record of every channel's P_c (plus the call's
    clip ratios), from the float64 rows of the whole stream.  params: one
    tuple, or one per call."""
    Dn = wide_rate // DSP
    y = R.channelize(R.normalise(raw, FMT[fmt]), Dn, tpp, wide_rate, list(freqs))
    out, pos = [], 0
    for k, n in enumerate(sizes):
        pw = np.mean(np.abs(y[:, pos:pos + n]) ** 2, axis=1)
        hard, near = S.clip_ratios(raw[2 * Dn * pos:2 * Dn * (pos + n)], FMT[fmt])
        par = params[k] if isinstance(params[0], tuple) else params
        recs = [dict(S.record(p, par), hard_clip_ratio=hard, near_clip_ratio=near) for p in pw]
        out.append(recs)
        pos += n
    return out


def compare(tag, got, want):
    """got: REC [C]; want: reference()'s dicts of one call.  Logs the worst
    errors, asserts the bars and the exact clip ratios; -> rms_ref [C]."""
    ref_db = np.array([w["dbfs"] for w in want])
    ref_rms = S.rms_of(ref_db)
    rms_err = np.abs(S.rms_of(got["dbfs"]) - ref_rms)
    loud = ref_rms >= 1e-3
    db_err = np.abs(got["dbfs"] - ref_db)
    cdb_err = np.abs(got["compensated_dbfs"] - np.array([w["compensated_dbfs"] for w in want]))
    lv_err = np.abs(got["level120"].astype(np.float64) - np.array([w["level120"] for w in want]))
    worst = lambda e: float(e[loud].max()) if loud.any() else 0.0  # noqa: E731
    st = dict(level_rms_err=float(rms_err.max()), level_db_err_loud=worst(db_err), level_cdb_err_loud=worst(cdb_err),
              level_level_err_loud=worst(lv_err), loud_channels=int(loud.sum()), groups_oracle=[])
    log_errors(tag, int(np.argmax(rms_err)), st)
    assert st["level_rms_err"] < RMS_TOL, (tag, st)
    assert st["level_db_err_loud"] < DB_TOL and st["level_cdb_err_loud"] < DB_TOL, (tag, st)
    assert st["level_level_err_loud"] < LEVEL_TOL, (tag, st)
    assert np.all(got["hard_clip_ratio"] == want[0]["hard_clip_ratio"]), tag
    assert np.all(got["near_clip_ratio"] == want[0]["near_clip_ratio"]), tag
    return ref_rms


@pytest.mark.parametrize("fmt", ["s16", "u8"])
def test_levels_against_float64(fmx, oracle, torch_cuda, fmt):
    """6 channels (0, 123 457, -900 000, Fs / 2, -Fs / 2 + 1 Hz and the empty
    600 kHz) of a 2.4 MS/s capture with tones of 0.3 / 0.1 / 0.03 / 0.01 / 0.01
    at the first five and noise of RMS 1e-3 per component; calls of 4096, 333,
    1, 17, 1028 and 4096 outputs through fmx_wb_process_block (k_fecf and
    k_frontend calls, n = 1, n no multiple of the workgroup's 512 samples),
    fmx_wb_signal behind each: every record within the bars, the smoothed level
    within 0.29 of SignalSmoother fed the reference's levels.  The same stream
    on a second object through fmx_wb_process into caller rows of stride 4099
    at a base that is only 4-byte aligned: the same records, bit for bit (the
    rows are the same, and the sum's order depends on n alone)."""
    raw = _tones(fmt, sum(SIZES) * D)
    got = run_levels(fmx, torch_cuda, fmt, FREQS, raw, SIZES, "block")
    want = reference(raw, fmt, SIZES)
    sm = [oracle.SignalSmoother() for _ in FREQS]
    for k, n in enumerate(SIZES):
        ref_rms = compare(f"wb_signal_{fmt}_call{k}_n{n}", got[k], want[k])
        # the reference itself: every tuned channel is loud, the empty one is not
        assert np.all(ref_rms[:5] >= 7e-3) and ref_rms[5] < 1e-3, (k, ref_rms)
        for c in range(len(FREQS)):
            s = sm[c](want[k][c]["level120"])
            assert abs(float(got[k]["level120_smoothed"][c]) - s) < LEVEL_TOL, (k, c, got[k][c], s)
    assert np.argmax(got[0]["dbfs"]) == 0 and np.argmin(got[0]["dbfs"]) == 5  # no channel mix-up
    staged = run_levels(fmx, torch_cuda, fmt, FREQS, raw, SIZES, "stage")
    assert staged.tobytes() == got.tobytes()


def test_d100_many_clip_partials(fmx, oracle, torch_cuda):
    """D = 100 (24 MS/s, int16), 3 channels, one fmx_wb_process call of 1024
    outputs: 102 400 raw samples, 50 clip partials; within the bars."""
    fs, freqs, n = 100 * DSP, (0, 1_307_000, -11_700_000), 1024
    raw = _tones("s16", n * 100, seed=2, fs=fs, freqs=freqs, amps=AMPS[:3])
    got = run_levels(fmx, torch_cuda, "s16", freqs, raw, [n], "stage", wide_rate=fs, tpp=28, block=n)
    want = reference(raw, "s16", [n], freqs=freqs, wide_rate=fs, tpp=28)
    ref_rms = compare("wb_signal_s16_D100", got[0], want[0])
    assert np.all(ref_rms >= 1e-3), ref_rms
    assert got[0]["hard_clip_ratio"][0] == 0.0


@pytest.mark.parametrize("fmt", ["u8", "s16"])
def test_clip_ratios_exact(fmx, torch_cuda, fmt):
    """Two calls (333 and 4096 outputs); in the last one u8 bytes 0, 1, 8, 9,
    247, 254, 255 -- int16 values with those top bytes b = (v >> 8) + 128 --
    planted at known counts on I only, on Q only and on both: hard and near
    ratios equal clip_ratios of the call's raw samples and the counts planted,
    the same in every record; the first call has none."""
    sizes = [333, 4096]
    raw = _tones(fmt, sum(sizes) * D).copy()
    assert S.clip_ratios(raw, FMT[fmt]) == (0.0, 0.0)  # |x| <= 0.47: nothing clipped before the planting
    val = (lambda b: b) if FMT[fmt] == R.U8 else (lambda b: ((b - 128) << 8) + 37)
    base, pos = 333 * D, 0
    hard = near = 0
    for b, cnt in ((0, 3), (1, 5), (8, 7), (9, 11), (247, 13), (254, 2), (255, 9)):
        for where in ("i", "q", "both"):
            for _ in range(cnt):
                s = base + 17 + 23 * pos  # distinct samples of the last call, across its clip workgroups
                pos += 1
                if where in ("i", "both"):
                    raw[2 * s] = val(b)
                if where in ("q", "both"):
                    raw[2 * s + 1] = val(b)
            hard += cnt * (b <= 1 or b >= 254)
            near += cnt * (b <= 8 or b >= 247)
    assert 17 + 23 * pos < 4096 * D
    got = run_levels(fmx, torch_cuda, fmt, FREQS, raw, sizes, "stage")
    n_in = 4096 * D
    want = S.clip_ratios(raw[2 * base:], FMT[fmt])
    assert want == (hard / n_in, near / n_in) and hard > 0 and near > hard
    assert np.all(got[0]["hard_clip_ratio"] == 0.0) and np.all(got[0]["near_clip_ratio"] == 0.0)
    assert np.all(got[1]["hard_clip_ratio"] == want[0]) and np.all(got[1]["near_clip_ratio"] == want[1]), got[1]


def test_smoother_parameters_and_resets(fmx, oracle, torch_cuda):
    """Six calls of 1024 outputs (int16), the tones scaled by 0.25, 1, 1.5,
    0.25, 1, 0.5; calls 0 and 1 with the default signal parameters, from call
    2 on with (12, 0.5, -2, -60, -15), set between calls 1 and 2.  Records
    within the bars; level120_smoothed within 0.29 of SignalSmoother fed the
    reference's level120; on channel 2 (0.03: never clamped) the smoothed level
    lies between the old and the new level on the rise (call 1) and the fall
    (call 3).  fmx_wb_signal_reset(2) before call 4 restarts channel 2 alone
    (its smoothed level is its level120; the others' are not).  fmx_wb_reset
    and fmx_wb_set_freq before call 5 restart none."""
    n, scales = 1024, (0.25, 1.0, 1.5, 0.25, 1.0, 0.5)
    raws = [_tones("s16", n * D, seed=10 + k, scale=s) for k, s in enumerate(scales)]
    params = [S.DEFAULT_PARAMS] * 2 + [PARAMS] * 4

    def events(i, h, wb):
        if i == 2:
            wb.set_signal_params(*PARAMS)
        if i == 4:
            wb.signal_reset(2)
        if i == 5:
            wb.reset(0)
            wb.set_freq(1, FREQS[1])
    got = run_levels(fmx, torch_cuda, "s16", FREQS, np.concatenate(raws), [n] * 6, "block", block=n, events=events)
    # the reference's stream restarts with fmx_wb_reset before call 5
    want = reference(np.concatenate(raws[:5]), "s16", [n] * 5, params=params[:5])
    want += reference(raws[5], "s16", [n], params=PARAMS)
    sm = [oracle.SignalSmoother() for _ in FREQS]
    for k in range(6):
        compare(f"wb_signal_smoother_call{k}", got[k], want[k])
        if k == 4:
            sm[2] = oracle.SignalSmoother()
        for c in range(len(FREQS)):
            s = sm[c](want[k][c]["level120"])
            assert abs(float(got[k]["level120_smoothed"][c]) - s) < LEVEL_TOL, (k, c, got[k][c], s)
    lv, sv = got["level120"][:, 2], got["level120_smoothed"][:, 2]
    assert sv[0] == lv[0]
    assert lv[0] < sv[1] < lv[1]           # the rise
    assert lv[3] < sv[3] < sv[2]           # the fall
    assert sv[4] == lv[4]                  # restarted
    for c in (0, 1):                       # not restarted: still on their way up from call 3's level
        assert got["level120_smoothed"][4, c] < got["level120"][4, c] - 0.5, (c, got[4][c])
    for c in (0, 1, 2):                    # fmx_wb_reset / fmx_wb_set_freq restart none: on their way down
        assert got["level120_smoothed"][5, c] > got["level120"][5, c] + 1.0, (c, got[5][c])


def run_band(fmx, torch, raw, ncalls, sync, with_signal=True):
    """ncalls fmx_wb_process_block calls of 4096 of the band capture on 5
    channels, fmx_wb_signal behind each (or never); sync "each" or "end" (every
    call has output and level buffers of its own).  -> (per call dicts of
    KEYS, records [ncalls][5])."""
    freqs = list(R.BAND_FREQ) + [R.BAND_EMPTY]
    Cn, GS = len(freqs), 8
    dev = torch.device("cuda")
    h = fmx.Handle(fmx.make_config(iq_rate=DSP, dsp_rate=DSP, block=B, bandwidth_hz=-1, deemphasis=1), Cn)
    wb = fmx.Wideband(h, fmx.make_wb_config(R.BAND_FS, DSP, fmx.FMX_WB_S16, 0, B), freqs)
    f = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)  # noqa: E731
    z = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)  # noqa: E731
    ns = ncalls
    T = dict(pcm_l=f(ns, Cn, B), pcm_r=f(ns, Cn, B), clip=f(ns, Cn), count=z(ns, Cn), stereo=z(ns, Cn),
             pilot=z(ns, Cn), indicator=z(ns, Cn), gcount=z(ns, Cn), grp=z(ns, Cn, GS, 4))
    lev = torch.zeros((ns, Cn * 40), dtype=torch.uint8, device=dev)
    d_raw = torch.from_numpy(raw).to(dev)
    torch.cuda.synchronize()
    for i in range(ncalls):
        out = fmx.BlockOut(None, 0, T["pcm_l"][i].data_ptr(), T["pcm_r"][i].data_ptr(), B, T["count"][i].data_ptr(),
                           T["stereo"][i].data_ptr(), T["pilot"][i].data_ptr(), T["clip"][i].data_ptr(),
                           T["grp"][i].data_ptr(), GS, T["gcount"][i].data_ptr(), None, T["indicator"][i].data_ptr())
        wb.process_block(d_raw.data_ptr() + 4 * R.BAND_D * B * i, B, out)
        if with_signal:
            wb.signal(lev[i].data_ptr())
        if sync == "each":
            h.sync()
    h.sync()
    host = {k: v.cpu().numpy() for k, v in T.items()}
    recs = lev.cpu().numpy().view(REC)
    wb.close()
    h.close()
    res = []
    for i in range(ncalls):
        r = {k: host[k][i].copy() for k in KEYS}
        for c in range(Cn):  # cells past a row's logical length are never written: not part of the output
            r["pcm_l"][c, int(r["count"][c]):] = 0.0
            r["pcm_r"][c, int(r["count"][c]):] = 0.0
            r["grp"][c, min(int(r["gcount"][c]), GS):] = 0
        res.append(r)
    return res, recs


def test_queued_calls_and_unchanged_outputs(fmx, torch_cuda):
    """12 fmx_wb_process_block calls of the band capture (four stations and an
    empty channel), fmx_wb_signal behind each: one sync behind the last call,
    a sync after every call, and the first again on a fresh handle give
    bit-identical records; PCM, counts, stereo flags, pilot, indicator, clip
    ratio and RDS groups are bit-identical to a run that never calls
    fmx_wb_signal.  The records are within the bars of the float64 rows; the
    stations' dbfs is ordered as their amplitudes 0.30 > 0.25 > 0.12 > 0.06
    with the empty channel below station 3; fmx_xdr_signal_line of a station's
    smoothed level and stereo indicator parses back to the level rounded to a
    tenth."""
    ncalls = 12
    raw_all, ref = band_capture()
    raw = raw_all[:2 * R.BAND_D * B * ncalls]
    out_end, rec_end = run_band(fmx, torch_cuda, raw, ncalls, "end")
    out_each, rec_each = run_band(fmx, torch_cuda, raw, ncalls, "each")
    out_again, rec_again = run_band(fmx, torch_cuda, raw, ncalls, "end")
    out_plain, _ = run_band(fmx, torch_cuda, raw, ncalls, "end", with_signal=False)
    assert rec_end.tobytes() == rec_each.tobytes() == rec_again.tobytes()
    for other in (out_each, out_again, out_plain):
        for i, (x, y) in enumerate(zip(out_end, other)):
            for key in KEYS:
                assert np.array_equal(x[key].view(np.uint32), y[key].view(np.uint32)), (i, key)
    assert all(int(r["count"].min()) > 0 for r in out_end)  # the receiver ran
    hard, near = S.clip_ratios(raw, R.S16)
    assert (hard, near) == (0.0, 0.0)
    for i in range(ncalls):
        pw = np.mean(np.abs(ref[:, B * i:B * (i + 1)]) ** 2, axis=1)
        want = [dict(S.record(p), hard_clip_ratio=0.0, near_clip_ratio=0.0) for p in pw]
        compare(f"wb_signal_band_call{i}", rec_end[i], want)
        d = rec_end[i]["dbfs"]
        assert d[0] > d[2] > d[1] > d[3] > d[4], (i, d)
        for c in range(4):
            lvl, ind = float(rec_end[i]["level120_smoothed"][c]), int(out_end[i]["indicator"][c])
            line = fmx.xdr_signal_line(lvl, ind, False)
            assert line == s_line(lvl, ind, 0, -1, -1), (i, c, line)
            assert line[0] == "S" and line[1] == ("s" if ind else "m") and line.endswith(",-1,-1\n"), line
            assert abs(float(line[2:].split(",")[0]) - lvl) <= 0.05 + 1e-4, (line, lvl)


def test_errors_and_untouched_cells(fmx, torch_cuda):
    """FMX_E_INVALID with fmx_wb_signal in the message: before any call, after
    only an n == 0 call, for a NULL d_level, for one misaligned by 4, and for
    a second fmx_wb_signal behind the same call; the refused calls write
    nothing and leave the call measurable.  A d_level array longer than
    n_channels keeps its pattern outside [0, n_channels)."""
    torch = torch_cuda
    L = fmx.lib()
    Cn = 3
    raw = _tones("s16", sum(SIZES) * D)
    h = fmx.Handle(fmx.make_config(iq_rate=DSP, dsp_rate=DSP, block=B), Cn)
    wb = fmx.Wideband(h, fmx.make_wb_config(FS, DSP, fmx.FMX_WB_S16, 0, B), list(FREQS[:3]))
    d_raw = torch.from_numpy(raw.copy()).to("cuda")
    stride = 513  # rows at a base that is 8-byte aligned only: the third load width
    buf = torch.zeros(2 + 2 * stride * Cn, dtype=torch.float32, device="cuda")
    d_rows = buf.data_ptr() + 8
    assert d_rows % 16 == 8
    G = H.Guarded(torch, "i32", 1, Cn + 4, off=2, tail=21, cell=10)

    def refused(ptr):
        rc = L.fmx_wb_signal(wb.w, C.c_void_p(ptr) if ptr is not None else None)
        msg = L.fmx_last_error(h.h)
        assert rc == -1 and b"fmx_wb_signal" in msg, (rc, msg)
    refused(G.ptr)                                       # before any call
    wb.process(d_raw.data_ptr(), 0, d_rows, stride)
    refused(G.ptr)                                       # an n == 0 call does not count
    wb.process(d_raw.data_ptr(), 512, d_rows, stride)
    refused(None)
    refused(G.ptr + 4)
    assert L.fmx_wb_signal_reset(wb.w, Cn) == -1 and L.fmx_wb_signal_reset(wb.w, -2) == -1
    assert b"fmx_wb_signal_reset" in L.fmx_last_error(h.h)
    h.sync()
    G.check(0, "refused calls")                          # nothing was written
    wb.signal(G.ptr)                                     # the refusals left the call measurable
    refused(G.ptr)                                       # twice in a row
    wb.process(d_raw.data_ptr() + 4 * D * 512, 0, d_rows, stride)
    refused(G.ptr)                                       # an n == 0 call in between changes nothing
    h.sync()
    got = G.raw()
    G.check(Cn, "longer array", got)
    rec = G.view(got)[0][:10 * Cn].copy().view(REC)
    want = reference(raw[:2 * D * 512], "s16", [512], freqs=FREQS[:3])
    compare("wb_signal_errors_call", rec, want[0])
    wb.close()
    h.close()
