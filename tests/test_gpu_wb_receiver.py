"""The band receiver in one call (fmx_wb_process_block):
one wide IQ capture in, every station's MPX, PCM, stereo state and RDS groups
out, on the pipelined step's four streams -- k_wb -> k_fecf -> k_pilot | k_rs
-> k_rds | k_pll | k_bits -> k_audio, or k_frontend on the rows for the call
shapes k_fecf does not take.

The band is tests/wb_ref.py's (section 18: four synthetic stations in one
int16 2.4 MS/s capture); the reference is the oracle's objects fed the float64
channelizer's rows, PCM clamped to [-1, 1] as main.cpp:1303-1308 clamps it
(the clamp oracle_pipeline_block, and so gpu_harness.run_oracle_pipeline,
applies; OracleChannel's afpost has none).  Bars: those
test_gpu_wideband.test_band_receiver_end_to_end holds the five stage calls to
(test_gpu_parity's MPX / PCM tolerances, twice those for station 3, whose
amplitude is half of station 1's while the channelizer's absolute error is the
same).  tests/test_wb_design.py shows on the CPU that the oracle decides this
band the same way under ten times the channelizer's error.
Achieved (worst channel, profiles/wb_receiver_parity_errors.jsonl): MPX max
4.7e-6 / RMS 3.1e-7 and PCM max 1.3e-5 / RMS 1.2e-6 in whole blocks; 6.0e-6 /
3.9e-7 and 1.6e-5 / 1.7e-6 over the ragged calls on either front end."""
import functools

import numpy as np
import pytest

import gpu_harness as H
import rds_wave as W
import wb_ref as R
from test_gpu_parity import MPX_MAX_TOL, MPX_RMS_TOL, PCM_MAX_TOL, PCM_RMS_TOL, log_errors

pytestmark = pytest.mark.gpu

B = R.BAND_N
DSP = R.BAND_DSP
GS = 8
UNIFORM = [B] * R.BAND_CALLS
# 1024: the smallest k_fecf call; 1028: a chunk that is no multiple of 8; 2052:
# two unequal chunks (1032 + 1020); 333, 1, 17, 1025: k_frontend calls -- each
# switch hands the carried state across kernels; 3000: two chunks again; then
# whole blocks and the capture's last 3808 samples
RAGGED = [4096, 1024, 1028, 2052, 333, 1, 17, 1025, 3000]
RAGGED = RAGGED + [B] * ((R.BAND_CALLS * B - sum(RAGGED)) // B)
RAGGED = RAGGED + [R.BAND_CALLS * B - sum(RAGGED)]
assert RAGGED[-1] == 3808 and sum(RAGGED) == R.BAND_CALLS * B
KEYS = ("mpx", "pcm_l", "pcm_r", "count", "stereo", "pilot", "indicator", "clip", "gcount", "grp")


@functools.lru_cache(maxsize=None)
def _capture():
    import fmx
    raw = R.band_capture(fmx)
    return raw, R.band_reference(raw)


def _handle(fmx, C, **kw):
    cfg = dict(iq_rate=DSP, dsp_rate=DSP, block=B, bandwidth_hz=-1, deemphasis=1)  # objects as constructed
    cfg.update(kw)
    return fmx.Handle(fmx.make_config(**cfg), C)


def _wideband(fmx, h, freqs, block=B):
    return fmx.Wideband(h, fmx.make_wb_config(R.BAND_FS, DSP, fmx.FMX_WB_S16, 0, block), list(freqs))


def run_rx(fmx, torch, raw, sizes, freqs=R.BAND_FREQ, sync="each", generic=False, events=None, ktimes=None, **cfg):
    """The capture through fmx_wb_process_block in calls of `sizes` outputs.
    sync: "each" (fmx_sync after every call), "third" (after every third call,
    three rotating output sets, as bench.py rotates them) or "end" (one
    fmx_sync behind the last call; every call has output buffers of its own --
    a copy-out between queued calls would not be ordered behind the handle's
    streams).  events(i, handle, wideband) runs before call i.  -> per call
    dicts of host arrays (KEYS; mpx cut to n columns) plus "groups"."""
    C, D = len(freqs), R.BAND_D
    dev = torch.device("cuda")
    h = _handle(fmx, C, **cfg)
    wb = _wideband(fmx, h, freqs)
    if generic:
        h.diag_set(fmx.FMX_DIAG_FE_GENERIC, 1)
    if ktimes is not None:
        h.timing_enable(True)
    every = {"each": 1, "third": 3, "end": len(sizes)}[sync]
    ns = len(sizes) if sync == "end" else 3
    f = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)  # noqa: E731
    z = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)  # noqa: E731
    T = dict(mpx=f(ns, C, B), pcm_l=f(ns, C, B), pcm_r=f(ns, C, B), clip=f(ns, C), count=z(ns, C), stereo=z(ns, C),
             pilot=z(ns, C), indicator=z(ns, C), gcount=z(ns, C), grp=z(ns, C, GS, 4))
    d_raw = torch.from_numpy(raw).to(dev)
    torch.cuda.synchronize()
    res, pend, pos = [None] * len(sizes), [], 0
    for i, n in enumerate(sizes):
        if events:
            events(i, h, wb)
        k = i % ns
        out = fmx.BlockOut(T["mpx"][k].data_ptr(), B, T["pcm_l"][k].data_ptr(), T["pcm_r"][k].data_ptr(), B,
                           T["count"][k].data_ptr(), T["stereo"][k].data_ptr(), T["pilot"][k].data_ptr(),
                           T["clip"][k].data_ptr(), T["grp"][k].data_ptr(), GS, T["gcount"][k].data_ptr(), None,
                           T["indicator"][k].data_ptr())
        wb.process_block(d_raw.data_ptr() + 4 * D * pos, n, out)
        pend.append((i, k, n))
        pos += n
        if (i + 1) % every == 0 or i + 1 == len(sizes):
            h.sync()
            host = {key: v.cpu().numpy() for key, v in T.items()}
            for (j, kk, nn) in pend:
                r = {key: host[key][kk].copy() for key in KEYS}
                r["mpx"] = r["mpx"][:, :nn].copy()
                r["groups"] = H._groups_of(r["grp"], r["gcount"], GS)
                for c in range(C):  # cells past a row's logical length are never written: not part of the output
                    r["pcm_l"][c, int(r["count"][c]):] = 0.0
                    r["pcm_r"][c, int(r["count"][c]):] = 0.0
                    r["grp"][c, min(int(r["gcount"][c]), GS):] = 0
                res[j] = r
            pend = []
    if ktimes is not None:
        ktimes.update(h.kernel_times())
    wb.close()
    h.close()
    return res


def oracle_cut(oracle, rows, sizes, reset_before=None, rows_after=None, mono=False):
    """One channel's baseband row (complex) through the oracle's demod ->
    stereo -> afpost -> rds (mono: demod alone, its mono output the PCM) in
    calls of `sizes`, PCM clamped to [-1, 1]; the channel is reset before call
    `reset_before` and reads rows_after from there on."""
    def inter(v):
        v = np.asarray(v, dtype=np.complex128)
        fl = np.empty(2 * v.size, np.float32)
        fl[0::2], fl[1::2] = v.real, v.imag
        return fl
    fa, fb = inter(rows), (inter(rows_after) if rows_after is not None else None)
    ch = H.OracleChannel(oracle)
    out, pos = [], 0
    for i, n in enumerate(sizes):
        if reset_before is not None and i == reset_before:
            ch.reset()
        src = fb if (fb is not None and reset_before is not None and i >= reset_before) else fa
        mpx, mono_out = ch.demod(src[2 * pos:2 * (pos + n)], n)
        mpx = mpx.copy()
        if mono:
            # the reference's mono block: both channels FMDemod's mono output x 0.5f, then the clamp
            # (oracle_pipeline_block's !cfg.stereo branch; fmx_process_block's mono step does the same)
            pl = pr = np.clip(mono_out * np.float32(0.5), np.float32(-1.0), np.float32(1.0))
            st, pil, groups = 0, 0, []
        else:
            l, r, st, pil = ch.stereo(mpx, n)
            pl, pr = ch.afpost(l, r, n, n)
            pl = np.clip(pl.copy(), np.float32(-1.0), np.float32(1.0))
            pr = np.clip(pr.copy(), np.float32(-1.0), np.float32(1.0))
            groups = ch.rds_groups(mpx, n)
        out.append(dict(mpx=mpx, pcm_l=pl, pcm_r=pr, stereo=st, pilot=pil, groups=groups))
        pos += n
    ch.close()
    return out


@functools.lru_cache(maxsize=None)
def _oracle(sizes, mono=False):
    """The four stations' oracle outputs for one cut of the capture, once per session."""
    import oracle
    _, ref = _capture()
    return W.pmap(lambda c: oracle_cut(oracle, ref[c].astype(np.complex64), list(sizes), mono=mono), range(4))


def check_channel(tag, c, g, o, sizes, k, gc=None, mpx_from=R.BAND_HEAD, pcm_from=2 * B, exact_from=None, first=0,
                  pi=None):
    """GPU run g (channel gc of it) against one channel's oracle calls o from
    call `first` on: groups and PCM counts equal call by call, MPX from DSP
    sample mpx_from on and PCM of the calls that start at DSP sample pcm_from
    or later within k times test_gpu_parity's bars; stereo flag and pilot
    tenths exact in the calls that start at sample exact_from or later."""
    gc = c if gc is None else gc
    start = np.concatenate([[0], np.cumsum(sizes)])
    dm, dp, ngroups = [], [], 0
    for i in range(first, len(sizes)):
        assert g[i]["groups"][gc] == o[i]["groups"], (tag, c, i, g[i]["groups"][gc], o[i]["groups"])
        for grp in o[i]["groups"]:
            if pi is not None and (grp[4] >> 6) == 0:
                assert grp[0] == pi, (tag, c, i, grp)
        ngroups += len(o[i]["groups"])
        m = len(o[i]["pcm_l"])
        assert int(g[i]["count"][gc]) == m, (tag, c, i, int(g[i]["count"][gc]), m)
        d = o[i]["mpx"] - g[i]["mpx"][gc]
        dm.append(d[max(0, mpx_from - int(start[i])):])
        if start[i] >= pcm_from:
            dp += [o[i]["pcm_l"] - g[i]["pcm_l"][gc, :m], o[i]["pcm_r"] - g[i]["pcm_r"][gc, :m]]
        if exact_from is not None and start[i] >= exact_from:
            got = (int(g[i]["stereo"][gc]), int(g[i]["pilot"][gc]))
            assert got == (o[i]["stereo"], o[i]["pilot"]), (tag, c, i, got, o[i]["stereo"], o[i]["pilot"])
    dm, dp = np.concatenate(dm).astype(np.float64), np.concatenate(dp).astype(np.float64)
    st = dict(mpx_max=float(np.max(np.abs(dm))), mpx_rms=float(np.sqrt(np.mean(dm * dm))),
              pcm_max=float(np.max(np.abs(dp))), pcm_rms=float(np.sqrt(np.mean(dp * dp))), groups_oracle=[])
    log_errors(tag, c, st)
    assert st["mpx_rms"] < k * MPX_RMS_TOL and st["mpx_max"] < k * MPX_MAX_TOL, (tag, c, st)
    assert st["pcm_rms"] < k * PCM_RMS_TOL and st["pcm_max"] < k * PCM_MAX_TOL, (tag, c, st)
    return ngroups


_runs = {}


def _one_call_run(fmx, torch):
    """Test 1's run (a sync after every third call, three output sets), once per session."""
    if "third" not in _runs:
        kt = {}
        _runs["third"] = (run_rx(fmx, torch, _capture()[0], UNIFORM, sync="third", ktimes=kt), kt)
    return _runs["third"]


def _same(a, b, chans=None):
    for i, (x, y) in enumerate(zip(a, b)):
        for key in KEYS:
            u, v = (x[key], y[key]) if chans is None else (x[key][chans], y[key][chans])
            assert np.array_equal(u.view(np.uint32), v.view(np.uint32)), (i, key)


def test_band_receiver_one_call(fmx, oracle, torch_cuda):
    """24 calls of 4096 on a 4-channel handle, a sync after every third call,
    three rotating output sets: groups equal call by call with PI 0x1000 +
    station, counts equal, stereo flag and pilot exact from call 2 on, MPX from
    output 128 on and PCM from call 2 on at test_band_receiver_end_to_end's
    bars; the fast path ran (k_fecf, k_pilot and k_rs launched, k_frontend
    never)."""
    g, kt = _one_call_run(fmx, torch_cuda)
    ora = _oracle(tuple(UNIFORM))
    ngroups = 0
    for c in range(4):
        ngroups += check_channel("wb_receiver_one_call", c, g, ora[c], UNIFORM, 2.0 if c == 3 else 1.0,
                                 exact_from=2 * B, pi=0x1000 + R.BAND_CH0 + c)
        assert ora[c][-1]["stereo"] == 1, c
        assert all(float(r["clip"][c]) == 0.0 for r in g), c  # |rows| <= 0.3: no sample near full scale
    assert ngroups >= 8
    print("KERNEL_TIMES", kt)
    for name in ("frontend", "pilot", "rs"):
        assert kt[name][1] == len(UNIFORM), (name, kt)
    assert kt["frontend_generic"][1] == 0, kt


@pytest.mark.parametrize("generic", [False, True], ids=["fecf", "generic"])
def test_ragged_calls_and_both_front_ends(fmx, oracle, torch_cuda, generic):
    """The capture in calls of 4096, 1024, 1028, 2052, 333, 1, 17, 1025, 3000,
    twenty of 4096 and the last 3808, the oracle cut the same way: groups and
    counts equal call by call, MPX from output 128 on, PCM of the calls from
    DSP sample 8192 on, at the same bars; then the same stream with
    FMX_DIAG_FE_GENERIC (k_frontend for every call)."""
    kt = {}
    g = run_rx(fmx, torch_cuda, _capture()[0], RAGGED, sync="each", generic=generic, ktimes=kt)
    ora = _oracle(tuple(RAGGED))
    for c in range(4):
        check_channel("wb_receiver_ragged_" + ("generic" if generic else "fecf"), c, g, ora[c], RAGGED,
                      2.0 if c == 3 else 1.0, pi=0x1000 + R.BAND_CH0 + c)
    fast = sum(1 for n in RAGGED if n >= 1024 and n % 4 == 0)
    assert kt["frontend"][1] == (0 if generic else fast), kt
    assert kt["frontend_generic"][1] == (len(RAGGED) if generic else len(RAGGED) - fast), kt


def test_outputs_do_not_depend_on_queuing_or_the_run(fmx, torch_cuda):
    """Test 1's stream with a sync after every call, with one sync behind the
    last call (every call queued ahead), with a sync after every third call on
    three rotating output sets (test 1's own run) and the last again on a
    fresh handle and channelizer: every output bit-identical, MPX included."""
    raw = _capture()[0]
    third, _ = _one_call_run(fmx, torch_cuda)
    _same(third, run_rx(fmx, torch_cuda, raw, UNIFORM, sync="each"))
    _same(third, run_rx(fmx, torch_cuda, raw, UNIFORM, sync="end"))
    _same(third, run_rx(fmx, torch_cuda, raw, UNIFORM, sync="third"))


def test_retune_between_queued_calls(fmx, oracle, torch_cuda):
    """5 channels, channel 4 at the empty frequency; before call 8, with no
    sync around it, fmx_wb_set_freq(4, station 1's frequency) and fmx_reset(4).
    From call 8 on channel 4 matches an OracleChannel reset at that call and
    fed the float64 rows of a channel that was always at that frequency (MPX
    head skipped again, PCM and the exact stereo flag / pilot from call 10 on);
    channels 0-3 are bit-identical to the run without the retune."""
    raw, ref = _capture()
    freqs = list(R.BAND_FREQ) + [R.BAND_EMPTY]

    def retune(i, h, wb):
        if i == 8:
            wb.set_freq(4, R.BAND_FREQ[1])
            h.reset(4)
    plain = run_rx(fmx, torch_cuda, raw, UNIFORM, freqs=freqs, sync="end")
    tuned = run_rx(fmx, torch_cuda, raw, UNIFORM, freqs=freqs, sync="end", events=retune)
    _same(plain, tuned, chans=slice(0, 4))
    _same(plain[:8], tuned[:8])
    o = oracle_cut(oracle, ref[4].astype(np.complex64), UNIFORM, reset_before=8, rows_after=ref[1].astype(np.complex64))
    n = check_channel("wb_receiver_retune", 1, tuned, o, UNIFORM, 1.0, gc=4, mpx_from=8 * B + R.BAND_HEAD,
                      pcm_from=10 * B, exact_from=10 * B, first=8, pi=0x1000 + R.BAND_CH0 + 1)
    assert n >= 1
    assert o[-1]["stereo"] == 1


def test_mono_without_rds(fmx, oracle, torch_cuda):
    """stereo = 0, rds = 0, 6 calls of 4096: both PCM rows match the oracle's
    FMDemod mono output as the reference block puts it out -- halved
    (main.cpp's mono branch, which fmx_process_block follows), then clamped --
    at the PCM bars (from call 2 on, MPX from output 128 on); group counts,
    stereo flag, pilot and indicator are 0."""
    sizes = [B] * 6
    raw = _capture()[0][:2 * R.BAND_D * sum(sizes)]
    kt = {}
    g = run_rx(fmx, torch_cuda, raw, sizes, sync="third", ktimes=kt, stereo=0, rds=0)
    ora = _oracle(tuple(sizes), mono=True)
    for c in range(4):
        check_channel("wb_receiver_mono", c, g, ora[c], sizes, 2.0 if c == 3 else 1.0)
    for r in g:
        for key in ("gcount", "stereo", "pilot", "indicator"):
            assert not r[key].any(), key
    assert kt["frontend"][1] == 6 and kt["pilot"][1] == 0 and kt["rs"][1] == 0 and kt["frontend_generic"][1] == 0, kt


def test_arguments(fmx, torch_cuda):
    """Argument errors (FMX_E_INVALID with fmx_wb_process_block in the text,
    FMX_E_CAPACITY for n > block), n = 0, and guard cells around padded PCM,
    MPX and group rows -- at a 16-B aligned base (k_fecf) and at a 4-B aligned
    one (k_rs cannot read such MPX rows: k_frontend)."""
    torch = torch_cuda
    dev = torch.device("cuda")
    L = fmx.lib()
    raw = _capture()[0]
    D, C = R.BAND_D, 4
    d_raw = torch.from_numpy(raw[:2 * D * 3 * B]).to(dev)
    f = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)  # noqa: E731
    z = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)  # noqa: E731
    pl, pr, cnt, sig = f(C, B), f(C, B), z(C), torch.zeros(C * 48, dtype=torch.uint8, device=dev)
    good = lambda: fmx.BlockOut(None, 0, pl.data_ptr(), pr.data_ptr(), B, cnt.data_ptr(), None, None, None, None, 0,  # noqa: E731
                                None, None, None)
    import ctypes as Ct

    def call(wb, n, out, h):
        rc = L.fmx_wb_process_block(wb.w, Ct.c_void_p(d_raw.data_ptr()), n, Ct.byref(out))
        return rc, L.fmx_last_error(h.h)

    h = _handle(fmx, C)
    wb = _wideband(fmx, h, R.BAND_FREQ, block=2048)
    o = good()
    o.d_signal = sig.data_ptr()
    rc, msg = call(wb, B, o, h)
    assert rc == -1 and b"fmx_wb_process_block" in msg and b"d_signal" in msg
    o = good()
    o.d_pcm_r = None
    rc, msg = call(wb, 1024, o, h)
    assert rc == -1 and b"fmx_wb_process_block" in msg
    rc, msg = call(wb, 2049, good(), h)  # the channelizer's block, below the handle's
    assert rc == -4, (rc, msg)
    # n = 0: nothing happens -- the rows of a following fmx_wb_process are those of a run without it
    rows = []
    for with_zero in (False, True):
        w2 = _wideband(fmx, h, R.BAND_FREQ, block=2048)
        bb = f(C, 2 * 1024)
        w2.process_block(d_raw.data_ptr(), 1024, good())
        if with_zero:
            assert call(w2, 0, good(), h)[0] == 0
        w2.process(d_raw.data_ptr() + 4 * D * 1024, 1024, bb.data_ptr(), 1024)
        h.sync()
        rows.append(bb.cpu().numpy())
        w2.close()
    assert np.array_equal(rows[0].view(np.uint32), rows[1].view(np.uint32))
    wb.close()
    w3 = _wideband(fmx, h, R.BAND_FREQ[:3])
    rc, msg = call(w3, 1024, good(), h)
    assert rc == -1 and b"fmx_wb_process_block" in msg and b"channel count" in msg
    w3.close()
    h.close()
    h10 = fmx.Handle(fmx.make_config(), C)  # iq_rate 2.4 MS/s: M = 10
    w10 = _wideband(fmx, h10, R.BAND_FREQ)
    rc, msg = call(w10, 1024, good(), h10)
    assert rc == -1 and b"fmx_wb_process_block" in msg and b"iq_rate" in msg
    w10.close()
    h10.close()
    h256 = fmx.Handle(fmx.make_config(iq_rate=256_000, dsp_rate=256_000), C)
    w256 = _wideband(fmx, h256, R.BAND_FREQ)
    rc, msg = call(w256, 1024, good(), h256)
    assert rc == -1 and b"fmx_wb_process_block" in msg and b"dsp_rate" in msg
    w256.close()
    h256.close()
    # guard cells: rows of B + pad cells inside sentinel-filled allocations
    for off, generic_calls in ((4, 1), (1, 3)):
        h = _handle(fmx, C)
        wb = _wideband(fmx, h, R.BAND_FREQ)
        h.timing_enable(True)
        stride = B + 12
        G = dict(mpx=H.Guarded(torch, "f32", C, stride, off=off), pl=H.Guarded(torch, "f32", C, stride, off=off),
                 pr=H.Guarded(torch, "f32", C, stride, off=off), grp=H.Guarded(torch, "i32", C, GS + 3, off=off, cell=4))
        st, pil, gcnt, clip, ind = z(C), z(C), z(C), f(C), z(C)
        out = fmx.BlockOut(G["mpx"].ptr, stride, G["pl"].ptr, G["pr"].ptr, stride, cnt.data_ptr(), st.data_ptr(),
                           pil.data_ptr(), clip.data_ptr(), G["grp"].ptr, GS + 3, gcnt.data_ptr(), None, ind.data_ptr())
        pos = 0
        for n in (B, 333, B):
            for v in G.values():
                v.fill()
            torch.cuda.synchronize()
            wb.process_block(d_raw.data_ptr() + 4 * D * pos, n, out)
            h.sync()
            pos += n
            k = cnt.cpu().numpy()
            G["mpx"].check(n, ("mpx", off, n))
            G["pl"].check(k, ("pcm_l", off, n))
            G["pr"].check(k, ("pcm_r", off, n))
            G["grp"].check(np.minimum(gcnt.cpu().numpy(), GS + 3), ("groups", off, n))
        kt = h.kernel_times()
        assert kt["frontend_generic"][1] == generic_calls and kt["frontend"][1] == 3 - generic_calls, (off, kt)
        wb.close()
        h.close()
