"""The wideband channelizer on the GPU (fmx_wb_*, kernel k_wb): one wide IQ
capture in, every tuned channel's complex baseband out, against

  * the oracle's ComplexDecimator at f = 0 (the operation is that decimator
    generalised to a tuned channel: index convention, scale and taps are its);
  * the float64 restatement tests/wb_ref.py (itself pinned to the oracle by
    tests/test_wb_design.py) at tuned channels, u8 and s16, D = 10 and 100;

plus bit-identity across call splits, fresh objects, retunes and caller
geometry, a sample counter above 2^40, and the end-to-end band: four synthetic
stations in one int16 capture through channelizer -> demod -> stereo -> afpost
-> rds on one handle, against the oracle's objects fed the float64
channelizer's rows.  Bar of every channelizer comparison: max |d| < 1e-5, the
project's fmx_decimate bar -- it is the same operation."""
import functools

import numpy as np
import pytest

import gpu_harness as H
import rds_wave as W
import wb_ref as R
from test_gpu_parity import MPX_MAX_TOL, MPX_RMS_TOL, PCM_MAX_TOL, PCM_RMS_TOL, log_errors

pytestmark = pytest.mark.gpu

WB_TOL = 1e-5
DSP = 240_000
SIZES = [4096, 333, 1, 17, 1025, 2720]  # ragged calls; in whole blocks: 2 x 4096
NCH = 19                                # a ragged second group of 16
FMT = {"u8": R.U8, "s16": R.S16}


def _freqs(Fs, n=NCH, seed=5):
    rng = np.random.default_rng(seed)
    base = [0, 1, -1, 123_457, -Fs // 2 + 1, Fs // 2]
    return base + [int(v) for v in rng.integers(-Fs // 2, Fs // 2, n - len(base))]


def _raw(fmt, n_samples, seed):
    """Full-scale noise, interleaved I/Q."""
    rng = np.random.default_rng(seed)
    if fmt == R.U8:
        return rng.integers(0, 256, 2 * n_samples, dtype=np.uint8)
    return rng.integers(-32768, 32768, 2 * n_samples).astype(np.int16)


def run_wb(fmx, torch, wcfg, freqs, raw, sizes, sample0=None, retunes=None, in_off=0, pad=0, dsp=DSP):
    """raw (uint8 / int16 interleaved I/Q) through fmx_wb_process in calls of
    `sizes` outputs -> complex64 [len(freqs)][sum(sizes)].  retunes {call:
    [(channel, freq)]} before that call; in_off: the input's byte offset in
    its allocation; pad: complex cells added to each output row, every cell
    outside the rows' first n checked against gpu_harness's sentinel."""
    C, D = len(freqs), wcfg.wide_rate // wcfg.dsp_rate
    h = fmx.Handle(fmx.make_config(iq_rate=dsp, dsp_rate=dsp, block=max(sizes)), C)
    wb = fmx.Wideband(h, wcfg, freqs)
    if sample0 is not None:
        wb.reset(sample0)
    dev = torch.device("cuda")
    t = torch.full((in_off + raw.nbytes + 64,), H.SENTINEL_BYTE, dtype=torch.uint8, device=dev)
    t[in_off:in_off + raw.nbytes] = torch.from_numpy(raw.view(np.uint8)).to(dev)
    per = 2 * raw.itemsize  # bytes per wide sample
    stride = max(sizes) + pad
    G = H.Guarded(torch, "f32", C, 2 * stride, off=1 if pad else 0, tail=21 if pad else 0)
    rows, pos = [], 0
    for i, n in enumerate(sizes):
        for (c, f) in (retunes or {}).get(i, []):
            wb.set_freq(c, f)
        if pad:
            G.fill()
            torch.cuda.synchronize()
        wb.process(t.data_ptr() + in_off + per * D * pos, n, G.ptr, stride)
        h.sync()
        raw_out = G.raw()
        if pad:
            G.check(2 * n, ("call", i, n), raw_out)
        rows.append(G.view(raw_out, np.float32)[:, :2 * n].copy().view(np.complex64))
        pos += n
    wb.close()
    h.close()
    return np.concatenate(rows, axis=1)


@functools.lru_cache(maxsize=None)
def _stream(fmt, D):
    """The stream of tests 7 / 8 / 10: raw samples, frequencies, float64 rows."""
    Fs = D * DSP
    raw = _raw(FMT[fmt], sum(SIZES) * D, 100 + D)
    freqs = _freqs(Fs)
    return raw, freqs, R.channelize(R.normalise(raw, FMT[fmt]), D, 28, Fs, freqs)


_gpu_rows = {}


def _ragged(fmx, torch, fmt, D):
    """The ragged-call GPU run of _stream(fmt, D), once per session."""
    if (fmt, D) not in _gpu_rows:
        raw, freqs, _ = _stream(fmt, D)
        wcfg = fmx.make_wb_config(D * DSP, DSP, FMT[fmt], 28, 4096)
        _gpu_rows[(fmt, D)] = run_wb(fmx, torch, wcfg, freqs, raw, SIZES)
    return _gpu_rows[(fmt, D)]


def _log(tag, c, d, ref):
    st = dict(wb_max=float(np.max(np.abs(d))), wb_rms=float(np.sqrt(np.mean(np.abs(d) ** 2))),
              wb_rel_rms=float(np.sqrt(np.mean(np.abs(d) ** 2) / max(np.mean(np.abs(ref) ** 2), 1e-300))),
              groups_oracle=[])
    log_errors(tag, c, st)
    return st


@pytest.mark.parametrize("D,tpp,dsp", [(10, 28, 240_000), (25, 12, 256_000)])
def test_f0_channel_is_the_reference_decimator(fmx, oracle, torch_cuda, D, tpp, dsp):
    """u8 input, channel 2 of 5 at f = 0, three calls of 1024 outputs of random
    bytes, against oracle_decim_execute_complex: max |d| < 1e-5 (fmx_decimate's
    bar; achieved 3.9e-7 at D = 10, 2.5e-7 at D = 25)."""
    Fs, n, calls = D * dsp, 1024, 3
    raw = _raw(R.U8, calls * n * D, 7 + D)
    freqs = [-Fs // 3, 250_000, 0, -77_777, Fs // 2]
    wcfg = fmx.make_wb_config(Fs, dsp, fmx.FMX_WB_U8, tpp, n)
    got = run_wb(fmx, torch_cuda, wcfg, freqs, raw, [n] * calls, dsp=dsp)[2]
    L = oracle.lib()
    dec = L.oracle_decim_create(D, tpp, 80.0)
    want = np.zeros(2 * calls * n, np.float32)
    for i in range(calls):
        x = np.ascontiguousarray(raw[2 * D * n * i:2 * D * n * (i + 1)])
        k = L.oracle_decim_execute_complex(dec, x.ctypes.data, n * D, want[2 * n * i:].ctypes.data, n)
        assert k == n
    L.oracle_decim_destroy(dec)
    want = want.view(np.complex64)
    st = _log(f"wb_f0_decimator_D{D}", 2, got - want, want)
    assert st["wb_max"] < WB_TOL, st


@pytest.mark.parametrize("fmt", ["s16", "u8"])
@pytest.mark.parametrize("D", [10, 25, 100])
def test_tuned_channels_against_float64(fmx, torch_cuda, fmt, D):
    """19 channels (0, +-1 Hz, 123 457, -Fs/2 + 1, Fs/2 and 13 random ones),
    tpp 28 (L = 2800 at D = 100), calls of 4096, 333, 1, 17, 1025 and 2720
    outputs of full-scale noise: max |d| < 1e-5 against float64 per channel.
    Achieved (worst channel's max / RMS): s16 D = 10 3.0e-7 / 5.1e-8, D = 25
    3.0e-7 / 4.7e-8, D = 100 2.9e-7 / 4.4e-8; u8 D = 10 2.5e-7 / 4.3e-8, D = 25
    2.7e-7 / 3.9e-8, D = 100 2.8e-7 / 3.7e-8 (profiles/wb_parity_errors.jsonl).  D = 25: an odd D, whose windows start on
    odd samples (the kernel then reads its LDS images one f16 at a time)."""
    _, freqs, ref = _stream(fmt, D)
    got = _ragged(fmx, torch_cuda, fmt, D)
    assert got.shape == ref.shape
    worst = 0.0
    for c in range(NCH):
        st = _log(f"wb_tuned_{fmt}_D{D}_f{freqs[c]}", c, got[c] - ref[c], ref[c])
        worst = max(worst, st["wb_max"])
    assert worst < WB_TOL, worst


@pytest.mark.parametrize("fmt", ["s16", "u8"])
@pytest.mark.parametrize("D", [10, 100])
def test_rows_do_not_depend_on_the_call_split(fmx, torch_cuda, fmt, D):
    """The same stream in whole blocks (2 x 4096) and in the ragged calls, and
    the ragged calls again on a fresh object: bit-identical rows."""
    raw, freqs, _ = _stream(fmt, D)
    ragged = _ragged(fmx, torch_cuda, fmt, D)
    wcfg = fmx.make_wb_config(D * DSP, DSP, FMT[fmt], 28, 4096)
    blocks = run_wb(fmx, torch_cuda, wcfg, freqs, raw, [4096, 4096])
    again = run_wb(fmx, torch_cuda, wcfg, freqs, raw, SIZES)
    assert np.array_equal(ragged.view(np.uint32), blocks.view(np.uint32))
    assert np.array_equal(ragged.view(np.uint32), again.view(np.uint32))


def test_sample_counter_above_2_40_and_retune(fmx, torch_cuda):
    """fmx_wb_reset(2^40 + 12 345) against float64 evaluated at that index
    (32-bit phase arithmetic would be off by whole radians), then
    fmx_wb_set_freq on channels 3 and 17 between calls: from that call on their
    rows are those of a float64 channel that was always at the new frequency
    (the history is raw input), and every other channel is bit-identical to
    the run without the retune."""
    D, Fs, s0 = 10, 10 * DSP, (1 << 40) + 12_345
    sizes = [1024, 1000, 777]
    raw, freqs, _ = _stream("s16", D)
    raw = raw[:2 * D * sum(sizes)]
    wcfg = fmx.make_wb_config(Fs, DSP, fmx.FMX_WB_S16, 28, 1024)
    new = {3: -654_321, 17: Fs // 2}
    plain = run_wb(fmx, torch_cuda, wcfg, freqs, raw, sizes, sample0=s0)
    tuned = run_wb(fmx, torch_cuda, wcfg, freqs, raw, sizes, sample0=s0, retunes={1: list(new.items())})
    x = R.normalise(raw, R.S16)
    ref = R.channelize(x, D, 28, Fs, freqs, sample0=s0)
    worst = max(_log("wb_counter_2_40", c, plain[c] - ref[c], ref[c])["wb_max"] for c in range(NCH))
    assert worst < WB_TOL, worst
    # the same rows with a 32-bit counter would be rotated: the check can tell
    wrong = R.channelize(x, D, 28, Fs, freqs, sample0=s0 & 0xFFFFFFFF)
    assert np.max(np.abs(wrong[3] - ref[3])) > 0.1
    ref_new = R.channelize(x, D, 28, Fs, [new[3], new[17]], sample0=s0)
    for j, c in enumerate((3, 17)):
        assert np.array_equal(tuned[c, :sizes[0]].view(np.uint32), plain[c, :sizes[0]].view(np.uint32))
        d = tuned[c, sizes[0]:] - ref_new[j, sizes[0]:]
        assert _log("wb_retuned", c, d, ref_new[j])["wb_max"] < WB_TOL
    others = [c for c in range(NCH) if c not in new]
    assert np.array_equal(tuned[others].view(np.uint32), plain[others].view(np.uint32))


@pytest.mark.parametrize("fmt,in_off", [("u8", 2), ("s16", 4), ("u8", 1), ("s16", 2)])
def test_caller_geometry(fmx, torch_cuda, fmt, in_off):
    """Input at base + 2 bytes (u8) / + 4 bytes (s16) and at its element
    alignment alone (+ 1 / + 2 bytes: the loads go element by element), output
    rows 4-byte aligned with 5 cells of padding between them: the guard cells
    stay intact and the rows are bit-identical to the dense run (the paths
    differ in how the samples are loaded, not in the arithmetic)."""
    D = 10
    raw, freqs, _ = _stream(fmt, D)
    wcfg = fmx.make_wb_config(D * DSP, DSP, FMT[fmt], 28, 4096)
    got = run_wb(fmx, torch_cuda, wcfg, freqs, raw, SIZES, in_off=in_off, pad=5)
    assert np.array_equal(got.view(np.uint32), _ragged(fmx, torch_cuda, fmt, D).view(np.uint32))


def test_capacity_and_arguments(fmx, torch_cuda):
    torch = torch_cuda
    h = fmx.Handle(fmx.make_config(iq_rate=DSP, dsp_rate=DSP), 2)
    wb = fmx.Wideband(h, fmx.make_wb_config(block=64), [0, 1000])
    buf = torch.zeros(4 * 65 * 10, dtype=torch.int16, device="cuda")
    out = torch.zeros((2, 2 * 65), dtype=torch.float32, device="cuda")
    L = fmx.lib()
    assert L.fmx_wb_process(wb.w, buf.data_ptr(), 65, out.data_ptr(), 65) == -4  # FMX_E_CAPACITY
    assert L.fmx_wb_process(wb.w, buf.data_ptr(), 64, out.data_ptr(), 63) == -1  # out_stride < n_out
    assert L.fmx_wb_set_freq(wb.w, 2, 0) == -1 and L.fmx_wb_set_freq(wb.w, 0, 1_200_001) == -1
    assert b"fmx_wb" in L.fmx_last_error(h.h)
    wb.process(buf.data_ptr(), 0, out.data_ptr(), 65)
    wb.close()
    h.close()


# ---- end to end: the band receiver ----
def run_band(fmx, torch, raw):
    """The int16 capture through channelizer -> demod -> stereo -> afpost ->
    rds on one 4-channel handle, BAND_N outputs per call.  The channelizer has
    a fifth channel tuned to an empty frequency; the stage calls read the first
    four rows.  -> (per call dicts as run_gpu_pipeline's, the channelizer's
    rows complex64 [5][n])."""
    C, n, D = len(R.BAND_FREQ), R.BAND_N, R.BAND_D
    dev = torch.device("cuda")
    h = fmx.Handle(fmx.make_config(bandwidth_hz=-1, deemphasis=1), C)  # objects as constructed
    wb = fmx.Wideband(h, fmx.make_wb_config(R.BAND_FS, R.BAND_DSP, fmx.FMX_WB_S16, 0, n),
                      list(R.BAND_FREQ) + [R.BAND_EMPTY])
    d_raw = torch.from_numpy(raw).to(dev)
    f = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)  # noqa: E731
    z = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)  # noqa: E731
    GS = 8
    bb, mpx, lf, rf, pl, pr = f(C + 1, 2 * n), f(C, n), f(C, n), f(C, n), f(C, n), f(C, n)
    st, pil, cnt, gcnt, grp = z(C), z(C), z(C), z(C), z(C, GS, 4)
    res, rows = [], []
    for i in range(R.BAND_CALLS):
        wb.process(d_raw.data_ptr() + 4 * D * n * i, n, bb.data_ptr(), n)
        h.demod(bb.data_ptr(), 2 * n, n, mpx.data_ptr(), n)
        h.stereo(mpx.data_ptr(), n, n, lf.data_ptr(), rf.data_ptr(), n, st.data_ptr(), pil.data_ptr())
        h.afpost(lf.data_ptr(), rf.data_ptr(), n, n, pl.data_ptr(), pr.data_ptr(), n, n, cnt.data_ptr())
        h.rds(mpx.data_ptr(), n, n, grp.data_ptr(), GS, gcnt.data_ptr())
        h.sync()
        rows.append(bb.cpu().numpy().view(np.complex64).copy())
        res.append(dict(mpx=mpx.cpu().numpy(), pcm_l=pl.cpu().numpy(), pcm_r=pr.cpu().numpy(),
                        count=cnt.cpu().numpy(), stereo=st.cpu().numpy(), pilot=pil.cpu().numpy(),
                        groups=H._groups_of(grp.cpu().numpy(), gcnt.cpu().numpy(), GS)))
    wb.close()
    h.close()
    return res, np.concatenate(rows, axis=1)


def test_band_receiver_end_to_end(fmx, oracle, torch_cuda):
    """Stations 700 .. 703 at -900 / -300 / +200 / +700 kHz, amplitudes 0.30 /
    0.12 / 0.25 / 0.06, in one int16 2.4 MS/s capture; 24 calls of 4096.
    Against the oracle's objects fed the float64 channelizer's rows (rounded
    to f32): RDS groups equal call by call with PI 0x1000 + station (which
    also proves the sign of the frequency axis), stereo flag and pilot exact
    from call 2 on, MPX from output 128 on and PCM from call 2 on at
    test_gpu_parity's bars -- twice those for station 3, whose amplitude is
    half of station 1's while the channelizer's absolute error is the same.
    The head left out is 128 of 98 304 samples per channel: the filter is still
    filling there, |y| ~ 1e-6 and the discriminator's phase arbitrary.  The
    empty channel's RMS is below 1/50 of station 3's.
    The input is one the oracle decides the same way under ten times the
    channelizer's error (tests/test_wb_design.py)."""
    raw = R.band_capture(fmx)
    ref = R.band_reference(raw)
    g, rows = run_band(fmx, torch_cuda, raw)
    n, NC, head = R.BAND_N, R.BAND_CALLS, R.BAND_HEAD
    assert head == 128
    for c in range(5):
        _log("wb_band_rows", c, rows[c] - ref[c], ref[c])
    ora = W.pmap(lambda c: R.oracle_chain(H, oracle, ref[c].astype(np.complex64)), range(4))
    ngroups = 0
    for c in range(4):
        o = ora[c]
        k = 2.0 if c == 3 else 1.0
        dm = np.concatenate([o[i]["mpx"] - g[i]["mpx"][c] for i in range(NC)])[head:].astype(np.float64)
        dp = []
        for i in range(NC):
            assert g[i]["groups"][c] == o[i]["groups"], (c, i, g[i]["groups"][c], o[i]["groups"])
            for grp in o[i]["groups"]:
                if (grp[4] >> 6) == 0:
                    assert grp[0] == 0x1000 + R.BAND_CH0 + c, (c, i, grp)
            ngroups += len(o[i]["groups"])
            assert int(g[i]["count"][c]) == len(o[i]["pcm_l"]), (c, i)
            if i >= 2:
                assert (int(g[i]["stereo"][c]), int(g[i]["pilot"][c])) == (o[i]["stereo"], o[i]["pilot"]), (c, i)
                m = len(o[i]["pcm_l"])
                dp += [o[i]["pcm_l"] - g[i]["pcm_l"][c, :m], o[i]["pcm_r"] - g[i]["pcm_r"][c, :m]]
        dp = np.concatenate(dp).astype(np.float64)
        st = dict(mpx_max=float(np.max(np.abs(dm))), mpx_rms=float(np.sqrt(np.mean(dm * dm))),
                  pcm_max=float(np.max(np.abs(dp))), pcm_rms=float(np.sqrt(np.mean(dp * dp))), groups_oracle=[])
        log_errors("wb_band_end_to_end", c, st)
        assert st["mpx_rms"] < k * MPX_RMS_TOL and st["mpx_max"] < k * MPX_MAX_TOL, (c, st)
        assert st["pcm_rms"] < k * PCM_RMS_TOL and st["pcm_max"] < k * PCM_MAX_TOL, (c, st)
        assert o[-1]["stereo"] == 1, c
    assert ngroups >= 8
    rms = lambda v: float(np.sqrt(np.mean(np.abs(v[head:]) ** 2)))  # noqa: E731
    assert rms(rows[4]) < rms(rows[3]) / 50.0, (rms(rows[4]), rms(rows[3]))
