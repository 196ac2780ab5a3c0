"""The capture bank on the GPU (fmx_wb_bank_*, kernels k_wbb, k_wbb_hist,
k_wbb_clip, k_wbb_level): many wide captures of one
format and rate channelized by one launch, each capture behaving as its own
fmx_wb object.

Yardsticks: the single objects themselves (fmx_wb_process, fmx_wb_signal,
fmx_wb_process_block -- bit for bit), tests/wb_ref.py's float64 channelizer at
the channelizer's bar (max |d| < 1e-5, tests/test_gpu_wideband.py), the
oracle's objects fed the float64 rows at test_band_receiver_end_to_end's bars
(twice those for station 3), and tests/test_gpu_wb_signal.py's bars and
float64 records for the RF level.
Shapes: four captures of 17, 0, 5 and 16 channels (a ragged group, an empty
capture, a short group, a full group), u8 D = 10, int16 D = 25 (odd D: the LDS
images are read one f16 at a time) and int16 D = 100; calls of 40, 1, 333, 17
and 512 outputs (several tiles per workgroup, n = 1, calls shorter than the
history of L - 1 = 279 samples / D).
Achieved (profiles/wb_bank_parity_errors.jsonl): rows against float64, worst
channel's max |d| 2.8e-7 (u8 D = 10), 2.9e-7 (int16 D = 25), 2.9e-7 (int16 D =
100); the 8-channel band receiver against the oracle, worst channel: MPX max
6.1e-6 / RMS 3.1e-7, PCM max 1.3e-5 / RMS 1.2e-6; level records against
float64, worst rms / dB / level120: 4.1e-8 / 3.2e-6 / 1.5e-5."""
import ctypes as C
import functools

import numpy as np
import pytest

import gpu_harness as H
import rds_wave as W
import wb_ref as R
import wb_scan_ref as S
from test_gpu_wb_receiver import KEYS as RX_KEYS
from test_gpu_wb_receiver import check_channel, run_rx
from test_gpu_wb_signal import REC, _tones, compare, reference
from test_gpu_wideband import WB_TOL, _log, _raw

pytestmark = pytest.mark.gpu

DSP = 240_000
FMT = {"u8": R.U8, "s16": R.S16}
COUNTS = (17, 0, 5, 16)
PAD = 13  # wide_stride = block * D + 13 samples, the padding at full scale
CASES = {"u8_D10": dict(fmt="u8", D=10, block=512, sizes=(40, 1, 333, 17, 512)),
         "s16_D25": dict(fmt="s16", D=25, block=512, sizes=(40, 1, 333, 17, 512)),
         "s16_D100": dict(fmt="s16", D=100, block=64, sizes=(40, 1, 17, 64))}


def _first(counts):
    return [0] + [int(v) for v in np.cumsum(counts)]


def _bank_freqs(Fs, counts, seed=11):
    """Per capture: 0, +Fs/2, -Fs/2, an odd Hz value, 1, -1, then random ones."""
    rng = np.random.default_rng(seed)
    base = [0, Fs // 2, -Fs // 2, 123_457, 1, -1]
    out = []
    for s, n in enumerate(counts):
        f = base[s % 3:] + [int(v) for v in rng.integers(-Fs // 2, Fs // 2, max(n, 6))]
        out.append(f[:n])
    return out


@functools.lru_cache(maxsize=None)
def _inputs(case):
    """Distinct full-scale noise per capture, the captures' frequencies and float64 rows."""
    k = CASES[case]
    D, Fs, total = k["D"], k["D"] * DSP, sum(k["sizes"])
    raws = [_raw(FMT[k["fmt"]], total * D, 300 + 7 * s + D) for s in range(len(COUNTS))]
    freqs = _bank_freqs(Fs, COUNTS)
    ref = [R.channelize(R.normalise(r, FMT[k["fmt"]]), D, R.tpp_rule(D), Fs, f) if f else None
           for r, f in zip(raws, freqs)]
    return raws, freqs, ref


class Wide:
    """The calls' input on the device: per call [S][wide_stride] samples,
    row s holding capture s's n * D samples of that call and full-scale
    padding (u8 255, int16 32767: hard-clipped values) behind them, at byte
    offset in_off of a sentinel-filled allocation."""

    def __init__(self, torch, fmt, D, block, sizes, raws, in_off=0):
        self.sb = 2 if FMT[fmt] == R.U8 else 4
        self.ws = block * D + PAD
        self.S = len(raws)
        dt, full = (np.uint8, 255) if FMT[fmt] == R.U8 else (np.int16, 32767)
        host = np.full((len(sizes), self.S, 2 * self.ws), full, dtype=dt)
        pos = 0
        for i, n in enumerate(sizes):
            for s, r in enumerate(raws):
                host[i, s, :2 * n * D] = r[2 * D * pos:2 * D * (pos + n)]
            pos += n
        self.t = torch.full((in_off + host.nbytes + 64,), H.SENTINEL_BYTE, dtype=torch.uint8, device="cuda")
        self.t[in_off:in_off + host.nbytes] = torch.from_numpy(host.view(np.uint8).reshape(-1)).to("cuda")
        self.base = self.t.data_ptr() + in_off

    def ptr(self, call, capture=0):
        return self.base + (call * self.S + capture) * self.ws * self.sb


def _handle(fmx, Cn, block):
    return fmx.Handle(fmx.make_config(iq_rate=DSP, dsp_rate=DSP, block=max(block, 1024)), max(Cn, 1))


def _collect(torch, G, lev, sizes, Cn, stride):
    raw = G.raw()
    lens = np.repeat([2 * n for n in sizes], Cn)
    G.check(lens, "bank rows", raw)
    v = G.view(raw, np.float32).reshape(len(sizes), Cn, 2 * stride)
    rows = np.concatenate([v[i, :, :2 * n].copy().view(np.complex64) for i, n in enumerate(sizes)], axis=1)
    recs = lev.cpu().numpy().view(REC) if lev is not None else None
    return rows, recs


def run_bank(fmx, torch, case, raws, freqs, sync="end", in_off=0, events=None, levels=(), fmt=None, tpp=0):
    """The captures through fmx_wb_bank_process, every call with input and
    output buffers of its own inside one sentinel-guarded allocation (rows of
    stride block + 3, the base 4-byte aligned).  events(i, bank) runs before
    call i; fmx_wb_bank_signal behind the calls in `levels`.
    -> rows complex64 [C][sum(sizes)], records [len(levels)][C]."""
    k = CASES[case]
    D, block, sizes = k["D"], k["block"], k["sizes"]
    fmt = fmt or k["fmt"]
    Cn, stride = sum(len(f) for f in freqs), block + 3
    h = _handle(fmx, Cn, block)
    bank = fmx.WidebandBank(h, fmx.make_wb_config(D * DSP, DSP, FMT[fmt], tpp, block), freqs)
    wide = Wide(torch, fmt, D, block, sizes, raws, in_off)
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


def run_singles(fmx, torch, case, raws, freqs, events=None, levels=(), params=None, fmt=None, tpp=0):
    """One fmx_wb object per non-empty capture, each fed its row of the same
    device input; events(i, s, wb) before call i of capture s.
    -> per capture (rows, records), None for an empty capture."""
    k = CASES[case]
    D, block, sizes = k["D"], k["block"], k["sizes"]
    fmt = fmt or k["fmt"]
    stride = block + 3
    h = _handle(fmx, 1, block)
    wide = Wide(torch, fmt, D, block, sizes, raws)
    out = []
    for s, f in enumerate(freqs):
        if not f:
            out.append(None)
            continue
        wb = fmx.Wideband(h, fmx.make_wb_config(D * DSP, DSP, FMT[fmt], tpp, block), f)
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


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("case", list(CASES))
def test_rows_equal_the_single_objects(fmx, torch_cuda, case):
    """Four captures of 17, 0, 5 and 16 channels (frequencies 0, +-Fs / 2,
    123 457 Hz among them), distinct full-scale noise per capture, calls of 40,
    1, 333, 17 and 512 outputs (D = 100: 40, 1, 17, 64), wide_stride = block * D
    + 13 with the padding at full scale, out_stride = block + 3 inside guard
    cells: each capture's rows torch.equal those of an fmx_wb object fed the
    same device row, and are within 1e-5 of float64; the level records behind
    the second and the last call carry each capture's own clip ratios, exactly
    (the padding would add to them); the whole input once more at an offset of
    one element (one byte / one int16: loads element by element) gives
    identical rows and records."""
    torch = torch_cuda
    raws, freqs, ref = _inputs(case)
    k = CASES[case]
    lv = (1, len(k["sizes"]) - 1)
    rows, recs = run_bank(fmx, torch, case, raws, freqs, levels=lv)
    off_rows, off_recs = run_bank(fmx, torch, case, raws, freqs, levels=lv, in_off=1 if k["fmt"] == "u8" else 2)
    single = run_singles(fmx, torch, case, raws, freqs, levels=lv)
    first = _first(COUNTS)
    assert rows.shape == (first[-1], sum(k["sizes"]))
    start = _first(k["sizes"])
    worst = 0.0
    for s in range(len(COUNTS)):
        a, b = first[s], first[s + 1]
        if a == b:
            continue
        assert torch.equal(torch.from_numpy(_bits(rows[a:b]).astype(np.int64)),
                           torch.from_numpy(_bits(single[s][0]).astype(np.int64))), (case, s)
        assert recs[:, a:b].tobytes() == single[s][1].tobytes(), (case, s)
        for c in range(a, b):
            st = _log(f"wb_bank_rows_{case}_cap{s}_f{freqs[s][c - a]}", c, rows[c] - ref[s][c - a], ref[s][c - a])
            worst = max(worst, st["wb_max"])
        for j, i in enumerate(lv):
            want = S.clip_ratios(raws[s][2 * k["D"] * start[i]:2 * k["D"] * start[i + 1]], FMT[k["fmt"]])
            assert np.all(recs[j]["hard_clip_ratio"][a:b] == want[0]), (case, s, i)
            assert np.all(recs[j]["near_clip_ratio"][a:b] == want[1]), (case, s, i)
    assert worst < WB_TOL, worst
    assert np.array_equal(_bits(rows), _bits(off_rows)) and recs.tobytes() == off_recs.tobytes()


RESET_AT, SAMPLE0, RETUNE_TO = 2, 12345, -654_321


def _bank_events(i, bank):
    if i == RESET_AT:
        bank.reset(2, SAMPLE0)
        bank.set_freq(_first(COUNTS)[3] + 4, RETUNE_TO)


def _single_events(i, s, wb):
    if i == RESET_AT and s == 2:
        wb.reset(SAMPLE0)
    if i == RESET_AT and s == 3:
        wb.set_freq(4, RETUNE_TO)


def test_reset_and_retune_per_capture(fmx, torch_cuda):
    """u8, D = 10.  Between the queued calls 1 and 2, with no sync anywhere
    before the end: fmx_wb_bank_reset(bank, 2, 12345) and fmx_wb_bank_set_freq
    of channel 4 of capture 3.  Capture 0 and capture 3's other channels stay
    bit-identical to the undisturbed run; capture 2 and the retuned channel
    equal single objects given the same calls -- and differ from the
    undisturbed run from call 2 on (the reset and the retune took effect),
    not before it."""
    case = "u8_D10"
    raws, freqs, _ = _inputs(case)
    plain, _ = run_bank(fmx, torch_cuda, case, raws, freqs)
    ev, _ = run_bank(fmx, torch_cuda, case, raws, freqs, events=_bank_events)
    single = run_singles(fmx, torch_cuda, case, raws, freqs, events=_single_events)
    first = _first(COUNTS)
    tuned = first[3] + 4
    same = [c for c in range(first[-1]) if not (first[2] <= c < first[3]) and c != tuned]
    assert np.array_equal(_bits(ev[same]), _bits(plain[same]))
    assert np.array_equal(_bits(ev[first[2]:first[3]]), _bits(single[2][0]))
    assert np.array_equal(_bits(ev[first[3]:first[4]]), _bits(single[3][0]))
    cut = _first(CASES[case]["sizes"])[RESET_AT]
    for c in list(range(first[2], first[3])) + [tuned]:
        assert np.array_equal(_bits(ev[c, :cut]), _bits(plain[c, :cut])), c
        assert not np.array_equal(_bits(ev[c, cut:]), _bits(plain[c, cut:])), c


def test_outputs_do_not_depend_on_queuing(fmx, torch_cuda):
    """The calls of the test above (reset and retune included) with level
    calls behind calls 1 and 4: a sync after every call, one sync behind all
    of them, and the latter again on a fresh bank give bit-identical rows and
    records."""
    case = "u8_D10"
    raws, freqs, _ = _inputs(case)
    runs = [run_bank(fmx, torch_cuda, case, raws, freqs, sync=sync, events=_bank_events, levels=(1, 4))
            for sync in ("each", "end", "end")]
    for rows, recs in runs[1:]:
        assert np.array_equal(_bits(rows), _bits(runs[0][0]))
        assert recs.tobytes() == runs[0][1].tobytes()


# ---- the band receiver: fmx_wb_bank_process_block ----
B, GS = R.BAND_N, 8
UNIFORM = [B] * R.BAND_CALLS
KEYS = RX_KEYS


@functools.lru_cache(maxsize=None)
def _captures():
    """Capture A: tests/wb_ref.py's band.  Capture B: A at half amplitude,
    requantised.  -> (raw A, raw B, float64 rows of A, of B), the rows in
    BAND_FREQ's order."""
    import fmx
    a = R.band_capture(fmx)
    b = np.rint(a.astype(np.float64) * 0.5).astype(np.int16)
    return a, b, R.band_reference(a), R.band_reference(b)


BANK_FREQS = [list(R.BAND_FREQ), list(R.BAND_FREQ)[::-1]]  # capture B's stations tuned in reverse order


def run_bank_rx(fmx, torch, raws, freqs, sizes, sync="third", generic=False, levels=False, wide_pad=PAD):
    """test_gpu_wb_receiver.run_rx with a bank: the captures through
    fmx_wb_bank_process_block in calls of `sizes`; the device input is
    [S][whole capture + pad] and a call's d_wide points at its first sample in
    row 0, wide_stride the row length.  -> (per call dicts as run_rx's,
    records [calls][C] when levels)."""
    Cn, D = sum(len(f) for f in freqs), R.BAND_D
    dev = torch.device("cuda")
    h = fmx.Handle(fmx.make_config(iq_rate=DSP, dsp_rate=DSP, block=B, bandwidth_hz=-1, deemphasis=1), Cn)
    bank = fmx.WidebandBank(h, fmx.make_wb_config(R.BAND_FS, DSP, fmx.FMX_WB_S16, 0, B), freqs)
    if generic:
        h.diag_set(fmx.FMX_DIAG_FE_GENERIC, 1)
    every = {"each": 1, "third": 3, "end": len(sizes)}[sync]
    ns = len(sizes) if sync == "end" else 3
    f = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)  # noqa: E731
    z = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)  # noqa: E731
    T = dict(mpx=f(ns, Cn, B), pcm_l=f(ns, Cn, B), pcm_r=f(ns, Cn, B), clip=f(ns, Cn), count=z(ns, Cn), stereo=z(ns, Cn),
             pilot=z(ns, Cn), indicator=z(ns, Cn), gcount=z(ns, Cn), grp=z(ns, Cn, GS, 4))
    lev = torch.zeros((len(sizes), Cn * 40), dtype=torch.uint8, device=dev)
    total = sum(sizes) * D
    ws = total + wide_pad
    host = np.full((len(raws), 2 * ws), 32767, dtype=np.int16)
    for s, r in enumerate(raws):
        host[s, :2 * total] = r[:2 * total]
    d_raw = torch.from_numpy(host).to(dev)
    torch.cuda.synchronize()
    res, pend, pos = [None] * len(sizes), [], 0
    for i, n in enumerate(sizes):
        k = i % ns
        out = fmx.BlockOut(T["mpx"][k].data_ptr(), B, T["pcm_l"][k].data_ptr(), T["pcm_r"][k].data_ptr(), B,
                           T["count"][k].data_ptr(), T["stereo"][k].data_ptr(), T["pilot"][k].data_ptr(),
                           T["clip"][k].data_ptr(), T["grp"][k].data_ptr(), GS, T["gcount"][k].data_ptr(), None,
                           T["indicator"][k].data_ptr())
        bank.process_block(d_raw.data_ptr() + 4 * D * pos, ws, n, out)
        if levels:
            bank.signal(lev[i].data_ptr())
        pend.append((i, k, n))
        pos += n
        if (i + 1) % every == 0 or i + 1 == len(sizes):
            h.sync()
            hostT = {key: v.cpu().numpy() for key, v in T.items()}
            for (j, kk, nn) in pend:
                r = {key: hostT[key][kk].copy() for key in KEYS}
                r["mpx"] = r["mpx"][:, :nn].copy()
                r["groups"] = H._groups_of(r["grp"], r["gcount"], GS)
                for c in range(Cn):  # cells past a row's logical length are never written
                    r["pcm_l"][c, int(r["count"][c]):] = 0.0
                    r["pcm_r"][c, int(r["count"][c]):] = 0.0
                    r["grp"][c, min(int(r["gcount"][c]), GS):] = 0
                res[j] = r
            pend = []
    recs = lev.cpu().numpy().view(REC) if levels else None
    bank.close()
    h.close()
    return res, recs


_runs = {}


def _bank8(fmx, torch):
    """The 8-channel run of captures A and B, 24 calls of 4096, once per session."""
    if "bank8" not in _runs:
        a, b, _, _ = _captures()
        _runs["bank8"] = run_bank_rx(fmx, torch, [a, b], BANK_FREQS, UNIFORM)[0]
    return _runs["bank8"]


def _same_channels(tag, x, y, cx, cy, keys=KEYS):
    """Channels cx of run x against channels cy of run y, every output, bit for bit."""
    bad = []
    for i, (p, q) in enumerate(zip(x, y)):
        for key in keys:
            if not np.array_equal(_bits(p[key][cx]), _bits(q[key][cy])):
                bad.append((i, key))
    assert not bad, (tag, bad[:12], len(bad))


def test_band_receiver_against_the_oracle(fmx, oracle, torch_cuda):
    """Capture A (the band of section 18) and capture B (A at half amplitude,
    requantised, its four stations tuned in reverse order) on one 8-channel
    stereo + RDS handle, 24 calls of 4096, against wb_ref.oracle_chain on the
    float64 rows: groups equal call by call with PI 0x1000 + station, counts
    equal, stereo flag and pilot exact from call 2 on, MPX from output 128 on
    and PCM from call 2 on at test_band_receiver_end_to_end's bars (twice
    those for station 3 of either capture)."""
    g = _bank8(fmx, torch_cuda)
    _, _, ref_a, ref_b = _captures()
    jobs = [(ref_a, c) for c in range(4)] + [(ref_b, 3 - j) for j in range(4)]  # bank channel 4 + j: station 3 - j of B
    ora = W.pmap(lambda j: R.oracle_chain(H, oracle, j[0][j[1]].astype(np.complex64)), jobs)
    ngroups = 0
    for gc, (_, st) in enumerate(jobs):
        ngroups += check_channel("wb_bank_receiver_" + ("A" if gc < 4 else "B"), st, g, ora[gc], UNIFORM,
                                 2.0 if st == 3 else 1.0, gc=gc, exact_from=2 * B, pi=0x1000 + R.BAND_CH0 + st)
        assert ora[gc][-1]["stereo"] == 1, gc
    assert ngroups >= 16


def test_band_receiver_equals_the_single_objects(fmx, torch_cuda):
    """A bank of one capture gives fmx_wb_process_block's outputs on a plain
    fmx_wb object, every one bit for bit; channels 0-3 and 4-7 of the
    8-channel run are bit-identical to two separate 4-channel handles run
    through fmx_wb_process_block on capture A and on capture B (reverse
    tuning): a channel's position in the handle does not matter."""
    torch = torch_cuda
    a, b, _, _ = _captures()
    wb_a = run_rx(fmx, torch, a, UNIFORM, sync="third")
    wb_b = run_rx(fmx, torch, b, UNIFORM, freqs=BANK_FREQS[1], sync="third")
    one = run_bank_rx(fmx, torch, [a], BANK_FREQS[:1], UNIFORM)[0]
    _same_channels("S=1", one, wb_a, slice(0, 4), slice(0, 4))
    g = _bank8(fmx, torch)
    _same_channels("channels 0-3", g, wb_a, slice(0, 4), slice(0, 4))
    _same_channels("channels 4-7", g, wb_b, slice(4, 8), slice(0, 4))


def test_band_receiver_ragged_on_the_generic_front_end(fmx, torch_cuda):
    """Calls of 4096, 1024, 333, 1 and 1028 with FMX_DIAG_FE_GENERIC
    (k_frontend on the rows for every call): the 8 channels equal the two
    4-channel handles' fmx_wb_process_block outputs under the same switch."""
    torch = torch_cuda
    sizes = [4096, 1024, 333, 1, 1028]
    a, b, _, _ = _captures()
    cut = 2 * R.BAND_D * sum(sizes)
    g = run_bank_rx(fmx, torch, [a[:cut], b[:cut]], BANK_FREQS, sizes, sync="each", generic=True)[0]
    wb_a = run_rx(fmx, torch, a[:cut], sizes, sync="each", generic=True)
    wb_b = run_rx(fmx, torch, b[:cut], sizes, freqs=BANK_FREQS[1], sync="each", generic=True)
    _same_channels("generic 0-3", g, wb_a, slice(0, 4), slice(0, 4))
    _same_channels("generic 4-7", g, wb_b, slice(4, 8), slice(0, 4))


# ---- the RF level: fmx_wb_bank_signal ----
LCOUNTS = (6, 5, 0, 17)
PARAMS3 = (12, 0.5, -2.0, -60.0, -15.0)


@functools.lru_cache(maxsize=None)
def _level_inputs():
    """u8, D = 10: tones (|x| <= 0.47, nothing clipped) with noise of its own
    per capture; in capture 1 alone, bytes 0, 1, 8, 9, 247, 254 and 255 planted
    in the last call."""
    k = CASES["u8_D10"]
    D, total = k["D"], sum(k["sizes"])
    raws = [_tones("u8", total * D, seed=40 + s).copy() for s in range(len(LCOUNTS))]
    for r in raws:
        assert S.clip_ratios(r, R.U8) == (0.0, 0.0)
    base = (total - k["sizes"][-1]) * D
    pos = 0
    for bv, cnt in ((0, 3), (1, 5), (8, 7), (9, 11), (247, 13), (254, 2), (255, 9)):
        for _ in range(cnt):
            raws[1][2 * (base + 17 + 23 * pos) + (pos & 1)] = bv
            pos += 1
    assert 17 + 23 * pos < k["sizes"][-1] * D
    from test_gpu_wb_signal import FREQS
    rng = np.random.default_rng(3)
    extra = [int(v) for v in rng.integers(-D * DSP // 2, D * DSP // 2, 11)]
    freqs = [list(FREQS), list(FREQS[:5]), [], list(FREQS) + extra]
    return raws, freqs


def test_levels_equal_the_single_objects(fmx, torch_cuda):
    """Captures of 6, 5, 0 and 17 channels, fmx_wb_bank_signal behind calls 1
    (n = 1) and 4 (n = 512), capture 3 with signal parameters (12, 0.5, -2,
    -60, -15): every record == that of an fmx_wb object given the same calls
    and parameters, every field, and within tests/test_gpu_wb_signal.py's bars
    of float64.  Clipped samples planted in capture 1 only: its ratios equal
    clip_ratios' counts exactly, the other captures' are 0.  Against a run with
    default parameters everywhere, only capture 3's compensated_dbfs and
    level120 (and smoothed level) move.  A second fmx_wb_bank_signal without a
    new call returns FMX_E_INVALID."""
    torch = torch_cuda
    case, lv = "u8_D10", (1, 4)
    k = CASES[case]
    raws, freqs = _level_inputs()
    first = _first(LCOUNTS)

    def ev(i, bank):
        if i == 0:
            bank.set_signal_params(3, *PARAMS3)
        if i == 2:  # behind call 1's level call: nothing new to measure
            rc = fmx.lib().fmx_wb_bank_signal(bank.b, C.c_void_p(scratch.data_ptr()))
            assert rc == -1 and b"fmx_wb_bank_signal" in fmx.lib().fmx_last_error(bank.handle.h)
    scratch = torch.zeros(first[-1] * 40, dtype=torch.uint8, device="cuda")
    _, recs = run_bank(fmx, torch, case, raws, freqs, events=ev, levels=lv)
    _, dflt = run_bank(fmx, torch, case, raws, freqs, levels=lv)
    single = run_singles(fmx, torch, case, raws, freqs, levels=lv, params={3: PARAMS3})
    start = _first(k["sizes"])
    for s in range(len(LCOUNTS)):
        a, b = first[s], first[s + 1]
        if a == b:
            continue
        assert recs[:, a:b].tobytes() == single[s][1].tobytes(), s
        par = PARAMS3 if s == 3 else S.DEFAULT_PARAMS
        want = reference(raws[s], "u8", k["sizes"], freqs=freqs[s], params=par)
        for j, i in enumerate(lv):
            compare(f"wb_bank_signal_cap{s}_call{i}", recs[j][a:b], want[i])
            cr = S.clip_ratios(raws[s][2 * k["D"] * start[i]:2 * k["D"] * start[i + 1]], R.U8)
            assert np.all(recs[j]["hard_clip_ratio"][a:b] == cr[0]) and np.all(recs[j]["near_clip_ratio"][a:b] == cr[1])
            assert (cr != (0.0, 0.0)) == (s == 1 and i == 4), (s, i, cr)
        if s != 3:
            assert recs[:, a:b].tobytes() == dflt[:, a:b].tobytes(), s
    a, b = first[3], first[4]
    for key in ("dbfs", "hard_clip_ratio", "near_clip_ratio"):
        assert np.array_equal(recs[key][:, a:b], dflt[key][:, a:b]), key
    assert np.allclose(recs["compensated_dbfs"][:, a:b] - dflt["compensated_dbfs"][:, a:b], -6.0 + 2.0, atol=1e-9)
    assert not np.array_equal(recs["level120"][:, a:b], dflt["level120"][:, a:b])


def test_level_calls_leave_the_receiver_alone(fmx, torch_cuda):
    """Six calls of the 8-channel band run with fmx_wb_bank_signal behind each:
    MPX, PCM, counts, flags and groups are bit-identical to the run without a
    level call; no record counts the full-scale padding behind the rows, and
    capture B's stations read 20 log10(2) dB below capture A's, in reverse
    order (within 0.01 dB: B's rounding noise is 1e-4 of its weakest
    station)."""
    torch = torch_cuda
    a, b, _, _ = _captures()
    sizes = UNIFORM[:6]
    cut = 2 * R.BAND_D * sum(sizes)
    g, recs = run_bank_rx(fmx, torch, [a[:cut], b[:cut]], BANK_FREQS, sizes, levels=True)
    _same_channels("with levels", g, _bank8(fmx, torch)[:6], slice(0, 8), slice(0, 8))
    assert np.all(recs["hard_clip_ratio"] == 0.0)  # the padding behind each row was not counted
    d = recs["dbfs"]
    assert np.all(np.abs((d[:, :4] - 20.0 * np.log10(2.0)) - d[:, 7:3:-1]) < 0.01), d[-1]  # B: half of A, reversed


def test_arguments(fmx, torch_cuda):
    """wide_stride < n * D, a channel total that is not the handle's and a
    non-NULL d_signal return FMX_E_INVALID, n > block FMX_E_CAPACITY; each
    message names its function.  n = 0 is accepted and does nothing."""
    torch = torch_cuda
    L = fmx.lib()
    D, Cn, blk = 10, 5, 2048
    h = fmx.Handle(fmx.make_config(iq_rate=DSP, dsp_rate=DSP, block=4096), Cn)
    wcfg = fmx.make_wb_config(D * DSP, DSP, fmx.FMX_WB_S16, 0, blk)
    bank = fmx.WidebandBank(h, wcfg, [[0, 1000], [], [5, -7, 9]])
    ws = blk * D
    d = torch.zeros(3 * 2 * ws + 64, dtype=torch.int16, device="cuda")
    rows = torch.zeros(Cn * 2 * blk, dtype=torch.float32, device="cuda")
    f = lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda")  # noqa: E731
    pl, pr, cnt = f(Cn, 4096), f(Cn, 4096), torch.zeros(Cn, dtype=torch.int32, device="cuda")
    sig = torch.zeros(Cn * 48, dtype=torch.uint8, device="cuda")
    good = lambda: fmx.BlockOut(None, 0, pl.data_ptr(), pr.data_ptr(), 4096, cnt.data_ptr(), None, None, None, None, 0,  # noqa: E731
                                None, None, None)
    err = lambda: L.fmx_last_error(h.h)  # noqa: E731
    p = C.c_void_p(d.data_ptr())
    assert L.fmx_wb_bank_process(bank.b, p, ws - 1, blk, C.c_void_p(rows.data_ptr()), blk) == -1
    assert b"fmx_wb_bank_process:" in err() and b"wide_stride" in err()
    assert L.fmx_wb_bank_process(bank.b, p, ws + 10, blk + 1, C.c_void_p(rows.data_ptr()), blk + 1) == -4
    assert b"fmx_wb_bank_process:" in err()
    assert L.fmx_wb_bank_process(bank.b, p, ws, 64, C.c_void_p(rows.data_ptr()), 63) == -1
    assert L.fmx_wb_bank_process_block(bank.b, p, 1024 * D - 1, 1024, C.byref(good())) == -1
    assert b"fmx_wb_bank_process_block" in err() and b"wide_stride" in err()
    o = good()
    o.d_signal = sig.data_ptr()
    assert L.fmx_wb_bank_process_block(bank.b, p, ws, 1024, C.byref(o)) == -1
    assert b"fmx_wb_bank_process_block" in err() and b"fmx_wb_bank_signal" in err()
    assert L.fmx_wb_bank_process_block(bank.b, p, ws + 10, blk + 1, C.byref(good())) == -4
    assert b"fmx_wb_bank_process_block" in err()
    assert L.fmx_wb_bank_set_freq(bank.b, Cn, 0) == -1 and b"fmx_wb_bank_set_freq" in err()
    assert L.fmx_wb_bank_reset(bank.b, 3, 0) == -1 and b"fmx_wb_bank_reset" in err()
    assert L.fmx_wb_bank_reset(bank.b, 0, -1) == -1
    assert L.fmx_wb_bank_set_signal_params(bank.b, 3, 0, 0.5, -4.0, -55.0, -19.0) == -1
    assert b"fmx_wb_bank_set_signal_params" in err()
    assert L.fmx_wb_bank_signal_reset(bank.b, Cn) == -1 and b"fmx_wb_bank_signal_reset" in err()
    assert L.fmx_wb_bank_signal(bank.b, C.c_void_p(sig.data_ptr())) == -1 and b"fmx_wb_bank_signal" in err()  # no call yet
    assert L.fmx_wb_bank_process(bank.b, p, 0, 0, None, 0) == 0
    assert L.fmx_wb_bank_process_block(bank.b, p, ws, 0, C.byref(good())) == 0
    bank.process_block(d.data_ptr(), ws, 1024, good())  # and a good call runs
    h.sync()
    assert int(cnt.cpu().numpy().min()) > 0
    bank.close()
    other = fmx.WidebandBank(h, wcfg, [[0, 1000], [5, -7]])  # 4 channels on a 5-channel handle
    assert L.fmx_wb_bank_process_block(other.b, p, ws, 1024, C.byref(good())) == -1
    assert b"fmx_wb_bank_process_block" in err() and b"channel" in err()
    other.close()
    # creation: a table that does not start at 0, one that decreases, a frequency outside the capture
    bad = C.c_void_p()
    for table, n in (((1, 2), 1), ((0, 3, 2), 2)):
        t = (C.c_int * len(table))(*table)
        fr = (C.c_int * 4)(0, 0, 0, 0)
        assert L.fmx_wb_bank_create(h.h, C.byref(wcfg), n, t, fr, C.byref(bad)) == -1 and not bad.value
        assert b"fmx_wb_bank_create" in err()
    t, fr = (C.c_int * 2)(0, 1), (C.c_int * 1)(1_200_001)
    assert L.fmx_wb_bank_create(h.h, C.byref(wcfg), 1, t, fr, C.byref(bad)) == -1 and b"fmx_wb_bank_create" in err()
    h.close()
