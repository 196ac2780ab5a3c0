"""The synthetic FM band on the GPU (fmx_synth_band_create / _generate, kernel
k_synth_band).

  1. device against fmx_synth_band_host within 1 LSB: the two run the same
     IEEE operations on the same integers and differ only in sin / cos ulps
     (< about 1e-8 LSB before rounding) and the float Gaussian (< 1e-3 LSB), so
     only a value on a rounding tie can move, and then by one step; every
     amplitude is >= 0.05, so a dropped or mistuned station (6 LSB in u8, 1638
     in int16) cannot hide.  test_synth_band.py's shapes at n = 2 T + 17, rows
     one element past a 16-byte-aligned base and at an aligned base, the two
     byte-identical, all sentinels intact;
     the same at 480 kHz, 10 MHz and 30.72 MHz, up to sample 2^40;
  2. cut invariance, byte for byte, at sample0 0 and 2^33 + 12 345;
  3. two runs byte-identical; a 3-capture object against 1-capture objects;
  4. end to end: wb_ref's band generated call by call straight into
     fmx_wb_process_block, no sync in between: RDS groups of every station in
     the transmitted order, stereo detected, nothing on the empty channel;
  5. the front end: image level of an impaired capture against the closed
     form, and FIXED with the exact inverse restoring the identity capture;
  6. what create and generate refuse, and the object kinds."""
import ctypes as C
import math

import numpy as np
import pytest

import gpu_harness as H
import wb_ref as R
from test_gpu_wb_signal import REC
from test_synth_band import BIG, CAPTURES, CH0, FE, FRONTENDS, _cfgs

pytestmark = pytest.mark.gpu

SENT, GUARD = 0x55, 64  # guard: samples before and after the buffer


@pytest.fixture(scope="module")
def handle(fmx, torch_cuda):
    h = fmx.Handle(fmx.make_config(iq_rate=240_000, dsp_rate=240_000, block=4096, bandwidth_hz=-1, deemphasis=1), 1)
    yield h
    h.close()


class Buf:
    """[S][stride] samples of the format in device memory between two guards
    of GUARD samples, everything SENT; off: elements past a 16-byte-aligned base."""

    def __init__(self, torch, s16, S, stride, off):
        self.esz = 2 if s16 else 1
        self.cells = S * stride
        pad = 16 + self.esz * off
        self.t = torch.full((pad + 2 * self.esz * (self.cells + 2 * GUARD) + 16,), SENT, dtype=torch.uint8, device="cuda")
        base = self.t.data_ptr()
        self.lead = (-base) % 16 + self.esz * off + 2 * self.esz * GUARD
        self.ptr = base + self.lead
        assert (self.ptr - self.esz * off) % 16 == 0
        self.S, self.stride, self.dt = S, stride, (np.int16 if s16 else np.uint8)

    def read(self):
        """-> samples [S][stride][2]; asserts the guards."""
        raw = self.t.cpu().numpy()
        nb = 2 * self.esz * self.cells
        assert (raw[:self.lead] == SENT).all() and (raw[self.lead + nb:] == SENT).all(), "guard cells written"
        return raw[self.lead:self.lead + nb].copy().view(self.dt).reshape(self.S, self.stride, 2)


def _sent(dt):
    return np.frombuffer(bytes([SENT, SENT]), dtype=dt)[0] if dt == np.int16 else SENT


def _gen(fmx, torch, band, s16, S, sample0, n, pad=5, off=0):
    b = Buf(torch, s16, S, n + pad, off)
    band.generate(sample0, n, b.ptr, n + pad)
    band.handle.sync()
    out = b.read()
    assert (out[:, n:] == _sent(b.dt)).all(), "padding written"
    return out[:, :n]


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("fs", [2_400_000, 2_048_000])
@pytest.mark.parametrize("fmt", ["s16", "u8"])
def test_device_against_host(fmx, torch_cuda, handle, fmt, fs, kind):
    s16 = fmt == "s16"
    n = 2 * fmx.synth_band_tile() + 17
    h, torch = handle, torch_cuda
    for sample0 in (0, BIG):
        for noise in (0.0, 0.01):
            cfg, _ = _cfgs(fmx, fmx.FMX_WB_S16 if s16 else fmx.FMX_WB_U8, fs, kind, noise)
            band = fmx.SynthBand(h, cfg, CH0, CAPTURES, FRONTENDS)
            odd = _gen(fmx, torch, band, s16, 3, sample0, n, off=1)
            even = _gen(fmx, torch, band, s16, 3, sample0, n, off=0)
            band.close()
            want = fmx.synth_band_host(cfg, CH0, CAPTURES, sample0, n, frontends=FRONTENDS, bits=band.bits)
            d = np.abs(odd.astype(np.int64) - want.astype(np.int64))
            print(f"{fmt} Fs={fs} kind={kind} sample0={sample0} noise={noise}: {int((d != 0).sum())} of {d.size} "
                  f"samples differ, max {int(d.max())} LSB")
            assert d.max() <= 1, (sample0, noise, int(d.max()), np.argwhere(d > 1)[:4])
            assert (odd == even).all()


@pytest.mark.parametrize("fs", [480_000, 10_000_000, 30_720_000])
def test_device_against_host_at_the_rate_limits(fmx, torch_cuda, handle, fs):
    """The lowest rate (the RDS half-bit index advances by more than one per
    256 samples there), a rational-rate capture's and the highest (the largest
    residues), stations at the band's edges, from sample 2^40 - n: 1 LSB as above."""
    n = fmx.synth_band_tile() + 17
    edge = fs // 2 - 5000
    caps = [[(-edge, 0.2), (fs // 8, 0.1), (edge, 0.2)], [(0, 0.3)]]
    for sample0 in (0, 2 ** 40 - n):
        cfg, _ = _cfgs(fmx, fmx.FMX_WB_S16, fs, 2, 0.01)
        band = fmx.SynthBand(handle, cfg, CH0, caps)
        got = _gen(fmx, torch_cuda, band, True, 2, sample0, n)
        band.close()
        want = fmx.synth_band_host(cfg, CH0, caps, sample0, n, bits=band.bits)
        d = np.abs(got.astype(np.int64) - want.astype(np.int64))
        print(f"Fs={fs} sample0={sample0}: {int((d != 0).sum())} of {d.size} samples differ, max {int(d.max())} LSB")
        assert d.max() <= 1, (sample0, int(d.max()), np.argwhere(d > 1)[:4])
        assert got[0].astype(np.int64).std() > 100


@pytest.mark.parametrize("fmt", ["s16", "u8"])
def test_cut_invariance(fmx, torch_cuda, handle, fmt):
    s16 = fmt == "s16"
    T = fmx.synth_band_tile()
    n = 3 * T + 5
    h, torch = handle, torch_cuda
    cfg, _ = _cfgs(fmx, fmx.FMX_WB_S16 if s16 else fmx.FMX_WB_U8, 2_048_000, 2, 0.01)
    band = fmx.SynthBand(h, cfg, CH0, CAPTURES, FRONTENDS)
    for sample0 in (0, BIG):
        whole = _gen(fmx, torch, band, s16, 3, sample0, n)
        b = Buf(torch, s16, 3, n, 0)
        at = 0
        for k in (1, 255, 257, T - 1, T + 1, n - (1 + 255 + 257 + 2 * T)):
            assert k > 0
            band.generate(sample0 + at, k, b.ptr + 2 * b.esz * at, n)
            at += k
        assert at == n
        h.sync()
        assert (b.read() == whole).all(), sample0
    band.close()


def test_runs_and_capture_split(fmx, torch_cuda, handle):
    h, torch = handle, torch_cuda
    n = fmx.synth_band_tile() + 300
    for noise in (0.0, 0.01):
        cfg, _ = _cfgs(fmx, fmx.FMX_WB_S16, 2_400_000, 2, noise)
        band = fmx.SynthBand(h, cfg, CH0, CAPTURES, FRONTENDS)
        a = _gen(fmx, torch, band, True, 3, BIG, n)
        assert (a == _gen(fmx, torch, band, True, 3, BIG, n)).all()
        band.close()
        g = 0
        for s, st in enumerate(CAPTURES):
            # the noise is seeded by the capture's index, which a 1-capture object cannot be given: with the
            # noise on only capture 0 has an equal; station g's content is channel CH0 + g, hence the ch0 offset
            if noise == 0.0 or s == 0:
                one = fmx.SynthBand(h, cfg, CH0 + g, [st], [FRONTENDS[s]])
                assert (_gen(fmx, torch, one, True, 1, BIG, n)[0] == a[s]).all(), (noise, s)
                one.close()
            g += len(st)


def test_band_into_the_receiver_without_a_sync(fmx, torch_cuda):
    """wb_ref's band (the stations of R.band_capture at 0.9 x BAND_AMP) made
    call by call on the GPU and received by fmx_wb_process_block on the same
    handle: nothing but stream order lies between generator and receiver."""
    B, D, calls, GS = R.BAND_N, R.BAND_D, R.BAND_CALLS, 8
    torch = torch_cuda
    freqs = list(R.BAND_FREQ) + [R.BAND_EMPTY]
    Cn = len(freqs)
    dev = torch.device("cuda")
    h = fmx.Handle(fmx.make_config(iq_rate=R.BAND_DSP, dsp_rate=R.BAND_DSP, block=B, bandwidth_hz=-1, deemphasis=1), Cn)
    wb = fmx.Wideband(h, fmx.make_wb_config(R.BAND_FS, R.BAND_DSP, fmx.FMX_WB_S16, 0, B), freqs)
    cfg = fmx.make_synth_band(wide_rate=R.BAND_FS, format=fmx.FMX_WB_S16, kind=2, n_bits=8192)
    band = fmx.SynthBand(h, cfg, R.BAND_CH0, [[(f, 0.9 * a) for f, a in zip(R.BAND_FREQ, R.BAND_AMP)]])
    f = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)  # noqa: E731
    z = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)  # noqa: E731
    pl, pr, cnt = f(Cn, B), f(Cn, B), z(Cn)
    stereo, gcount, grp = z(calls, Cn), z(calls, Cn), z(calls, Cn, GS, 4)
    wide = torch.zeros(2 * B * D, dtype=torch.int16, device=dev)
    torch.cuda.synchronize()
    for i in range(calls):
        band.generate(i * B * D, B * D, wide.data_ptr(), B * D)
        out = fmx.BlockOut(None, 0, pl.data_ptr(), pr.data_ptr(), B, cnt.data_ptr(), stereo[i].data_ptr(), None, None,
                           grp[i].data_ptr(), GS, gcount[i].data_ptr(), None, None)
        wb.process_block(wide.data_ptr(), B, out)
    h.sync()
    stereo, gcount, grp = stereo.cpu().numpy(), gcount.cpu().numpy(), grp.cpu().numpy()
    band.close()
    wb.close()
    h.close()
    table = band.groups  # [4][78][4]
    total = 0
    for c in range(4):
        got = [g for i in range(calls) for g in H._groups_of(grp[i], gcount[i], GS)[c]]
        sent = [tuple(int(v) for v in w) for w in table[c]]
        # errors: two bits per block, A in the top pair; level 3 marks a block the decoder did not receive
        # (the group in which block sync was found arrives with its first blocks marked so): such a block
        # carries no word, every other block must be the transmitted one
        recv = [[(g[4] >> (6 - 2 * k)) & 3 != 3 for k in range(4)] for g in got]
        cands = [{j for j, w in enumerate(sent) if all(w[k] == g[k] for k in range(4) if r[k])} for g, r in zip(got, recv)]
        clean = sum(1 for g in got if g[4] == 0)
        print(f"station {c}: {len(got)} groups, {clean} without a flagged block, errors {[g[4] for g in got]}, "
              f"table entries {[sorted(x)[:3] for x in cands]}")
        assert all(any(r) for r in recv) and all(cands), (c, got)
        # successive groups are successive in the table, cyclically (a 0A group recurs every 8 entries, so a
        # group may match several entries: one chain through the matches must exist)
        assert any(all((j0 + k) % len(sent) in cands[k] for k in range(len(got))) for j0 in cands[0]), (c, cands)
        assert clean >= 2, (c, got)
        assert stereo[calls - 1, c] == 1, (c, stereo[:, c])
        total += clean
    assert total >= 8
    assert gcount[:, 4].sum() == 0 and stereo[calls - 1, 4] == 0


def test_front_end_image_and_exact_inverse(fmx, torch_cuda):
    torch = torch_cuda
    n, D, fs = 96_000, 10, 2_400_000
    dev = torch.device("cuda")
    h = fmx.Handle(fmx.make_config(iq_rate=240_000, dsp_rate=240_000, block=4096, bandwidth_hz=-1, deemphasis=1), 2)
    cfg = fmx.make_synth_band(wide_rate=fs, format=fmx.FMX_WB_S16, kind=1, max_offset_hz=0, noise_std=0.003)
    rows = torch.zeros(2, 2 * (n // D), dtype=torch.float32, device=dev)
    lev = torch.zeros(2 * 10, dtype=torch.int32, device=dev)
    wide = torch.zeros(2 * n, dtype=torch.int16, device=dev)

    def arm(frontend, fixed):
        band = fmx.SynthBand(h, cfg, CH0, [[(300_000, 0.5)]], frontend)
        wb = fmx.Wideband(h, fmx.make_wb_config(fs, 240_000, fmx.FMX_WB_S16, 0, n // D), [300_000, -300_000])
        if fixed is not None:
            wb.set_iq_correction(fmx.FMX_IQC_FIXED, fixed)
        band.generate(0, n, wide.data_ptr(), n)
        wb.process(wide.data_ptr(), n // D, rows.data_ptr(), n // D)
        wb.signal(lev.data_ptr())
        h.sync()
        rec = lev.cpu().numpy().view(REC)
        wb.close()
        band.close()
        return float(rec["dbfs"][0]), float(rec["dbfs"][1])

    s0, L0 = arm(None, None)
    s1, L1 = arm([FE], None)
    s2, L2 = arm([FE], (FE[0], FE[1], 1.0 / FE[2], -FE[3] / FE[2]))
    h.close()
    g, th = 1.06, math.radians(4.0)
    want = 20.0 * math.log10(abs(1 - g * complex(math.cos(th), math.sin(th))) / abs(1 + g * complex(math.cos(th), -math.sin(th))))
    print(f"station {s0:.2f} / {s1:.2f} / {s2:.2f} dBFS; image identity {L0:.2f}, impaired {L1:.2f} "
          f"({L1 - s1:.2f} dB from the station, closed form {want:.2f}), corrected {L2:.2f}")
    assert abs((L1 - s1) - want) <= 1.0
    assert abs(L2 - L0) <= 1.0
    assert L1 - L0 > 15.0  # the impairment is what raised the image


def test_refusals_and_object_kinds(fmx, torch_cuda, handle):
    L = fmx.lib()
    h, torch = handle, torch_cuda
    err = lambda: L.fmx_last_error(h.h).decode()  # noqa: E731
    cfg = fmx.make_synth_band(kind=1)
    first = (C.c_int * 2)(0, 1)
    st = (fmx.SynthStation * 1)(fmx.SynthStation(1_195_001, 0.1))
    obj = C.c_void_p(1)
    assert L.fmx_synth_band_create(h.h, C.byref(cfg), 0, 1, first, st, None, None, C.byref(obj)) == -1 and not obj.value
    assert err().startswith("fmx_synth_band_create: ") and "wide_rate / 2" in err()
    k2 = fmx.make_synth_band(kind=2, n_bits=208)
    st[0].freq_hz = 0
    assert L.fmx_synth_band_create(h.h, C.byref(k2), 0, 1, first, st, None, None, C.byref(obj)) == -1
    assert err().startswith("fmx_synth_band_create: ") and "bit table" in err()
    assert L.fmx_synth_band_create(h.h, C.byref(cfg), 0, 1, first, st, None, None, None) == -1
    assert err().startswith("fmx_synth_band_create: ")

    band = fmx.SynthBand(h, cfg, 0, [[(0, 0.1)], []])
    buf = Buf(torch, True, 2, 16, 0)
    for args, what in (((-1, 8, buf.ptr, 16), "sample0"), ((0, 17, buf.ptr, 16), "wide_stride"),
                       ((2 ** 40 - 7, 8, buf.ptr, 16), "2^40"), ((0, 8, None, 16), "null"),
                       ((0, 8, buf.ptr + 1, 16), "aligned"), ((0, -1, buf.ptr, 16), "n_samples")):
        assert L.fmx_synth_band_generate(band.b, args[0], args[1], C.c_void_p(args[2]), args[3]) == -1, what
        assert err().startswith("fmx_synth_band_generate: ") and what in err(), (what, err())
    assert L.fmx_synth_band_generate(band.b, 0, 0, None, 0) == 0  # n_samples == 0 does nothing
    h.sync()
    assert (buf.read() == _sent(np.int16)).all()
    # a band is no channelizer, bank or scan object, and those are no band
    lev = torch.zeros(64, dtype=torch.int32, device="cuda")
    assert L.fmx_wb_process(band.b, C.c_void_p(buf.ptr), 1, None, 1) == -1 and "synthetic band" in err()
    assert L.fmx_wb_bank_process(band.b, C.c_void_p(buf.ptr), 16, 1, None, 1) == -1 and "synthetic band" in err()
    assert L.fmx_wb_scan_process(band.b, C.c_void_p(buf.ptr), 64, C.c_void_p(lev.data_ptr())) == -1 and "synthetic band" in err()
    assert L.fmx_wb_bank_scan_process(band.b, C.c_void_p(buf.ptr), 16, 64, C.c_void_p(lev.data_ptr())) == -1
    assert "not an fmx_wb_bank_scan object" in err()
    assert L.fmx_wb_set_iq_correction(band.b, fmx.FMX_IQC_OFF, None, 0.0) == -1 and "synthetic band" in err()
    assert L.fmx_wb_destroy(band.b) == -1 and "synthetic band" in err()
    wb = fmx.Wideband(h, fmx.make_wb_config(2_400_000, 240_000, fmx.FMX_WB_S16, 0, 64), [0])
    assert L.fmx_synth_band_generate(wb.w, 0, 8, C.c_void_p(buf.ptr), 16) == -1
    assert "fmx_synth_band_generate: not an fmx_synth_band object" in err()
    assert L.fmx_synth_band_destroy(wb.w) == -1 and "fmx_synth_band_destroy: not an fmx_synth_band object" in err()
    wb.close()
    # the band still works
    out = _gen(fmx, torch, band, True, 2, 5, 40)
    assert (out == fmx.synth_band_host(cfg, 0, [[(0, 0.1)], []], 5, 40)).sum() >= out.size - 2
    band.close()
