"""The synthetic FM band without a GPU (fmx_synth_band_*):
  1. header, binding and ABI history name the functions; FMX_ABI_VERSION is 13;
  2. fmx_synth_band_host against the numpy restatement (synth_band_ref.py):
     int16 and u8, Fs 2 400 000 and 2 048 000, three captures of (3, 0, 2)
     stations, all three kinds, sample0 0 and 2^33 + 12 345, n = 3000 at a
     stride of n + 5, noise off and on, one non-identity front end.  Every
     sample within 1 LSB: the two sides differ only in sin / cos ulps, which
     move a pre-rounding value by less than about 1e-8 LSB, and in the float
     Gaussian (< 1e-3 LSB), so only a value on a rounding tie can move, and
     then by one step.  Every amplitude is >= 0.05: a dropped or mistuned
     station moves u8 samples by up to 6 LSB and int16 samples by up to 1638,
     so it cannot hide under the allowance.  Padding keeps its sentinel;
  3. cut invariance on the host, and one thread against eight, byte for byte;
  4. the front end's algebra with the noise off;
  5. every refusal, each naming its function; NULL-object calls need no device;
  6. (test_synth_band_sanitized.py)
  7. the code object's metadata: two k_synth_band instances, no scratch, no
     spills; the sibling tests' kernel counts hold and the new names match none
     of their patterns."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import synth_band_ref as SB
from test_resources import _kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fmx_synth_band_content", "fmx_synth_band_tile", "fmx_synth_band_host", "fmx_synth_band_create",
         "fmx_synth_band_generate", "fmx_synth_band_destroy")
CAPTURES = [[(-700_000, 0.30), (-100_000, 0.20), (300_000, 0.05)], [], [(500_000, 0.25), (800_000, 0.10)]]
FE = (0.02, -0.015, 1.06 * math.cos(math.radians(4.0)), 1.06 * math.sin(math.radians(4.0)))
FRONTENDS = [(0.0, 0.0, 1.0, 0.0), (0.0, 0.0, 1.0, 0.0), FE]
N, PAD, CH0, BIG = 3000, 5, 40, 2 ** 33 + 12_345
SENT = 0x55


def _cfgs(fmx, fmt, fs, kind, noise):
    kw = dict(wide_rate=fs, format=fmt, kind=kind, seed_base=0xBEEF, max_offset_hz=5000, rds_level=0.05,
              n_bits=208, noise_std=noise)
    return fmx.make_synth_band(**kw), kw


def _host(fmx, cfg, sample0, n, captures=CAPTURES, frontends=FRONTENDS, threads=1, pad=PAD):
    out = np.full((len(captures), n + pad, 2), SENT, dtype=np.int16 if cfg.format == fmx.FMX_WB_S16 else np.uint8)
    fmx.synth_band_host(cfg, CH0, captures, sample0, n, frontends=frontends, wide_stride=n + pad, threads=threads,
                        out=out)
    return out


def test_header_binding_and_abi_history(fmx):
    with open(os.path.join(ROOT, "include", "fmx.h")) as fh:
        header = fh.read()
    L = fmx.lib()
    for name in NAMES:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert getattr(L, name).argtypes is not None, name
        assert name in header.split("#define FMX_ABI_VERSION")[0], name  # the ABI history names it
    assert re.search(r"^#define FMX_ABI_VERSION 13$", header, re.M)
    for name in ("SynthBandConfig", "SynthStation", "SynthFrontend", "make_synth_band", "synth_band_host", "SynthBand"):
        assert hasattr(fmx, name), name
    assert fmx.synth_band_tile() > 0 and fmx.synth_band_tile() % 256 == 0
    cfg, _ = _cfgs(fmx, fmx.FMX_WB_S16, 2_048_000, 2, 0.01)
    c = fmx.synth_band_content(cfg)
    assert (c.iq_rate, c.kind, c.amplitude, c.noise_std, c.seed_base, c.max_offset_hz, c.n_bits, c.level_spread_db) == \
        (2_048_000, 2, 1.0, 0.0, 0xBEEF, 5000, 208, 0.0)
    assert c.rds_level == np.float32(0.05)


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("fs", [2_400_000, 2_048_000])
@pytest.mark.parametrize("fmt", ["s16", "u8"])
def test_host_against_the_restatement(fmx, fmt, fs, kind):
    f = fmx.FMX_WB_S16 if fmt == "s16" else fmx.FMX_WB_U8
    for sample0 in (0, BIG):
        for noise in (0.0, 0.01):
            cfg, kw = _cfgs(fmx, f, fs, kind, noise)
            bits = fmx.synth_band_bits(cfg, CH0, 5)[1]
            got = _host(fmx, cfg, sample0, N)
            _, want = SB.band(kw, CH0, CAPTURES, sample0, N, FRONTENDS, bits)
            d = np.abs(got[:, :N].astype(np.int64) - want.astype(np.int64))
            print(f"{fmt} Fs={fs} kind={kind} sample0={sample0} noise={noise}: {int((d != 0).sum())} of {d.size} "
                  f"samples differ, max {int(d.max())} LSB")
            assert d.max() <= 1, (sample0, noise, int(d.max()), np.argwhere(d > 1)[:4])
            assert (got[:, N:] == SENT).all()
            # the stations are there: a capture with stations is no constant row
            assert got[0, :N].astype(np.int64).std() > 1 and got[2, :N].astype(np.int64).std() > 1


@pytest.mark.parametrize("fmt", ["s16", "u8"])
def test_host_cut_and_thread_invariance(fmx, fmt):
    f = fmx.FMX_WB_S16 if fmt == "s16" else fmx.FMX_WB_U8
    for sample0 in (0, BIG):
        cfg, _ = _cfgs(fmx, f, 2_048_000, 2, 0.01)
        whole = _host(fmx, cfg, sample0, N)
        assert (whole == _host(fmx, cfg, sample0, N, threads=8)).all()
        parts, at = [], 0
        for n in (1, 255, 257, N - 513):
            parts.append(_host(fmx, cfg, sample0 + at, n, pad=0))
            at += n
        assert at == N
        assert (np.concatenate(parts, axis=1) == whole[:, :N]).all()


@pytest.mark.parametrize("fmt", ["s16", "u8"])
def test_front_end_algebra(fmx, fmt):
    f = fmx.FMX_WB_S16 if fmt == "s16" else fmx.FMX_WB_U8
    cfg, kw = _cfgs(fmx, f, 2_400_000, 1, 0.0)
    caps = [[(300_000, 0.5), (-450_000, 0.2)]]
    got = _host(fmx, cfg, 77, N, captures=caps, frontends=[FE])
    pre, want = SB.band(kw, CH0, caps, 77, N, [FE], None)
    d = np.abs(got[:, :N].astype(np.int64) - want.astype(np.int64))
    print(f"{fmt}: {int((d != 0).sum())} of {d.size} samples differ")
    assert d.max() <= 1
    # the restatement's front end is the stated algebra on the identity capture's values
    pre0, _ = SB.band(kw, CH0, caps, 77, N, None, None)
    s, o = (32768.0, 0.0) if fmt == "s16" else (127.5, 127.5)
    i0, q0 = (pre0[0, :, 0] - o) / s, (pre0[0, :, 1] - o) / s
    assert np.allclose((pre[0, :, 0] - o) / s, i0 + FE[0], atol=1e-12)
    assert np.allclose((pre[0, :, 1] - o) / s, FE[2] * q0 + FE[3] * i0 + FE[1], atol=1e-12)


def _refused(fmx, what, cfg=None, n_captures=1, first=(0, 1), stations=((100_000, 0.1),), frontends=None, sample0=0,
             n=8, bits=True, out=True, stride=8, null_cfg=False, null_first=False, null_stations=False):
    L = fmx.lib()
    cfg = cfg or fmx.make_synth_band(kind=1)
    t_first = (C.c_int * len(first))(*first)
    t_st = (fmx.SynthStation * max(len(stations), 1))(*[fmx.SynthStation(a, b) for a, b in stations])
    t_fe = (fmx.SynthFrontend * len(frontends))(*[fmx.SynthFrontend(*v) for v in frontends]) if frontends else None
    G = max(first[-1], 1) if len(first) else 1
    b = np.zeros((G if cfg.kind == 2 else 1, max(cfg.n_bits, 1)), np.uint8) if bits else None
    o = np.zeros((max(n_captures, 1), max(stride, 1), 2), np.int16)
    rc = L.fmx_synth_band_host(None if null_cfg else C.byref(cfg), 0, n_captures, None if null_first else t_first,
                               None if null_stations else t_st, t_fe, sample0, n,
                               b.ctypes.data if b is not None else None, o.ctypes.data if out else None, stride, 2)
    msg = L.fmx_synth_band_error().decode()
    assert rc == -1, (what, rc)
    assert msg.startswith("fmx_synth_band_host: ") and len(msg) > 25, (what, msg)
    assert not o.any(), what  # nothing was written
    return msg


def test_refusals_name_their_function(fmx):
    mk = fmx.make_synth_band
    r = lambda what, **kw: _refused(fmx, what, **kw)  # noqa: E731
    assert "null" in r("cfg", null_cfg=True)
    assert "null" in r("first", null_first=True)
    assert "null" in r("stations", null_stations=True)
    assert "null" in r("out", out=False)
    assert "first_station" in r("first entry", first=(1, 2))
    assert "first_station" in r("decreasing", n_captures=2, first=(0, 1, 0))
    assert "n_captures" in r("no capture", n_captures=0)
    assert "n_captures" in r("1025 captures", n_captures=1025, first=tuple([0] * 1026))
    assert "8192" in r("8193 stations", first=(0, 8193), stations=tuple([(0, 0.1)] * 8193))
    assert "wide_rate / 2" in r("past the edge", stations=((1_195_001, 0.1),))
    assert "wide_rate / 2" in r("past the lower edge", stations=((-1_195_001, 0.1),))
    assert "amplitude" in r("negative amplitude", stations=((0, -0.1),))
    assert "amplitude" in r("NaN amplitude", stations=((0, float("nan")),))
    assert "q_gain" in r("q_gain 0", frontends=[(0.0, 0.0, 0.0, 0.0)])
    assert "q_gain" in r("q_gain < 0", frontends=[(0.0, 0.0, -1.0, 0.0)])
    assert "finite" in r("infinite dc_i", frontends=[(float("inf"), 0.0, 1.0, 0.0)])
    assert "format" in r("format", cfg=mk(kind=1, format=2))
    assert "wide_rate" in r("rate below", cfg=mk(kind=1, wide_rate=479_999))
    assert "wide_rate" in r("rate above", cfg=mk(kind=1, wide_rate=30_720_001))
    assert "n_bits" in r("short bit table", cfg=mk(kind=2, n_bits=103))
    assert "bit table" in r("no bit table", cfg=mk(kind=2, n_bits=208), bits=False)
    assert "wide_stride" in r("stride", n=9, stride=8)
    assert "sample0" in r("negative sample0", sample0=-1)
    assert "2^40" in r("past the end", sample0=2 ** 40 - 7)
    # the edge itself is legal
    cfg = mk(kind=1)
    assert fmx.synth_band_host(cfg, 0, [[(1_195_000, 0.1)]], 2 ** 40 - 8, 8).shape == (1, 8, 2)


def test_null_object_calls_need_no_gpu(fmx):
    L = fmx.lib()
    cfg = fmx.make_synth_band(kind=1)
    first = (C.c_int * 2)(0, 1)
    st = (fmx.SynthStation * 1)(fmx.SynthStation(0, 0.1))
    obj = C.c_void_p(1)
    assert L.fmx_synth_band_create(None, C.byref(cfg), 0, 1, first, st, None, None, C.byref(obj)) == -1 and not obj.value
    assert L.fmx_synth_band_generate(None, 0, 16, None, 16) == -1
    assert L.fmx_synth_band_destroy(None) == -1
    assert L.fmx_synth_band_content(None, None) == -1
    assert L.fmx_synth_band_error().decode().startswith("fmx_synth_band_content: ")


def test_code_object(tmp_path):
    ks = _kernels(tmp_path)
    pick = lambda pat: {k: v for k, v in ks.items() if re.search(pat, k)}  # noqa: E731
    band = pick(r"12k_synth_bandILb[01]EEEvNS_6SbArgsE")
    assert len(band) == 2 and len(pick(r"k_synth_band")) == 2, sorted(pick(r"k_synth_band"))
    for name, f in band.items():
        assert f.get("private_segment_fixed_size", 0) == 0, (name, f)
        assert f.get("vgpr_spill_count", 0) == 0 and f.get("sgpr_spill_count", 0) == 0, (name, f)
        assert f.get("agpr_count", 0) == 0 and f.get("vgpr_count", 0) <= 128, (name, f)  # four waves per SIMD
        assert f.get("group_segment_fixed_size", 0) <= 8192, (name, f)
    # the sibling tests' counts, by their own patterns
    counts = {r"\d+k_wbbI": 4, r"\d+k_wbrI": 4, r"7k_rbankILb[01]ELb[01]E": 4, r"10k_bank_iqcILb[01]ELb[01]E": 4,
              r"7k_bscanILb[01]ELb[01]E": 4, r"15k_scan_bank_iqcILb[01]ELb[01]E": 4, r"8k_wb_iqcILb[01]ELb[01]E": 4,
              r"9k_wb_scanILb[01]ELb[01]EEEvNS_10WbScanArgs": 4}
    for pat, n in counts.items():
        assert len(pick(pat)) == n, (pat, sorted(pick(pat)))
    for pat in (r"\d+k_wbb", r"\d+k_wbr", r"k_rbank", r"k_bank_iqc", r"k_bscan", r"k_scan_bank_iqc", r"k_wb_iqc",
                r"k_wb_scan"):
        assert not any(re.search(pat, k) for k in band), pat
