"""The C ABI (include/fmx.h) at the freedoms it gives a caller and the rest of
the GPU suite never uses: buffers with their own strides and base offsets
(no 16-B alignment, stride != row length), stage entry points over a whole
handle of 19 channels with ragged call sizes, resets and setters, and stage
calls mixed with fmx_process_block on one handle.

Every caller-owned output lives inside a larger allocation filled with a
sentinel (gpu_harness.Guarded); after every call every cell outside the
logical output (MPX [c][0..n), PCM [c][0..count[c]), groups [c][0..min(count,
stride))) must still hold it.  References: the oracle pipeline
(test_gpu_parity.check, unchanged bars) and the oracle's single objects, each
fed the input its GPU stage was given.  19 channels: k_rs / k_pll workgroups
of 16 + 3, k_rds of 8 + 8 + 3, one partial k_bits wave.

Which kernels a geometry keeps (fmx.h "buffer geometry")
is asserted from fmx_kernel_times' launch counts."""
import numpy as np
import pytest

import gpu_harness as H
import rds_wave as W
from test_gpu_parity import MPX_MAX_TOL, PCM_RMS_TOL, check, log_errors, make_iq

pytestmark = pytest.mark.gpu

C19, NBLK, B, M = 19, 14, 4096, 10
ROW = 2 * B * M * NBLK
RING_ALWAYS = 1
E_INVALID, E_CAPACITY = -1, -4
_CACHE = {}


def _shared(fmx, oracle, torch):
    """The 19-channel IQ, its oracle rows and the dense handle's run, computed
    once and left unchanged (process_block geometry cases, mixed-call test)."""
    if not _CACHE:
        iq, _ = make_iq(fmx, 2, C19, NBLK, ch0=900)
        outs = W.pmap(lambda c: H.run_oracle_pipeline(oracle, oracle.make_cfg(), iq[c], NBLK), range(C19))
        kt = {}
        dense = H.run_gpu_pipeline(fmx, torch, fmx.make_config(), iq, NBLK, ktimes=kt)
        _CACHE.update(iq=iq, outs=outs, dense=dense, dense_kt={k: v[1] for k, v in kt.items()})
    return _CACHE["iq"], _CACHE["outs"], _CACHE["dense"], _CACHE["dense_kt"]


# mpx / pcm: (base offset, stride) in floats; grp: in 16-byte records; iq:
# (byte offset, bytes added to the row).  Offsets of 4 floats keep a 16-B
# aligned base with guard cells in front of it.
GEOM = {
    "pad16": dict(mpx=(4, B + 4), pcm=(4, B + 4), grp=(1, 9), iq=(0, 16)),
    "odd_stride": dict(mpx=(4, B + 1), pcm=(4, B + 3), grp=(1, 11), iq=(0, 0)),
    "odd_base": dict(mpx=(1, B + 4), pcm=(1, B), grp=(0, 8), iq=(0, 0)),
    "iq_unaligned": dict(mpx=(0, B), pcm=(0, B), grp=(0, 8), iq=(2, 2)),
}
# launches of the whole run per kernel (fmx_kernel_times)
LAUNCHES = {
    "pad16": dict(frontend=NBLK, rs=NBLK, pilot=NBLK, frontend_generic=0),
    "odd_stride": dict(frontend=NBLK, rs=0, pilot=NBLK, frontend_generic=0),
    "odd_base": dict(frontend=NBLK, rs=0, pilot=NBLK, frontend_generic=0),
    "iq_unaligned": dict(frontend=0, rs=0, pilot=0, frontend_generic=NBLK),
}
# Bit-identical to the dense handle where the same arithmetic kernels ran:
# everything for pad16.  Without k_rs the RDS resampler runs inside k_fe8
# (RS = true) as FMA chains, k_rs sums in blocks of 4 on MFMA -- a few ulp
# apart (the comment above k_rs, fmx_kernels.hip) -- so there MPX, clip, pilot,
# flags, counts and PCM are bit-identical and the groups equal.  The generic
# front end (iq_unaligned) is another arithmetic: oracle bars only.
IDENTICAL = {"pad16": True, "odd_stride": True, "odd_base": True, "iq_unaligned": False}


@pytest.mark.parametrize("case", list(GEOM))
def test_process_block_on_caller_geometry(fmx, oracle, torch_cuda, case):
    """fmx_process_block, 19 channels x 14 blocks, outputs (and for two cases
    the IQ) on caller geometry: every channel against the oracle pipeline at
    the parity bars, the kernels the geometry should keep, guard cells intact
    after every block (run_gpu_geometry), outputs bit-identical to a handle on
    dense buffers."""
    iq, outs, dense, dense_kt = _shared(fmx, oracle, torch_cuda)
    assert (dense_kt["frontend"], dense_kt["rs"], dense_kt["pilot"], dense_kt["frontend_generic"]) == \
        (NBLK, NBLK, NBLK, 0), dense_kt
    kt = {}
    g = H.run_gpu_geometry(fmx, torch_cuda, fmx.make_config(), iq, NBLK, GEOM[case], ktimes=kt)
    launches = {k: v[1] for k, v in kt.items()}
    for k, want in LAUNCHES[case].items():
        assert launches[k] == want, (case, k, launches)
    ngroups = 0
    for c in range(C19):
        ngroups += len(check(g, outs[c], c, NBLK, f"abi_{case}")["groups_oracle"])
    assert ngroups >= 2
    if not IDENTICAL[case]:
        return
    for b in range(NBLK):
        s, d = g[b], dense[b]
        for k in ("mpx", "count", "stereo", "pilot", "indicator", "clip"):
            assert np.array_equal(s[k].view(np.uint8), d[k].view(np.uint8)), (case, b, k)
        for c in range(C19):
            n = int(d["count"][c])
            for k in ("pcm_l", "pcm_r"):
                assert np.array_equal(s[k][c, :n].view(np.uint32), d[k][c, :n].view(np.uint32)), (case, b, c, k)
        assert s["groups"] == d["groups"], (case, b)


def test_shared_mpx_unsynchronised(fmx, torch_cuda):
    """The bench's calling pattern, no host synchronisation between blocks,
    with ONE caller MPX buffer given to every call: the front end of step k + 1
    may write it only after step k's readers (k_pilot, k_rs, k_pll) are done.
    Every block's PCM, counts, flags, pilot, clip and groups, and the last
    block's MPX, bit-identical to a run with one MPX buffer per block."""
    torch = torch_cuda
    C, nblk = 64, 12
    cfg = fmx.make_config()
    scfg = fmx.make_synth(kind=2, n_bits=8192)
    bits, _ = fmx.synth_rds_bits(scfg, 0, C)
    dev = torch.device("cuda")
    d_bits = torch.from_numpy(bits).to(dev)
    row = 2 * B * M * nblk
    d_iq = torch.empty((C, row), dtype=torch.uint8, device=dev)
    h = fmx.Handle(cfg, C)
    h.synth_device(scfg, 0, C, 0, B * M * nblk, d_bits.data_ptr(), d_iq.data_ptr(), row)
    h.sync()
    h.close()
    a = H.run_gpu_unsynchronised(fmx, torch, cfg, d_iq, row, C, nblk, shared_mpx=True)
    b = H.run_gpu_unsynchronised(fmx, torch, cfg, d_iq, row, C, nblk, shared_mpx=False)
    for k in a:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
    assert np.all(a["cnt"] >= 546) and np.all(a["cnt"] <= 547)
    assert np.all(a["st"][-1] == 1) and np.any(a["mpx"] != 0.0)
    assert int(a["gcnt"].sum()) >= 2


# --------------------------------------------------------------------------
# B. stage entry points over 19 channels
# --------------------------------------------------------------------------
def _events(h, i):
    for ch in H.STAGE_RESETS.get(i, ()):
        h.reset(ch)
    for (key, value, ch) in H.STAGE_PARAMS.get(i, ()):
        h.set_param(key, value, ch)


def _vec(G, R, k, dtype=np.int32):
    return G[k].view(R[k], dtype)[0].copy()


def test_stage_chain_19_channels_ragged(fmx, oracle, torch_cuda):
    """fmx_decimate -> fmx_demod (with mono) -> fmx_stereo -> fmx_afpost ->
    fmx_rds on one handle of 19 channels, every buffer skewed (base one element
    in, strides that differ from each other and are no multiple of 4, the IQ
    rows at an odd address an odd number of bytes apart), call sizes
    gpu_harness.STAGE_SIZES, fmx_reset of channels 5 and 18 before call 6,
    force_mono / deemph_us / deviation_hz on channels 2 / 16 / 1 before call 8.
    Per channel the oracle's own five objects, each fed the input its GPU stage
    was given, with the same resets and setters.  Bars (test_stage_entry_points'):
    decimator max < 1e-5, MPX max < MPX_MAX_TOL, mono and L/R RMS over the
    channel's whole run < PCM_RMS_TOL, afpost max < 1e-5; counts, stereo flag,
    pilot tenths and groups exact.  The input is one the oracle decides the same
    way under ten times the GPU's MPX error (tests/test_abi_stage_plan.py; no
    channel or call position had to be rejected)."""
    torch = torch_cuda
    C, sizes = H.STAGE_C, H.STAGE_SIZES
    iq = H.stage_iq(fmx)
    cfg = fmx.make_config(bandwidth_hz=-1, deemphasis=1)  # objects as constructed (75 us, ctor IQ filter)
    h = fmx.Handle(cfg, C)
    keep, iq_base, iq_stride = H.skewed_iq(torch, iq, 1, 7)
    assert iq_base % 2 == 1 and iq_stride % 2 == 1
    S = dict(bb=2 * B + 6, mpx=B + 1, mono=B + 3, lr=B + 5, out=B + 7, grp=9)
    assert all(v % 4 for v in S.values()) and len(set(S.values())) == len(S)
    G = dict(bb=H.Guarded(torch, "f32", C, S["bb"]), mpx=H.Guarded(torch, "f32", C, S["mpx"]),
             mono=H.Guarded(torch, "f32", C, S["mono"]), lf=H.Guarded(torch, "f32", C, S["lr"]),
             rf=H.Guarded(torch, "f32", C, S["lr"]), ol=H.Guarded(torch, "f32", C, S["out"]),
             orr=H.Guarded(torch, "f32", C, S["out"]), grp=H.Guarded(torch, "i32", C, S["grp"], cell=4))
    for k in ("cnt", "st", "pil", "acnt", "gcnt"):
        G[k] = H.Guarded(torch, "i32", 1, C)
    calls = []
    pos = 0
    for i, n in enumerate(sizes):
        _events(h, i)
        for g in G.values():
            g.fill()
        torch.cuda.synchronize()
        h.decimate(iq_base + 2 * M * pos, iq_stride, n, G["bb"].ptr, S["bb"])
        h.demod(G["bb"].ptr, S["bb"], n, G["mpx"].ptr, S["mpx"], G["mono"].ptr, S["mono"], G["cnt"].ptr)
        h.stereo(G["mpx"].ptr, S["mpx"], n, G["lf"].ptr, G["rf"].ptr, S["lr"], G["st"].ptr, G["pil"].ptr)
        h.afpost(G["lf"].ptr, G["rf"].ptr, S["lr"], n, G["ol"].ptr, G["orr"].ptr, S["out"], B, G["acnt"].ptr)
        h.rds(G["mpx"].ptr, S["mpx"], n, G["grp"].ptr, S["grp"], G["gcnt"].ptr)
        h.sync()
        R = {k: g.raw() for k, g in G.items()}
        v = {k: _vec(G, R, k) for k in ("cnt", "st", "pil", "acnt", "gcnt")}
        tag = ("call", i, n)
        for k in v:
            G[k].check(C, tag + (k,), R[k])
        assert np.all(v["cnt"] >= 0) and np.all(v["acnt"] >= 0) and np.all(v["gcnt"] >= 0), (tag, v)
        G["bb"].check(2 * n, tag + ("bb",), R["bb"])
        G["mpx"].check(n, tag + ("mpx",), R["mpx"])
        G["mono"].check(v["cnt"], tag + ("mono",), R["mono"])
        G["lf"].check(n, tag + ("left",), R["lf"])
        G["rf"].check(n, tag + ("right",), R["rf"])
        G["ol"].check(v["acnt"], tag + ("out_l",), R["ol"])
        G["orr"].check(v["acnt"], tag + ("out_r",), R["orr"])
        G["grp"].check(np.minimum(v["gcnt"], S["grp"]), tag + ("groups",), R["grp"])
        rec = dict(v, n=n, pos=pos, groups=H.records_to_groups(G["grp"].view(R["grp"]).view(np.uint8), v["gcnt"],
                                                              S["grp"]))
        for k in ("bb", "mpx", "mono", "lf", "rf", "ol", "orr"):
            rec[k] = G[k].view(R[k], np.float32).copy()
        calls.append(rec)
        pos += n
    h.close()
    del keep

    def one(c):
        ch = H.OracleChannel(oracle)
        st = dict(decim_max=0.0, mpx_max=0.0, afpost_max=0.0)
        sq = dict(mpx=[0.0, 0], mono=[0.0, 0], lr=[0.0, 0])
        bad, go, gg = [], [], []

        def acc(key, d):
            sq[key][0] += float(np.sum(d.astype(np.float64) ** 2))
            sq[key][1] += d.size

        for i, r in enumerate(calls):
            n, p = r["n"], r["pos"]
            H.stage_events(ch, i, c)
            obb = ch.decimate(iq[c, 2 * M * p:2 * M * (p + n)], n)
            st["decim_max"] = max(st["decim_max"], float(np.max(np.abs(obb - r["bb"][c, :2 * n]))))
            om, omono = ch.demod(r["bb"][c, :2 * n], n)
            k = int(r["cnt"][c])
            if len(omono) != k:
                bad.append((i, "mono count", len(omono), k))
            k = min(k, len(omono))
            st["mpx_max"] = max(st["mpx_max"], float(np.max(np.abs(om - r["mpx"][c, :n]))))
            acc("mpx", om - r["mpx"][c, :n])
            acc("mono", omono[:k] - r["mono"][c, :k])
            ol_, or_, s_, p_ = ch.stereo(r["mpx"][c, :n], n)
            if (s_, p_) != (int(r["st"][c]), int(r["pil"][c])):
                bad.append((i, "stereo flag / pilot", (s_, p_), (int(r["st"][c]), int(r["pil"][c]))))
            acc("lr", ol_ - r["lf"][c, :n])
            acc("lr", or_ - r["rf"][c, :n])
            al, ar = ch.afpost(r["lf"][c, :n], r["rf"][c, :n], n, B)
            k = int(r["acnt"][c])
            if len(al) != k:
                bad.append((i, "afpost count", len(al), k))
            k = min(k, len(al))
            if k:
                st["afpost_max"] = max(st["afpost_max"], float(np.max(np.abs(al[:k] - r["ol"][c, :k]))),
                                       float(np.max(np.abs(ar[:k] - r["orr"][c, :k]))))
            go.append(ch.rds_groups(r["mpx"][c, :n], n))
            gg.append(r["groups"][c])
        ch.close()
        rms = {k: (v[0] / max(v[1], 1)) ** 0.5 for k, v in sq.items()}
        st.update(mpx_rms=rms["mpx"], mono_rms=rms["mono"], pcm_rms=rms["lr"], mismatches=len(bad),
                  groups_oracle=[x for lst in go for x in lst])
        return st, bad, go, gg

    res = W.pmap(one, range(C))
    ngroups = 0
    for c, (st, bad, go, gg) in enumerate(res):
        log_errors("abi_stage_chain", c, st)
        info = (c, {k: v for k, v in st.items() if not k.startswith("groups")})
        assert not bad, (c, bad[:6])
        assert st["decim_max"] < 1e-5, info
        assert st["mpx_max"] < MPX_MAX_TOL, info
        assert st["mono_rms"] < PCM_RMS_TOL, info
        assert st["pcm_rms"] < PCM_RMS_TOL, info
        assert st["afpost_max"] < 1e-5, info
        assert gg == go, (c, gg, go)
        ngroups += len(st["groups_oracle"])
    assert ngroups >= 2


def _decimate_runs(fmx, oracle, torch, iq_rate, Mx, u8):
    """fmx_decimate (the stage schedule's first 14 call sizes) or
    fmx_decimate_u8 (all of them) of 19 channels, with the schedule's resets,
    skewed buffers; -> per channel the worst differences against the oracle's
    ComplexDecimator."""
    C, sizes = H.STAGE_C, (H.STAGE_SIZES if u8 else H.STAGE_SIZES[:14])
    iq = H.stage_iq(fmx, iq_rate=iq_rate, M=Mx, sizes=sizes)
    cfg = fmx.make_config(iq_rate=iq_rate, dsp_rate=iq_rate // Mx)
    h = fmx.Handle(cfg, C)
    keep, iq_base, iq_stride = H.skewed_iq(torch, iq, 1, 7)
    stride = 2 * B + (3 if u8 else 6)
    out = H.Guarded(torch, "u8" if u8 else "f32", C, stride)
    got, pos = [], 0
    for i, n in enumerate(sizes):
        for ch in H.STAGE_RESETS.get(i, ()):
            h.reset(ch)
        out.fill()
        torch.cuda.synchronize()
        (h.decimate_u8 if u8 else h.decimate)(iq_base + 2 * Mx * pos, iq_stride, n, out.ptr, stride)
        h.sync()
        raw = out.raw()
        out.check(2 * n, ("call", i, n), raw)
        got.append(out.view(raw, None if u8 else np.float32)[:, :2 * n].copy())
        pos += n
    h.close()
    del keep

    def one(c):
        ch = H.OracleChannel(oracle, M=Mx, fs=iq_rate // Mx)
        worst, differ, total, p = 0.0, 0, 0, 0
        for i, n in enumerate(sizes):
            if c in H.STAGE_RESETS.get(i, ()):
                ch.reset()
            x = iq[c, 2 * Mx * p:2 * Mx * (p + n)]
            if u8:
                d = np.abs(ch.decimate_u8(x, n).astype(np.int32) - got[i][c].astype(np.int32))
                differ += int(np.count_nonzero(d))
            else:
                d = np.abs(ch.decimate(x, n) - got[i][c])
            worst = max(worst, float(d.max()))
            total += d.size
            p += n
        ch.close()
        return worst, differ, total

    return W.pmap(one, range(C))


@pytest.mark.parametrize("iq_rate,Mx", [(2_048_000, 8), (1_024_000, 4), (512_000, 2)])
def test_decimate_stage_other_factors(fmx, oracle, torch_cuda, iq_rate, Mx):
    """fmx_decimate alone at M = 8, 4 and 2 (the generic front end's
    instantiations no other stage test reaches), 19 channels, ragged sizes,
    byte-offset IQ rows: max |d| < 1e-5 against ComplexDecimator::executeComplex."""
    for c, (worst, _, _) in enumerate(_decimate_runs(fmx, oracle, torch_cuda, iq_rate, Mx, False)):
        print(f"ABI decimate M={Mx} channel {c}: max |d| {worst:.3g}")
        assert worst < 1e-5, (Mx, c, worst)


def test_decimate_u8_stage(fmx, oracle, torch_cuda):
    """fmx_decimate_u8 (ComplexDecimator::execute) on a handle of its own at
    the chain's sizes: <= 1 LSB, <= 0.2 % of the bytes differing
    (tests/cpp/facade_test.cpp's bars)."""
    for c, (worst, differ, total) in enumerate(_decimate_runs(fmx, oracle, torch_cuda, 2_400_000, 10, True)):
        print(f"ABI decimate_u8 channel {c}: max {worst:.0f} LSB, {differ} of {total} bytes differ")
        assert worst <= 1, (c, worst)
        assert differ * 1000 <= 2 * total, (c, differ, total)


def test_demod_u8_and_downsample_direct_handle(fmx, oracle, torch_cuda):
    """fmx_demod_u8 (FMDemod::processSplit on bytes, with mono and the clipping
    ratio) and fmx_downsample (FMDemod::downsampleAudio, fed the first handle's
    MPX) on 256 kHz direct handles, 19 channels, ragged sizes, skewed buffers.
    Carrier amplitude 1.0: the byte peaks clip, so the ratio is not 0."""
    torch = torch_cuda
    C, fs = H.STAGE_C, 256_000
    sizes = H.STAGE_SIZES[:16]
    iq = H.stage_iq(fmx, iq_rate=fs, M=1, sizes=sizes, amplitude=1.0, noise_std=0.02)
    cfg = fmx.make_config(iq_rate=fs, dsp_rate=fs, bandwidth_hz=-1, deemphasis=1)
    hd, hs = fmx.Handle(cfg, C), fmx.Handle(cfg, C)
    keep, iq_base, iq_stride = H.skewed_iq(torch, iq, 1, 7)
    S = dict(mpx=B + 1, mono=B + 3, down=B + 5)
    G = dict(mpx=H.Guarded(torch, "f32", C, S["mpx"]), mono=H.Guarded(torch, "f32", C, S["mono"]),
             down=H.Guarded(torch, "f32", C, S["down"]), clip=H.Guarded(torch, "f32", 1, C),
             cnt=H.Guarded(torch, "i32", 1, C), dcnt=H.Guarded(torch, "i32", 1, C))
    calls, pos = [], 0
    for i, n in enumerate(sizes):
        for ch in H.STAGE_RESETS.get(i, ()):
            hd.reset(ch)
            hs.reset(ch)
        for g in G.values():
            g.fill()
        torch.cuda.synchronize()
        hd.demod_u8(iq_base + 2 * pos, iq_stride, n, G["mpx"].ptr, S["mpx"], G["mono"].ptr, S["mono"], G["cnt"].ptr,
                    G["clip"].ptr)
        hd.sync()
        hs.downsample(G["mpx"].ptr, S["mpx"], n, G["down"].ptr, S["down"], G["dcnt"].ptr)
        hs.sync()
        R = {k: g.raw() for k, g in G.items()}
        cnt, dcnt = _vec(G, R, "cnt"), _vec(G, R, "dcnt")
        tag = ("call", i, n)
        for k in ("clip", "cnt", "dcnt"):
            G[k].check(C, tag + (k,), R[k])
        assert np.all(cnt >= 0) and np.all(dcnt >= 0), (tag, cnt, dcnt)
        G["mpx"].check(n, tag + ("mpx",), R["mpx"])
        G["mono"].check(cnt, tag + ("mono",), R["mono"])
        G["down"].check(dcnt, tag + ("down",), R["down"])
        calls.append(dict(n=n, pos=pos, cnt=cnt, dcnt=dcnt, clip=_vec(G, R, "clip", np.float32),
                          **{k: G[k].view(R[k], np.float32).copy() for k in ("mpx", "mono", "down")}))
        pos += n
    hd.close()
    hs.close()
    del keep

    def one(c):
        a, b = H.OracleChannel(oracle, M=1, fs=fs), H.OracleChannel(oracle, M=1, fs=fs)
        bad, mpx_max, clip_max = [], 0.0, 0.0
        sq = dict(mpx=[0.0, 0], mono=[0.0, 0], down=[0.0, 0])
        for i, r in enumerate(calls):
            n, p = r["n"], r["pos"]
            if c in H.STAGE_RESETS.get(i, ()):
                a.reset()
                b.reset()
            om, omono, oclip = a.demod_u8(iq[c, 2 * p:2 * (p + n)], n)
            od = b.downsample(r["mpx"][c, :n], n)
            if len(omono) != int(r["cnt"][c]) or len(od) != int(r["dcnt"][c]):
                bad.append((i, "counts", len(omono), int(r["cnt"][c]), len(od), int(r["dcnt"][c])))
                continue
            if np.float32(oclip) != r["clip"][c]:
                bad.append((i, "clip ratio", oclip, float(r["clip"][c])))
            clip_max = max(clip_max, oclip)
            mpx_max = max(mpx_max, float(np.max(np.abs(om - r["mpx"][c, :n]))))
            for key, d in (("mpx", om - r["mpx"][c, :n]), ("mono", omono - r["mono"][c, :len(omono)]),
                           ("down", od - r["down"][c, :len(od)])):
                sq[key][0] += float(np.sum(d.astype(np.float64) ** 2))
                sq[key][1] += d.size
        a.close()
        b.close()
        rms = {k: (v[0] / max(v[1], 1)) ** 0.5 for k, v in sq.items()}
        return dict(mpx_max=mpx_max, mpx_rms=rms["mpx"], pcm_rms=rms["mono"], down_rms=rms["down"],
                    clip_max=clip_max, groups_oracle=[]), bad

    any_clip = 0.0
    for c, (st, bad) in enumerate(W.pmap(one, range(C))):
        log_errors("abi_demod_u8_downsample", c, st)
        assert not bad, (c, bad[:6])
        assert st["mpx_max"] < MPX_MAX_TOL, (c, st)
        assert st["pcm_rms"] < PCM_RMS_TOL, (c, st)
        assert st["down_rms"] < PCM_RMS_TOL, (c, st)
        any_clip = max(any_clip, st["clip_max"])
    assert any_clip > 0.0


def test_stage_error_paths(fmx, torch_cuda):
    """n > block: FMX_E_CAPACITY from every stage call; fmx_afpost with cap
    below the produced count: FMX_E_CAPACITY, nothing written, and the next
    call gives what a handle that never saw the failed call gives (the timing
    set is restored); fmx_decimate on an M = 1 handle: FMX_E_INVALID.  None of
    them launches a kernel (fmx_kernel_times) or writes an output."""
    torch = torch_cuda
    C, n = 3, 1500
    dev = torch.device("cuda")
    cfg = fmx.make_config()
    hs = [fmx.Handle(cfg, C), fmx.Handle(cfg, C)]
    L, h = hs[0].L, hs[0]
    big = H.Guarded(torch, "f32", C, 2 * B + 8)
    iq = torch.zeros((C, 2 * M * (B + 1)), dtype=torch.uint8, device=dev)
    h.timing_enable(True)
    p, s, cnt = big.ptr, 2 * B + 8, H.Guarded(torch, "i32", 1, C)
    import ctypes as Ct
    vp = Ct.c_void_p
    over = B + 1
    rcs = dict(
        decimate=L.fmx_decimate(h.h, vp(iq.data_ptr()), iq.shape[1], over, vp(p), s),
        decimate_u8=L.fmx_decimate_u8(h.h, vp(iq.data_ptr()), iq.shape[1], over, vp(p), s),
        demod=L.fmx_demod(h.h, vp(p), s, over, vp(p), s, None, 0, None),
        stereo=L.fmx_stereo(h.h, vp(p), s, over, vp(p), vp(p), s, None, None),
        afpost=L.fmx_afpost(h.h, vp(p), vp(p), s, over, vp(p), vp(p), s, B, vp(cnt.ptr)),
        rds=L.fmx_rds(h.h, vp(p), s, over, None, 0, vp(cnt.ptr)),
        downsample=L.fmx_downsample(h.h, vp(p), s, over, vp(p), s, vp(cnt.ptr)),
        process_block=L.fmx_process_block(h.h, vp(iq.data_ptr()), iq.shape[1], over, None))
    assert all(rc == E_CAPACITY for rc in rcs.values()), rcs
    # afpost: cap below the count this call produces (1500 inputs -> 200 outputs)
    rng = np.random.default_rng(7)
    x = torch.from_numpy((0.3 * rng.standard_normal((2, C, n))).astype(np.float32)).to(dev)
    outs = [(H.Guarded(torch, "f32", C, B + 3), H.Guarded(torch, "f32", C, B + 3), H.Guarded(torch, "i32", 1, C))
            for _ in hs]
    ol, orr, oc = outs[0]
    rc = L.fmx_afpost(h.h, vp(x[0].data_ptr()), vp(x[1].data_ptr()), n, n, vp(ol.ptr), vp(orr.ptr), B + 3, 100,
                      vp(oc.ptr))
    assert rc == E_CAPACITY, rc
    h.sync()
    launches = {k: v[1] for k, v in h.kernel_times().items()}
    assert not any(launches.values()), launches
    for g in (ol, orr, oc, big, cnt):
        g.check(0, "failed calls")
    for hh, (a, b, k) in zip(hs, outs):
        hh.afpost(x[0].data_ptr(), x[1].data_ptr(), n, n, a.ptr, b.ptr, B + 3, B, k.ptr)
        hh.sync()
    k0, k1 = outs[0][2].view(dtype=np.int32)[0], outs[1][2].view(dtype=np.int32)[0]
    assert np.array_equal(k0, k1) and np.all(np.abs(k0 - 200) <= 1), (k0, k1)  # 1500 * 32 / 240
    for j in (0, 1):
        outs[0][j].check(k0, "afpost after the failed call")
        assert np.array_equal(outs[0][j].view(), outs[1][j].view()), j
    for hh in hs:
        hh.close()
    # M = 1: no decimator
    hd = fmx.Handle(fmx.make_config(iq_rate=256_000, dsp_rate=256_000), C)
    rc = hd.L.fmx_decimate(hd.h, vp(iq.data_ptr()), iq.shape[1], 1024, vp(p), s)
    assert rc == E_INVALID, rc
    hd.sync()
    big.check(0, "decimate on M = 1")
    hd.close()


# --------------------------------------------------------------------------
# C. sequences across entry points
# --------------------------------------------------------------------------
def test_checkpointed_rds_reset_then_generic_process_block(fmx, oracle, torch_cuda):
    """The sequence fmx_rds' comment (fmx_capi.cpp) named as untested: a
    checkpointed fmx_rds call (3001 samples at 256 kHz: 2005 RDS-rate samples,
    the ring left to checkpoints), fmx_reset of two channels (the list path),
    then fmx_process_block with n = 3001 -- the generic front end (n % 4 != 0),
    which writes its RDS-rate samples into the slot the fmx_rds call used (a
    stage call does not advance the step) before the RDS reset part has
    refilled the ring from it.  It comes twice, at the start and mid-stream
    (there with a 333-sample call behind the reset as well), between ragged
    process_block calls as test_ring_refill_ragged_process_block_generic_
    front_end makes them.  fmx_rds is given the MPX a plain handle's
    process_block produced for that stretch of the IQ.
    Against a handle with FMX_DIAG_RDS_RING_ALWAYS (its ring is always valid,
    so its resets never refill): every output of every call bit-identical, the
    rings equal.  Against the oracle's RDSDecoder given the same MPX, call
    sizes and resets: groups equal, every channel.
    Before process_block ran the RDS reset part ahead of such a front end,
    this failed at call 1: the ring read back for reset channel 3 differed
    from the always-written one."""
    torch = torch_cuda
    C, Mx, fs = 20, 8, 256_000
    rates = dict(iq_rate=2_048_000, dsp_rate=fs)
    calls = [("rds", 3001, ()), ("pb", 3001, (3, 7)), ("pb", 333, ()), ("pb", 3001, ()), ("pb", 3001, ()),
             ("rds", 3001, ()), ("pb", 3001, (8, 19)), ("pb", 333, ()), ("rds", 3001, ()), ("pb", 333, (0, 12))]
    calls += [("pb", n, ()) for n in [3001, 333, 333, 3001] * 8]
    sizes = [n for _, n, _ in calls]
    iq, _ = make_iq(fmx, 2, C, 1, iq_rate=rates["iq_rate"], M=Mx, ch0=300, n=sum(sizes))
    cfg = fmx.make_config(**rates)
    dev = torch.device("cuda")
    d_iq = torch.from_numpy(np.ascontiguousarray(iq)).to(dev)
    GS = 8

    def bufs():
        f = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)  # noqa: E731
        z = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)  # noqa: E731
        return dict(mpx=f(C, B), pl=f(C, B), pr=f(C, B), cnt=z(C), st=z(C), pil=z(C), clip=f(C), grp=z(C, GS, 4),
                    gcnt=z(C), ind=z(C))

    def block_out(b):
        return fmx.BlockOut(b["mpx"].data_ptr(), B, b["pl"].data_ptr(), b["pr"].data_ptr(), B, b["cnt"].data_ptr(),
                            b["st"].data_ptr(), b["pil"].data_ptr(), b["clip"].data_ptr(), b["grp"].data_ptr(), GS,
                            b["gcnt"].data_ptr(), None, b["ind"].data_ptr())

    # the MPX of the stretches fmx_rds is given: a plain handle over the whole IQ
    h0, b0 = fmx.Handle(cfg, C), bufs()
    o0, src, pos = block_out(b0), {}, 0
    for i, (kind, n, _) in enumerate(calls):
        h0.process_block(d_iq.data_ptr() + 2 * Mx * pos, iq.shape[1], n, o0)
        h0.sync()
        if kind == "rds":
            src[i] = b0["mpx"].clone()
        pos += n
    h0.close()

    hs = [fmx.Handle(cfg, C), fmx.Handle(cfg, C)]
    hs[1].diag_set(RING_ALWAYS, 1)
    bs = [bufs(), bufs()]
    outs = [block_out(b) for b in bs]
    got, fed = [[] for _ in range(C)], []
    pos = 0
    for i, (kind, n, resets) in enumerate(calls):
        for h, o, b in zip(hs, outs, bs):
            for ch in resets:
                h.reset(ch)
            if kind == "rds":
                h.rds(src[i].data_ptr(), B, n, b["grp"].data_ptr(), GS, b["gcnt"].data_ptr())
            else:
                h.process_block(d_iq.data_ptr() + 2 * Mx * pos, iq.shape[1], n, o)
            h.sync()
        keys = ("gcnt", "grp") if kind == "rds" else ("cnt", "st", "pil", "gcnt", "grp", "ind", "clip")
        for k in keys:
            a, b = bs[0][k].cpu().numpy(), bs[1][k].cpu().numpy()
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (i, kind, n, k)
        if kind == "pb":
            for k, w in (("mpx", n), ("pl", B), ("pr", B)):
                a, b = bs[0][k][:, :w].cpu().numpy(), bs[1][k][:, :w].cpu().numpy()
                assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (i, kind, n, k)
        for c, lst in enumerate(H._groups_of(bs[0]["grp"].cpu().numpy(), bs[0]["gcnt"].cpu().numpy(), GS)):
            got[c].append(lst)
        fed.append((src[i] if kind == "rds" else bs[0]["mpx"])[:, :n].cpu().numpy().copy())
        # rings: behind the process_block calls that follow a reset, behind
        # short calls, at the end (a ring read refills and validates every
        # ring, so not behind the fmx_rds calls: their checkpoints must stand
        # when the reset comes)
        if kind == "pb" and (resets or n == 333 or i == len(calls) - 1):
            ra, rb = [[h.diag_rds_ring(c) for c in (0, 3, 7, 8, 12, 19)] for h in hs]
            for c, a, b in zip((0, 3, 7, 8, 12, 19), ra, rb):
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (i, n, c)
                assert np.any(a != 0.0), (i, c)
        pos += n
    for h in hs:
        h.close()

    def one(c):
        d = W.OracleRds(oracle, fs)
        want = []
        for i, (_, n, resets) in enumerate(calls):
            if c in resets:
                d.reset()
            want.append(d.process(fed[i][c])[0])
        d.close()
        return want

    ngroups = 0
    for c, want in enumerate(W.pmap(one, range(C))):
        assert got[c] == want, (c, got[c], want)
        ngroups += sum(len(x) for x in want)
    assert ngroups >= 3


def test_stage_calls_mixed_with_process_block(fmx, oracle, torch_cuda):
    """fmx.h: the stage entry points keep the "same state as
    fmx_process_block".  One handle of 19 channels runs blocks 0-5 through
    fmx_process_block, blocks 6-7 through the five stage calls (intermediates
    in skewed caller buffers; fmx_demod without mono, as the reference's stereo
    path; the clamp of main.cpp applied to fmx_afpost's output here), blocks
    8-13 through fmx_process_block again -- the pipelined streams, the
    speculated RDS schedule and the timing sets all cross the stage calls.
    Every channel against the oracle pipeline of the 14 blocks at the parity
    bars, groups, flags and counts exact."""
    torch = torch_cuda
    iq, outs, _, _ = _shared(fmx, oracle, torch)
    C = C19
    dev = torch.device("cuda")
    cfg = fmx.make_config()
    h = fmx.Handle(cfg, C)
    d_iq = torch.from_numpy(np.ascontiguousarray(iq)).to(dev)
    GS = 8
    f = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)  # noqa: E731
    z = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)  # noqa: E731
    T = dict(mpx=f(C, B), pl=f(C, B), pr=f(C, B), cnt=z(C), st=z(C), pil=z(C), clip=f(C), grp=z(C, GS, 4), gcnt=z(C),
             ind=z(C))
    out = fmx.BlockOut(T["mpx"].data_ptr(), B, T["pl"].data_ptr(), T["pr"].data_ptr(), B, T["cnt"].data_ptr(),
                       T["st"].data_ptr(), T["pil"].data_ptr(), T["clip"].data_ptr(), T["grp"].data_ptr(), GS,
                       T["gcnt"].data_ptr(), None, T["ind"].data_ptr())
    S = dict(bb=2 * B + 6, mpx=B + 1, lr=B + 5, out=B + 7, grp=9)
    G = dict(bb=H.Guarded(torch, "f32", C, S["bb"]), mpx=H.Guarded(torch, "f32", C, S["mpx"]),
             lf=H.Guarded(torch, "f32", C, S["lr"]), rf=H.Guarded(torch, "f32", C, S["lr"]),
             ol=H.Guarded(torch, "f32", C, S["out"]), orr=H.Guarded(torch, "f32", C, S["out"]),
             grp=H.Guarded(torch, "i32", C, S["grp"], cell=4))
    for k in ("st", "pil", "acnt", "gcnt"):
        G[k] = H.Guarded(torch, "i32", 1, C)
    res = []
    for b in range(NBLK):
        base = d_iq.data_ptr() + b * 2 * B * M
        if b in (6, 7):
            for g in G.values():
                g.fill()
            torch.cuda.synchronize()
            h.decimate(base, iq.shape[1], B, G["bb"].ptr, S["bb"])
            h.demod(G["bb"].ptr, S["bb"], B, G["mpx"].ptr, S["mpx"])
            h.stereo(G["mpx"].ptr, S["mpx"], B, G["lf"].ptr, G["rf"].ptr, S["lr"], G["st"].ptr, G["pil"].ptr)
            h.afpost(G["lf"].ptr, G["rf"].ptr, S["lr"], B, G["ol"].ptr, G["orr"].ptr, S["out"], B, G["acnt"].ptr)
            h.rds(G["mpx"].ptr, S["mpx"], B, G["grp"].ptr, S["grp"], G["gcnt"].ptr)
            h.sync()
            R = {k: g.raw() for k, g in G.items()}
            v = {k: _vec(G, R, k) for k in ("st", "pil", "acnt", "gcnt")}
            tag = ("stage block", b)
            for k in v:
                G[k].check(C, tag + (k,), R[k])
            G["bb"].check(2 * B, tag + ("bb",), R["bb"])
            for k in ("mpx", "lf", "rf"):
                G[k].check(B, tag + (k,), R[k])
            G["ol"].check(v["acnt"], tag + ("out_l",), R["ol"])
            G["orr"].check(v["acnt"], tag + ("out_r",), R["orr"])
            G["grp"].check(np.minimum(v["gcnt"], S["grp"]), tag + ("groups",), R["grp"])
            pcm = {}
            for k in ("ol", "orr"):
                x = G[k].view(R[k], np.float32).copy()
                for c in range(C):  # main.cpp:1302-1308 clamps what AFPostProcessor gave
                    x[c, :v["acnt"][c]] = np.clip(x[c, :v["acnt"][c]], -1.0, 1.0)
                pcm[k] = x
            res.append(dict(mpx=G["mpx"].view(R["mpx"], np.float32)[:, :B].copy(), pcm_l=pcm["ol"], pcm_r=pcm["orr"],
                            count=v["acnt"], stereo=v["st"], pilot=v["pil"], indicator=v["st"], clip=None,
                            groups=H.records_to_groups(G["grp"].view(R["grp"]).view(np.uint8), v["gcnt"], S["grp"])))
        else:
            h.process_block(base, iq.shape[1], B, out)
            h.sync()
            N = {k: t.cpu().numpy().copy() for k, t in T.items()}
            res.append(dict(mpx=N["mpx"], pcm_l=N["pl"], pcm_r=N["pr"], count=N["cnt"], stereo=N["st"],
                            pilot=N["pil"], indicator=N["ind"], clip=N["clip"],
                            groups=H._groups_of(N["grp"], N["gcnt"], GS)))
    h.close()
    ngroups = 0
    for c in range(C):
        ngroups += len(check(res, outs[c], c, NBLK, "abi_mixed_stage_calls")["groups_oracle"])
    assert ngroups >= 2
