"""Shared driver for the GPU parity tests and smoke(): runs the same
synthetic IQ through libfmx (GPU) and through the oracle (CPU) block by
block and returns both outputs."""
import numpy as np


def run_gpu_pipeline(fmx, torch, cfg, iq, nblk, n=None, resets=None, params=None, retunes=None, ktimes=None):
    """iq: uint8 [C][nblk * 2*B*M]. Returns per-block lists of numpy outputs.
    resets {block: channel}, retunes {block: (channel, mute_samples)},
    params {block: [(key, value, channel)]} are applied before that block.
    ktimes (a dict): filled with fmx_kernel_times ({kernel: (ms, launches)})
    of the whole run.  Each block's "group_block_index" holds the
    block_index field of every record in "groups"."""
    C = iq.shape[0]
    B = cfg.block
    M = cfg.iq_rate // cfg.dsp_rate
    n = n or B
    h = fmx.Handle(cfg, C)
    dev = torch.device("cuda")
    d_iq = torch.from_numpy(np.ascontiguousarray(iq)).to(dev)
    mpx = torch.zeros((C, B), dtype=torch.float32, device=dev)
    pl = torch.zeros((C, B), dtype=torch.float32, device=dev)
    pr = torch.zeros((C, B), dtype=torch.float32, device=dev)
    cnt = torch.zeros(C, dtype=torch.int32, device=dev)
    st = torch.zeros(C, dtype=torch.int32, device=dev)
    pil = torch.zeros(C, dtype=torch.int32, device=dev)
    clip = torch.zeros(C, dtype=torch.float32, device=dev)
    ind = torch.zeros(C, dtype=torch.int32, device=dev)
    GS = 8
    grp = torch.zeros((C, GS, 4), dtype=torch.int32, device=dev)  # 16-byte fmx_rds_group
    gcnt = torch.zeros(C, dtype=torch.int32, device=dev)
    out = fmx.BlockOut(mpx.data_ptr(), B, pl.data_ptr(), pr.data_ptr(), B, cnt.data_ptr(),
                       st.data_ptr(), pil.data_ptr(), clip.data_ptr(), grp.data_ptr(), GS,
                       gcnt.data_ptr(), None, ind.data_ptr())
    res = []
    row = iq.shape[1]
    if ktimes is not None:
        h.timing_enable(True)
    for b in range(nblk):
        if resets and b in resets:
            h.reset(resets[b])
        if retunes and b in retunes:
            h.retune(*retunes[b])
        if params and b in params:
            for (k, v, ch) in params[b]:
                h.set_param(k, v, ch)
        base = d_iq.data_ptr() + b * 2 * n * M
        h.process_block(base, row, n, out)
        h.sync()
        g = grp.cpu().numpy().view(np.uint8).reshape(C, GS, 16)
        gc = gcnt.cpu().numpy()
        groups, gblocks = [], []
        for c in range(C):
            lst, bl = [], []
            for k in range(min(int(gc[c]), GS)):
                w = g[c, k]
                a, bb, cc, d = np.frombuffer(w[:8].tobytes(), dtype=np.uint16)
                lst.append((int(a), int(bb), int(cc), int(d), int(w[8])))
                bl.append(int(np.frombuffer(w[12:16].tobytes(), dtype=np.uint32)[0]))
            groups.append(lst)
            gblocks.append(bl)
        res.append(dict(mpx=mpx[:, :n].cpu().numpy().copy(), pcm_l=pl.cpu().numpy().copy(),
                        pcm_r=pr.cpu().numpy().copy(), count=cnt.cpu().numpy().copy(),
                        stereo=st.cpu().numpy().copy(), pilot=pil.cpu().numpy().copy(),
                        clip=clip.cpu().numpy().copy(), indicator=ind.cpu().numpy().copy(),
                        groups=groups, group_block_index=gblocks))
    if ktimes is not None:
        ktimes.update(h.kernel_times())
    h.close()
    return res


def run_oracle_pipeline(oracle, ocfg, iq_row, nblk, n=None, resets=None, params=None, retunes=None):
    B = ocfg.block
    M = ocfg.iq_rate // ocfg.dsp_rate
    n = n or B
    p = oracle.Pipeline(ocfg)
    res = []
    for b in range(nblk):
        if resets and b in resets:
            p.reset()
        if retunes and b in retunes:
            p.retune(retunes[b])
        if params and b in params:
            for (k, v) in params[b]:
                p.set_param(k, v)
        res.append(p.block(iq_row[b * 2 * n * M:(b + 1) * 2 * n * M]))
    return res


def compare(gres, ores, c, nblk, pcm_blocks=None):
    """Per-channel comparison stats.  pcm_blocks (optional) restricts the PCM
    and pilot-level statistics to those blocks."""
    mpx_err = 0.0
    mpx_sq = 0.0
    mpx_n = 0
    pcm_sq = 0.0
    pcm_n = 0
    pcm_max = 0.0
    st_mismatch = 0
    pil_mismatch = 0
    pil_maxdiff = 0
    cnt_mismatch = 0
    ind_mismatch = 0
    g_gpu, g_ora = [], []
    mpx_where = None
    for b in range(nblk):
        o, g = ores[b], gres[b]
        if g["mpx"] is not None:  # None: a run without the MPX output (bench mode)
            dm = o["mpx"] - g["mpx"][c, :len(o["mpx"])]
            if dm.size and float(np.max(np.abs(dm))) > mpx_err:
                mpx_where = (b, int(np.argmax(np.abs(dm))))
            mpx_err = max(mpx_err, float(np.max(np.abs(dm))))
            mpx_sq += float(np.sum(dm.astype(np.float64) ** 2))
            mpx_n += dm.size
        k = len(o["pcm_l"])
        if int(g["count"][c]) != k:
            cnt_mismatch += 1
        st_mismatch += int(o["stereo"] != int(g["stereo"][c]))
        ind_mismatch += int(o["indicator"] != int(g["indicator"][c]))
        g_gpu += g["groups"][c]
        g_ora += o["groups"]
        if pcm_blocks is not None and b not in pcm_blocks:
            continue
        k = min(k, int(g["count"][c]))
        dl = o["pcm_l"][:k] - g["pcm_l"][c, :k]
        dr = o["pcm_r"][:k] - g["pcm_r"][c, :k]
        pcm_sq += float(np.sum(dl * dl) + np.sum(dr * dr))
        pcm_n += 2 * k
        pcm_max = max(pcm_max, float(np.max(np.abs(dl))) if k else 0.0, float(np.max(np.abs(dr))) if k else 0.0)
        pil_mismatch += int(o["pilot"] != int(g["pilot"][c]))
        pil_maxdiff = max(pil_maxdiff, abs(int(o["pilot"]) - int(g["pilot"][c])))
    return dict(mpx_max=mpx_err, mpx_where=mpx_where, mpx_rms=(mpx_sq / max(mpx_n, 1)) ** 0.5,
                pcm_rms=(pcm_sq / max(pcm_n, 1)) ** 0.5, pcm_max=pcm_max,
                stereo_mismatch=st_mismatch, indicator_mismatch=ind_mismatch, pilot_mismatch=pil_mismatch, pilot_maxdiff=pil_maxdiff, count_mismatch=cnt_mismatch,
                groups_gpu=g_gpu, groups_oracle=g_ora)


def _groups_of(grp_rows, gcnt_rows, GS):
    """grp_rows: int32 [K][GS][4] (16-byte fmx_rds_group records), gcnt_rows [K]."""
    g = grp_rows.view(np.uint8).reshape(len(gcnt_rows), GS, 16)
    out = []
    for j in range(len(gcnt_rows)):
        lst = []
        for k in range(min(int(gcnt_rows[j]), GS)):
            w = g[j, k]
            a, bb, cc, d = np.frombuffer(w[:8].tobytes(), dtype=np.uint16)
            lst.append((int(a), int(bb), int(cc), int(d), int(w[8])))
        out.append(lst)
    return out


def run_gpu_pipelined(fmx, torch, cfg, C, scfg, nblk, keep, ch0=0, with_mpx=False, warmup=5, all_groups=None,
                      retunes=None):
    """The bench's timed mode (bench.py step()): every block through
    fmx_process_block back to back, NO host synchronisation between blocks,
    kernel timing switched on after `warmup` blocks as the bench does, the
    RF-level output on, and the front end of step k overlapping steps k-1 /
    k-2 on the four streams.  Outputs go to per-block device buffers (the
    bench rotates three sets it never reads), so nothing is read back until
    the last block has been submitted.  Channels [ch0, ch0 + C) of the
    synthetic plan (a rank's fmx_dist shard).  Returns (per-block results
    indexed by position in keep, host IQ rows of keep, transmitted groups of
    keep, per-block stereo fraction over all C channels).  all_groups: a list
    that receives every channel's decoded groups over all blocks (full-size
    property checks).  retunes {block: [(channel, mute_samples), ...]}:
    fmx_retune calls queued before that block's fmx_process_block (no
    synchronisation, as a live receiver retunes)."""
    B = cfg.block
    M = cfg.iq_rate // cfg.dsp_rate
    n_iq = B * M
    h = fmx.Handle(cfg, C)
    dev = torch.device("cuda")
    bits, tx = fmx.synth_rds_bits(scfg, ch0, C)
    d_bits = torch.from_numpy(bits).to(dev)
    row = 2 * n_iq * nblk
    d_iq = torch.empty((C, row), dtype=torch.uint8, device=dev)
    h.synth_device(scfg, ch0, C, 0, n_iq * nblk, d_bits.data_ptr(), d_iq.data_ptr(), row)
    h.sync()  # the synth (stream sA) has read d_bits before torch may reuse its memory
    del d_bits
    GS = 8
    pl = torch.full((nblk, C, B), float("nan"), dtype=torch.float32, device=dev)
    pr = torch.full((nblk, C, B), float("nan"), dtype=torch.float32, device=dev)
    mpx = torch.full((nblk, C, B), float("nan"), dtype=torch.float32, device=dev) if with_mpx else None
    ints = torch.full((6, nblk, C), -1, dtype=torch.int32, device=dev)  # count, stereo, pilot, gcount, indicator
    clip = torch.zeros((nblk, C), dtype=torch.float32, device=dev)
    grp = torch.zeros((nblk, C, GS, 4), dtype=torch.int32, device=dev)
    sig = torch.zeros((nblk, C, 10), dtype=torch.float32, device=dev)
    h.sync()
    torch.cuda.synchronize()
    for b in range(nblk):
        if b == warmup:
            h.timing_enable(True)
        for (ch, mute) in (retunes or {}).get(b, []):
            h.retune(ch, mute)
        out = fmx.BlockOut(mpx[b].data_ptr() if with_mpx else None, B if with_mpx else 0,
                           pl[b].data_ptr(), pr[b].data_ptr(), B, ints[0, b].data_ptr(), ints[1, b].data_ptr(),
                           ints[2, b].data_ptr(), clip[b].data_ptr(), grp[b].data_ptr(), GS, ints[3, b].data_ptr(),
                           sig[b].data_ptr(), ints[4, b].data_ptr())
        h.process_block(d_iq.data_ptr() + b * 2 * n_iq, row, B, out)
    h.sync()
    torch.cuda.synchronize()
    kt = h.kernel_times()
    kidx = torch.tensor(keep, dtype=torch.long, device=dev)
    sel = lambda t: t.index_select(1, kidx).cpu().numpy()  # noqa: E731  [nblk][len(keep)]...
    PL, PR = sel(pl), sel(pr)
    MPX = sel(mpx) if with_mpx else None
    I = ints.index_select(2, kidx).cpu().numpy()  # [6][nblk][len(keep)]
    CL = sel(clip)
    G = sel(grp)
    SG = sel(sig)  # 40-byte fmx_signal_level records
    recs = [[fmx.SignalLevel.from_buffer_copy(SG[b, j].tobytes()) for j in range(len(keep))] for b in range(nblk)]
    stereo_all = ints[1].float().mean(dim=1).cpu().numpy()
    if all_groups is not None:
        ga = grp.cpu().numpy()  # [nblk][C][GS][4]
        gca = ints[3].cpu().numpy()
        per = [_groups_of(ga[b], gca[b], GS) for b in range(nblk)]
        all_groups.extend([g for b in range(nblk) for g in per[b][c]] for c in range(C))
        del ga
    res = []
    for b in range(nblk):
        d = dict(pcm_l=PL[b], pcm_r=PR[b], count=I[0, b], stereo=I[1, b], pilot=I[2, b], indicator=I[4, b],
                 clip=CL[b], groups=_groups_of(G[b], I[3, b], GS), sig=recs[b])
        d["mpx"] = MPX[b] if with_mpx else None
        res.append(d)
    iq_keep = d_iq.index_select(0, kidx).cpu().numpy()
    h.close()
    return res, iq_keep, tx[keep], stereo_all, kt


def run_gpu_sampled(fmx, torch, cfg, C, scfg, nblk, keep, setup=None, retunes=None, n_bits=None):
    """Full-size run: C channels of synthetic IQ generated in HBM
    (fmx_synth_device), every block through fmx_process_block, and only the
    rows of the channels in `keep` copied back.  setup: [(key, value,
    channel)] applied after creation; retunes: {block: (channel, mute)}.
    Returns (per-block results indexed by position in keep, host IQ rows of
    keep [len(keep)][nblk * 2*B*M], transmitted groups of keep)."""
    import numpy as np
    B = cfg.block
    M = cfg.iq_rate // cfg.dsp_rate
    n_iq = B * M
    h = fmx.Handle(cfg, C)
    for (k, v, ch) in (setup or []):
        h.set_param(k, v, ch)
    dev = torch.device("cuda")
    bits, tx = fmx.synth_rds_bits(scfg, 0, C)
    d_bits = torch.from_numpy(bits).to(dev)
    row = 2 * n_iq * nblk
    d_iq = torch.empty((C, row), dtype=torch.uint8, device=dev)
    h.synth_device(scfg, 0, C, 0, n_iq * nblk, d_bits.data_ptr(), d_iq.data_ptr(), row)
    kidx = torch.tensor(keep, dtype=torch.long, device=dev)
    mpx = torch.zeros((C, B), dtype=torch.float32, device=dev)
    pl = torch.zeros((C, B), dtype=torch.float32, device=dev)
    pr = torch.zeros((C, B), dtype=torch.float32, device=dev)
    cnt = torch.zeros(C, dtype=torch.int32, device=dev)
    st = torch.zeros(C, dtype=torch.int32, device=dev)
    pil = torch.zeros(C, dtype=torch.int32, device=dev)
    clip = torch.zeros(C, dtype=torch.float32, device=dev)
    ind = torch.zeros(C, dtype=torch.int32, device=dev)
    GS = 8
    grp = torch.zeros((C, GS, 4), dtype=torch.int32, device=dev)
    gcnt = torch.zeros(C, dtype=torch.int32, device=dev)
    out = fmx.BlockOut(mpx.data_ptr(), B, pl.data_ptr(), pr.data_ptr(), B, cnt.data_ptr(),
                       st.data_ptr(), pil.data_ptr(), clip.data_ptr(), grp.data_ptr(), GS,
                       gcnt.data_ptr(), None, ind.data_ptr())
    res = []
    for b in range(nblk):
        if retunes and b in retunes:
            h.retune(*retunes[b])
        h.process_block(d_iq.data_ptr() + b * 2 * n_iq, row, B, out)
        h.sync()
        sel = lambda t: t.index_select(0, kidx).cpu().numpy().copy()  # noqa: E731
        g = sel(grp).view(np.uint8).reshape(len(keep), GS, 16)
        gc = sel(gcnt)
        groups = []
        for j in range(len(keep)):
            lst = []
            for k in range(min(int(gc[j]), GS)):
                w = g[j, k]
                a, bb, cc, d = np.frombuffer(w[:8].tobytes(), dtype=np.uint16)
                lst.append((int(a), int(bb), int(cc), int(d), int(w[8])))
            groups.append(lst)
        res.append(dict(mpx=sel(mpx), pcm_l=sel(pl), pcm_r=sel(pr), count=sel(cnt), stereo=sel(st),
                        pilot=sel(pil), clip=sel(clip), indicator=sel(ind), groups=groups,
                        stereo_all=float(st.float().mean().item())))
    iq_keep = d_iq.index_select(0, kidx).cpu().numpy()
    h.close()
    return res, iq_keep, tx[keep]


# ---- caller geometry: buffers inside larger sentinel-filled allocations ----
SENTINEL_F32 = 0x7FC0DEAD   # a quiet NaN no kernel produces
SENTINEL_BYTE = 0xA5        # bytes and ints (0xA5A5A5A5)


class Guarded:
    """A caller-owned buffer of `rows` rows of `stride` cells whose base lies
    `off` cells inside a larger allocation filled with a sentinel (`tail`
    more cells behind the last row).  kind: "f32", "i32" or "u8"; `cell`:
    elements per cell (4 x i32 for a 16-byte fmx_rds_group record).  The
    allocation itself is torch's (256-B aligned), so `off` alone sets the
    base's alignment."""

    def __init__(self, torch, kind, rows, stride, off=1, tail=21, cell=1):
        self.kind, self.rows, self.stride, self.off, self.cell = kind, rows, stride, off, cell
        self.ncell = off + rows * stride + tail
        dev = torch.device("cuda")
        if kind == "u8":
            self.t = torch.empty(self.ncell * cell, dtype=torch.uint8, device=dev)
            self.pat, self.raw_dtype = SENTINEL_BYTE, np.uint8
        else:
            self.t = torch.empty(self.ncell * cell, dtype=torch.int32, device=dev)
            self.pat = SENTINEL_F32 if kind == "f32" else SENTINEL_BYTE * 0x01010101
            self.raw_dtype = np.uint32
        self.fill()

    def fill(self):
        self.t.fill_(self.pat - (1 << 32) if self.pat >= (1 << 31) else self.pat)

    @property
    def ptr(self):
        return self.t.data_ptr() + self.off * self.cell * self.t.element_size()

    def raw(self):
        """The whole allocation on the host, unsigned."""
        return self.t.cpu().numpy().view(self.raw_dtype)

    def view(self, raw=None, dtype=None):
        """[rows][stride * cell] of the buffer proper (dtype: a numpy view type)."""
        raw = self.raw() if raw is None else raw
        v = raw[self.off * self.cell:(self.off + self.rows * self.stride) * self.cell].reshape(self.rows, -1)
        return v if dtype is None else v.view(dtype)

    def check(self, lens, tag, raw=None):
        """Every cell outside row r's first lens[r] cells (a scalar: every
        row's) still holds the sentinel -- before the base, between the rows'
        logical ends and the next row, behind the last row; a float cell
        inside holds none (it was written)."""
        raw = self.raw() if raw is None else raw
        lens = np.broadcast_to(np.asarray(lens, dtype=np.int64), (self.rows,))
        assert np.all(lens >= 0) and np.all(lens <= self.stride), (tag, lens.min(), lens.max(), self.stride)
        inside = np.zeros(self.ncell, dtype=bool)
        col = np.arange(self.stride)
        inside[self.off:self.off + self.rows * self.stride] = (col[None, :] < lens[:, None]).reshape(-1)
        cellmask = np.repeat(inside, self.cell)
        bad = np.nonzero(~cellmask & (raw != self.pat))[0]
        assert bad.size == 0, (tag, "guard cells overwritten", bad.size,
                               [(int(i) // self.cell - self.off) for i in bad[:8]])
        if self.kind == "f32":
            assert not np.any(raw[cellmask] == self.pat), (tag, "logical cells left unwritten")


def records_to_groups(rec_u8, counts, stride):
    """rec_u8: uint8 [C][stride * 16] fmx_rds_group records -> per channel
    [(a, b, c, d, errors)] of its first min(count, stride) records."""
    out = []
    for c in range(len(counts)):
        lst = []
        for k in range(min(int(counts[c]), stride)):
            w = rec_u8[c, 16 * k:16 * k + 16]
            a, bb, cc, d = np.frombuffer(w[:8].tobytes(), dtype=np.uint16)
            lst.append((int(a), int(bb), int(cc), int(d), int(w[8])))
        out.append(lst)
    return out


def skewed_iq(torch, iq, off, pad):
    """The rows of iq (uint8 [C][row]) on the device at byte offset `off` of
    an allocation, `row + pad` bytes apart.  -> (tensor, base address, stride)."""
    C, row = iq.shape
    stride = row + pad
    t = torch.full((off + C * stride + 64,), SENTINEL_BYTE, dtype=torch.uint8, device=torch.device("cuda"))
    t[off:off + C * stride].view(C, stride)[:, :row] = torch.from_numpy(np.ascontiguousarray(iq)).to(t.device)
    return t, t.data_ptr() + off, stride


def run_gpu_geometry(fmx, torch, cfg, iq, nblk, geom, ktimes=None):
    """run_gpu_pipeline on caller geometry: every output of fmx_process_block
    lives in a Guarded allocation, refilled with the sentinel before each call
    and checked after it (MPX [c][0..n), PCM [c][0..count[c]), groups
    [c][0..min(count, stride)), the per-channel vectors [0..C)).
    geom: mpx / pcm = (base offset, stride) in floats, grp = (offset, stride)
    in records, iq = (byte offset, bytes added to the row).  Returns the
    per-block dicts of run_gpu_pipeline (PCM rows cut to the stride)."""
    C = iq.shape[0]
    B = cfg.block
    M = cfg.iq_rate // cfg.dsp_rate
    n = B
    h = fmx.Handle(cfg, C)
    keep, iq_base, iq_stride = skewed_iq(torch, iq, *geom["iq"])
    mo, ms = geom["mpx"]
    po, ps = geom["pcm"]
    go, gs = geom["grp"]
    G = dict(mpx=Guarded(torch, "f32", C, ms, off=mo), pl=Guarded(torch, "f32", C, ps, off=po),
             pr=Guarded(torch, "f32", C, ps, off=po), grp=Guarded(torch, "i32", C, gs, off=go, cell=4),
             clip=Guarded(torch, "f32", 1, C))
    for k in ("cnt", "st", "pil", "ind", "gcnt"):
        G[k] = Guarded(torch, "i32", 1, C)
    out = fmx.BlockOut(G["mpx"].ptr, ms, G["pl"].ptr, G["pr"].ptr, ps, G["cnt"].ptr, G["st"].ptr, G["pil"].ptr,
                       G["clip"].ptr, G["grp"].ptr, gs, G["gcnt"].ptr, None, G["ind"].ptr)
    if ktimes is not None:
        h.timing_enable(True)
    res = []
    for b in range(nblk):
        for g in G.values():
            g.fill()
        torch.cuda.synchronize()
        h.process_block(iq_base + b * 2 * n * M, iq_stride, n, out)
        h.sync()
        R = {k: g.raw() for k, g in G.items()}
        vec = {k: G[k].view(R[k], np.float32 if k == "clip" else np.int32)[0].copy()
               for k in ("cnt", "st", "pil", "ind", "gcnt", "clip")}
        tag = ("block", b)
        for k in vec:
            G[k].check(C, tag + (k,), R[k])
        assert np.all(vec["cnt"] >= 0) and np.all(vec["cnt"] <= ps), (tag, vec["cnt"])
        assert np.all(vec["gcnt"] >= 0), (tag, vec["gcnt"])
        G["mpx"].check(n, tag + ("mpx",), R["mpx"])
        G["pl"].check(vec["cnt"], tag + ("pcm_l",), R["pl"])
        G["pr"].check(vec["cnt"], tag + ("pcm_r",), R["pr"])
        G["grp"].check(np.minimum(vec["gcnt"], gs), tag + ("groups",), R["grp"])
        rec = G["grp"].view(R["grp"]).view(np.uint8)
        res.append(dict(mpx=G["mpx"].view(R["mpx"], np.float32)[:, :n].copy(),
                        pcm_l=G["pl"].view(R["pl"], np.float32).copy(), pcm_r=G["pr"].view(R["pr"], np.float32).copy(),
                        count=vec["cnt"], stereo=vec["st"], pilot=vec["pil"], clip=vec["clip"], indicator=vec["ind"],
                        groups=records_to_groups(rec, vec["gcnt"], gs), gcount=vec["gcnt"]))
    if ktimes is not None:
        ktimes.update(h.kernel_times())
    h.close()
    del keep
    return res


def run_gpu_unsynchronised(fmx, torch, cfg, d_iq, row, C, nblk, shared_mpx):
    """The bench's calling pattern -- every block through fmx_process_block
    with NO host synchronisation in between -- with either one MPX buffer that
    every call is given (shared_mpx) or one per block.  Every other output
    goes to per-block buffers.  -> dict of host arrays [nblk][C]...; "mpx":
    the last block's."""
    B = cfg.block
    M = cfg.iq_rate // cfg.dsp_rate
    dev = torch.device("cuda")
    h = fmx.Handle(cfg, C)
    GS = 8
    f = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)  # noqa: E731
    z = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)  # noqa: E731
    T = dict(pl=f(nblk, C, B), pr=f(nblk, C, B), clip=f(nblk, C), cnt=z(nblk, C), st=z(nblk, C), pil=z(nblk, C),
             ind=z(nblk, C), gcnt=z(nblk, C), grp=z(nblk, C, GS, 4))
    mpx = f(1 if shared_mpx else nblk, C, B)
    torch.cuda.synchronize()
    for b in range(nblk):
        m = mpx[0 if shared_mpx else b]
        out = fmx.BlockOut(m.data_ptr(), B, T["pl"][b].data_ptr(), T["pr"][b].data_ptr(), B, T["cnt"][b].data_ptr(),
                           T["st"][b].data_ptr(), T["pil"][b].data_ptr(), T["clip"][b].data_ptr(),
                           T["grp"][b].data_ptr(), GS, T["gcnt"][b].data_ptr(), None, T["ind"][b].data_ptr())
        h.process_block(d_iq.data_ptr() + b * 2 * B * M, row, B, out)
    h.sync()
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in T.items()}
    res["mpx"] = mpx[-1].cpu().numpy()
    h.close()
    return res


# ---- the stage entry points over 19 channels: call schedule and oracle objects ----
# (tests/test_gpu_abi_geometry.py runs it on the GPU, tests/test_abi_stage_plan.py
# checks on the CPU that the oracle decides this input the same way under ten
# times the GPU's MPX error)
STAGE_C = 19
STAGE_CH0 = 700
# call sizes: whole blocks, then ragged ones (1, 2 and 17 samples, sizes that
# are no multiple of 16 or of 4, 1023 / 1024 / 1025 around k_fe8's least call),
# then whole blocks until RDS groups appear
STAGE_SIZES = [4096, 4096, 333, 1, 17, 1500, 4096, 2, 1023, 1024, 1025, 4096, 4096, 4096] + [4096] * 8
STAGE_RESETS = {6: (5, 18)}  # before call 6: fmx_reset of channels 5 and 18
# before call 8, (key, value, channel) of fmx_set_param
STAGE_PARAMS = {8: (("force_mono", 1, 2), ("deemph_us", 60, 16), ("deviation_hz", 70000, 1))}


def stage_iq(fmx, iq_rate=2_400_000, M=10, C=STAGE_C, ch0=STAGE_CH0, sizes=STAGE_SIZES, kind=2, **synth):
    """uint8 [C][2 * sum(sizes) * M] of the synthetic plan's channels ch0 .. ch0 + C - 1."""
    scfg = fmx.make_synth(iq_rate=iq_rate, kind=kind, n_bits=8192, **synth)
    bits, _ = fmx.synth_rds_bits(scfg, ch0, C)
    return fmx.synth_host(scfg, ch0, C, 0, sum(sizes) * M, bits)


class OracleChannel:
    """One channel's five reference objects as constructed (75 us, the ctor's
    IQ filter), with the resets and setters of the stage schedule."""

    def __init__(self, oracle, M=10, fs=240_000):
        self.o, self.L = oracle, oracle.lib()
        L = self.L
        tpp = 28 if M >= 8 else (20 if M >= 4 else 12)
        self.dec = L.oracle_decim_create(M, tpp, 80.0) if M > 1 else None
        self.dem = L.oracle_demod_create(fs, 32_000)
        self.ste = L.oracle_stereo_create(fs, 32_000)
        self.af = L.oracle_afpost_create(fs, 32_000)
        self.rds = L.oracle_rds_create(fs)
        self.M = M

    def close(self):
        L = self.L
        if self.dem is None:
            return
        if self.dec:
            L.oracle_decim_destroy(self.dec)
        L.oracle_demod_destroy(self.dem)
        L.oracle_stereo_destroy(self.ste)
        L.oracle_afpost_destroy(self.af)
        L.oracle_rds_destroy(self.rds)
        self.dem = None

    __del__ = close

    def reset(self):
        L = self.L
        if self.dec:
            L.oracle_decim_reset(self.dec)
        L.oracle_demod_reset(self.dem)
        L.oracle_stereo_reset(self.ste)
        L.oracle_afpost_reset(self.af)
        L.oracle_rds_reset(self.rds)

    def set_param(self, key, value):
        L = self.L
        if key == "force_mono":
            L.oracle_stereo_set(self.ste, 2, value)
        elif key == "deemph_us":
            L.oracle_demod_set(self.dem, 1, value)
            L.oracle_afpost_set_deemphasis(self.af, value)
        elif key == "deviation_hz":
            L.oracle_demod_set(self.dem, 5, value)
        else:
            raise KeyError(key)

    def decimate(self, iq_u8, n):
        out = np.zeros(2 * max(n, 1), np.float32)
        x = np.ascontiguousarray(iq_u8)
        k = self.L.oracle_decim_execute_complex(self.dec, x.ctypes.data, n * self.M, out.ctypes.data, n)
        assert k == n, (k, n)
        return out[:2 * n]

    def decimate_u8(self, iq_u8, n):
        out = np.zeros(2 * max(n, 1), np.uint8)
        x = np.ascontiguousarray(iq_u8)
        k = self.L.oracle_decim_execute(self.dec, x.ctypes.data, n * self.M, out.ctypes.data, n)
        assert k == n, (k, n)
        return out[:2 * n]

    def demod(self, bb, n):
        """-> (mpx [n], mono [k])"""
        x = np.ascontiguousarray(bb, dtype=np.float32)
        mpx, mono = np.zeros(max(n, 1), np.float32), np.zeros(max(n, 1), np.float32)
        k = self.L.oracle_demod_process_split_complex(self.dem, x.ctypes.data, mpx.ctypes.data, mono.ctypes.data, n)
        return mpx[:n], mono[:k]

    def demod_u8(self, iq_u8, n):
        """-> (mpx [n], mono [k], clip ratio)"""
        x = np.ascontiguousarray(iq_u8)
        mpx, mono = np.zeros(max(n, 1), np.float32), np.zeros(max(n, 1), np.float32)
        k = self.L.oracle_demod_process_split(self.dem, x.ctypes.data, mpx.ctypes.data, mono.ctypes.data, n)
        return mpx[:n], mono[:k], float(self.L.oracle_demod_clip_ratio(self.dem))

    def downsample(self, mpx, n):
        x = np.ascontiguousarray(mpx, dtype=np.float32)
        out = np.zeros(max(n, 1), np.float32)
        k = self.L.oracle_demod_downsample(self.dem, x.ctypes.data, out.ctypes.data, n)
        return out[:k]

    def stereo(self, mpx, n):
        """-> (left [n], right [n], stereo flag, pilot tenths)"""
        import ctypes as Ct
        x = np.ascontiguousarray(mpx, dtype=np.float32)
        l, r = np.zeros(max(n, 1), np.float32), np.zeros(max(n, 1), np.float32)
        s, p = Ct.c_int(), Ct.c_int()
        k = self.L.oracle_stereo_process(self.ste, x.ctypes.data, l.ctypes.data, r.ctypes.data, n, Ct.byref(s),
                                         Ct.byref(p))
        assert k == n, (k, n)
        return l[:n], r[:n], s.value, p.value

    def afpost(self, left, right, n, cap):
        x, y = np.ascontiguousarray(left, dtype=np.float32), np.ascontiguousarray(right, dtype=np.float32)
        ol, orr = np.zeros(max(cap, 1), np.float32), np.zeros(max(cap, 1), np.float32)
        k = self.L.oracle_afpost_process(self.af, x.ctypes.data, y.ctypes.data, n, ol.ctypes.data, orr.ctypes.data,
                                         cap)
        return ol[:k], orr[:k]

    def rds_groups(self, mpx, n):
        x = np.ascontiguousarray(mpx, dtype=np.float32)
        g = (self.o.OracleGroup * 16)()
        ng = self.L.oracle_rds_process(self.rds, x.ctypes.data, n, g, 16, None, 0, None)
        assert ng <= 16
        return self.o.groups_to_tuples(g, ng)


def stage_events(ch, i, c):
    """Apply call i's resets and setters of the stage schedule to OracleChannel
    ch of channel c."""
    if c in STAGE_RESETS.get(i, ()):
        ch.reset()
    for (key, value, cc) in STAGE_PARAMS.get(i, ()):
        if cc == c:
            ch.set_param(key, value)
