"""The RDS ring as checkpoints (round 6).

k_rds keeps the last 256 mixed RDS-rate samples of every channel (the
reference's 255-tap FIR window, which SubcarrierSet::reset keeps,
subcarrier.cpp:108) for the partial-sum rebuild after a reset moves the
decimation phase.  Round 5 wrote that ring every call: 2 KB per channel per
step, 8.4 of k_rds's 10.5 MB written per launch at 4096 channels.  Round 6:
a call of >= 256 samples writes per-round NCO checkpoints instead, and the
ring is refilled from them and the call's RDS-rate input (still in its
intermediate slot) where it is needed -- a reset's rebuild, a short call
after a long one, fmx_diag_rds_ring.

Checked here against the round-5 behaviour on the same handle shape
(fmx_diag_set(FMX_DIAG_RDS_RING_ALWAYS)): the refilled ring equals the ring
k_rds wrote, bit for bit, and every output of the two handles is identical
through resets and mixed long / short calls -- process_block (pipelined
streams) and the fmx_rds stage entry point; the groups also against the
oracle."""
import numpy as np
import pytest

import gpu_harness as H
import rds_wave as W
from test_gpu_parity import make_iq

pytestmark = pytest.mark.gpu

RING_ALWAYS = 1


def _rings(hs, chans):
    return [[h.diag_rds_ring(c) for c in chans] for h in hs]


def _assert_rings_equal(hs, chans, tag):
    ra, rb = _rings(hs, chans)
    for c, a, b in zip(chans, ra, rb):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (tag, c, np.argwhere(a != b)[:5])
        assert np.any(a != 0.0), (tag, c)  # a ring of real samples, not the creation zeros


def test_ring_refill_matches_written_ring_process_block(fmx, oracle, torch_cuda):
    """20 channels (three k_rds workgroups, the last partial) through
    process_block on two handles, one writing the ring every call; resets of
    channels 3 and 17 before block 6 and of every channel before block 12
    (the rebuild reads the refilled ring); rings compared after blocks 3, 6,
    12 and 19, all outputs compared every block, groups against the oracle."""
    torch = torch_cuda
    C, nblk, B, M = 20, 20, 4096, 10
    iq, _ = make_iq(fmx, 2, C, nblk, ch0=300)
    cfg = fmx.make_config()
    dev = torch.device("cuda")
    d_iq = torch.from_numpy(np.ascontiguousarray(iq)).to(dev)
    hs = [fmx.Handle(cfg, C), fmx.Handle(cfg, C)]
    hs[1].diag_set(RING_ALWAYS, 1)
    GS = 8

    def bufs():
        return dict(mpx=torch.zeros((C, B), dtype=torch.float32, device=dev),
                    pl=torch.zeros((C, B), dtype=torch.float32, device=dev),
                    pr=torch.zeros((C, B), dtype=torch.float32, device=dev),
                    cnt=torch.zeros(C, dtype=torch.int32, device=dev),
                    st=torch.zeros(C, dtype=torch.int32, device=dev),
                    pil=torch.zeros(C, dtype=torch.int32, device=dev),
                    clip=torch.zeros(C, dtype=torch.float32, device=dev),
                    grp=torch.zeros((C, GS, 4), dtype=torch.int32, device=dev),
                    gcnt=torch.zeros(C, dtype=torch.int32, device=dev),
                    ind=torch.zeros(C, dtype=torch.int32, device=dev))

    bs = [bufs(), bufs()]
    outs = [fmx.BlockOut(b["mpx"].data_ptr(), B, b["pl"].data_ptr(), b["pr"].data_ptr(), B, b["cnt"].data_ptr(),
                         b["st"].data_ptr(), b["pil"].data_ptr(), b["clip"].data_ptr(), b["grp"].data_ptr(), GS,
                         b["gcnt"].data_ptr(), None, b["ind"].data_ptr()) for b in bs]
    resets = {6: [3, 17], 12: [-1]}
    groups = [[[] for _ in range(C)] for _ in range(2)]
    for blk in range(nblk):
        for h in hs:
            for ch in resets.get(blk, []):
                h.reset(ch)
        for h, o in zip(hs, outs):
            h.process_block(d_iq.data_ptr() + blk * 2 * B * M, iq.shape[1], B, o)
        for h in hs:
            h.sync()
        for k in ("mpx", "pl", "pr", "cnt", "st", "pil", "gcnt", "grp", "ind"):
            a, b = bs[0][k].cpu().numpy(), bs[1][k].cpu().numpy()
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (blk, k)
        g = bs[0]["grp"].cpu().numpy().view(np.uint8).reshape(C, GS, 16)
        gc = bs[0]["gcnt"].cpu().numpy()
        for c in range(C):
            for q in range(min(int(gc[c]), GS)):
                w = g[c, q]
                a, bb, cc, d = np.frombuffer(w[:8].tobytes(), dtype=np.uint16)
                groups[0][c].append((int(a), int(bb), int(cc), int(d), int(w[8])))
        if blk in (3, 6, 12, 19):
            _assert_rings_equal(hs, [0, 3, 7, 8, 17, 19], f"block {blk}")
    for h in hs:
        h.close()
    ngroups = 0
    for c in (0, 3, 17):
        rs = {b: c for b, lst in resets.items() if c in lst or -1 in lst}
        o = H.run_oracle_pipeline(oracle, oracle.make_cfg(), iq[c], nblk, resets=rs)
        og = [tuple(x) for blk in o for x in blk["groups"]]
        assert groups[0][c] == og, c
        ngroups += len(og)
    assert ngroups >= 3


def test_ring_refill_short_and_long_rds_calls(fmx, torch_cuda):
    """fmx_rds (RDSDecoder::process) on two handles with calls of 4096, 300
    (213 RDS-rate samples: k_rds refills the ring before writing its own
    samples) and 1000 MPX samples in a mixed order, resets between some of
    them; rings compared after every call, groups identical."""
    torch = torch_cuda
    C, B = 12, 4096
    nblk = 6
    cfg = fmx.make_config()
    # MPX rows from the full pipeline (a real RDS subcarrier)
    iq, _ = make_iq(fmx, 2, C, nblk, ch0=500)
    g = H.run_gpu_pipeline(fmx, torch, cfg, iq, nblk)
    mpx = np.concatenate([blk["mpx"] for blk in g], axis=1)  # [C][nblk * B]
    dev = torch.device("cuda")
    d_mpx = torch.from_numpy(np.ascontiguousarray(mpx)).to(dev)
    row = mpx.shape[1]
    hs = [fmx.Handle(cfg, C), fmx.Handle(cfg, C)]
    hs[1].diag_set(RING_ALWAYS, 1)
    grp = [torch.zeros((C, 8, 4), dtype=torch.int32, device=dev) for _ in hs]
    gcnt = [torch.zeros(C, dtype=torch.int32, device=dev) for _ in hs]
    sizes = [4096, 4096, 300, 300, 4096, 1000, 300, 4096, 300, 4096, 4096, 1000]
    resets = {2: 5, 4: -1, 6: 11, 9: 0}
    pos = 0
    for i, n in enumerate(sizes):
        if pos + n > row:
            break
        for h in hs:
            if i in resets:
                h.reset(resets[i])
        for k, h in enumerate(hs):
            h.rds(d_mpx.data_ptr() + 4 * pos, row, n, grp[k].data_ptr(), 8, gcnt[k].data_ptr())
        for h in hs:
            h.sync()
        assert np.array_equal(gcnt[0].cpu().numpy(), gcnt[1].cpu().numpy()), i
        assert np.array_equal(grp[0].cpu().numpy(), grp[1].cpu().numpy()), i
        _assert_rings_equal(hs, [0, 5, 7, 11], f"call {i} (n={n})")
        pos += n
    for h in hs:
        h.close()


@pytest.mark.parametrize("ring_reads", ["every call", "after short calls"])
@pytest.mark.parametrize("seq", list(W.BARELY_LONG))
def test_ring_refill_previous_call_barely_long(fmx, oracle, torch_cuda, seq, ring_reads):
    """fmx_rds on two handles, one writing the ring every call, through short
    calls right after barely-long ones; after every call the rings are equal
    (and hold samples) and the groups are equal, and the first handle's groups
    equal the oracle's RDS stage given the same call sizes and resets, so the
    diagnostic handle is not the only witness.
    fmx_diag_rds_ring refills the ring of EVERY checkpointed channel from the
    intact row and marks it valid, so with a ring read after every call k_rds's
    own refill never runs; "after short calls" reads the rings only behind
    calls of <= 300 samples and at the end, which leaves the refill to k_rds.
    Consecutive fmx_rds calls share one slot, and the front end does write
    this call's samples over row[0 .. count) of the previous call's, but of
    the refilled entries only row[count_prev - 256 + count .. count_prev)
    outlive the call's own ring stores, and count_prev >= 256 (the comment in
    fmx_rds, fmx_capi.cpp)."""
    torch = torch_cuda
    C, fs = W.BARELY_LONG_ROWS, 240_000
    steps = W.BARELY_LONG[seq]
    sizes, want_resets = W.split_steps(steps, C)
    rows = W.barely_long_rows(fs)
    dev = torch.device("cuda")
    d_mpx = torch.from_numpy(np.ascontiguousarray(rows)).to(dev)
    row = rows.shape[1]
    hs = [fmx.Handle(fmx.make_config(), C), fmx.Handle(fmx.make_config(), C)]
    hs[1].diag_set(RING_ALWAYS, 1)
    grp = [torch.zeros((C, 8, 4), dtype=torch.int32, device=dev) for _ in hs]
    gcnt = [torch.zeros(C, dtype=torch.int32, device=dev) for _ in hs]
    got = [[] for _ in range(C)]  # per channel, per call
    pos = i = 0
    for s in steps:
        if not isinstance(s, int):
            for h in hs:
                h.reset(s[1])
            continue
        for k, h in enumerate(hs):
            h.rds(d_mpx.data_ptr() + 4 * pos, row, s, grp[k].data_ptr(), 8, gcnt[k].data_ptr())
        for h in hs:
            h.sync()
        k0, k1 = gcnt[0].cpu().numpy(), gcnt[1].cpu().numpy()
        g0, g1 = grp[0].cpu().numpy(), grp[1].cpu().numpy()
        assert np.array_equal(k0, k1), (i, s)
        for c, lst in enumerate(H._groups_of(g0, k0, 8)):
            assert lst == H._groups_of(g1[c:c + 1], k1[c:c + 1], 8)[0], (i, s, c)
            got[c].append(lst)
        if ring_reads == "every call" or s <= 300 or i == len(sizes) - 1:
            _assert_rings_equal(hs, [0, 5, 7, 11], f"call {i} (n={s})")
        pos += s
        i += 1
    for h in hs:
        h.close()
    ngroups = 0
    for c in range(C):
        want = W.oracle_rds_calls(oracle, rows[c], fs, sizes=sizes, resets=want_resets[c])[0]
        assert got[c] == want, c
        ngroups += sum(len(x) for x in want)
    assert ngroups >= 3
    print(f"\nbarely long {seq} / {ring_reads}: {ngroups} groups compared with the oracle")


@pytest.mark.parametrize("ring_reads", ["every call", "after short calls"])
def test_ring_refill_ragged_process_block_generic_front_end(fmx, oracle, torch_cuda, ring_reads):
    """process_block at 2.048 MS/s / 256 kHz (M = 8) with call sizes that are
    no multiple of 4 -- the generic k_frontend path, whose k_rds is not the
    fused one and so leaves the ring to checkpoints -- long (3001) and short
    (333: 222 RDS-rate samples) in a ragged order, a sync after every call
    (the refill logic only, not the streams).  A reset of channel 3 before
    call 4 (long after long: k_reset's refill shows in the rebuilt sums, that
    is in the outputs) and of channel 7 before call 9 (short after long: 34
    ring entries of k_reset's refill outlive the call).  Every output
    identical between the handle that checkpoints and the one that writes the
    ring, groups equal to the oracle pipeline's with the same sizes and
    resets, rings equal.
    A ring read (fmx_diag_rds_ring) refills every checkpointed channel's ring
    and marks it valid, so read after every call it leaves neither k_rds nor
    k_reset a refill to do; "after short calls" reads the rings only behind
    the 333-sample calls -- where k_rds's refill, or k_reset's, must have run
    first -- and behind the last call."""
    torch = torch_cuda
    C, B, M = 20, 4096, 8
    rates = dict(iq_rate=2_048_000, dsp_rate=256_000)
    sizes = [3001, 3001, 333, 3001] + [3001, 333, 333, 3001] * 9
    resets = {4: 3, 9: 7}
    assert sizes[8] == 3001 and sizes[9] == 333
    assert len(sizes) == 40 and all(n % 4 for n in sizes)
    iq, _ = make_iq(fmx, 2, C, 1, iq_rate=rates["iq_rate"], M=M, ch0=300, n=sum(sizes))
    cfg = fmx.make_config(**rates)
    dev = torch.device("cuda")
    d_iq = torch.from_numpy(np.ascontiguousarray(iq)).to(dev)
    hs = [fmx.Handle(cfg, C), fmx.Handle(cfg, C)]
    hs[1].diag_set(RING_ALWAYS, 1)
    GS = 8

    def bufs():
        f = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)  # noqa: E731
        z = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)  # noqa: E731
        return dict(mpx=f(C, B), pl=f(C, B), pr=f(C, B), cnt=z(C), st=z(C), pil=z(C), clip=f(C), grp=z(C, GS, 4),
                    gcnt=z(C), ind=z(C))

    bs = [bufs(), bufs()]
    outs = [fmx.BlockOut(b["mpx"].data_ptr(), B, b["pl"].data_ptr(), b["pr"].data_ptr(), B, b["cnt"].data_ptr(),
                         b["st"].data_ptr(), b["pil"].data_ptr(), b["clip"].data_ptr(), b["grp"].data_ptr(), GS,
                         b["gcnt"].data_ptr(), None, b["ind"].data_ptr()) for b in bs]
    got = [[] for _ in range(C)]
    pos = 0
    for i, n in enumerate(sizes):
        for h, o in zip(hs, outs):
            if i in resets:
                h.reset(resets[i])
            h.process_block(d_iq.data_ptr() + 2 * M * pos, iq.shape[1], n, o)
            h.sync()
        for k in ("cnt", "st", "pil", "gcnt", "grp", "ind"):
            a, b = bs[0][k].cpu().numpy(), bs[1][k].cpu().numpy()
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (i, k)
        for k, w in (("mpx", n), ("pl", B), ("pr", B)):
            a, b = bs[0][k][:, :w].cpu().numpy(), bs[1][k][:, :w].cpu().numpy()
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (i, k)
        for c, lst in enumerate(H._groups_of(bs[0]["grp"].cpu().numpy(), bs[0]["gcnt"].cpu().numpy(), GS)):
            got[c].append(lst)
        if ring_reads == "every call" or n == 333 or i == len(sizes) - 1:
            _assert_rings_equal(hs, [0, 3, 7, 8, 19], f"call {i} (n={n})")
        pos += n
    for h in hs:
        h.close()
    ngroups = 0
    for c in (0, 3, 7, 8, 19):
        p = oracle.Pipeline(oracle.make_cfg(**rates))
        want, pos = [], 0
        for i, n in enumerate(sizes):
            if resets.get(i) == c:
                p.reset()
            want.append(p.block(iq[c, 2 * M * pos:2 * M * (pos + n)])["groups"])
            pos += n
        assert got[c] == want, c
        ngroups += sum(len(x) for x in want)
    assert ngroups >= 3
