"""The reference's block-sync edge streams through the GPU RDS decoder.

tests/golden/blocksync.json holds eight bit streams (clean, offset start,
correctable bursts, random flips, sync loss, bit slips, noise, a change of
station) with the groups the reference's own BlockStream emits for them.
Here they are transmitted verbatim -- as the transmitter's RDS term into
fmx_rds (the front end's resampler path, k_rds, k_bits' block sync one lane
per channel with neighbouring lanes in different sync states) and as
synthetic IQ through fmx_process_block (the k_rs path) -- and the decoded
groups must equal the oracle's call by call and begin with the fixture's
list.  Every comparison is exact.  The inputs (lead-ins, padding, reset
calls, channel numbers, noise seeds) are chosen and checked on the CPU by
tests/test_rds_edge_streams.py, never by a GPU result.
"""
import time

import numpy as np
import pytest

import gpu_harness as H
import rds_wave as W

pytestmark = pytest.mark.gpu

GS = 8


def _flat(per):
    return [g for call in per for g in call]


def run_stage(fmx, torch, cfg, rows, resets=None, n=W.CALL):
    """rows [C][ncalls * n] float32 through fmx_rds on one handle in calls of
    n; every call writes its own slice of one device buffer, one copy at the
    end.  resets {call: [channels]} (fmx_reset before that call).  -> per
    channel, per call group lists; GPU wall seconds of the calls."""
    C, total = rows.shape
    ncalls = total // n
    dev = torch.device("cuda")
    d_mpx = torch.from_numpy(np.ascontiguousarray(rows)).to(dev)
    grp = torch.zeros((ncalls, C, GS, 4), dtype=torch.int32, device=dev)
    cnt = torch.full((ncalls, C), -1, dtype=torch.int32, device=dev)
    h = fmx.Handle(cfg, C)
    h.sync()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(ncalls):
        for ch in (resets or {}).get(i, []):
            h.reset(ch)
        h.rds(d_mpx.data_ptr() + 4 * i * n, total, n, grp[i].data_ptr(), GS, cnt[i].data_ptr())
    h.sync()
    wall = time.perf_counter() - t0
    g, k = grp.cpu().numpy(), cnt.cpu().numpy()
    h.close()
    assert k.min() >= 0 and k.max() <= GS, (k.min(), k.max())  # every call wrote every channel's count
    per_call = [H._groups_of(g[i], k[i], GS) for i in range(ncalls)]
    return [[per_call[i][c] for i in range(ncalls)] for c in range(C)], wall


def _report(tag, gpu, wall):
    codes = W.block_codes([g for ch in gpu for g in _flat(ch)])
    print(f"\n{tag}: {sum(len(_flat(ch)) for ch in gpu)} groups compared, blocks clean/corrected/missing "
          f"{codes[0]}/{codes[1]}/{codes[3]}, GPU wall {wall:.2f} s")
    return codes


@pytest.mark.parametrize("rates", [dict(iq_rate=2_400_000, dsp_rate=240_000), dict(iq_rate=2_048_000, dsp_rate=256_000)],
                         ids=["240k", "256k"])
def test_edge_streams_through_fmx_rds(fmx, oracle, torch_cuda, rates):
    """72 channels on one handle, channel c carrying stream c % 8 behind
    LEADS[c // 8] one-bits, padded to one length (rds_wave.PAD): two k_bits
    waves, the second partial, nine k_rds workgroups.  Per channel the groups
    of every call equal the oracle's of that call, and the whole list begins
    with the fixture's."""
    fs = rates["dsp_rate"]
    gpu, wall = run_stage(fmx, torch_cuda, fmx.make_config(**rates), W.stage_rows(fs))
    ora = W.stage_oracle(oracle, fs)
    codes = _report(f"fmx_rds edge streams {fs}", gpu, wall)
    for c in range(72):
        name, _, want = W.fixture()[c % 8]
        for i, (a, b) in enumerate(zip(gpu[c], ora[c][0])):
            assert a == b, (c, name, i)
        assert len(gpu[c]) == len(ora[c][0])
        assert _flat(gpu[c])[:len(want)] == want, (c, name)
    # the GPU's own output holds what this test is about
    assert codes[1] >= 9 * (37 + 51 + 3 + 4 + 3) and codes[3] >= 9 * (3 + 16 + 31 + 83 + 38), codes
    for c in range(6, 72, 8):  # `noise`: nothing up to the stream's end
        end = (W.LEADS[c // 8] + 3000) * fs * 2 // 2375 // W.CALL
        assert _flat(gpu[c][:end]) == [], c


def test_edge_streams_with_resets_in_mid_stream(fmx, oracle, torch_cuda):
    """The same rows at 240 kHz on a fresh handle; fmx_reset of every channel
    c % 3 == 1 before call 60 and of all channels before call 141, the oracle
    reset at the same calls: identical groups call by call.  At least one
    reset channel was in sync at each reset (a group in the 10 calls before)
    and emits again after it."""
    resets = {call: ([-1] if sel is None else W.reset_rows(sel)) for call, sel in W.STAGE_RESETS}
    gpu, wall = run_stage(fmx, torch_cuda, fmx.make_config(), W.stage_rows(240_000), resets=resets)
    ora = W.stage_oracle(oracle, 240_000, W.STAGE_RESETS)
    hit = W.resets_hit_synced_rows(ora)
    assert len(hit[0]) >= 1 and len(hit[1]) >= 1, hit
    _report("fmx_rds edge streams with resets", gpu, wall)
    for c in range(72):
        for i, (a, b) in enumerate(zip(gpu[c], ora[c][0])):
            assert a == b, (c, i)
    plain = W.stage_oracle(oracle, 240_000)
    assert any(ora[c][0] != plain[c][0] for c in hit[1])  # the resets changed what is decoded


def test_edge_streams_through_the_full_chain(fmx, oracle, torch_cuda):
    """Channels 100..107 of the synthetic plan carry the eight streams behind
    131 one-bits (rds_wave.chain_plan): the IQ through fmx_process_block (the
    k_rs resampler path).  Per block each channel's groups equal the oracle
    pipeline's, each record's block_index names the call that emitted it, and
    the whole list begins with the fixture's."""
    torch = torch_cuda
    iq, nblk = W.chain_iq(fmx)
    per, _, _ = W.chain_oracle(fmx, oracle)
    t0 = time.perf_counter()
    g = H.run_gpu_pipeline(fmx, torch, fmx.make_config(), iq, nblk)
    wall = time.perf_counter() - t0
    gpu = [[g[b]["groups"][i] for b in range(nblk)] for i in range(8)]
    _report("process_block edge streams", gpu, wall)
    for i, (name, _, want) in enumerate(W.fixture()):
        for b in range(nblk):
            assert gpu[i][b] == per[i][b], (name, b)
            assert g[b]["group_block_index"][i] == [b] * len(gpu[i][b]), (name, b)
        assert _flat(gpu[i])[:len(want)] == want, name


def test_noise_rows_through_fmx_rds(fmx, oracle, torch_cuda):
    """`clean` under gaussian noise of sigma 0.15 (seeds chosen on the CPU:
    the oracle decides them the same way under ten times the GPU-to-oracle
    MPX difference) on channels 0, 7, 8 and 63 of a 64-channel handle, the
    rest carrying `clean`: identical groups call by call, and the GPU's own
    output has at least 5 corrected and 5 missing blocks on each noisy
    channel."""
    fs = 240_000
    clean = W.mpx_from_bits(W.padded(W.fixture()[0][1], 0), fs)
    rows = np.tile(clean, (64, 1))
    noisy = dict(zip((0, 7, 8, 63), W.NOISE_SEEDS))
    for c, seed in noisy.items():
        rows[c] = W.noise_row(seed, fs)
    gpu, wall = run_stage(fmx, torch_cuda, fmx.make_config(), rows)
    _report("fmx_rds noise rows", gpu, wall)
    want_clean = W.oracle_rds_calls(oracle, clean, fs)[0]
    assert _flat(want_clean)[:40] == W.fixture()[0][2]
    for c in range(64):
        want = W.oracle_rds_calls(oracle, rows[c], fs)[0] if c in noisy else want_clean
        for i, (a, b) in enumerate(zip(gpu[c], want)):
            assert a == b, (c, i)
        if c in noisy:
            codes = W.block_codes(_flat(gpu[c]))
            print(f"noise seed {noisy[c]} channel {c}: corrected {codes[1]}, missing {codes[3]}")
            assert codes[1] >= 5 and codes[3] >= 5, (c, codes)
