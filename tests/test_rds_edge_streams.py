"""The inputs of tests/test_gpu_rds_edge_streams.py, made trustworthy on the
CPU before a GPU sees them: the golden block-sync streams
(tests/golden/blocksync.json, bits and the groups the reference's own
BlockStream emits) turned into waveforms by tests/rds_wave.py, through the
oracle's RDS stage and through the oracle's whole pipeline, must give the
fixture's groups back exactly.  Every choice of input -- the lead-ins, the
full-chain channel numbers, the noise seeds -- is made here, by the oracle
against the fixture or against itself, never by a GPU result."""
import numpy as np
import pytest

import rds_wave as W

FS = (240_000, 256_000)
STREAMS = [name for name, _, _ in W.fixture()]
DELAY = 3  # the oracle's demodulator hands the sent bits through three bits late


def _flat(per):
    return [g for call in per for g in call]


# ---- the helper itself ----
def test_mpx_from_bits_is_the_transmitters_rds_term():
    """Sample by sample against the formula, written out naively."""
    d = np.array([1, 0, 0, 1, 1, 1, 0, 1] * 6, np.uint8)
    fs = 240_000
    x = W.mpx_from_bits(d, fs)
    assert x.dtype == np.float32 and x.size == (d.size * fs * 2 // 2375) // 4096 * 4096 == 8192
    e = np.bitwise_xor.accumulate(d)
    assert list(e[:6]) == [1, 1, 1, 0, 1, 0]
    for t in list(range(0, 700)) + [4095, 4096, 8191]:
        h = (t * 2375) // fs
        s = (1.0 if e[h >> 1] else -1.0) * (-1.0 if h & 1 else 1.0)
        assert x[t] == np.float32(0.05 * s * np.sin(2 * np.pi * ((57000 * t) % fs) / fs)), t


def test_splitmix64_known_answers():
    # the published test vector of splitmix64 seeded with 0 (first two outputs)
    assert W.splitmix64(0) == 0xE220A8397B1DCDAF
    assert W.splitmix64(0x9E3779B97F4A7C15) == 0x6E789E6AA1B965F4


@pytest.mark.parametrize("iq_rate,dsp_rate", [(2_400_000, 240_000), (2_048_000, 256_000)])
def test_synth_table_puts_the_pattern_where_predicted(fmx, oracle, iq_rate, dsp_rate):
    """A known random pattern transmitted by fmx.synth_host from synth_table's
    table comes out of the oracle (pipeline -> MPX -> RDS stage) as the same
    bits at one constant delay for channels with different bit-clock offsets:
    a wrong k0 would move a channel's pattern by the error."""
    n_data = 420
    d = np.random.default_rng(11).integers(0, 2, n_data, dtype=np.uint8)
    n_bits = n_data + 40
    M = iq_rate // dsp_rate
    nblk = int(n_data / 1187.5 * dsp_rate / 4096)
    scfg = fmx.make_synth(iq_rate=iq_rate, kind=2, seed_base=0xF00D, n_bits=n_bits)
    chans = (100, 101, 4242)
    offs = [W.rds_off(scfg.seed_base, ch, iq_rate) for ch in chans]
    assert len({((o * 2375) // iq_rate) >> 1 for o in offs}) == 3  # three different k0
    delays = []
    for ch in chans:
        table = W.synth_table(d, scfg.seed_base, ch, iq_rate, n_bits)
        iq = fmx.synth_host(scfg, ch, 1, 0, 4096 * M * nblk, table[None, :])[0]
        p = oracle.Pipeline(oracle.make_cfg(iq_rate=iq_rate, dsp_rate=dsp_rate))
        mpx = np.concatenate([p.block(iq[b * 2 * 4096 * M:(b + 1) * 2 * 4096 * M])["mpx"] for b in range(nblk)])
        _, bits = W.oracle_rds_calls(oracle, mpx, dsp_rate)
        ok = [dl for dl in range(0, 12) if bits.size - dl >= 300
              and np.array_equal(bits[70 + dl:bits.size], d[70:bits.size - dl])]
        assert len(ok) == 1, (ch, ok)
        delays.append(ok[0])
    # the stage's own delay is 3 (test_stage_oracle_gives_the_fixture_groups);
    # where sample 0 falls late in bit k0 the decoder never sees that bit and
    # counts from the next one: 2.  A channel that starts in the first half
    # of its bit must show 3 -- a k0 off by one would show 2 or 4 there
    fracs = [((o * 2375) % (2 * iq_rate)) / (2 * iq_rate) for o in offs]
    assert sum(f < 0.5 for f in fracs) >= 1
    for f, dl in zip(fracs, delays):
        assert dl == DELAY if f < 0.5 else dl in (DELAY - 1, DELAY), (fracs, delays)


# ---- A1: stage level, the oracle against the fixture ----
def _bits_follow(bits, sent, upto=None):
    """The decoded bits are the sent bits DELAY late from bit 60 to the row's
    end (the row is cut to whole calls: up to 21 bits and the delay short),
    or to bit `upto`."""
    n = min(bits.size - DELAY, sent.size)
    if n < sent.size - 30:
        return False
    n = min(n, upto or n)
    return np.array_equal(bits[60 + DELAY:n + DELAY], sent[60:n])


@pytest.mark.parametrize("fs", FS)
@pytest.mark.parametrize("lead", W.LEADS)
@pytest.mark.parametrize("si", range(8), ids=STREAMS)
def test_stage_oracle_gives_the_fixture_groups(oracle, si, lead, fs):
    """Every stream x lead-in x rate behind a tail of 130 zero bits, in calls
    of 4096: the groups begin with the fixture's list exactly and the decoded
    bits are the sent bits three bits late from bit 60 on, through the stream
    and 63 bits of the tail: the first 64-bit window of the biphase decoder
    that holds zero bits only makes it slip
    (test_long_zero_tail_is_no_input_for_an_exact_comparison).  (What follows the
    fixture's list -- at most a (0,0,0,0,255) group out of the tail -- is not
    asserted.)"""
    _, stream, want = W.fixture()[si]
    sent = W.padded(stream, lead)
    assert sent.size - lead - stream.size >= 130
    per, bits = W.oracle_rds_calls(oracle, W.mpx_from_bits(sent, fs), fs)
    assert _flat(per)[:len(want)] == want
    assert _bits_follow(bits, sent, upto=lead + stream.size + 63)


def test_long_zero_tail_is_no_input_for_an_exact_comparison(oracle):
    """Why the common-length rows are not padded with zero bits (rds_wave.PAD):
    the biphase decoder (subcarrier.cpp:50-86) re-decides its clock polarity
    every 128 symbols from the summed |differences| at even and at odd
    symbols.  Zero data bits are a bare alternation of half-bit symbols, the
    two sums are then equal but for rounding, and the first window of 64 bits
    with nothing else in it flips the polarity: behind `clean` every bit comes
    through for at least 64 bits of the tail, and then one does not."""
    _, stream, _ = W.fixture()[0]
    sent = np.concatenate([stream, np.zeros(900, np.uint8)])
    _, bits = W.oracle_rds_calls(oracle, W.mpx_from_bits(sent, 240_000), 240_000)
    n = min(bits.size - DELAY, sent.size)
    bad = np.flatnonzero(bits[DELAY:n + DELAY] != sent[:n])
    bad = bad[bad >= 60]
    assert bad.size and stream.size + 64 <= bad[0] < stream.size + 192, bad[:4]


@pytest.mark.parametrize("fs", FS)
def test_stage_rows_of_the_gpu_test_are_suitable(oracle, fs):
    """The 72 rows tests/test_gpu_rds_edge_streams.py feeds fmx_rds (stream
    c % 8 behind LEADS[c // 8], padded to one length): the oracle's groups
    begin with the fixture's list, its decoded bits follow the sent bits to
    the row's end, and four copies perturbed by about ten times the
    GPU-to-oracle MPX RMS give the same groups in the same calls and the same
    bits from bit 60 on -- no decision on these rows hangs on a tie."""
    sent = W.stage_bits()
    res = W.stage_oracle(oracle, fs)

    def stable(c):
        per, bits = res[c]
        x = W.mpx_from_bits(sent[c], fs)
        for ps in (100, 101, 102, 103):
            per2, bits2 = W.oracle_rds_calls(oracle, W.perturbed(x, ps), fs)
            if per2 != per or bits2.size != bits.size or not np.array_equal(bits2[60:], bits[60:]):
                return False
        return True

    ok = W.pmap(stable, range(72))
    for c in range(72):
        per, bits = res[c]
        want = W.fixture()[c % 8][2]
        assert _flat(per)[:len(want)] == want, c
        assert _bits_follow(bits, sent[c]), c
        assert ok[c], c
        if c % 8 == 6:  # `noise`: no group up to the stream's end, lead-in or not
            end = (W.LEADS[c // 8] + 3000) * fs * 2 // 2375 // W.CALL
            assert _flat(per[:end]) == [], c


def test_mid_stream_resets_hit_rows_in_sync(oracle):
    """The GPU test's resets (rows c % 3 == 1 before call 60, every row
    before call 141) land on rows that are in sync -- a group in the 10 calls
    before, groups again after -- and the oracle, reset at the same calls,
    decides the same way on four perturbed copies of every row."""
    res = W.stage_oracle(oracle, 240_000, W.STAGE_RESETS)
    hit = W.resets_hit_synced_rows(res)
    assert len(hit[0]) >= 1 and len(hit[1]) >= 1, hit
    sent = W.stage_bits()

    def stable(c):
        rs = W.reset_calls(c, W.STAGE_RESETS)
        x = W.mpx_from_bits(sent[c], 240_000)
        return all(W.oracle_rds_calls(oracle, W.perturbed(x, ps), 240_000, resets=rs)[0] == res[c][0]
                   for ps in (100, 101, 102, 103))

    assert all(W.pmap(stable, range(72)))


@pytest.mark.parametrize("seq", list(W.BARELY_LONG))
def test_barely_long_call_sequences_are_decision_stable(oracle, seq):
    """The ring tests' short-after-barely-long call sequences
    (tests/test_gpu_rds_ring.py) on their 12 rows: the oracle, given the same
    call sizes and resets, emits at least 3 groups and emits the same groups
    in the same calls for four perturbed copies of every row."""
    sizes, resets = W.split_steps(W.BARELY_LONG[seq], W.BARELY_LONG_ROWS)
    rows = W.barely_long_rows()
    n = 0
    for c in range(W.BARELY_LONG_ROWS):
        per = W.oracle_rds_calls(oracle, rows[c], 240_000, sizes=sizes, resets=resets[c])[0]
        for ps in (100, 101, 102, 103):
            assert W.oracle_rds_calls(oracle, W.perturbed(rows[c], ps), 240_000, sizes=sizes,
                                      resets=resets[c])[0] == per, (c, ps)
        n += len(_flat(per))
    assert n >= 3


# ---- A2: the fixture holds what the GPU tests are meant to exercise ----
def test_fixture_covers_corrected_missing_and_lost_sync():
    fx = {name: groups for name, _, groups in W.fixture()}
    assert STREAMS == ["clean", "offset_start", "bursts", "flips_2e-2", "sync_loss", "slips", "noise", "two_stations"]
    codes = {k: W.block_codes(v) for k, v in fx.items()}
    assert codes["bursts"][1] >= 30
    for k in ("sync_loss", "slips", "two_stations"):
        assert codes[k][3] >= 30 and codes[k][1] >= 3, (k, codes[k])
    assert len(fx["slips"]) < len(fx["clean"])
    assert fx["noise"] == []
    # today's counts, code 0 / 1 / 3
    assert [(codes[k][0], codes[k][1], codes[k][3]) for k in ("bursts", "flips_2e-2", "sync_loss", "slips",
                                                              "two_stations")] == [
        (120, 37, 3), (93, 51, 16), (126, 3, 31), (69, 4, 83), (139, 3, 38)]


# ---- A3: full chain, the oracle against the fixture ----
def test_full_chain_oracle_gives_the_fixture_groups(fmx, oracle):
    """Channels 100..107 of the synthetic plan carry the eight streams behind
    131 one-bits.  The channel numbers are part of the test: on channels 1 and
    5 the front end's start transient moves the acquisition by a group, so
    those are no input for an exact comparison.  The pipeline's MPX through
    the RDS stage alone gives the pipeline's groups block by block, and so do
    four perturbed copies of it: the chain's decisions hang on no tie."""
    scfg, tables, nblk = W.chain_plan(fmx)
    assert nblk * 4096 * 1187.5 / 240_000 <= scfg.n_bits  # the table never wraps
    per, mpx, _ = W.chain_oracle(fmx, oracle)

    def stable(i):
        return all(W.oracle_rds_calls(oracle, x, 240_000)[0] == per[i]
                   for x in [mpx[i]] + [W.perturbed(mpx[i], ps) for ps in (100, 101, 102, 103)])

    ok = W.pmap(stable, range(8))
    for i, (name, _, want) in enumerate(W.fixture()):
        assert _flat(per[i])[:len(want)] == want, name
        assert ok[i], name


# ---- A4: the noise rows are decided the same way under a perturbation ----
@pytest.mark.parametrize("seed", W.NOISE_SEEDS)
def test_noise_rows_are_decision_stable(oracle, seed):
    """clean + gaussian noise of sigma 0.15: the oracle's groups and decoded
    bits are identical for the row and for four copies perturbed by about ten
    times the GPU-to-oracle MPX RMS of DESIGN 3 (sigma 0.2 is not stable: the
    oracle disagrees with itself there).  The row still has what the GPU test
    wants to see: corrected and missing blocks."""
    x = W.noise_row(seed)
    per, bits = W.oracle_rds_calls(oracle, x, 240_000)
    for ps in (100, 101, 102, 103):
        per2, bits2 = W.oracle_rds_calls(oracle, W.perturbed(x, ps), 240_000)
        assert per2 == per, ps
        assert np.array_equal(bits2, bits), ps
    codes = W.block_codes(_flat(per))
    assert codes[1] >= 5 and codes[3] >= 5, codes


def test_clean_row_beside_the_noise_rows_is_decision_stable(oracle):
    """The other 60 channels of the GPU noise test carry `clean` behind no
    lead-in with its 130-bit zero tail (the noise rows' own signal).  Decoded
    bits in such a tail do move under a perturbation, so what the GPU test
    compares is checked here: the groups of every call, the (0,0,0,0,255)
    group out of the tail included, are the same for twelve perturbed
    copies, and begin with the fixture's list."""
    x = W.mpx_from_bits(W.padded(W.fixture()[0][1], 0), 240_000)
    per = W.oracle_rds_calls(oracle, x, 240_000)[0]
    assert _flat(per)[:40] == W.fixture()[0][2]
    same = W.pmap(lambda ps: W.oracle_rds_calls(oracle, W.perturbed(x, ps), 240_000)[0] == per, range(100, 112))
    assert all(same), same
