"""RDS test inputs made from bit streams (plain numpy, no GPU), and the
oracle's RDS stage behind two small wrappers.

The golden block-sync streams (tests/golden/blocksync.json: data bits and the
groups the reference's own BlockStream emits for them) reach the GPU decoder
as waveforms: mpx_from_bits() is the synthetic transmitter's RDS term
(fmx_synth.h, fmx_synth_fm_phase) on its own -- an MPX row for fmx_rds --
and synth_table() lays a stream into the cyclic encoded bit table
fmx.synth_host takes, so that the channel's first transmitted bit is the
stream's first.  The inputs are chosen on the CPU only
(tests/test_rds_edge_streams.py); the GPU tests read them from here.
"""
import ctypes as C
import functools
import json
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")

CALL = 4096
# lead-ins of one-bits in front of a stream.  52 is left out on purpose: two
# whole all-ones blocks change the oracle's acquisition (the fixture's first
# group is then missed), so it is no input for an exact comparison.
LEADS = (0, 1, 5, 13, 26, 37, 77, 104, 131)
TAIL = 130  # data bits after a stream, at least
# PAD.  Rows of one common length are filled up behind the stream with seeded
# random data bits, not with zero bits: zero data bits are a bare alternation
# of half-bit symbols, and the biphase decoder (subcarrier.cpp:50-86), which
# re-decides its clock polarity every 128 symbols from the summed differences
# at even and at odd symbols, decides the first 64-bit window that holds
# nothing else on a tie.  The oracle's decoded bits and, in places, its
# groups then change under a perturbation of 1e-5 of the input, so such a
# tail is no input for an exact comparison
# (tests/test_rds_edge_streams.py).  Block sync is causal: the pad cannot
# change the groups the stream itself gives.
WORKERS = min(8, os.cpu_count() or 1)
_MASK = (1 << 64) - 1


@functools.lru_cache(maxsize=None)
def fixture():
    """[(name, data bits uint8, [(a, b, c, d, errors), ...])] in file order."""
    with open(os.path.join(GOLD, "blocksync.json")) as f:
        fx = json.load(f)["streams"]
    return [(s["name"], np.frombuffer(s["bits"].encode(), dtype=np.uint8) - ord("0"),
             [tuple(g) for g in s["groups"]]) for s in fx]


def block_codes(groups):
    """Counts of the per-block error codes (two bits per block, block A in the
    top two: 0 clean, 1 corrected, 3 missing) over a group list."""
    n = {0: 0, 1: 0, 2: 0, 3: 0}
    for g in groups:
        for sh in (6, 4, 2, 0):
            n[(g[4] >> sh) & 3] += 1
    return n


def encode(data_bits):
    return np.bitwise_xor.accumulate(np.asarray(data_bits, dtype=np.uint8))


def padded(bits, lead, total=None, pad_seed=None):
    """lead one-bits, the stream, then TAIL zero data bits -- or, with
    `total`, seeded random data bits up to that length (PAD above)."""
    bits = np.asarray(bits, dtype=np.uint8)
    if total is None:
        return np.concatenate([np.ones(lead, np.uint8), bits, np.zeros(TAIL, np.uint8)])
    assert total >= lead + bits.size + TAIL
    pad = np.random.default_rng(pad_seed).integers(0, 2, total - lead - bits.size, dtype=np.uint8)
    return np.concatenate([np.ones(lead, np.uint8), bits, pad])


def n_samples(n_bits, fs):
    """len(d) fs / 1187.5 samples, cut to whole calls of 4096."""
    return (n_bits * fs * 2 // 2375) // CALL * CALL


@functools.lru_cache(maxsize=4)
def _carrier(n, fs, level):
    """level * (+1 first half-bit, -1 second) * sin(2 pi ((57000 t) mod fs) / fs), float64, and k[t]."""
    t = np.arange(n, dtype=np.int64)
    h = (t * 2375) // fs
    car = level * np.sin(2.0 * np.pi * ((57000 * t) % fs).astype(np.float64) / fs)
    car[(h & 1) == 1] *= -1.0
    return car, (h >> 1)


def mpx_from_bits(data_bits, fs, level=0.05):
    """The transmitter's RDS term alone: mpx[t] = level s sin(2 pi ((57000 t)
    mod fs) / fs) with h = (t 2375) // fs, k = h >> 1, s = (+1 if e[k] else -1)
    (-1 if h & 1 else +1), e the differentially encoded bits; float64, rounded
    once to float32."""
    e = encode(data_bits)
    n = n_samples(e.size, fs)
    car, k = _carrier(n, fs, level)
    sgn = (2.0 * e.astype(np.float64) - 1.0)[k]
    return (car * sgn).astype(np.float32)


def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & _MASK
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _MASK
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _MASK
    return x ^ (x >> 31)


def rds_off(seed_base, ch, iq_rate):
    """fmx_synth_channel's RDS bit-clock offset of channel ch, in samples."""
    s = splitmix64((seed_base + ch) & 0xFFFFFFFF)
    return splitmix64(s ^ 4) % (2 * iq_rate)


def synth_table(data_bits, seed_base, ch, iq_rate, n_bits):
    """The cyclic encoded table of one fmx.synth_host channel whose first
    transmitted bit (sample 0) is data_bits[0]: table[(k0 + j) % n_bits] =
    e[j], k0 the bit index of sample 0."""
    e = encode(data_bits)
    assert e.size <= n_bits
    k0 = ((rds_off(seed_base, ch, iq_rate) * 2375) // iq_rate) >> 1
    table = np.zeros(n_bits, np.uint8)
    table[(k0 + np.arange(e.size)) % n_bits] = e
    return table


class OracleRds:
    """The oracle's RDS stage (RDSDecoder::process) for one channel."""

    def __init__(self, oracle, fs):
        self.L = oracle.lib()
        self.G = oracle.OracleGroup
        self.tuples = oracle.groups_to_tuples
        self.p = self.L.oracle_rds_create(int(fs))

    def close(self):
        if self.p:
            self.L.oracle_rds_destroy(self.p)
            self.p = None

    __del__ = close

    def reset(self):
        self.L.oracle_rds_reset(self.p)

    def process(self, mpx):
        """-> (groups of this call [(a, b, c, d, errors)], decoded bits uint8)."""
        mpx = np.ascontiguousarray(mpx, dtype=np.float32)
        cap, bcap = 16, mpx.size // 64 + 16
        g = (self.G * cap)()
        bits = np.zeros(bcap, np.uint8)
        nb = C.c_int()
        ng = self.L.oracle_rds_process(self.p, mpx.ctypes.data, mpx.size, g, cap, bits.ctypes.data, bcap, C.byref(nb))
        assert ng <= cap and nb.value <= bcap
        return self.tuples(g, ng), bits[:nb.value]


def oracle_rds_calls(oracle, mpx, fs, sizes=None, resets=()):
    """One row through the oracle's RDS stage in calls of `sizes` (default:
    4096 over the whole row); oracle_rds_reset before every call index in
    `resets`.  -> (per-call group lists, all decoded bits)."""
    if sizes is None:
        assert mpx.size % CALL == 0
        sizes = [CALL] * (mpx.size // CALL)
    d = OracleRds(oracle, fs)
    per, bits, pos = [], [], 0
    for i, n in enumerate(sizes):
        if i in resets:
            d.reset()
        g, b = d.process(mpx[pos:pos + n])
        per.append(g)
        bits.append(b)
        pos += n
    d.close()
    return per, np.concatenate(bits) if bits else np.zeros(0, np.uint8)


def pmap(fn, items):
    """fn over items on a small thread pool (ctypes releases the GIL)."""
    with ThreadPoolExecutor(WORKERS) as ex:
        return list(ex.map(fn, items))


# ---- the 72-row stage layout: row c carries stream c % 8 behind LEADS[c // 8] ----
def stage_bits():
    """72 rows of data bits, padded (PAD above) to one common length."""
    fx = fixture()
    total = max(LEADS) + max(b.size for _, b, _ in fx) + TAIL
    return [padded(fx[c % 8][1], LEADS[c // 8], total, 1000 + c) for c in range(8 * len(LEADS))]


def stage_rows(fs):
    """[72][ncalls * 4096] float32 MPX rows of stage_bits()."""
    return np.stack([mpx_from_bits(d, fs) for d in stage_bits()])


@functools.lru_cache(maxsize=None)
def stage_oracle(oracle, fs, resets=()):
    """The oracle's per-call groups and decoded bits of every stage row:
    [(per-call groups, bits)] * 72.  resets: ((call, every/residue or None),
    ...) -- reset before `call` of the rows c with c % every == residue, or of
    every row (None)."""
    bits = stage_bits()

    def one(c):
        return oracle_rds_calls(oracle, mpx_from_bits(bits[c], fs), fs, resets=reset_calls(c, resets))

    return pmap(one, range(len(bits)))


# resets in mid-stream: rows c % 3 == 1 before call 60, every row before call
# 141.  (Not 140: reset there, row 63 re-acquires on a tie -- the oracle gives
# other groups in call 150 for three of four perturbed copies of the row;
# 141 is the nearest call at which every row is stable,
# tests/test_rds_edge_streams.py.)
STAGE_RESETS = ((60, (3, 1)), (141, None))


def _selected(c, sel):
    return sel is None or c % sel[0] == sel[1]


def reset_rows(sel, n_rows=72):
    """The rows a reset with selector `sel` ((every, residue), or None: all) hits."""
    return [c for c in range(n_rows) if _selected(c, sel)]


def reset_calls(c, resets):
    """The calls before which row c is reset, of resets ((call, selector), ...)."""
    return {call for call, sel in resets if _selected(c, sel)}


def resets_hit_synced_rows(res):
    """For each reset of STAGE_RESETS, the rows it hit in sync: a group in the
    10 calls before the reset, and a group again after it."""
    out = []
    for call, sel in STAGE_RESETS:
        out.append([c for c in reset_rows(sel)
                    if any(res[c][0][i] for i in range(call - 10, call)) and any(res[c][0][i] for i in
                                                                                  range(call, len(res[c][0])))])
    return out


# Call sequences for tests/test_gpu_rds_ring.py: a checkpointed call that is
# only barely long -- 400 MPX samples are about 285 RDS-rate samples, 360
# about 256 (checkpoints instead of ring stores from 256 on), 500 about 356 --
# and right after it a short one (300: about 213).  The short call's refill
# reads the last 256 samples of the previous call's RDS-rate row, and with a
# previous count below 256 + this call's count some of those lie where this
# call's front end has already written (consecutive fmx_rds calls share a
# slot).  The 30 long calls are there so that groups appear.
BARELY_LONG = {
    "400-300-300": [4096, 400, 300, 300, 4096, ("reset", -1)] + [4096] * 30,
    "360-300-reset-500-300": [4096, 360, 300, ("reset", 5), 500, 300] + [4096] * 30,
}


BARELY_LONG_ROWS = 12  # the first 12 stage rows: the eight streams, then four behind one one-bit


def split_steps(steps, n_rows):
    """-> (call sizes, per row the set of calls a reset precedes)."""
    sizes, resets = [], [set() for _ in range(n_rows)]
    for s in steps:
        if isinstance(s, int):
            sizes.append(s)
        else:
            for c in (range(n_rows) if s[1] < 0 else [s[1]]):
                resets[c].add(len(sizes))
    return sizes, resets


def barely_long_rows(fs=240_000):
    n = max(sum(x for x in steps if isinstance(x, int)) for steps in BARELY_LONG.values())
    return np.stack([mpx_from_bits(d, fs)[:n] for d in stage_bits()[:BARELY_LONG_ROWS]])


# ---- the full-chain layout: channel 100 + i of the synthetic plan carries stream i ----
CHAIN_CH0 = 100
CHAIN_LEAD = 131


def chain_plan(fmx, iq_rate=2_400_000, dsp_rate=240_000):
    """(synth config, bit tables [8][n_bits], blocks): one common n_bits, the
    run cut so that the table never wraps."""
    fx = fixture()
    n_bits = CHAIN_LEAD + max(b.size for _, b, _ in fx) + TAIL
    scfg = fmx.make_synth(iq_rate=iq_rate, kind=2, seed_base=0xF00D, noise_std=0.0, n_bits=n_bits)
    tables = np.stack([synth_table(padded(fx[i][1], CHAIN_LEAD, n_bits, 2000 + i), scfg.seed_base, CHAIN_CH0 + i, iq_rate,
                                   n_bits) for i in range(8)])
    nblk = int(n_bits / 1187.5 * dsp_rate / CALL)
    return scfg, tables, nblk


def chain_iq(fmx, iq_rate=2_400_000, dsp_rate=240_000):
    scfg, tables, nblk = chain_plan(fmx, iq_rate, dsp_rate)
    M = iq_rate // dsp_rate
    return fmx.synth_host(scfg, CHAIN_CH0, 8, 0, CALL * M * nblk, tables), nblk


@functools.lru_cache(maxsize=None)
def chain_oracle(fmx, oracle, iq_rate=2_400_000, dsp_rate=240_000):
    """The oracle pipeline over chain_iq(): ([channel][block] group lists,
    [channel] MPX rows, blocks)."""
    iq, nblk = chain_iq(fmx, iq_rate, dsp_rate)
    M = iq_rate // dsp_rate

    def one(i):
        p = oracle.Pipeline(oracle.make_cfg(iq_rate=iq_rate, dsp_rate=dsp_rate))
        o = [p.block(iq[i, b * 2 * CALL * M:(b + 1) * 2 * CALL * M]) for b in range(nblk)]
        return [x["groups"] for x in o], np.concatenate([x["mpx"] for x in o])

    res = pmap(one, range(8))
    return [r[0] for r in res], [r[1] for r in res], nblk


# ---- noise rows: the clean stream under gaussian noise the oracle still decides the same way ----
# seed 2 is left out: one of its perturbed copies decodes two bits (184, 185) differently
NOISE_SEEDS = (1, 3, 4, 5)
NOISE_SIGMA = 0.15


def noise_row(seed, fs=240_000):
    d = padded(fixture()[0][1], 0)
    x = mpx_from_bits(d, fs).astype(np.float64)
    x = x + np.random.default_rng(seed).normal(0.0, NOISE_SIGMA, x.size)
    return x.astype(np.float32)


def perturbed(x, seed):
    """x (1 + 1e-5 N) + 1e-6 N': about ten times the GPU-to-oracle MPX RMS."""
    rng = np.random.default_rng(seed)
    y = x.astype(np.float64) * (1.0 + 1e-5 * rng.normal(size=x.size)) + 1e-6 * rng.normal(size=x.size)
    return y.astype(np.float32)
