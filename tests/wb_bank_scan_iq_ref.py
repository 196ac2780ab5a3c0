"""float64 restatement of the per-capture DC / IQ-imbalance correction of the
band scan over a capture bank (fmx_wb_bank_scan_set_iq_correction, DESIGN.md
section 29), shared by tests/test_wb_bank_scan_iqcorr.py and
tests/test_gpu_wb_bank_scan_iqcorr.py.  It holds nothing new: per capture,
wb_iq_ref.scan_call and wb_iq_ref.estimate on that capture's row, concatenated
as wb_bank_scan_ref.scan_call concatenates; and wb_iq_ref.impaired_capture
with its constants as parameters, because the captures of a bank need
different front ends."""
import functools

import numpy as np

import wb_iq_ref as Q
import wb_ref as R
import wb_scan_ref as S


def scan_call(rows, fmt, D, tpp, Fs, freqs_per_capture, n_out, ps, params=None):
    """The records of one read, one dict per point of every capture in order.
    rows[s]: capture s's interleaved raw samples (at least n_out * D); ps[s]:
    the correction (dc_i, dc_q, gain, cross) of capture s in this read
    (wb_iq_ref.IDENTITY for a capture in OFF); params[s]: its signal
    parameters (None: the defaults)."""
    out = []
    for s, freqs in enumerate(freqs_per_capture):
        if not len(freqs):
            continue
        sp = S.DEFAULT_PARAMS if params is None or params[s] is None else params[s]
        out += Q.scan_call(rows[s], fmt, D, tpp, Fs, list(freqs), n_out, ps[s], sp)
    return out


def estimates(rows, fmt, D, n_out, states, alphas):
    """wb_iq_ref.estimate per capture over its own n_out * D samples of the
    read.  states[s]: capture s's smoothed moments (None: the first read since
    its set); alphas[s]: its smoothing.  -> ([p per capture], [state per
    capture])."""
    ps, out = [], []
    for s, row in enumerate(rows):
        p, st = Q.estimate(np.asarray(row)[:2 * n_out * D], fmt, states[s], alphas[s])
        ps.append(p)
        out.append(st)
    return ps, out


@functools.lru_cache(maxsize=None)
def impaired(fmt, seed, stations, q_gain, skew_deg, dc, n=Q.CAP_N, fs=Q.CAP_FS):
    """wb_iq_ref.impaired_capture with its constants as arguments: n samples
    at fs, interleaved raw I/Q (read-only).  stations: ((amplitude, Hz, tone
    Hz), ...), FM at 75 kHz deviation, plus white noise of 0.003 per component
    from default_rng(seed); the Q path has gain q_gain and skew_deg degrees of
    skew, DC is dc = (I, Q); rounded and clipped to the format."""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64) / fs
    s = np.zeros(n, np.complex128)
    for amp, hz, tone in stations:
        ph = 2.0 * np.pi * hz * t + (Q.CAP_DEV_HZ / tone) * np.sin(2.0 * np.pi * tone * t)
        s = s + amp * np.exp(1j * ph)
    s = s + Q.CAP_NOISE * (rng.normal(size=n) + 1j * rng.normal(size=n))
    return front_end(s, fmt, q_gain, skew_deg, dc)


def front_end(s, fmt, q_gain, skew_deg, dc):
    """Complex samples through a zero-IF front end with a Q path of its own ->
    interleaved raw I/Q (read-only)."""
    sk = np.radians(skew_deg)
    i = s.real + dc[0]
    q = q_gain * (s.imag * np.cos(sk) + s.real * np.sin(sk)) + dc[1]
    if fmt == R.U8:
        raw = np.empty(2 * len(s), np.uint8)
        quant = lambda v: np.clip(np.rint(v * 127.5 + 127.5), 0, 255)  # noqa: E731
    else:
        raw = np.empty(2 * len(s), np.int16)
        quant = lambda v: np.clip(np.rint(v * 32768.0), -32768, 32767)  # noqa: E731
    raw[0::2], raw[1::2] = quant(i), quant(q)
    raw.setflags(write=False)
    return raw


# The three front ends of the ghost tests: capture 0 is wb_iq_ref's own example
FRONT_ENDS = (
    dict(seed=Q.CAP_SEED, stations=((Q.CAP_AMP, Q.CAP_STATION_HZ, Q.CAP_TONE_HZ),), q_gain=Q.CAP_Q_GAIN,
         skew_deg=Q.CAP_SKEW_DEG, dc=Q.CAP_DC),
    dict(seed=25, stations=((0.4, -500_000, 700),), q_gain=0.95, skew_deg=-3.0, dc=(-0.012, 0.025)),
    dict(seed=26, stations=((0.35, 200_000, 1300), (0.2, 500_000, 900)), q_gain=1.08, skew_deg=-5.0, dc=(0.030, 0.010)),
)
GHOST_START, GHOST_STEP, GHOST_POINTS = -600_000, 100_000, 13
GHOST_N_OUT, GHOST_D, GHOST_TPP = 2048, 10, 28
GHOST_THRESHOLD_DBFS, GHOST_SPACING = -45.0, 1
STATIONS = ([300_000], [-500_000], [200_000, 500_000])
GHOSTS = ([-300_000, 0, 300_000], [-500_000, 0, 500_000], [-500_000, 200_000, 500_000])  # uncorrected peaks


def ghost_rows(fmt):
    """The three impaired captures; capture 0 is impaired_capture(fmt) itself."""
    return [Q.impaired_capture(fmt)] + [impaired(fmt, **FRONT_ENDS[s]) for s in (1, 2)]
