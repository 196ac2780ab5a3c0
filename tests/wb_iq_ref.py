"""float64 / int64 restatement of the DC-offset and IQ-imbalance correction of
wide captures (fmx_wb_set_iq_correction, fmx_iq_estimate; include/fmx.h,
DESIGN.md section 24), on top of tests/wb_ref.py and tests/wb_scan_ref.py:

    x' = (I - dc_i) + j (gain (Q - dc_q) + cross (I - dc_i))

with the parameters p = (dc_i, dc_q, gain, cross) in units of x.  Every output
of a call is the channelizer's formula on x' with the call's own parameters
over its whole window; before the stream's start x = 0 and x' = C(0).

`estimate` is the estimator (exact int64 sums of the raw values, then a dozen
double operations), `correct` the correction, `rows` a stream of calls, each
evaluated with its own parameters, `scan_call` one read of the band scan,
`impaired_capture` the example the tests measure image rejection on."""
import functools

import numpy as np

import wb_ref as R
import wb_scan_ref as S

IDENTITY = (0.0, 0.0, 1.0, 0.0)

# impaired_capture: an FM station through a front end with DC and a Q path of its own
CAP_FS, CAP_N, CAP_SEED = 2_400_000, 96_000, 24
CAP_STATION_HZ, CAP_AMP, CAP_DEV_HZ, CAP_TONE_HZ = 300_000, 0.5, 75_000, 1_000
CAP_NOISE = 0.003                       # per component
CAP_Q_GAIN, CAP_SKEW_DEG = 1.06, 4.0
CAP_DC = (0.020, -0.015)
# the inverse of that front end
CAP_TRUE = (CAP_DC[0], CAP_DC[1], 1.0 / (CAP_Q_GAIN * np.cos(np.radians(CAP_SKEW_DEG))),
            -np.tan(np.radians(CAP_SKEW_DEG)))


def unit(fmt):
    """Raw units per unit of x."""
    return 255.0 if fmt == R.U8 else 32768.0


def raw_values(raw, fmt):
    """v = 2 b - 255 for u8, v for int16, as int64 (I, Q)."""
    v = np.asarray(raw).astype(np.int64)
    if fmt == R.U8:
        v = 2 * v - 255
    return v[0::2], v[1::2]


def estimate(raw, fmt, state=None, alpha=1.0):
    """The estimator over one call's raw samples.  state: the five smoothed raw
    moments (E I, E Q, E I^2, E Q^2, E IQ) of the calls before, None for the
    first call after the mode was set.  -> (p, state)."""
    i, q = raw_values(raw, fmt)
    n = len(i)
    sums = [int(np.sum(i)), int(np.sum(q)), int(np.sum(i * i)), int(np.sum(q * q)), int(np.sum(i * q))]
    call = [float(s) / float(n) for s in sums]
    m = call if state is None else [a + alpha * (c - a) for a, c in zip(state, call)]
    mI, mQ = m[0], m[1]
    cII, cQQ, cIQ = m[2] - mI * mI, m[3] - mQ * mQ, m[4] - mI * mQ
    gain, cross = 1.0, 0.0
    if cII > 0.0:
        v = cQQ - cIQ * cIQ / cII
        if v > 1e-9 * cQQ:
            gain = float(np.sqrt(cII / v))
            cross = -gain * cIQ / cII
    u = unit(fmt)
    return (mI / u, mQ / u, gain, cross), m


def correct(x, p):
    x = np.asarray(x, dtype=np.complex128)
    dc_i, dc_q, gain, cross = p
    i = x.real - dc_i
    return i + 1j * (gain * (x.imag - dc_q) + cross * i)


def rows(raw_calls, fmt, D, tpp, Fs, freqs, params, sample0=0):
    """raw_calls: the stream from the reset on, cut into calls (interleaved
    raw I/Q, a whole number of outputs each); params: one p per call.  Each
    call's outputs come from the whole stream so far, L zeros ahead of it
    (x = 0 before the stream's start), corrected with the call's own
    parameters.  -> complex128 [len(freqs)][outputs of all calls]."""
    L = D * tpp
    out, sofar = [], np.zeros(0, np.complex128)
    for raw, p in zip(raw_calls, params):
        x = R.normalise(raw, fmt)
        n = len(x) // D
        sofar = np.concatenate([sofar, x])
        xx = correct(np.concatenate([np.zeros(L, np.complex128), sofar]), p)
        y = R.channelize(xx, D, tpp, Fs, freqs, sample0=sample0 - L)
        out.append(y[:, y.shape[1] - n:])
    return np.concatenate(out, axis=1)


def scan_call(raw, fmt, D, tpp, Fs, freqs, n_out, p, params=S.DEFAULT_PARAMS):
    """wb_scan_ref.scan_call on the corrected samples; the clip ratios stay the raw samples'."""
    raw = np.asarray(raw)[:2 * n_out * D]
    hard, near = S.clip_ratios(raw, fmt)
    y = R.channelize(correct(R.normalise(raw, fmt), p), D, tpp, Fs, freqs)[:, tpp:n_out]
    out = []
    for pw in np.mean(np.abs(y) ** 2, axis=1):
        r = S.record(pw, params)
        r.update(hard_clip_ratio=hard, near_clip_ratio=near)
        out.append(r)
    return out


@functools.lru_cache(maxsize=None)
def impaired_capture(fmt):
    """96 000 samples at 2.4 MS/s, interleaved raw I/Q (read-only): an FM
    station of amplitude 0.5 at +300 kHz (75 kHz deviation, 1 kHz tone) plus
    white noise of 0.003 per component; the Q path has gain 1.06 and 4 degrees
    of skew, DC is +0.020 on I and -0.015 on Q; rounded and clipped to the
    format.  CAP_TRUE undoes the front end."""
    rng = np.random.default_rng(CAP_SEED)
    t = np.arange(CAP_N, dtype=np.float64) / CAP_FS
    ph = 2.0 * np.pi * CAP_STATION_HZ * t + (CAP_DEV_HZ / CAP_TONE_HZ) * np.sin(2.0 * np.pi * CAP_TONE_HZ * t)
    s = CAP_AMP * np.exp(1j * ph) + CAP_NOISE * (rng.normal(size=CAP_N) + 1j * rng.normal(size=CAP_N))
    sk = np.radians(CAP_SKEW_DEG)
    i = s.real + CAP_DC[0]
    q = CAP_Q_GAIN * (s.imag * np.cos(sk) + s.real * np.sin(sk)) + CAP_DC[1]
    if fmt == R.U8:
        raw = np.empty(2 * CAP_N, np.uint8)
        quant = lambda v: np.clip(np.rint(v * 127.5 + 127.5), 0, 255)  # noqa: E731
    else:
        raw = np.empty(2 * CAP_N, np.int16)
        quant = lambda v: np.clip(np.rint(v * 32768.0), -32768, 32767)  # noqa: E731
    raw[0::2], raw[1::2] = quant(i), quant(q)
    raw.setflags(write=False)
    return raw


def image_ratio_db(y):
    """y: rows of the channels at (+300 kHz, -300 kHz) -> mean |y|^2 of the second over the first, dB."""
    return float(10.0 * np.log10(np.mean(np.abs(y[1]) ** 2) / np.mean(np.abs(y[0]) ** 2)))
