"""float64 restatement of the band scan (fmx_wb_scan_*),
shared by tests/test_wb_scan.py and tests/test_gpu_wb_scan.py.  One call is
one read of every point:

    P_p  = mean_{n = tpp .. n_out - 1} |y_p[n]|^2,  y = wb_ref.channelize of the call's samples
    rms  = sqrt(max(1e-15, 0.5 P_p)),  dbfs = 20 log10(rms + 1e-12)

and compensated_dbfs / level120 as computeSignalLevel (signal_level.cpp:187-195;
level120 through one float conversion), the clip ratios from integer counts
of the call's raw samples, the smoother oracle.SignalSmoother."""
import numpy as np

import wb_ref as R

DEFAULT_PARAMS = (0, 0.5, -4.0, -55.0, -19.0)  # gain dB, factor, bias, floor, ceil


def points(start_hz, step_hz, n_points):
    return [start_hz + p * step_hz for p in range(n_points)]


def record(power, params=DEFAULT_PARAMS):
    """The level fields of one point from P = mean |y|^2."""
    gain_db, comp, bias, floor_db, ceil_db = params
    rms = np.sqrt(max(1e-15, 0.5 * float(power)))
    dbfs = 20.0 * np.log10(rms + 1e-12)
    comp_db = dbfs - (float(gain_db) * comp) + bias
    safe_ceil = max(ceil_db, floor_db + 1.0)
    norm = (comp_db - floor_db) / (safe_ceil - floor_db)
    level = float(np.clip(np.float32(norm * 120.0), np.float32(0.0), np.float32(120.0)))
    return dict(level120=level, dbfs=float(dbfs), compensated_dbfs=float(comp_db))


def clip_ratios(raw, fmt):
    """(hard, near): clipped samples / samples of interleaved raw I/Q; u8 by
    the reference's byte thresholds, int16 by its top byte b = (v >> 8) + 128."""
    raw = np.asarray(raw)
    b = raw.astype(np.int64) if fmt == R.U8 else (raw.astype(np.int64) >> 8) + 128
    i, q = b[0::2], b[1::2]
    n = len(i)
    hard = int(np.count_nonzero((i <= 1) | (i >= 254) | (q <= 1) | (q >= 254)))
    near = int(np.count_nonzero((i <= 8) | (i >= 247) | (q <= 8) | (q >= 247)))
    return hard / float(n), near / float(n)


def powers(raw, fmt, D, tpp, Fs, freqs, n_out):
    """P_p of one call: raw holds (at least) the call's n_out * D samples, interleaved."""
    x = R.normalise(np.asarray(raw)[:2 * n_out * D], fmt)
    y = R.channelize(x, D, tpp, Fs, freqs)[:, tpp:n_out]
    return np.mean(np.abs(y) ** 2, axis=1)


def scan_call(raw, fmt, D, tpp, Fs, freqs, n_out, params=DEFAULT_PARAMS):
    """The records of one call (without the smoothed level), one dict per point."""
    hard, near = clip_ratios(np.asarray(raw)[:2 * n_out * D], fmt)
    out = []
    for pw in powers(raw, fmt, D, tpp, Fs, freqs, n_out):
        r = record(pw, params)
        r.update(hard_clip_ratio=hard, near_clip_ratio=near)
        out.append(r)
    return out


def rms_of(dbfs):
    """The rms a record's dbfs was formed from."""
    return 10.0 ** (np.asarray(dbfs, dtype=np.float64) / 20.0) - 1e-12
