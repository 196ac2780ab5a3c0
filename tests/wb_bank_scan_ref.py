"""float64 restatement of the band scan over a capture bank
(fmx_wb_bank_scan_*), shared by
tests/test_wb_bank_scan.py and tests/test_gpu_wb_bank_scan.py.  It holds
nothing new: per capture, wb_scan_ref.scan_call on that capture's row and
frequencies, concatenated."""
import wb_scan_ref as S


def first_point(freqs_per_capture):
    first = [0]
    for f in freqs_per_capture:
        first.append(first[-1] + len(f))
    return first


def groups(first):
    """The work list fmx_wb_bank_scan_groups returns: (capture, first point,
    points 1..64) per 64 points of a capture, none for an empty capture."""
    out = []
    for s in range(len(first) - 1):
        for p in range(first[s], first[s + 1], 64):
            out.append((s, p, min(64, first[s + 1] - p)))
    return out


def scan_call(rows, fmt, D, tpp, Fs, freqs_per_capture, n_out, params=None):
    """The records of one call, one dict per point of every capture in order.
    rows[s]: capture s's interleaved raw samples (at least n_out * D);
    params[s]: capture s's signal parameters (None: the defaults)."""
    out = []
    for s, freqs in enumerate(freqs_per_capture):
        if not len(freqs):
            continue
        p = S.DEFAULT_PARAMS if params is None or params[s] is None else params[s]
        out += S.scan_call(rows[s], fmt, D, tpp, Fs, list(freqs), n_out, p)
    return out
