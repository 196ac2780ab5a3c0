"""float64 restatement of the rational-rate channelizer (fmx_wb_create_rational,
DESIGN.md section 23), shared by tests/test_wb_rational.py and
tests/test_gpu_wb_rational.py.  With wide_rate / dsp_rate = P / Q in lowest
terms, Lup = P tpp, h = firdes_kaiser(Lup, fc, 80 dB) (tests/wb_ref.py's
restatement), fc = min(0.45 / P, 0.45) in float and G = Q 2 fc:

    y_c[n] = G sum_i h[nP - iQ] x[i] exp(-j 2 pi f_c (s0 + i) / Fs),  0 <= nP - iQ < Lup, x[i < 0] = 0

`direct` evaluates single outputs straight from that line; `channelize`
evaluates whole streams in the factored form: for n = Q m + r with
r P = Q a_r + b_r and i0 = m P + a_r,

    y_c[n] = e^{-j theta(i0)} sum_j W_r[j] x[i0 - j],  W_r[j] = G h[Q j + b_r] e^{+j 2 pi f_c j / Fs}

Every phase is reduced in integers before it becomes an angle."""
import math

import numpy as np

import wb_ref as R


def ratio(wide_rate, dsp_rate):
    g = math.gcd(wide_rate, dsp_rate)
    return wide_rate // g, dsp_rate // g


def tpp_rule(P, Q):
    return 28 if P >= 8 * Q else (20 if P >= 4 * Q else 12)


def gains(P, Q, tpp):
    """G h[k], k = 0 .. Lup-1, at the up-sampled rate Q Fs."""
    fc = R.cutoff(P)
    return Q * 2.0 * fc * R.kaiser_taps(P * tpp, fc)


def phases(P, Q, tpp):
    """[(a_r, b_r, L_r)] for r = 0 .. Q-1."""
    Lup = P * tpp
    return [(r * P // Q, r * P % Q, -((-(Lup - r * P % Q)) // Q)) for r in range(Q)]


def weights(P, Q, tpp, Fs, f, r):
    """W_r[j], j = 0 .. L_r-1."""
    _, b, L = phases(P, Q, tpp)[r]
    j = np.arange(L, dtype=np.int64)
    turns = ((int(f) % Fs) * j) % Fs
    return gains(P, Q, tpp)[Q * j + b] * np.exp(2j * np.pi * turns / Fs)


def direct(x, P, Q, tpp, Fs, f, n, sample0=0):
    """Output n of one channel, term by term from the defining sum."""
    g = gains(P, Q, tpp)
    x = np.asarray(x, dtype=np.complex128)
    acc = 0.0 + 0.0j
    i = (n * P) // Q
    while i >= 0 and n * P - i * Q < P * tpp:
        if i < len(x):
            turns = ((int(f) % Fs) * ((int(sample0) + i) % Fs)) % Fs
            acc += g[n * P - i * Q] * x[i] * np.exp(-2j * np.pi * turns / Fs)
        i -= 1
    return complex(acc)


def channelize(x, P, Q, tpp, Fs, freqs, sample0=0):
    """x: complex128 stream from the reset on (x[0] has index sample0).
    -> complex128 [len(freqs)][(len(x) // P) * Q]."""
    x = np.asarray(x, dtype=np.complex128)
    M = len(x) // P
    C = len(freqs)
    ph = phases(P, Q, tpp)
    Lmax = max(L for _, _, L in ph)
    xp = np.concatenate([np.zeros(Lmax - 1, np.complex128), x[:M * P]])
    out = np.empty((C, M * Q), np.complex128)
    step = xp.strides[0]
    for r, (a, _, L) in enumerate(ph):
        # row m: x[i0 - (L - 1)] .. x[i0], i0 = m P + a; the taps reversed to match
        Wm = np.stack([weights(P, Q, tpp, Fs, f, r)[::-1] for f in freqs])  # [C][L]
        first = (Lmax - 1) + a - (L - 1)
        acc = np.empty((M, C), np.complex128)
        for m0 in range(0, M, 2048):
            m1 = min(M, m0 + 2048)
            win = np.lib.stride_tricks.as_strided(xp[first + m0 * P:], shape=(m1 - m0, L), strides=(P * step, step),
                                                  writeable=False)
            acc[m0:m1] = win @ Wm.T
        s = (int(sample0) % Fs + np.arange(M, dtype=np.int64) * P + a) % Fs
        for c, f in enumerate(freqs):
            turns = ((int(f) % Fs) * s) % Fs
            out[c, r::Q] = acc[:, c] * np.exp(-2j * np.pi * turns / Fs)
    return out
