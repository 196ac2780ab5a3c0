"""float64 restatement of the wideband channelizer (fmx_wb_*, DESIGN.md
section 18), shared by tests/test_wb_design.py and tests/test_gpu_wideband.py:

    y_c[n] = 2 fc sum_k h[k] x[nD - k] exp(-j 2 pi f_c (s0 + nD - k) / Fs)

h = firdes_kaiser(L = D tpp, fc, 80 dB) restated after oracle/fmx_oracle.cpp
(Kaiser window by numpy's I0), fc = min(0.45 / D, 0.45) in float, x[i < 0] = 0,
s0 the index of the stream's first sample.  Every phase is reduced in integers
before it becomes an angle.  `channelize` evaluates whole streams (the sum
factored as e^{-j theta(nD)} sum_k W[k] x[nD - k], by blocks of D samples);
`direct` evaluates single outputs straight from the line above."""
import numpy as np

U8, S16 = 0, 1


def tpp_rule(D):
    return 28 if D >= 8 else (20 if D >= 4 else 12)


def cutoff(D):
    return float(min(np.float32(0.45) / np.float32(D), np.float32(0.45)))


def kaiser_taps(L, fc, As=80.0):
    """liquid_firdes_kaiser(L, fc, As, 0): sinc(2 fc t) * kaiser(beta), unnormalised."""
    beta = float(np.float32(0.1102) * (np.float32(As) - np.float32(8.7)))
    t = np.arange(L, dtype=np.float64) - (L - 1) / 2.0
    r = 2.0 * t / L
    w = np.i0(beta * np.sqrt(np.maximum(0.0, 1.0 - r * r))) / np.i0(beta)
    return np.sinc(2.0 * fc * t) * w


def gains(D, tpp):
    """2 fc h[k], k = 0 .. L-1 (the decimator's scale times its taps)."""
    fc = cutoff(D)
    return 2.0 * fc * kaiser_taps(D * tpp, fc)


def weights(D, tpp, Fs, f):
    """W[k] = 2 fc h[k] exp(+j 2 pi f k / Fs)."""
    k = np.arange(D * tpp, dtype=np.int64)
    turns = ((int(f) % Fs) * k) % Fs
    return gains(D, tpp) * np.exp(2j * np.pi * turns / Fs)


def normalise(raw, fmt):
    """Interleaved raw I/Q (uint8 or int16) -> complex128 as the channelizer scales it."""
    v = np.asarray(raw).astype(np.float64)
    v = (v - 127.5) / 127.5 if fmt == U8 else v / 32768.0
    return v[0::2] + 1j * v[1::2]


def channelize(x, D, tpp, Fs, freqs, sample0=0):
    """x: complex128 stream from the reset on (x[0] has index sample0).
    -> complex128 [len(freqs)][len(x) // D]."""
    x = np.asarray(x, dtype=np.complex128)
    N = len(x) // D
    C = len(freqs)
    Wm = np.stack([weights(D, tpp, Fs, f) for f in freqs])  # [C][L]
    xp = np.concatenate([np.zeros(tpp * D, np.complex128), x[:N * D], np.zeros(D, np.complex128)])
    B = xp.reshape(N + tpp + 1, D)  # B[m][r] = x[(m - tpp) D + r]
    acc = np.zeros((N, C), np.complex128)
    for q in range(tpp):
        # k = q D + p: p = 0 reads x[(n - q) D], p > 0 reads x[(n - q - 1) D + (D - p)]
        G = np.zeros((D, C), np.complex128)
        G[1:, :] = Wm[:, q * D + 1:(q + 1) * D][:, ::-1].T
        lo = tpp - q
        acc += B[lo - 1:lo - 1 + N] @ G
        acc += np.outer(B[lo:lo + N, 0], Wm[:, q * D])
    n = np.arange(N, dtype=np.int64)
    s = (int(sample0) % Fs + n * D) % Fs
    out = np.empty((C, N), np.complex128)
    for c, f in enumerate(freqs):
        turns = ((int(f) % Fs) * s) % Fs
        out[c] = acc[:, c] * np.exp(-2j * np.pi * turns / Fs)
    return out


# ---- the band of the end-to-end tests: four synthetic stations in one 2.4 MS/s capture ----
BAND_FS, BAND_DSP, BAND_D = 2_400_000, 240_000, 10
BAND_CH0 = 700                                       # synthetic plan's stations 700 .. 703: PI 0x12bc ..
BAND_FREQ = (-900_000, -300_000, 200_000, 700_000)   # where the stations sit in the capture
BAND_AMP = (0.30, 0.12, 0.25, 0.06)                  # relative to the synth's own 0.8
BAND_EMPTY = 450_000                                 # a fifth channel, tuned where no station is
BAND_CALLS, BAND_N = 24, 4096
BAND_HEAD = 128                                      # outputs after the reset left out of the MPX comparison


def band_capture(fmx):
    """int16 [2 * BAND_CALLS * BAND_N * BAND_D] interleaved I/Q: the stations
    (fmx.synth_host, stereo + RDS) mixed to BAND_FREQ at BAND_AMP, summed,
    x 0.9, rounded."""
    n = BAND_CALLS * BAND_N * BAND_D
    scfg = fmx.make_synth(iq_rate=BAND_FS, kind=2, n_bits=8192)
    bits, _ = fmx.synth_rds_bits(scfg, BAND_CH0, len(BAND_FREQ))
    iq = fmx.synth_host(scfg, BAND_CH0, len(BAND_FREQ), 0, n, bits)
    i = np.arange(n, dtype=np.int64)
    x = np.zeros(n, np.complex128)
    for c, (f, a) in enumerate(zip(BAND_FREQ, BAND_AMP)):
        turns = ((f % BAND_FS) * (i % BAND_FS)) % BAND_FS
        x += (a / 0.8) * normalise(iq[c], U8) * np.exp(2j * np.pi * turns / BAND_FS)
    x *= 0.9
    raw = np.empty(2 * n, np.int16)
    raw[0::2] = np.clip(np.rint(x.real * 32768.0), -32768, 32767)
    raw[1::2] = np.clip(np.rint(x.imag * 32768.0), -32768, 32767)
    return raw


def band_reference(raw):
    """The float64 channelizer's rows of the four stations and the empty channel, complex128 [5][n]."""
    return channelize(normalise(raw, S16), BAND_D, tpp_rule(BAND_D), BAND_FS, list(BAND_FREQ) + [BAND_EMPTY])


def oracle_chain(H, oracle, bb, noise=0.0, seed=0):
    """One station's baseband row (complex, BAND_CALLS * BAND_N) through the
    oracle's demod -> stereo -> afpost -> rds, BAND_N per call; noise: complex
    Gaussian noise of that RMS relative to the row's, added first.
    -> per call dicts mpx, pcm_l, pcm_r, stereo, pilot, groups."""
    bb = np.asarray(bb, dtype=np.complex128)
    if noise:
        rng = np.random.default_rng(seed)
        s = noise * np.sqrt(np.mean(np.abs(bb) ** 2) / 2.0)
        bb = bb + s * (rng.normal(size=bb.size) + 1j * rng.normal(size=bb.size))
    f = np.empty(2 * bb.size, np.float32)
    f[0::2], f[1::2] = bb.real, bb.imag
    ch = H.OracleChannel(oracle)
    out = []
    for i in range(BAND_CALLS):
        n = BAND_N
        mpx, _ = ch.demod(f[2 * n * i:2 * n * (i + 1)], n)
        l, r, st, pil = ch.stereo(mpx, n)
        pl, pr = ch.afpost(l, r, n, n)
        out.append(dict(mpx=mpx.copy(), pcm_l=pl.copy(), pcm_r=pr.copy(), stereo=st, pilot=pil,
                        groups=ch.rds_groups(mpx, n)))
    ch.close()
    return out


def direct(x, D, tpp, Fs, f, n, sample0=0):
    """Output n of one channel, term by term: mix every sample at its absolute index, then filter."""
    g = gains(D, tpp)
    k = np.arange(D * tpp, dtype=np.int64)
    i = n * D - k
    ok = i >= 0
    xi = np.where(ok, np.asarray(x, dtype=np.complex128)[np.where(ok, i, 0)], 0.0)
    turns = np.array([((int(f) % Fs) * ((int(sample0) + int(v)) % Fs)) % Fs for v in i], dtype=np.float64)
    return complex(np.sum(g * xi * np.exp(-2j * np.pi * turns / Fs)))
