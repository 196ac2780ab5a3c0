"""numpy float64 restatement of the synthetic FM band (include/fmx.h, "synthetic
FM band"), written from the definition and sharing no code with the library:

  turn(f, i) = ((f mod Fs)(i mod Fs)) mod Fs,  A(f, i) = 2 pi turn(f, i) / Fs
  Isin(a, f, ph) = (75000 a / f)(cos ph - cos(A + ph))
  Icos(a, f, ph) = (75000 a / f)(sin(A + ph) - sin ph)
  phi = A(freq_hz + f_off, i) + PHI,  (I, Q) += amplitude (cos phi, sin phi)
  noise, front end, rint, clamp.

The channel parameters (fmx_synth_channel) and the Gaussian (fmx_gauss) are
restated in float32, as the library computes them."""
import numpy as np

M64 = (1 << 64) - 1
TWO_PI = 6.283185307179586
F32 = np.float32


def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def u01(h):
    return F32((h >> 40) + 1) * F32(1.0 / 16777216.0)


def channel(kind, fs, seed_base, max_offset_hz, ch):
    """fmx_synth_channel of the content config for channel ch."""
    s = splitmix64((seed_base + ch) & 0xFFFFFFFF)
    h1, h2, h3 = splitmix64(s ^ 1), splitmix64(s ^ 2), splitmix64(s ^ 3)
    span = 2 * max_offset_hz + 1
    c = {"f_off": (h1 % span) - max_offset_hz if span > 1 else 0}
    if kind == 0:
        c.update(f_l=1000, f_r=3000, a_l=F32(0.45), a_r=F32(0.45), ph_l=F32(0), ph_r=F32(0))
    else:
        f_l = 300 + h2 % 9700
        f_r = 300 + (h2 >> 20) % 9700
        if f_r == f_l:
            f_r += 37
        c.update(f_l=f_l, f_r=f_r,
                 a_l=F32(0.5) + F32(0.4) * u01(h3), a_r=F32(0.5) + F32(0.4) * u01(h3 >> 13),
                 ph_l=F32(6.2831853) * u01(h2 >> 7), ph_r=F32(6.2831853) * u01(h3 >> 29))
    c["rds_off"] = splitmix64(s ^ 4) % (2 * fs)
    return c


def _sm_vec(x):
    x = x + np.uint64(0x9E3779B97F4A7C15)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def gauss(keys):
    """fmx_gauss over an array of uint64 keys, float32."""
    with np.errstate(over="ignore"):
        h1, h2 = _sm_vec(keys), _sm_vec(keys ^ np.uint64(0xA5A5A5A5))
    to_u = lambda h: ((h >> np.uint64(40)) + np.uint64(1)).astype(F32) * F32(1.0 / 16777216.0)  # noqa: E731
    u1, u2 = to_u(h1), to_u(h2)
    return np.sqrt(F32(-2.0) * np.log(u1), dtype=F32) * np.cos(F32(6.2831853) * u2, dtype=F32)


def _A(f, i, fs):
    turn = ((f % fs) * (i % fs)) % fs
    return TWO_PI * turn.astype(np.float64) / float(fs)


def _isin(a, f, ph, i, fs):
    return (75000.0 * a / float(f)) * (np.cos(ph) - np.cos(_A(f, i, fs) + ph))


def _icos(a, f, ph, i, fs):
    return (75000.0 * a / float(f)) * (np.sin(_A(f, i, fs) + ph) - np.sin(ph))


def band(cfg, ch0, captures, sample0, n, frontends=None, bits=None):
    """cfg: dict(wide_rate, format (0 u8, 1 int16), kind, seed_base,
    max_offset_hz, rds_level, n_bits, noise_std); captures: [[(freq_hz,
    amplitude), ...], ...]; bits: [stations][n_bits] for kind 2.  Returns the
    pre-rounding values [captures][n][2] (in LSB of the format, before rint and
    clamp) and the quantised samples."""
    fs, kind = int(cfg["wide_rate"]), int(cfg["kind"])
    i = np.int64(sample0) + np.arange(n, dtype=np.int64)
    pre = np.zeros((len(captures), n, 2))
    g = 0
    for s, stations in enumerate(captures):
        I, Q = np.zeros(n), np.zeros(n)
        for (freq_hz, amplitude) in stations:
            c = channel(kind, fs, cfg["seed_base"], cfg["max_offset_hz"], ch0 + g)
            al, ar, pl, pr = float(c["a_l"]), float(c["a_r"]), float(c["ph_l"]), float(c["ph_r"])
            fl, fr = c["f_l"], c["f_r"]
            if kind == 0:
                P = _isin(al, fl, pl, i, fs) + _isin(ar, fr, pr, i, fs)
            else:
                P = _isin(0.45 * al, fl, pl, i, fs) + _isin(0.45 * ar, fr, pr, i, fs)
                P = P + _icos(0.225 * al, fl - 38000, pl, i, fs)
                P = P - _icos(0.225 * al, fl + 38000, pl, i, fs)
                P = P - _icos(0.225 * ar, fr - 38000, pr, i, fs)
                P = P + _icos(0.225 * ar, fr + 38000, pr, i, fs)
                P = P + _isin(0.09, 19000, 0.0, i, fs)
                if kind == 2:
                    nr = i + np.int64(c["rds_off"])
                    h = (2375 * nr) // fs
                    bit = bits[g][(h >> 1) % cfg["n_bits"]]
                    sgn = np.where(bit != 0, 1.0, -1.0) * np.where((h & 1) != 0, -1.0, 1.0)
                    P = P + sgn * (75000.0 * float(F32(cfg["rds_level"])) / 57000.0) * (1.0 - np.cos(_A(57000, nr, fs)))
            phi = _A(freq_hz + c["f_off"], i, fs) + P
            a = float(F32(amplitude))
            I = I + a * np.cos(phi)
            Q = Q + a * np.sin(phi)
            g += 1
        ns = float(F32(cfg["noise_std"]))
        if ns > 0:
            base = splitmix64(((cfg["seed_base"] << 32) ^ s ^ 0xBA4D) & M64)
            with np.errstate(over="ignore"):
                keys = np.uint64(base) + np.uint64(2) * i.astype(np.uint64)
                I = I + ns * gauss(keys).astype(np.float64)
                Q = Q + ns * gauss(keys + np.uint64(1)).astype(np.float64)
        dc_i, dc_q, q_gain, q_cross = (0.0, 0.0, 1.0, 0.0) if frontends is None else frontends[s]
        I2 = I + dc_i
        Q2 = q_gain * Q + q_cross * I + dc_q
        if cfg["format"] == 1:
            pre[s, :, 0], pre[s, :, 1] = 32768.0 * I2, 32768.0 * Q2
        else:
            pre[s, :, 0], pre[s, :, 1] = 127.5 * I2 + 127.5, 127.5 * Q2 + 127.5
    if cfg["format"] == 1:
        q = np.clip(np.rint(pre), -32768, 32767).astype(np.int16)
    else:
        q = np.clip(np.rint(pre), 0, 255).astype(np.uint8)
    return pre, q
