"""fmx -- Python (ctypes) binding of libfmx.so, the MI355X many-channel FM
demodulator.  Mirrors include/fmx.h one to one; device buffers are plain
integer addresses (e.g. ``torch.Tensor.data_ptr()`` of a CUDA/HIP tensor).

The binding never falls back to a CPU path: if libfmx.so is missing or no GPU
is present, the calls raise.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FMX_LIB") or os.path.join(_HERE, "libfmx.so")  # FMX_LIB: A/B builds (diagnostic)

FMX_OK = 0
FMX_AGC_OFF, FMX_AGC_FAST, FMX_AGC_SLOW = 0, 1, 2
FMX_BLEND_SOFT, FMX_BLEND_NORMAL, FMX_BLEND_AGGRESSIVE = 0, 1, 2
FMX_DEEMPH_50US, FMX_DEEMPH_75US, FMX_DEEMPH_OFF = 0, 1, 2
PARAM = dict(bandwidth_hz=1, w0_hz=2, deemphasis=3, dsp_agc=4, blend=5,
             force_mono=6, force_stereo=7, bandwidth_mode=8, deemph_us=9, deviation_hz=10)
K_FRONTEND, K_STEREO, K_AUDIO, K_RDS, K_RS, K_PILOT, K_FRONTEND_GENERIC, K_BITS = 0, 1, 2, 3, 4, 5, 6, 7
KERNEL_NAMES = ["frontend", "stereo", "audio", "rds", "rs", "pilot", "frontend_generic", "bits"]
FMX_DIAG_RDS_RING_ALWAYS, FMX_DIAG_FE_GENERIC = 1, 2


class Config(C.Structure):
    _fields_ = [(n, C.c_int) for n in (
        "iq_rate", "dsp_rate", "out_rate", "block", "w0_bandwidth_hz",
        "bandwidth_hz", "dsp_agc", "stereo", "blend", "deemphasis",
        "force_mono", "force_stereo", "rds")]


class RdsGroup(C.Structure):
    _fields_ = [("a", C.c_uint16), ("b", C.c_uint16), ("c", C.c_uint16),
                ("d", C.c_uint16), ("errors", C.c_uint8), ("pad", C.c_uint8),
                ("block_index", C.c_uint32)]


class SignalLevel(C.Structure):
    _fields_ = [("level120", C.c_float), ("level120_smoothed", C.c_float), ("dbfs", C.c_double),
                ("compensated_dbfs", C.c_double), ("hard_clip_ratio", C.c_double),
                ("near_clip_ratio", C.c_double)]


class BlockOut(C.Structure):
    _fields_ = [("d_mpx", C.c_void_p), ("mpx_stride", C.c_int),
                ("d_pcm_l", C.c_void_p), ("d_pcm_r", C.c_void_p),
                ("pcm_stride", C.c_int), ("d_pcm_count", C.c_void_p),
                ("d_stereo", C.c_void_p), ("d_pilot_tenths", C.c_void_p),
                ("d_clip_ratio", C.c_void_p), ("d_groups", C.c_void_p),
                ("groups_stride", C.c_int), ("d_group_count", C.c_void_p),
                ("d_signal", C.c_void_p), ("d_stereo_indicator", C.c_void_p)]


class XdrPiState(C.Structure):
    _fields_ = [("pi_buf", C.c_uint16 * 64), ("pi_err", C.c_uint8 * 8), ("fill", C.c_uint8),
                ("pos", C.c_uint8), ("last_state", C.c_uint8), ("pad", C.c_uint8),
                ("last_value", C.c_uint16), ("pad2", C.c_uint16)]


class SynthConfig(C.Structure):
    _fields_ = [("iq_rate", C.c_int), ("kind", C.c_int), ("amplitude", C.c_float),
                ("noise_std", C.c_float), ("seed_base", C.c_uint32),
                ("max_offset_hz", C.c_int), ("rds_level", C.c_float),
                ("n_bits", C.c_int), ("level_spread_db", C.c_float)]


FMX_WB_U8, FMX_WB_S16 = 0, 1


class SynthBandConfig(C.Structure):
    _fields_ = [("wide_rate", C.c_int), ("format", C.c_int), ("kind", C.c_int), ("seed_base", C.c_uint32),
                ("max_offset_hz", C.c_int), ("rds_level", C.c_float), ("n_bits", C.c_int), ("noise_std", C.c_float)]


class SynthStation(C.Structure):
    _fields_ = [("freq_hz", C.c_int), ("amplitude", C.c_float)]


class SynthFrontend(C.Structure):
    """fmx_synth_frontend: I' = I + dc_i, Q' = q_gain Q + q_cross I + dc_q."""
    _fields_ = [(n, C.c_double) for n in ("dc_i", "dc_q", "q_gain", "q_cross")]


class WbConfig(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("wide_rate", "dsp_rate", "format", "taps_per_phase", "block")]


class WbScanConfig(C.Structure):
    _fields_ = [("wb", WbConfig), ("start_hz", C.c_int), ("step_hz", C.c_int), ("n_points", C.c_int)]


FMX_IQC_OFF, FMX_IQC_FIXED, FMX_IQC_AUTO = 0, 1, 2


class IqCorrection(C.Structure):
    """fmx_iq_correction: x' = (I - dc_i) + j (gain (Q - dc_q) + cross (I - dc_i)), units of x."""
    _fields_ = [(n, C.c_double) for n in ("dc_i", "dc_q", "gain", "cross")]

    def astuple(self):
        return (self.dc_i, self.dc_q, self.gain, self.cross)


_lib = None
_OPTIONAL = {"fmx_build_info", "fmx_host_stats", "fmx_diag_set", "fmx_diag_rds_ring"}  # absent from older libraries (A/B against past revisions)


def lib():
    """Load libfmx.so (raises OSError when the HIP extension is missing)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise OSError(f"libfmx.so not built: {LIB_PATH} (run __graft_entry__.build())")
    L = C.CDLL(LIB_PATH)
    vp, i, sz, fp = C.c_void_p, C.c_int, C.c_size_t, C.POINTER(C.c_float)
    sig = {
        "fmx_build_info": (C.c_char_p, []),
        "fmx_device_count": (i, []),
        "fmx_create": (i, [C.POINTER(Config), i, i, C.POINTER(vp)]),
        "fmx_destroy": (i, [vp]),
        "fmx_last_error": (C.c_char_p, [vp]),
        "fmx_sync": (i, [vp]),
        "fmx_num_channels": (i, [vp]),
        "fmx_reset": (i, [vp, i]),
        "fmx_retune": (i, [vp, i, i]),
        "fmx_set_param": (i, [vp, i, i, i]),
        "fmx_set_signal_params": (i, [vp, i, i, C.c_double, C.c_double, C.c_double, C.c_double]),
        "fmx_process_block": (i, [vp, vp, sz, i, C.POINTER(BlockOut)]),
        "fmx_decimate": (i, [vp, vp, sz, i, vp, i]),
        "fmx_decimate_u8": (i, [vp, vp, sz, i, vp, sz]),
        "fmx_demod": (i, [vp, vp, i, i, vp, i, vp, i, vp]),
        "fmx_demod_u8": (i, [vp, vp, sz, i, vp, i, vp, i, vp, vp]),
        "fmx_downsample": (i, [vp, vp, i, i, vp, i, vp]),
        "fmx_stereo": (i, [vp, vp, i, i, vp, vp, i, vp, vp]),
        "fmx_afpost": (i, [vp, vp, vp, i, i, vp, vp, i, i, vp]),
        "fmx_rds": (i, [vp, vp, i, i, vp, i, vp]),
        "fmx_wb_create": (i, [vp, C.POINTER(WbConfig), C.POINTER(i), i, C.POINTER(vp)]),
        "fmx_wb_create_rational": (i, [vp, C.POINTER(WbConfig), C.POINTER(i), i, C.POINTER(vp)]),
        "fmx_wb_ratio": (i, [C.POINTER(WbConfig), C.POINTER(i), C.POINTER(i), C.POINTER(i)]),
        "fmx_wb_weights_rational": (i, [C.POINTER(WbConfig), i, i, fp, i]),
        "fmx_wb_rational_geometry": (i, [C.POINTER(WbConfig), i, C.POINTER(i), i]),
        "fmx_wb_destroy": (i, [vp]),
        "fmx_wb_set_freq": (i, [vp, i, i]),
        "fmx_wb_reset": (i, [vp, C.c_int64]),
        "fmx_wb_process": (i, [vp, vp, i, vp, i]),
        "fmx_wb_process_block": (i, [vp, vp, i, C.POINTER(BlockOut)]),
        "fmx_wb_signal": (i, [vp, vp]),
        "fmx_wb_set_signal_params": (i, [vp, i, C.c_double, C.c_double, C.c_double, C.c_double]),
        "fmx_wb_signal_reset": (i, [vp, i]),
        "fmx_diag_lds_bytes": (i, [i]),
        "fmx_wb_bank_create": (i, [vp, C.POINTER(WbConfig), i, C.POINTER(i), C.POINTER(i), C.POINTER(vp)]),
        "fmx_wb_bank_create_rational": (i, [vp, C.POINTER(WbConfig), i, C.POINTER(i), C.POINTER(i), C.POINTER(vp)]),
        "fmx_wb_bank_destroy": (i, [vp]),
        "fmx_wb_bank_set_freq": (i, [vp, i, i]),
        "fmx_wb_bank_reset": (i, [vp, i, C.c_int64]),
        "fmx_wb_bank_process": (i, [vp, vp, C.c_size_t, i, vp, i]),
        "fmx_wb_bank_process_block": (i, [vp, vp, C.c_size_t, i, C.POINTER(BlockOut)]),
        "fmx_wb_bank_signal": (i, [vp, vp]),
        "fmx_wb_bank_set_signal_params": (i, [vp, i, i, C.c_double, C.c_double, C.c_double, C.c_double]),
        "fmx_wb_bank_signal_reset": (i, [vp, i]),
        "fmx_wb_bank_groups": (i, [C.POINTER(i), i, C.POINTER(i), i]),
        "fmx_wb_weights": (i,[C.POINTER(WbConfig), i, fp, i]),
        "fmx_wb_scan_create": (i, [vp, C.POINTER(WbScanConfig), C.POINTER(vp)]),
        "fmx_wb_scan_destroy": (i, [vp]),
        "fmx_wb_scan_set_signal_params": (i, [vp, i, C.c_double, C.c_double, C.c_double, C.c_double]),
        "fmx_wb_scan_reset": (i, [vp]),
        "fmx_wb_scan_process": (i, [vp, vp, i, vp]),
        "fmx_wb_scan_points": (i, [C.POINTER(WbScanConfig), C.POINTER(i), i]),
        "fmx_scan_peaks": (i, [C.POINTER(C.c_double), i, C.c_double, i, C.POINTER(i), i]),
        "fmx_wb_bank_scan_create": (i, [vp, C.POINTER(WbConfig), i, C.POINTER(i), C.POINTER(i), C.POINTER(vp)]),
        "fmx_wb_bank_scan_destroy": (i, [vp]),
        "fmx_wb_bank_scan_set_signal_params": (i, [vp, i, i, C.c_double, C.c_double, C.c_double, C.c_double]),
        "fmx_wb_bank_scan_reset": (i, [vp, i]),
        "fmx_wb_bank_scan_process": (i, [vp, vp, C.c_size_t, i, vp]),
        "fmx_wb_bank_scan_groups": (i, [C.POINTER(i), i, C.POINTER(i), i]),
        "fmx_wb_set_iq_correction": (i, [vp, i, C.POINTER(IqCorrection), C.c_double]),
        "fmx_wb_iq_correction": (i, [vp, C.POINTER(IqCorrection)]),
        "fmx_wb_scan_set_iq_correction": (i, [vp, i, C.POINTER(IqCorrection), C.c_double]),
        "fmx_wb_scan_iq_correction": (i, [vp, C.POINTER(IqCorrection)]),
        "fmx_wb_bank_set_iq_correction": (i, [vp, i, i, C.POINTER(IqCorrection), C.c_double]),
        "fmx_wb_bank_iq_correction": (i, [vp, i, C.POINTER(IqCorrection)]),
        "fmx_wb_bank_scan_set_iq_correction": (i, [vp, i, i, C.POINTER(IqCorrection), C.c_double]),
        "fmx_wb_bank_scan_iq_correction": (i, [vp, i, C.POINTER(IqCorrection)]),
        "fmx_iq_estimate": (i, [vp, i, C.c_long, C.POINTER(IqCorrection)]),
        "fmx_malloc": (i, [vp, C.POINTER(vp), sz]),
        "fmx_free": (i, [vp, vp]),
        "fmx_memcpy_h2d": (i, [vp, vp, vp, sz]),
        "fmx_memcpy_d2h": (i, [vp, vp, vp, sz]),
        "fmx_memset": (i, [vp, vp, i, sz]),
        "fmx_timing_enable": (i, [vp, i]),
        "fmx_kernel_times": (i, [vp, C.POINTER(C.c_double), C.POINTER(i), i]),
        "fmx_host_stats": (i, [vp, C.POINTER(C.c_double), i]),
        "fmx_diag_set": (i, [vp, i, i]),
        "fmx_diag_rds_ring": (i, [vp, i, fp]),
        "fmx_synth_rds_bits": (i, [C.POINTER(SynthConfig), C.c_uint32, i, vp, vp]),
        "fmx_synth_host": (i, [C.POINTER(SynthConfig), C.c_uint32, i, C.c_int64, i, vp, vp, sz, i]),
        "fmx_synth_device": (i, [vp, C.POINTER(SynthConfig), C.c_uint32, i, C.c_int64, i, vp, vp, sz]),
        "fmx_synth_band_content": (i, [C.POINTER(SynthBandConfig), C.POINTER(SynthConfig)]),
        "fmx_synth_band_tile": (i, []),
        "fmx_synth_band_error": (C.c_char_p, []),
        "fmx_synth_band_host": (i, [C.POINTER(SynthBandConfig), C.c_uint32, i, C.POINTER(i), C.POINTER(SynthStation),
                                    C.POINTER(SynthFrontend), C.c_int64, i, vp, vp, sz, i]),
        "fmx_synth_band_create": (i, [vp, C.POINTER(SynthBandConfig), C.c_uint32, i, C.POINTER(i),
                                      C.POINTER(SynthStation), C.POINTER(SynthFrontend), vp, C.POINTER(vp)]),
        "fmx_synth_band_generate": (i, [vp, C.c_int64, i, vp, sz]),
        "fmx_synth_band_destroy": (i, [vp]),
        "fmx_design_taps": (i, [C.POINTER(Config), i, fp, i]),
        "fmx_resamp_schedule": (i, [C.c_float, i, C.POINTER(C.c_int), fp, i]),
        "fmx_xdr_pi_reset": (None, [C.POINTER(XdrPiState)]),
        "fmx_xdr_rds_lines": (i, [C.POINTER(XdrPiState), vp, i, C.c_char_p, i]),
        "fmx_xdr_scan_line": (i, [vp, vp, vp, i, C.c_char_p, i]),
        "fmx_xdr_signal_line": (i, [C.c_float, i, i, i, i, C.c_char_p, i]),
        "fmx_wav_header": (i, [C.c_uint32, vp]),
        "fmx_pcm_to_s16": (i, [vp, vp, i, i, C.POINTER(C.c_float), vp]),
        "fmx_iq_capture": (i, [C.c_char_p, vp, i, i]),
        "fmx_iq_replay": (i, [C.c_char_p, C.c_longlong, i, vp]),
    }
    for name, (res, args) in sig.items():
        if name in _OPTIONAL and not hasattr(L, name):
            continue  # an older library (A/B runs against a past revision)
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args
    _lib = L
    return L


def build_info():
    """fmx_build_info(): "src=<sources' SHA-256, 16 hex> defs=<variant defines>"."""
    L = lib()
    return L.fmx_build_info().decode() if hasattr(L, "fmx_build_info") else "n/a (library without fmx_build_info)"


def make_config(iq_rate=2_400_000, dsp_rate=240_000, out_rate=32_000, block=4096,
                w0_bandwidth_hz=194_000, bandwidth_hz=0, dsp_agc=0, stereo=1,
                blend=1, deemphasis=0, force_mono=0, force_stereo=0, rds=1):
    return Config(iq_rate, dsp_rate, out_rate, block, w0_bandwidth_hz, bandwidth_hz,
                  dsp_agc, stereo, blend, deemphasis, force_mono, force_stereo, rds)


def make_synth(iq_rate=2_400_000, kind=2, amplitude=0.8, noise_std=0.0,
               seed_base=0xF00D, max_offset_hz=5000, rds_level=0.05, n_bits=4096, level_spread_db=0.0):
    return SynthConfig(iq_rate, kind, amplitude, noise_std, seed_base, max_offset_hz,
                       rds_level, n_bits, level_spread_db)


class FmxError(RuntimeError):
    pass


class Handle:
    """One batch of N independent channels on one GPU."""

    def __init__(self, cfg, n_channels, device=0):
        self.L = lib()
        self.cfg = cfg
        self.n = n_channels
        h = C.c_void_p()
        rc = self.L.fmx_create(C.byref(cfg), n_channels, device, C.byref(h))
        self.h = h
        if rc != FMX_OK:
            msg = self.L.fmx_last_error(h).decode() if h.value else "?"
            if h.value:
                self.L.fmx_destroy(h)
            self.h = None
            raise FmxError(f"fmx_create failed ({rc}): {msg}")

    def _ck(self, rc, what):
        if rc != FMX_OK:
            raise FmxError(f"{what} failed ({rc}): {self.L.fmx_last_error(self.h).decode()}")

    def close(self):
        if self.h is not None:
            self.L.fmx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        self._ck(self.L.fmx_sync(self.h), "fmx_sync")

    def reset(self, channel=-1):
        self._ck(self.L.fmx_reset(self.h, channel), "fmx_reset")

    def retune(self, channel=-1, mute_samples=-1):
        """Runtime::reset + retune fade/mute (main.cpp:1028-1042, 1310-1337)."""
        self._ck(self.L.fmx_retune(self.h, channel, mute_samples), "fmx_retune")

    def set_param(self, key, value, channel=-1):
        k = PARAM[key] if isinstance(key, str) else key
        self._ck(self.L.fmx_set_param(self.h, channel, k, value), "fmx_set_param")

    def set_signal_params(self, applied_gain_db=0, gain_comp_factor=0.5, bias_db=-4.0, floor_dbfs=-55.0,
                          ceil_dbfs=-19.0, channel=-1):
        self._ck(self.L.fmx_set_signal_params(self.h, channel, applied_gain_db, gain_comp_factor, bias_db,
                                              floor_dbfs, ceil_dbfs), "fmx_set_signal_params")

    def process_block(self, d_iq, iq_stride, n, out):
        self._ck(self.L.fmx_process_block(self.h, C.c_void_p(d_iq), iq_stride, n, C.byref(out)),
                 "fmx_process_block")

    def decimate(self, d_iq, iq_stride, n_out, d_out, out_stride):
        self._ck(self.L.fmx_decimate(self.h, C.c_void_p(d_iq), iq_stride, n_out,
                                     C.c_void_p(d_out), out_stride), "fmx_decimate")

    def decimate_u8(self, d_iq, iq_stride, n_out, d_out, out_stride):
        self._ck(self.L.fmx_decimate_u8(self.h, C.c_void_p(d_iq), iq_stride, n_out,
                                        C.c_void_p(d_out), out_stride), "fmx_decimate_u8")

    def demod(self, d_iq, in_stride, n, d_mpx, mpx_stride, d_mono=None, mono_stride=0, d_count=None):
        self._ck(self.L.fmx_demod(self.h, C.c_void_p(d_iq), in_stride, n, C.c_void_p(d_mpx), mpx_stride,
                                  C.c_void_p(d_mono), mono_stride, C.c_void_p(d_count)), "fmx_demod")

    def demod_u8(self, d_iq, iq_stride, n, d_mpx, mpx_stride, d_mono=None, mono_stride=0, d_count=None, d_clip=None):
        self._ck(self.L.fmx_demod_u8(self.h, C.c_void_p(d_iq), iq_stride, n, C.c_void_p(d_mpx), mpx_stride,
                                     C.c_void_p(d_mono), mono_stride, C.c_void_p(d_count), C.c_void_p(d_clip)),
                 "fmx_demod_u8")

    def downsample(self, d_mpx, mpx_stride, n, d_out, out_stride, d_count):
        self._ck(self.L.fmx_downsample(self.h, C.c_void_p(d_mpx), mpx_stride, n, C.c_void_p(d_out), out_stride,
                                       C.c_void_p(d_count)), "fmx_downsample")

    def stereo(self, d_mpx, mpx_stride, n, d_l, d_r, lr_stride, d_st=None, d_pilot=None):
        self._ck(self.L.fmx_stereo(self.h, C.c_void_p(d_mpx), mpx_stride, n, C.c_void_p(d_l),
                                   C.c_void_p(d_r), lr_stride, C.c_void_p(d_st), C.c_void_p(d_pilot)),
                 "fmx_stereo")

    def afpost(self, d_l, d_r, in_stride, n, d_ol, d_or, out_stride, cap, d_count):
        self._ck(self.L.fmx_afpost(self.h, C.c_void_p(d_l), C.c_void_p(d_r), in_stride, n,
                                   C.c_void_p(d_ol), C.c_void_p(d_or), out_stride, cap,
                                   C.c_void_p(d_count)), "fmx_afpost")

    def rds(self, d_mpx, mpx_stride, n, d_groups, groups_stride, d_count):
        self._ck(self.L.fmx_rds(self.h, C.c_void_p(d_mpx), mpx_stride, n, C.c_void_p(d_groups),
                                groups_stride, C.c_void_p(d_count)), "fmx_rds")

    def synth_device(self, scfg, ch0, n_ch, sample0, n_samples, d_bits, d_out, out_stride):
        self._ck(self.L.fmx_synth_device(self.h, C.byref(scfg), ch0, n_ch, sample0, n_samples,
                                         C.c_void_p(d_bits), C.c_void_p(d_out), out_stride),
                 "fmx_synth_device")

    def timing_enable(self, on=True, every=1):
        """Per-kernel HIP-event timing; every=N times the launches of every N-th step only."""
        self._ck(self.L.fmx_timing_enable(self.h, max(1, int(every)) if on else 0), "fmx_timing_enable")

    def kernel_times(self):
        nk = len(KERNEL_NAMES)
        ms = (C.c_double * nk)()
        cnt = (C.c_int * nk)()
        self._ck(self.L.fmx_kernel_times(self.h, ms, cnt, nk), "fmx_kernel_times")
        return {KERNEL_NAMES[k]: (ms[k], cnt[k]) for k in range(nk)}

    def diag_set(self, what, value):
        """fmx_diag_set: what 1 = k_rds writes the RDS ring every call, 2 =
        Wideband.process_block takes the generic front end for every n."""
        self._ck(self.L.fmx_diag_set(self.h, what, value), "fmx_diag_set")

    def diag_rds_ring(self, channel):
        """The channel's 256-sample RDS FIR ring, oldest first, as a [256, 2]
        float32 array (synchronous; refilled from checkpoints first)."""
        import numpy as np
        out = np.zeros((256, 2), np.float32)
        self._ck(self.L.fmx_diag_rds_ring(self.h, channel, out.ctypes.data_as(C.POINTER(C.c_float))),
                 "fmx_diag_rds_ring")
        return out

    def host_stats(self):
        """Host waits on pinned schedule images since the last call: (waits,
        waits that blocked, milliseconds blocked)."""
        v = (C.c_double * 3)()
        self._ck(self.L.fmx_host_stats(self.h, v, 3), "fmx_host_stats")
        return {"image_waits": int(v[0]), "blocked": int(v[1]), "blocked_ms": round(v[2], 4)}


def make_wb_config(wide_rate=2_400_000, dsp_rate=240_000, format=FMX_WB_S16, taps_per_phase=0, block=4096):
    return WbConfig(wide_rate, dsp_rate, format, taps_per_phase, block)


class Wideband:
    """The wideband channelizer of one Handle (fmx_wb_*): one wide IQ capture
    in, the complex baseband rows of len(freq_hz) tuned channels out --
    Handle.demod's input.  Close it before its handle.  rational: create it
    with fmx_wb_create_rational (wide_rate / dsp_rate = P / Q; every call's
    output count is then a multiple of Q and consumes n P / Q samples)."""

    def __init__(self, handle, wcfg, freq_hz, rational=False):
        self.L = lib()
        self.handle = handle
        self.cfg = wcfg
        self.n = len(freq_hz)
        f = (C.c_int * self.n)(*[int(v) for v in freq_hz])
        w = C.c_void_p()
        name = "fmx_wb_create_rational" if rational else "fmx_wb_create"
        rc = getattr(self.L, name)(handle.h, C.byref(wcfg), f, self.n, C.byref(w))
        self.w = w if rc == FMX_OK else None
        if rc != FMX_OK:
            raise FmxError(f"{name} failed ({rc}): {self.L.fmx_last_error(handle.h).decode()}")

    def _ck(self, rc, what):
        if rc != FMX_OK:
            raise FmxError(f"{what} failed ({rc}): {self.L.fmx_last_error(self.handle.h).decode()}")

    def close(self):
        if self.w is not None and self.handle.h is not None:
            self.L.fmx_wb_destroy(self.w)
        self.w = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_freq(self, channel, freq_hz):
        self._ck(self.L.fmx_wb_set_freq(self.w, channel, int(freq_hz)), "fmx_wb_set_freq")

    def reset(self, sample0=0):
        self._ck(self.L.fmx_wb_reset(self.w, sample0), "fmx_wb_reset")

    def process(self, d_wide, n_out, d_out, out_stride):
        """d_wide: n_out * D interleaved I/Q samples; d_out: [n][out_stride] complex float."""
        self._ck(self.L.fmx_wb_process(self.w, C.c_void_p(d_wide), n_out, C.c_void_p(d_out), out_stride),
                 "fmx_wb_process")

    def process_block(self, d_wide, n, out):
        """The band receiver in one call (fmx_wb_process_block): n * D wide
        samples in, Handle.process_block's outputs (a BlockOut, d_signal None)
        for every channel; queued, valid after Handle.sync()."""
        self._ck(self.L.fmx_wb_process_block(self.w, C.c_void_p(d_wide), n, C.byref(out)),
                 "fmx_wb_process_block")

    def signal(self, d_level):
        """fmx_wb_signal: the RF level of every channel from the rows of the
        call just queued (process or process_block), once per call; d_level:
        [n] fmx_signal_level (40 bytes each, 8-byte aligned).  Queued on the
        stage stream, valid after Handle.sync()."""
        self._ck(self.L.fmx_wb_signal(self.w, C.c_void_p(d_level)), "fmx_wb_signal")

    def set_signal_params(self, applied_gain_db=0, gain_comp_factor=0.5, bias_db=-4.0, floor_dbfs=-55.0,
                          ceil_dbfs=-19.0):
        self._ck(self.L.fmx_wb_set_signal_params(self.w, applied_gain_db, gain_comp_factor, bias_db, floor_dbfs,
                                                 ceil_dbfs), "fmx_wb_set_signal_params")

    def signal_reset(self, channel=-1):
        """Restarts one channel's level smoother (-1: every channel's)."""
        self._ck(self.L.fmx_wb_signal_reset(self.w, channel), "fmx_wb_signal_reset")

    def set_iq_correction(self, mode, fixed=None, alpha=0.0):
        """fmx_wb_set_iq_correction: FMX_IQC_OFF, FMX_IQC_FIXED (fixed: an
        IqCorrection or (dc_i, dc_q, gain, cross)) or FMX_IQC_AUTO (alpha in
        (0, 1], 0: 1 / 16); holds from the next process call on."""
        self._ck(self.L.fmx_wb_set_iq_correction(self.w, mode, _iq_fixed(fixed), alpha), "fmx_wb_set_iq_correction")

    def iq_correction(self):
        """fmx_wb_iq_correction: waits for the queued calls; (dc_i, dc_q, gain, cross) as of the last one."""
        out = IqCorrection()
        self._ck(self.L.fmx_wb_iq_correction(self.w, C.byref(out)), "fmx_wb_iq_correction")
        return out.astuple()


def _iq_fixed(fixed):
    if fixed is None or isinstance(fixed, IqCorrection):
        return fixed
    return IqCorrection(*[float(v) for v in fixed])


def iq_estimate(raw, format):
    """fmx_iq_estimate (host only): the estimator of one buffer of interleaved
    raw I/Q (numpy uint8 for FMX_WB_U8, int16 for FMX_WB_S16), no smoothing
    -> (dc_i, dc_q, gain, cross)."""
    import numpy as np
    raw = np.ascontiguousarray(raw, dtype=np.int16 if format == FMX_WB_S16 else np.uint8)
    out = IqCorrection()
    rc = lib().fmx_iq_estimate(raw.ctypes.data_as(C.c_void_p), format, raw.size // 2, C.byref(out))
    if rc != FMX_OK:
        raise FmxError(f"fmx_iq_estimate failed ({rc})")
    return out.astuple()


class WidebandBank:
    """The capture bank of one Handle (fmx_wb_bank_*): len(freq_hz) wide
    captures of one configuration, capture s with the channels freq_hz[s] (a
    list, possibly empty), channelized by one launch.  The bank's channels
    are the captures' in order; d_wide is [captures][wide_stride] samples.
    Close it before its handle.  rational: create it with
    fmx_wb_bank_create_rational (wide_rate / dsp_rate = P / Q; every call's
    output count is then a multiple of Q and consumes n P / Q samples of
    every row)."""

    def __init__(self, handle, wcfg, freq_hz, rational=False):
        self.L = lib()
        self.handle = handle
        self.cfg = wcfg
        self.captures = len(freq_hz)
        self.first = [0]
        for f in freq_hz:
            self.first.append(self.first[-1] + len(f))
        self.n = self.first[-1]
        flat = [int(v) for f in freq_hz for v in f]
        first = (C.c_int * (self.captures + 1))(*self.first)
        f = (C.c_int * max(self.n, 1))(*flat)
        b = C.c_void_p()
        name = "fmx_wb_bank_create_rational" if rational else "fmx_wb_bank_create"
        rc = getattr(self.L, name)(handle.h, C.byref(wcfg), self.captures, first, f, C.byref(b))
        self.b = b if rc == FMX_OK else None
        if rc != FMX_OK:
            raise FmxError(f"{name} failed ({rc}): {self.L.fmx_last_error(handle.h).decode()}")
        # wide samples of every row per output: D, or P / Q of a rational bank
        self.ratio = wb_ratio(wcfg)[:2] if rational else (wcfg.wide_rate // wcfg.dsp_rate, 1)

    def _ck(self, rc, what):
        if rc != FMX_OK:
            raise FmxError(f"{what} failed ({rc}): {self.L.fmx_last_error(self.handle.h).decode()}")

    def close(self):
        if self.b is not None and self.handle.h is not None:
            self.L.fmx_wb_bank_destroy(self.b)
        self.b = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_freq(self, channel, freq_hz):
        self._ck(self.L.fmx_wb_bank_set_freq(self.b, channel, int(freq_hz)), "fmx_wb_bank_set_freq")

    def reset(self, capture=-1, sample0=0):
        """Restarts one capture's stream (-1: every capture's) at sample0."""
        self._ck(self.L.fmx_wb_bank_reset(self.b, capture, sample0), "fmx_wb_bank_reset")

    def process(self, d_wide, wide_stride, n_out, d_out, out_stride):
        """d_wide: [captures][wide_stride] interleaved I/Q samples, n_out * D
        (a rational bank: n_out * P / Q, see consumed) of each row read;
        d_out: [n][out_stride] complex float."""
        self._ck(self.L.fmx_wb_bank_process(self.b, C.c_void_p(d_wide), wide_stride, n_out, C.c_void_p(d_out),
                                            out_stride), "fmx_wb_bank_process")

    def consumed(self, n):
        """Wide samples of every row a call of n outputs reads: n * D, or
        n * P / Q of a rational bank (n a multiple of Q)."""
        P, Q = self.ratio
        return n // Q * P

    def process_block(self, d_wide, wide_stride, n, out):
        """fmx_wb_bank_process_block: Wideband.process_block for every
        capture's stations; consumed(n) samples of each row are read."""
        self._ck(self.L.fmx_wb_bank_process_block(self.b, C.c_void_p(d_wide), wide_stride, n, C.byref(out)),
                 "fmx_wb_bank_process_block")

    def signal(self, d_level):
        """fmx_wb_bank_signal: Wideband.signal for every channel of the bank;
        the clip ratios are those of the capture's consumed(n) raw samples."""
        self._ck(self.L.fmx_wb_bank_signal(self.b, C.c_void_p(d_level)), "fmx_wb_bank_signal")

    def set_signal_params(self, capture=-1, applied_gain_db=0, gain_comp_factor=0.5, bias_db=-4.0, floor_dbfs=-55.0,
                          ceil_dbfs=-19.0):
        self._ck(self.L.fmx_wb_bank_set_signal_params(self.b, capture, applied_gain_db, gain_comp_factor, bias_db,
                                                      floor_dbfs, ceil_dbfs), "fmx_wb_bank_set_signal_params")

    def signal_reset(self, channel=-1):
        self._ck(self.L.fmx_wb_bank_signal_reset(self.b, channel), "fmx_wb_bank_signal_reset")

    def set_iq_correction(self, mode, fixed=None, alpha=0.0, capture=-1):
        """fmx_wb_bank_set_iq_correction: Wideband.set_iq_correction for one
        capture (-1: every capture), from the next process call on."""
        self._ck(self.L.fmx_wb_bank_set_iq_correction(self.b, capture, mode, _iq_fixed(fixed), alpha),
                 "fmx_wb_bank_set_iq_correction")

    def iq_correction(self, capture):
        """fmx_wb_bank_iq_correction: waits for the queued calls; the capture's
        (dc_i, dc_q, gain, cross) as of the last one."""
        out = IqCorrection()
        self._ck(self.L.fmx_wb_bank_iq_correction(self.b, capture, C.byref(out)), "fmx_wb_bank_iq_correction")
        return out.astuple()


def wb_bank_groups(first_channel):
    """fmx_wb_bank_groups: the bank kernel's work list as [(capture, first
    channel, channels)] for a first_channel table of captures + 1 entries."""
    first = [int(v) for v in first_channel]
    n = len(first) - 1
    cap = max(n, 0) + (max(first[-1], 0) // 16 if first else 0) + 1
    t = (C.c_int * max(len(first), 1))(*first)
    out = (C.c_int * (3 * cap))()
    g = lib().fmx_wb_bank_groups(t, n, out, cap)
    if g < 0:
        raise FmxError(f"fmx_wb_bank_groups failed ({g})")
    return [tuple(out[3 * k:3 * k + 3]) for k in range(g)]


def wb_weights(wcfg, freq_hz):
    """fmx_wb_weights: W[k] as complex64 [L], read back from the f16 tables."""
    import numpy as np
    n = lib().fmx_wb_weights(C.byref(wcfg), int(freq_hz), None, 0)
    if n < 0:
        raise FmxError(f"fmx_wb_weights failed ({n})")
    buf = np.zeros(n, dtype=np.float32)
    lib().fmx_wb_weights(C.byref(wcfg), int(freq_hz), buf.ctypes.data_as(C.POINTER(C.c_float)), n)
    return buf.view(np.complex64)


def wb_ratio(wcfg):
    """fmx_wb_ratio: (P, Q, taps of the longest phase) of wide_rate / dsp_rate = P / Q."""
    P, Q, taps = C.c_int(), C.c_int(), C.c_int()
    rc = lib().fmx_wb_ratio(C.byref(wcfg), C.byref(P), C.byref(Q), C.byref(taps))
    if rc != FMX_OK:
        raise FmxError(f"fmx_wb_ratio failed ({rc})")
    return P.value, Q.value, taps.value


def wb_weights_rational(wcfg, freq_hz, phase):
    """fmx_wb_weights_rational: phase's W_r[j] as complex64 [L_r], read back from the f16 tables."""
    import numpy as np
    n = lib().fmx_wb_weights_rational(C.byref(wcfg), int(freq_hz), int(phase), None, 0)
    if n < 0:
        raise FmxError(f"fmx_wb_weights_rational failed ({n})")
    buf = np.zeros(n, np.float32)
    lib().fmx_wb_weights_rational(C.byref(wcfg), int(freq_hz), int(phase), buf.ctypes.data_as(C.POINTER(C.c_float)), n)
    return buf.view(np.complex64)


def wb_rational_geometry(wcfg, n_out):
    """fmx_wb_rational_geometry: the tiling of a call of n_out outputs as a
    dict (nt, window, lds_bytes, workgroups, tiles, Lp) with "tile": int32
    [tiles][4] of (phase, a_r, image offset, its workgroup's window)."""
    import numpy as np
    n = lib().fmx_wb_rational_geometry(C.byref(wcfg), int(n_out), None, 0)
    if n < 0:
        raise FmxError(f"fmx_wb_rational_geometry failed ({n})")
    buf = np.zeros(n, np.int32)
    lib().fmx_wb_rational_geometry(C.byref(wcfg), int(n_out), buf.ctypes.data_as(C.POINTER(C.c_int)), n)
    keys = ("nt", "window", "lds_bytes", "workgroups", "tiles", "Lp")
    g = {k: int(v) for k, v in zip(keys, buf[:6])}
    g["tile"] = buf[6:].reshape(-1, 4)
    return g


def make_wb_scan_config(wide_rate=2_400_000, dsp_rate=240_000, format=FMX_WB_S16, taps_per_phase=0, block=4096,
                        start_hz=-1_100_000, step_hz=100_000, n_points=23):
    return WbScanConfig(WbConfig(wide_rate, dsp_rate, format, taps_per_phase, block), start_hz, step_hz, n_points)


class WidebandScan:
    """The band scan of one Handle (fmx_wb_scan_*): one wide IQ capture in,
    one fmx_signal_level record per scan point out.  Close it before its handle."""

    def __init__(self, handle, scfg):
        self.L = lib()
        self.handle = handle
        self.cfg = scfg
        self.n = scfg.n_points
        s = C.c_void_p()
        rc = self.L.fmx_wb_scan_create(handle.h, C.byref(scfg), C.byref(s))
        self.s = s if rc == FMX_OK else None
        if rc != FMX_OK:
            raise FmxError(f"fmx_wb_scan_create failed ({rc}): {self.L.fmx_last_error(handle.h).decode()}")

    def _ck(self, rc, what):
        if rc != FMX_OK:
            raise FmxError(f"{what} failed ({rc}): {self.L.fmx_last_error(self.handle.h).decode()}")

    def close(self):
        if self.s is not None and self.handle.h is not None:
            self.L.fmx_wb_scan_destroy(self.s)
        self.s = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_signal_params(self, applied_gain_db=0, gain_comp_factor=0.5, bias_db=-4.0, floor_dbfs=-55.0,
                          ceil_dbfs=-19.0):
        self._ck(self.L.fmx_wb_scan_set_signal_params(self.s, applied_gain_db, gain_comp_factor, bias_db, floor_dbfs,
                                                      ceil_dbfs), "fmx_wb_scan_set_signal_params")

    def reset(self):
        self._ck(self.L.fmx_wb_scan_reset(self.s), "fmx_wb_scan_reset")

    def process(self, d_wide, n_out, d_level):
        """d_wide: n_out * D interleaved I/Q samples; d_level: [n_points] fmx_signal_level (40 bytes each)."""
        self._ck(self.L.fmx_wb_scan_process(self.s, C.c_void_p(d_wide), n_out, C.c_void_p(d_level)),
                 "fmx_wb_scan_process")

    def set_iq_correction(self, mode, fixed=None, alpha=0.0):
        """fmx_wb_scan_set_iq_correction: as Wideband.set_iq_correction, for the reads from the next one on."""
        self._ck(self.L.fmx_wb_scan_set_iq_correction(self.s, mode, _iq_fixed(fixed), alpha),
                 "fmx_wb_scan_set_iq_correction")

    def iq_correction(self):
        out = IqCorrection()
        self._ck(self.L.fmx_wb_scan_iq_correction(self.s, C.byref(out)), "fmx_wb_scan_iq_correction")
        return out.astuple()


class WidebandBankScan:
    """The band scan over a capture bank (fmx_wb_bank_scan_*):
    len(freqs_per_capture) wide captures of one plan, capture s with the scan
    points freqs_per_capture[s] (a list, possibly empty, Hz from that
    capture's centre), all read by one call.  The records are the captures'
    in order: capture s owns [first_point[s], first_point[s + 1]).  Close it
    before its handle."""

    def __init__(self, handle, wcfg, freqs_per_capture):
        self.L = lib()
        self.handle = handle
        self.cfg = wcfg
        self.captures = len(freqs_per_capture)
        self.first_point = [0]
        for f in freqs_per_capture:
            self.first_point.append(self.first_point[-1] + len(f))
        self.n_points = self.first_point[-1]
        flat = [int(v) for f in freqs_per_capture for v in f]
        first = (C.c_int * (self.captures + 1))(*self.first_point)
        f = (C.c_int * max(self.n_points, 1))(*flat)
        b = C.c_void_p()
        rc = self.L.fmx_wb_bank_scan_create(handle.h, C.byref(wcfg), self.captures, first, f, C.byref(b))
        self.b = b if rc == FMX_OK else None
        if rc != FMX_OK:
            raise FmxError(f"fmx_wb_bank_scan_create failed ({rc}): {self.L.fmx_last_error(handle.h).decode()}")

    def _ck(self, rc, what):
        if rc != FMX_OK:
            raise FmxError(f"{what} failed ({rc}): {self.L.fmx_last_error(self.handle.h).decode()}")

    def close(self):
        if self.b is not None and self.handle.h is not None:
            self.L.fmx_wb_bank_scan_destroy(self.b)
        self.b = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def process(self, d_wide, wide_stride, n_out, d_level):
        """d_wide: [captures][wide_stride] interleaved I/Q samples, n_out * D
        of each row read; d_level: [n_points] fmx_signal_level (40 bytes each)."""
        self._ck(self.L.fmx_wb_bank_scan_process(self.b, C.c_void_p(d_wide), wide_stride, n_out, C.c_void_p(d_level)),
                 "fmx_wb_bank_scan_process")

    def set_signal_params(self, capture=-1, applied_gain_db=0, gain_comp_factor=0.5, bias_db=-4.0, floor_dbfs=-55.0,
                          ceil_dbfs=-19.0):
        self._ck(self.L.fmx_wb_bank_scan_set_signal_params(self.b, capture, applied_gain_db, gain_comp_factor,
                                                           bias_db, floor_dbfs, ceil_dbfs),
                 "fmx_wb_bank_scan_set_signal_params")

    def reset(self, capture=-1):
        """Clears the level smoothers of one capture's points (-1: all)."""
        self._ck(self.L.fmx_wb_bank_scan_reset(self.b, capture), "fmx_wb_bank_scan_reset")

    def set_iq_correction(self, mode, fixed=None, alpha=0.0, capture=-1):
        """fmx_wb_bank_scan_set_iq_correction: WidebandScan.set_iq_correction
        for one capture (-1: every capture), from the next read on."""
        self._ck(self.L.fmx_wb_bank_scan_set_iq_correction(self.b, capture, mode, _iq_fixed(fixed), alpha),
                 "fmx_wb_bank_scan_set_iq_correction")

    def iq_correction(self, capture):
        """fmx_wb_bank_scan_iq_correction: waits for the queued calls; the
        capture's (dc_i, dc_q, gain, cross) as of the last read."""
        out = IqCorrection()
        self._ck(self.L.fmx_wb_bank_scan_iq_correction(self.b, capture, C.byref(out)),
                 "fmx_wb_bank_scan_iq_correction")
        return out.astuple()


def wb_bank_scan_groups(first_point):
    """fmx_wb_bank_scan_groups: the bank scan kernel's work list as [(capture,
    first point, points)] for a first_point table of captures + 1 entries."""
    first = [int(v) for v in first_point]
    n = len(first) - 1
    cap = max(n, 0) + (max(first[-1], 0) // 64 if first else 0) + 1
    t = (C.c_int * max(len(first), 1))(*first)
    out = (C.c_int * (3 * cap))()
    g = lib().fmx_wb_bank_scan_groups(t, n, out, cap)
    if g < 0:
        raise FmxError(f"fmx_wb_bank_scan_groups failed ({g})")
    return [tuple(out[3 * k:3 * k + 3]) for k in range(g)]


def wb_scan_points(scfg):
    """fmx_wb_scan_points: the plan's point frequencies (Hz from the capture's centre)."""
    n = lib().fmx_wb_scan_points(C.byref(scfg), None, 0)
    if n < 0:
        raise FmxError(f"fmx_wb_scan_points failed ({n})")
    f = (C.c_int * n)()
    lib().fmx_wb_scan_points(C.byref(scfg), f, n)
    return list(f)


def scan_peaks(dbfs, min_dbfs, min_spacing):
    """fmx_scan_peaks: ascending indices of the local maxima of dbfs at or above min_dbfs."""
    v = [float(x) for x in dbfs]
    n = len(v)
    arr = (C.c_double * max(n, 1))(*v)
    idx = (C.c_int * max(n, 1))()
    k = lib().fmx_scan_peaks(arr, n, float(min_dbfs), int(min_spacing), idx, n)
    if k < 0:
        raise FmxError(f"fmx_scan_peaks failed ({k})")
    return list(idx[:k])


def synth_rds_bits(scfg, ch0, n_ch):
    import numpy as np
    bits = np.zeros((n_ch, scfg.n_bits), dtype=np.uint8)
    ng = scfg.n_bits // 104
    groups = np.zeros((n_ch, ng, 4), dtype=np.uint16)
    rc = lib().fmx_synth_rds_bits(C.byref(scfg), ch0, n_ch, bits.ctypes.data, groups.ctypes.data)
    if rc != FMX_OK:
        raise FmxError("fmx_synth_rds_bits failed")
    return bits, groups


def synth_host(scfg, ch0, n_ch, sample0, n_samples, bits=None, threads=8):
    import numpy as np
    out = np.zeros((n_ch, 2 * n_samples), dtype=np.uint8)
    bp = bits.ctypes.data if bits is not None else None
    rc = lib().fmx_synth_host(C.byref(scfg), ch0, n_ch, sample0, n_samples, bp,
                              out.ctypes.data, out.shape[1], threads)
    if rc != FMX_OK:
        raise FmxError("fmx_synth_host failed")
    return out


def make_synth_band(wide_rate=2_400_000, format=FMX_WB_S16, kind=2, seed_base=0xF00D, max_offset_hz=5000,
                    rds_level=0.05, n_bits=4096, noise_std=0.0):
    return SynthBandConfig(wide_rate, format, kind, seed_base, max_offset_hz, rds_level, n_bits, noise_std)


def synth_band_tile():
    """fmx_synth_band_tile: samples per workgroup of the band kernel."""
    return lib().fmx_synth_band_tile()


def synth_band_content(bcfg):
    """fmx_synth_band_content: the SynthConfig whose channel ch0 + g is station g's content."""
    out = SynthConfig()
    if lib().fmx_synth_band_content(C.byref(bcfg), C.byref(out)) != FMX_OK:
        raise FmxError(f"fmx_synth_band_content failed: {lib().fmx_synth_band_error().decode()}")
    return out


def _synth_band_tables(captures, frontends):
    """captures: [[(freq_hz, amplitude), ...], ...]; frontends: None or one
    (dc_i, dc_q, q_gain, q_cross) per capture -> the C tables."""
    first = [0]
    for c in captures:
        first.append(first[-1] + len(c))
    flat = [(int(f), float(a)) for c in captures for (f, a) in c]
    t_first = (C.c_int * len(first))(*first)
    t_st = (SynthStation * max(len(flat), 1))(*[SynthStation(f, a) for f, a in flat])
    t_fe = None
    if frontends is not None:
        if len(frontends) != len(captures):
            raise ValueError("one front end per capture")
        t_fe = (SynthFrontend * max(len(frontends), 1))(*[SynthFrontend(*[float(v) for v in fe]) for fe in frontends])
    return first, t_first, t_st, t_fe


def synth_band_bits(bcfg, ch0, n_stations):
    """The content config, the RDS bit rows [n_stations][n_bits] and the
    transmitted groups [n_stations][n_bits // 104][4] of a band's stations
    (fmx_synth_rds_bits on the content config); bits and groups are None
    unless the band's kind is 2."""
    content = synth_band_content(bcfg)
    if bcfg.kind != 2 or bcfg.n_bits <= 0:
        return content, None, None
    bits, groups = synth_rds_bits(content, ch0, n_stations)
    return content, bits, groups


def synth_band_host(bcfg, ch0, captures, sample0, n_samples, frontends=None, bits="auto", wide_stride=None,
                    threads=8, out=None):
    """fmx_synth_band_host: the band on the CPU, [captures][wide_stride][2]
    int16 or uint8.  bits: the RDS bit rows, None, or "auto" (made from the
    content config when the kind is 2); out: an array to fill (cells past
    n_samples of a row are left as they are)."""
    import numpy as np
    first, t_first, t_st, t_fe = _synth_band_tables(captures, frontends)
    if isinstance(bits, str):
        bits = synth_band_bits(bcfg, ch0, first[-1])[1]
    stride = n_samples if wide_stride is None else wide_stride
    if out is None:
        out = np.zeros((len(captures), max(stride, 0), 2), dtype=np.int16 if bcfg.format == FMX_WB_S16 else np.uint8)
    rc = lib().fmx_synth_band_host(C.byref(bcfg), ch0, len(captures), t_first, t_st, t_fe, sample0, n_samples,
                                   bits.ctypes.data if bits is not None else None, out.ctypes.data, stride, threads)
    if rc != FMX_OK:
        raise FmxError(f"fmx_synth_band_host failed ({rc}): {lib().fmx_synth_band_error().decode()}")
    return out


class SynthBand:
    """The synthetic FM band on the GPU (fmx_synth_band_*): len(captures) wide
    captures of one rate and format, capture s with the stations captures[s],
    a list (possibly empty) of (freq_hz, amplitude); station g of all has the
    content of channel ch0 + g of .content.  .bits and .groups are the RDS bit
    rows and the transmitted groups of a kind-2 band (else None).  generate
    is one launch on the handle's stage stream.  Close it before its handle."""

    def __init__(self, handle, cfg, ch0, captures, frontends=None):
        self.L = lib()
        self.handle = handle
        self.cfg = cfg
        self.ch0 = ch0
        self.captures = len(captures)
        self.b = None
        self.first_station, t_first, t_st, t_fe = _synth_band_tables(captures, frontends)
        self.n_stations = self.first_station[-1]
        self.content, self.bits, self.groups = synth_band_bits(cfg, ch0, self.n_stations)
        b = C.c_void_p()
        rc = self.L.fmx_synth_band_create(handle.h, C.byref(cfg), ch0, self.captures, t_first, t_st, t_fe,
                                          self.bits.ctypes.data if self.bits is not None else None, C.byref(b))
        if rc != FMX_OK:
            raise FmxError(f"fmx_synth_band_create failed ({rc}): {self.L.fmx_last_error(handle.h).decode()}")
        self.b = b

    def _ck(self, rc, what):
        if rc != FMX_OK:
            raise FmxError(f"{what} failed ({rc}): {self.L.fmx_last_error(self.handle.h).decode()}")

    def close(self):
        if self.b is not None and self.handle.h is not None:
            self.L.fmx_synth_band_destroy(self.b)
        self.b = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def generate(self, sample0, n, d_out, wide_stride):
        """d_out: [captures][wide_stride] interleaved I/Q samples of the band's
        format; samples sample0 .. sample0 + n of every capture are written."""
        self._ck(self.L.fmx_synth_band_generate(self.b, sample0, n, C.c_void_p(d_out), wide_stride),
                 "fmx_synth_band_generate")


def design_taps(cfg, which):
    import numpy as np
    n = lib().fmx_design_taps(C.byref(cfg), which, None, 0)
    if n < 0:
        raise FmxError("fmx_design_taps failed")
    buf = np.zeros(n, dtype=np.float32)
    lib().fmx_design_taps(C.byref(cfg), which,
                          buf.ctypes.data_as(C.POINTER(C.c_float)), n)
    return buf


def resamp_schedule(del_, n_in):
    import numpy as np
    cap = int(n_in / max(del_, 0.5)) + 16
    packed = np.zeros(cap, dtype=np.int32)
    mu = np.zeros(cap, dtype=np.float32)
    k = lib().fmx_resamp_schedule(C.c_float(del_), n_in,
                                  packed.ctypes.data_as(C.POINTER(C.c_int)),
                                  mu.ctypes.data_as(C.POINTER(C.c_float)), cap)
    return packed[:k], mu[:k]


# ---- host-side formats (fmx_host.cpp): XDR RDS / scan lines, WAV, IQ files ----
class XdrRds:
    """Per-channel XDRServer RDS state (PI debounce) turning fmx_rds_group
    records into the server's "P"/"R" lines."""

    def __init__(self):
        self.st = XdrPiState()
        lib().fmx_xdr_pi_reset(C.byref(self.st))

    def lines(self, groups):
        """groups: list of (a, b, c, d, errors) -> list of lines (no newline)."""
        import numpy as np
        n = len(groups)
        arr = (RdsGroup * max(n, 1))()
        for k, (a, b, c, d, e) in enumerate(groups):
            arr[k] = RdsGroup(a, b, c, d, e, 0, 0)
        cap = 32 * max(n, 1) + 1
        buf = C.create_string_buffer(cap)
        rc = lib().fmx_xdr_rds_lines(C.byref(self.st), C.cast(arr, C.c_void_p), n, buf, cap)
        if rc < 0:
            raise FmxError(f"fmx_xdr_rds_lines failed ({rc})")
        return buf.value.decode().splitlines()


def xdr_scan_line(freq_khz, level_sum, reads):
    import numpy as np
    f = np.ascontiguousarray(freq_khz, dtype=np.int32)
    s = np.ascontiguousarray(level_sum, dtype=np.float64)
    r = np.ascontiguousarray(reads, dtype=np.int32)
    cap = 24 * len(f) + 2
    buf = C.create_string_buffer(cap)
    rc = lib().fmx_xdr_scan_line(f.ctypes.data, s.ctypes.data, r.ctypes.data, len(f), buf, cap)
    if rc < 0:
        raise FmxError(f"fmx_xdr_scan_line failed ({rc})")
    return buf.value.decode()


def xdr_signal_line(level, stereo=False, forced_mono=False, cci=-1, aci=-1):
    """fmx_xdr_signal_line: the XDR server's "S" line of one station (with its newline)."""
    buf = C.create_string_buffer(64)
    rc = lib().fmx_xdr_signal_line(float(level), int(bool(stereo)), int(bool(forced_mono)), int(cci), int(aci), buf, 64)
    if rc < 0:
        raise FmxError(f"fmx_xdr_signal_line failed ({rc})")
    return buf.value.decode()


def wav_header(data_bytes):
    import numpy as np
    h = np.zeros(44, dtype=np.uint8)
    lib().fmx_wav_header(data_bytes, h.ctypes.data)
    return h.tobytes()


def pcm_to_s16(left, right, volume_percent=100, volume_scale=0.85):
    """Returns (interleaved int16 array, new volume_scale)."""
    import numpy as np
    l = np.ascontiguousarray(left, dtype=np.float32)
    r = np.ascontiguousarray(right, dtype=np.float32)
    out = np.zeros(2 * len(l), dtype=np.int16)
    vs = C.c_float(volume_scale)
    rc = lib().fmx_pcm_to_s16(l.ctypes.data, r.ctypes.data, len(l), volume_percent, C.byref(vs), out.ctypes.data)
    if rc < 0:
        raise FmxError("fmx_pcm_to_s16 failed")
    return out, vs.value


def iq_capture(path, iq, append=True):
    import numpy as np
    a = np.ascontiguousarray(iq, dtype=np.uint8)
    rc = lib().fmx_iq_capture(path.encode(), a.ctypes.data, a.size // 2, 1 if append else 0)
    if rc < 0:
        raise FmxError("fmx_iq_capture failed")
    return rc


def iq_replay(path, sample_offset, n_samples):
    import numpy as np
    out = np.zeros(2 * n_samples, dtype=np.uint8)
    k = lib().fmx_iq_replay(path.encode(), sample_offset, n_samples, out.ctypes.data)
    if k < 0:
        raise FmxError("fmx_iq_replay failed")
    return out[:2 * k]
