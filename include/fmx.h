/*
 * fmx.h -- C ABI of the MI355X many-channel FM demodulator (libfmx.so).
 *
 * This is the drop-in boundary for bkram/fmtuner-sdr's per-block DSP hot path
 * (SURVEY.md 8b).  One handle holds N independent channels, each with the
 * exact state of one set of reference objects:
 *
 *   ComplexDecimator   include/dsp/liquid_primitives.h:161-188
 *   FMDemod            include/fm_demod.h:11-67
 *   StereoDecoder      include/stereo_decoder.h:10-55
 *   AFPostProcessor    include/af_post_processor.h:9-37
 *   RDSDecoder         include/rds_decoder.h:17-29
 *
 * and one call of fmx_process_block() replaces one iteration of the
 * reference's per-block body (src/main.cpp:1239-1308) for every channel.
 * The C++ facades in include/fmx_blocks.hpp map one reference object onto one
 * channel slot and keep the reference's method signatures.
 *
 * Conventions (reference-compatible):
 *   - sizes are SAMPLES, not bytes; IQ buffers are 2*n bytes, I then Q;
 *   - the caller owns every buffer; outputs are written from index 0;
 *   - functions return 0 (FMX_OK) or a negative FMX_E* code; the message is
 *     available from fmx_last_error(); nothing throws across the ABI;
 *   - pointers named d_* are DEVICE pointers (hipMalloc'd memory on the
 *     handle's device), pointers named h_* are host pointers;
 *   - buffer geometry: a base pointer needs its element's own alignment only
 *     (1 for u8 IQ, 4 for float / int / fmx_rds_group, 8 for fmx_signal_level)
 *     and a stride is any element count >= the row's logical length; a row's
 *     cells past its logical length (MPX n, PCM pcm_count[c], groups
 *     min(count, groups_stride)) are never written.  The fast kernels need
 *     more and the host checks it per call: IQ base, iq_stride and 2*n*M
 *     multiples of 16 bytes (k_fe8), MPX base 16-B aligned and mpx_stride a
 *     multiple of 4 floats (k_rs, k_pilot's 16-B loads).  Any other geometry
 *     is correct, on slower kernels;
 *   - a handle is not thread-safe (like the reference objects); all work is
 *     queued on the handle's own HIP stream, fmx_sync() waits for it.
 *
 * No HIP or torch types appear in this header.
 */
#ifndef FMX_H
#define FMX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI history: the synthetic FM band (fmx_synth_band_content, fmx_synth_band_tile, fmx_synth_band_host,
 * fmx_synth_band_create, fmx_synth_band_generate, fmx_synth_band_destroy, and fmx_synth_band_error for the
 * host calls' messages: wide captures of many stations, generated on the GPU) arrived at 13 without a bump:
 * additions only; the bank scan's correction per capture (fmx_wb_bank_scan_set_iq_correction,
 * fmx_wb_bank_scan_iq_correction) arrived at 13 without a bump: additions only;
 * the band scan over a capture bank (fmx_wb_bank_scan_create, fmx_wb_bank_scan_destroy,
 * fmx_wb_bank_scan_set_signal_params, fmx_wb_bank_scan_reset, fmx_wb_bank_scan_process, fmx_wb_bank_scan_groups:
 * every capture's scan points read in one call) arrived at 13 without a bump: additions only;
 * the capture bank at rational rates (fmx_wb_bank_create_rational: many 2.048, 10 or 20 MS/s captures
 * channelized at P / Q in one call) arrived at 13 without a bump, as the bank and the rational rates did: an addition only;
 * the bank's correction per capture (fmx_wb_bank_set_iq_correction, fmx_wb_bank_iq_correction) arrived at 13
 * without a bump: additions only; the DC / IQ-imbalance correction (fmx_wb_set_iq_correction, fmx_wb_iq_correction,
 * fmx_wb_scan_set_iq_correction, fmx_wb_scan_iq_correction, fmx_iq_estimate, fmx_iq_correction, FMX_IQC_*)
 * arrived at 13 without a bump, as the bank and the rational rates did: additions only; rational wide rates (fmx_wb_create_rational, fmx_wb_ratio, fmx_wb_weights_rational,
 * fmx_wb_rational_geometry: 20, 10 and 2.048 MS/s captures channelized at P / Q) arrived at 13 without a bump,
 * as the bank did: additions only; the capture bank (fmx_wb_bank_*: many wide captures channelized in one call) arrived at 13
 * without a bump: its symbols are additions, no existing symbol, struct or enum changed, and a caller built
 * against the earlier 13 runs unchanged (a caller that needs the bank looks its symbols up);
 * 13 adds the band receiver's RF level (fmx_wb_signal, fmx_wb_set_signal_params,
 * fmx_wb_signal_reset: every station's level from the rows of the call just queued) and fmx_xdr_signal_line;
 * 12 adds the one-call band receiver (fmx_wb_process_block: one wide IQ capture in, every
 * station's audio, stereo state and RDS groups out), FMX_DIAG_FE_GENERIC and fmx_diag_lds_bytes; 11 adds the band scan (fmx_wb_scan_*, fmx_scan_peaks: one wide IQ capture in, the RF
 * level of every scan point out); 10 adds the wideband channelizer (fmx_wb_*: one wide IQ capture in, every tuned
 * channel's baseband out); 9 (round 6) adds fmx_diag_set / fmx_diag_rds_ring and fmx_build_info; 8 (round 5) adds FMX_K_BITS (FMX_K_COUNT 8); 7 (round 5) adds fmx_host_stats and FMX_K_FRONTEND_GENERIC (FMX_K_COUNT 7); 6 (round 4) adds FMX_K_PILOT (FMX_K_COUNT 6); 5 (round 4) added FMX_K_RS (FMX_K_COUNT 5; fmx_kernel_times
 * fills at most n entries); 4 (round 3) added fmx_synth_config.level_spread_db,
 * which changed that struct's size: callers must be rebuilt against this
 * header. */
#define FMX_ABI_VERSION 13

enum {
  FMX_OK = 0,
  FMX_E_INVALID = -1,   /* bad argument / unsupported configuration        */
  FMX_E_HIP = -2,       /* HIP runtime failure                             */
  FMX_E_NOMEM = -3,     /* device allocation failed                        */
  FMX_E_CAPACITY = -4,  /* n exceeds the block size the handle was made for */
  FMX_E_NODEVICE = -5   /* no HIP device / kernels not loadable            */
};

/* dsp_agc (config.h:51) */
enum { FMX_AGC_OFF = 0, FMX_AGC_FAST = 1, FMX_AGC_SLOW = 2 };
/* stereo_blend (config.h:52) */
enum { FMX_BLEND_SOFT = 0, FMX_BLEND_NORMAL = 1, FMX_BLEND_AGGRESSIVE = 2 };
/* tuner.deemphasis (main.cpp:699-708) */
enum { FMX_DEEMPH_50US = 0, FMX_DEEMPH_75US = 1, FMX_DEEMPH_OFF = 2 };

typedef struct {
  int iq_rate;         /* SDR rate, integer multiple of dsp_rate             */
  int dsp_rate;        /* 240000 (2.4 MS/s / 10) or 256000 (reference)       */
  int out_rate;        /* 32000                                              */
  int block;           /* max DSP samples per call (dsp_block_samples)       */
  int w0_bandwidth_hz; /* processing.w0_bandwidth_hz                         */
  int bandwidth_hz;    /* XDR W value (0 = W0)                               */
  int dsp_agc;         /* FMX_AGC_*                                          */
  int stereo;          /* processing.stereo                                  */
  int blend;           /* FMX_BLEND_*                                        */
  int deemphasis;      /* FMX_DEEMPH_*                                       */
  int force_mono;
  int force_stereo;
  int rds;             /* decode RDS                                          */
} fmx_config;

/* One RDS group as the reference's RDSGroup (rds_decoder.h:9-15). */
typedef struct {
  uint16_t a, b, c, d;
  uint8_t errors; /* (eA<<6)|(eB<<4)|(eC<<2)|eD, e: 0 ok, 1 corrected, 3 missing */
  uint8_t pad;
  uint32_t block_index; /* fmx_process_block call that emitted it */
} fmx_rds_group;

/* RF-domain level of the raw u8 IQ of one call, as computeSignalLevel
 * (src/signal_level.cpp:145-204) + smoothSignalLevel (:206-214) of the
 * reference's per-read path (main.cpp:1166-1174). */
typedef struct {
  float level120;          /* SignalLevelResult::level120                     */
  float level120_smoothed; /* smoothSignalLevel(level120, per-channel state)  */
  double dbfs;
  double compensated_dbfs;
  double hard_clip_ratio;
  double near_clip_ratio;
} fmx_signal_level;

/* Device output buffers of fmx_process_block (all optional except where
 * noted; pass NULL to skip).  Strides are in elements. */
typedef struct {
  float *d_mpx;            /* [C][mpx_stride] discriminator MPX at dsp_rate   */
  int mpx_stride;
  float *d_pcm_l;          /* [C][pcm_stride] clamped 32 kHz audio (required) */
  float *d_pcm_r;          /* [C][pcm_stride]                                 */
  int pcm_stride;
  int *d_pcm_count;        /* [C] samples written per channel (required)      */
  int *d_stereo;           /* [C] StereoDecoder::isStereo()                   */
  int *d_pilot_tenths;     /* [C] getPilotLevelTenthsKHz()                    */
  float *d_clip_ratio;     /* [C] FMDemod::getClippingRatio()                 */
  fmx_rds_group *d_groups; /* [C][groups_stride]                              */
  int groups_stride;
  int *d_group_count;      /* [C]                                             */
  fmx_signal_level *d_signal; /* [C] RF level of this call's IQ (u8 input)    */
  int *d_stereo_indicator; /* [C] XDR stereo flag: isStereo() || (forceMono &&
                              stereo && pilot >= 2.0 kHz), main.cpp:1298-1300 */
} fmx_block_out;

/* ---- build record ----
 * "src=<16 hex> defs=<A/B defines>": the first 16 hex digits of the SHA-256
 * of the sources this library was compiled from (fmtuner-sdr_amd/Makefile
 * FMX_SRC_SHA: csrc/, include/fmx.h, include/fmx_blocks.hpp and the Makefile,
 * concatenated in sorted path order) and the variant defines (empty for the
 * shipped library).  __graft_entry__.smoke() checks it against the tree. */
const char *fmx_build_info(void);

/* ---- lifetime ---- */
int fmx_device_count(void);
int fmx_create(const fmx_config *cfg, int n_channels, int device, void **handle);
int fmx_destroy(void *handle);
const char *fmx_last_error(void *handle);
int fmx_sync(void *handle);
int fmx_num_channels(void *handle);

/* Runtime::reset fan-out (main.cpp:686-691: demod, stereo, afPost,
 * decimator) plus the RDS worker reset (main.cpp:909-916).  channel = -1
 * resets every channel. */
int fmx_reset(void *handle, int channel);
/* The retune path of main.cpp:1028-1042: the same reset fan-out, then the
 * PCM of the next mute_samples 32 kHz outputs (per channel, across calls) is
 * faded out over OUTPUT_RATE/200 samples, muted, and faded back in, as
 * main.cpp:1310-1337 does after the clamp.  mute_samples < 0 takes the
 * reference's kRetuneMuteSamples = OUTPUT_RATE/25 (main.cpp:696-697); 0
 * cancels a running mute.  At most 65535. */
int fmx_retune(void *handle, int channel, int mute_samples);

/* Per-channel settings mirroring the reference setters; channel = -1 = all. */
enum {
  FMX_PARAM_BANDWIDTH_HZ = 1,  /* FMDemod::setBandwidthHz (fm_demod.cpp:168)   */
  FMX_PARAM_W0_HZ = 2,         /* FMDemod::setW0BandwidthHz (:206)             */
  FMX_PARAM_DEEMPHASIS = 3,    /* tuner.deemphasis 0/1/2 -> both demod + AF   */
  FMX_PARAM_DSP_AGC = 4,       /* FMDemod::setDspAgcMode (:210)                */
  FMX_PARAM_BLEND = 5,         /* StereoDecoder::setBlendMode                  */
  FMX_PARAM_FORCE_MONO = 6,    /* StereoDecoder::setForceMono                  */
  FMX_PARAM_FORCE_STEREO = 7,  /* StereoDecoder::setForceStereo                */
  FMX_PARAM_BANDWIDTH_MODE = 8, /* FMDemod::setBandwidthMode (TEF table)       */
  FMX_PARAM_DEEMPH_US = 9,     /* setDeemphasis(tau_us) of FMDemod + AFPostProcessor,
                                  any tau; <= 0 switches it off (fm_demod.cpp:50-62) */
  FMX_PARAM_DEVIATION_HZ = 10  /* FMDemod::setDeviation(Hz) (fm_demod.cpp:64-71)  */
};
int fmx_set_param(void *handle, int channel, int key, int value);
/* computeSignalLevel's arguments (main.cpp:1166-1170): applied tuner gain
 * (dB), gain compensation factor (kSignalGainCompFactor 0.5, main.cpp:513),
 * config sdr.signal_bias_db / signal_floor_dbfs / signal_ceil_dbfs
 * (config.h:27-29; defaults -4 / -55 / -19).  channel = -1 = all. */
int fmx_set_signal_params(void *handle, int channel, int applied_gain_db, double gain_comp_factor,
                          double bias_db, double floor_dbfs, double ceil_dbfs);

/* One reference block for every channel.  d_iq: [C][iq_stride] bytes, each
 * row holding 2*n*M interleaved u8 I/Q (M = iq_rate / dsp_rate); n <= block.
 * Queued on the handle's stream; results are valid after fmx_sync(). */
int fmx_process_block(void *handle, const uint8_t *d_iq, size_t iq_stride, int n,
                      const fmx_block_out *out);

/* ---- per-object stages (same state as fmx_process_block) ----
 * Each mirrors one reference method, batched over all C channels. */
/* ComplexDecimator::executeComplex: d_out [C][out_stride] complex float */
int fmx_decimate(void *handle, const uint8_t *d_iq, size_t iq_stride, int n_out, float *d_out,
                 int out_stride);
/* ComplexDecimator::execute (liquid_primitives.cpp:422-459): the same
 * decimation, requantised to interleaved u8 (clamp(y*127.5 + 127.5) -> u8);
 * d_out [C][out_stride] bytes, 2 per output sample */
int fmx_decimate_u8(void *handle, const uint8_t *d_iq, size_t iq_stride, int n_out, uint8_t *d_out,
                    size_t out_stride);
/* FMDemod::processSplitComplex(iq, mpx, mono, n): d_iq_cf complex float
 * [C][in_stride]; d_mono may be NULL (stereo mode: returns 0 samples). */
int fmx_demod(void *handle, const float *d_iq_cf, int in_stride, int n, float *d_mpx, int mpx_stride,
              float *d_mono, int mono_stride, int *d_mono_count);
/* FMDemod::processSplit(iq, mpx, mono, n) on u8 IQ at dsp_rate (iq_rate ==
 * dsp_rate; byte LUT (v-127)/127.5, clip = byte 0/255, fm_demod.cpp:219-249) */
int fmx_demod_u8(void *handle, const uint8_t *d_iq, size_t iq_stride, int n, float *d_mpx, int mpx_stride,
                 float *d_mono, int mono_stride, int *d_mono_count, float *d_clip_ratio);
/* FMDemod::downsampleAudio(demod, audio, n): mono resampler + de-emphasis +
 * DC block on MPX (fm_demod.cpp:279-295) */
int fmx_downsample(void *handle, const float *d_mpx, int mpx_stride, int n, float *d_out, int out_stride,
                   int *d_count);
/* StereoDecoder::processAudio */
int fmx_stereo(void *handle, const float *d_mpx, int mpx_stride, int n, float *d_left, float *d_right,
               int lr_stride, int *d_stereo, int *d_pilot_tenths);
/* AFPostProcessor::process (outCapacity = cap) */
int fmx_afpost(void *handle, const float *d_left, const float *d_right, int in_stride, int n,
               float *d_out_l, float *d_out_r, int out_stride, int cap, int *d_count);
/* RDSDecoder::process: groups of this call per channel */
int fmx_rds(void *handle, const float *d_mpx, int mpx_stride, int n, fmx_rds_group *d_groups,
            int groups_stride, int *d_group_count);

/* ---- wideband channelizer: one wide IQ capture in, every channel's baseband out ----
 * The reference's ComplexDecimator generalised to tuned channels.  With
 * D = wide_rate / dsp_rate, L = D * taps_per_phase taps h = firdes_kaiser(L,
 * fc, 80 dB), fc = min(0.45 / D, 0.45), channel c tuned to freq_hz[c]
 * (relative to the capture's centre, |f| <= wide_rate / 2) produces
 *   y_c[n] = 2 fc sum_k h[k] x[nD - k] exp(-j 2 pi f_c (nD - k) / wide_rate)
 * with x[i < 0] = 0, i the wide-sample index since the last reset plus its
 * sample0, x = (b - 127.5) / 127.5 for FMX_WB_U8 (interleaved u8 I/Q) and
 * v / 32768 for FMX_WB_S16 (interleaved int16 I/Q).  At f = 0 this is
 * ComplexDecimator::executeComplex.  d_out is [n_channels][out_stride] complex
 * float at dsp_rate: fmx_demod's input on a handle of n_channels channels.
 * The object keeps the last L - 1 raw wide samples and a 64-bit sample
 * counter; its outputs do not depend on how the stream is cut into calls.
 * Calls are queued on the handle's stream (a following fmx_demod is ordered
 * behind them); the object is destroyed before its handle.  Geometry: d_wide
 * needs its element's alignment only (1 byte for u8, 2 for int16), d_out 4
 * bytes; out_stride counts complex elements and is >= n_out (fmx_demod's
 * in_stride counts floats: 2 * out_stride); cells past n_out are never
 * written. */
enum { FMX_WB_U8 = 0, FMX_WB_S16 = 1 };
typedef struct {
  int wide_rate;      /* integer multiple D of dsp_rate, 2 <= D <= 128 (P / Q of it: fmx_wb_create_rational) */
  int dsp_rate;
  int format;         /* FMX_WB_*                                                  */
  int taps_per_phase; /* 4..28; 0: the reference's rule (28 from D = 8, 20 from 4, else 12) */
  int block;          /* max outputs per channel and call                          */
} fmx_wb_config;
int fmx_wb_create(void *handle, const fmx_wb_config *cfg, const int *freq_hz, int n_channels, void **wb);
int fmx_wb_destroy(void *wb);
/* ordered after the calls queued so far and before later ones; from the next
 * call on the channel's outputs are those of a channel that had always been
 * at freq_hz (the history is raw input) */
int fmx_wb_set_freq(void *wb, int channel, int freq_hz);
/* clears the history; the next call's first wide sample has index sample0 */
int fmx_wb_reset(void *wb, int64_t sample0);
/* consumes n_out * D wide samples (n_out <= block, else FMX_E_CAPACITY) */
int fmx_wb_process(void *wb, const void *d_wide, int n_out, float *d_out, int out_stride);
/* The band receiver in one call: one reference block (main.cpp:1239-1308) for
 * every channel of the channelizer.  Consumes n * D wide samples; the outputs
 * are fmx_process_block's for a handle whose decimator had produced the
 * channelizer's rows: PCM (clamped; fmx_retune's fade and mute apply), counts,
 * stereo flag, pilot tenths, stereo indicator, RDS groups and counts, d_mpx;
 * stereo and RDS as the handle's config says.  d_clip_ratio is
 * FMDemod::getClippingRatio of processSplitComplex on the rows (the share of
 * the call's n samples with |re| or |im| >= 0.995).  d_signal must be NULL
 * (FMX_E_INVALID otherwise): fmx_wb_signal below, called behind this call,
 * delivers every station's RF level from this call's own rows.
 * Conditions: the handle has iq_rate == dsp_rate, the channelizer that
 * dsp_rate and the handle's channel count (FMX_E_INVALID otherwise, the
 * message names this function); n <= min(the handle's block, the
 * channelizer's), else FMX_E_CAPACITY; d_pcm_l, d_pcm_r and d_pcm_count are
 * required; n == 0 does nothing.  Queued like fmx_process_block, on the same
 * four streams and without draining them: calls may be queued ahead, and
 * fmx_reset / fmx_retune / fmx_wb_set_freq between queued calls take effect
 * at the next call.  The channelizer's history and sample counter advance as
 * in fmx_wb_process, and a stream may mix the two calls; the rows themselves
 * stay inside the object (fmx_wb_process returns them).  Calls of n >= 1024
 * with n % 4 == 0 run the fast front end (k_fecf, then k_pilot / k_rs as after
 * k_fe8); every other n >= 1 is correct on the generic one. */
int fmx_wb_process_block(void *wb, const void *d_wide, int n, const fmx_block_out *out);
/* The RF level of every channel from the rows of the object's most recent
 * non-empty call (fmx_wb_process or fmx_wb_process_block; a call of n == 0
 * does nothing and does not count): what the reference computes on every read
 * (main.cpp:1166-1174) and hands to XDRServer::updateSignal every block
 * (main.cpp:1301).  The definition is the band scan's (below), taken over the
 * rows the channelizer produced: with y_c[m], m = 0 .. n - 1, channel c's row
 * of that call, history and sample counter included as fmx_wb_process defines
 * them,
 *   P_c  = (1 / n) sum_m |y_c[m]|^2
 *   rms  = sqrt(max(1e-15, 0.5 P_c)),  dbfs = 20 log10(rms + 1e-12)
 * and compensated_dbfs, level120 (one float conversion), level120_smoothed
 * (one smoother per channel of the object), hard_clip_ratio and
 * near_clip_ratio (of the call's n * D raw samples, the same in every record)
 * as the scan forms them; no mean is removed, for the scan's reason.  What
 * differs from the scan: every one of the n outputs counts -- the object has
 * the history, so no window reaches before known samples; the first
 * taps_per_phase outputs after fmx_wb_reset are the filter filling from zeros
 * and count as they are; every n >= 1 is valid.
 * d_level is [n_channels], 8-byte aligned; cells outside [0, n_channels) are
 * never written.  The call is queued on the handle's stage stream behind the
 * call it measures and ahead of the object's next call; it neither joins nor
 * drains the other streams, so fmx_wb_process_block calls stay queued ahead.
 * Results are valid after fmx_sync; d_level may rotate with the caller's
 * output sets.  The object remembers the measured call's d_wide, n, rows and
 * stride: after fmx_wb_process the rows are the caller's d_out, and d_out
 * and d_wide must stay as they were until this call's work is done (after
 * fmx_wb_process_block: d_wide).  Any geometry fmx_wb_process accepts is read
 * correctly (4-byte aligned rows, any out_stride >= n_out), and the sum's
 * order depends on n alone: equal rows give equal records, bit for bit.
 * A call is measured once: FMX_E_INVALID (the message names this function)
 * when no call has been made since creation, when the most recent call has
 * been measured already (the smoother would advance twice), for a NULL d_level
 * and for one that is not 8-byte aligned. */
int fmx_wb_signal(void *wb, fmx_signal_level *d_level);
/* One set per object (the capture has one tuner gain); defaults as
 * fmx_set_signal_params' (gain 0, factor 0.5, bias -4, floor -55, ceil -19).
 * The values travel with each launch: a change holds from the next
 * fmx_wb_signal on. */
int fmx_wb_set_signal_params(void *wb, int applied_gain_db, double gain_comp_factor, double bias_db,
                             double floor_dbfs, double ceil_dbfs);
/* Restarts channel's level smoother (-1: every channel's), ordered behind the
 * level calls queued so far.  fmx_wb_reset and fmx_wb_set_freq leave the
 * smoothers alone: the reference's rfLevelSmoother (main.cpp:698) lives
 * across retunes. */
int fmx_wb_signal_reset(void *wb, int channel);
/* host only: the channel weights W[k] = 2 fc h[k] exp(+j 2 pi f k / wide_rate),
 * k = 0..L-1, as 2L floats (re, im) read back from the kernel's f16 hi + lo
 * tables.  Returns 2L (negative on error). */
int fmx_wb_weights(const fmx_wb_config *cfg, int freq_hz, float *out, int cap);

/* ---- rational rates: wide_rate / dsp_rate = P / Q in lowest terms ----
 * fmx_wb_create refuses a wide_rate that is no multiple of dsp_rate;
 * fmx_wb_create_rational takes it (20 MS/s to 240 kHz is 250 / 3, 10 MS/s
 * 125 / 3, 2.048 MS/s 128 / 15, 2 MS/s 25 / 3).  The prototype is designed at
 * the up-sampled rate Q wide_rate: Lup = P taps_per_phase taps h =
 * firdes_kaiser(Lup, fc, 80 dB), fc = min(0.45 / P, 0.45), gain G = Q 2 fc
 * (taps_per_phase 0: 28 from P / Q = 8, 20 from 4, else 12), and output n is
 * "mix, then interpolate by Q and decimate by P":
 *   y_c[n] = G sum_i h[nP - iQ] x[i] exp(-j 2 pi f_c i / wide_rate),  0 <= nP - iQ < Lup
 * with x and i as above.  Q = 1 is fmx_wb_create's formula term for term, and
 * there fmx_wb_create_rational is fmx_wb_create (the same object, rows bit for
 * bit).  Accepted: Q <= 16, 2 <= P / Q <= 128, and one tile's window of
 * 15 P + a + Lp samples (a = floor((Q - 1) P / Q), Lp = ceil(Lup / Q) rounded
 * up to 32) within 80 KB at 8 bytes per int16 sample, 4 per u8 sample: 10 MS/s
 * to 256 kHz (625 / 16) is refused for FMX_WB_S16 and legal for FMX_WB_U8.
 * Every other ratio is FMX_E_INVALID, the message naming the condition.
 * The object is an fmx_wb object: fmx_wb_destroy, _set_freq, _reset, _process,
 * _process_block, _signal, _set_signal_params and _signal_reset take it.  What
 * differs at Q > 1: n_out (n of fmx_wb_process_block) must be a multiple of Q,
 * else FMX_E_INVALID with a message naming Q -- so every call starts at phase 0
 * and consumes the integer n_out P / Q wide samples; block need not be a
 * multiple of Q; fmx_wb_process_block's rate condition is wide_rate Q ==
 * dsp_rate P (the fast front end still needs n >= 1024 and n % 4 == 0, e.g.
 * n = 4092 at Q = 3); fmx_wb_signal's clip ratios are over the call's n P / Q
 * raw samples; the history holds ceil(Lup / Q) - 1 raw samples.
 * Out of scope: the band scan stays integer (the scan's dsp_rate is free, so
 * a 20 MS/s scan at 200 kHz needs no rational plan; the capture bank takes
 * P / Q through fmx_wb_bank_create_rational below); and
 * there is no int8 format -- a HackRF caller flips bit 7 of each byte and
 * passes FMX_WB_U8.  These symbols arrived without a bump of FMX_ABI_VERSION
 * (see above). */
int fmx_wb_create_rational(void *handle, const fmx_wb_config *cfg, const int *freq_hz, int n_channels, void **wb);
/* host only: P, Q and the taps of the longest phase; FMX_OK or FMX_E_INVALID */
int fmx_wb_ratio(const fmx_wb_config *cfg, int *P, int *Q, int *taps);
/* host only: phase r's weights W_r[j] = G h[Q j + b_r] exp(+j 2 pi f j /
 * wide_rate), r P = Q a_r + b_r, j = 0..L_r-1, as 2 L_r floats (re, im) read
 * back from the kernel's f16 hi + lo tables.  Returns 2 L_r (negative on error). */
int fmx_wb_weights_rational(const fmx_wb_config *cfg, int freq_hz, int phase, float *out, int cap);
/* host only: how a call of n_out outputs (a multiple of Q, <= block) is tiled.
 * out[0..5]: tiles per workgroup, the largest workgroup window in samples, its
 * LDS bytes, workgroups, tiles, Lp; then per tile T = mb Q + r (the 16 outputs
 * (16 mb + col) Q + r) four ints: r, a_r, the offset of column 0's window in
 * its workgroup's LDS image, that workgroup's window in samples.  Column col
 * reads Lp samples from offset + col P on.  Returns the ints needed (nothing
 * is written when cap is less), negative on error. */
int fmx_wb_rational_geometry(const fmx_wb_config *cfg, int n_out, int *out, int cap);

/* ---- capture bank: many wide captures of one format and rate channelized in one call ----
 * A bank holds n_captures captures of one fmx_wb_config (1..1024).  Capture s
 * owns the bank's channels [first_channel[s], first_channel[s + 1]) --
 * first_channel[0] is 0, the table does not decrease, an empty capture is
 * legal -- and is fed row s of d_wide, laid out [n_captures][wide_stride]
 * wide samples (wide_stride >= n * D; samples past n * D of a row are never
 * read; the base needs the element's alignment only, an unaligned base takes
 * element loads and gives identical rows).  Each capture behaves as an fmx_wb
 * object created with the same configuration and the frequencies
 * freq_hz[first_channel[s] .. first_channel[s + 1]) and fed that row: output
 * rows, histories, 64-bit sample counters, the ordering of set_freq on the
 * stage stream, n == 0, the "measured once" rule of the level call and the
 * error codes all carry over, and the rows are bit for bit the single
 * object's.  One kernel launch channelizes every capture (DESIGN.md section
 * 22); the captures' counters and history fill live on the device, so calls,
 * resets and parameter changes stay queued without host synchronisation.
 * Per capture: the reset (dongles restart independently; the other captures'
 * outputs stay bit-identical), the signal parameters (every tuner has its own
 * gain) and the clip ratios of the level records (those of that capture's
 * n * D raw samples).  Smoothers are per channel.
 * fmx_wb_bank_process_block is fmx_wb_process_block with the bank in the
 * channelizer's place: the same conditions (the bank's channel total is the
 * handle's), the same step behind it; fmx_wb_bank_signal is fmx_wb_signal.
 * These symbols arrived without a bump of FMX_ABI_VERSION (see above). */
int fmx_wb_bank_create(void *handle, const fmx_wb_config *cfg, int n_captures,
                       const int *first_channel /* [n_captures + 1] */,
                       const int *freq_hz /* [first_channel[n_captures]] */, void **bank);
int fmx_wb_bank_destroy(void *bank);
int fmx_wb_bank_set_freq(void *bank, int channel, int freq_hz);
/* capture's stream restarts at wide-sample index sample0 (-1: every capture's),
 * ordered on the stage stream between the calls queued before and after it */
int fmx_wb_bank_reset(void *bank, int capture, int64_t sample0);
int fmx_wb_bank_process(void *bank, const void *d_wide, size_t wide_stride /* samples */, int n_out, float *d_out,
                        int out_stride);
int fmx_wb_bank_process_block(void *bank, const void *d_wide, size_t wide_stride, int n, const fmx_block_out *out);
int fmx_wb_bank_signal(void *bank, fmx_signal_level *d_level);
/* capture's set (-1: every capture's), ordered on the stage stream: it holds
 * for the level calls queued after it */
int fmx_wb_bank_set_signal_params(void *bank, int capture, int applied_gain_db, double gain_comp_factor,
                                  double bias_db, double floor_dbfs, double ceil_dbfs);
int fmx_wb_bank_signal_reset(void *bank, int channel /* -1: all */);
/* host only, no GPU needed: the channelizer kernel's work list, one group
 * {capture, first channel, channels 1..16} per 16 channels of a capture and
 * none for an empty capture, as out[G][3].  cap counts groups.  Returns G;
 * FMX_E_INVALID for a bad table or n_captures outside 1..1024, FMX_E_CAPACITY
 * for more than 65 535 groups; -G, with nothing written, when cap < G or out
 * is NULL (n_captures + first_channel[n_captures] / 16 groups always do). */
int fmx_wb_bank_groups(const int *first_channel, int n_captures, int *out, int cap);

/* ---- capture bank at rational rates: wide_rate / dsp_rate = P / Q for every capture ----
 * fmx_wb_bank_create refuses a wide_rate that is no multiple of dsp_rate;
 * fmx_wb_bank_create_rational takes what fmx_wb_create_rational takes (Q <= 16,
 * 2 <= P / Q <= 128, one tile's window within 80 KB for the format) and
 * refuses the rest with FMX_E_INVALID, the message naming this function and
 * the condition; the table rules are fmx_wb_bank_create's.  With Q = 1 it is
 * fmx_wb_bank_create (the same object, rows bit for bit).  The result is a
 * bank: fmx_wb_bank_destroy, _set_freq, _reset, _process, _process_block,
 * _signal, _set_signal_params and _signal_reset take it, and capture s behaves
 * as an fmx_wb_create_rational object with the same configuration and the
 * frequencies freq_hz[first_channel[s] .. first_channel[s + 1]), fed row s:
 * output rows, the history of ceil(Lup / Q) - 1 raw samples, the 64-bit
 * counter, the ordering of set_freq on the stage stream, n == 0 and the
 * "measured once" rule of the level call, bit for bit.  One launch channelizes
 * every capture.  What differs from the integer bank at
 * Q > 1: n_out (n of fmx_wb_bank_process_block) must be a multiple of Q, else
 * FMX_E_INVALID with a message naming the function and Q; block need not be a
 * multiple.  A call consumes n_out P / Q wide samples of every row:
 * wide_stride >= n_out P / Q, else FMX_E_INVALID; samples of a row past that
 * are never read.  fmx_wb_bank_process_block's rate condition is
 * wide_rate Q == dsp_rate P, in 64 bits.  fmx_wb_bank_signal's clip ratios are
 * those of the capture's own n P / Q raw samples.
 * fmx_wb_bank_set_iq_correction and fmx_wb_bank_iq_correction on such a bank
 * return FMX_E_INVALID with a message naming the function, as the single
 * rational object's calls do: the correction at rational rates is out of
 * scope, as are mixed rates within one bank.
 * This symbol arrived without a bump of FMX_ABI_VERSION (see above). */
int fmx_wb_bank_create_rational(void *handle, const fmx_wb_config *cfg, int n_captures,
                                const int *first_channel /* [n_captures + 1] */,
                                const int *freq_hz /* [first_channel[n_captures]] */, void **bank);

/* ---- band scan: the RF level of every scan point from one wide capture ----
 * The reference's scan (main.cpp:1064-1121: retune, three reads,
 * computeSignalLevel of each) on a shared capture.  Point p lies at
 * start_hz + p * step_hz from the capture's centre; wb.dsp_rate is the
 * points' measurement rate (D = wide_rate / dsp_rate, pass band +-0.45
 * dsp_rate) and need not be the handle's.  One call is one read of every
 * point: it consumes n_out * D wide samples and keeps nothing of the signal
 * (the stream may have gaps between reads, as after the reference's retune).
 * With y_p[n] the channelizer's output above for a channel at point p, x
 * indexed from the call's first sample, tpp = L / D:
 *   P_p  = 1 / (n_out - tpp) sum_{n = tpp}^{n_out - 1} |y_p[n]|^2
 *   rms  = sqrt(max(1e-15, 0.5 P_p)),  dbfs = 20 log10(rms + 1e-12)
 * and compensated_dbfs, level120, level120_smoothed (one smoother per point)
 * as computeSignalLevel / smoothSignalLevel (signal_level.cpp:187-214).  The
 * outputs n < tpp, whose windows reach before the call, are left out: no
 * sample before the call's first is needed.  0.5 P is the reference's
 * 0.5 (varI + varQ) WITHOUT its mean removal: the reference removes the mean
 * of one tuned read, which a shared capture has no counterpart of, so a
 * capture's DC offset shows at the points within the pass band of the centre
 * (as in fmx_wb_process's rows).  hard_clip_ratio and near_clip_ratio are
 * those of the call's n_out * D raw samples (clipped samples / samples; u8 by
 * the reference's byte thresholds, signal_level.cpp:172-177, an int16 by its
 * top byte b = (v >> 8) + 128), the same in every record.  n_out <= tpp is
 * FMX_E_INVALID, n_out > block FMX_E_CAPACITY.  Calls are queued on the
 * handle's stream; the object is destroyed before its handle.  Geometry:
 * d_wide needs its element's alignment only, d_level 8 bytes; cells outside
 * [0, n_points) are never written.  The signal parameters default to
 * fmx_set_signal_params' (gain 0, factor 0.5, bias -4, floor -55, ceil -19). */
typedef struct {
  fmx_wb_config wb;
  int start_hz, step_hz, n_points; /* step_hz >= 1, 1 <= n_points <= 8192, every point within +- wide_rate / 2 */
} fmx_wb_scan_config;
int fmx_wb_scan_create(void *handle, const fmx_wb_scan_config *cfg, void **scan);
int fmx_wb_scan_destroy(void *scan);
int fmx_wb_scan_set_signal_params(void *scan, int applied_gain_db, double gain_comp_factor, double bias_db,
                                  double floor_dbfs, double ceil_dbfs);
/* clears the per-point level smoothers (ordered after the calls queued so far) */
int fmx_wb_scan_reset(void *scan);
int fmx_wb_scan_process(void *scan, const void *d_wide, int n_out, fmx_signal_level *d_level);
/* host only: validates the configuration and writes the first min(cap, n_points)
 * point frequencies (freq_hz may be NULL).  Returns n_points (negative on error). */
int fmx_wb_scan_points(const fmx_wb_scan_config *cfg, int *freq_hz, int cap);
/* host only: point p is a peak when dbfs[p] >= min_dbfs, dbfs[p] > dbfs[q] for
 * p - min_spacing <= q < p and dbfs[p] >= dbfs[q] for p < q <= p + min_spacing
 * (a tie goes to the lowest index).  Writes the first min(cap, count) indices,
 * ascending; returns the count (negative on error). */
int fmx_scan_peaks(const double *dbfs, int n, double min_dbfs, int min_spacing, int *idx, int cap);

/* ---- band scan over a capture bank: every capture's scan points in one call ----
 * The scan for the bank's rig (sixteen dongles that together see the band):
 * one call takes d_wide[n_captures][wide_stride] and writes one
 * fmx_signal_level per scan point of every capture; fmx_scan_peaks over a
 * capture's slice of the records gives the frequencies fmx_wb_bank_create
 * takes.
 * Plan and tables: cfg is the scan's plan, as fmx_wb_scan_config.wb is, and
 * the accepted configurations are the same: dsp_rate is the points'
 * measurement rate and need not be the handle's, wide_rate is an integer
 * multiple D of it, 2 <= D <= 128, taps_per_phase and block mean what they
 * mean in fmx_wb_scan_create and block must exceed taps_per_phase.  Capture s
 * owns the points [first_point[s], first_point[s + 1]): first_point[0] is 0,
 * the table does not decrease, an empty capture is legal; 1 <= n_captures <=
 * 1024 and 1 <= first_point[n_captures] <= 8192.  freq_hz[p] is relative to
 * the centre of the point's own capture and lies within +- wide_rate / 2.  The
 * list is free-form, not a start / step grid: dongle centres rarely sit on the
 * station grid.
 * Equivalence: capture s behaves as an fmx_wb_scan object with the same
 * fmx_wb_config and the same frequencies, fed row s of d_wide.  Where its
 * frequencies form a start / step grid its records are bit for bit that
 * object's -- dbfs, compensated_dbfs, level120, level120_smoothed and both clip
 * ratios; where they do not, each record is bit for bit that of a one-point
 * scan object at that frequency (a point's sum order is fixed by D, the padded
 * filter length, the format and n_out alone).
 * A call is one read of every point of every capture.  It consumes n_out * D
 * samples of each row: wide_stride >= n_out * D, else FMX_E_INVALID; samples
 * of a row past n_out * D are never read and nothing of the signal is kept
 * between calls.  The outputs n < tpp are left out, as in the single scan;
 * n_out <= tpp is FMX_E_INVALID, n_out > block FMX_E_CAPACITY.
 * The clip ratios of a record are those of its capture's own n_out * D raw
 * samples.  The signal parameters are per capture (every tuner has its own
 * gain; -1: every capture's) and default to fmx_set_signal_params'; a set is
 * ordered on the stage stream and holds for the process calls queued after it.
 * fmx_wb_bank_scan_reset clears the level smoothers of the capture's points
 * (-1: all), ordered behind the calls queued so far; the other captures'
 * smoothers are untouched.
 * Geometry: the d_wide base needs its element's alignment only (an unaligned
 * base takes element loads and gives identical records), d_level 8 bytes;
 * cells outside [0, first_point[n_captures]) are never written.  Calls are
 * queued on the handle's stream exactly as fmx_wb_scan_process queues them,
 * nothing synchronises with the host, and the object is destroyed before its
 * handle.  One MFMA launch reads every point.
 * The object is a kind of its own: every fmx_wb_bank_scan_* call handed an
 * fmx_wb, bank or scan object returns FMX_E_INVALID with a message naming the
 * function, the six IQ-correction calls (fmx_wb_set_iq_correction,
 * fmx_wb_iq_correction, their _scan_ and their _bank_ forms) refuse a bank scan
 * the same way, and every call with a NULL object returns FMX_E_INVALID
 * without touching a device.
 * DC offset and IQ imbalance are corrected per capture by
 * fmx_wb_bank_scan_set_iq_correction below.
 * Out of scope: rational rates, for the single scan's reason (the scan's dsp_rate is free, so 2.048 MS/s
 * scans at D = 8 or 16); mixed rates or formats within one object.
 * These symbols arrived without a bump of FMX_ABI_VERSION (see above). */
int fmx_wb_bank_scan_create(void *handle, const fmx_wb_config *cfg, int n_captures,
                            const int *first_point /* [n_captures + 1] */,
                            const int *freq_hz /* [first_point[n_captures]] */, void **bscan);
int fmx_wb_bank_scan_destroy(void *bscan);
int fmx_wb_bank_scan_set_signal_params(void *bscan, int capture /* -1: all */, int applied_gain_db,
                                       double gain_comp_factor, double bias_db, double floor_dbfs, double ceil_dbfs);
int fmx_wb_bank_scan_reset(void *bscan, int capture /* -1: all */);
int fmx_wb_bank_scan_process(void *bscan, const void *d_wide, size_t wide_stride /* samples */, int n_out,
                             fmx_signal_level *d_level /* [first_point[n_captures]] */);
/* host only, no GPU: the scan kernel's work list, one entry {capture, first
 * point, points 1..64} per 64 points of a capture and none for an empty
 * capture, as out[G][3].  cap counts entries.  Returns and errors as
 * fmx_wb_bank_groups: G; FMX_E_INVALID for a bad table or n_captures outside
 * 1..1024; -G, with nothing written, when cap < G or out is NULL. */
int fmx_wb_bank_scan_groups(const int *first_point, int n_captures, int *out /* [G][3] */, int cap);

/* ---- DC offset and IQ imbalance of a wide capture ----
 * A zero-IF front end adds a DC offset (a carrier at the capture's centre)
 * and mismatches its I and Q paths in gain and phase (every station at +f
 * mirrored to -f, 25 to 40 dB down).  With x = I + jQ the normalised sample
 * as fmx_wb_process defines it, the corrected sample is
 *   x' = (I - dc_i) + j (gain (Q - dc_q) + cross (I - dc_i))
 * and every output of a call -- rows, and through them fmx_wb_process_block's
 * audio and RDS, fmx_wb_signal's levels, the scan's records -- is the
 * channelizer's formula on x', with the parameters in force for THAT CALL over
 * its whole window, history samples included (the history is kept raw).
 * Before the stream's start x is 0 as without correction, and the correction
 * applies to those zeros too (x' = C(0)).  The clip ratios stay those of the
 * raw samples.  Identity parameters (0, 0, 1, 0) give the uncorrected rows as
 * numbers.
 *   FMX_IQC_OFF    (default) no correction: the object launches the kernels
 *                  it launched before this call existed
 *   FMX_IQC_FIXED  the caller's parameters
 *   FMX_IQC_AUTO   estimated on the GPU from each call's own raw samples (the
 *                  estimate is in force for the call it was taken from), with
 *                  no host synchronisation
 * In OFF and FIXED the rows do not depend on how the stream is cut into
 * calls; in AUTO they DO, because the parameters change with every call.
 * Estimator: with v the raw value (2 b - 255 for u8, v for int16), the sums
 * of I, Q, I^2, Q^2 and IQ over the call's raw samples are formed as 64-bit
 * integers (exact: no summation order matters) and divided by the sample
 * count; each of the five moments is smoothed across calls, m <- m + alpha
 * (m_call - m), the first call after the mode was set initialising m; with
 * mI, mQ and the central moments cII, cQQ, cIQ of m,
 *   v = cQQ - cIQ^2 / cII,  gain = sqrt(cII / v),  cross = -gain cIQ / cII,
 *   dc = (mI, mQ) in units of x
 * (Gram-Schmidt: Q' has I's power and no correlation with it).  If !(cII > 0)
 * or !(v > 1e-9 cQQ), gain = 1 and cross = 0; dc still applies.  alpha must
 * lie in (0, 1] for AUTO; 0 selects 1 / 16 (a design choice -- about 16 calls
 * of memory -- not a measurement).  `fixed` is needed for FIXED and ignored
 * otherwise.  The call is ordered on the stage stream and holds from the next
 * process call on; setting a mode again restarts the estimate; fmx_wb_reset
 * and fmx_wb_set_freq leave it alone (it is a property of the hardware).  The
 * scan treats each read independently as before; only the smoothed moments
 * carry over between reads.  FMX_E_INVALID (message naming the function) for
 * a bad mode, an alpha outside the range, a NULL `fixed` in FIXED, a
 * non-finite field or gain <= 0.  Out of scope, FMX_E_INVALID as well: an
 * object made by fmx_wb_create_rational at Q > 1 (19.2 and 24 MS/s are
 * integer rates); frequency-dependent imbalance is not modelled.  A capture
 * bank takes fmx_wb_bank_set_iq_correction below, and these four calls refuse
 * it.  fmx_wb_iq_correction / fmx_wb_scan_iq_correction wait for the
 * queued calls and return the parameters as of the last one (identity in OFF).
 * These symbols arrived without a bump of FMX_ABI_VERSION (see above). */
typedef struct { double dc_i, dc_q, gain, cross; } fmx_iq_correction; /* units of x */
enum { FMX_IQC_OFF = 0, FMX_IQC_FIXED = 1, FMX_IQC_AUTO = 2 };
int fmx_wb_set_iq_correction(void *wb, int mode, const fmx_iq_correction *fixed, double alpha);
int fmx_wb_iq_correction(void *wb, fmx_iq_correction *h_out);
int fmx_wb_scan_set_iq_correction(void *scan, int mode, const fmx_iq_correction *fixed, double alpha);
int fmx_wb_scan_iq_correction(void *scan, fmx_iq_correction *h_out);
/* host only, no GPU: the estimator of one buffer of n_samples interleaved raw
 * I/Q pairs (format FMX_WB_*), without smoothing: the formula a caller or a
 * test can check against.  FMX_E_INVALID for n_samples <= 0, a NULL argument
 * or an unknown format. */
int fmx_iq_estimate(const void *h_raw, int format, long n_samples, fmx_iq_correction *out);

/* ---- capture bank: DC offset and IQ imbalance per capture ----
 * Every front end behind a bank has its own DC and its own I/Q mismatch, so
 * every capture has its own mode, parameters, alpha and smoothed moments.
 * Capture s behaves as an fmx_wb object with the same configuration and
 * frequencies, fed row s, that was given the same fmx_wb_set_iq_correction
 * calls at the same points of its stream: its rows -- and through them
 * fmx_wb_bank_process_block's outputs and fmx_wb_bank_signal's records -- and
 * the read-back agree bit for bit in every mode, a capture left in OFF beside
 * corrected ones included.  AUTO's sums run over the capture's own n * D raw
 * samples of the call (the padding of a row is never read); the clip ratios
 * stay those of the raw samples; an empty capture is legal in every mode, and
 * in AUTO its read-back follows the estimator on its row.  The set is ordered
 * on the stage stream, holds from the next process call on and restarts that
 * capture's estimate; fmx_wb_bank_reset and fmx_wb_bank_set_freq leave the
 * estimate alone.  A call costs one estimator, one finisher and one
 * channelizer launch whatever the number of captures, with no host
 * synchronisation; a bank whose captures are all in OFF launches what it
 * launched before these calls existed.
 * FMX_E_INVALID (message naming the function) for a capture outside
 * [-1, n_captures), whatever fmx_wb_set_iq_correction refuses, a NULL h_out,
 * capture -1 in the read-back and an object that is not a bank.
 * These symbols arrived without a bump of FMX_ABI_VERSION (see above). */
/* capture's correction (-1: every capture's); modes, parameters, alpha, validation,
 * ordering and the estimator exactly as fmx_wb_set_iq_correction */
int fmx_wb_bank_set_iq_correction(void *bank, int capture, int mode, const fmx_iq_correction *fixed, double alpha);
/* waits for the queued calls; capture's parameters as of the last one (identity in OFF) */
int fmx_wb_bank_iq_correction(void *bank, int capture, fmx_iq_correction *h_out);

/* ---- band scan over a capture bank: DC offset and IQ imbalance per capture ----
 * An uncorrected scan of a zero-IF front end finds a ghost at 0 Hz and one
 * image per strong station, and a bank that tunes itself from the scan spends
 * channels on them; every dongle has its own DC and mismatch, so every capture
 * of a bank scan has its own mode, parameters, alpha and smoothed moments.
 * Capture s behaves as an fmx_wb_scan object with the same fmx_wb_config and
 * frequencies, fed row s, that was given the same
 * fmx_wb_scan_set_iq_correction calls at the same points of its stream: the
 * records (all six fields) and the read-back agree bit for bit in every mode,
 * a capture left in OFF beside corrected ones included; off a start / step
 * grid each record is bit for bit a one-point scan object's at that frequency
 * set the same way.  AUTO's sums run over the capture's own n_out * D raw
 * samples of the read (the padding of a row is never read) and each read is
 * otherwise independent: only the smoothed moments carry over.  The clip
 * ratios stay those of the raw samples; an empty capture is legal in every
 * mode, and in AUTO its read-back follows the estimator on its row.  The set
 * is ordered on the stage stream behind the reads queued so far, holds from
 * the next read on and restarts that capture's estimate;
 * fmx_wb_bank_scan_reset and fmx_wb_bank_scan_set_signal_params leave the
 * estimate alone.  A read costs at most five launches whatever the number of
 * captures, with no host synchronisation; an object whose captures are all in
 * OFF allocates nothing and launches what it launched before these calls
 * existed.
 * FMX_E_INVALID (message naming the function) for a capture outside
 * [-1, n_captures), whatever fmx_wb_set_iq_correction refuses, a NULL h_out,
 * capture -1 in the read-back and an object that is not a bank scan; a NULL
 * object returns FMX_E_INVALID without touching a device.
 * These symbols arrived without a bump of FMX_ABI_VERSION (see above). */
/* capture's correction (-1: every capture's) */
int fmx_wb_bank_scan_set_iq_correction(void *bscan, int capture, int mode,
                                       const fmx_iq_correction *fixed, double alpha);
/* waits for the queued calls; capture's parameters as of the last read (identity in OFF) */
int fmx_wb_bank_scan_iq_correction(void *bscan, int capture, fmx_iq_correction *h_out);

/* ---- device memory helpers (so C/FFI callers need no HIP headers) ---- */
int fmx_malloc(void *handle, void **d_ptr, size_t bytes);
int fmx_free(void *handle, void *d_ptr);
int fmx_memcpy_h2d(void *handle, void *d_dst, const void *h_src, size_t bytes);
int fmx_memcpy_d2h(void *handle, void *h_dst, const void *d_src, size_t bytes);
int fmx_memset(void *handle, void *d_ptr, int value, size_t bytes);

/* ---- HIP-event timing of the hot kernels (bench roofline support) ----
 * When enabled, every launch of each kernel is bracketed by events on the
 * stream it runs on; fmx_kernel_times returns the summed milliseconds and
 * launch counts per kernel id since the last reset. */
enum {
  FMX_K_FRONTEND = 0, /* decimate + DC + IQ FIR + AGC + discriminator (+ pilot BPF, + RDS
                         resample when process_block does not run them as kernels of their own);
                         fmx_wb_process_block's k_fecf counts here (k_wb is not timed)           */
  FMX_K_STEREO = 1,   /* pilot PLL + blend + L-R matrix (one lane per channel)                 */
  FMX_K_AUDIO = 2,    /* L/R 15 kHz FIRs + 32 kHz resampler + de-emphasis + DC + clamp         */
  FMX_K_RDS = 3,      /* 57 kHz BPSK demod + symsync (+ biphase + block sync in fmx_rds)        */
  FMX_K_RS = 4,       /* the 240k -> 171k RDS resampler when process_block runs it as its own
                         kernel (k_rs, on the RDS stream ahead of k_rds)                        */
  FMX_K_PILOT = 5,    /* the 19 kHz pilot BPF when process_block runs it as its own kernel
                         (k_pilot, on the front-end stream after k_fe8)                         */
  FMX_K_FRONTEND_GENERIC = 6, /* process_block's front end when it runs as the generic k_frontend
                         (calls of n < 1024 samples, unaligned IQ rows) instead of k_fe8 (of k_fecf in
                         fmx_wb_process_block); FMX_K_FRONTEND then counts k_fe8 / k_fecf launches only */
  FMX_K_BITS = 7,     /* process_block's RDS bit decoders (biphase, delta, block sync, groups:
                         k_bits, on the audio stream ahead of k_audio)                          */
  FMX_K_COUNT = 8
};
/* enable: 0 off, 1 every step's launches, N > 1 the launches of every N-th
 * step only (a sample: fewer event packets on the streams in the timed region) */
int fmx_timing_enable(void *handle, int enable);
/* diagnostic: frontend per-stage clocks, 8 values (diagnostics library
 * libfmx_diag.so, handle created with FMX_STAMPS=1 in the environment;
 * FMX_E_INVALID otherwise -- the product libfmx.so reads no environment) */
int fmx_debug_stamps(void *handle, unsigned long long *out, int n);
int fmx_kernel_times(void *handle, double *ms, int *launches, int n);
/* host-side waits of fmx_process_block since the last call (then reset):
 * out[0] waits on a pinned schedule image's last reader, out[1] those that
 * found it still pending (the host blocked), out[2] milliseconds blocked.
 * Fills at most n (<= 3) entries. */
int fmx_host_stats(void *handle, double *out, int n);
/* diagnostics (round 6).  A call of >= 256 RDS-rate samples leaves the RDS
 * FIR's 256-sample ring (the mixed samples a reset's decimation-phase
 * rebuild reads) to per-round NCO checkpoints instead of writing it; it is
 * refilled, bit-identically, when needed.  fmx_diag_set(FMX_DIAG_RDS_RING_ALWAYS,
 * 1) makes k_rds write it every call (round 5's behaviour; the test arm);
 * fmx_diag_rds_ring copies the channel's ring, oldest sample first, as 256
 * (re, im) float pairs to host memory (synchronous; refills it first). */
/* fmx_diag_set(FMX_DIAG_FE_GENERIC, 1) makes fmx_wb_process_block take the
 * generic front end (k_frontend on the rows) for every n: the A/B arm of
 * tools/bench_band_receiver.py and a test arm; no effect on any other call. */
enum { FMX_DIAG_RDS_RING_ALWAYS = 1, FMX_DIAG_FE_GENERIC = 2 };
int fmx_diag_set(void *handle, int what, int value);
/* host only: the dynamic LDS bytes a front-end launch takes on top of the
 * kernel's static LDS (which the code object records): which 0 = k_fe8 at
 * M = 10 with k_rs behind it (fmx_process_block at 2.4 MS/s), 1 = k_fecf.
 * tests/test_fecf_resources.py compares the two kernels' totals. */
int fmx_diag_lds_bytes(int which);
int fmx_diag_rds_ring(void *handle, int channel, float *out);

/* ---- synthetic IQ (bench / tests input; see fmx_synth.h) ---- */
typedef struct {
  int iq_rate;
  int kind;        /* 0 mono two-tone, 1 stereo, 2 stereo + RDS             */
  float amplitude; /* 0.8                                                   */
  float noise_std; /* AWGN per component (0 = none)                         */
  uint32_t seed_base;
  int max_offset_hz;
  float rds_level; /* 0.05                                                  */
  int n_bits;      /* RDS bit-table length per channel                      */
  float level_spread_db; /* per-channel carrier level: amplitude * 10^(-u d / 20),
                            u in (0, 1] from the channel seed, d this value
                            (0 = every channel at `amplitude`)              */
} fmx_synth_config;
/* RDS test pattern: encoded (differential) bits [n_ch][n_bits] and, if
 * h_groups != NULL, the transmitted groups [n_ch][n_bits/104][4]. */
int fmx_synth_rds_bits(const fmx_synth_config *cfg, uint32_t ch0, int n_ch, uint8_t *h_bits,
                       uint16_t *h_groups);
/* host generation: h_out [n_ch][2*n_samples]; h_bits [n_ch][n_bits] or NULL */
int fmx_synth_host(const fmx_synth_config *cfg, uint32_t ch0, int n_ch, int64_t sample0, int n_samples,
                   const uint8_t *h_bits, uint8_t *h_out, size_t out_stride, int threads);
/* device generation on the handle's stream: d_out [n_ch][out_stride] */
int fmx_synth_device(void *handle, const fmx_synth_config *cfg, uint32_t ch0, int n_ch, int64_t sample0,
                     int n_samples, const uint8_t *d_bits, uint8_t *d_out, size_t out_stride);

/* ---- synthetic FM band: wide captures of many stations (fmx_synth_band.h) ----
 * A band is n_captures captures of one rate wide_rate (any integer 480 000 ..
 * 30 720 000 Hz) and one format (FMX_WB_U8 / FMX_WB_S16).  Capture s holds
 * the stations [first_station[s], first_station[s + 1]): the table starts at 0
 * and does not decrease (fmx_wb_bank_create's rules), an empty capture is
 * legal (noise only); 1 <= n_captures <= 1024, 0 <= stations <= 8192 in all.
 * Station g (global index) is an FM carrier of `amplitude` (finite, >= 0) at
 * freq_hz from the capture's centre, |freq_hz| + max_offset_hz <= wide_rate / 2,
 * with the content of channel ch0 + g of the generator above:
 * fmx_synth_band_content writes that generator's config (iq_rate = wide_rate,
 * amplitude 1, no noise, no level spread), and RDS bit row g is row g of
 * fmx_synth_rds_bits(content, ch0, stations) (kind 2 needs 104 <= n_bits <= 2^24
 * and the table).  The phase of every tone is a closed form of the absolute
 * sample index i (0 <= sample0, sample0 + n_samples <= 2^40) through exact
 * integer residues, and phase and station sum are in double, so a sample
 * depends on (config, tables, capture, i) alone: the bytes do not depend on
 * how a stream is cut into calls, on the grid, or on the run.  noise_std > 0
 * adds white Gaussian noise per component, seeded by seed_base and the
 * capture's index.  The front end of capture s (NULL table: the identity
 * 0, 0, 1, 0; finite, q_gain > 0) then gives I' = I + dc_i and
 * Q' = q_gain Q + q_cross I + dc_q, which fmx_wb_set_iq_correction(FIXED,
 * {dc_i, dc_q, 1 / q_gain, -q_cross / q_gain}) inverts exactly.  Quantised
 * with ties to even: u8 clamp(rint(127.5 v + 127.5), 0, 255), int16
 * clamp(rint(32768 v), -32768, 32767), interleaved I, Q.
 *
 * Output is [n_captures][wide_stride] samples, wide_stride >= n_samples; cells
 * past n_samples of a row are never written.  fmx_synth_band_host writes host
 * memory on `threads` threads and needs no GPU.  fmx_synth_band_create
 * validates, derives every station once and puts the tables into device
 * memory; fmx_synth_band_generate is one launch queued on the handle's stage
 * stream (the one fmx_wb_process is queued on), with no host synchronisation
 * and no host-to-device copy, so a following channelizer call on the same
 * handle needs no sync.  d_out needs the element's alignment only (2 bytes for
 * int16, 1 for u8); an unaligned base takes narrower stores and gives
 * identical bytes.  n_samples == 0 does nothing.
 *
 * Every refusal is FMX_E_INVALID with a message naming the function and the
 * condition: in fmx_last_error of the handle for create / generate / destroy,
 * and in fmx_synth_band_error (the calling thread's last refusal) for the two
 * host calls.  A NULL object or handle returns it without touching a device.
 * The object is a kind of its own: every other fmx_* call that takes an
 * object refuses it, and these calls refuse every other object.
 * host and device agree to 1 LSB (they differ by the ulps of sin / cos and of
 * the noise's float functions, which can only move a value across a rounding
 * tie).  These symbols arrived without a bump of FMX_ABI_VERSION (see above). */
typedef struct {
  int wide_rate, format, kind; /* kind: 0 mono two-tone, 1 stereo, 2 stereo + RDS */
  uint32_t seed_base;
  int max_offset_hz;
  float rds_level;
  int n_bits;
  float noise_std;
} fmx_synth_band_config;
typedef struct {
  int freq_hz;
  float amplitude;
} fmx_synth_station;
typedef struct {
  double dc_i, dc_q, q_gain, q_cross;
} fmx_synth_frontend;
int fmx_synth_band_content(const fmx_synth_band_config *cfg, fmx_synth_config *out); /* host only */
int fmx_synth_band_tile(void); /* host only: samples per workgroup of the kernel */
const char *fmx_synth_band_error(void); /* host only: the calling thread's last refusal by the two host calls */
int fmx_synth_band_host(const fmx_synth_band_config *cfg, uint32_t ch0, int n_captures, const int *first_station,
                        const fmx_synth_station *stations, const fmx_synth_frontend *frontends /* or NULL */,
                        int64_t sample0, int n_samples, const uint8_t *h_bits /* [stations][n_bits] or NULL */,
                        void *h_out, size_t wide_stride /* samples */, int threads);
int fmx_synth_band_create(void *handle, const fmx_synth_band_config *cfg, uint32_t ch0, int n_captures,
                          const int *first_station, const fmx_synth_station *stations,
                          const fmx_synth_frontend *frontends /* or NULL */, const uint8_t *h_bits, void **band);
int fmx_synth_band_generate(void *band, int64_t sample0, int n_samples, void *d_out, size_t wide_stride);
int fmx_synth_band_destroy(void *band);

/* ---- diagnostics (host only, no GPU needed) ---- */
/* Filter taps the handle would use: which = 0 decimator, 1 IQ FIR,
 * 2 pilot BPF, 3 L/R LPF, 4 audio resampler prototype, 5 RDS resampler
 * prototype, 6 RDS 2.4 kHz LPF, 7 symsync RRC, 8 symsync derivative;
 * the MFMA tables read back as float taps:
 * 10 pilot BPF fragments, 11 IQ FIR fragments, 12 L/R LPF fragments (k_audio),
 * 13 decimator A fragments (row 0), 9 the same fragments' rows 0..15.
 * Returns the tap count (negative on error). */
int fmx_design_taps(const fmx_config *cfg, int which, float *out, int cap);
/* liquid resamp_rrrf output schedule for rate 1/del over n_in inputs from
 * the reset state: packed = i | (branch << 16) | (boundary << 24). */
int fmx_resamp_schedule(float del, int n_in, int *packed, float *mu, int cap);

/* ---- host-side consumers of the GPU outputs ----
 * The reference's wire and file formats, fed from fmx_process_block's
 * outputs (copied to the host).  No GPU needed. */
/* Per-channel PI debounce state of the XDR server (xdr_server.h:151-156). */
typedef struct {
  uint16_t pi_buf[64];
  uint8_t pi_err[8];
  uint8_t fill, pos, last_state, pad;
  uint16_t last_value, pad2;
} fmx_xdr_pi_state;
/* XDRServer ctor / setFrequencyState reset (xdr_server.cpp:261-266, 465-470). */
void fmx_xdr_pi_reset(fmx_xdr_pi_state *s);
/* XDRServer::updateRDS for n groups of one channel (xdr_server.cpp:189-213,
 * 403-457): writes the queued lines ("P%04X" + '?' per block-A error level,
 * "R%04X%04X%04X%02X"), each ending in '\n', NUL-terminated.  Returns the bytes
 * written, or -(bytes needed + 1) when cap is too small (then nothing is
 * written and the state is unchanged). */
int fmx_xdr_rds_lines(fmx_xdr_pi_state *s, const fmx_rds_group *groups, int n, char *out, int cap);
/* Scan line of main.cpp:1069-1113 as XDRServer::pushScanLine queues it
 * ("U" + "f=level,..." with level = (float)(level_sum / reads) at one
 * decimal; points with reads == 0 skipped; empty when no point).  level_sum
 * holds summed fmx_signal_level.level120 values.  Same return convention. */
int fmx_xdr_scan_line(const int *freq_khz, const double *level_sum, const int *reads, int n, char *out, int cap);
/* XDRServer::updateSignal + buildSignalLine (xdr_server.cpp:368-397): the
 * level line of one station, "S" mode "%.1f" "," cci "," aci "\n" of
 * deci / 10.0 with deci = (int)round(clamp(level, 0, 120) * 10) in float (a
 * NaN level counts as 0); mode is m (mono), s (stereo), M (forced mono) or S
 * (forced mono while stereo is detected).  level: a record's
 * level120_smoothed; stereo: d_stereo_indicator; the reference sends -1 for
 * cci and aci.  NUL-terminated; fmx_xdr_rds_lines' return convention. */
int fmx_xdr_signal_line(float level, int stereo, int forced_mono, int cci, int aci, char *out, int cap);
/* AudioOutput::writeWAVHeader (audio_output.cpp:1346-1377): 44 bytes for
 * data_bytes of S16LE 32 kHz stereo.  Returns 44. */
int fmx_wav_header(uint32_t data_bytes, uint8_t *out44);
/* AudioOutput::write volume ramp (:1432-1467) + writeWAVData (:1379-1398):
 * n stereo frames -> 2n interleaved int16; *volume_scale carries the sink's
 * m_currentVolumeScale (initially 0.85).  Returns n. */
int fmx_pcm_to_s16(const float *left, const float *right, int n, int volume_percent, float *volume_scale,
                   int16_t *out);
/* writeIqCapture (main.cpp:742-747): n raw I/Q byte pairs to path
 * (append != 0 appends).  fmx_iq_replay reads n pairs at a sample offset
 * back (returns the pairs read). */
int fmx_iq_capture(const char *path, const uint8_t *iq, int n_samples, int append);
int fmx_iq_replay(const char *path, long long sample_offset, int n_samples, uint8_t *out);

#ifdef __cplusplus
}
#endif
#endif
