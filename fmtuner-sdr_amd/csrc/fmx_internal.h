// fmx_internal.h -- host-side internals of libfmx (not part of the ABI).
#ifndef FMX_INTERNAL_H
#define FMX_INTERNAL_H

#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/fmx.h"
#include "fmx_design.h"
#include "fmx_iqc.h"

namespace fmx {

// ---- design (fmx_design.cpp) ----
struct DesignExtras {
  std::vector<float> proto_af, proto_rds, rrc, rrc_d;
};
void firdes_kaiser(unsigned n, float fc, float As, float mu, float *h);
uint32_t nco_constrain(float theta);
int design_build(const fmx_config &cfg, FmxDesign *d, DesignExtras *ex, std::string *err);
int bandwidth_select(int bw_hz, int w0);
int tef_bandwidth_hz(int mode);

// liquid resamp_rrrf timing state (float tau, interp/boundary), simulated on
// the host because it does not depend on the signal.
struct ResampTiming {
  float tau = 0.0f, bf = 0.0f, mu = 0.0f, del = 1.0f;
  int b = 0, state = 0;
};
void timing_reset(ResampTiming &t);
int timing_run(ResampTiming &t, int n_in, FmxSched *out, int cap);
bool timing_equal(const ResampTiming &a, const ResampTiming &b);

// ---- kernel argument blocks (fmx_kernels.hip) ----
enum FeInMode { FE_IN_U8_DECIM = 0, FE_IN_CF = 1, FE_IN_U8_DIRECT = 2, FE_IN_MPX = 3 };

// process_block runs the 19 kHz pilot BPF of a k_fe8 step as its own kernel
// (k_pilot, after k_fe8 on the front-end stream); k_fe8 then writes only the
// MPX and its history rows (FeArgs::st_hist_out)
struct FeArgs {
  const FmxDesign *des;
  int des_fs;        // DSP rate (host copy of des->fs, for the launcher)
  const FmxChanParam *par;
  int C, n, in_mode;
  // inputs
  const uint8_t *iq;
  size_t iq_stride;
  const float *in_f; // complex (FE_IN_CF) or mpx (FE_IN_MPX)
  int in_stride;
  // outputs
  float *bb_out;     // complex decimator output (fmx_decimate), may be null
  int bb_stride;
  float *mpx_out;
  int mpx_stride;
  float *pilot_out;  // null = no pilot BPF (k_frontend only: k_fe8 has none, k_pilot follows it)
  int pilot_stride;
  int st_hist_out;   // write the stereo history rows (st_hist_wr) even without the pilot BPF
  float *rds_out;    // null = no RDS resampling
  int rds_stride;
  int *rds_count;    // [C]
  float *clip_out;   // [C]
  unsigned long long *sig_sums; // [C][6] RF-level byte sums (u8 inputs; k_audio evaluates them), may be null
  unsigned long long *dbg;    // [8] stage clocks (diagnostics build, FMX_STAMPS), may be null
  // stages
  int do_demod;      // run DC + IQ FIR + AGC + discriminator
  // state
  uint8_t *dec_hist;
  int *dec_valid;
  float *dc_v;       // [C][2]
  float2_t *iq_hist; // [C][FMX_IQ_MAXLEN-1]
  float *agc;        // [C][2]
  float *fd_prev;    // [C][2]
  const float *st_hist_rd; // [C][FMX_HIST] stereo MPX history before this call
  float *st_hist_wr;       // [C][FMX_HIST] history after this call (another buffer)
  float *rds_hist;   // [C][32]
  // schedules
  const FmxSched *rds_sched; // [groups][rds_sched_stride]
  const int *rds_sched_n;    // [groups]
  const int *rds_group;      // [C]
  int rds_sched_stride;
  // k_fe8 leaves the RDS resampler to k_rs: it writes the previous call's
  // last 32 MPX samples here ([C][32]) instead of resampling (may be null)
  float *rds_win_out;
  // the NEXT step's RDS schedule slot, copied by the first workgroups of this
  // launch from the mapped pinned image (fmx_capi.cpp process_block): no copy
  // kernel on the front end's stream between two front ends; n16 = 0: none
  const void *next_sched_src;
  void *next_sched_dst;
  unsigned next_sched_n16;
};

struct PllArgs {
  const FmxDesign *des;
  const FmxChanParam *par;
  int C, n;
  const float *pilot;
  int pilot_stride;
  const float *mpx;
  int mpx_stride;
  const float *st_hist_rd; // [C][FMX_HIST] history the frontend of this call read
  float *lraw, *rraw;
  int lr_stride;
  int lr_tiled;            // raw L/R in pair tiles (lr_tile_idx, fmx_kernels.hip), else [C][lr_stride]
  FmxStereoState *st;
  int *stereo_out, *pilot_tenths_out;
  int *indicator_out;      // [C] XDR stereo indicator (main.cpp:1298-1300), may be null
  unsigned long long *dbg; // [16] per-wave work / barrier clocks (diagnostic, FMX_STAMPS=1), may be null
  int n_cu;                // CUs of the handle's device (launch_pll's workgroup shape)
};

struct AudioArgs {
  const FmxDesign *des;
  const FmxChanParam *par;
  int C, n, mode; // mode 0 stereo (LR FIR + AF), 1 AF only, 2 mono (FMDemod), 3 mono pipeline
  int cap;
  const float *in_l, *in_r;
  int in_stride;
  int in_tiled;    // in_l / in_r in pair tiles (raw L/R from k_pll), else [C][in_stride]
  float *out_l, *out_r;
  int out_stride;
  int *out_count;
  float *lr_hist;  // [C][2][FMX_LR_LEN-1]
  float *af_win;   // [C][2][32]
  float *af_iir;   // [C][4]
  float *mono_win; // [C][32]
  float *mono_iir; // [C][2]
  float *lr_out_l, *lr_out_r; // optional filtered L/R at dsp rate (fmx_stereo)
  int lr_out_stride;
  const FmxSched *sched; // [groups][sched_stride]
  const int *sched_n;
  const int *group; // [C]
  int sched_stride;
  int clamp;
  int *mute;       // [C][2] retune fade/mute {remaining, total} (main.cpp:1310-1337), may be null
  int mute_fade;   // OUTPUT_RATE / 200
  // RF level of the step (computeSignalLevel / smoothSignalLevel) from the
  // front end's byte sums, when sig_out is set
  fmx_signal_level *sig_out;          // [C]
  const unsigned long long *sig_sums; // [C][6]
  long sig_samples;                   // IQ samples behind the sums
  const double *sig_par;              // [C][4] gain*factor, bias, floor, ceil
  float *sig_smooth;                  // [C][2] smoother value, initialized flag
};

struct RdsArgs {
  const FmxDesign *des;
  int C;
  const float *in; // 171 kHz samples
  int in_stride;
  const int *in_count; // [C]
  FmxRdsState *st;
  float *ring; // [C][FMX_RDS_RING][2]
  // the previous RDS call's input rows (its slot; same stride), for the ring
  // refill of a short call after a long one (FmxRdsState::ring_ok)
  const float *in_prev;
  int ring_always; // write the ring every call (FMX_RDS_RING_ALWAYS=1: the round-5 behaviour, the A/B and test arm)
  fmx_rds_group *groups;
  int groups_stride;
  int *group_count;
  uint32_t block_index;
  unsigned long long *dbg; // [8] stage clocks (diagnostic, FMX_STAMPS=1), may be null
  // the call's PSK2 symbols, k_rds -> k_bits (the bit decoders)
  float *sym;         // [C][sym_stride] real parts
  int sym_stride;
  int *sym_count;     // [C]
  float *sym_last_im; // [C] the last symbol's imaginary part (BiphaseDecoder's prev)
};

// k_pilot: the 19 kHz pilot BPF of a process_block step (after k_fe8)
struct PilotArgs {
  const FmxDesign *des;
  int des_pilot_len;        // host copy of des->pilot_len (launcher check)
  int C, n;
  const float *mpx;         // this step's MPX rows (the front end's output)
  int mpx_stride;
  const float *st_hist_rd;  // [C][FMX_HIST] the previous call's last MPX samples
  float *out;               // pilot rows (k_pll's input)
  int out_stride;
  int vec;                  // set by the launcher: 16-B rows
};

// k_rs: the 240k -> 171k RDS resampler of a process_block step (liquid
// resamp_rrrf, host timing schedule), 16 channels per workgroup on FP32 MFMA
struct RsArgs {
  const FmxDesign *des;
  int C, n;
  const float *mpx;     // this step's MPX rows (the front end's output)
  int mpx_stride;
  const float *win;     // [C][32] the previous call's last 32 MPX samples
  const FmxSched *sched; // [groups][sched_stride]
  const int *sched_n;   // [groups]
  const int *group;     // [C]
  int sched_stride;
  float *out;           // RDS-rate rows
  int out_stride;
  int parts;            // workgroups per gpw channel groups (each a contiguous run of output tiles)
  int gpw;              // 16-channel groups per workgroup (even): a tile's band matrix is built once for them
};

// launchers (fmx_kernels.hip); stream is a hipStream_t
// vec: the caller guarantees every channel's decimator history is full
// (dec_valid == L-1) -- only k_frontend's VEC form needs it; k_fe8 takes cold
// and warm channels alike; 16-B row alignment is checked here.
// Events bound to the NEXT main-kernel launch of this thread (k_fe8 /
// k_frontend, k_pll, k_audio, k_rs, k_rds) through hipExtLaunchKernel: `stop`
// completes with the kernel and `start` (timing) takes its start time -- no
// marker packets between two kernels of a stream.  Consumed by that launch.
void set_launch_events(void *start, void *stop);
int launch_frontend_m(const FeArgs &a, int M, int tpp, void *stream, bool vec = false);
// whether launch_frontend_m would run k_fe8 for these arguments
bool frontend_is_fe8(const FeArgs &a, int M, int tpp);
// k_fecf (fmx_fecf.inc): the fast front end on complex-float rows at the DSP
// rate (fmx_wb_process_block); fecf_ok: whether it takes these arguments --
// every other FE_IN_CF call runs k_frontend (launch_frontend_m(a, 1, 1, ...))
bool fecf_ok(const FeArgs &a);
int launch_fecf(const FeArgs &a, void *stream);
int fe_launch_lds_bytes(int which); // fmx_diag_lds_bytes
int launch_pll(const PllArgs &a, void *stream);
int launch_pilot(const PilotArgs &a, void *stream);
int launch_audio(const AudioArgs &a, void *stream);
int launch_rds(const RdsArgs &a, void *stream);      // k_rds then k_bits (one timer over both)
struct ResetArgs;
int launch_rds_sym(const RdsArgs &a, void *stream);  // k_rds alone: the call's symbols
int launch_ring_fill(const ResetArgs &a, void *stream); // every channel's RDS ring refilled where ring_ok = 0
int launch_bits(const RdsArgs &a, void *stream);     // k_bits alone: the bit decoders
// k_rs launch geometry (fmx_capi.cpp): FMX_RS_G 16-channel groups per
// workgroup, and per workgroup at most this many steps -- a step is one
// 16-output tile of one group -- by channel count
#ifndef FMX_RS_G
#define FMX_RS_G 4
#endif
#ifndef FMX_RS_BIG
#define FMX_RS_BIG 92   // from 4096 channels on
#endif
#ifndef FMX_RS_TMAX
#define FMX_RS_TMAX 12  // from 2048 channels
#endif
#ifndef FMX_RS_SMALL
#define FMX_RS_SMALL 6  // below 2048 channels
#endif
int launch_rs(const RsArgs &a, void *stream);
int launch_synth(const fmx_synth_config &cfg, uint32_t ch0, int n_ch, int64_t sample0, int n_samples,
                 const uint8_t *bits, uint8_t *out, size_t out_stride, void *stream);
struct ResetArgs {
  const FmxDesign *des;
  int C;
  const int *mask; // [C] bitmask of parts to reset
  FmxStereoState *st;
  FmxRdsState *rds;
  float *ring;
  uint8_t *dec_hist;
  int *dec_valid;
  float *dc_v;
  float2_t *iq_hist;
  float *agc;
  float *fd_prev;
  float *st_hist; // [FMX_ST_BUFS][C][FMX_HIST]
  float *lr_hist, *af_win, *af_iir, *mono_win, *mono_iir;
  float *rds_hist;
  int *mute;      // [C][2]
  const float *rds_prev; // the last RDS call's input rows (the ring refill before a rebuild)
  int rds_stride;
};
// per-step intermediates (MPX, pilot, RDS-rate, raw L/R): front end k runs
// while stereo/RDS/audio of steps k-1, k-2 drain
#ifndef FMX_NBUF
#define FMX_NBUF 3
#endif
#define FMX_ST_BUFS (FMX_NBUF + 1) // rotating stereo-history buffers
enum ResetParts {
  RS_DECIM = 1,    // ComplexDecimator::reset
  RS_DEMOD = 2,    // FMDemod::reset (DC, IQ FIR, discriminator, mono chain)
  RS_AGC = 4,      // AGC re-init (FMDemod::reset when ready, setDspAgcMode)
  RS_STEREO = 8,   // StereoDecoder::reset
  RS_AF = 16,      // AFPostProcessor::reset
  RS_RDS = 32,     // RDSDecoder::reset (symsync + NCO + block stream)
  RS_IQFIR = 64,   // IQ FIR re-created (setBandwidthHz)
  RS_DEEMPH = 128, // de-emphasis IIRs re-created (setDeemphasis)
  RS_CREATE = 256, // object construction (everything, incl. RDS resampler/AGC)
  RS_MUTE = 512,   // retune fade/mute start; mute length in bits 16..31 (main.cpp:1034-1035)
  RS_FREQDEM = 1024 // discriminator re-created (FMDemod::setDeviation)
};
// the stream-local parts of a channel reset (reset_channel, fmx_kernels.hip):
// each part's state is read / written by the kernels of one process_block
// stream only
enum ResetStreamPart {
  RSP_FRONT = 1,  // sA: decimator / IQ FIR / DC / AGC / discriminator state, stereo history rows
  RSP_STEREO = 2, // sB: FmxStereoState (k_pll)
  RSP_RDS = 4,    // sC: FmxRdsState up to the bit decoders, mix-down ring (k_rds)
  RSP_AUDIO = 8,  // sD: L/R FIR history, AF / mono resampler + IIRs, retune mute (k_audio)
  RSP_BITS = 16,  // sD: FmxRdsState's bit decoders, bi_prev_re on (k_bits)
  RSP_ALL = 31
};
#define FMX_RESET_LIST 64 // channels per k_reset_list launch (a kernel argument, no upload)
struct ResetList {
  int n;
  int ch[FMX_RESET_LIST];
  int m[FMX_RESET_LIST];
};
int launch_reset(const ResetArgs &a, void *stream);
int launch_reset_list(const ResetArgs &a, const ResetList &L, int parts, int st_buf, void *stream);
// ---- wideband channelizer (fmx_wb_design.cpp, fmx_wb.inc) ----
// Geometry and taps of one fmx_wb_config; the f16 weight rows are built per
// channel frequency from it.
struct WbPlan {
  int D = 0, tpp = 0, L = 0, Lp = 0; // Lp: L rounded up to the MFMA's K = 32
  int fs = 0, format = 0, block = 0; // wide rate, FMX_WB_*, outputs per call at most
  int sexp = 0;                      // weights enter the tables as W * 2^sexp
  float fc = 0.0f;
  std::vector<double> g;             // 2 fc h[k], k = 0..L-1
};
int wb_plan(const fmx_wb_config &cfg, WbPlan *p, std::string *err);
bool wb_freq_ok(const WbPlan &p, int freq_hz);
// one channel's rows [4][Lp] (re hi, re lo, im hi, im lo): entry kk holds tap
// k = Lp - 1 - kk (zero for k >= L) as f16 bits
void wb_weight_rows(const WbPlan &p, int freq_hz, uint16_t *rows);
// W[k] (re, im) read back from such rows
void wb_rows_to_taps(const WbPlan &p, const uint16_t *rows, float *out);
uint32_t wb_freq_mod(const WbPlan &p, int freq_hz); // f mod Fs in [0, Fs)
// wb_plan of cfg.wb plus the scan's conditions on its points
int wb_scan_plan(const fmx_wb_scan_config &cfg, WbPlan *p, std::string *err);

struct WbArgs {
  const void *in;       // n_out * D wide samples, interleaved I/Q
  int s16;              // int16 pairs, else u8 pairs
  int in_al;            // a whole sample (2 or 4 bytes) may be loaded at once
  int D, L, Lp, n_out, C;
  const uint16_t *w;    // [C][4][Lp] weight rows
  const uint32_t *fpos; // [C] f mod Fs
  const void *hist;     // the last L - 1 raw samples before this call
  void *hist_out;       // the same after it (another buffer)
  int valid;            // samples of hist that exist (since the last reset)
  uint32_t fs;          // wide rate
  uint32_t base_mod;    // the call's first sample index mod Fs
  double inv_fs;
  float scale;          // accumulator -> output
  float *out;
  int out_stride;
  int nt;               // 16-output tiles per workgroup (set by the launcher)
};
int launch_wb(const WbArgs &a, void *stream);

// ---- rational-rate channelizer (fmx_wb_design.cpp, fmx_wb_rational.inc) ----
// wide_rate / dsp_rate = P / Q in lowest terms: Q integer channelizers of
// decimation P whose outputs interleave.  Output n = Q m + r ends at wide
// sample i0 = m P + a_r and uses the taps h[Q j + b_r], r P = Q a_r + b_r.
#define FMX_WBR_QMAX 16
constexpr int kWbLdsMax = 80 * 1024; // WB_LDS_MAX (fmx_wb_core.inc)
constexpr int kWbNtMax = 16;         // WB_NT_MAX
struct WbrPlan {
  int P = 0, Q = 0, tpp = 0, Lup = 0, Lp = 0; // Lp: the largest L_r rounded up to the MFMA's K = 32
  int Lh = 0;                        // the largest L_r: the history holds Lh - 1 raw samples
  int fs = 0, format = 0, block = 0;
  int sexp = 0;                      // one scale for every phase's tables
  float fc = 0.0f;
  int a[FMX_WBR_QMAX] = {}, b[FMX_WBR_QMAX] = {}, Lr[FMX_WBR_QMAX] = {};
  std::vector<double> g;             // Q 2 fc h[k], k = 0..Lup-1, at the up-sampled rate Q Fs
};
// taps = false: the geometry alone (g and sexp stay empty)
int wbr_plan(const fmx_wb_config &cfg, WbrPlan *p, std::string *err, bool taps = true);
// one channel's rows [Q][4][Lp]: phase r's entry kk holds tap j = Lp - 1 - kk
// (zero for j >= L_r), W_r[j] = g[Q j + b_r] e^{+j 2 pi f j / Fs}
void wbr_weight_rows(const WbrPlan &p, int freq_hz, uint16_t *rows);
// W_r[j] (re, im), j = 0..L_r-1, read back from such rows
void wbr_rows_to_taps(const WbrPlan &p, const uint16_t *rows, int phase, float *out);
// The kernel's tiling.  Tile T = mb Q + r is the 16 outputs (16 mb + col) Q + r;
// workgroup w takes the tiles [w nt, (w + 1) nt) and stages the wide samples
// from 16 mb0 P - (Lp - 1) on, mb0 its first tile's mb.
// k_wbr, its launcher and fmx_wb_rational_geometry all compute with these.
constexpr int wbr_window(int P, int a_last, int Lp, int mb0, int mb1) { return (16 * (mb1 - mb0) + 15) * P + a_last + Lp; }
struct WbrGroup {
  int T0, T1; // the workgroup's first and last tile
  int mb0;    // the block of 16 outputs per phase its image starts at
  int window; // samples it stages
};
constexpr WbrGroup wbr_group(int wg, int nt, int ntiles, int P, int Q, int a_last, int Lp) {
  const int T0 = wg * nt, T1 = (T0 + nt < ntiles ? T0 + nt : ntiles) - 1;
  return WbrGroup{T0, T1, T0 / Q, wbr_window(P, a_last, Lp, T0 / Q, T1 / Q)};
}
// where tile T's column 0 starts in the image of a workgroup whose image starts at block mb0
constexpr int wbr_tile_offset(int P, int Q, int a_r, int T, int mb0) { return 16 * (T / Q - mb0) * P + a_r; }
// tiles per workgroup: as many as fit WB_LDS_MAX wherever the workgroup starts, at most WB_NT_MAX and what the call needs
int wbr_tiles(int P, int Q, int a_last, int Lp, int s16, int n_out);

struct WbrArgs {
  const void *in;       // n_out P / Q wide samples, interleaved I/Q
  int s16, in_al;       // as WbArgs
  int P, Q, Lh, Lp, n_out, C; // n_out a multiple of Q
  int a[FMX_WBR_QMAX];  // a_r
  const uint16_t *w;    // [C][Q][4][Lp] weight rows
  const uint32_t *fpos; // [C] f mod Fs
  const void *hist;     // the last Lh - 1 raw samples before this call
  void *hist_out;
  int valid;
  uint32_t fs, base_mod;
  double inv_fs;
  float scale;
  float *out;
  int out_stride;
  int nt, ntiles;       // tiles per workgroup, tiles of the call (set by the launcher)
  long n_in;            // n_out P / Q (set by the launcher)
};
int launch_wbr(const WbrArgs &a, void *stream);

// ---- band scan (fmx_wb_scan.inc; plan and weight rows are the channelizer's) ----
struct WbScanArgs {
  const void *in;          // n_out * D wide samples, interleaved I/Q
  int s16, in_al;          // as WbArgs
  int D, tpp, Lp, n_out, P; // P scan points
  const uint16_t *w;       // [P][4][Lp] weight rows
  float *partial;          // [(P + 15) / 16][nwg][16] sums of |raw y|^2
  uint32_t *clip;          // [nclip][2] hard- and near-clipped samples
  float *sm;               // [P][2] smoother value, initialised flag
  fmx_signal_level *level; // [P]
  double pscale;           // raw |y|^2 -> |y|^2
  double sp[4];            // gain*factor, bias, floor, ceil
  int nt, nwg, nclip;      // tiles per workgroup, workgroups per point group, clip workgroups (set by the launcher)
};
int wb_scan_tiles(int D, int Lp, int s16);
int wb_scan_workgroups(int n_out, int tpp, int nt);
int wb_scan_clip_workgroups(long n_in);
int launch_wb_scan(const WbScanArgs &a, void *stream);

// ---- band receiver's RF level (fmx_wb_level.inc): the level of every channel from one call's rows ----
struct WbLevelArgs {
  const float *rows;       // [C][2 * stride] the call's complex rows (k_wb's output)
  int stride, n, C;        // stride in complex samples, n outputs per channel
  const void *in;          // the call's n * D wide samples, interleaved I/Q
  int s16, D;              // as WbArgs
  uint32_t *clip;          // [nclip][2] hard- and near-clipped samples (k_wb_scan_clip's)
  float *sm;               // [C][2] smoother value, initialised flag
  fmx_signal_level *level; // [C]
  double sp[4];            // gain*factor, bias, floor, ceil
  int nclip;               // clip workgroups (set by the launcher)
  long n_in;               // the call's raw samples when they are not n * D (a rational object: n P / Q; D is then unused); 0: n * D
};
int launch_wb_level(const WbLevelArgs &a, void *stream);

// ---- DC offset and IQ imbalance (fmx_iqc.h, fmx_wb_iqc.inc) ----
// (SR, SI) of one channel's rows: the sums of its taps as the kernel multiplies them (units of W * 2^sexp)
void wb_tap_sums(const WbPlan &p, const uint16_t *rows, float *out2);
int iqc_workgroups(long n_in, int s16);                                  // k_iqc_sums' grid: [workgroups][5] int64 partials
int launch_iqc_set(FmxIqcBlock *blk, const FmxIqcBlock &v, void *stream); // the whole block (FIXED, or AUTO's restart)
// the estimator and its finisher over one call's raw samples: the block holds the call's parameters behind them
int launch_iqc_estimate(const void *in, long n_in, int s16, double alpha, long long *partial, FmxIqcBlock *blk, void *stream);
// launch_wb / launch_wb_scan with the corrected kernels; tsum: [C][2] / [P][2] tap sums (device)
int launch_wb_iqc(const WbArgs &a, const FmxIqcBlock *iqc, const float *tsum, void *stream);
int launch_wb_scan_iqc(const WbScanArgs &a, const FmxIqcBlock *iqc, const float *tsum, void *stream);

// ---- capture bank (fmx_wb_bank.inc): S captures of one plan channelized by one launch ----
#define FMX_WBB_CAPTURES_MAX 1024
#define FMX_WBB_GROUPS_MAX 65535 // the kernel's grid.y
// one capture's stream position, kept on the device: k_wbb reads it, k_wbb_hist
// (one writer per capture) advances it, k_wbb_set_state rewrites it
struct WbbState {
  uint64_t counter; // wide-sample index of the next call's first sample
  int valid;        // samples of the capture's history that exist (since its last reset)
  int pad;
};
struct WbbArgs {
  const void *in;          // [S][wide_stride] wide samples, interleaved I/Q; n_out * D of each row are read
  size_t wide_stride;      // samples
  int s16, in_al;          // as WbArgs
  int D, L, Lp, n_out, C, S; // C: the channels of all captures
  const uint16_t *w;       // [C][4][Lp] weight rows
  const uint32_t *fpos;    // [C] f mod Fs
  const void *hist;        // [S][L - 1] raw samples before this call
  void *hist_out;          // the same after it (another buffer)
  WbbState *state;         // [S]
  const int *groups;       // [G][3] capture, first channel, channels (1..16): fmx_wb_bank_groups
  int G;
  uint32_t fs;
  double inv_fs;
  float scale;
  float *out;
  int out_stride;
  int nt;                  // set by the launcher
};
// the work list of k_wbb (fmx_wb_design.cpp; fmx_wb_bank_groups is its C entry)
int wbb_groups(const int *first_channel, int n_captures, int *out, int cap);
int launch_wbb(const WbbArgs &a, void *stream); // k_wbb, then k_wbb_hist (which advances the state)
int launch_wbb_set_state(WbbState *state, int S, int capture /* -1: all */, uint64_t counter, void *stream);
int launch_wbb_set_params(double *sp /* [S][4] */, int S, int capture /* -1: all */, const double *v, void *stream);
struct WbbLevelArgs {
  const float *rows;       // as WbLevelArgs, C the channels of all captures
  int stride, n, C, S;
  const void *in;          // the call's [S][wide_stride] wide samples
  size_t wide_stride;
  int s16, D;
  uint32_t *clip;          // [S][nclip][2]
  const int *chan_cap;     // [C] the capture a channel belongs to
  float *sm;               // [C][2]
  fmx_signal_level *level; // [C]
  const double *sp;        // [S][4] gain*factor, bias, floor, ceil of each capture (device)
  int nclip;               // set by the launcher
  long n_in;               // a capture's raw samples of the call when they are not n * D (a rational bank: n P / Q; D is then unused); 0: n * D
};
int launch_wbb_level(const WbbLevelArgs &a, void *stream);

// ---- the bank at rational rates (fmx_wb_bank_rational.inc) ----
// k_wbr's tile list (grid.x) over k_wbb's group table (grid.y): WbrArgs with
// in, hist, valid and base_mod per capture, as WbbArgs has them
struct RbankArgs {
  const void *in;          // [S][wide_stride] wide samples; n_out P / Q of each row are read
  size_t wide_stride;      // samples
  int s16, in_al;          // as WbArgs
  int P, Q, Lh, Lp, n_out, C, S; // n_out a multiple of Q; C: the channels of all captures
  int a[FMX_WBR_QMAX];     // a_r
  const uint16_t *w;       // [C][Q][4][Lp] weight rows
  const uint32_t *fpos;    // [C] f mod Fs
  const void *hist;        // [S][Lh - 1] raw samples before this call
  void *hist_out;          // the same after it (another buffer)
  WbbState *state;         // [S]
  const int *groups;       // [G][3] as WbbArgs
  int G;
  uint32_t fs;
  double inv_fs;
  float scale;
  float *out;
  int out_stride;
  int nt, ntiles;          // as WbrArgs (set by the launcher)
  long n_in;               // n_out P / Q (set by the launcher)
};
int launch_rbank(const RbankArgs &a, void *stream); // k_rbank, then k_rbank_hist (which advances the state)

// ---- the bank's DC / IQ-imbalance correction (fmx_wb_bank_iqc.inc) ----
// one capture's mode and smoothing, kept on the device beside its FmxIqcBlock:
// k_bank_iqc_set writes it, the estimator, the finisher and k_bank_iqc read it
struct WbbIqcMode {
  double alpha; // AUTO's smoothing, in (0, 1]
  int mode;     // FMX_IQC_*
  int pad;
};
struct WbbIqcArgs {
  FmxIqcBlock *blk;    // [S]
  WbbIqcMode *mode;    // [S]
  long long *partial;  // [S][workgroups of the call][5] the estimator's sums
  const float *tsum;   // [C][2] tap sums (SR, SI)
};
// capture's block, mode and alpha (-1: every capture's) on the stream
int launch_wbb_iqc_set(const WbbIqcArgs &q, int S, int capture, const FmxIqcBlock &v, int mode, double alpha, void *stream);
// the estimator and the finisher over the first n_in raw samples of row s of
// [S][wide_stride] for every capture in AUTO (the bank's call, the bank scan's read)
int launch_wbb_iqc_estimate(const void *in, size_t wide_stride, long n_in, int s16, int S, const WbbIqcArgs &q, void *stream);
// launch_wbb with k_bank_iqc in k_wbb's place
int launch_wbb_iqc(const WbbArgs &a, const WbbIqcArgs &q, void *stream);

// ---- band scan over a capture bank (fmx_wb_bank_scan.inc) ----
#define FMX_BSCAN_POINTS_MAX 8192 // the single scan's limit, over all captures
struct BscanArgs {
  const void *in;          // [S][wide_stride] wide samples, interleaved I/Q; n_out * D of each row are read
  size_t wide_stride;      // samples
  int s16, in_al;          // as WbArgs
  int D, tpp, Lp, n_out, P, S; // P: the points of all captures
  const uint16_t *w;       // [P][4][Lp] weight rows
  const int *groups;       // [G][3] capture, first point, points (1..64): fmx_wb_bank_scan_groups
  int G;
  const int *pt_slot;      // [P] 16 (4 entry + wave) + column: where the point's partials lie
  const int *pt_cap;       // [P] the capture a point belongs to
  float *partial;          // [4 G][nwg][16] sums of |raw y|^2
  uint32_t *clip;          // [S][nclip][2] (k_wbb_clip's)
  float *sm;               // [P][2] smoother value, initialised flag
  fmx_signal_level *level; // [P]
  double pscale;           // raw |y|^2 -> |y|^2
  const double *sp;        // [S][4] gain*factor, bias, floor, ceil of each capture (device)
  int nt, nwg, nclip;      // as WbScanArgs (set by the launcher)
};
// the work list of k_bscan (fmx_wb_design.cpp; fmx_wb_bank_scan_groups is its C entry)
int bscan_groups(const int *first_point, int n_captures, int *out, int cap);
int launch_bscan(const BscanArgs &a, void *stream); // k_wbb_clip, k_bscan, k_bscan_level
// a read with a capture out of OFF (fmx_wb_bank_scan_iqc.inc):
// the bank's estimator (any_auto), k_wbb_clip, k_scan_bank_iqc, k_bscan_level;
// q.tsum: [P][2] tap sums of the points
int launch_bscan_iqc(const BscanArgs &a, const WbbIqcArgs &q, int any_auto, void *stream);

int launch_iq_to_u8(const float *in, int in_stride, int C, int n, uint8_t *out, size_t out_stride, void *stream);
int launch_copy16(const void *src, void *dst, size_t n16, void *stream); // 16-B words, any memory the device maps

} // namespace fmx

#endif
