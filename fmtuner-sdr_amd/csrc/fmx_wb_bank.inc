/* ================================================================== */
/* k_wbb: the capture bank -- S wide captures of one plan channelized  */
/* by one launch (fmx_wb_bank_*, DESIGN.md section 22)                 */
/* ================================================================== */
/* Capture s owns the channels [first_channel[s], first_channel[s + 1]) of the
 * bank and row s of the call's input [S][wide_stride].  The kernel's work is
 * a flat device table of groups {capture, first channel, channels 1..16}
 * (fmx_wb_bank_groups): one entry per 16 channels of a capture, none for an
 * empty capture, blockIdx.y its index.  k_wbb is k_wb's use of the shared
 * pieces (fmx_wb_core.inc) with in, hist, valid and base_mod taken from the
 * group's capture and the channels from the group; the image, the chains and
 * the rotation are the one definition k_wb runs, so a capture's rows are bit
 * for bit those of an fmx_wb object fed its row.
 * Each capture's {counter, valid} lives on the device (WbbState): k_wbb reads
 * it, k_wbb_hist (one writer per capture, behind k_wbb on the stream)
 * advances it, k_wbb_set_state rewrites it for a reset -- calls, resets and
 * parameter changes stay queued with no host synchronisation and no staging
 * image that would have to outlive the call. */
template <bool S16, bool EVEN> __global__ __launch_bounds__(256) void k_wbb(WbbArgs a) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // the workgroup's group and its capture
  const int *grp = a.groups + 3 * (size_t)blockIdx.y;
  const int cap = grp[0], c0 = grp[1], cn = grp[2];
  const size_t sb = S16 ? 4 : 2; // bytes of a wide sample
  const unsigned char *cin = static_cast<const unsigned char *>(a.in) + (size_t)cap * a.wide_stride * sb;
  const unsigned char *chist = static_cast<const unsigned char *>(a.hist) + (size_t)cap * (size_t)(a.L - 1) * sb;
  const int valid = a.state[cap].valid;
  const uint32_t base_mod = (uint32_t)(a.state[cap].counter % (uint64_t)a.fs);
  const int n0 = (int)blockIdx.x * 16 * a.nt; // first output of the workgroup
  const int NI = (16 * a.nt - 1) * a.D + a.Lp; // samples of the window
  const int NIp = (NI + 7) & ~7;
  const WbImage m = wb_image(NIp);
  wb_stage<S16, true>(m, NI, NIp, (long)n0 * a.D - (a.Lp - 1), (long)a.n_out * a.D, valid, cin, chist, a.L, a.in_al, tid);
  const int col = lane & 15, g = lane >> 4;
  // a ragged group computes its last channel again in the spare rows (not stored)
  const int ca = c0 + min(col, cn - 1);
  const uint16_t *wrow = a.w + (size_t)ca * 4 * a.Lp + 8 * g;
  for (int t = wave; t < a.nt; t += 4) {
    const int nt0 = n0 + 16 * t;
    if (nt0 >= a.n_out) break;
    wb_f32x4 rr, ii, ri, ir;
    wb_tile<S16, EVEN>(m, (16 * t + col) * a.D + 8 * g, wrow, a.Lp, rr, ii, ri, ir);
    // lane: output nt0 + col of the group's channels 4 g + i
    const int n = nt0 + col;
    if (n >= a.n_out) continue;
    const uint64_t smod = ((uint64_t)base_mod + (uint64_t)n * (uint64_t)a.D) % a.fs; // the output's sample index mod Fs
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (4 * g + i >= cn) break;
      const int c = c0 + 4 * g + i;
      wb_rotate_store(a.fpos[c], smod, a.fs, a.inv_fs, rr[i] - ii[i], ri[i] + ir[i], a.scale,
                      a.out + 2 * ((size_t)c * a.out_stride + n));
    }
  }
}

// k_wb_hist with a capture dimension (blockIdx.y): the last L - 1 raw samples
// of (history, this call's row) of every capture into the other history
// buffer.  Thread 0 of a capture's first workgroup then advances the
// capture's state: nothing in this kernel reads it, and k_wbb, its one
// reader, has ended before this kernel starts.
template <typename T> __global__ void k_wbb_hist(WbbArgs a) {
  const int j = (int)blockIdx.x * 256 + threadIdx.x;
  const int cap = (int)blockIdx.y;
  const long n_in = (long)a.n_out * a.D;
  if (j == 0) {
    WbbState *s = a.state + cap;
    s->valid = (int)min((long)(a.L - 1), (long)s->valid + n_in);
    s->counter += (uint64_t)n_in;
  }
  if (j >= a.L - 1) return;
  const T *cin = static_cast<const T *>(a.in) + 2 * (size_t)cap * a.wide_stride;
  const T *chist = static_cast<const T *>(a.hist) + 2 * (size_t)cap * (size_t)(a.L - 1);
  const long i = n_in - (a.L - 1) + j;
  const T *src = i >= 0 ? cin + 2 * i : chist + 2 * (j + n_in);
  T *dst = static_cast<T *>(a.hist_out) + 2 * ((size_t)cap * (size_t)(a.L - 1) + (size_t)j);
  dst[0] = src[0];
  dst[1] = src[1];
}

// a reset on the stream: one thread, its values by argument
__global__ void k_wbb_set_state(WbbState *state, int S, int capture, uint64_t counter) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  for (int s = capture < 0 ? 0 : capture; s < (capture < 0 ? S : capture + 1); ++s) {
    state[s].counter = counter;
    state[s].valid = 0; // k_wbb reads zeros for samples before the stream's start
  }
}

// a capture's signal parameters on the stream: one thread, the values by argument
__global__ void k_wbb_set_params(double *sp, int S, int capture, double v0, double v1, double v2, double v3) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  for (int s = capture < 0 ? 0 : capture; s < (capture < 0 ? S : capture + 1); ++s) {
    sp[4 * s] = v0;
    sp[4 * s + 1] = v1;
    sp[4 * s + 2] = v2;
    sp[4 * s + 3] = v3;
  }
}

// A bank call around `launch`, which starts the channelizer kernel (k_wbb, or
// k_bank_iqc of fmx_wb_bank_iqc.inc): the checks and the tiling ahead of it,
// k_wbb_hist behind it.
template <class Launch> static int wbb_run(const WbbArgs &a0, void *stream, Launch launch) {
  WbbArgs a = a0;
  if (a.S <= 0 || a.n_out <= 0) return FMX_OK;
  if (a.S > FMX_WBB_CAPTURES_MAX || a.G < 0 || a.G > FMX_WBB_GROUPS_MAX || a.C < 0 ||
      a.wide_stride < (size_t)a.n_out * (size_t)a.D)
    return FMX_E_INVALID;
  if (a.D < 2 || a.L != (a.L / a.D) * a.D || a.Lp < a.L || (a.Lp & 31)) return FMX_E_INVALID;
  a.nt = wb_tiles(a.D, a.Lp, a.s16, a.n_out); // the tiling is the single object's
  if (a.nt < 1) return FMX_E_INVALID;
  a.in_al = wb_in_aligned(a.in, a.s16); // every row starts a whole number of samples behind the base
  const size_t smem = wb_lds_bytes((16 * a.nt - 1) * a.D + a.Lp, a.s16);
  if (smem > WB_LDS_MAX) return FMX_E_INVALID;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (a.G > 0) {
    const dim3 grid((unsigned)((a.n_out + 16 * a.nt - 1) / (16 * a.nt)), (unsigned)a.G);
    const int rc = launch(a, smem, grid, st);
    if (rc != FMX_OK) return rc;
  }
  const dim3 hgrid((unsigned)((a.L - 1 + 255) / 256), (unsigned)a.S);
  if (a.s16) hipLaunchKernelGGL(k_wbb_hist<int16_t>, hgrid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(k_wbb_hist<uint8_t>, hgrid, dim3(256), 0, st, a);
  return hipGetLastError() == hipSuccess ? FMX_OK : FMX_E_HIP;
}

int launch_wbb(const WbbArgs &a0, void *stream) {
  return wbb_run(a0, stream, [](const WbbArgs &a, size_t smem, dim3 grid, hipStream_t st) {
    return WB_LAUNCH(k_wbb, a.s16, (a.D & 1) == 0, grid, smem, st, a);
  });
}

int launch_wbb_set_state(WbbState *state, int S, int capture, uint64_t counter, void *stream) {
  if (!state || S < 1 || capture < -1 || capture >= S) return FMX_E_INVALID;
  hipLaunchKernelGGL(k_wbb_set_state, dim3(1), dim3(1), 0, static_cast<hipStream_t>(stream), state, S, capture, counter);
  return hipGetLastError() == hipSuccess ? FMX_OK : FMX_E_HIP;
}

int launch_wbb_set_params(double *sp, int S, int capture, const double *v, void *stream) {
  if (!sp || !v || S < 1 || capture < -1 || capture >= S) return FMX_E_INVALID;
  hipLaunchKernelGGL(k_wbb_set_params, dim3(1), dim3(1), 0, static_cast<hipStream_t>(stream), sp, S, capture, v[0], v[1],
                     v[2], v[3]);
  return hipGetLastError() == hipSuccess ? FMX_OK : FMX_E_HIP;
}

/* ---- the bank's RF level (fmx_wb_bank_signal): k_wb_scan_clip and k_wb_level with a capture dimension ---- */
// the same 2048 samples per workgroup over the n_in raw samples (n D, or a
// rational bank's n P / Q) of row blockIdx.y of the call's input: the counts
// to clip[capture][workgroup][2]
template <typename T> __global__ __launch_bounds__(256) void k_wbb_clip(WbbLevelArgs a) {
  wb_clip_count(static_cast<const T *>(a.in) + 2 * (size_t)blockIdx.y * a.wide_stride, a.n_in,
                a.clip + 2 * ((size_t)blockIdx.y * a.nclip + blockIdx.x));
}

// the channel's capture selects the clip partials and the parameter set
template <int W> __global__ __launch_bounds__(256) void k_wbb_level(WbbLevelArgs a) {
  const int c = (int)blockIdx.x; // the grid is C workgroups
  const double sum = wb_row_power<W>(a.rows + (size_t)c * 2 * (size_t)a.stride, a.n);
  if (threadIdx.x != 0) return;
  const int cap = a.chan_cap[c];
  a.level[c] = wb_level_record(sum, 1.0, (double)a.n, a.clip + 2 * (size_t)cap * a.nclip, a.nclip,
                               (double)a.n_in, a.sp + 4 * (size_t)cap, a.sm + 2 * (size_t)c);
}

int launch_wbb_level(const WbbLevelArgs &a0, void *stream) {
  WbbLevelArgs a = a0;
  if (a.C <= 0 || a.S <= 0 || a.n <= 0 || a.stride < a.n || (a.n_in == 0 && a.D < 1) || a.n_in < 0 || !a.rows || !a.in ||
      !a.clip || !a.sm || !a.level || !a.chan_cap || !a.sp)
    return FMX_E_INVALID;
  if (a.n_in == 0) a.n_in = (long)a.n * a.D; // else a rational bank's call: n P / Q raw samples of every row
  if (a.wide_stride < (size_t)a.n_in) return FMX_E_INVALID;
  if ((reinterpret_cast<uintptr_t>(a.rows) & 3) || (reinterpret_cast<uintptr_t>(a.level) & 7)) return FMX_E_INVALID;
  a.nclip = wb_scan_clip_workgroups(a.n_in);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 cgrid((unsigned)a.nclip, (unsigned)a.S);
  if (a.s16) hipLaunchKernelGGL(k_wbb_clip<int16_t>, cgrid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(k_wbb_clip<uint8_t>, cgrid, dim3(256), 0, st, a);
  if (hipGetLastError() != hipSuccess) return FMX_E_HIP;
  const uintptr_t base = reinterpret_cast<uintptr_t>(a.rows);
  const dim3 grid((unsigned)a.C);
  if ((base & 15) == 0 && (a.stride & 1) == 0) hipLaunchKernelGGL(k_wbb_level<16>, grid, dim3(256), 0, st, a);
  else if ((base & 7) == 0) hipLaunchKernelGGL(k_wbb_level<8>, grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(k_wbb_level<4>, grid, dim3(256), 0, st, a);
  return hipGetLastError() == hipSuccess ? FMX_OK : FMX_E_HIP;
}
