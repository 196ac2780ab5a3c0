/* ================================================================== */
/* DC offset and IQ imbalance per capture of the bank                   */
/* (fmx_wb_bank_set_iq_correction; DESIGN.md section 26)                */
/* ================================================================== */
/* Every capture of a bank has a front end of its own, so each has its own
 * FmxIqcBlock and its own {mode, alpha} (WbbIqcMode), both in device memory
 * and both written on the stage stream by k_bank_iqc_set: a set stays queued
 * between the calls like a reset does.  A call of a bank with a capture out
 * of OFF is
 *   k_bank_iqc_sums    (any capture in AUTO) k_iqc_sums' workgroup over row
 *                      blockIdx.y: exact int64 partials [S][workgroups][5];
 *                      the workgroups of a capture not in AUTO return at once
 *   k_bank_iqc_finish  (any capture in AUTO) one thread per capture in AUTO:
 *                      k_iqc_finish's body with the capture's alpha
 *   k_bank_iqc         k_wbb with k_wb_iqc's epilogue; a capture in OFF takes
 *                      k_wbb's own epilogue, chosen per workgroup
 *   k_wbb_hist         as ever
 * whatever the number of captures, and nothing waits for the host.  The
 * pieces are the family's (fmx_wb_core.inc) and the estimator's
 * (fmx_wb_iqc.inc), so capture s gives the bits an fmx_wb object gives that
 * was set the same way.  A bank whose captures are all in OFF launches k_wbb. */

template <bool S16, bool EVEN>
__global__ __launch_bounds__(256) void k_bank_iqc(WbbArgs a, const FmxIqcBlock *iqc, const WbbIqcMode *mode, const float *tsum) {
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
  // the capture's mode and the call's parameters: uniform loads, ahead of the K loop
  const bool corrected = mode[cap].mode != FMX_IQC_OFF;
  const float d_i = iqc[cap].k[0], d_q = iqc[cap].k[1], gain = iqc[cap].k[2], cross = iqc[cap].k[3];
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
      float *po = a.out + 2 * ((size_t)c * a.out_stride + n);
      if (corrected) { // k_wb_iqc's epilogue
        const WbRot rot = wb_rotation(a.fpos[c], smod, a.fs, a.inv_fs);
        const float SR = tsum[2 * c], SI = tsum[2 * c + 1];
        const WbSum y = wb_iqc_mix(rr[i], ii[i], ri[i], ir[i], d_i * SR, d_i * SI, d_q * SR, d_q * SI, gain, cross);
        wb_store(rot, y.re, y.im, a.scale, po);
      } else { // k_wbb's
        wb_rotate_store(a.fpos[c], smod, a.fs, a.inv_fs, rr[i] - ii[i], ri[i] + ir[i], a.scale, po);
      }
    }
  }
}

// k_iqc_sums with a capture dimension (blockIdx.y) over row s of the call's
// input: partial[s][workgroup][5].  A row takes 16-B loads when its own
// address allows them; the sums are exact either way.
template <typename T>
__global__ __launch_bounds__(256) void k_bank_iqc_sums(const void *in, size_t wide_stride, long n_in, const WbbIqcMode *mode,
                                                       long long *partial) {
  const int cap = (int)blockIdx.y;
  if (mode[cap].mode != FMX_IQC_AUTO) return; // the whole workgroup
  const T *row = static_cast<const T *>(in) + 2 * (size_t)cap * wide_stride;
  const int al16 = (reinterpret_cast<uintptr_t>(row) & 15) == 0;
  iqc_sum_workgroup<T>(row, n_in, al16, partial + 5 * ((size_t)cap * gridDim.x + blockIdx.x));
}

// one thread per capture in AUTO: its partials in index order, its alpha
__global__ __launch_bounds__(64) void k_bank_iqc_finish(const long long *partial, int nwg, long n_in, double unit,
                                                        const WbbIqcMode *mode, FmxIqcBlock *blk, int S) {
  const int s = (int)blockIdx.x * 64 + threadIdx.x;
  if (s >= S || mode[s].mode != FMX_IQC_AUTO) return;
  iqc_finish_block(partial + 5 * (size_t)s * nwg, nwg, n_in, mode[s].alpha, unit, blk + s);
}

// a capture's block, mode and alpha on the stream: one thread, the values by argument
__global__ void k_bank_iqc_set(FmxIqcBlock *blk, WbbIqcMode *tab, int S, int capture, FmxIqcBlock v, int mode, double alpha) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  for (int s = capture < 0 ? 0 : capture; s < (capture < 0 ? S : capture + 1); ++s) {
    blk[s] = v;
    tab[s].alpha = alpha;
    tab[s].mode = mode;
    tab[s].pad = 0;
  }
}

int launch_wbb_iqc_set(const WbbIqcArgs &q, int S, int capture, const FmxIqcBlock &v, int mode, double alpha, void *stream) {
  if (!q.blk || !q.mode || S < 1 || capture < -1 || capture >= S) return FMX_E_INVALID;
  hipLaunchKernelGGL(k_bank_iqc_set, dim3(1), dim3(1), 0, static_cast<hipStream_t>(stream), q.blk, q.mode, S, capture, v,
                     mode, alpha);
  return hipGetLastError() == hipSuccess ? FMX_OK : FMX_E_HIP;
}

// the first n_in raw samples of rows [S][wide_stride]: the bank's call and the bank scan's read
int launch_wbb_iqc_estimate(const void *in, size_t wide_stride, long n_in, int s16, int S, const WbbIqcArgs &q, void *stream) {
  if (!in || !q.blk || !q.mode || !q.partial || S < 1 || S > FMX_WBB_CAPTURES_MAX || n_in < 1 || wide_stride < (size_t)n_in)
    return FMX_E_INVALID;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int nwg = iqc_workgroups(n_in, s16);
  const dim3 grid((unsigned)nwg, (unsigned)S);
  if (s16) hipLaunchKernelGGL(k_bank_iqc_sums<int16_t>, grid, dim3(256), 0, st, in, wide_stride, n_in, q.mode, q.partial);
  else hipLaunchKernelGGL(k_bank_iqc_sums<uint8_t>, grid, dim3(256), 0, st, in, wide_stride, n_in, q.mode, q.partial);
  if (hipGetLastError() != hipSuccess) return FMX_E_HIP;
  hipLaunchKernelGGL(k_bank_iqc_finish, dim3((unsigned)((S + 63) / 64)), dim3(64), 0, st, q.partial, nwg, n_in,
                     s16 ? 32768.0 : 255.0, q.mode, q.blk, S);
  return hipGetLastError() == hipSuccess ? FMX_OK : FMX_E_HIP;
}

int launch_wbb_iqc(const WbbArgs &a0, const WbbIqcArgs &q, void *stream) {
  if (!q.blk || !q.mode || !q.tsum) return FMX_E_INVALID;
  return wbb_run(a0, stream, [=](const WbbArgs &a, size_t smem, dim3 grid, hipStream_t st) {
    return WB_LAUNCH(k_bank_iqc, a.s16, (a.D & 1) == 0, grid, smem, st, a, q.blk, q.mode, q.tsum);
  });
}
