/* ================================================================== */
/* k_wb: the wideband channelizer (fmx_wb_process, DESIGN.md section 18) */
/* ================================================================== */
/* The shared pieces (fmx_wb_core.inc) as one object's call.  Workgroup =
 * 16 channels (blockIdx.y) x nt tiles of 16 consecutive outputs (4 waves,
 * tile t on wave t & 3): it stages the window of its (16 nt - 1) D + Lp wide
 * samples from the call's input and the object's history, runs wb_tile per
 * tile with the windows D apart, and rotates output n by the phase of wide
 * sample base + n D.  k_wb_hist then keeps the last L - 1 raw samples for the
 * next call. */
template <bool S16, bool EVEN> __global__ __launch_bounds__(256) void k_wb(WbArgs a) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n0 = (int)blockIdx.x * 16 * a.nt; // first output of the workgroup
  const int NI = (16 * a.nt - 1) * a.D + a.Lp; // samples of the window
  const int NIp = (NI + 7) & ~7;
  const WbImage m = wb_image(NIp);
  wb_stage<S16, true>(m, NI, NIp, (long)n0 * a.D - (a.Lp - 1), (long)a.n_out * a.D, a.valid, a.in, a.hist, a.L, a.in_al, tid);
  const int col = lane & 15, g = lane >> 4;
  // a ragged last group computes its last channel again in the spare rows (not stored)
  const int ca = min(16 * (int)blockIdx.y + col, a.C - 1);
  const uint16_t *wrow = a.w + (size_t)ca * 4 * a.Lp + 8 * g;
  for (int t = wave; t < a.nt; t += 4) {
    const int nt0 = n0 + 16 * t;
    if (nt0 >= a.n_out) break;
    wb_f32x4 rr, ii, ri, ir;
    wb_tile<S16, EVEN>(m, (16 * t + col) * a.D + 8 * g, wrow, a.Lp, rr, ii, ri, ir);
    // lane: output nt0 + col of channels 16 group + 4 g + i
    const int n = nt0 + col;
    if (n >= a.n_out) continue;
    const uint64_t smod = ((uint64_t)a.base_mod + (uint64_t)n * (uint64_t)a.D) % a.fs; // the output's sample index mod Fs
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = 16 * (int)blockIdx.y + 4 * g + i;
      if (c >= a.C) break;
      wb_rotate_store(a.fpos[c], smod, a.fs, a.inv_fs, rr[i] - ii[i], ri[i] + ir[i], a.scale,
                      a.out + 2 * ((size_t)c * a.out_stride + n));
    }
  }
}

// the last L - 1 raw samples of (history, this call's input) into the other history buffer
template <typename T> __global__ void k_wb_hist(WbArgs a) {
  const int j = (int)blockIdx.x * 256 + threadIdx.x;
  if (j >= a.L - 1) return;
  const long n_in = (long)a.n_out * a.D;
  const long i = n_in - (a.L - 1) + j;
  const T *src = i >= 0 ? static_cast<const T *>(a.in) + 2 * i : static_cast<const T *>(a.hist) + 2 * (j + n_in);
  T *dst = static_cast<T *>(a.hist_out) + 2 * (size_t)j;
  dst[0] = src[0];
  dst[1] = src[1];
}

// launch_wb and launch_wb_iqc: the checks, the tiling, `launch` for the
// channelizer's kernel (a, LDS bytes, grid, stream) and the history kernel
template <class Launch> static int wb_run(const WbArgs &a0, void *stream, Launch launch) {
  WbArgs a = a0;
  if (a.C <= 0 || a.n_out <= 0) return FMX_OK;
  if (a.D < 2 || a.L != (a.L / a.D) * a.D || a.Lp < a.L || (a.Lp & 31) || a.valid < 0 || a.valid > a.L - 1)
    return FMX_E_INVALID;
  a.nt = wb_tiles(a.D, a.Lp, a.s16, a.n_out);
  if (a.nt < 1) return FMX_E_INVALID;
  a.in_al = wb_in_aligned(a.in, a.s16);
  const size_t smem = wb_lds_bytes((16 * a.nt - 1) * a.D + a.Lp, a.s16);
  if (smem > WB_LDS_MAX) return FMX_E_INVALID;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)((a.n_out + 16 * a.nt - 1) / (16 * a.nt)), (unsigned)((a.C + 15) / 16));
  const int rc = launch(a, smem, grid, st);
  if (rc != FMX_OK) return rc;
  const dim3 hgrid((unsigned)((a.L - 1 + 255) / 256));
  if (a.s16) hipLaunchKernelGGL(k_wb_hist<int16_t>, hgrid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(k_wb_hist<uint8_t>, hgrid, dim3(256), 0, st, a);
  return hipGetLastError() == hipSuccess ? FMX_OK : FMX_E_HIP;
}

int launch_wb(const WbArgs &a0, void *stream) {
  return wb_run(a0, stream, [](const WbArgs &a, size_t smem, dim3 grid, hipStream_t st) {
    return WB_LAUNCH(k_wb, a.s16, (a.D & 1) == 0, grid, smem, st, a);
  });
}
