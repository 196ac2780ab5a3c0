/* ================================================================== */
/* k_wb_scan: the band scan (fmx_wb_scan_process, DESIGN.md section 19) */
/* ================================================================== */
/* One call is one read of every scan point: with y_p[n] the channelizer's
 * output of a channel tuned to point p, x indexed from the call's first
 * sample,
 *   P_p = 1 / (n_out - tpp) sum_{n = tpp}^{n_out - 1} |y_p[n]|^2
 * -- |y| needs no rotation, and the outputs n < tpp, whose windows reach before
 * the call, are left out, so there is no history.  The image, the weight rows
 * and the chains are the family's (fmx_wb_core.inc: wb_stage without history,
 * wb_scan_mac); what the scan adds:
 *   - a workgroup is 4 point groups (one per wave, 16 points each) x nt <= 4
 *     tiles of 16 outputs from output tpp + 16 nt blockIdx.x on: a wave holds
 *     the accumulators of all its tiles (nt x rr / ii / ri / ir) and loads each
 *     weight fragment once for them, and the window is staged once for 64
 *     points.  (The LDS budget holds 4 tiles at D = 100 in int16, so the
 *     tiles a wave can share its weights among are the workgroup's.)
 *   - the epilogue forms re^2 + im^2 of the columns in [tpp, n_out), adds the
 *     wave's tiles in tile order in registers, then the 16 columns by DPP row
 *     rotations (8, 4, 2, 1 lanes), and stores one f32 per point into
 *     partial[point group][workgroup][16].  No atomics; a point's sum order
 *     is fixed by (D, Lp, format, n_out) alone, whatever else the plan holds.
 * k_wb_scan_clip counts the call's clipped raw samples per workgroup;
 * k_wb_scan_level adds a point's partials and the clip counts in index order
 * and writes the record. */
template <bool S16, bool EVEN> __global__ __launch_bounds__(256) void k_wb_scan(WbScanArgs a) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n0 = a.tpp + (int)blockIdx.x * 16 * a.nt; // first output of the workgroup
  const int NI = (16 * a.nt - 1) * a.D + a.Lp;       // samples of the window
  const int NIp = (NI + 7) & ~7;
  const WbImage m = wb_image(NIp);
  // the image starts at sample n0 D - (Lp - 1) >= L - Lp + 1 > -32, and the
  // entries before sample 0 meet the rows' zero padding only
  wb_stage<S16, false>(m, NI, NIp, (long)n0 * a.D - (a.Lp - 1), (long)a.n_out * a.D, 0, a.in, nullptr, 0, a.in_al, tid);
  const int grp = 4 * (int)blockIdx.y + wave; // the wave's point group
  if (16 * grp >= a.P) return;
  const int col = lane & 15, g = lane >> 4;
  // a ragged last group computes its last point again in the spare rows (not read)
  const int pa = min(16 * grp + col, a.P - 1);
  // tiles of the workgroup that hold an output below n_out (wave-uniform)
  const int tiles = min(a.nt, (a.n_out - n0 + 15) >> 4);
  wb_f32x4 rr[WB_SCAN_NT], ii[WB_SCAN_NT], ri[WB_SCAN_NT], ir[WB_SCAN_NT];
  wb_scan_mac<S16, EVEN>(m, a.w + (size_t)pa * 4 * a.Lp + 8 * g, a.Lp, a.D, col, g, tiles, rr, ii, ri, ir);
  // lane: output n0 + 16 t + col of points 16 grp + 4 g + i
  float pw[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int t = 0; t < WB_SCAN_NT; ++t) {
    const int n = n0 + 16 * t + col;
    const bool live = t < tiles && n >= a.tpp && n < a.n_out;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float re = rr[t][i] - ii[t][i], im = ri[t][i] + ir[t][i];
      pw[i] += live ? re * re + im * im : 0.0f;
    }
  }
  wb_scan_reduce_store(pw, col, a.partial + ((size_t)grp * gridDim.x + blockIdx.x) * 16 + 4 * g);
}

// every raw sample of the call once, 2048 per workgroup: the counts to clip[workgroup][2]
template <typename T> __global__ __launch_bounds__(256) void k_wb_scan_clip(WbScanArgs a) {
  wb_clip_count(static_cast<const T *>(a.in), (long)a.n_out * a.D, a.clip + 2 * (size_t)blockIdx.x);
}

// One lane per point: its partials over the workgroups in index order, in double, to the record
__global__ __launch_bounds__(64) void k_wb_scan_level(WbScanArgs a) {
  const int p = (int)blockIdx.x * 64 + threadIdx.x;
  if (p >= a.P) return;
  const float *pp = a.partial + (size_t)(p >> 4) * a.nwg * 16 + (p & 15);
  double sum = 0.0;
  for (int wg = 0; wg < a.nwg; ++wg) sum += (double)pp[(size_t)wg * 16];
  a.level[p] = wb_level_record(sum, a.pscale, (double)(a.n_out - a.tpp), a.clip, a.nclip, (double)((long)a.n_out * a.D),
                               a.sp, a.sm + 2 * (size_t)p);
}

// tiles per workgroup: what the LDS budget holds, at most WB_SCAN_NT -- a
// function of the plan alone, so that a point's sum order is too
int wb_scan_tiles(int D, int Lp, int s16) { return (int)std::min<long>(wb_tiles_fit(D, Lp, s16), WB_SCAN_NT); }
int wb_scan_workgroups(int n_out, int tpp, int nt) { return (n_out - tpp + 16 * nt - 1) / (16 * nt); }
int wb_scan_clip_workgroups(long n_in) { return (int)((n_in + 2047) / 2048); }

// launch_wb_scan and launch_wb_scan_iqc: the checks, the tiling, the clip
// kernel, `launch` for the scan's kernel (a, LDS bytes, grid, stream) and the level kernel
template <class Launch> static int wb_scan_run(const WbScanArgs &a0, void *stream, Launch launch) {
  WbScanArgs a = a0;
  if (a.P <= 0 || a.D < 2 || a.tpp < 1 || a.Lp < a.D * a.tpp || (a.Lp & 31) || a.n_out <= a.tpp) return FMX_E_INVALID;
  a.nt = wb_scan_tiles(a.D, a.Lp, a.s16);
  if (a.nt < 1) return FMX_E_INVALID;
  a.nwg = wb_scan_workgroups(a.n_out, a.tpp, a.nt);
  a.nclip = wb_scan_clip_workgroups((long)a.n_out * a.D);
  a.in_al = wb_in_aligned(a.in, a.s16);
  const size_t smem = wb_lds_bytes((16 * a.nt - 1) * a.D + a.Lp, a.s16);
  if (smem > WB_LDS_MAX) return FMX_E_INVALID;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (a.s16) hipLaunchKernelGGL(k_wb_scan_clip<int16_t>, dim3((unsigned)a.nclip), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(k_wb_scan_clip<uint8_t>, dim3((unsigned)a.nclip), dim3(256), 0, st, a);
  if (hipGetLastError() != hipSuccess) return FMX_E_HIP;
  const int rc = launch(a, smem, dim3((unsigned)a.nwg, (unsigned)((a.P + 63) / 64)), st);
  if (rc != FMX_OK) return rc;
  hipLaunchKernelGGL(k_wb_scan_level, dim3((unsigned)((a.P + 63) / 64)), dim3(64), 0, st, a);
  return hipGetLastError() == hipSuccess ? FMX_OK : FMX_E_HIP;
}

int launch_wb_scan(const WbScanArgs &a0, void *stream) {
  return wb_scan_run(a0, stream, [](const WbScanArgs &a, size_t smem, dim3 grid, hipStream_t st) {
    return WB_LAUNCH(k_wb_scan, a.s16, (a.D & 1) == 0, grid, smem, st, a);
  });
}
