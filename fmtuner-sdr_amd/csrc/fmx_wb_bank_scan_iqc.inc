/* ================================================================== */
/* DC offset and IQ imbalance per capture of the bank scan              */
/* (fmx_wb_bank_scan_set_iq_correction; DESIGN.md section 29)           */
/* ================================================================== */
/* Every capture of a bank scan has a front end of its own, so each has its
 * own FmxIqcBlock and its own {mode, alpha} (WbbIqcMode), as the captures of
 * a bank have (fmx_wb_bank_iqc.inc): k_bank_iqc_set writes them on the stage
 * stream, k_bank_iqc_sums and k_bank_iqc_finish estimate them from row s of
 * the read.  A read of an object with a capture out of OFF is
 *   k_bank_iqc_sums, k_bank_iqc_finish   (any capture in AUTO)
 *   k_wbb_clip                           as ever: the raw samples' counts
 *   k_scan_bank_iqc                      k_bscan with k_wb_scan_iqc's epilogue;
 *                                        a capture in OFF takes k_bscan's own
 *                                        epilogue, chosen per workgroup
 *   k_bscan_level                        as ever
 * whatever the number of captures, and nothing waits for the host.  The
 * pieces are the family's (fmx_wb_core.inc), so capture s gives the bits an
 * fmx_wb_scan object gives that was set the same way.  An object whose
 * captures are all in OFF launches k_bscan. */

template <bool S16, bool EVEN>
__global__ __launch_bounds__(256) void k_scan_bank_iqc(BscanArgs a, const FmxIqcBlock *iqc, const WbbIqcMode *mode,
                                                        const float *tsum) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // the workgroup's entry and its capture's row
  const int *ent = a.groups + 3 * (size_t)blockIdx.y;
  const int cap = ent[0], p0 = ent[1], pn = ent[2];
  const size_t sb = S16 ? 4 : 2; // bytes of a wide sample
  const unsigned char *cin = static_cast<const unsigned char *>(a.in) + (size_t)cap * a.wide_stride * sb;
  const int n0 = a.tpp + (int)blockIdx.x * 16 * a.nt; // first output of the workgroup
  const int NI = (16 * a.nt - 1) * a.D + a.Lp;       // samples of the window
  const int NIp = (NI + 7) & ~7;
  const WbImage m = wb_image(NIp);
  // as k_bscan: nothing of the row at or past sample n_out D is read
  wb_stage<S16, false>(m, NI, NIp, (long)n0 * a.D - (a.Lp - 1), (long)a.n_out * a.D, 0, cin, nullptr, 0, a.in_al, tid);
  if (16 * wave >= pn) return; // the entry's points [16 wave, 16 wave + 16)
  // the capture's mode and the read's parameters: uniform loads, ahead of the K loop
  const bool corrected = mode[cap].mode != FMX_IQC_OFF;
  const float d_i = iqc[cap].k[0], d_q = iqc[cap].k[1], gain = iqc[cap].k[2], cross = iqc[cap].k[3];
  const int col = lane & 15, g = lane >> 4;
  // a ragged wave computes its last point again in the spare rows (not read)
  const int pa = p0 + min(16 * wave + col, pn - 1);
  // tiles of the workgroup that hold an output below n_out (wave-uniform)
  const int tiles = min(a.nt, (a.n_out - n0 + 15) >> 4);
  wb_f32x4 rr[WB_SCAN_NT], ii[WB_SCAN_NT], ri[WB_SCAN_NT], ir[WB_SCAN_NT];
  wb_scan_mac<S16, EVEN>(m, a.w + (size_t)pa * 4 * a.Lp + 8 * g, a.Lp, a.D, col, g, tiles, rr, ii, ri, ir);
  // lane: output n0 + 16 t + col of the wave's points 4 g + i
  float pw[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (corrected) { // k_wb_scan_iqc's epilogue: the constants of the lane's four points
    float cR[4], cI[4], cQR[4], cQI[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int p = p0 + min(16 * wave + 4 * g + i, pn - 1);
      const float SR = tsum[2 * p], SI = tsum[2 * p + 1];
      cR[i] = d_i * SR;
      cI[i] = d_i * SI;
      cQR[i] = d_q * SR;
      cQI[i] = d_q * SI;
    }
#pragma unroll
    for (int t = 0; t < WB_SCAN_NT; ++t) {
      const int n = n0 + 16 * t + col;
      const bool live = t < tiles && n >= a.tpp && n < a.n_out;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float p = 0.0f;
        if (live) { // only a counted column is mixed
          const WbSum y = wb_iqc_mix(rr[t][i], ii[t][i], ri[t][i], ir[t][i], cR[i], cI[i], cQR[i], cQI[i], gain, cross);
          p = y.re * y.re + y.im * y.im;
        }
        pw[i] += p;
      }
    }
  } else { // k_bscan's
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
  }
  const size_t slot = 4 * (size_t)blockIdx.y + wave;
  wb_scan_reduce_store(pw, col, a.partial + (slot * gridDim.x + blockIdx.x) * 16 + 4 * g);
}

// launch_bscan with the estimator ahead (any_auto) and k_scan_bank_iqc in k_bscan's place
int launch_bscan_iqc(const BscanArgs &a0, const WbbIqcArgs &q, int any_auto, void *stream) {
  if (!q.blk || !q.mode || !q.tsum) return FMX_E_INVALID;
  if (any_auto) {
    const int rc = launch_wbb_iqc_estimate(a0.in, a0.wide_stride, (long)a0.n_out * a0.D, a0.s16, a0.S, q, stream);
    if (rc != FMX_OK) return rc;
  }
  return bscan_run(a0, stream, [=](const BscanArgs &a, size_t smem, dim3 grid, hipStream_t st) {
    return WB_LAUNCH(k_scan_bank_iqc, a.s16, (a.D & 1) == 0, grid, smem, st, a, q.blk, q.mode, q.tsum);
  });
}
