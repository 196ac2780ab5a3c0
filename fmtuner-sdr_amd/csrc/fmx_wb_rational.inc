/* ================================================================== */
/* k_wbr: the rational-rate channelizer (fmx_wb_create_rational,       */
/* DESIGN.md section 23)                                               */
/* ================================================================== */
/* wide_rate / dsp_rate = P / Q in lowest terms.  Output n = Q m + r ends at
 * wide sample i0 = m P + a_r (r P = Q a_r + b_r) and is
 *   y_c[n] = e^{-j theta_c(i0)} sum_j W_{c,r}[j] x[i0 - j],
 *   W_{c,r}[j] = Q 2 fc h[Q j + b_r] e^{+j 2 pi f_c j / Fs}:
 * Q integer channelizers of decimation P whose outputs interleave, each k_wb's
 * GEMM with its own rows.  The call's work is a flat list of tiles: tile
 * T = mb Q + r is the 16 outputs n = (16 mb + col) Q + r, all of phase r, their
 * windows P samples apart.
 *   rows (A)    the channel's phase-r rows [c][r][re hi, re lo, im hi, im lo][Lp]
 *               (entry kk = tap Lp - 1 - kk, zero from tap L_r on)
 *   columns (B) lane l holds output column l & 15 and the 8 samples from
 *               (16 (mb - mb0) + col) P + a_r + 32 ks + 8 (l >> 4) of the
 *               workgroup's LDS image, mb0 the mb of the workgroup's first tile
 *   K           Lp taps for every phase, 32 per step
 * The image, the chains and the rotation are the family's (fmx_wb_core.inc;
 * the rotation's sample index is i0); every output of a phase sums in the
 * same order wherever its tile falls, so rows do not depend on the call split
 * (a call is a multiple of Q outputs and starts at phase 0), and at Q = 1 the
 * rows are the integer object's.  A fragment starts on an even sample -- and
 * is read as dwords -- when P and a_r are both even; the other tiles read
 * element by element.  Workgroup w takes the tiles [w nt, (w + 1) nt) (tile t
 * on wave t & 3) and stages the window wbr_window() of them once.  k_wbr_hist
 * then keeps the last Lh - 1 raw samples, Lh the largest L_r. */
static_assert(kWbLdsMax == WB_LDS_MAX && kWbNtMax == WB_NT_MAX, "the host's tiling uses k_wb's limits");

// PEVEN: P is even, so a tile of an even a_r reads dwords
template <bool S16, bool PEVEN> __global__ __launch_bounds__(256) void k_wbr(WbrArgs a) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const WbrGroup wg = wbr_group((int)blockIdx.x, a.nt, a.ntiles, a.P, a.Q, a.a[a.Q - 1], a.Lp);
  const int T0 = wg.T0, T1 = wg.T1, mb0 = wg.mb0, NI = wg.window;
  const int NIp = (NI + 7) & ~7;
  const WbImage img = wb_image(NIp);
  wb_stage<S16, true>(img, NI, NIp, (long)mb0 * 16 * a.P - (a.Lp - 1), a.n_in, a.valid, a.in, a.hist, a.Lh, a.in_al, tid);
  const int col = lane & 15, g = lane >> 4;
  const int M = a.n_out / a.Q; // outputs per phase
  // a ragged last group computes its last channel again in the spare rows (not stored)
  const int ca = min(16 * (int)blockIdx.y + col, a.C - 1);
  for (int T = T0 + wave; T <= T1; T += 4) {
    const int mb = T / a.Q, r = T - mb * a.Q;
    const int ar = a.a[r];
    const uint16_t *wrow = a.w + ((size_t)ca * a.Q + r) * 4 * a.Lp + 8 * g;
    const int xb = wbr_tile_offset(a.P, a.Q, ar, T, mb0) + col * a.P + 8 * g;
    wb_f32x4 rr, ii, ri, ir;
    if (PEVEN && (ar & 1) == 0) wb_tile<S16, true>(img, xb, wrow, a.Lp, rr, ii, ri, ir);
    else wb_tile<S16, false>(img, xb, wrow, a.Lp, rr, ii, ri, ir);
    // lane: output (16 mb + col) Q + r of channels 16 group + 4 g + i
    const int m = 16 * mb + col;
    if (m >= M) continue;
    const int n = m * a.Q + r;
    const uint64_t i0 = (uint64_t)m * (uint64_t)a.P + (uint64_t)ar;
    const uint64_t smod = ((uint64_t)a.base_mod + i0) % a.fs; // the output's sample index mod Fs
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = 16 * (int)blockIdx.y + 4 * g + i;
      if (c >= a.C) break;
      wb_rotate_store(a.fpos[c], smod, a.fs, a.inv_fs, rr[i] - ii[i], ri[i] + ir[i], a.scale,
                      a.out + 2 * ((size_t)c * a.out_stride + n));
    }
  }
}

// the last Lh - 1 raw samples of (history, this call's input) into the other history buffer
template <typename T> __global__ void k_wbr_hist(WbrArgs a) {
  const int j = (int)blockIdx.x * 256 + threadIdx.x;
  if (j >= a.Lh - 1) return;
  const long i = a.n_in - (a.Lh - 1) + j;
  const T *src = i >= 0 ? static_cast<const T *>(a.in) + 2 * i : static_cast<const T *>(a.hist) + 2 * (j + a.n_in);
  T *dst = static_cast<T *>(a.hist_out) + 2 * (size_t)j;
  dst[0] = src[0];
  dst[1] = src[1];
}

int launch_wbr(const WbrArgs &a0, void *stream) {
  WbrArgs a = a0;
  if (a.C <= 0 || a.n_out <= 0) return FMX_OK;
  if (a.Q < 1 || a.Q > FMX_WBR_QMAX || a.P < 2 * a.Q || a.n_out % a.Q != 0 || a.Lh < 1 || a.Lp < a.Lh || (a.Lp & 31) ||
      a.valid < 0 || a.valid > a.Lh - 1)
    return FMX_E_INVALID;
  for (int r = 0; r < a.Q; ++r)
    if (a.a[r] != (int)((long)r * a.P / a.Q)) return FMX_E_INVALID;
  a.nt = wbr_tiles(a.P, a.Q, a.a[a.Q - 1], a.Lp, a.s16, a.n_out);
  if (a.nt < 1) return FMX_E_INVALID;
  a.ntiles = (a.n_out / a.Q + 15) / 16 * a.Q;
  a.n_in = (long)a.n_out / a.Q * a.P;
  a.in_al = wb_in_aligned(a.in, a.s16);
  // the largest window of any workgroup: nt tiles from the last phase on
  const int span = 1 + (a.nt - 1 + a.Q - 1) / a.Q;
  const int NI = wbr_window(a.P, a.a[a.Q - 1], a.Lp, 0, span - 1);
  const size_t smem = wb_lds_bytes(NI, a.s16);
  if (smem > WB_LDS_MAX) return FMX_E_INVALID;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)((a.ntiles + a.nt - 1) / a.nt), (unsigned)((a.C + 15) / 16));
  const int rc = WB_LAUNCH(k_wbr, a.s16, (a.P & 1) == 0, grid, smem, st, a);
  if (rc != FMX_OK) return rc;
  if (a.Lh > 1) {
    const dim3 hgrid((unsigned)((a.Lh - 1 + 255) / 256));
    if (a.s16) hipLaunchKernelGGL(k_wbr_hist<int16_t>, hgrid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_wbr_hist<uint8_t>, hgrid, dim3(256), 0, st, a);
  }
  return hipGetLastError() == hipSuccess ? FMX_OK : FMX_E_HIP;
}
