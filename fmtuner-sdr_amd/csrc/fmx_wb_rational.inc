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
 * Chains, order per K step, raw-integer images, scale and rotation are k_wb's
 * (the rotation's sample index is i0); every output of a phase sums in the
 * same order wherever its tile falls, so rows do not depend on the call split
 * (a call is a multiple of Q outputs and starts at phase 0).  A fragment
 * starts on an even sample -- and is read as dwords -- when P and a_r are both
 * even; the other tiles read element by element.  Workgroup w takes the tiles
 * [w nt, (w + 1) nt) (tile t on wave t & 3) and stages the window
 * wbr_window() of them once.  k_wbr_hist then keeps the last Lh - 1 raw
 * samples, Lh the largest L_r. */
static_assert(kWbLdsMax == WB_LDS_MAX && kWbNtMax == WB_NT_MAX, "the host's tiling uses k_wb's limits");

template <bool S16, bool EVEN>
static __device__ __forceinline__ void wbr_tile(const _Float16 *ih, const _Float16 *qh, const _Float16 *il,
                                                const _Float16 *ql, int xb, const uint16_t *wrow, int Lp, wb_f32x4 &rr,
                                                wb_f32x4 &ii, wb_f32x4 &ri, wb_f32x4 &ir) {
  const int KS = Lp >> 5;
  auto wld = [&](int ks, int part) __attribute__((always_inline)) {
    return *reinterpret_cast<const wb_u32x4 *>(wrow + (size_t)part * Lp + 32 * ks);
  };
  wb_u32x4 n_rh = wld(0, 0), n_rl = wld(0, 1), n_ih = wld(0, 2), n_il = wld(0, 3);
  for (int ks = 0; ks < KS; ++ks) {
    const wb_f16x8 wrh = __builtin_bit_cast(wb_f16x8, n_rh), wrl = __builtin_bit_cast(wb_f16x8, n_rl);
    const wb_f16x8 wih = __builtin_bit_cast(wb_f16x8, n_ih), wil = __builtin_bit_cast(wb_f16x8, n_il);
    if (ks + 1 < KS) {
      n_rh = wld(ks + 1, 0);
      n_rl = wld(ks + 1, 1);
      n_ih = wld(ks + 1, 2);
      n_il = wld(ks + 1, 3);
    }
    const int x = xb + 32 * ks;
    const wb_f16x8 xih = wb_frag<EVEN>(ih + x), xqh = wb_frag<EVEN>(qh + x);
    rr = __builtin_amdgcn_mfma_f32_16x16x32_f16(wrh, xih, rr, 0, 0, 0);
    ii = __builtin_amdgcn_mfma_f32_16x16x32_f16(wih, xqh, ii, 0, 0, 0);
    ri = __builtin_amdgcn_mfma_f32_16x16x32_f16(wrh, xqh, ri, 0, 0, 0);
    ir = __builtin_amdgcn_mfma_f32_16x16x32_f16(wih, xih, ir, 0, 0, 0);
    if (S16) {
      const wb_f16x8 xil = wb_frag<EVEN>(il + x), xql = wb_frag<EVEN>(ql + x);
      rr = __builtin_amdgcn_mfma_f32_16x16x32_f16(wrh, xil, rr, 0, 0, 0);
      ii = __builtin_amdgcn_mfma_f32_16x16x32_f16(wih, xql, ii, 0, 0, 0);
      ri = __builtin_amdgcn_mfma_f32_16x16x32_f16(wrh, xql, ri, 0, 0, 0);
      ir = __builtin_amdgcn_mfma_f32_16x16x32_f16(wih, xil, ir, 0, 0, 0);
    }
    rr = __builtin_amdgcn_mfma_f32_16x16x32_f16(wrl, xih, rr, 0, 0, 0);
    ii = __builtin_amdgcn_mfma_f32_16x16x32_f16(wil, xqh, ii, 0, 0, 0);
    ri = __builtin_amdgcn_mfma_f32_16x16x32_f16(wrl, xqh, ri, 0, 0, 0);
    ir = __builtin_amdgcn_mfma_f32_16x16x32_f16(wil, xih, ir, 0, 0, 0);
  }
}

// PEVEN: P is even, so a tile of an even a_r reads dwords
template <bool S16, bool PEVEN> __global__ __launch_bounds__(256) void k_wbr(WbrArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char wb_smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const WbrGroup wg = wbr_group((int)blockIdx.x, a.nt, a.ntiles, a.P, a.Q, a.a[a.Q - 1], a.Lp);
  const int T0 = wg.T0, T1 = wg.T1, mb0 = wg.mb0, NI = wg.window;
  const int NIp = (NI + 7) & ~7;
  _Float16 *ih = reinterpret_cast<_Float16 *>(wb_smem);
  _Float16 *qh = ih + NIp, *il = qh + NIp, *ql = il + NIp; // il, ql: s16 only
  // image entry idx = wide sample a0 + idx of this call (negative: the history)
  const long a0 = (long)mb0 * 16 * a.P - (a.Lp - 1);
  const long n_in = a.n_in;
  for (int idx = tid; idx < NIp; idx += 256) {
    const long i = a0 + idx;
    int vi = 0, vq = 0; // before the stream's start and past the call's input: zeros
    if (idx < NI && i >= -(long)a.valid && i < n_in) {
      if (S16) {
        const int16_t *src = i < 0 ? static_cast<const int16_t *>(a.hist) + 2 * (a.Lh - 1 + i)
                                   : static_cast<const int16_t *>(a.in) + 2 * i;
        if (i < 0 || a.in_al) {
          const uint32_t v = *reinterpret_cast<const uint32_t *>(src);
          vi = (int16_t)(v & 0xFFFFu);
          vq = (int16_t)(v >> 16);
        } else {
          vi = src[0];
          vq = src[1];
        }
      } else {
        const uint8_t *src = i < 0 ? static_cast<const uint8_t *>(a.hist) + 2 * (a.Lh - 1 + i)
                                   : static_cast<const uint8_t *>(a.in) + 2 * i;
        uint32_t bi, bq;
        if (i < 0 || a.in_al) {
          const uint32_t v = *reinterpret_cast<const uint16_t *>(src);
          bi = v & 0xFFu;
          bq = v >> 8;
        } else {
          bi = src[0];
          bq = src[1];
        }
        vi = 2 * (int)bi - 255;
        vq = 2 * (int)bq - 255;
      }
    }
    const float fi = (float)vi, fq = (float)vq;
    const _Float16 hi = (_Float16)fi, hq = (_Float16)fq;
    ih[idx] = hi;
    qh[idx] = hq;
    if (S16) { // |v - hi| <= 8: exact
      il[idx] = (_Float16)(fi - (float)hi);
      ql[idx] = (_Float16)(fq - (float)hq);
    }
  }
  __syncthreads();
  const int col = lane & 15, g = lane >> 4;
  const int M = a.n_out / a.Q; // outputs per phase
  // a ragged last group computes its last channel again in the spare rows (not stored)
  const int ca = min(16 * (int)blockIdx.y + col, a.C - 1);
  for (int T = T0 + wave; T <= T1; T += 4) {
    const int mb = T / a.Q, r = T - mb * a.Q;
    const int ar = a.a[r];
    const uint16_t *wrow = a.w + ((size_t)ca * a.Q + r) * 4 * a.Lp + 8 * g;
    const int xb = wbr_tile_offset(a.P, a.Q, ar, T, mb0) + col * a.P + 8 * g;
    wb_f32x4 rr = {0.0f, 0.0f, 0.0f, 0.0f}, ii = rr, ri = rr, ir = rr;
    if (PEVEN && (ar & 1) == 0) wbr_tile<S16, true>(ih, qh, il, ql, xb, wrow, a.Lp, rr, ii, ri, ir);
    else wbr_tile<S16, false>(ih, qh, il, ql, xb, wrow, a.Lp, rr, ii, ri, ir);
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
      const uint64_t p = ((uint64_t)a.fpos[c] * smod) % a.fs; // theta = p / Fs turns
      const double turns = (double)p * a.inv_fs;
      const int quad = (int)(4.0 * turns + 0.5); // 0..4
      const float rem = (float)(turns - 0.25 * (double)quad); // |rem| <= 1/8 turn
      float sn, cs;
      sincospif(2.0f * rem, &sn, &cs);
      if (quad & 1) { // a quarter turn more: (cos, sin) -> (-sin, cos)
        const float tmp = cs;
        cs = -sn;
        sn = tmp;
      }
      if (quad & 2) {
        cs = -cs;
        sn = -sn;
      }
      const float re = rr[i] - ii[i], im = ri[i] + ir[i];
      float *po = a.out + 2 * ((size_t)c * a.out_stride + n);
      po[0] = (re * cs + im * sn) * a.scale; // (re + j im) e^{-j theta}
      po[1] = (im * cs - re * sn) * a.scale;
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

template <bool S16, bool PEVEN> static int wbr_launch(const WbrArgs &a, size_t smem, dim3 grid, hipStream_t st) {
  static bool configured = false;
  if (!configured) {
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(&k_wbr<S16, PEVEN>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, WB_LDS_MAX) != hipSuccess)
      return FMX_E_HIP;
    configured = true;
  }
  hipLaunchKernelGGL((k_wbr<S16, PEVEN>), grid, dim3(256), smem, st, a);
  return hipGetLastError() == hipSuccess ? FMX_OK : FMX_E_HIP;
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
  const uintptr_t al = a.s16 ? 3 : 1;
  a.in_al = (reinterpret_cast<uintptr_t>(a.in) & al) == 0;
  // the largest window of any workgroup: nt tiles from the last phase on
  const int span = 1 + (a.nt - 1 + a.Q - 1) / a.Q;
  const int NI = wbr_window(a.P, a.a[a.Q - 1], a.Lp, 0, span - 1);
  const size_t smem = (size_t)((NI + 7) & ~7) * (a.s16 ? 8 : 4);
  if (smem > WB_LDS_MAX) return FMX_E_INVALID;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)((a.ntiles + a.nt - 1) / a.nt), (unsigned)((a.C + 15) / 16));
  const bool even = (a.P & 1) == 0;
  int rc;
  if (a.s16) rc = even ? wbr_launch<true, true>(a, smem, grid, st) : wbr_launch<true, false>(a, smem, grid, st);
  else rc = even ? wbr_launch<false, true>(a, smem, grid, st) : wbr_launch<false, false>(a, smem, grid, st);
  if (rc != FMX_OK) return rc;
  if (a.Lh > 1) {
    const dim3 hgrid((unsigned)((a.Lh - 1 + 255) / 256));
    if (a.s16) hipLaunchKernelGGL(k_wbr_hist<int16_t>, hgrid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_wbr_hist<uint8_t>, hgrid, dim3(256), 0, st, a);
  }
  return hipGetLastError() == hipSuccess ? FMX_OK : FMX_E_HIP;
}
