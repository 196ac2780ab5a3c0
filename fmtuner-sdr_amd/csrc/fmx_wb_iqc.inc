/* ================================================================== */
/* DC offset and IQ imbalance of wide captures (fmx_wb_set_iq_correction,  */
/* fmx_wb_scan_set_iq_correction; DESIGN.md section 24)                     */
/* ================================================================== */
/* x' = (I - dc_i) + j (gain (Q - dc_q) + cross (I - dc_i)) is affine in the
 * raw samples, so the channelizer's output on x' is a recombination of the
 * four real sums k_wb and k_wb_scan keep apart (rr = sum Wr I, ii = sum Wi Q,
 * ri = sum Wr Q, ir = sum Wi I) plus a constant per channel: with SR + j SI
 * the sum of the channel's L taps and d_i, d_q the DC values in raw units,
 *   rI = rr - d_i SR   iI = ir - d_i SI   rQ = ri - d_q SR   iQ = ii - d_q SI
 *   re = rI - (gain iQ + cross iI)        im = (gain rQ + cross rI) + iI
 * k_wb_iqc and k_wb_scan_iqc are k_wb and k_wb_scan (fmx_wb.inc,
 * fmx_wb_scan.inc: the same staging, operand layout, accumulator chains and
 * product order) with that epilogue; they read the four parameters from the
 * object's FmxIqcBlock in device memory (wave-uniform, ahead of the K loop),
 * so nothing waits for the host.  The zeros before the stream's start are
 * corrected like every sample (x' = C(0)), which is what keeps the DC term a
 * constant.  The block is written on the same stream, ahead of the kernel:
 *   FIXED  k_iqc_fixed, once, when the mode is set
 *   AUTO   k_iqc_sums (the call's sum I, sum Q, sum I^2, sum Q^2, sum IQ as
 *          int64 partials per workgroup: exact, so independent of the grid)
 *          then k_iqc_finish (one thread: the partials in index order, the
 *          smoothing and Gram-Schmidt of fmx_iqc.h in double). */
#define IQC_WG_BYTES (64 * 1024) // raw bytes per k_iqc_sums workgroup: 16 loads of 16 B per thread

// one raw sample into the five sums
static __device__ __forceinline__ void iqc_acc(long long s[5], int vi, int vq) {
  s[0] += vi;
  s[1] += vq;
  s[2] += (long long)vi * vi;
  s[3] += (long long)vq * vq;
  s[4] += (long long)vi * vq;
}

// T = uint8_t: v = 2 b - 255; T = int16_t: v.  Workgroup w sums the samples
// [w SPW, (w + 1) SPW): by 16-B loads when the input is 16-B aligned (al16),
// sample by sample otherwise.  partial[w][5].
template <typename T> __global__ __launch_bounds__(256) void k_iqc_sums(const void *in, long n_in, int al16, long long *partial) {
  constexpr int SPV = 16 / (2 * (int)sizeof(T));        // samples per 16-B load
  constexpr long SPW = IQC_WG_BYTES / (2 * sizeof(T)); // samples per workgroup
  __shared__ long long red[4][5];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long s0 = (long)blockIdx.x * SPW, s1 = min(s0 + SPW, n_in);
  const T *p = static_cast<const T *>(in);
  long long s[5] = {0, 0, 0, 0, 0};
  long done = s0; // samples below it are summed by the wide loop
  if (al16) {     // s0 is a multiple of SPV: every 16-B word is aligned
    const long nv = (s1 - s0) / SPV;
    const wb_u32x4 *pv = reinterpret_cast<const wb_u32x4 *>(p + 2 * s0);
    for (long v = tid; v < nv; v += 256) {
      const wb_u32x4 w = pv[v];
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        if (sizeof(T) == 2) {
          iqc_acc(s, (int16_t)(w[d] & 0xFFFFu), (int16_t)(w[d] >> 16));
        } else {
          iqc_acc(s, 2 * (int)(w[d] & 0xFFu) - 255, 2 * (int)((w[d] >> 8) & 0xFFu) - 255);
          iqc_acc(s, 2 * (int)((w[d] >> 16) & 0xFFu) - 255, 2 * (int)(w[d] >> 24) - 255);
        }
      }
    }
    done = s0 + nv * SPV;
  }
  for (long i = done + tid; i < s1; i += 256) {
    const int vi = p[2 * i], vq = p[2 * i + 1];
    if (sizeof(T) == 2) iqc_acc(s, vi, vq);
    else iqc_acc(s, 2 * vi - 255, 2 * vq - 255);
  }
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    for (int d = 32; d >= 1; d >>= 1) s[j] += __shfl_xor(s[j], d);
    if (lane == 0) red[wave][j] = s[j];
  }
  __syncthreads();
  if (tid < 5) partial[5 * (size_t)blockIdx.x + tid] = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
}

__global__ __launch_bounds__(64) void k_iqc_finish(const long long *partial, int nwg, long n_in, double alpha, double unit,
                                                   FmxIqcBlock *blk) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  long long s[5] = {0, 0, 0, 0, 0};
  for (int w = 0; w < nwg; ++w)
#pragma unroll
    for (int j = 0; j < 5; ++j) s[j] += partial[5 * (size_t)w + j];
  FmxIqcBlock b = *blk;
  fmx_iqc_finish(s, n_in, alpha, unit, &b);
  *blk = b;
}

// FIXED (and the restart of AUTO, init = 0): the whole block
__global__ __launch_bounds__(64) void k_iqc_fixed(FmxIqcBlock *blk, FmxIqcBlock v) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  *blk = v;
}

int iqc_workgroups(long n_in, int s16) {
  const long spw = IQC_WG_BYTES / (s16 ? 4 : 2);
  return (int)((n_in + spw - 1) / spw);
}

int launch_iqc_set(FmxIqcBlock *blk, const FmxIqcBlock &v, void *stream) {
  if (!blk) return FMX_E_INVALID;
  hipLaunchKernelGGL(k_iqc_fixed, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), blk, v);
  return hipGetLastError() == hipSuccess ? FMX_OK : FMX_E_HIP;
}

int launch_iqc_estimate(const void *in, long n_in, int s16, double alpha, long long *partial, FmxIqcBlock *blk, void *stream) {
  if (!in || !partial || !blk || n_in < 1 || !(alpha > 0.0 && alpha <= 1.0)) return FMX_E_INVALID;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int nwg = iqc_workgroups(n_in, s16);
  const int al16 = (reinterpret_cast<uintptr_t>(in) & 15) == 0;
  if (s16) hipLaunchKernelGGL(k_iqc_sums<int16_t>, dim3((unsigned)nwg), dim3(256), 0, st, in, n_in, al16, partial);
  else hipLaunchKernelGGL(k_iqc_sums<uint8_t>, dim3((unsigned)nwg), dim3(256), 0, st, in, n_in, al16, partial);
  if (hipGetLastError() != hipSuccess) return FMX_E_HIP;
  hipLaunchKernelGGL(k_iqc_finish, dim3(1), dim3(64), 0, st, partial, nwg, n_in, alpha, s16 ? 32768.0 : 255.0, blk);
  return hipGetLastError() == hipSuccess ? FMX_OK : FMX_E_HIP;
}

/* ---- the corrected channelizer: k_wb with the epilogue above ---- */
// tsum[c] = (SR, SI): the sums of channel c's taps as its weight rows hold them
template <bool S16, bool EVEN>
__global__ __launch_bounds__(256) void k_wb_iqc(WbArgs a, const FmxIqcBlock *iqc, const float *tsum) {
  extern __shared__ __attribute__((aligned(16))) unsigned char wb_smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n0 = (int)blockIdx.x * 16 * a.nt; // first output of the workgroup
  const int NI = (16 * a.nt - 1) * a.D + a.Lp; // samples of the window
  const int NIp = (NI + 7) & ~7;
  _Float16 *ih = reinterpret_cast<_Float16 *>(wb_smem);
  _Float16 *qh = ih + NIp, *il = qh + NIp, *ql = il + NIp; // il, ql: s16 only
  // image entry idx = wide sample a0 + idx of this call (negative: the history)
  const long a0 = (long)n0 * a.D - (a.Lp - 1);
  const long n_in = (long)a.n_out * a.D;
  for (int idx = tid; idx < NIp; idx += 256) {
    const long i = a0 + idx;
    int vi = 0, vq = 0; // before the stream's start and past the call's input: zeros
    if (idx < NI && i >= -(long)a.valid && i < n_in) {
      if (S16) {
        const int16_t *src = i < 0 ? static_cast<const int16_t *>(a.hist) + 2 * (a.L - 1 + i)
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
        const uint8_t *src = i < 0 ? static_cast<const uint8_t *>(a.hist) + 2 * (a.L - 1 + i)
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
  // the call's parameters: one uniform load per wave, ahead of the K loop
  const float d_i = iqc->k[0], d_q = iqc->k[1], gain = iqc->k[2], cross = iqc->k[3];
  const int col = lane & 15, g = lane >> 4;
  const int KS = a.Lp >> 5;
  // a ragged last group computes its last channel again in the spare rows (not stored)
  const int ca = min(16 * (int)blockIdx.y + col, a.C - 1);
  const uint16_t *wrow = a.w + (size_t)ca * 4 * a.Lp + 8 * g;
  auto wld = [&](int ks, int part) __attribute__((always_inline)) {
    return *reinterpret_cast<const wb_u32x4 *>(wrow + (size_t)part * a.Lp + 32 * ks);
  };
  for (int t = wave; t < a.nt; t += 4) {
    const int nt0 = n0 + 16 * t;
    if (nt0 >= a.n_out) break;
    const int xb = (16 * t + col) * a.D + 8 * g;
    wb_f32x4 rr = {0.0f, 0.0f, 0.0f, 0.0f}, ii = rr, ri = rr, ir = rr;
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
    // lane: output nt0 + col of channels 16 group + 4 g + i
    const int n = nt0 + col;
    if (n >= a.n_out) continue;
    const uint64_t smod = ((uint64_t)a.base_mod + (uint64_t)n * (uint64_t)a.D) % a.fs; // the output's sample index mod Fs
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = 16 * (int)blockIdx.y + 4 * g + i;
      if (c >= a.C) break;
      const uint64_t p = ((uint64_t)a.fpos[c] * smod) % a.fs; // theta = p / Fs turns
      const double turns = (double)p * a.inv_fs;
      const int quad = (int)(4.0 * turns + 0.5); // 0..4
      const float r = (float)(turns - 0.25 * (double)quad); // |r| <= 1/8 turn
      float sn, cs;
      sincospif(2.0f * r, &sn, &cs);
      if (quad & 1) { // a quarter turn more: (cos, sin) -> (-sin, cos)
        const float tmp = cs;
        cs = -sn;
        sn = tmp;
      }
      if (quad & 2) {
        cs = -cs;
        sn = -sn;
      }
      const float SR = tsum[2 * c], SI = tsum[2 * c + 1];
      const float rI = rr[i] - d_i * SR, iI = ir[i] - d_i * SI;
      const float rQ = ri[i] - d_q * SR, iQ = ii[i] - d_q * SI;
      const float re = rI - (gain * iQ + cross * iI), im = (gain * rQ + cross * rI) + iI;
      float *po = a.out + 2 * ((size_t)c * a.out_stride + n);
      po[0] = (re * cs + im * sn) * a.scale; // (re + j im) e^{-j theta}
      po[1] = (im * cs - re * sn) * a.scale;
    }
  }
}

template <bool S16, bool EVEN>
static int wb_iqc_launch(const WbArgs &a, const FmxIqcBlock *iqc, const float *tsum, size_t smem, dim3 grid, hipStream_t st) {
  static bool configured = false;
  if (!configured) {
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(&k_wb_iqc<S16, EVEN>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, WB_LDS_MAX) != hipSuccess)
      return FMX_E_HIP;
    configured = true;
  }
  hipLaunchKernelGGL((k_wb_iqc<S16, EVEN>), grid, dim3(256), smem, st, a, iqc, tsum);
  return hipGetLastError() == hipSuccess ? FMX_OK : FMX_E_HIP;
}

// launch_wb with k_wb_iqc in k_wb's place: the same checks, tiling, grid and history kernel
int launch_wb_iqc(const WbArgs &a0, const FmxIqcBlock *iqc, const float *tsum, void *stream) {
  WbArgs a = a0;
  if (!iqc || !tsum) return FMX_E_INVALID;
  if (a.C <= 0 || a.n_out <= 0) return FMX_OK;
  if (a.D < 2 || a.L != (a.L / a.D) * a.D || a.Lp < a.L || (a.Lp & 31) || a.valid < 0 || a.valid > a.L - 1)
    return FMX_E_INVALID;
  a.nt = wb_tiles(a);
  if (a.nt < 1) return FMX_E_INVALID;
  const uintptr_t al = a.s16 ? 3 : 1;
  a.in_al = (reinterpret_cast<uintptr_t>(a.in) & al) == 0;
  const int NI = (16 * a.nt - 1) * a.D + a.Lp;
  const size_t smem = (size_t)((NI + 7) & ~7) * (a.s16 ? 8 : 4);
  if (smem > WB_LDS_MAX) return FMX_E_INVALID;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)((a.n_out + 16 * a.nt - 1) / (16 * a.nt)), (unsigned)((a.C + 15) / 16));
  const bool even = (a.D & 1) == 0;
  int rc;
  if (a.s16) rc = even ? wb_iqc_launch<true, true>(a, iqc, tsum, smem, grid, st) : wb_iqc_launch<true, false>(a, iqc, tsum, smem, grid, st);
  else rc = even ? wb_iqc_launch<false, true>(a, iqc, tsum, smem, grid, st) : wb_iqc_launch<false, false>(a, iqc, tsum, smem, grid, st);
  if (rc != FMX_OK) return rc;
  const dim3 hgrid((unsigned)((a.L - 1 + 255) / 256));
  if (a.s16) hipLaunchKernelGGL(k_wb_hist<int16_t>, hgrid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(k_wb_hist<uint8_t>, hgrid, dim3(256), 0, st, a);
  return hipGetLastError() == hipSuccess ? FMX_OK : FMX_E_HIP;
}

/* ---- the corrected scan: k_wb_scan with the epilogue above, then re^2 + im^2 ---- */
// every output from tpp on has its whole window inside the call, so the
// constant d SR is exact here too.  tsum[p] = (SR, SI) of point p.
template <bool S16, bool EVEN>
__global__ __launch_bounds__(256) void k_wb_scan_iqc(WbScanArgs a, const FmxIqcBlock *iqc, const float *tsum) {
  extern __shared__ __attribute__((aligned(16))) unsigned char wb_smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n0 = a.tpp + (int)blockIdx.x * 16 * a.nt; // first output of the workgroup
  const int NI = (16 * a.nt - 1) * a.D + a.Lp;       // samples of the window
  const int NIp = (NI + 7) & ~7;
  _Float16 *ih = reinterpret_cast<_Float16 *>(wb_smem);
  _Float16 *qh = ih + NIp, *il = qh + NIp, *ql = il + NIp; // il, ql: s16 only
  // image entry idx = wide sample a0 + idx of this call; a0 >= L - Lp + 1 > -32,
  // and the entries before sample 0 meet the rows' zero padding only
  const long a0 = (long)n0 * a.D - (a.Lp - 1);
  const long n_in = (long)a.n_out * a.D;
  for (int idx = tid; idx < NIp; idx += 256) {
    const long i = a0 + idx;
    int vi = 0, vq = 0; // outside the call's input: zeros
    if (idx < NI && i >= 0 && i < n_in) {
      if (S16) {
        const int16_t *src = static_cast<const int16_t *>(a.in) + 2 * i;
        if (a.in_al) {
          const uint32_t v = *reinterpret_cast<const uint32_t *>(src);
          vi = (int16_t)(v & 0xFFFFu);
          vq = (int16_t)(v >> 16);
        } else {
          vi = src[0];
          vq = src[1];
        }
      } else {
        const uint8_t *src = static_cast<const uint8_t *>(a.in) + 2 * i;
        uint32_t bi, bq;
        if (a.in_al) {
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
  const int grp = 4 * (int)blockIdx.y + wave; // the wave's point group
  if (16 * grp >= a.P) return;
  // the read's parameters: one uniform load per wave, ahead of the K loop
  const float d_i = iqc->k[0], d_q = iqc->k[1], gain = iqc->k[2], cross = iqc->k[3];
  const int col = lane & 15, g = lane >> 4;
  const int KS = a.Lp >> 5;
  // a ragged last group computes its last point again in the spare rows (not read)
  const int pa = min(16 * grp + col, a.P - 1);
  const uint16_t *wrow = a.w + (size_t)pa * 4 * a.Lp + 8 * g;
  auto wld = [&](int ks, int part) __attribute__((always_inline)) {
    return *reinterpret_cast<const wb_u32x4 *>(wrow + (size_t)part * a.Lp + 32 * ks);
  };
  // tiles of the workgroup that hold an output below n_out (wave-uniform)
  const int tiles = min(a.nt, (a.n_out - n0 + 15) >> 4);
  const wb_f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
  wb_f32x4 rr[WB_SCAN_NT], ii[WB_SCAN_NT], ri[WB_SCAN_NT], ir[WB_SCAN_NT];
#pragma unroll
  for (int t = 0; t < WB_SCAN_NT; ++t) rr[t] = ii[t] = ri[t] = ir[t] = zero;
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
#pragma unroll
    for (int t = 0; t < WB_SCAN_NT; ++t) {
      if (t < tiles) {
        const int x = (16 * t + col) * a.D + 8 * g + 32 * ks;
        const wb_f16x8 xih = wb_frag<EVEN>(ih + x), xqh = wb_frag<EVEN>(qh + x);
        rr[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wrh, xih, rr[t], 0, 0, 0);
        ii[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wih, xqh, ii[t], 0, 0, 0);
        ri[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wrh, xqh, ri[t], 0, 0, 0);
        ir[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wih, xih, ir[t], 0, 0, 0);
        if (S16) {
          const wb_f16x8 xil = wb_frag<EVEN>(il + x), xql = wb_frag<EVEN>(ql + x);
          rr[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wrh, xil, rr[t], 0, 0, 0);
          ii[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wih, xql, ii[t], 0, 0, 0);
          ri[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wrh, xql, ri[t], 0, 0, 0);
          ir[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wih, xil, ir[t], 0, 0, 0);
        }
        rr[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wrl, xih, rr[t], 0, 0, 0);
        ii[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wil, xqh, ii[t], 0, 0, 0);
        ri[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wrl, xqh, ri[t], 0, 0, 0);
        ir[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wil, xih, ir[t], 0, 0, 0);
      }
    }
  }
  // lane: output n0 + 16 t + col of points 16 grp + 4 g + i; the constants of its four points
  float cR[4], cI[4], cQR[4], cQI[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int p = min(16 * grp + 4 * g + i, a.P - 1);
    const float SR = tsum[2 * p], SI = tsum[2 * p + 1];
    cR[i] = d_i * SR;
    cI[i] = d_i * SI;
    cQR[i] = d_q * SR;
    cQI[i] = d_q * SI;
  }
  float pw[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int t = 0; t < WB_SCAN_NT; ++t) {
    const int n = n0 + 16 * t + col;
    const bool live = t < tiles && n >= a.tpp && n < a.n_out;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float rI = rr[t][i] - cR[i], iI = ir[t][i] - cI[i];
      const float rQ = ri[t][i] - cQR[i], iQ = ii[t][i] - cQI[i];
      const float re = rI - (gain * iQ + cross * iI), im = (gain * rQ + cross * rI) + iI;
      pw[i] += live ? re * re + im * im : 0.0f;
    }
  }
  // the 16 columns are the 16 lanes of a DPP row: rotate by 8, 4, 2, 1 and add
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    pw[i] += wb_row_ror<0x128>(pw[i]);
    pw[i] += wb_row_ror<0x124>(pw[i]);
    pw[i] += wb_row_ror<0x122>(pw[i]);
    pw[i] += wb_row_ror<0x121>(pw[i]);
  }
  if (col == 0) {
    float *po = a.partial + ((size_t)grp * gridDim.x + blockIdx.x) * 16 + 4 * g;
#pragma unroll
    for (int i = 0; i < 4; ++i) po[i] = pw[i];
  }
}

template <bool S16, bool EVEN>
static int wb_scan_iqc_launch(const WbScanArgs &a, const FmxIqcBlock *iqc, const float *tsum, size_t smem, dim3 grid,
                              hipStream_t st) {
  static bool configured = false;
  if (!configured) {
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(&k_wb_scan_iqc<S16, EVEN>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, WB_LDS_MAX) != hipSuccess)
      return FMX_E_HIP;
    configured = true;
  }
  hipLaunchKernelGGL((k_wb_scan_iqc<S16, EVEN>), grid, dim3(256), smem, st, a, iqc, tsum);
  return hipGetLastError() == hipSuccess ? FMX_OK : FMX_E_HIP;
}

// launch_wb_scan with k_wb_scan_iqc in k_wb_scan's place (the clip and level kernels are the scan's)
int launch_wb_scan_iqc(const WbScanArgs &a0, const FmxIqcBlock *iqc, const float *tsum, void *stream) {
  WbScanArgs a = a0;
  if (!iqc || !tsum) return FMX_E_INVALID;
  if (a.P <= 0 || a.D < 2 || a.tpp < 1 || a.Lp < a.D * a.tpp || (a.Lp & 31) || a.n_out <= a.tpp) return FMX_E_INVALID;
  a.nt = wb_scan_tiles(a.D, a.Lp, a.s16);
  if (a.nt < 1) return FMX_E_INVALID;
  a.nwg = wb_scan_workgroups(a.n_out, a.tpp, a.nt);
  a.nclip = wb_scan_clip_workgroups((long)a.n_out * a.D);
  const uintptr_t al = a.s16 ? 3 : 1;
  a.in_al = (reinterpret_cast<uintptr_t>(a.in) & al) == 0;
  const int NI = (16 * a.nt - 1) * a.D + a.Lp;
  const size_t smem = (size_t)((NI + 7) & ~7) * (a.s16 ? 8 : 4);
  if (smem > WB_LDS_MAX) return FMX_E_INVALID;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (a.s16) hipLaunchKernelGGL(k_wb_scan_clip<int16_t>, dim3((unsigned)a.nclip), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(k_wb_scan_clip<uint8_t>, dim3((unsigned)a.nclip), dim3(256), 0, st, a);
  if (hipGetLastError() != hipSuccess) return FMX_E_HIP;
  const dim3 grid((unsigned)a.nwg, (unsigned)((a.P + 63) / 64));
  const bool even = (a.D & 1) == 0;
  int rc;
  if (a.s16)
    rc = even ? wb_scan_iqc_launch<true, true>(a, iqc, tsum, smem, grid, st) : wb_scan_iqc_launch<true, false>(a, iqc, tsum, smem, grid, st);
  else
    rc = even ? wb_scan_iqc_launch<false, true>(a, iqc, tsum, smem, grid, st) : wb_scan_iqc_launch<false, false>(a, iqc, tsum, smem, grid, st);
  if (rc != FMX_OK) return rc;
  hipLaunchKernelGGL(k_wb_scan_level, dim3((unsigned)((a.P + 63) / 64)), dim3(64), 0, st, a);
  return hipGetLastError() == hipSuccess ? FMX_OK : FMX_E_HIP;
}
