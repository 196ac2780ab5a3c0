/* ================================================================== */
/* k_wb: the wideband channelizer (fmx_wb_process, DESIGN.md section 18) */
/* ================================================================== */
/* y_c[n] = e^{-j theta_c(nD)} sum_k W_c[k] x[nD - k], W_c[k] = 2 fc h[k]
 * e^{+j 2 pi f_c k / Fs}: a complex GEMM of the channels' weights against
 * strided windows of the one wide signal, on v_mfma_f32_16x16x32_f16.
 *   rows (A)    16 channels; lane l holds channel l & 15, K entries
 *               8 (l >> 4) .. + 7: 16 B of the channel's weight rows
 *               [c][re hi, re lo, im hi, im lo][Lp] (entry kk = tap
 *               Lp - 1 - kk, so that K runs with the sample index)
 *   columns (B) 16 consecutive outputs; lane l holds output l & 15 and the 8
 *               consecutive samples from (16 t + col) D + 32 ks + 8 (l >> 4)
 *               of the workgroup's LDS image
 *   K           the Lp taps, 32 per step
 * Four f32 chains per tile (rr, ii, ri, ir), each hi*hi, hi*lo, lo*hi per K
 * step in that order (u8 data is one exact f16: hi*hi, lo*hi); re = rr - ii,
 * im = ri + ir.  Every output sums its taps in the same order wherever its
 * tile starts, so the rows do not depend on how a stream is cut into calls.
 * Workgroup = 16 channels x nt tiles of 16 outputs (4 waves, tile t on wave
 * t & 3): it stages the window of its (16 nt - 1) D + Lp wide samples once,
 * de-interleaved into f16 I / Q images (s16: hi + lo images; raw integers,
 * 2 b - 255 for u8 -- the scale is applied to the sums), from the call's
 * input and the raw history of the calls before.  The rotation's phase is
 * (f_c (i mod Fs)) mod Fs in 64-bit integers, i the output's wide-sample
 * index.  k_wb_hist then keeps the last L - 1 raw samples for the next call. */
#define WB_LDS_MAX (80 * 1024) // dynamic LDS per workgroup at most: two workgroups per CU
#define WB_NT_MAX 16           // tiles per workgroup at most (4 per wave)

typedef _Float16 wb_f16x8 __attribute__((ext_vector_type(8)));
typedef float wb_f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int wb_u32x4 __attribute__((ext_vector_type(4)));

// 8 consecutive f16 of an image: on dwords when every window starts on an
// even sample (D even), else one by one
template <bool EVEN> static __device__ __forceinline__ wb_f16x8 wb_frag(const _Float16 *p) {
  if (EVEN) {
    const uint32_t *q = reinterpret_cast<const uint32_t *>(p);
    return __builtin_bit_cast(wb_f16x8, wb_u32x4{q[0], q[1], q[2], q[3]});
  }
  wb_f16x8 v;
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = p[j];
  return v;
}

template <bool S16, bool EVEN> __global__ __launch_bounds__(256) void k_wb(WbArgs a) {
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
      const float re = rr[i] - ii[i], im = ri[i] + ir[i];
      float *po = a.out + 2 * ((size_t)c * a.out_stride + n);
      po[0] = (re * cs + im * sn) * a.scale; // (re + j im) e^{-j theta}
      po[1] = (im * cs - re * sn) * a.scale;
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

template <bool S16, bool EVEN> static int wb_launch(const WbArgs &a, size_t smem, dim3 grid, hipStream_t st) {
  static bool configured = false;
  if (!configured) {
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(&k_wb<S16, EVEN>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, WB_LDS_MAX) != hipSuccess)
      return FMX_E_HIP;
    configured = true;
  }
  hipLaunchKernelGGL((k_wb<S16, EVEN>), grid, dim3(256), smem, st, a);
  return hipGetLastError() == hipSuccess ? FMX_OK : FMX_E_HIP;
}

// tiles per workgroup: as many as the LDS budget holds, at most WB_NT_MAX and what the call needs
static int wb_tiles(const WbArgs &a) {
  const long cap = WB_LDS_MAX / (a.s16 ? 8 : 4) - 8; // samples of the window
  long nt = ((cap - a.Lp) / a.D + 1) / 16;
  nt = std::min<long>(nt, WB_NT_MAX);
  nt = std::min<long>(nt, (a.n_out + 15) / 16);
  return (int)nt;
}

int launch_wb(const WbArgs &a0, void *stream) {
  WbArgs a = a0;
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
  if (a.s16) rc = even ? wb_launch<true, true>(a, smem, grid, st) : wb_launch<true, false>(a, smem, grid, st);
  else rc = even ? wb_launch<false, true>(a, smem, grid, st) : wb_launch<false, false>(a, smem, grid, st);
  if (rc != FMX_OK) return rc;
  const dim3 hgrid((unsigned)((a.L - 1 + 255) / 256));
  if (a.s16) hipLaunchKernelGGL(k_wb_hist<int16_t>, hgrid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(k_wb_hist<uint8_t>, hgrid, dim3(256), 0, st, a);
  return hipGetLastError() == hipSuccess ? FMX_OK : FMX_E_HIP;
}
