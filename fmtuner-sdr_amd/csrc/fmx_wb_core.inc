/* ================================================================== */
/* The wideband family's shared pieces (DESIGN.md section 25): what     */
/* k_wb, k_wb_scan, k_wbb, k_wbr, k_rbank, k_wb_iqc, k_wb_scan_iqc and  */
/* the level and clip kernels are put together from                     */
/* ================================================================== */
/* y_c[n] = e^{-j theta_c(i0)} sum_k W_c[k] x[i0 - k], W_c[k] = 2 fc h[k]
 * e^{+j 2 pi f_c k / Fs}, i0 the wide sample output n ends at: a complex GEMM
 * of the channels' weights against strided windows of the one wide signal, on
 * v_mfma_f32_16x16x32_f16.
 *   rows (A)    16 channels; lane l holds channel l & 15, K entries
 *               8 (l >> 4) .. + 7: 16 B of the channel's weight rows
 *               [re hi, re lo, im hi, im lo][Lp] (entry kk = tap Lp - 1 - kk,
 *               so that K runs with the sample index)
 *   columns (B) 16 outputs; lane l holds output l & 15 and the 8 consecutive
 *               samples from the output's window start + 32 ks + 8 (l >> 4) of
 *               the workgroup's LDS image
 *   K           the Lp taps, 32 per step
 * wb_stage writes the image: the workgroup's window of wide samples, once,
 * de-interleaved into f16 I / Q images (s16: hi + lo images; raw integers,
 * 2 b - 255 for u8 -- the scale is applied to the sums), from the call's input
 * and the raw history of the calls before.  wb_tile (one tile) and wb_scan_mac
 * (a wave's tiles over one read of the weights) run four f32 chains per tile
 * (rr, ii, ri, ir), each hi*hi, hi*lo, lo*hi per K step in that order (u8 data
 * is one exact f16: hi*hi, lo*hi); re = rr - ii, im = ri + ir.  Every output
 * sums its taps in the same order wherever its tile starts, so rows do not
 * depend on how a stream is cut into calls.  wb_rotate_store turns a sum by the
 * phase (f_c (i0 mod Fs)) mod Fs, in 64-bit integers, and stores it.
 * There is one definition of the image, of the chain order and of the
 * rotation: the kernels differ in where their window, weight rows and outputs
 * lie and in what they do with the sums, and in nothing these pieces hold. */
#define WB_LDS_MAX (80 * 1024) // dynamic LDS per workgroup at most: two workgroups per CU
#define WB_NT_MAX 16           // tiles per workgroup at most (4 per wave)
#define WB_SCAN_NT 4           // the scan's tiles per workgroup (and per wave) at most

typedef _Float16 wb_f16x8 __attribute__((ext_vector_type(8)));
typedef float wb_f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int wb_u32x4 __attribute__((ext_vector_type(4)));

// 8 consecutive f16 of an image: on dwords when every window starts on an
// even sample, else one by one
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

// the workgroup's dynamic LDS: four images of NIp entries (il, ql: s16 only)
extern __shared__ __attribute__((aligned(16))) unsigned char wb_smem[];
struct WbImage {
  _Float16 *ih, *qh, *il, *ql;
};
static __device__ __forceinline__ WbImage wb_image(int NIp) {
  _Float16 *ih = reinterpret_cast<_Float16 *>(wb_smem);
  return WbImage{ih, ih + NIp, ih + 2 * NIp, ih + 3 * NIp};
}

// Image entry idx = wide sample a0 + idx of this call, idx < NI; zeros before
// the stream's start, past the call's n_in samples and from NI to NIp.
// HIST: a negative sample is entry Lh - 1 + i of the history's Lh - 1 samples,
// of which the last `valid` exist (always whole samples: loaded at once).
// Without HIST there is nothing before sample 0 (the scan).
template <bool S16, bool HIST>
static __device__ __forceinline__ void wb_stage(const WbImage &m, int NI, int NIp, long a0, long n_in, int valid,
                                                const void *in, const void *hist, int Lh, int in_al, int tid) {
  for (int idx = tid; idx < NIp; idx += 256) {
    const long i = a0 + idx;
    int vi = 0, vq = 0;
    if (idx < NI && i >= (HIST ? -(long)valid : 0L) && i < n_in) {
      const bool old = HIST && i < 0;
      if (S16) {
        const int16_t *src = old ? static_cast<const int16_t *>(hist) + 2 * (Lh - 1 + i)
                                 : static_cast<const int16_t *>(in) + 2 * i;
        if (old || in_al) {
          const uint32_t v = *reinterpret_cast<const uint32_t *>(src);
          vi = (int16_t)(v & 0xFFFFu);
          vq = (int16_t)(v >> 16);
        } else {
          vi = src[0];
          vq = src[1];
        }
      } else {
        const uint8_t *src = old ? static_cast<const uint8_t *>(hist) + 2 * (Lh - 1 + i)
                                 : static_cast<const uint8_t *>(in) + 2 * i;
        uint32_t bi, bq;
        if (old || in_al) {
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
    m.ih[idx] = hi;
    m.qh[idx] = hq;
    if (S16) { // |v - hi| <= 8: exact
      m.il[idx] = (_Float16)(fi - (float)hi);
      m.ql[idx] = (_Float16)(fq - (float)hq);
    }
  }
  __syncthreads();
}

// one K step of one tile: the chains' products in their one order
template <bool S16, bool EVEN>
static __device__ __forceinline__ void wb_kstep(const WbImage &m, int x, wb_f16x8 wrh, wb_f16x8 wrl, wb_f16x8 wih,
                                                wb_f16x8 wil, wb_f32x4 &rr, wb_f32x4 &ii, wb_f32x4 &ri, wb_f32x4 &ir) {
  const wb_f16x8 xih = wb_frag<EVEN>(m.ih + x), xqh = wb_frag<EVEN>(m.qh + x);
  rr = __builtin_amdgcn_mfma_f32_16x16x32_f16(wrh, xih, rr, 0, 0, 0);
  ii = __builtin_amdgcn_mfma_f32_16x16x32_f16(wih, xqh, ii, 0, 0, 0);
  ri = __builtin_amdgcn_mfma_f32_16x16x32_f16(wrh, xqh, ri, 0, 0, 0);
  ir = __builtin_amdgcn_mfma_f32_16x16x32_f16(wih, xih, ir, 0, 0, 0);
  if (S16) {
    const wb_f16x8 xil = wb_frag<EVEN>(m.il + x), xql = wb_frag<EVEN>(m.ql + x);
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

// The K loop of one tile.  wrow: the lane's 16 B of its channel's four rows;
// xb: where the lane's window starts in the image.  The next step's weights
// are loaded ahead of this step's products.
template <bool S16, bool EVEN>
static __device__ __forceinline__ void wb_tile(const WbImage &m, int xb, const uint16_t *wrow, int Lp, wb_f32x4 &rr,
                                               wb_f32x4 &ii, wb_f32x4 &ri, wb_f32x4 &ir) {
  const int KS = Lp >> 5;
  auto wld = [&](int ks, int part) __attribute__((always_inline)) {
    return *reinterpret_cast<const wb_u32x4 *>(wrow + (size_t)part * Lp + 32 * ks);
  };
  rr = ii = ri = ir = wb_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
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
    wb_kstep<S16, EVEN>(m, xb + 32 * ks, wrh, wrl, wih, wil, rr, ii, ri, ir);
  }
}

// The scan's K loop: a wave's `tiles` <= WB_SCAN_NT tiles of 16 outputs, D
// apart from image entry 0 on, over one read of each weight fragment.
template <bool S16, bool EVEN>
static __device__ __forceinline__ void wb_scan_mac(const WbImage &m, const uint16_t *wrow, int Lp, int D, int col, int g,
                                                   int tiles, wb_f32x4 (&rr)[WB_SCAN_NT], wb_f32x4 (&ii)[WB_SCAN_NT],
                                                   wb_f32x4 (&ri)[WB_SCAN_NT], wb_f32x4 (&ir)[WB_SCAN_NT]) {
  const int KS = Lp >> 5;
  auto wld = [&](int ks, int part) __attribute__((always_inline)) {
    return *reinterpret_cast<const wb_u32x4 *>(wrow + (size_t)part * Lp + 32 * ks);
  };
  const wb_f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
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
    for (int t = 0; t < WB_SCAN_NT; ++t)
      if (t < tiles)
        wb_kstep<S16, EVEN>(m, (16 * t + col) * D + 8 * g + 32 * ks, wrh, wrl, wih, wil, rr[t], ii[t], ri[t], ir[t]);
  }
}

// v rotated right within its row of 16 lanes (DPP row_ror: CTRL = 0x120 + lanes)
template <int CTRL> static __device__ __forceinline__ float wb_row_ror(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, false));
}

// The scan's partial: a lane's four sums over its columns; the 16 columns are
// the 16 lanes of a DPP row: rotate by 8, 4, 2, 1 and add, column 0 stores.
static __device__ __forceinline__ void wb_scan_reduce_store(float (&pw)[4], int col, float *po) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    pw[i] += wb_row_ror<0x128>(pw[i]);
    pw[i] += wb_row_ror<0x124>(pw[i]);
    pw[i] += wb_row_ror<0x122>(pw[i]);
    pw[i] += wb_row_ror<0x121>(pw[i]);
  }
  if (col == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) po[i] = pw[i];
  }
}

// e^{-j theta} as (cos, sin) of theta = (fpos smod mod Fs) / Fs turns, smod the
// output's wide-sample index mod Fs
struct WbRot {
  float cs, sn;
};
static __device__ __forceinline__ WbRot wb_rotation(uint32_t fpos, uint64_t smod, uint32_t fs, double inv_fs) {
  const uint64_t p = ((uint64_t)fpos * smod) % fs;
  const double turns = (double)p * inv_fs;
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
  return WbRot{cs, sn};
}
// po[0..1] = (re + j im) e^{-j theta} scale
static __device__ __forceinline__ void wb_store(WbRot t, float re, float im, float scale, float *po) {
  po[0] = (re * t.cs + im * t.sn) * scale;
  po[1] = (im * t.cs - re * t.sn) * scale;
}
static __device__ __forceinline__ void wb_rotate_store(uint32_t fpos, uint64_t smod, uint32_t fs, double inv_fs, float re,
                                                       float im, float scale, float *po) {
  wb_store(wb_rotation(fpos, smod, fs, inv_fs), re, im, scale, po);
}

// The corrected sample's sums from the four chains (fmx_wb_iqc.inc): cR = d_i SR,
// cI = d_i SI, cQR = d_q SR, cQI = d_q SI, the DC terms of the channel
struct WbSum {
  float re, im;
};
static __device__ __forceinline__ WbSum wb_iqc_mix(float rr, float ii, float ri, float ir, float cR, float cI, float cQR,
                                                   float cQI, float gain, float cross) {
  const float rI = rr - cR, iI = ir - cI;
  const float rQ = ri - cQR, iQ = ii - cQI;
  return WbSum{rI - (gain * iQ + cross * iI), (gain * rQ + cross * rI) + iI};
}

/* ---- the level records' pieces (k_wb_scan_level, k_wb_level, k_wbb_level; the clip kernels) ---- */
// Hard- and near-clipped raw samples (signal_level.cpp:172-177 on bytes; an
// int16 by its top byte, b = (v >> 8) + 128) among the workgroup's 2048 of the
// n_in samples at `in`: the two counts to dst[0..1]
template <typename T> static __device__ __forceinline__ void wb_clip_count(const T *in, long n_in, uint32_t *dst) {
  __shared__ uint32_t red[4][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint32_t hard = 0, nearc = 0;
  for (int k = 0; k < 8; ++k) {
    const long i = (long)blockIdx.x * 2048 + 256 * k + tid;
    if (i >= n_in) break;
    uint32_t bi, bq;
    if (sizeof(T) == 2) {
      bi = (uint32_t)(((int)in[2 * i] >> 8) + 128);
      bq = (uint32_t)(((int)in[2 * i + 1] >> 8) + 128);
    } else {
      bi = (uint32_t)in[2 * i];
      bq = (uint32_t)in[2 * i + 1];
    }
    const uint32_t lo = min(bi, bq), hi = max(bi, bq);
    hard += (lo <= 1u || hi >= 254u) ? 1u : 0u;
    nearc += (lo <= 8u || hi >= 247u) ? 1u : 0u;
  }
  for (int d = 32; d >= 1; d >>= 1) {
    hard += __shfl_xor(hard, d);
    nearc += __shfl_xor(nearc, d);
  }
  if (lane == 0) {
    red[wave][0] = hard;
    red[wave][1] = nearc;
  }
  __syncthreads();
  if (tid < 2) dst[tid] = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
}

// sum |y[m]|^2, m < n, of one complex row by a workgroup of four waves; the
// sum is thread 0's return value.  The row is read as pairs of samples: thread
// t takes the pairs t, t + 256, ... and adds each pair's two terms
// re re + im im, formed and accumulated in double, in index order; the 64
// lanes of a wave are added in a butterfly (xor 32, 16, 8, 4, 2, 1), the four
// waves through LDS in index order.  The order is a function of n alone, not
// of the load width W (16 B per pair, 8 B per sample or 4 B per float).
template <int W> static __device__ __forceinline__ double wb_row_power(const float *row, int n) {
  __shared__ double red[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int np = (n + 1) >> 1; // pairs, the last one half empty at an odd n
  double acc = 0.0;
#pragma unroll 4
  for (int p = tid; p < np; p += 256) {
    const float *s = row + 4 * (size_t)p;
    const bool two = 2 * p + 1 < n; // nothing past sample n - 1 is read
    float r0, i0, r1 = 0.0f, i1 = 0.0f;
    if (W == 16 && two) {
      const float4 v = *reinterpret_cast<const float4 *>(s);
      r0 = v.x;
      i0 = v.y;
      r1 = v.z;
      i1 = v.w;
    } else if (W >= 8) {
      const float2 u = *reinterpret_cast<const float2 *>(s);
      r0 = u.x;
      i0 = u.y;
      if (two) {
        const float2 v = *reinterpret_cast<const float2 *>(s + 2);
        r1 = v.x;
        i1 = v.y;
      }
    } else {
      r0 = s[0];
      i0 = s[1];
      if (two) {
        r1 = s[2];
        i1 = s[3];
      }
    }
    acc += (double)r0 * (double)r0 + (double)i0 * (double)i0;
    if (two) acc += (double)r1 * (double)r1 + (double)i1 * (double)i1;
  }
  for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d);
  if (lane == 0) red[wave] = acc;
  __syncthreads();
  if (tid != 0) return 0.0;
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// One record from the mean power pw = sum pscale / count of a channel or point
// and the nclip clip partials of the call's nn raw samples, added in index
// order, by signal_level_eval's formulas (signal_level.cpp:187-195;
// rms^2 = 0.5 pw: the reference's 0.5 (varI + varQ) without the mean removal
// of one tuned read, which a shared capture has no counterpart of) and
// smoothSignalLevel (signal_level.cpp:206-214) on sm = {value, initialised}.
// sp: gain*factor, bias, floor, ceil.
static __device__ __forceinline__ fmx_signal_level wb_level_record(double sum, double pscale, double count,
                                                                   const uint32_t *clip, int nclip, double nn,
                                                                   const double *sp, float *sm) {
  unsigned long long hard = 0, nearc = 0;
  for (int k = 0; k < nclip; ++k) {
    hard += clip[2 * k];
    nearc += clip[2 * k + 1];
  }
  const double pw = sum * pscale / count;
  fmx_signal_level r;
  const double rms = sqrt(fmax(1e-15, 0.5 * pw));
  r.dbfs = 20.0 * log10(rms + 1e-12);
  r.compensated_dbfs = r.dbfs - sp[0] + sp[1];
  const double safeCeil = fmax(sp[3], sp[2] + 1.0);
  const double norm = (r.compensated_dbfs - sp[2]) / (safeCeil - sp[2]);
  const float l = (float)(norm * 120.0);
  r.level120 = l < 0.0f ? 0.0f : (l > 120.0f ? 120.0f : l);
  r.hard_clip_ratio = (double)hard / nn;
  r.near_clip_ratio = (double)nearc / nn;
  if (sm[1] == 0.0f) {
    sm[0] = r.level120;
    sm[1] = 1.0f;
  } else {
    const float alpha = (r.level120 > sm[0]) ? 0.42f : 0.18f;
    sm[0] += (r.level120 - sm[0]) * alpha;
  }
  r.level120_smoothed = sm[0];
  return r;
}

/* ---- host side ---- */
// Launch kernel K of 256 threads with `smem` bytes of dynamic LDS; its limit
// is raised to WB_LDS_MAX once per kernel.
template <auto K, class... A> static int wb_launch(dim3 grid, size_t smem, hipStream_t st, const A &...args) {
  static bool configured = false;
  if (!configured) {
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(K), hipFuncAttributeMaxDynamicSharedMemorySize, WB_LDS_MAX) !=
        hipSuccess)
      return FMX_E_HIP;
    configured = true;
  }
  hipLaunchKernelGGL(K, grid, dim3(256), smem, st, args...);
  return hipGetLastError() == hipSuccess ? FMX_OK : FMX_E_HIP;
}
// wb_launch of K<s16, even>
#define WB_LAUNCH(K, s16, even, ...)                                                                                  \
  ((s16) ? ((even) ? wb_launch<K<true, true>>(__VA_ARGS__) : wb_launch<K<true, false>>(__VA_ARGS__))                   \
         : ((even) ? wb_launch<K<false, true>>(__VA_ARGS__) : wb_launch<K<false, false>>(__VA_ARGS__)))

// bytes of the images of a window of NI samples
static size_t wb_lds_bytes(int NI, int s16) { return (size_t)((NI + 7) & ~7) * (s16 ? 8 : 4); }
// a whole raw sample (2 or 4 bytes) of `in` may be loaded at once
static int wb_in_aligned(const void *in, int s16) { return (reinterpret_cast<uintptr_t>(in) & (s16 ? 3 : 1)) == 0; }
// 16-output tiles, their windows D apart, that the LDS budget holds
static long wb_tiles_fit(int D, int Lp, int s16) {
  const long cap = WB_LDS_MAX / (s16 ? 8 : 4) - 8; // samples of the window
  return ((cap - Lp) / D + 1) / 16;
}
// tiles per workgroup: as many as the LDS budget holds, at most WB_NT_MAX and what the call needs
static int wb_tiles(int D, int Lp, int s16, int n_out) {
  return (int)std::min<long>({wb_tiles_fit(D, Lp, s16), (long)WB_NT_MAX, ((long)n_out + 15) / 16});
}
