/* ================================================================== */
/* k_wb_scan: the band scan (fmx_wb_scan_process, DESIGN.md section 19) */
/* ================================================================== */
/* One call is one read of every scan point: with y_p[n] the channelizer's
 * output of a channel tuned to point p (fmx_wb.inc), x indexed from the
 * call's first sample,
 *   P_p = 1 / (n_out - tpp) sum_{n = tpp}^{n_out - 1} |y_p[n]|^2
 * -- |y| needs no rotation, and the outputs n < tpp, whose windows reach before
 * the call, are left out, so there is no history.  k_wb's operand layout,
 * weight rows and products (hi*hi, hi*lo, lo*hi per K step, raw integer
 * samples as exact f16) carry over; what differs:
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
#define WB_SCAN_NT 4 // tiles per workgroup (and per wave) at most

// v rotated right within its row of 16 lanes (DPP row_ror: CTRL = 0x120 + lanes)
template <int CTRL> static __device__ __forceinline__ float wb_row_ror(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, false));
}

template <bool S16, bool EVEN> __global__ __launch_bounds__(256) void k_wb_scan(WbScanArgs a) {
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

// hard- and near-clipped raw samples of the call (signal_level.cpp:172-177 on
// bytes; an int16 by its top byte, b = (v >> 8) + 128): every sample once,
// 2048 per workgroup, the counts to clip[workgroup][2]
template <typename T> __global__ __launch_bounds__(256) void k_wb_scan_clip(WbScanArgs a) {
  __shared__ uint32_t red[4][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long n_in = (long)a.n_out * a.D;
  const T *in = static_cast<const T *>(a.in);
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
  if (tid < 2) a.clip[2 * (size_t)blockIdx.x + tid] = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
}

// One lane per point: its partials over the workgroups in index order, in
// double, to the record by signal_level_eval's formulas (rms^2 = 0.5 P: the
// reference's 0.5 (varI + varQ) without the mean removal of one tuned read,
// which a shared capture has no counterpart of) and smoothSignalLevel.
__global__ __launch_bounds__(64) void k_wb_scan_level(WbScanArgs a) {
  const int p = (int)blockIdx.x * 64 + threadIdx.x;
  if (p >= a.P) return;
  const float *pp = a.partial + (size_t)(p >> 4) * a.nwg * 16 + (p & 15);
  double sum = 0.0;
  for (int wg = 0; wg < a.nwg; ++wg) sum += (double)pp[(size_t)wg * 16];
  unsigned long long hard = 0, nearc = 0;
  for (int k = 0; k < a.nclip; ++k) {
    hard += a.clip[2 * k];
    nearc += a.clip[2 * k + 1];
  }
  const double nn = (double)((long)a.n_out * a.D);
  const double pw = sum * a.pscale / (double)(a.n_out - a.tpp);
  const double *sp = a.sp; // gain*factor, bias, floor, ceil
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
  // smoothSignalLevel (signal_level.cpp:206-214)
  float *sm = a.sm + 2 * (size_t)p;
  if (sm[1] == 0.0f) {
    sm[0] = r.level120;
    sm[1] = 1.0f;
  } else {
    const float alpha = (r.level120 > sm[0]) ? 0.42f : 0.18f;
    sm[0] += (r.level120 - sm[0]) * alpha;
  }
  r.level120_smoothed = sm[0];
  a.level[p] = r;
}

template <bool S16, bool EVEN> static int wb_scan_launch(const WbScanArgs &a, size_t smem, dim3 grid, hipStream_t st) {
  static bool configured = false;
  if (!configured) {
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(&k_wb_scan<S16, EVEN>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, WB_LDS_MAX) != hipSuccess)
      return FMX_E_HIP;
    configured = true;
  }
  hipLaunchKernelGGL((k_wb_scan<S16, EVEN>), grid, dim3(256), smem, st, a);
  return hipGetLastError() == hipSuccess ? FMX_OK : FMX_E_HIP;
}

// tiles per workgroup: what the LDS budget holds, at most WB_SCAN_NT -- a
// function of the plan alone, so that a point's sum order is too
int wb_scan_tiles(int D, int Lp, int s16) {
  const long cap = WB_LDS_MAX / (s16 ? 8 : 4) - 8; // samples of the window
  const long nt = ((cap - Lp) / D + 1) / 16;
  return (int)std::min<long>(nt, WB_SCAN_NT);
}
int wb_scan_workgroups(int n_out, int tpp, int nt) { return (n_out - tpp + 16 * nt - 1) / (16 * nt); }
int wb_scan_clip_workgroups(long n_in) { return (int)((n_in + 2047) / 2048); }

int launch_wb_scan(const WbScanArgs &a0, void *stream) {
  WbScanArgs a = a0;
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
  if (a.s16) rc = even ? wb_scan_launch<true, true>(a, smem, grid, st) : wb_scan_launch<true, false>(a, smem, grid, st);
  else rc = even ? wb_scan_launch<false, true>(a, smem, grid, st) : wb_scan_launch<false, false>(a, smem, grid, st);
  if (rc != FMX_OK) return rc;
  hipLaunchKernelGGL(k_wb_scan_level, dim3((unsigned)((a.P + 63) / 64)), dim3(64), 0, st, a);
  return hipGetLastError() == hipSuccess ? FMX_OK : FMX_E_HIP;
}
