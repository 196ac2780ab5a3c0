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
 * k_wb_iqc and k_wb_scan_iqc put the family's pieces together as k_wb and
 * k_wb_scan do (fmx_wb_core.inc: one image, one chain order, one rotation)
 * and pass the four sums through wb_iqc_mix where those form rr - ii and
 * ri + ir (an object in OFF launches k_wb / k_wb_scan themselves); they read
 * the four parameters from the
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

// T = uint8_t: v = 2 b - 255; T = int16_t: v.  Workgroup blockIdx.x sums the
// samples [w SPW, (w + 1) SPW) of the n_in at `in`: by 16-B loads when the
// input is 16-B aligned (al16), sample by sample otherwise.  dst[5].
// (k_iqc_sums; k_bank_iqc_sums of fmx_wb_bank_iqc.inc on a capture's row)
template <typename T> static __device__ __forceinline__ void iqc_sum_workgroup(const void *in, long n_in, int al16, long long *dst) {
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
  if (tid < 5) dst[tid] = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
}

// partial[w][5]
template <typename T> __global__ __launch_bounds__(256) void k_iqc_sums(const void *in, long n_in, int al16, long long *partial) {
  iqc_sum_workgroup<T>(in, n_in, al16, partial + 5 * (size_t)blockIdx.x);
}

// one thread: the nwg partials in index order, then fmx_iqc_finish on the block
static __device__ __forceinline__ void iqc_finish_block(const long long *partial, int nwg, long n_in, double alpha,
                                                        double unit, FmxIqcBlock *blk) {
  long long s[5] = {0, 0, 0, 0, 0};
  for (int w = 0; w < nwg; ++w)
#pragma unroll
    for (int j = 0; j < 5; ++j) s[j] += partial[5 * (size_t)w + j];
  FmxIqcBlock b = *blk;
  fmx_iqc_finish(s, n_in, alpha, unit, &b);
  *blk = b;
}

__global__ __launch_bounds__(64) void k_iqc_finish(const long long *partial, int nwg, long n_in, double alpha, double unit,
                                                   FmxIqcBlock *blk) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  iqc_finish_block(partial, nwg, n_in, alpha, unit, blk);
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

/* ---- the corrected channelizer: k_wb with wb_iqc_mix ahead of the rotation ---- */
// tsum[c] = (SR, SI): the sums of channel c's taps as its weight rows hold them
template <bool S16, bool EVEN>
__global__ __launch_bounds__(256) void k_wb_iqc(WbArgs a, const FmxIqcBlock *iqc, const float *tsum) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n0 = (int)blockIdx.x * 16 * a.nt; // first output of the workgroup
  const int NI = (16 * a.nt - 1) * a.D + a.Lp; // samples of the window
  const int NIp = (NI + 7) & ~7;
  const WbImage m = wb_image(NIp);
  wb_stage<S16, true>(m, NI, NIp, (long)n0 * a.D - (a.Lp - 1), (long)a.n_out * a.D, a.valid, a.in, a.hist, a.L, a.in_al, tid);
  // the call's parameters: one uniform load per wave, ahead of the K loop
  const float d_i = iqc->k[0], d_q = iqc->k[1], gain = iqc->k[2], cross = iqc->k[3];
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
      const WbRot rot = wb_rotation(a.fpos[c], smod, a.fs, a.inv_fs);
      const float SR = tsum[2 * c], SI = tsum[2 * c + 1];
      const WbSum y = wb_iqc_mix(rr[i], ii[i], ri[i], ir[i], d_i * SR, d_i * SI, d_q * SR, d_q * SI, gain, cross);
      wb_store(rot, y.re, y.im, a.scale, a.out + 2 * ((size_t)c * a.out_stride + n));
    }
  }
}

int launch_wb_iqc(const WbArgs &a0, const FmxIqcBlock *iqc, const float *tsum, void *stream) {
  if (!iqc || !tsum) return FMX_E_INVALID;
  return wb_run(a0, stream, [=](const WbArgs &a, size_t smem, dim3 grid, hipStream_t st) {
    return WB_LAUNCH(k_wb_iqc, a.s16, (a.D & 1) == 0, grid, smem, st, a, iqc, tsum);
  });
}

/* ---- the corrected scan: k_wb_scan with wb_iqc_mix ahead of re^2 + im^2 ---- */
// every output from tpp on has its whole window inside the call, so the
// constant d SR is exact here too.  tsum[p] = (SR, SI) of point p.
template <bool S16, bool EVEN>
__global__ __launch_bounds__(256) void k_wb_scan_iqc(WbScanArgs a, const FmxIqcBlock *iqc, const float *tsum) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n0 = a.tpp + (int)blockIdx.x * 16 * a.nt; // first output of the workgroup
  const int NI = (16 * a.nt - 1) * a.D + a.Lp;       // samples of the window
  const int NIp = (NI + 7) & ~7;
  const WbImage m = wb_image(NIp);
  wb_stage<S16, false>(m, NI, NIp, (long)n0 * a.D - (a.Lp - 1), (long)a.n_out * a.D, 0, a.in, nullptr, 0, a.in_al, tid);
  const int grp = 4 * (int)blockIdx.y + wave; // the wave's point group
  if (16 * grp >= a.P) return;
  // the read's parameters: one uniform load per wave, ahead of the K loop
  const float d_i = iqc->k[0], d_q = iqc->k[1], gain = iqc->k[2], cross = iqc->k[3];
  const int col = lane & 15, g = lane >> 4;
  // a ragged last group computes its last point again in the spare rows (not read)
  const int pa = min(16 * grp + col, a.P - 1);
  // tiles of the workgroup that hold an output below n_out (wave-uniform)
  const int tiles = min(a.nt, (a.n_out - n0 + 15) >> 4);
  wb_f32x4 rr[WB_SCAN_NT], ii[WB_SCAN_NT], ri[WB_SCAN_NT], ir[WB_SCAN_NT];
  wb_scan_mac<S16, EVEN>(m, a.w + (size_t)pa * 4 * a.Lp + 8 * g, a.Lp, a.D, col, g, tiles, rr, ii, ri, ir);
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
      float p = 0.0f;
      if (live) { // only a counted column is mixed
        const WbSum y = wb_iqc_mix(rr[t][i], ii[t][i], ri[t][i], ir[t][i], cR[i], cI[i], cQR[i], cQI[i], gain, cross);
        p = y.re * y.re + y.im * y.im;
      }
      pw[i] += p;
    }
  }
  wb_scan_reduce_store(pw, col, a.partial + ((size_t)grp * gridDim.x + blockIdx.x) * 16 + 4 * g);
}

int launch_wb_scan_iqc(const WbScanArgs &a0, const FmxIqcBlock *iqc, const float *tsum, void *stream) {
  if (!iqc || !tsum) return FMX_E_INVALID;
  return wb_scan_run(a0, stream, [=](const WbScanArgs &a, size_t smem, dim3 grid, hipStream_t st) {
    return WB_LAUNCH(k_wb_scan_iqc, a.s16, (a.D & 1) == 0, grid, smem, st, a, iqc, tsum);
  });
}
