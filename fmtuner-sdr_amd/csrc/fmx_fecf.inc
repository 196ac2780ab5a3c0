/* ================================================================== */
/* k_fecf: the fast front end on complex-float rows at the DSP rate    */
/* (fmx_wb_process_block, DESIGN.md section 20)                        */
/* ================================================================== */
/* Everything k_fe8<M, TPP, RS = false> does after its decimator, on rows
 * that already are at the DSP rate (the channelizer's): clip count, DC
 * blockers (affine scan, 8 samples per thread), the IQ FIR on
 * v_mfma_f32_16x16x32_f16 (f16 hi + lo images x 2^10, three products per K
 * step and component), AGC, discriminator, MPX store; on the call's last
 * chunk the stereo history rows and the RDS window.  No pilot BPF and no RDS
 * resampler: k_pilot and k_rs follow it, as they follow k_fe8.  The
 * arithmetic and its order are k_fe8's statement by statement (the stages
 * are duplicated here, not shared: k_fe8's body stays as it is), and the
 * carried state is the arrays k_fe8 and k_frontend use, so a channel may
 * alternate between the three from call to call.
 * One 256-thread workgroup per channel; chunks are cut as k_fe8 cuts them
 * (ceil(n / FE8_T) chunks of one size cs, a multiple of 8, the last one takes
 * the rest).  LDS: the four IQ images, yb, the IQ FIR history and the shared
 * words -- 35 KB, static; the unpadded MPX copy of the last chunk aliases the
 * images (dead after the IQ FIR).  The taps come from FmxDesign::iq_frag (L2),
 * not from an LDS window: untuned. */
struct FecfLds {
  static constexpr int IQW = FE_HALO_IQ + FE8_T + 32; // history + chunk + zero slack, as Fe8Layout::IQW
  _Float16 img[4][IQW] __attribute__((aligned(16))); // I hi, I lo, Q hi, Q lo of the DC blockers' outputs x 2^10
  float2 yb[FE8_T + 1] __attribute__((aligned(16))); // [0] the discriminator's r_prev, [1 + j] IQ FIR output j
  float2 hx[FE_HALO_IQ];                             // IQ FIR history (f32)
  FeShared sh;
};
static_assert((FecfLds::IQW * 2) % 16 == 0 && (FE_HALO_IQ * 2) % 16 == 0, "16-B aligned image rows");
static_assert((32 + FE8_T) * 4 <= 4 * FecfLds::IQW * 2, "the MPX copy inside the images");
static_assert(sizeof(FecfLds) <= Fe8Layout<10, 28, false>::BYTES, "a subset of k_fe8's LDS regions");

__global__ __launch_bounds__(256) void k_fecf(FeArgs a) {
  __shared__ FecfLds S;
  typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
  typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));
  typedef float f32x4_t __attribute__((ext_vector_type(4)));
  _Float16 *xih = S.img[0], *xil = S.img[1], *xqh = S.img[2], *xql = S.img[3];
  float2 *yb = S.yb, *hx = S.hx;
  float *uc = reinterpret_cast<float *>(&S.img[0][0]); // uc[32 + j]: MPX sample j of the last chunk (aliases the images)
  FeShared *sh = &S.sh;
  constexpr float kIqIn = 1024.0f;
  const int c = blockIdx.x;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int j0 = 8 * tid;
  const FmxDesign *__restrict__ D = a.des;
  const int n = a.n;
  const FmxChanParam par = a.par[c];
  const int iqL = D->iq_len[par.iqsel];
  const float iqscale = D->iq_scale[par.iqsel];
  const bool hist_out = a.st_hist_out != 0; // the stereo history rows (k_pilot's and k_pll's)
  const bool rds = a.rds_out != nullptr;    // k_rs resamples: this kernel hands it the window
  const float dc_a1 = -1.0f + 0.0005f; // iirfilt_rrrf_create_dc_blocker(0.0005)
  const float dc_c = -dc_a1;
  const float *row = a.in_f + (size_t)c * a.in_stride;

  // ---- carried state ----
  for (int h = tid; h < FE_HALO_IQ; h += 256) {
    const float2_t v = a.iq_hist[(size_t)c * (FMX_IQ_MAXLEN - 1) + h];
    hx[h] = make_float2(v.x, v.y);
  }
  float agc_g = 1.0f, agc_y2p = 1.0f;
  if (tid == 0) {
    sh->carry_i = a.dc_v[2 * c];
    sh->carry_q = a.dc_v[2 * c + 1];
    sh->fd_re = a.fd_prev[2 * c];
    sh->fd_im = a.fd_prev[2 * c + 1];
    sh->clip = 0;
    if (par.agc != 0) {
      agc_g = a.agc[2 * c];
      agc_y2p = a.agc[2 * c + 1];
    }
  }
  const float agc_bw = (par.agc == 1) ? 0.01f : 0.001f;
  int sched_n = 0;
  if (rds) {
    sched_n = a.rds_sched_n[a.rds_group[c]];
    // the previous call's last 32 MPX samples: k_rs's window (this call's replace them below)
    if (tid < 32) a.rds_win_out[(size_t)c * 32 + tid] = a.rds_hist[(size_t)c * 32 + tid];
  }
  const int nch = (n + FE8_T - 1) / FE8_T;
  const int cs = (((n + nch - 1) / nch) + 7) & ~7;
  __syncthreads();

  for (int n0 = 0; n0 < n; n0 += cs) {
    const int cnt = min(cs, n - n0); // samples of this chunk (a multiple of 4)
    // ================= the rows: 8 consecutive complex samples per thread =================
    float2 xv[8];
    {
      // 16-B loads of two samples; cnt is even, so a pair is inside the chunk or past it (zeros)
      const float4 *p = reinterpret_cast<const float4 *>(row + 2 * (size_t)(n0 + j0));
      int myclip = 0;
#pragma unroll
      for (int r = 0; r < 8; r += 2) {
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (j0 + r < cnt) v = p[r >> 1];
        xv[r] = make_float2(v.x, v.y);
        xv[r + 1] = make_float2(v.z, v.w);
      }
#pragma unroll
      for (int r = 0; r < 8; ++r)
        if (j0 + r < cnt && (fabsf(xv[r].x) >= 0.995f || fabsf(xv[r].y) >= 0.995f)) myclip++;
      if (myclip) atomicAdd(&sh->clip, myclip);
    }
    // IQ FIR history and the zero slack past the chunk (read with zero taps)
    if (tid < FE_HALO_IQ) {
      const float2 v = hx[tid];
      const float sI = v.x * kIqIn, sQ = v.y * kIqIn;
      const _Float16 hI = (_Float16)sI, hQ = (_Float16)sQ;
      xih[tid] = hI;
      xil[tid] = (_Float16)(sI - (float)hI);
      xqh[tid] = hQ;
      xql[tid] = (_Float16)(sQ - (float)hQ);
    }
    if (tid < 32) {
      const int i = FE_HALO_IQ + FE8_T + tid;
      xih[i] = xil[i] = xqh[i] = xql[i] = (_Float16)0.0f;
    }
    // ================= DC blockers: affine scan, 8 per thread =================
    {
      float A = 1.0f, BI = 0.0f, BQ = 0.0f;
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        BI = xv[r].x + dc_c * BI;
        BQ = xv[r].y + dc_c * BQ;
        A = dc_c * A;
      }
      wave_affine_scan(A, BI, BQ);
      if (lane == 63) {
        sh->wave_a[wave] = A;
        sh->wave_bi[wave] = BI;
        sh->wave_bq[wave] = BQ;
      }
      float eA, eI, eQ;
      wave_affine_prev(A, BI, BQ, eA, eI, eQ);
      __syncthreads();
      float vI = sh->carry_i, vQ = sh->carry_q;
      for (int w = 0; w < wave; ++w) {
        // scalar asm in mul-then-add order, as k_fe8's cross-wave carry (tests/test_isa_scan.py)
        const float wa = sh->wave_a[w], wi = sh->wave_bi[w], wq = sh->wave_bq[w];
        asm("v_mul_f32 %0, %2, %0\n\tv_add_f32 %0, %0, %3\n\tv_mul_f32 %1, %2, %1\n\tv_add_f32 %1, %1, %4"
            : "+v"(vI), "+v"(vQ)
            : "v"(wa), "v"(wi), "v"(wq));
      }
      vI = eA * vI + eI;
      vQ = eA * vQ + eQ;
      // the state before this thread's first element, then the reference's op order
      f16x8_t ih, il, qh, ql;
      const int rlast = (tid == (cnt - 1) >> 3) ? ((cnt - 1) & 7) : -1; // the chunk's last sample
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const float tI = dc_a1 * vI, tQ = dc_a1 * vQ;
        const float nI = xv[r].x - tI, nQ = xv[r].y - tQ;
        const float oI = nI - vI, oQ = nQ - vQ;
        const float sI = oI * kIqIn, sQ = oQ * kIqIn;
        ih[r] = (_Float16)sI;
        il[r] = (_Float16)(sI - (float)ih[r]);
        qh[r] = (_Float16)sQ;
        ql[r] = (_Float16)(sQ - (float)qh[r]);
        // the next chunk's IQ FIR history (f32; read above before the scan's barrier)
        if (j0 + r >= cnt - FE_HALO_IQ && j0 + r < cnt) hx[j0 + r - (cnt - FE_HALO_IQ)] = make_float2(oI, oQ);
        vI = nI;
        vQ = nQ;
        if (r == rlast) {
          sh->carry_n[0] = nI;
          sh->carry_n[1] = nQ;
        }
      }
      *reinterpret_cast<f16x8_t *>(xih + FE_HALO_IQ + j0) = ih;
      *reinterpret_cast<f16x8_t *>(xil + FE_HALO_IQ + j0) = il;
      *reinterpret_cast<f16x8_t *>(xqh + FE_HALO_IQ + j0) = qh;
      *reinterpret_cast<f16x8_t *>(xql + FE_HALO_IQ + j0) = ql;
      __syncthreads();
      if (tid == 0) {
        sh->carry_i = sh->carry_n[0];
        sh->carry_q = sh->carry_n[1];
      }
    }
    __syncthreads();
    // ================= IQ FIR =================
    {
      // v_mfma_f32_16x16x32_f16 tiles as k_fe8's: transposed (images as A,
      // taps as B, FmxDesign::iq_frag), K = the block's P8 + 15 inputs; three
      // MFMAs per K step and component (hi*hi, lo*hi, hi*lo) into f32
      // accumulators.  Each wave: two tiles (512 outputs) of I and of Q.
      const int P8 = fir8_len(iqL);
      const int KSI = D->iq_ks[par.iqsel];
      const int col = lane & 15, g = lane >> 4;
      const int xb = FE_HALO_IQ + 16 * (32 * wave + col) - (P8 - 1) + 8 * g; // 8-aligned: P8 = 8k + 1
      const f16x8_t *bih = reinterpret_cast<const f16x8_t *>(xih + xb);
      const f16x8_t *bil = reinterpret_cast<const f16x8_t *>(xil + xb);
      const f16x8_t *bqh = reinterpret_cast<const f16x8_t *>(xqh + xb);
      const f16x8_t *bql = reinterpret_cast<const f16x8_t *>(xql + xb);
      const u32x4 *fa = reinterpret_cast<const u32x4 *>(&D->iq_frag[par.iqsel][0][0][0][0]) + lane;
      f32x4_t ai[2], aq[2];
      ai[0] = ai[1] = aq[0] = aq[1] = f32x4_t{0.0f, 0.0f, 0.0f, 0.0f};
      u32x4 ah = fa[0], al = fa[64];
      for (int ks = 0; ks < KSI; ++ks) {
        const f16x8_t ahi = __builtin_bit_cast(f16x8_t, ah), alo = __builtin_bit_cast(f16x8_t, al);
        if (ks + 1 < KSI) {
          ah = fa[128 * (ks + 1)];
          al = fa[128 * (ks + 1) + 64];
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const f16x8_t ihi = bih[32 * u + 4 * ks], ilo = bil[32 * u + 4 * ks]; // + 256 u + 32 ks samples
          const f16x8_t qhi = bqh[32 * u + 4 * ks], qlo = bql[32 * u + 4 * ks];
          ai[u] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ihi, ahi, ai[u], 0, 0, 0);
          aq[u] = __builtin_amdgcn_mfma_f32_16x16x32_f16(qhi, ahi, aq[u], 0, 0, 0);
          ai[u] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ilo, ahi, ai[u], 0, 0, 0);
          aq[u] = __builtin_amdgcn_mfma_f32_16x16x32_f16(qlo, ahi, aq[u], 0, 0, 0);
          ai[u] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ihi, alo, ai[u], 0, 0, 0);
          aq[u] = __builtin_amdgcn_mfma_f32_16x16x32_f16(qhi, alo, aq[u], 0, 0, 0);
        }
      }
      const float osc = iqscale * (1.0f / (4096.0f * kIqIn)); // exact: a power-of-two rescale
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        // lane: outputs 256 (2 wave + u) + 16 (4 g + i) + col -- 16 lanes, 16
        // consecutive float2: conflict-free ds_write_b64
#pragma unroll
        for (int i = 0; i < 4; ++i)
          yb[1 + 256 * (2 * wave + u) + 16 * (4 * g + i) + col] = make_float2(ai[u][i] * osc, aq[u][i] * osc);
      }
      if (tid == 0) yb[0] = make_float2(sh->fd_re, sh->fd_im);
    }
    __syncthreads();
    // ================= AGC (serial, only when enabled) =================
    if (par.agc != 0) {
      if (tid == 0) {
        for (int j = 0; j < cnt; ++j) {
          const float2 x = yb[1 + j];
          const float yr = x.x * agc_g, yi = x.y * agc_g;
          const float y2 = yr * yr + yi * yi;
          agc_y2p = (float)((1.0 - (double)agc_bw) * (double)agc_y2p + (double)(agc_bw * y2));
          if (agc_y2p > 1e-6f) agc_g *= expf(-0.5f * agc_bw * logf(agc_y2p));
          if (agc_g > 1e6f) agc_g = 1e6f;
          yb[1 + j] = make_float2(yr, yi);
        }
      }
      __syncthreads();
    }
    // ================= discriminator =================
    float mv[8];
    {
      const float ref = (par.fd_ref != 0.0f) ? par.fd_ref : D->fd_ref; // freqdem 1 / (2 pi kf)
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int j = tid + 256 * k;
        const float2 p = yb[j], r = yb[1 + j];
        const float re = p.x * r.x + p.y * r.y;
        const float im = p.x * r.y - p.y * r.x;
        const float m = fmx_atan2f(im, re) * ref; // select-free (fmx_math.h)
        mv[k] = m;
        if (a.mpx_out && j < cnt) a.mpx_out[(size_t)c * a.mpx_stride + n0 + j] = m;
      }
      if (tid == 0) {
        sh->fd_re = yb[cnt].x;
        sh->fd_im = yb[cnt].y;
      }
    }
    __syncthreads(); // the images and yb are dead: the next chunk, or the MPX copy below, may take them
    // the call's last FMX_HIST samples: the next call's stereo history rows;
    // its last 32 the next call's RDS resampler window (every chunk holds at
    // least 904 samples, see k_fe8)
    if (n0 + cnt >= n && (rds || hist_out)) {
#pragma unroll
      for (int k = 0; k < 8; ++k) uc[32 + tid + 256 * k] = mv[k];
      __syncthreads(); // uc complete
      if (hist_out) {
        static_assert(FMX_HIST == 512, "two history words per thread");
        float *hw = a.st_hist_wr + (size_t)c * FMX_HIST;
        hw[tid] = uc[32 + cnt - FMX_HIST + tid];
        hw[256 + tid] = uc[32 + cnt - 256 + tid];
      }
      if (rds && tid < 32) a.rds_hist[(size_t)c * 32 + tid] = uc[cnt + tid];
    }
  }

  // ---- write back state ----
  for (int h = tid; h < FE_HALO_IQ; h += 256) {
    const float2 v = hx[h];
    a.iq_hist[(size_t)c * (FMX_IQ_MAXLEN - 1) + h] = float2_t{v.x, v.y};
  }
  if (tid == 0) {
    a.dc_v[2 * c] = sh->carry_i;
    a.dc_v[2 * c + 1] = sh->carry_q;
    a.fd_prev[2 * c] = sh->fd_re;
    a.fd_prev[2 * c + 1] = sh->fd_im;
    if (par.agc != 0) {
      a.agc[2 * c] = agc_g;
      a.agc[2 * c + 1] = agc_y2p;
    }
  }
  if (rds && tid == 0) a.rds_count[c] = sched_n;
  if (tid == 0 && a.clip_out) a.clip_out[c] = (float)sh->clip / (float)n;
  fe_next_sched_copy(a);
}

// k_fecf takes complex-float rows at the DSP rate, 16-B aligned with a stride
// of whole 16-B groups (two complex samples), in calls of n >= FE8_MIN_N
// samples with n % 4 == 0 (the chunks are k_fe8's); every other call shape
// runs k_frontend in FE_IN_CF mode
bool fecf_ok(const FeArgs &a) {
  if (a.in_mode != FE_IN_CF) return false;
  const bool aligned = (reinterpret_cast<uintptr_t>(a.in_f) & 15) == 0 && (a.in_stride & 3) == 0;
  return aligned && a.n >= FE8_MIN_N && (a.n & 3) == 0 && a.do_demod && !a.bb_out && a.des_fs >= 190000;
}
// dynamic LDS a launch takes on top of the kernel's static LDS (the code
// object records only the latter): 0 k_fe8<10, 28, false> (process_block's
// front end at 2.4 MS/s), 1 k_fecf (none: its LDS is static)
int fe_launch_lds_bytes(int which) {
  if (which == 0) return Fe8Layout<10, 28, false>::BYTES;
  return which == 1 ? 0 : -1;
}
// no pilot BPF and no resampler inside: k_pilot and k_rs (rds_win_out) follow
int launch_fecf(const FeArgs &a, void *stream) {
  if (!fecf_ok(a) || a.pilot_out || (a.rds_out && !a.rds_win_out) || 2L * a.n > a.in_stride) return FMX_E_INVALID;
  return fmx_launch(k_fecf, dim3(a.C), dim3(256), 0, static_cast<hipStream_t>(stream), a);
}
