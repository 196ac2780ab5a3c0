// fmx_pll.inc -- k_pll, the StereoDecoder per-sample loop
// (stereo_decoder.cpp:169-285), included once by fmx_kernels.hip; the design
// is described above the include.
// CH channels (rows) per workgroup (round 5: 16 up to 2 048 channels, 24
// above -- launch_pll): the P waves take 4 rows x 16 samples each
#define PLL_T 16                           // samples per tile: one DPP row of 16 lanes per channel
#ifndef FMX_PLL_SERIAL_PRIO
#define FMX_PLL_SERIAL_PRIO 2              // s_setprio of W0 and WB (A/B switch)
#endif
#define PLL_NPW(CH) ((CH) / 4)             // item-parallel waves
#define PLL_WAVES(CH) (2 + PLL_NPW(CH))    // W0 (chain), WB (blend), the P waves
// ring sizes are powers of two (slot = tile & (N - 1))
#define PLL_NINP 8                         // pilot tiles: issued 3 ahead, read by W0 (k, k+1) and stage A (k-1): >= 5
#define PLL_NM 4                           // mpx tiles: issued 1 ahead, read by stage A: >= 3
#define PLL_ND 8                           // delayed MPX: issued 1 ahead, read by stage B three iterations later: >= 5
#define PLL_NC 4                           // cos(2 phase), stage A -> stage B: >= 3
#define PLL_NIT(NT) ((NT) + 3)             // iterations: W0 tile k, A k-1, WB k-2, B k-3
#ifndef PLL_PUNROLL
#define PLL_PUNROLL 8                      // P waves' loop unroll (a multiple of every ring size; 1: not unrolled)
#endif
template <int CH> struct alignas(16) PllShared {
  static_assert(CH % 4 == 0 && CH * PLL_T == 64 * PLL_NPW(CH), "one item per P-wave lane");
  float inp[PLL_NINP][CH][PLL_T];      // pilot tiles (LDS-DMA by the P waves)
  float inm[PLL_NM][CH][PLL_T];        // mpx tiles (LDS-DMA by the P waves)
  float dly[PLL_ND][CH][PLL_T];        // delay-line output per item (LDS-DMA by the P waves)
  uint32_t s0t[2][CH][PLL_T];          // W0 -> A: NCO word after each step
  float tg[2][CH][PLL_T];              // A -> WB: blend target
  float bl[2][CH][PLL_T];              // WB -> B: blend after each sample
  float cs[PLL_NC][CH][PLL_T];         // A -> B: cos(2 phase)
  int flags[CH];                       // bit0 force mono, bit1 force stereo, bit2 detected, bits 8.. blend mode
  float gate[CH];
  float fin[5][CH];                    // block-end values: pbm, mm, pilot I, pilot Q (A), blend (WB)
};

// the L/R matrix of one sample from the delayed MPX and cos(2 phase), in the
// reference's order (stereo_decoder.cpp:218-224): mono, left - mono, right - mono
__device__ __forceinline__ void pll_matrix(float delayed, float cos2, float *mono, float *dl, float *dr) {
  const float monoNorm = delayed * 0.5f;
  const float lr = 2.0f * delayed * cos2;
  const float sl = (delayed + lr) * 0.5f;
  const float sr = (delayed - lr) * 0.5f;
  *mono = monoNorm;
  *dl = sl - monoNorm;
  *dr = sr - monoNorm;
}

// DPP within the 16-lane row of a channel: lane 15 of the row to all 16 lanes
// (row_newbcast:15, gfx90a+) and row_ror:1 (lane t reads t - 1, lane 0 reads
// lane 15)
__device__ __forceinline__ float pll_bcast15(float x) {
  return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, x), 0x15F, 0xF, 0xF, false));
}
__device__ __forceinline__ float pll_ror1(float x) {
  return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, x), 0x121, 0xF, 0xF, false));
}

// <= 80 VGPRs (six waves per SIMD's 512; amdgpu_num_vgpr is not honoured by
// this compiler, the occupancy attribute is): a k_pll wave and a k_rs wave
// (96) beside two k_fe8 waves (168 each)
template <int CH>
__global__ __launch_bounds__(64 * PLL_WAVES(CH)) __attribute__((amdgpu_waves_per_eu(6))) void k_pll(PllArgs a) {
  __shared__ PllShared<CH> shm;
  PllShared<CH> *sh = &shm;
  // Stage barrier: LDS writes complete (lgkmcnt) + s_barrier.  Not
  // __syncthreads(): its fence would also drain the P waves' stores and
  // LDS-DMA (vmcnt), which are meant to stay in flight across the barrier.
#define PLL_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")
#ifdef FMX_STAMPS
  unsigned long long pw_work = 0, pw_wait = 0, pw_vm = 0, pw_last = __builtin_amdgcn_s_memtime();
#define PLL_SYNC()                                                   \
  {                                                                  \
    unsigned long long t_ = __builtin_amdgcn_s_memtime();            \
    pw_work += t_ - pw_last;                                         \
    PLL_BARRIER();                                                   \
    pw_last = __builtin_amdgcn_s_memtime();                          \
    pw_wait += pw_last - t_;                                         \
  }
#define PLL_STAMP_OUT()                                              \
  if (a.dbg && (threadIdx.x & 63) == 0) {                            \
    atomicAdd(a.dbg + 2 * (threadIdx.x >> 6), pw_work);              \
    atomicAdd(a.dbg + 2 * (threadIdx.x >> 6) + 1, pw_wait);          \
    atomicAdd(a.dbg + 16 + (threadIdx.x >> 6), pw_vm);               \
  }
#else
#define PLL_SYNC() PLL_BARRIER();
#define PLL_STAMP_OUT()
#endif
  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  const int lane = tid & 63;
  const int c0 = blockIdx.x * CH;
  const FmxDesign *__restrict__ D = a.des;
  const int n = a.n;
  const int NT = (n + PLL_T - 1) / PLL_T;
  constexpr float kS = 0.9995f;
  constexpr float kI = 1.0f - 0.9995f;
  if (n <= 0) {  // processAudio(n == 0) returns before touching state
    const int ch = c0 + tid;
    if (tid < CH && ch < a.C) {
      if (a.stereo_out) a.stereo_out[ch] = a.st[ch].detected;
      if (a.pilot_tenths_out) a.pilot_tenths_out[ch] = a.st[ch].level;
      if (a.indicator_out) a.indicator_out[ch] = a.st[ch].detected || (a.par[ch].force_mono && a.st[ch].level >= 20);
    }
    return;
  }
  if (tid < CH) {
    const int ch = c0 + tid;
    int f = 0;
    float g = 1.0f;
    if (ch < a.C) {
      const FmxChanParam par = a.par[ch];
      f = (par.force_mono ? 1 : 0) | (par.force_stereo ? 2 : 0) | (a.st[ch].detected ? 4 : 0) | (par.blend << 8);
      g = D->gate[par.blend];
    }
    sh->flags[tid] = f;
    sh->gate[tid] = g;
  }
  // serial waves (W0, WB): lane = row (channel c0 + lane); lanes >= CH
  // idle (they read row lrow and store nothing)
  const int lrow = lane < CH ? lane : CH - 1;
  const int c = c0 + lane;
  const bool act = lane < CH && c < a.C;
  const bool own = lane < CH;
  if (wave == 0) {
    // ---------------- W0: the PLL feedback chain (stereo_decoder.cpp:178-192) ----------------
    if (FMX_PLL_SERIAL_PRIO > 0) __builtin_amdgcn_s_setprio(FMX_PLL_SERIAL_PRIO);
    const FmxStereoState s0 = act ? a.st[c] : FmxStereoState{};
    // theta is carried + FMX_CHAIN_TOFF (the chain sine's rounding offset,
    // fmx_math.h; 0 for the other forms): the recurrence is offset-invariant,
    // the words W0 hands to the P waves (sh->s0t) are offset, and the block's
    // last word loses the offset below
    uint32_t theta = s0.theta + FMX_CHAIN_TOFF, dtheta = s0.dtheta;
    // liquid pll_step: dtheta += constrain(e alpha), theta += constrain(e
    // beta) (then step: theta += dtheta), constrain(x) = frac(x / 2 pi) 2^32.
    // The chain per sample (fmx_chain_words / fmx_chain_sin, fmx_math.h): one
    // packed multiply {pa, pb} vcoQ, two truncating converts, one add3, one
    // v_alignbit_b32 and v_sin -- the pilot's pre-products pa, pb (one packed
    // multiply per sample) and theta + dtheta fold off the chain.  Round 5:
    // 9 VALU per sample instead of 15 plus two SALU (a lone wave issues one
    // wave64 VALU op per ~4 clocks, so the count, not only the depth, sets the
    // chain's pace; profiles/r05*_pll_chain*).
    typedef float f2 __attribute__((ext_vector_type(2)));
    const float ka = D->pll_alpha * 0.159154943091895f, kb = D->pll_beta * 0.159154943091895f;
    const f2 kab = f2{ka * 4294967296.0f, kb * 4294967296.0f};
    float vcoQ = fmx_chain_sin(theta);
    __syncthreads(); // pilot tiles 0..2 in LDS
    // the pilot tile is read one iteration ahead, so its LDS latency
    // overlaps the chain of the current tile
    float4 pcur[PLL_T / 4], pnxt[PLL_T / 4];
#pragma unroll
    for (int q = 0; q < PLL_T / 4; ++q) pnxt[q] = pcur[q] = *reinterpret_cast<const float4 *>(&sh->inp[0][lrow][4 * q]);
    for (int k = 0; k < PLL_NIT(NT); ++k) {
      if (k + 1 < NT) {
#pragma unroll
        for (int q = 0; q < PLL_T / 4; ++q)
          pnxt[q] = *reinterpret_cast<const float4 *>(&sh->inp[(k + 1) & (PLL_NINP - 1)][lrow][4 * q]);
      }
      // full tiles run without per-sample guards (a compile-time case)
      auto tile = [&](auto full_c, int cnt) __attribute__((always_inline)) {
        constexpr bool FULL = decltype(full_c)::value;
        float pv[PLL_T];
#pragma unroll
        for (int q = 0; q < PLL_T / 4; ++q) {
          pv[4 * q] = pcur[q].x; pv[4 * q + 1] = pcur[q].y; pv[4 * q + 2] = pcur[q].z; pv[4 * q + 3] = pcur[q].w;
        }
        uint32_t tw[PLL_T];
        f2 pab[PLL_T];
#pragma unroll
        for (int t = 0; t < PLL_T; ++t) pab[t] = f2{pv[t], pv[t]} * kab;
#pragma unroll
        for (int t = 0; t < PLL_T; ++t) {
          if (FULL || t < cnt) {
            // pilot sin(phase) alpha (beta) / 2 pi 2^32 -> the words -> pll_step + step
            fmx_chain_step(pab[t].x, pab[t].y, vcoQ, theta, dtheta);
            vcoQ = fmx_chain_sin(theta);
          }
          tw[t] = theta;
        }
        if (own) {
#pragma unroll
          for (int q = 0; q < PLL_T / 4; ++q)
            *reinterpret_cast<uint4 *>(&sh->s0t[k & 1][lane][4 * q]) =
                make_uint4(tw[4 * q], tw[4 * q + 1], tw[4 * q + 2], tw[4 * q + 3]);
        }
      };
      if (k < NT) {
        const int cnt = min(PLL_T, n - k * PLL_T);
        if (cnt == PLL_T) tile(std::true_type{}, cnt);
        else tile(std::false_type{}, cnt);
      }
#pragma unroll
      for (int q = 0; q < PLL_T / 4; ++q) pcur[q] = pnxt[q];
      PLL_SYNC()
    }
    PLL_SYNC() // A / WB block-end values in sh->fin
    PLL_STAMP_OUT()
    if (!act) return;
    // the word before the block's last step (m_pllFreq of the last sample),
    // from the last two tiles' words still in sh->s0t
    const int cntL = n - (NT - 1) * PLL_T;
    const uint32_t tprev = cntL >= 2 ? sh->s0t[(NT - 1) & 1][lane][cntL - 2] - FMX_CHAIN_TOFF
                                     : (NT >= 2 ? sh->s0t[(NT - 2) & 1][lane][PLL_T - 1] - FMX_CHAIN_TOFF : s0.theta);
    theta -= FMX_CHAIN_TOFF;
    // ---- block-end stereo detection (stereo_decoder.cpp:243-285) ----
    FmxStereoState s = s0;
    s.theta = theta;
    s.dtheta = dtheta;
    s.pll_phase = d_nco_phase(theta);
    // m_pllFreq of the last sample: clamp(unwrap(phaseNext - phaseNow))
    s.pll_freq = d_clamp(d_unwrap(s.pll_phase - d_nco_phase(tprev)), D->pll_min, D->pll_max);
    s.pilot_band_mag = sh->fin[0][lane];
    s.mpx_mag = sh->fin[1][lane];
    s.pilot_i = sh->fin[2][lane];
    s.pilot_q = sh->fin[3][lane];
    s.blend = sh->fin[4][lane];
    const float nominal = D->nominal;
    const FmxChanParam par = a.par[c];
    const bool fstereo = par.force_stereo != 0;
    const float fsf = (float)D->fs;
    bool detected = s.detected != 0;
    const float mag = sqrtf((s.pilot_i * s.pilot_i) + (s.pilot_q * s.pilot_q));
    s.pilot_magnitude = (s.pilot_magnitude * 0.9f) + (mag * 0.1f);
    const float mpxThr = detected ? 0.0028f : 0.005f;
    const float ratio = s.pilot_band_mag / fmaxf(s.mpx_mag, 1e-3f);
    const float coh = s.pilot_magnitude / fmaxf(s.pilot_band_mag, 1e-4f);
    const float ratioThr = detected ? 0.022f : 0.040f;
    const float cohThr = detected ? 0.11f : 0.18f;
    const float errHz = fabsf(s.pll_freq - nominal) * fsf / (2.0f * kPiF);
    const float pllThr = detected ? 320.0f : 180.0f;
    const bool present = (s.mpx_mag > mpxThr) && (ratio > ratioThr) && (coh > cohThr) && (errHz < pllThr);
    if (!fstereo) {
      if (!detected) {
        if (present) {
          s.pilot_count++;
          s.loss_count = 0;
          if (s.pilot_count >= 6) detected = true;
        } else {
          s.pilot_count = 0;
        }
      } else if (present) {
        s.loss_count = 0;
      } else if (++s.loss_count >= 24) {
        detected = false;
        s.pilot_count = 0;
        s.loss_count = 0;
      }
    }
    const float calibrated = s.pilot_magnitude * 8.0f;
    int lvl = (int)roundf(calibrated * 750.0f);
    s.level = lvl < 0 ? 0 : (lvl > 750 ? 750 : lvl);
    s.detected = detected ? 1 : 0;
    a.st[c] = s;
    if (a.stereo_out) a.stereo_out[c] = s.detected;
    if (a.pilot_tenths_out) a.pilot_tenths_out[c] = s.level;
    // XDR stereo indicator: stereoDetected || (forceMono && stereo && pilot >= 20)
    // (main.cpp:1298-1300; k_pll runs only with processing.stereo)
    if (a.indicator_out) a.indicator_out[c] = (s.detected || (par.force_mono && s.level >= 20)) ? 1 : 0;
  } else if (wave == 1) {
    // ---------------- WB: the blend smoother (stereo_decoder.cpp:226-228) ----------------
    if (FMX_PLL_SERIAL_PRIO > 0) __builtin_amdgcn_s_setprio(FMX_PLL_SERIAL_PRIO);
    const float blend0 = act ? a.st[c].blend : 0.0f;
    __syncthreads();
    float blend = blend0;
    const int mode = sh->flags[lrow] >> 8;
    const float attack = D->blend_attack[mode], release = D->blend_release[mode];
    for (int k = 0; k < PLL_NIT(NT); ++k) {
      const int kt = k - 2;
      // full tiles without per-sample guards (a compile-time case, as W0)
      auto tile = [&](auto full_c, int cnt) __attribute__((always_inline)) {
        constexpr bool FULL = decltype(full_c)::value;
        float tv[PLL_T], bv[PLL_T];
#pragma unroll
        for (int q = 0; q < PLL_T / 4; ++q) {
          const float4 x = *reinterpret_cast<const float4 *>(&sh->tg[kt & 1][lrow][4 * q]);
          tv[4 * q] = x.x; tv[4 * q + 1] = x.y; tv[4 * q + 2] = x.z; tv[4 * q + 3] = x.w;
        }
#pragma unroll
        for (int t = 0; t < PLL_T; ++t) {
          // blend += (tgt - blend) * (tgt > blend ? attack : release),
          // select-free: exactly one of the two products is nonzero and
          // adding the other (+0 / -0) leaves the sum unchanged
          if (FULL || t < cnt) {
            const float d = tv[t] - blend;
            blend = (blend + fmaxf(d, 0.0f) * attack) + fminf(d, 0.0f) * release;
          }
          bv[t] = blend;
        }
        if (own) {
#pragma unroll
          for (int q = 0; q < PLL_T / 4; ++q)
            *reinterpret_cast<float4 *>(&sh->bl[kt & 1][lane][4 * q]) =
                make_float4(bv[4 * q], bv[4 * q + 1], bv[4 * q + 2], bv[4 * q + 3]);
        }
      };
      if (kt >= 0 && kt < NT) {
        const int cnt = min(PLL_T, n - kt * PLL_T);
        if (cnt == PLL_T) tile(std::true_type{}, cnt);
        else tile(std::false_type{}, cnt);
      }
      PLL_SYNC()
    }
    if (own) sh->fin[4][lane] = blend;
    PLL_SYNC()
    PLL_STAMP_OUT()
  } else {
    // ---------------- P0..P3: one item (row, t) of every tile per lane ----------------
    const int pw = wave - 2;
    const int item = lane + 64 * pw;
    const int row = item / PLL_T, tt = item % PLL_T;
    const bool tlast = tt == PLL_T - 1;
    const int ch = c0 + row;
    const bool chv = ch < a.C;
    const float nominal = D->nominal, fsf = (float)D->fs;
    const float pmin = D->pll_min, pmax = D->pll_max;
    const int Dly = D->delay_len;
    // kS^(t + 1) for the carry into sample t of a tile, kS^d for the scan steps
    float kp1;
    {
      double p = 1.0;
      for (int i = 0; i <= tt; ++i) p *= (double)kS;
      kp1 = (float)p;
    }
    const float k1 = kS, k2 = (float)((double)kS * kS), k4 = (float)((double)k2 * k2), k8 = (float)((double)k4 * k4);
    // carried state of this row: the previous sample's sine / cosine / phase
    // (lanes t = 15 offer them to t = 0 of the next tile) and the four
    // recurrences (pilot / MPX envelopes, pilot I / Q integrators)
    float prev_s, prev_c, prev_ph, cr0, cr1, cr2, cr3;
    {
      FmxStereoState s0{};
      if (chv) s0 = a.st[ch];
      word_sincos(s0.theta, &prev_s, &prev_c);
      prev_ph = d_nco_phase(s0.theta);
      cr0 = s0.pilot_band_mag;
      cr1 = s0.mpx_mag;
      cr2 = s0.pilot_i;
      cr3 = s0.pilot_q;
    }
    // Moves into LDS, one dword per lane: the wave-uniform part of each
    // address (the workgroup's rows, the tile) in SGPRs, the lane's part (its
    // row and sample) a constant byte offset.  Rows past the handle read the
    // last valid row; tiles past the block re-read the last tile; in the last
    // tile, samples past n read sample n - 1 (never past the row).
    const int rv = min(CH, a.C - c0) - 1;            // last valid row of the workgroup
    const int rowc = min(row, rv);
    const int cntL = n - (NT - 1) * PLL_T;               // samples in the last tile
    const int ttL = min(tt, cntL - 1);
    const uint32_t vo_p = (uint32_t)((rowc * a.pilot_stride + tt) * 4), vo_pL = (uint32_t)((rowc * a.pilot_stride + ttL) * 4);
    const uint32_t vo_m = (uint32_t)((rowc * a.mpx_stride + tt) * 4), vo_mL = (uint32_t)((rowc * a.mpx_stride + ttL) * 4);
    const float *pil0 = a.pilot + (size_t)c0 * a.pilot_stride, *mpx0 = a.mpx + (size_t)c0 * a.mpx_stride;
    // the delay line's output mpx[t - Dly] (stereo_decoder.cpp:207-212): the
    // previous call's history for t < Dly (tiles before the first whole-MPX
    // tile take a per-lane address)
    const float *hrow = a.st_hist_rd + (size_t)(c0 + rowc) * FMX_HIST + FMX_HIST;
    const float *mrow = a.mpx + (size_t)(c0 + rowc) * a.mpx_stride;
    const int jD = (Dly + PLL_T - 1) / PLL_T;            // first tile whose delayed samples are all in this call's MPX
    const uint32_t lds_p = lds_addr(&sh->inp[0][0][0]) + 256u * pw;
    const uint32_t lds_m = lds_addr(&sh->inm[0][0][0]) + 256u * pw;
    const uint32_t lds_d = lds_addr(&sh->dly[0][0][0]) + 256u * pw;
    constexpr uint32_t TB = CH * PLL_T * 4; // bytes per tile
    auto dma_pilot = [&](int j) __attribute__((always_inline)) {
      const int jj = min(j, NT - 1);
      dma_dword_s(pil0 + PLL_T * jj, jj == NT - 1 ? vo_pL : vo_p, lds_p + TB * (j & (PLL_NINP - 1)));
    };
    auto dma_mpx = [&](int j) __attribute__((always_inline)) {
      const int jj = min(j, NT - 1);
      dma_dword_s(mpx0 + PLL_T * jj, jj == NT - 1 ? vo_mL : vo_m, lds_m + TB * (j & (PLL_NM - 1)));
    };
    auto dma_dly = [&](int j) __attribute__((always_inline)) {
      const int jj = min(j, NT - 1);
      const uint32_t lds = lds_d + TB * (j & (PLL_ND - 1));
      if (jj >= jD) {
        dma_dword_s(mpx0 + PLL_T * jj - Dly, jj == NT - 1 ? vo_mL : vo_m, lds);
      } else {
        const int t = PLL_T * jj + (jj == NT - 1 ? ttL : tt) - Dly;
        dma_dword(t >= 0 ? mrow + t : hrow + t, lds);
      }
    };
    // raw L/R: sample t of channel ch at lr_base + lr_off + J j (pair tiles:
    // J = 32, the workgroup's base c0 * stride since c0 is even)
    const int lr_off = a.lr_tiled ? ((row >> 1) * (a.lr_stride >> 4)) * 32 + (row & 1) * 16 + tt : row * a.lr_stride + tt;
    const int lrJ = a.lr_tiled ? 32 : PLL_T;
    // the stores as buffer stores: a lane with nothing to store takes an
    // out-of-range offset (dropped), so every iteration issues exactly two
    // and the counted wait below stays exact
    // (rows rounded up to 8 as allocated: a pair tile spans its odd row's
    // samples even when that row is past the handle)
    const uint32_t lr_rows = (uint32_t)min(CH, (a.C - c0 + 7) & ~7);
    const __amdgpu_buffer_rsrc_t lbr = make_rsrc(a.lraw + (size_t)c0 * a.lr_stride, lr_rows * (uint32_t)a.lr_stride * 4u);
    const __amdgpu_buffer_rsrc_t rbr = make_rsrc(a.rraw + (size_t)c0 * a.lr_stride, lr_rows * (uint32_t)a.lr_stride * 4u);
    __builtin_amdgcn_s_waitcnt(0x0F70);         // vmcnt(0): the state loads retired before the DMA stream
#pragma unroll
    for (int j = 0; j < 3; ++j) dma_pilot(j);
    dma_mpx(0);
    dma_dly(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    // per-row constants of the blend target: flags (force mono / stereo,
    // detected), gate, shaping mode (stereo_decoder.cpp:98-166)
    const int fl = sh->flags[row];
    const float gate = sh->gate[row];
    const int mode = fl >> 8;
    const bool tzero = (fl & 1) || !(fl & 6); // force mono, or not detected and not forced stereo
    const bool tone = !(fl & 1) && (fl & 2);  // force stereo
    const float g_ratio = 0.022f * gate, g_coh = 0.11f * gate;
    // one iteration: stage A of tile k-1 (doA), stage B of tile k-3 (doB);
    // fullA: tile k-1 is whole (constants in the steady loop below)
    auto piter = [&](const int k, const bool doA, const bool doB, const bool fullA) __attribute__((always_inline)) {
      // every LDS read of the iteration first (one round trip): stage B's
      // operands of tile k-3, stage A's of tile k-1 (the moves below go to
      // other ring slots)
      const int jb = k - 3, j = k - 1;
      float blend = 0.0f, delayed = 0.0f, c2B = 0.0f, pilot = 0.0f, mpx = 0.0f;
      uint32_t th = 0u;
      if (doB) {
        blend = sh->bl[jb & 1][row][tt];
        delayed = sh->dly[jb & (PLL_ND - 1)][row][tt];
        c2B = sh->cs[jb & (PLL_NC - 1)][row][tt];
      }
      if (doA) {
        th = sh->s0t[j & 1][row][tt] - FMX_CHAIN_TOFF;
        pilot = sh->inp[j & (PLL_NINP - 1)][row][tt];
        mpx = sh->inm[j & (PLL_NM - 1)][row][tt];
      }
      // ---- stage B (tile k-3): L/R matrix with the blend, raw L/R stores
      // (stereo_decoder.cpp:218-231); issued before the moves, so that the
      // stores have the whole next iteration to retire
      if (doB) {
        float mo, dl, dr;
        pll_matrix(delayed, c2B, &mo, &dl, &dr);
        const float ol = mo + (dl * blend);
        const float orr = mo + (dr * blend);
        const uint32_t off = (chv && jb * PLL_T + tt < n) ? 4u * (uint32_t)(lrJ * jb + lr_off) : 0xFFFFFFFFu;
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, ol), lbr, off, 0, 0);
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, orr), rbr, off, 0, 0);
      }
      // ---- this iteration's moves: pilot tile k+3, MPX and delay-line tile k+1
      dma_pilot(k + 3);
      dma_mpx(k + 1);
      dma_dly(k + 1);
      // ---- stage A (tile k-1) ----
      if (doA) {
        // phase (stereo_decoder.cpp:178-195): sin / cos / phase of the word
        // after this sample's step; the VCO of this sample is the previous
        // word's (lane t - 1, or the previous tile's t = 15 for t = 0)
        float sN, cN;
        word_sincos(th, &sN, &cN);
        const float ph = d_nco_phase(th);
        const float sP = pll_ror1(tlast ? prev_s : sN);
        const float cP = pll_ror1(tlast ? prev_c : cN);
        const float phP = pll_ror1(tlast ? prev_ph : ph);
        prev_s = sN;
        prev_c = cN;
        prev_ph = ph;
        const float fr = __builtin_amdgcn_fmed3f(d_unwrap(ph - phP), pmin, pmax); // m_pllFreq: clamp(dphi)
        const float c2 = (cN * cN) - (sN * sN);
        // the four linear recurrences x = kS x + u (stereo_decoder.cpp:174-177,
        // 194-195) as an inclusive scan over the tile's 16 lanes, plus the
        // carry of the previous tile's last sample
        float x0 = fabsf(pilot) * kI, x1 = fabsf(mpx) * kI;
        float x2 = (pilot * cP) * kI, x3 = (pilot * sP) * kI;
        // one v_fmac_f32 with the row shift on its first source per step:
        // x += shr(x) k (lanes t < d read 0; the same single-rounding fma as
        // a v_mov_dpp + v_fmac pair, round 4 r04as).  The four chains interleave, so a value is
        // read by DPP three VALU ops after its write; the s_nop covers the
        // values the compiler wrote right before the block (VALU write -> DPP
        // read: two wait states)
#define PLL_FD(D) "row_shr:" #D " row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        asm volatile("s_nop 1\n\t"
                     "v_fmac_f32_dpp %0, %0, %4 " PLL_FD(1) "v_fmac_f32_dpp %1, %1, %4 " PLL_FD(1)
                     "v_fmac_f32_dpp %2, %2, %4 " PLL_FD(1) "v_fmac_f32_dpp %3, %3, %4 " PLL_FD(1)
                     "v_fmac_f32_dpp %0, %0, %5 " PLL_FD(2) "v_fmac_f32_dpp %1, %1, %5 " PLL_FD(2)
                     "v_fmac_f32_dpp %2, %2, %5 " PLL_FD(2) "v_fmac_f32_dpp %3, %3, %5 " PLL_FD(2)
                     "v_fmac_f32_dpp %0, %0, %6 " PLL_FD(4) "v_fmac_f32_dpp %1, %1, %6 " PLL_FD(4)
                     "v_fmac_f32_dpp %2, %2, %6 " PLL_FD(4) "v_fmac_f32_dpp %3, %3, %6 " PLL_FD(4)
                     "v_fmac_f32_dpp %0, %0, %7 " PLL_FD(8) "v_fmac_f32_dpp %1, %1, %7 " PLL_FD(8)
                     "v_fmac_f32_dpp %2, %2, %7 " PLL_FD(8) "v_fmac_f32_dpp %3, %3, %7 " PLL_FD(8)
                     : "+v"(x0), "+v"(x1), "+v"(x2), "+v"(x3)
                     : "v"(k1), "v"(k2), "v"(k4), "v"(k8));
#undef PLL_FD
        const float o0 = cr0, o1 = cr1, o2 = cr2, o3 = cr3;
        const float pbm = fmaf(kp1, o0, x0);
        const float mm = fmaf(kp1, o1, x1);
        const float pi_ = fmaf(kp1, o2, x2);
        const float pq = fmaf(kp1, o3, x3);
        // the row's values after the tile's last sample: the next carries --
        // a whole tile by DPP row_newbcast:15 (no LDS round trip), the
        // block's last (partial) tile by ds_bpermute from lane cnt - 1
        const int cntj = fullA ? PLL_T : min(PLL_T, n - j * PLL_T);
        if (cntj == PLL_T) {
          cr0 = pll_bcast15(pbm);
          cr1 = pll_bcast15(mm);
          cr2 = pll_bcast15(pi_);
          cr3 = pll_bcast15(pq);
        } else {
          const int src = 4 * ((lane & ~(PLL_T - 1)) + cntj - 1);
          cr0 = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(src, __builtin_bit_cast(int, pbm)));
          cr1 = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(src, __builtin_bit_cast(int, mm)));
          cr2 = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(src, __builtin_bit_cast(int, pi_)));
          cr3 = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(src, __builtin_bit_cast(int, pq)));
        }
        const float mag2 = (pi_ * pi_) + (pq * pq);
        // keep the integrators and the old carries live past the carries'
        // ds_bpermute, so that no LDS return lands in the sources of the
        // packed multiply-adds above (tests/test_isa_scan.py)
        asm volatile("" ::"v"(pi_), "v"(pq), "v"(pbm), "v"(mm), "v"(o0), "v"(o1), "v"(o2), "v"(o3));
        // blend target (stereo_decoder.cpp:120-166, 196-205): hardware sqrt /
        // reciprocal, divisions by constants as products with their
        // reciprocals, clamps as v_med3 (~1 ulp; the target only steers the
        // blend smoother)
        const float magNow = __builtin_amdgcn_sqrtf(mag2);
        const float ratioNow = pbm * __builtin_amdgcn_rcpf(fmaxf(mm, 1e-3f));
        const float cohNow = magNow * __builtin_amdgcn_rcpf(fmaxf(pbm, 1e-4f));
        const float errHzNow = fabsf(fr - nominal) * fsf * (1.0f / (2.0f * kPiF));
        constexpr float cR = 0.040f - 0.022f, cC = 0.18f - 0.11f, cPl = 320.0f - 180.0f;
        const float ratioQ = __builtin_amdgcn_fmed3f((ratioNow - 0.022f) * (1.0f / cR), 0.0f, 1.0f);
        const float cohQ = __builtin_amdgcn_fmed3f((cohNow - 0.11f) * (1.0f / cC), 0.0f, 1.0f);
        const float pllQ = __builtin_amdgcn_fmed3f((320.0f - errHzNow) * (1.0f / cPl), 0.0f, 1.0f);
        const float q = fminf(ratioQ, fminf(cohQ, pllQ));
        const bool gated = ratioNow < g_ratio || cohNow < g_coh || errHzNow > (320.0f * 1.10f);
        const float q2 = q * q;
        const float shaped = (mode == 0) ? __builtin_amdgcn_sqrtf(q) : ((mode == 2) ? q2 * q : q2);
        // force mono -> 0, force stereo -> 1, not detected -> 0 (computeBlendTarget's paths)
        const float tgt = tzero ? 0.0f : (tone ? 1.0f : (gated ? 0.0f : __builtin_amdgcn_fmed3f(shaped, 0.0f, 1.0f)));
        sh->tg[j & 1][row][tt] = tgt;
        sh->cs[j & (PLL_NC - 1)][row][tt] = c2;
      }
      // every move issued before this iteration's has landed (the two
      // stores of this iteration, when there are any, and its three moves
      // may still be in flight)
#ifdef FMX_STAMPS // the P waves' wait for the moves (in the work clock otherwise)
      {
        const unsigned long long t_ = __builtin_amdgcn_s_memtime();
        pw_work += t_ - pw_last;
        pw_last = t_;
      }
#endif
      if (doB) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
#ifdef FMX_STAMPS
      {
        const unsigned long long t_ = __builtin_amdgcn_s_memtime();
        pw_vm += t_ - pw_last;
        pw_last = t_;
      }
#endif
      PLL_SYNC()
    };
    // the first three iterations (no stage B yet), the steady ones (k in
    // [3, NT - 1]: both stages, tile k-1 whole; unrolled by PLL_PUNROLL, the
    // ring sizes' multiple, so that every ring slot is a constant and the LDS
    // accesses and moves take immediate offsets -- round 5), the last ones
    for (int k = 0; k < min(3, PLL_NIT(NT)); ++k) piter(k, k >= 1 && k - 1 < NT, false, false);
    for (int k0 = 3; k0 < NT; k0 += PLL_PUNROLL) {
#pragma unroll
      for (int u = 0; u < PLL_PUNROLL; ++u) {
        const int k = k0 + u;
        if (k >= NT) break;
        piter(k, true, true, true);
      }
    }
    for (int k = max(3, NT); k < PLL_NIT(NT); ++k) piter(k, k - 1 < NT, true, false);
    if (tt == 0) {
      sh->fin[0][row] = cr0;
      sh->fin[1][row] = cr1;
      sh->fin[2][row] = cr2;
      sh->fin[3][row] = cr3;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // the last moves landed
    PLL_SYNC()
    PLL_STAMP_OUT()
  }
#undef PLL_SYNC
#undef PLL_STAMP_OUT
#undef PLL_BARRIER
}
