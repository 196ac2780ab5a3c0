/* ================================================================== */
/* k_wbb: the capture bank -- S wide captures of one plan channelized  */
/* by one launch (fmx_wb_bank_*, DESIGN.md section 22)                 */
/* ================================================================== */
/* Capture s owns the channels [first_channel[s], first_channel[s + 1]) of the
 * bank and row s of the call's input [S][wide_stride].  The kernel's work is
 * a flat device table of groups {capture, first channel, channels 1..16}
 * (fmx_wb_bank_groups): one entry per 16 channels of a capture, none for an
 * empty capture, blockIdx.y its index.  k_wbb is k_wb's body, statement for
 * statement and in k_wb's order -- the same LDS images, the same four chains
 * with hi*hi, hi*lo, lo*hi per K step, the same rotation and store -- with
 * in, hist, valid and base_mod taken from the group's capture, so a capture's
 * rows are bit for bit those of an fmx_wb object fed its row.  It is a copy
 * and not a parameter of k_wb: k_wb's assembly stays what it was.
 * Each capture's {counter, valid} lives on the device (WbbState): k_wbb reads
 * it, k_wbb_hist (one writer per capture, behind k_wbb on the stream)
 * advances it, k_wbb_set_state rewrites it for a reset -- calls, resets and
 * parameter changes stay queued with no host synchronisation and no staging
 * image that would have to outlive the call. */
template <bool S16, bool EVEN> __global__ __launch_bounds__(256) void k_wbb(WbbArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char wbb_smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // the workgroup's group and its capture
  const int *grp = a.groups + 3 * (size_t)blockIdx.y;
  const int cap = grp[0], c0 = grp[1], cn = grp[2];
  const size_t sb = S16 ? 4 : 2; // bytes of a wide sample
  const unsigned char *cin = static_cast<const unsigned char *>(a.in) + (size_t)cap * a.wide_stride * sb;
  const unsigned char *chist = static_cast<const unsigned char *>(a.hist) + (size_t)cap * (size_t)(a.L - 1) * sb;
  const int valid = a.state[cap].valid;
  const uint32_t base_mod = (uint32_t)(a.state[cap].counter % (uint64_t)a.fs);
  const int n0 = (int)blockIdx.x * 16 * a.nt; // first output of the workgroup
  const int NI = (16 * a.nt - 1) * a.D + a.Lp; // samples of the window
  const int NIp = (NI + 7) & ~7;
  _Float16 *ih = reinterpret_cast<_Float16 *>(wbb_smem);
  _Float16 *qh = ih + NIp, *il = qh + NIp, *ql = il + NIp; // il, ql: s16 only
  // image entry idx = wide sample a0 + idx of this call (negative: the history)
  const long a0 = (long)n0 * a.D - (a.Lp - 1);
  const long n_in = (long)a.n_out * a.D;
  for (int idx = tid; idx < NIp; idx += 256) {
    const long i = a0 + idx;
    int vi = 0, vq = 0; // before the stream's start and past the call's input: zeros
    if (idx < NI && i >= -(long)valid && i < n_in) {
      if (S16) {
        const int16_t *src = i < 0 ? reinterpret_cast<const int16_t *>(chist) + 2 * (a.L - 1 + i)
                                   : reinterpret_cast<const int16_t *>(cin) + 2 * i;
        if (i < 0 || a.in_al) {
          const uint32_t v = *reinterpret_cast<const uint32_t *>(src);
          vi = (int16_t)(v & 0xFFFFu);
          vq = (int16_t)(v >> 16);
        } else {
          vi = src[0];
          vq = src[1];
        }
      } else {
        const uint8_t *src = i < 0 ? reinterpret_cast<const uint8_t *>(chist) + 2 * (a.L - 1 + i)
                                   : reinterpret_cast<const uint8_t *>(cin) + 2 * i;
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
  // a ragged group computes its last channel again in the spare rows (not stored)
  const int ca = c0 + min(col, cn - 1);
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
    // lane: output nt0 + col of the group's channels 4 g + i
    const int n = nt0 + col;
    if (n >= a.n_out) continue;
    const uint64_t smod = ((uint64_t)base_mod + (uint64_t)n * (uint64_t)a.D) % a.fs; // the output's sample index mod Fs
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (4 * g + i >= cn) break;
      const int c = c0 + 4 * g + i;
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

// k_wb_hist with a capture dimension (blockIdx.y): the last L - 1 raw samples
// of (history, this call's row) of every capture into the other history
// buffer.  Thread 0 of a capture's first workgroup then advances the
// capture's state: nothing in this kernel reads it, and k_wbb, its one
// reader, has ended before this kernel starts.
template <typename T> __global__ void k_wbb_hist(WbbArgs a) {
  const int j = (int)blockIdx.x * 256 + threadIdx.x;
  const int cap = (int)blockIdx.y;
  const long n_in = (long)a.n_out * a.D;
  if (j == 0) {
    WbbState *s = a.state + cap;
    s->valid = (int)min((long)(a.L - 1), (long)s->valid + n_in);
    s->counter += (uint64_t)n_in;
  }
  if (j >= a.L - 1) return;
  const T *cin = static_cast<const T *>(a.in) + 2 * (size_t)cap * a.wide_stride;
  const T *chist = static_cast<const T *>(a.hist) + 2 * (size_t)cap * (size_t)(a.L - 1);
  const long i = n_in - (a.L - 1) + j;
  const T *src = i >= 0 ? cin + 2 * i : chist + 2 * (j + n_in);
  T *dst = static_cast<T *>(a.hist_out) + 2 * ((size_t)cap * (size_t)(a.L - 1) + (size_t)j);
  dst[0] = src[0];
  dst[1] = src[1];
}

// a reset on the stream: one thread, its values by argument
__global__ void k_wbb_set_state(WbbState *state, int S, int capture, uint64_t counter) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  for (int s = capture < 0 ? 0 : capture; s < (capture < 0 ? S : capture + 1); ++s) {
    state[s].counter = counter;
    state[s].valid = 0; // k_wbb reads zeros for samples before the stream's start
  }
}

// a capture's signal parameters on the stream: one thread, the values by argument
__global__ void k_wbb_set_params(double *sp, int S, int capture, double v0, double v1, double v2, double v3) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  for (int s = capture < 0 ? 0 : capture; s < (capture < 0 ? S : capture + 1); ++s) {
    sp[4 * s] = v0;
    sp[4 * s + 1] = v1;
    sp[4 * s + 2] = v2;
    sp[4 * s + 3] = v3;
  }
}

template <bool S16, bool EVEN> static int wbb_launch(const WbbArgs &a, size_t smem, dim3 grid, hipStream_t st) {
  static bool configured = false;
  if (!configured) {
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(&k_wbb<S16, EVEN>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, WB_LDS_MAX) != hipSuccess)
      return FMX_E_HIP;
    configured = true;
  }
  hipLaunchKernelGGL((k_wbb<S16, EVEN>), grid, dim3(256), smem, st, a);
  return hipGetLastError() == hipSuccess ? FMX_OK : FMX_E_HIP;
}

int launch_wbb(const WbbArgs &a0, void *stream) {
  WbbArgs a = a0;
  if (a.S <= 0 || a.n_out <= 0) return FMX_OK;
  if (a.S > FMX_WBB_CAPTURES_MAX || a.G < 0 || a.G > FMX_WBB_GROUPS_MAX || a.C < 0 ||
      a.wide_stride < (size_t)a.n_out * (size_t)a.D)
    return FMX_E_INVALID;
  if (a.D < 2 || a.L != (a.L / a.D) * a.D || a.Lp < a.L || (a.Lp & 31)) return FMX_E_INVALID;
  // wb_tiles and launch_wb's LDS size: the tiling is the single object's
  WbArgs t{};
  t.s16 = a.s16;
  t.D = a.D;
  t.Lp = a.Lp;
  t.n_out = a.n_out;
  a.nt = wb_tiles(t);
  if (a.nt < 1) return FMX_E_INVALID;
  const uintptr_t al = a.s16 ? 3 : 1; // every row starts a whole number of samples behind the base
  a.in_al = (reinterpret_cast<uintptr_t>(a.in) & al) == 0;
  const int NI = (16 * a.nt - 1) * a.D + a.Lp;
  const size_t smem = (size_t)((NI + 7) & ~7) * (a.s16 ? 8 : 4);
  if (smem > WB_LDS_MAX) return FMX_E_INVALID;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (a.G > 0) {
    const dim3 grid((unsigned)((a.n_out + 16 * a.nt - 1) / (16 * a.nt)), (unsigned)a.G);
    const bool even = (a.D & 1) == 0;
    int rc;
    if (a.s16) rc = even ? wbb_launch<true, true>(a, smem, grid, st) : wbb_launch<true, false>(a, smem, grid, st);
    else rc = even ? wbb_launch<false, true>(a, smem, grid, st) : wbb_launch<false, false>(a, smem, grid, st);
    if (rc != FMX_OK) return rc;
  }
  const dim3 hgrid((unsigned)((a.L - 1 + 255) / 256), (unsigned)a.S);
  if (a.s16) hipLaunchKernelGGL(k_wbb_hist<int16_t>, hgrid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(k_wbb_hist<uint8_t>, hgrid, dim3(256), 0, st, a);
  return hipGetLastError() == hipSuccess ? FMX_OK : FMX_E_HIP;
}

int launch_wbb_set_state(WbbState *state, int S, int capture, uint64_t counter, void *stream) {
  if (!state || S < 1 || capture < -1 || capture >= S) return FMX_E_INVALID;
  hipLaunchKernelGGL(k_wbb_set_state, dim3(1), dim3(1), 0, static_cast<hipStream_t>(stream), state, S, capture, counter);
  return hipGetLastError() == hipSuccess ? FMX_OK : FMX_E_HIP;
}

int launch_wbb_set_params(double *sp, int S, int capture, const double *v, void *stream) {
  if (!sp || !v || S < 1 || capture < -1 || capture >= S) return FMX_E_INVALID;
  hipLaunchKernelGGL(k_wbb_set_params, dim3(1), dim3(1), 0, static_cast<hipStream_t>(stream), sp, S, capture, v[0], v[1],
                     v[2], v[3]);
  return hipGetLastError() == hipSuccess ? FMX_OK : FMX_E_HIP;
}

/* ---- the bank's RF level (fmx_wb_bank_signal): k_wb_scan_clip and k_wb_level with a capture dimension ---- */
// k_wb_scan_clip's counting, the same 2048 samples per workgroup, over row
// blockIdx.y of the call's input: the counts to clip[capture][workgroup][2]
template <typename T> __global__ __launch_bounds__(256) void k_wbb_clip(WbbLevelArgs a) {
  __shared__ uint32_t red[4][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long n_in = (long)a.n * a.D;
  const T *in = static_cast<const T *>(a.in) + 2 * (size_t)blockIdx.y * a.wide_stride;
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
  if (tid < 2)
    a.clip[2 * ((size_t)blockIdx.y * a.nclip + blockIdx.x) + tid] = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
}

// k_wb_level; the channel's capture selects the clip partials and the
// parameter set.  The sum's order is k_wb_level's, a function of n alone.
template <int W> __global__ __launch_bounds__(256) void k_wbb_level(WbbLevelArgs a) {
  __shared__ double red[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = (int)blockIdx.x; // the grid is C workgroups
  const float *row = a.rows + (size_t)c * 2 * (size_t)a.stride;
  const int np = (a.n + 1) >> 1; // pairs, the last one half empty at an odd n
  double acc = 0.0;
#pragma unroll 4
  for (int p = tid; p < np; p += 256) {
    const float *s = row + 4 * (size_t)p;
    const bool two = 2 * p + 1 < a.n; // nothing past sample n - 1 is read
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
  if (tid != 0) return;
  const double sum = ((red[0] + red[1]) + red[2]) + red[3];
  const int cap = a.chan_cap[c];
  const uint32_t *clip = a.clip + 2 * (size_t)cap * a.nclip;
  unsigned long long hard = 0, nearc = 0;
  for (int k = 0; k < a.nclip; ++k) {
    hard += clip[2 * k];
    nearc += clip[2 * k + 1];
  }
  const double nn = (double)((long)a.n * a.D);
  const double pw = sum / (double)a.n;
  const double *sp = a.sp + 4 * (size_t)cap; // gain*factor, bias, floor, ceil
  // the record as k_wb_level forms it
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
  float *sm = a.sm + 2 * (size_t)c;
  if (sm[1] == 0.0f) {
    sm[0] = r.level120;
    sm[1] = 1.0f;
  } else {
    const float alpha = (r.level120 > sm[0]) ? 0.42f : 0.18f;
    sm[0] += (r.level120 - sm[0]) * alpha;
  }
  r.level120_smoothed = sm[0];
  a.level[c] = r;
}

int launch_wbb_level(const WbbLevelArgs &a0, void *stream) {
  WbbLevelArgs a = a0;
  if (a.C <= 0 || a.S <= 0 || a.n <= 0 || a.stride < a.n || a.D < 1 || !a.rows || !a.in || !a.clip || !a.sm || !a.level ||
      !a.chan_cap || !a.sp || a.wide_stride < (size_t)a.n * (size_t)a.D)
    return FMX_E_INVALID;
  if ((reinterpret_cast<uintptr_t>(a.rows) & 3) || (reinterpret_cast<uintptr_t>(a.level) & 7)) return FMX_E_INVALID;
  a.nclip = wb_scan_clip_workgroups((long)a.n * a.D);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 cgrid((unsigned)a.nclip, (unsigned)a.S);
  if (a.s16) hipLaunchKernelGGL(k_wbb_clip<int16_t>, cgrid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(k_wbb_clip<uint8_t>, cgrid, dim3(256), 0, st, a);
  if (hipGetLastError() != hipSuccess) return FMX_E_HIP;
  const uintptr_t base = reinterpret_cast<uintptr_t>(a.rows);
  const dim3 grid((unsigned)a.C);
  if ((base & 15) == 0 && (a.stride & 1) == 0) hipLaunchKernelGGL(k_wbb_level<16>, grid, dim3(256), 0, st, a);
  else if ((base & 7) == 0) hipLaunchKernelGGL(k_wbb_level<8>, grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(k_wbb_level<4>, grid, dim3(256), 0, st, a);
  return hipGetLastError() == hipSuccess ? FMX_OK : FMX_E_HIP;
}
