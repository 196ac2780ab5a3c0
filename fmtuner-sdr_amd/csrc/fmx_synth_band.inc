// fmx_synth_band.inc -- k_synth_band: the synthetic FM band on the GPU
// (included by fmx_kernels.hip; definition in fmx_synth_band.h, DESIGN.md
// section 30).
//
// Grid (ceil(n / SB_TILE), captures), 256 threads; thread t owns the samples
// t + 256 q of its tile, q < SB_Q, so a wave's stores are contiguous.  The
// cost is the double sin / cos of every station-sample (about ten), so nothing
// else may sit in the sample loop: a residue turn(f, i) = (f i) mod Fs is never
// taken by a 64-bit division there.  Per workgroup and chunk of SB_CHUNK
// stations, the threads stage in LDS each station's constants, the residue of
// each of its nine frequencies at the tile's first sample, and (256 f) mod Fs.
// A thread's first residue is then one reduction of r0 + f t < 2^34, and each
// further sample is an add and a conditional subtract.  The RDS half-bit
// index advances the same way, as quotient (mod 2 n_bits) and remainder of
// 2375 (i + rds_off) / Fs.  The reductions multiply by 1 / Fs in double and
// correct the quotient by at most one, which is exact for operands below 2^52.
constexpr int SB_CHUNK = 16; // stations staged at a time: 16 threads each

struct SbStage {
  fmx_sb_station st;
  uint32_t r0[FMX_SB_RES];   // turn(f, i0); [8]: 57 kHz on i0 + rds_off
  uint32_t step[FMX_SB_RES]; // (256 f) mod Fs
  uint32_t rem0, hb0;        // (2375 nr0) mod Fs, floor(2375 nr0 / Fs) mod 2 n_bits
};

// x = q m + r, 0 <= r < m, for x < 2^52: q from the double product, off by one at the most
__device__ __forceinline__ uint32_t sb_divmod(uint64_t x, uint32_t m, double inv, uint64_t *quo) {
  uint64_t q = (uint64_t)((double)x * inv);
  int64_t r = (int64_t)x - (int64_t)(q * m);
  if (r < 0) {
    r += m;
    --q;
  } else if (r >= (int64_t)m) {
    r -= m;
    ++q;
  }
  *quo = q;
  return (uint32_t)r;
}
__device__ __forceinline__ uint32_t sb_mod(uint64_t x, uint32_t m, double inv) {
  uint64_t q;
  return sb_divmod(x, m, inv, &q);
}

template <bool S16> __global__ __launch_bounds__(256) void k_synth_band(SbArgs a) {
  __shared__ SbStage lds[SB_CHUNK];
  const int t = threadIdx.x, s = blockIdx.y;
  const uint32_t fs = (uint32_t)a.fs;
  const double fsd = (double)a.fs;
  const uint32_t tile0 = blockIdx.x * (uint32_t)SB_TILE;  // < n <= 2^31
  const int64_t i0 = a.sample0 + (int64_t)tile0;
  const uint32_t im0 = sb_mod((uint64_t)a.im0 + tile0, fs, a.inv_fs); // i0 mod Fs
  const uint32_t nb2 = 2u * (uint32_t)a.n_bits;
  const bool rds_on = a.kind == FMX_SYNTH_STEREO_RDS;
  const int nres = a.kind == FMX_SYNTH_MONO ? 3 : 8; // residues in use, the 57 kHz one aside
  double vi[SB_Q], vq[SB_Q];
#pragma unroll
  for (int q = 0; q < SB_Q; ++q) vi[q] = vq[q] = 0.0;

  const int g0 = a.first[s], g1 = a.first[s + 1];
  for (int c0 = g0; c0 < g1; c0 += SB_CHUNK) {
    const int nc = g1 - c0 < SB_CHUNK ? g1 - c0 : SB_CHUNK;
    __syncthreads(); // the chunk before has been read
    {
      const int j = t >> 4, slot = t & 15;
      if (j < nc) {
        const fmx_sb_station *src = a.st + (c0 + j);
        SbStage &L = lds[j];
        for (int d = slot; d < FMX_SB_STATION_DOUBLES; d += 16)
          reinterpret_cast<double *>(&L.st)[d] = reinterpret_cast<const double *>(src)[d];
        if (slot < FMX_SB_RES) {
          const uint32_t fm = src->fm[slot];
          uint32_t im = im0;
          if (slot == FMX_SB_R57) im = sb_mod((uint64_t)(i0 + src->rds_off), fs, a.inv_fs);
          L.st.fm[slot] = fm;
          L.r0[slot] = sb_mod((uint64_t)fm * im, fs, a.inv_fs);
          L.step[slot] = sb_mod((uint64_t)fm << 8, fs, a.inv_fs);
        } else if (slot == FMX_SB_RES && rds_on) {
          uint64_t h0, hq;
          L.rem0 = sb_divmod(2375ull * (uint64_t)(i0 + src->rds_off), fs, a.inv_fs, &h0);
          L.hb0 = sb_divmod(h0, nb2, a.inv_2nb, &hq);
        }
      }
    }
    __syncthreads();
    for (int j = 0; j < nc; ++j) {
      const SbStage &L = lds[j];
      uint32_t r[FMX_SB_RES], step[FMX_SB_RES];
#pragma unroll
      for (int m = 0; m < FMX_SB_RES; ++m) {
        r[m] = 0;
        step[m] = 0;
        if (m < nres || (m == FMX_SB_R57 && rds_on)) {
          r[m] = sb_mod((uint64_t)L.r0[m] + (uint64_t)L.st.fm[m] * (uint32_t)t, fs, a.inv_fs);
          step[m] = L.step[m];
        }
      }
      uint32_t rem = 0, hb = 0;
      const uint8_t *bits = nullptr;
      if (rds_on) {
        uint64_t dq;
        rem = sb_divmod((uint64_t)L.rem0 + 2375u * (uint32_t)t, fs, a.inv_fs, &dq);
        hb = L.hb0 + (uint32_t)dq; // dq <= 2 and hb0 < 2 n_bits, 2 n_bits >= 208
        if (hb >= nb2) hb -= nb2;
        bits = a.bits + (size_t)(c0 + j) * (size_t)a.n_bits;
      }
      const double amp = L.st.amp;
      // one copy of the sample's code: the loop stays rolled, sample q's sums sit in
      // vi[0], vq[0] while it runs, and SB_Q rotations put every sum back in its place
#pragma unroll 1
      for (int q = 0; q < SB_Q; ++q) {
        double rds = 0.0;
        if (rds_on) rds = fmx_sb_rds_sign(bits[hb >> 1], (int)(hb & 1u));
        // fmx_sb_phi with the tone loop rolled as well: the tone's residue sits in r[1]
        // and seven rotations of r[1..7] (two of r[1..2] on a mono band) restore the order
        double p = 0.0;
        if (a.kind == FMX_SYNTH_MONO) {
#pragma unroll 1
          for (int j = 0; j < 2; ++j) {
            p = fmx_sb_tone(j, p, L.st.k[j], L.st.c0[j], L.st.ph[j], r[1], fsd);
            const uint32_t r1 = r[1];
            r[1] = r[2];
            r[2] = r1;
          }
        } else {
#pragma unroll 1
          for (int j = 0; j < FMX_SB_TONES; ++j) {
            p = fmx_sb_tone(j, p, L.st.k[j], L.st.c0[j], L.st.ph[j], r[1], fsd);
            const uint32_t r1 = r[1];
#pragma unroll
            for (int m = 1; m < FMX_SB_TONES; ++m) r[m] = r[m + 1];
            r[FMX_SB_TONES] = r1;
          }
          if (rds_on) p += fmx_sb_rds_term(rds, a.krds, r[FMX_SB_R57], fsd);
        }
        fmx_sb_add(amp, fmx_sb_angle(r[0], fsd) + p, &vi[0], &vq[0]);
        const double ti = vi[0], tq = vq[0];
#pragma unroll
        for (int m = 0; m + 1 < SB_Q; ++m) {
          vi[m] = vi[m + 1];
          vq[m] = vq[m + 1];
        }
        vi[SB_Q - 1] = ti;
        vq[SB_Q - 1] = tq;
#pragma unroll
        for (int m = 0; m < FMX_SB_RES; ++m) {
          r[m] += step[m];
          if (r[m] >= fs) r[m] -= fs;
        }
        if (rds_on) { // 2375 * 256 more: quotient and remainder staged by the launcher
          rem += a.rstep_r;
          hb += a.rstep_q;
          if (rem >= fs) {
            rem -= fs;
            ++hb;
          }
          if (hb >= nb2) hb -= nb2;
        }
      }
    }
  }

  const double fe[4] = {a.fe[4 * s], a.fe[4 * s + 1], a.fe[4 * s + 2], a.fe[4 * s + 3]};
  const uint64_t nbase = fmx_sb_noise_base(a.seed_base, s);
  using E = typename std::conditional<S16, int16_t, uint8_t>::type;
  E *row = static_cast<E *>(a.out) + 2 * (size_t)s * a.wide_stride;
#pragma unroll
  for (int q = 0; q < SB_Q; ++q) {
    const uint32_t n = tile0 + (uint32_t)t + 256u * (uint32_t)q;
    if (n >= (uint32_t)a.n) continue;
    double xi = vi[q], xq = vq[q];
    if (a.noise_std > 0.0) fmx_sb_noise(a.noise_std, nbase, a.sample0 + (int64_t)n, &xi, &xq);
    fmx_sb_frontend(fe, &xi, &xq);
    E *o = row + 2 * (size_t)n;
    if (S16) {
      const uint16_t bi = (uint16_t)fmx_sb_quant_s16(xi), bq = (uint16_t)fmx_sb_quant_s16(xq);
      if (a.wide_store) {
        *reinterpret_cast<uint32_t *>(o) = (uint32_t)bi | ((uint32_t)bq << 16);
      } else {
        o[0] = (E)bi;
        o[1] = (E)bq;
      }
    } else {
      const uint8_t bi = fmx_sb_quant_u8(xi), bq = fmx_sb_quant_u8(xq);
      if (a.wide_store) {
        *reinterpret_cast<uint16_t *>(o) = (uint16_t)((uint16_t)bi | ((uint16_t)bq << 8));
      } else {
        o[0] = (E)bi;
        o[1] = (E)bq;
      }
    }
  }
}

int launch_synth_band(const SbArgs &a0, void *stream) {
  SbArgs a = a0;
  if (a.n <= 0) return FMX_OK;
  if (!a.out || !a.st || !a.first || !a.fe || a.S < 1 || a.S > FMX_SB_CAPTURES_MAX) return FMX_E_INVALID;
  if (a.fs < FMX_SB_RATE_MIN || a.fs > FMX_SB_RATE_MAX || a.wide_stride < (size_t)a.n) return FMX_E_INVALID;
  if (a.kind == FMX_SYNTH_STEREO_RDS && (!a.bits || a.n_bits < 104 || a.n_bits > FMX_SB_NBITS_MAX)) return FMX_E_INVALID;
  const size_t elem = a.s16 ? 2 : 1;
  const uintptr_t p = reinterpret_cast<uintptr_t>(a.out);
  if (p & (elem - 1)) return FMX_E_INVALID;
  // a row starts 2 elem wide_stride bytes after the one before: aligned as the base is
  a.wide_store = (p & (2 * elem - 1)) == 0;
  a.inv_fs = 1.0 / (double)a.fs;
  a.inv_2nb = a.n_bits > 0 ? 1.0 / (2.0 * (double)a.n_bits) : 1.0;
  a.im0 = (uint32_t)(a.sample0 % a.fs);
  a.rstep_q = (2375u * 256u) / (uint32_t)a.fs;
  a.rstep_r = (2375u * 256u) % (uint32_t)a.fs;
  const dim3 grid((unsigned)((a.n + SB_TILE - 1) / SB_TILE), (unsigned)a.S);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (a.s16) hipLaunchKernelGGL(k_synth_band<true>, grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(k_synth_band<false>, grid, dim3(256), 0, st, a);
  return hipGetLastError() == hipSuccess ? FMX_OK : FMX_E_HIP;
}

