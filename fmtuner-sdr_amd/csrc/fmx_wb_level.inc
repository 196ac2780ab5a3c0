/* ================================================================== */
/* k_wb_level: the RF level of every channel of the channelizer from   */
/* one call's rows (fmx_wb_signal, DESIGN.md section 21)               */
/* ================================================================== */
/* With y_c[m], m = 0 .. n - 1, channel c's row of the call (k_wb's output,
 * the object's own rows after fmx_wb_process_block, the caller's after
 * fmx_wb_process),
 *   P_c = (1 / n) sum_m |y_c[m]|^2
 * and the record as the band scan forms it from its P_p (k_wb_scan_level).
 * One workgroup of four waves per channel.  The row is read as pairs of
 * complex samples: thread t takes the pairs t, t + 256, ... and adds each
 * pair's two terms re re + im im, formed and accumulated in double, in index
 * order; the 64 lanes of a wave are added in a butterfly (xor 32, 16, 8, 4, 2,
 * 1), the four waves through LDS in index order.  The order is a function of
 * n alone -- not of the load width (16 B per pair where the rows' base and
 * stride allow it, else 8 B per sample, else 4 B per float) and not of the
 * channel count; no atomics.  Thread 0 then adds k_wb_scan_clip's partials of
 * the call's raw samples in index order, evaluates the record, advances the
 * channel's smoother and writes the record. */
template <int W> __global__ __launch_bounds__(256) void k_wb_level(WbLevelArgs a) {
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
  unsigned long long hard = 0, nearc = 0;
  for (int k = 0; k < a.nclip; ++k) {
    hard += a.clip[2 * k];
    nearc += a.clip[2 * k + 1];
  }
  const double nn = (double)a.n_in; // the call's raw samples
  const double pw = sum / (double)a.n;
  const double *sp = a.sp; // gain*factor, bias, floor, ceil
  // the record as k_wb_scan_level forms it (signal_level.cpp:187-195, no mean removed)
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

// k_wb_scan_clip over the call's raw samples (the scan's kernel, launched as
// it is: it reads in, n_out, D and clip alone), then one workgroup per channel
int launch_wb_level(const WbLevelArgs &a0, void *stream) {
  WbLevelArgs a = a0;
  if (a.C <= 0 || a.n <= 0 || a.stride < a.n || (a.n_in == 0 && a.D < 1) || !a.rows || !a.in || !a.clip || !a.sm || !a.level)
    return FMX_E_INVALID;
  if ((reinterpret_cast<uintptr_t>(a.rows) & 3) || (reinterpret_cast<uintptr_t>(a.level) & 7)) return FMX_E_INVALID;
  WbScanArgs s{};
  s.in = a.in;
  s.n_out = a.n;
  s.D = a.D;
  if (a.n_in == 0) a.n_in = (long)a.n * a.D;
  else { // a rational object's call: its n_in raw samples, counted as n_in x 1
    if (a.n_in < 0 || a.n_in > 0x7FFFFFFFL) return FMX_E_INVALID;
    s.n_out = (int)a.n_in;
    s.D = 1;
  }
  a.nclip = wb_scan_clip_workgroups(a.n_in);
  hipStream_t st = static_cast<hipStream_t>(stream);
  s.clip = a.clip;
  if (a.s16) hipLaunchKernelGGL(k_wb_scan_clip<int16_t>, dim3((unsigned)a.nclip), dim3(256), 0, st, s);
  else hipLaunchKernelGGL(k_wb_scan_clip<uint8_t>, dim3((unsigned)a.nclip), dim3(256), 0, st, s);
  if (hipGetLastError() != hipSuccess) return FMX_E_HIP;
  const uintptr_t base = reinterpret_cast<uintptr_t>(a.rows);
  const dim3 grid((unsigned)a.C);
  if ((base & 15) == 0 && (a.stride & 1) == 0) hipLaunchKernelGGL(k_wb_level<16>, grid, dim3(256), 0, st, a);
  else if ((base & 7) == 0) hipLaunchKernelGGL(k_wb_level<8>, grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(k_wb_level<4>, grid, dim3(256), 0, st, a);
  return hipGetLastError() == hipSuccess ? FMX_OK : FMX_E_HIP;
}
