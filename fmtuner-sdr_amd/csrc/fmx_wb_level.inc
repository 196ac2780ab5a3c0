/* ================================================================== */
/* k_wb_level: the RF level of every channel of the channelizer from   */
/* one call's rows (fmx_wb_signal, DESIGN.md section 21)               */
/* ================================================================== */
/* With y_c[m], m = 0 .. n - 1, channel c's row of the call (k_wb's output,
 * the object's own rows after fmx_wb_process_block, the caller's after
 * fmx_wb_process),
 *   P_c = (1 / n) sum_m |y_c[m]|^2
 * and the record as the band scan forms it from its P_p.  One workgroup of
 * four waves per channel: wb_row_power over the row (the load width W is what
 * the rows' base and stride allow; the sum's order is a function of n alone
 * and not of W or the channel count; no atomics), then thread 0 evaluates
 * wb_level_record with k_wb_scan_clip's partials of the call's raw samples
 * (fmx_wb_core.inc). */
template <int W> __global__ __launch_bounds__(256) void k_wb_level(WbLevelArgs a) {
  const int c = (int)blockIdx.x; // the grid is C workgroups
  const double sum = wb_row_power<W>(a.rows + (size_t)c * 2 * (size_t)a.stride, a.n);
  if (threadIdx.x != 0) return;
  a.level[c] = wb_level_record(sum, 1.0, (double)a.n, a.clip, a.nclip, (double)a.n_in, a.sp, a.sm + 2 * (size_t)c);
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
