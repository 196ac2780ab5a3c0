/* ================================================================== */
/* k_bscan: the band scan over a capture bank -- every scan point of   */
/* S wide captures read by one launch (fmx_wb_bank_scan_*, DESIGN.md   */
/* section 28)                                                         */
/* ================================================================== */
/* Capture s owns the points [first_point[s], first_point[s + 1]) and row s of
 * the call's input [S][wide_stride].  The work is a flat device table of
 * entries {capture, first point, points 1..64} (fmx_wb_bank_scan_groups): one
 * per 64 points of a capture, none for an empty capture, blockIdx.y its index.
 * k_bscan is k_wb_scan's use of the shared pieces (fmx_wb_core.inc: wb_stage
 * without history, wb_scan_mac, wb_scan_reduce_store) with the row taken from
 * the entry's capture and the wave's 16 points from the entry: the image, the
 * chains, the tiling (wb_scan_tiles, wb_scan_workgroups, the grid starting at
 * output tpp) and the column reduction are the one definition k_wb_scan runs,
 * so a point's sum order stays fixed by (D, Lp, format, n_out) alone and its
 * record is bit for bit that of an fmx_wb_scan object fed the capture's row.
 * Partials go to a slot per (entry, wave): partial[4 entry + wave][workgroup]
 * [16].  No atomics, no rotation, no history.  The clip counts are k_wbb_clip's
 * (clip[capture][workgroup][2]) and the parameter sets k_wbb_set_params' on
 * the object's own [S][4] table; k_bscan_level finds a point's slot and
 * capture in two small tables built at creation. */
template <bool S16, bool EVEN> __global__ __launch_bounds__(256) void k_bscan(BscanArgs a) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // the workgroup's entry and its capture's row
  const int *ent = a.groups + 3 * (size_t)blockIdx.y;
  const int cap = ent[0], p0 = ent[1], pn = ent[2];
  const size_t sb = S16 ? 4 : 2; // bytes of a wide sample
  const unsigned char *cin = static_cast<const unsigned char *>(a.in) + (size_t)cap * a.wide_stride * sb;
  const int n0 = a.tpp + (int)blockIdx.x * 16 * a.nt; // first output of the workgroup
  const int NI = (16 * a.nt - 1) * a.D + a.Lp;       // samples of the window
  const int NIp = (NI + 7) & ~7;
  const WbImage m = wb_image(NIp);
  // as k_wb_scan: the entries before sample 0 meet the rows' zero padding only,
  // and nothing of the row at or past sample n_out D is read
  wb_stage<S16, false>(m, NI, NIp, (long)n0 * a.D - (a.Lp - 1), (long)a.n_out * a.D, 0, cin, nullptr, 0, a.in_al, tid);
  if (16 * wave >= pn) return; // the entry's points [16 wave, 16 wave + 16)
  const int col = lane & 15, g = lane >> 4;
  // a ragged wave computes its last point again in the spare rows (not read)
  const int pa = p0 + min(16 * wave + col, pn - 1);
  // tiles of the workgroup that hold an output below n_out (wave-uniform)
  const int tiles = min(a.nt, (a.n_out - n0 + 15) >> 4);
  wb_f32x4 rr[WB_SCAN_NT], ii[WB_SCAN_NT], ri[WB_SCAN_NT], ir[WB_SCAN_NT];
  wb_scan_mac<S16, EVEN>(m, a.w + (size_t)pa * 4 * a.Lp + 8 * g, a.Lp, a.D, col, g, tiles, rr, ii, ri, ir);
  // lane: output n0 + 16 t + col of the wave's points 4 g + i
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
  const size_t slot = 4 * (size_t)blockIdx.y + wave;
  wb_scan_reduce_store(pw, col, a.partial + (slot * gridDim.x + blockIdx.x) * 16 + 4 * g);
}

// One lane per point: its slot's partials over the workgroups in index order,
// in double, to the record with its capture's clip counts and parameter set --
// k_wb_scan_level's arithmetic term for term
__global__ __launch_bounds__(64) void k_bscan_level(BscanArgs a) {
  const int p = (int)blockIdx.x * 64 + threadIdx.x;
  if (p >= a.P) return;
  const int at = a.pt_slot[p], cap = a.pt_cap[p]; // 16 slot + the point's column of it
  const float *pp = a.partial + (size_t)(at >> 4) * a.nwg * 16 + (at & 15);
  double sum = 0.0;
  for (int wg = 0; wg < a.nwg; ++wg) sum += (double)pp[(size_t)wg * 16];
  a.level[p] = wb_level_record(sum, a.pscale, (double)(a.n_out - a.tpp), a.clip + 2 * (size_t)cap * a.nclip, a.nclip,
                               (double)((long)a.n_out * a.D), a.sp + 4 * (size_t)cap, a.sm + 2 * (size_t)p);
}

// k_wbb_clip over the n_out D raw samples of every row, the scan kernel
// (k_bscan, or fmx_wb_bank_scan_iqc.inc's) over (workgroups of the call) x
// (entries), k_bscan_level over the points
template <class Launch> static int bscan_run(const BscanArgs &a0, void *stream, Launch launch) {
  BscanArgs a = a0;
  if (a.P <= 0 || a.S <= 0 || a.S > FMX_WBB_CAPTURES_MAX || a.G <= 0 || a.G > FMX_WBB_GROUPS_MAX || a.D < 2 || a.tpp < 1 ||
      a.Lp < a.D * a.tpp || (a.Lp & 31) || a.n_out <= a.tpp || a.wide_stride < (size_t)a.n_out * (size_t)a.D)
    return FMX_E_INVALID;
  if (!a.in || !a.w || !a.groups || !a.pt_slot || !a.pt_cap || !a.partial || !a.clip || !a.sm || !a.level || !a.sp)
    return FMX_E_INVALID;
  a.nt = wb_scan_tiles(a.D, a.Lp, a.s16); // the tiling is the single scan's
  if (a.nt < 1) return FMX_E_INVALID;
  a.nwg = wb_scan_workgroups(a.n_out, a.tpp, a.nt);
  a.nclip = wb_scan_clip_workgroups((long)a.n_out * a.D);
  a.in_al = wb_in_aligned(a.in, a.s16); // every row starts a whole number of samples behind the base
  const size_t smem = wb_lds_bytes((16 * a.nt - 1) * a.D + a.Lp, a.s16);
  if (smem > WB_LDS_MAX) return FMX_E_INVALID;
  hipStream_t st = static_cast<hipStream_t>(stream);
  WbbLevelArgs c{}; // what k_wbb_clip reads: in, wide_stride, n_in, clip, nclip
  c.in = a.in;
  c.wide_stride = a.wide_stride;
  c.n_in = (long)a.n_out * a.D;
  c.clip = a.clip;
  c.nclip = a.nclip;
  const dim3 cgrid((unsigned)a.nclip, (unsigned)a.S);
  if (a.s16) hipLaunchKernelGGL(k_wbb_clip<int16_t>, cgrid, dim3(256), 0, st, c);
  else hipLaunchKernelGGL(k_wbb_clip<uint8_t>, cgrid, dim3(256), 0, st, c);
  if (hipGetLastError() != hipSuccess) return FMX_E_HIP;
  const int rc = launch(a, smem, dim3((unsigned)a.nwg, (unsigned)a.G), st);
  if (rc != FMX_OK) return rc;
  hipLaunchKernelGGL(k_bscan_level, dim3((unsigned)((a.P + 63) / 64)), dim3(64), 0, st, a);
  return hipGetLastError() == hipSuccess ? FMX_OK : FMX_E_HIP;
}

int launch_bscan(const BscanArgs &a0, void *stream) {
  return bscan_run(a0, stream, [](const BscanArgs &a, size_t smem, dim3 grid, hipStream_t st) {
    return WB_LAUNCH(k_bscan, a.s16, (a.D & 1) == 0, grid, smem, st, a);
  });
}
