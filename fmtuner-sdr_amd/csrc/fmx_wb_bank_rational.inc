/* ================================================================== */
/* k_rbank: the capture bank at rational rates -- S wide captures of    */
/* one P / Q plan channelized by one launch                             */
/* (fmx_wb_bank_create_rational, DESIGN.md section 27)                  */
/* ================================================================== */
/* k_wbr's tile list with k_wbb's capture dimension.  blockIdx.x runs over
 * k_wbr's tile workgroups (wbr_group: tiles T = mb Q + r, nt per workgroup,
 * one staged window for them), blockIdx.y over the bank's group table
 * {capture, first channel, channels 1..16}.  A workgroup takes in, hist, valid
 * and base_mod from its group's capture -- row cap of the call's input,
 * cap (Lh - 1) samples into the histories, WbbState[cap] -- and its weight
 * rows from the group's channels: [c][r][4][Lp].  The image, the chains and
 * the rotation are the family's (fmx_wb_core.inc), the frame and the tile
 * offsets k_wbr's (wbr_group, wbr_tile_offset), every phase runs the full
 * Lp / 32 K steps: a capture's rows are bit for bit those of an
 * fmx_wb_create_rational object fed its row, however the stream is cut into
 * calls.  k_rbank_hist (behind k_rbank on the stream) keeps every capture's
 * last Lh - 1 raw samples and advances its state by n_out / Q * P samples. */
template <bool S16, bool PEVEN> __global__ __launch_bounds__(256) void k_rbank(RbankArgs a) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // the workgroup's group and its capture
  const int *grp = a.groups + 3 * (size_t)blockIdx.y;
  const int cap = grp[0], c0 = grp[1], cn = grp[2];
  const size_t sb = S16 ? 4 : 2; // bytes of a wide sample
  const unsigned char *cin = static_cast<const unsigned char *>(a.in) + (size_t)cap * a.wide_stride * sb;
  const unsigned char *chist = static_cast<const unsigned char *>(a.hist) + (size_t)cap * (size_t)(a.Lh - 1) * sb;
  const int valid = a.state[cap].valid;
  const uint32_t base_mod = (uint32_t)(a.state[cap].counter % (uint64_t)a.fs);
  const WbrGroup wg = wbr_group((int)blockIdx.x, a.nt, a.ntiles, a.P, a.Q, a.a[a.Q - 1], a.Lp);
  const int T0 = wg.T0, T1 = wg.T1, mb0 = wg.mb0, NI = wg.window;
  const int NIp = (NI + 7) & ~7;
  const WbImage img = wb_image(NIp);
  wb_stage<S16, true>(img, NI, NIp, (long)mb0 * 16 * a.P - (a.Lp - 1), a.n_in, valid, cin, chist, a.Lh, a.in_al, tid);
  const int col = lane & 15, g = lane >> 4;
  const int M = a.n_out / a.Q; // outputs per phase
  // a ragged group computes its last channel again in the spare rows (not stored)
  const int ca = c0 + min(col, cn - 1);
  for (int T = T0 + wave; T <= T1; T += 4) {
    const int mb = T / a.Q, r = T - mb * a.Q;
    const int ar = a.a[r];
    const uint16_t *wrow = a.w + ((size_t)ca * a.Q + r) * 4 * a.Lp + 8 * g;
    const int xb = wbr_tile_offset(a.P, a.Q, ar, T, mb0) + col * a.P + 8 * g;
    wb_f32x4 rr, ii, ri, ir;
    if (PEVEN && (ar & 1) == 0) wb_tile<S16, true>(img, xb, wrow, a.Lp, rr, ii, ri, ir);
    else wb_tile<S16, false>(img, xb, wrow, a.Lp, rr, ii, ri, ir);
    // lane: output (16 mb + col) Q + r of the group's channels 4 g + i
    const int m = 16 * mb + col;
    if (m >= M) continue;
    const int n = m * a.Q + r;
    const uint64_t i0 = (uint64_t)m * (uint64_t)a.P + (uint64_t)ar;
    const uint64_t smod = ((uint64_t)base_mod + i0) % a.fs; // the output's sample index mod Fs
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (4 * g + i >= cn) break;
      const int c = c0 + 4 * g + i;
      wb_rotate_store(a.fpos[c], smod, a.fs, a.inv_fs, rr[i] - ii[i], ri[i] + ir[i], a.scale,
                      a.out + 2 * ((size_t)c * a.out_stride + n));
    }
  }
}

// k_wbr_hist with a capture dimension (blockIdx.y), and k_wbb_hist's state
// advance by thread 0 of a capture's first workgroup: nothing in this kernel
// reads the state, and k_rbank, its one reader, has ended before this kernel
// starts.
template <typename T> __global__ void k_rbank_hist(RbankArgs a) {
  const int j = (int)blockIdx.x * 256 + threadIdx.x;
  const int cap = (int)blockIdx.y;
  if (j == 0) {
    WbbState *s = a.state + cap;
    s->valid = (int)min((long)(a.Lh - 1), (long)s->valid + a.n_in);
    s->counter += (uint64_t)a.n_in;
  }
  if (j >= a.Lh - 1) return;
  const T *cin = static_cast<const T *>(a.in) + 2 * (size_t)cap * a.wide_stride;
  const T *chist = static_cast<const T *>(a.hist) + 2 * (size_t)cap * (size_t)(a.Lh - 1);
  const long i = a.n_in - (a.Lh - 1) + j;
  const T *src = i >= 0 ? cin + 2 * i : chist + 2 * (j + a.n_in);
  T *dst = static_cast<T *>(a.hist_out) + 2 * ((size_t)cap * (size_t)(a.Lh - 1) + (size_t)j);
  dst[0] = src[0];
  dst[1] = src[1];
}

int launch_rbank(const RbankArgs &a0, void *stream) {
  RbankArgs a = a0;
  if (a.S <= 0 || a.n_out <= 0) return FMX_OK;
  if (a.S > FMX_WBB_CAPTURES_MAX || a.G < 0 || a.G > FMX_WBB_GROUPS_MAX || a.C < 0) return FMX_E_INVALID;
  if (a.Q < 1 || a.Q > FMX_WBR_QMAX || a.P < 2 * a.Q || a.n_out % a.Q != 0 || a.Lh < 1 || a.Lp < a.Lh || (a.Lp & 31))
    return FMX_E_INVALID;
  for (int r = 0; r < a.Q; ++r)
    if (a.a[r] != (int)((long)r * a.P / a.Q)) return FMX_E_INVALID;
  a.n_in = (long)a.n_out / a.Q * a.P;
  if (a.wide_stride < (size_t)a.n_in) return FMX_E_INVALID;
  a.nt = wbr_tiles(a.P, a.Q, a.a[a.Q - 1], a.Lp, a.s16, a.n_out); // the tiling is the single object's
  if (a.nt < 1) return FMX_E_INVALID;
  a.ntiles = (a.n_out / a.Q + 15) / 16 * a.Q;
  a.in_al = wb_in_aligned(a.in, a.s16); // every row starts a whole number of samples behind the base
  // the largest window of any workgroup: nt tiles from the last phase on
  const int span = 1 + (a.nt - 1 + a.Q - 1) / a.Q;
  const int NI = wbr_window(a.P, a.a[a.Q - 1], a.Lp, 0, span - 1);
  const size_t smem = wb_lds_bytes(NI, a.s16);
  if (smem > WB_LDS_MAX) return FMX_E_INVALID;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (a.G > 0) {
    const dim3 grid((unsigned)((a.ntiles + a.nt - 1) / a.nt), (unsigned)a.G);
    const int rc = WB_LAUNCH(k_rbank, a.s16, (a.P & 1) == 0, grid, smem, st, a);
    if (rc != FMX_OK) return rc;
  }
  const dim3 hgrid((unsigned)std::max(1, (a.Lh - 1 + 255) / 256), (unsigned)a.S);
  if (a.s16) hipLaunchKernelGGL(k_rbank_hist<int16_t>, hgrid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(k_rbank_hist<uint8_t>, hgrid, dim3(256), 0, st, a);
  return hipGetLastError() == hipSuccess ? FMX_OK : FMX_E_HIP;
}
