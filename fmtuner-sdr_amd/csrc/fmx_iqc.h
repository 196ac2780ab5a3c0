// fmx_iqc.h -- the DC / IQ-imbalance estimator's arithmetic (fmx.h,
// "DC offset and IQ imbalance"), shared by the device
// finisher k_iqc_finish (fmx_wb_iqc.inc) and the host's fmx_iq_estimate
// (fmx_wb_design.cpp) so that both evaluate one text.
#ifndef FMX_IQC_H
#define FMX_IQC_H

#include <stdint.h>

#include "../../include/fmx.h"

#ifdef __HIPCC__
#define FMX_IQC_HD __host__ __device__ __forceinline__
#else
#include <cmath>
#define FMX_IQC_HD inline
#endif

// The parameter block of one object, in device memory: the estimator (AUTO)
// or k_iqc_fixed (FIXED) writes it, the corrected kernels read k, and
// fmx_wb_iq_correction reads x back.
struct FmxIqcBlock {
  float k[4];          // d_i, d_q in raw units (2 b - 255 for u8, v for int16), gain, cross
  fmx_iq_correction x; // the same in units of x
  double m[5];         // smoothed raw moments E I, E Q, E I^2, E Q^2, E IQ
  int init;            // m holds a call's moments (0 after the mode is set)
  int pad;
};

// The call's five exact sums over n raw samples -> the block.  unit: raw units
// per unit of x (255 for u8, 32768 for int16).  alpha in (0, 1].
FMX_IQC_HD void fmx_iqc_finish(const long long s[5], long long n, double alpha, double unit, FmxIqcBlock *b) {
  const double nn = (double)n;
  for (int j = 0; j < 5; ++j) {
    const double mc = (double)s[j] / nn;
    b->m[j] = b->init ? b->m[j] + alpha * (mc - b->m[j]) : mc;
  }
  b->init = 1;
  const double mI = b->m[0], mQ = b->m[1];
  const double cII = b->m[2] - mI * mI, cQQ = b->m[3] - mQ * mQ, cIQ = b->m[4] - mI * mQ;
  double gain = 1.0, cross = 0.0;
  if (cII > 0.0) {
    const double v = cQQ - cIQ * cIQ / cII;
    if (v > 1e-9 * cQQ) {
      gain = sqrt(cII / v);
      cross = -gain * cIQ / cII;
    }
  }
  b->x.dc_i = mI / unit;
  b->x.dc_q = mQ / unit;
  b->x.gain = gain;
  b->x.cross = cross;
  b->k[0] = (float)mI;
  b->k[1] = (float)mQ;
  b->k[2] = (float)gain;
  b->k[3] = (float)cross;
}

#endif
