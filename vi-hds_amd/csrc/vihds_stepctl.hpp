// Error-controlled sub-steps per trajectory for generated models (vihds/modelgen.py: step_tolerance = (rtol, atol) beside
// substeps = M; vihds_models.hpp: step_control<M>).  Every trajectory picks, for every observation interval [t_k, t_k+1], its
// own number of steps of the model's scheme by step doubling, 1 -> 2 -> 4 -> .. -> M, defined exactly -- with Phi^c the c
// steps of the scheme from y_k on the times of a sub-grid with c steps (SubGridN below):
//     coarse = Phi^1(y_k);  c = 1
//     repeat:
//         fine = Phi^2c(y_k)
//         r = max over species i of |fine_i - coarse_i| / (atol + rtol * max(|fine_i|, |coarse_i|))
//         if r <= 1:    y_k+1 = fine, count = 2c, passed;      stop
//         if 2c == M:   y_k+1 = fine, count = M,  saturated;   stop
//         coarse = fine;  c = 2c
// A NaN or infinite r fails the test (it is written r <= 1.f).  The result travels as one float per time point in the last row
// of the trajectory buffer: at point k + 1 the count of the interval that ended there, +count where the test passed and -M
// where the ladder was exhausted (the tolerance was not met there); 0 at point 0.  The adjoint reads that row and never
// repeats the ladder: the counts are frozen, a choice carries no gradient.
//
// The functions below are the one place the sub-grid times, the ratio and the row's code are formed.  They are __host__
// __device__ and use no HIP intrinsic: a stand-alone host program can run them (tests/test_modelgen_stepctl_host.py compiles one
// with the address and undefined-behaviour sanitizers).
#pragma once

#include "vihds_substeps.hpp"

namespace vihds {

// SubGrid<MS> with a run-time count c >= 1: the same formulas, so for c = 1, 2, 4, 8 (1.f / c is exact) the same bits
struct SubGridN {
  float t_lo, t_hi, hs;
  int c;
  VIHDS_SUB_HD SubGridN(float t0, float t1, int count) : t_lo(t0), t_hi(t1), hs((t1 - t0) * (1.f / (float)count)), c(count) {}
  // s_j, j = 0 .. c
  VIHDS_SUB_HD float at(int j) const { return j < c ? __builtin_fmaf((float)j, hs, t_lo) : t_hi; }
};

// r of the acceptance test over the N species.  A NaN term makes r NaN (fmaxf would drop it), so the caller's r <= 1.f fails
template <int N>
VIHDS_SUB_HD float step_ratio(const float* fine, const float* coarse, float rtol, float atol) {
  float r = 0.f, nan_term = 0.f;
  bool bad = false;
  for (int i = 0; i < N; ++i) {
    const float af = __builtin_fabsf(fine[i]), ac = __builtin_fabsf(coarse[i]);
    const float q = __builtin_fabsf(fine[i] - coarse[i]) / (atol + rtol * (af > ac ? af : ac));
    if (!(q == q)) {
      bad = true;
      nan_term = q;
    }
    r = q > r ? q : r;
  }
  return bad ? nan_term : r;
}

// the row's float of an interval: +count where the test passed, -ceiling where the ladder was exhausted
VIHDS_SUB_HD float step_code(int count, bool passed) { return passed ? (float)count : -(float)count; }
// ... and the count the adjoint runs with: |code| clamped into 1 .. ceiling before it bounds a loop or indexes LDS (a zeroed or
// foreign row -- 0, NaN, anything -- gives a count in range)
VIHDS_SUB_HD int step_count_of(float code, int ceiling) {
  const float m = __builtin_fabsf(code);
  if (!(m >= 1.f)) return 1;
  return m >= (float)ceiling ? ceiling : (int)m;
}

}  // namespace vihds
