// Sub-steps per observation interval for generated models (vihds/modelgen.py: substeps = m; vihds_models.hpp: substeps<M>).
// A fixed-grid scheme takes m steps of its own over each observation interval [t_k, t_k+1], defined exactly -- with
//     hs = (t_k+1 - t_k) * (1.f / m)
// sub-step j = 0 .. m-1 runs from s_j to s_j+1, where
//     s_j = fmaf((float)j, hs, t_k)  for j < m,      s_m = t_k+1 exactly
// so s_0 = t_k and the last sub-step ends on the observation point itself, whatever the rounding of hs.  modeuler's fixed
// step h0 becomes h0 * (1.f / m).  Only the states at the observation points are stored, observed and scored.
//
// SubGrid is the one place these times are formed: the forward time loop and the adjoint (which recomputes the interval's
// intermediate states from the stored y_k) both ask it, so the adjoint's sub-states are the forward's bit for bit.
// It is a __host__ __device__ template and uses no HIP intrinsic: a stand-alone host program can run it
// (tests/test_modelgen_substeps_host.py compiles one with the address and undefined-behaviour sanitizers).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VIHDS_SUB_HD __host__ __device__ __forceinline__
#else
#define VIHDS_SUB_HD inline
#endif

namespace vihds {

// the sub-steps a generated model may ask for (vihds.modelgen.MAX_SUBSTEPS)
constexpr int kMaxSubsteps = 8;
// the steps of a lead-in phase before the first observation point (vihds.modelgen.MAX_LEAD_IN_STEPS): SubGrid<n>(t_0 - L, t_0)
constexpr int kMaxLeadInSteps = 8;
static_assert(kMaxLeadInSteps <= kMaxSubsteps, "the lead-in grid is a SubGrid");

template <int MS>
struct SubGrid {
  static_assert(MS >= 1 && MS <= kMaxSubsteps, "substeps: 1 .. 8");
  float t_lo, t_hi, hs;
  VIHDS_SUB_HD SubGrid(float t0, float t1) : t_lo(t0), t_hi(t1), hs((t1 - t0) * (1.f / MS)) {}
  // s_j, j = 0 .. MS
  VIHDS_SUB_HD float at(int j) const { return j < MS ? __builtin_fmaf((float)j, hs, t_lo) : t_hi; }
  // the fixed step of modeuler (the first observation interval's length) for one sub-step
  VIHDS_SUB_HD static float fixed_step(float h0) { return h0 * (1.f / MS); }
};

}  // namespace vihds
