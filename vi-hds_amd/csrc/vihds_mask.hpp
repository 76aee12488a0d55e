// Missing observations of generated models (vihds/modelgen.py: missing_observations = True; vihds_models.hpp: masked_obs<M>).
// A data row of such a model carries one mask word per time point in its row of cond, behind the forcing samples and ahead of
// the noise key:  [n_conditions treatments | K x T forcing samples | T mask words | key lo, key hi].  Word k is the float
//     sum_j observed[j][k] * 2^j          (an integer 0 .. 15, exact in float32; bit j: signal j has a read at point k)
// At the scoring point of time point k and signal j, with m = bit j of (int)word_k,
//     ob'   = m ? obs[j][k] : xp[j]       the predicted signal stands in for the placeholder: the residual-0 point of any density
//     lp[j] += m ? term(ob') : 0          forward
//     seed  = m ? glp[j] : 0              adjoint (the residuals are formed from ob' as well)
// Everything is a select: the placeholder under the mask (NaN, inf, anything) never enters the arithmetic, nothing is multiplied
// by 0 and no branch depends on the data.
//
// ObsMask is the one place the word is decoded: the forward time loop and the adjoint both ask it.  It is __host__ __device__
// and uses no HIP intrinsic: a stand-alone host program can run it (tests/test_modelgen_missing_host.py compiles one with the
// address and undefined-behaviour sanitizers).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VIHDS_MASK_HD __host__ __device__ __forceinline__
#else
#define VIHDS_MASK_HD inline
#endif

namespace vihds {

constexpr int kMaskSignals = 4;  // bits of a mask word: the four observed signals

struct ObsMask {
  int bits;  // bit j set: signal j is observed at this time point
  VIHDS_MASK_HD ObsMask() : bits((1 << kMaskSignals) - 1) {}
  // (the host wrote an integer 0 .. 15; whatever else arrives -- a NaN, a negative or a huge value -- decodes to a defined
  // 4-bit pattern without a conversion that is undefined: the comparison is false for a NaN)
  VIHDS_MASK_HD explicit ObsMask(float word)
      : bits((word >= 0.f && word < 16.f) ? ((int)word & ((1 << kMaskSignals) - 1)) : 0) {}
  VIHDS_MASK_HD bool observed(int j) const { return ((bits >> j) & 1) != 0; }
  // ob': the read where there is one, the predicted signal where there is none
  VIHDS_MASK_HD float read(int j, float ob, float xp) const { return observed(j) ? ob : xp; }
  // a log-likelihood term, or the seed of its adjoint: itself where the signal is observed, 0 where it is not
  VIHDS_MASK_HD float gate(int j, float v) const { return observed(j) ? v : 0.f; }
};

// the word the host writes for the four flags of one time point (vihds.modelgen.mask_words is this sum)
VIHDS_MASK_HD float mask_word(bool o0, bool o1, bool o2, bool o3) {
  return (float)((o0 ? 1 : 0) + (o1 ? 2 : 0) + (o2 ? 4 : 0) + (o3 ? 8 : 0));
}

}  // namespace vihds
