// dr_blackbox kernels for the configuration of the reference's specs/dr_blackbox_icml.yaml (BlackboxIcml, vihds_blackbox.hpp).
#include "vihds_ode_kernels.hpp"
#include "vihds_bb_variant.hpp"
#include "vihds_blackbox_split.hpp"

// Compiled TWICE (csrc/Makefile): VIHDS_BB_PART 1 = the forward launch of the cooperating-wavefront kernels alone, built
// with -fno-slp-vectorize (its VALU stream is faster unpacked: 99.0 -> 94.4 us at config 4); everything else -- the adjoint,
// which is faster with LLVM's packed fp32 (213.8 vs 226.6 us), the other variants, the tables -- as part 2 without the flag.
namespace vihds {
using BB = BlackboxIcml;
#if defined(VIHDS_BB_PART) && VIHDS_BB_PART == 1
int launch_dr_blackbox_split_fwd(int solver, const OdeArgs& a, hipStream_t st, const ThetaStageArgs* ts) {
  return launch_bb_split_dir<BbMfma, false>(solver, a, st, ts);
}
}  // namespace vihds
#ifdef VIHDS_BB_STAMPS
extern "C" int vihds_debug_bb_fwd_stamps(unsigned long long* buf) {
  return (int)hipMemcpyToSymbol(HIP_SYMBOL(vihds::vihds_bb_stamp_buf), &buf, sizeof(buf));
}
#endif
#else
int launch_dr_blackbox_split_fwd(int solver, const OdeArgs& a, hipStream_t st, const ThetaStageArgs* ts);
int launch_dr_blackbox(bool backward, int solver, const OdeArgs& a, hipStream_t st, const LaunchMode& mode) {
  // kernel_variant 1 = VALU, one thread per trajectory (vihds_blackbox.hpp); otherwise the MFMA formulation
  const bool per_thread = a.kernel_variant == 1 || solver_is_adaptive(solver) || mode.grid;
  // (vihds_theta_ode_fwd: the sampling stage exists in the cooperating-wavefront forward only)
  if (mode.theta && (backward || per_thread)) return VIHDS_E_UNSUPPORTED;
  if (per_thread) return launch_ode<BB>(backward, solver, a, st, mode);
  // otherwise the two networks on two wavefronts and the Gram tiles on two more (vihds_blackbox_split.hpp)
  if (!backward) {
    const int rc = launch_dr_blackbox_split_fwd(solver, a, st, mode.theta);
    // (a time grid too long for the cooperating-wavefront forward's staged inputs: the thread-per-trajectory forward)
    return (rc == VIHDS_E_UNSUPPORTED && !mode.theta) ? launch_ode<BB>(false, solver, a, st, mode) : rc;
  }
  return launch_bb_split_dir<BbMfma, true>(solver, a, st);
}
// The ICML sizes as the record every size set has (vihds_bb_variant.hpp): vihds_api.hip resolves a dr_blackbox problem to
// this one or to a side library's, and reads sizes, launcher and aux layout from whichever it got.
static long long bb_builtin_gram_floats(int n) { return (long long)BbMfma::gram_floats(n); }
static const BbVariant kBuiltinVariant = {2, 25, 20, BB::NLAT, BB::N, BB::NSLOT, BB::NF, BB::NTAIL, BB::n_weights,
                                          launch_dr_blackbox, 1, bb_builtin_gram_floats, launch_bb_gram_reduce<BbMfma>};
const BbVariant* bb_builtin_variant() { return &kBuiltinVariant; }
}  // namespace vihds
#endif  // VIHDS_BB_PART
#ifdef VIHDS_BB_STAMPS
extern "C" int vihds_debug_bb_stamps(unsigned long long* buf) {
  return (int)hipMemcpyToSymbol(HIP_SYMBOL(vihds::vihds_bb_stamp_buf), &buf, sizeof(buf));
}
#endif
