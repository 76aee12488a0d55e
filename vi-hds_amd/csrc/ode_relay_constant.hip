// Instantiates the fused forward / adjoint ODE kernels for one model (one translation unit per model so the
// library builds in parallel).  Model definition: vihds_models.hpp.
#include "vihds_lane_family.hpp"

namespace vihds {
int launch_relay_constant(bool backward, int solver, const OdeArgs& a, hipStream_t st, const LaunchMode& mode) {
  return lane_family_launch<RelayConstant, RlRelay, false>(backward, solver, a, st, mode);
}
}  // namespace vihds
