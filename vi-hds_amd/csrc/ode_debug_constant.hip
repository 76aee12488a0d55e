// Instantiates the fused forward / adjoint ODE kernels for one model (one translation unit per model so the
// library builds in parallel).  Model definition: vihds_models.hpp.
#include "vihds_ode_kernels.hpp"

namespace vihds {
int launch_debug_constant(bool backward, int solver, const OdeArgs& a, hipStream_t st, const LaunchMode& mode) {
  return launch_ode<DebugConstant>(backward, solver, a, st, mode);
}
}  // namespace vihds
