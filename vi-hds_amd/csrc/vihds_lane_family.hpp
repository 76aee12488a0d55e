// Launcher of the model families with lane-split kernels (vihds_relay_lanes.hpp): relay / degrader / prpr / auto_constant,
// with constant (PREC false) or neural precisions.
#pragma once
#include <type_traits>

#include "vihds_ode_kernels.hpp"
#include "vihds_relay_lanes.hpp"

namespace vihds {
// Below 16 384 trajectories: one lane per state, sixteen lanes per trajectory (Rl, the family's lane model).  The adaptive
// controller, a hidden layer in the precision network and kernel_variant 1 keep one thread per trajectory, and so does a
// backward that wants the precision network's weight gradients without the small per-block buffer of
// vihds_ode_bwd_aux_floats in `aux`.  The sampling stage (vihds_theta_ode_fwd) exists in the lane-split kernels only.
template <class Core, class Rl, bool PREC>
inline int lane_family_launch(bool backward, int solver, const OdeArgs& a, hipStream_t st, const LaunchMode& mode) {
  if (!mode.grid && relay_lanes_applicable(a.n, solver, a.kernel_variant, a.n_hidden_prec) &&
      !(PREC && backward && a.g_weights && !a.aux))
    return relay_lanes_launch<Rl, PREC>(backward, solver, a, st, mode.theta);
  if (mode.theta) return VIHDS_E_UNSUPPORTED;
  return launch_ode<std::conditional_t<PREC, WithPrec<Core>, Core>>(backward, solver, a, st, mode);
}
}  // namespace vihds
