// One model generated from a Python definition (vihds/modelgen.py; see ../vihds_gen_model.hpp) as a side library, built with
//   -DVIHDS_GEN_HEADER="<generated header>"
// as eleven objects compiled in parallel (Makefile, target `generated`): one per solver (-DVIHDS_ONLY_SOLVER=<id>: the
// kernels of that solver behind vihds_gen_launch_<id>) and the table object (no VIHDS_ONLY_SOLVER: the GenModelRecord
// that dispatches to them).  The generated header defines VIHDS_GEN_CORE (the struct) and VIHDS_GEN_NEURAL (0 / 1).
#include "../vihds_ode_kernels.hpp"
#include "../vihds_gen_model.hpp"

#ifndef VIHDS_GEN_HEADER
#error "define VIHDS_GEN_HEADER (the header vihds/modelgen.py wrote)"
#endif
#include VIHDS_GEN_HEADER

namespace vihds {
template <bool NEURAL>
struct GenSel {
  using type = VIHDS_GEN_CORE;
};
template <>
struct GenSel<true> {
  using type = WithPrec<VIHDS_GEN_CORE>;
};
static_assert(!(VIHDS_GEN_NEURAL != 0 && own_prec<VIHDS_GEN_CORE>::value),
              "a model with a precision map of its own does not take NeuralPrecisions");
static_assert(!(VIHDS_GEN_NEURAL != 0 && own_lik<VIHDS_GEN_CORE>::value),
              "a model with an observation log density of its own does not take NeuralPrecisions");
static_assert(!(VIHDS_GEN_NEURAL != 0 && has_jacobian<VIHDS_GEN_CORE>::value),
              "an implicit model does not take NeuralPrecisions: the precision ODE has no Jacobian");
static_assert(!(substeps<VIHDS_GEN_CORE>::value > 1 && (VIHDS_GEN_NEURAL != 0 || net_fields<VIHDS_GEN_CORE>::value > 0)),
              "a model with sub-steps takes no networks and no NeuralPrecisions: the adjoint's dump holds (T-1) x stages evaluations");
static_assert(substeps<VIHDS_GEN_CORE>::value >= 1 && substeps<VIHDS_GEN_CORE>::value <= kMaxSubsteps,
              "substeps: 1 .. 8 (vihds_substeps.hpp)");
static_assert(!step_control<VIHDS_GEN_CORE>::value ||
                  ((substeps<VIHDS_GEN_CORE>::value == 2 || substeps<VIHDS_GEN_CORE>::value == 4 || substeps<VIHDS_GEN_CORE>::value == 8) &&
                   n_delays<VIHDS_GEN_CORE>::value == 0 && !has_diffusion<VIHDS_GEN_CORE>::value),
              "step control: SUBSTEPS is the ladder's ceiling 2, 4 or 8; no delays and no process noise (vihds_stepctl.hpp)");
static_assert(!(VIHDS_GEN_NEURAL != 0 && has_jump<VIHDS_GEN_CORE>::value),
              "a model with a state jump does not take NeuralPrecisions: WithPrec<> does not forward jump / jump_vjp");
static_assert(!(VIHDS_GEN_NEURAL != 0 && (has_start<VIHDS_GEN_CORE>::value || lead_in<VIHDS_GEN_CORE>::value > 0)),
              "a model with a start map or a lead-in phase does not take NeuralPrecisions: WithPrec<> does not forward them");
static_assert(!(lead_in<VIHDS_GEN_CORE>::value > 0 && net_fields<VIHDS_GEN_CORE>::value > 0),
              "a model with a lead-in phase takes no networks: the adjoint's dump holds (T-1) x stages evaluations");
static_assert(lead_in<VIHDS_GEN_CORE>::value >= 0 && lead_in<VIHDS_GEN_CORE>::value <= kMaxLeadInSteps,
              "lead_in_steps: 1 .. 8 (vihds_substeps.hpp)");
static_assert(!(VIHDS_GEN_NEURAL != 0 && n_delays<VIHDS_GEN_CORE>::value > 0),
              "a model with delayed reads does not take NeuralPrecisions: WithPrec<> forwards neither N_DELAYS nor set_delay");
static_assert(!(n_delays<VIHDS_GEN_CORE>::value > 0 &&
                (has_jacobian<VIHDS_GEN_CORE>::value || substeps<VIHDS_GEN_CORE>::value > 1 || has_jump<VIHDS_GEN_CORE>::value ||
                 lead_in<VIHDS_GEN_CORE>::value > 0 || net_fields<VIHDS_GEN_CORE>::value > 0)),
              "delayed reads combine with the explicit fixed-grid schemes only: no implicit, substeps, jump, lead_in or networks");
static_assert(n_delays<VIHDS_GEN_CORE>::value >= 0 && n_delays<VIHDS_GEN_CORE>::value <= 4, "delays: at most 4");
static_assert(!(has_diffusion<VIHDS_GEN_CORE>::value &&
                (VIHDS_GEN_NEURAL != 0 || has_jacobian<VIHDS_GEN_CORE>::value || net_fields<VIHDS_GEN_CORE>::value > 0 ||
                 lead_in<VIHDS_GEN_CORE>::value > 0 || n_delays<VIHDS_GEN_CORE>::value > 0)),
              "process noise combines with the explicit fixed-grid schemes only: no NeuralPrecisions, implicit, networks, lead_in or delays");
static_assert(noise_channels<VIHDS_GEN_CORE>::value >= 0 && noise_channels<VIHDS_GEN_CORE>::value <= 8 &&
                  (noise_channels<VIHDS_GEN_CORE>::value == 0 || has_diffusion<VIHDS_GEN_CORE>::value),
              "noise channels: at most 8 (two Philox blocks per step), and such a struct declares HAS_DIFFUSION (vihds_sde.hpp)");
static_assert(!(VIHDS_GEN_NEURAL != 0 && has_steady<VIHDS_GEN_CORE>::value > 0),
              "a model with steady species does not take NeuralPrecisions: WithPrec<> does not forward steady / steady_vjp");
static_assert(has_steady<VIHDS_GEN_CORE>::value >= 0 && has_steady<VIHDS_GEN_CORE>::value <= kMaxSteady,
              "steady_species: at most 8 (vihds_steady.hpp)");
using GenM = GenSel<VIHDS_GEN_NEURAL != 0>::type;
typedef int (*gen_launch_fn)(bool, int, const OdeArgs&, hipStream_t, const LaunchMode&);
}  // namespace vihds

#define VIHDS_GEN_CAT2(a, b) a##b
#define VIHDS_GEN_CAT(a, b) VIHDS_GEN_CAT2(a, b)

#ifdef VIHDS_ONLY_SOLVER
extern "C" int VIHDS_GEN_CAT(vihds_gen_launch_, VIHDS_ONLY_SOLVER)(bool backward, int solver, const vihds::OdeArgs& a,
                                                                  hipStream_t st, const vihds::LaunchMode& mode) {
  return vihds::launch_ode<vihds::GenM>(backward, solver, a, st, mode);
}
#else
#define VIHDS_GEN_DECL(k) \
  extern "C" int vihds_gen_launch_##k(bool, int, const vihds::OdeArgs&, hipStream_t, const vihds::LaunchMode&);
VIHDS_GEN_DECL(0) VIHDS_GEN_DECL(1) VIHDS_GEN_DECL(2) VIHDS_GEN_DECL(3) VIHDS_GEN_DECL(4) VIHDS_GEN_DECL(5)
VIHDS_GEN_DECL(6) VIHDS_GEN_DECL(7) VIHDS_GEN_DECL(8) VIHDS_GEN_DECL(9)
// (object 9, the implicit solver: kernels for a model generated with implicit = True, a declining function for any other)
static_assert(VIHDS_SOLVER_COUNT == 10, "one object per solver: extend the table and the Makefile");
namespace vihds {
// (the entry points of vihds_api.hip decline the sampling stage, the one-pass summaries and the device-resident adaptive
// solver for registered models before any launcher is called: of the launch modes only the host-driven controller arrives here)
template <class M>
static int n_weights_of(int H) {
  if constexpr (M::NEURAL_PREC) return VIHDS_GEN_CORE::NW + M::n_weights(H);
  else return VIHDS_GEN_CORE::NW;
}
static int n_weights_gen(int H) { return n_weights_of<GenM>(H); }
static const char* const* slot_names_gen() {
  static const char* n[GenM::NSLOT];
  for (int s = 0; s < GenM::NSLOT; ++s) n[s] = GenM::slot_name(s);
  return n;
}
static int launch_gen(bool backward, int solver, const OdeArgs& a, hipStream_t st, const LaunchMode& mode) {
  static const gen_launch_fn table[VIHDS_SOLVER_COUNT] = {vihds_gen_launch_0, vihds_gen_launch_1, vihds_gen_launch_2,
                                                          vihds_gen_launch_3, vihds_gen_launch_4, vihds_gen_launch_5,
                                                          vihds_gen_launch_6, vihds_gen_launch_7, vihds_gen_launch_8,
                                                          vihds_gen_launch_9};
  if (solver < 0 || solver >= VIHDS_SOLVER_COUNT) return VIHDS_E_BADARG;
  return table[solver](backward, solver, a, st, mode);
}
}  // namespace vihds

extern "C" const vihds::GenModelRecord* vihds_generated_model_v1(void) {
  using namespace vihds;
  static const GenModelRecord r = {VIHDS_ABI_VERSION, (int)sizeof(OdeArgs), VIHDS_HDR_HASH, traj_rows<GenM>::value, GenM::NSLOT, GenM::NC, GenM::OBS, GenM::NEURAL_PREC ? 1 : 0,
                                   slot_names_gen(), n_weights_gen, launch_gen, VIHDS_GEN_CORE::NW,
                                   net_fields<VIHDS_GEN_CORE>::value, own_prec<GenM>::value ? 1 : 0,
                                   n_forcings<GenM>::value, implicit_order<GenM>::value, substeps<GenM>::value,
                                   has_jump<GenM>::value ? 1 : 0, has_start<GenM>::value ? 1 : 0, lead_in<GenM>::value,
                                   n_delays<GenM>::value, has_diffusion<GenM>::value ? 1 : 0,
                                   masked_obs<GenM>::value ? 1 : 0, step_control<GenM>::value ? 1 : 0,
                                   has_steady<GenM>::value};
  return &r;
}
#endif
