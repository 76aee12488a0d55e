// Fused ODE-integration kernels: one thread per (row b, IWAE sample s) trajectory, the whole time loop inside
// the kernel, state and effective parameters in VGPRs, trajectory written [T][N][B][S] so that each store
// instruction of a wave covers 64 consecutive floats.
//
// Forward  = reference OdeModel.simulate (vihds/ode.py:66-82) + observe (:84-93) + expand_precisions
//            (vihds/precisions.py:31-35) + log_prob_observations (vihds/training.py:24-44), fused.
// Backward = discrete adjoint of the chosen scheme, i.e. exactly the gradient autograd produces for the
//            reference's python time loop: for each step (last to first) reload y_k from the stored
//            trajectory, recompute the stage states, and pull the adjoint back through the stages.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <type_traits>
#include <vector>

#include "../../include/vihds_hip.h"
#include "vihds_args.hpp"
#include "vihds_models.hpp"
#include "vihds_rk_adaptive.hpp"
#include "vihds_implicit.hpp"
#include "vihds_delay.hpp"
#include "vihds_substeps.hpp"
#include "vihds_stepctl.hpp"
#include "vihds_sde.hpp"
#include "vihds_mask.hpp"
#include "vihds_blackbox.hpp"
#include "vihds_iwae_inline.hpp"

namespace vihds {

constexpr float LOG2PI_F = 1.8378770664093453f;  // math.log(2*math.pi), vihds/training.py:43


// The fixed observation maps.  (A model with a map of its own, M::OBS == OBS_CUSTOM, is never handed to these: the forward
// and the adjoint kernel call its members, and the kernels that only know the fixed maps are not launched for it.)
template <int OBS>
__device__ __forceinline__ void observe(const float* y, float* xp) {
  static_assert(OBS != OBS_CUSTOM, "a custom observation map is the model's own member observe(y, p, xp)");
  xp[0] = y[0];
  xp[1] = y[0] * y[1];
  if (OBS == OBS_DEFAULT) {  // vihds/ode.py:84-93
    xp[2] = y[0] * (y[2] + y[4]);
    xp[3] = y[0] * (y[3] + y[5]);
  } else if (OBS == OBS_INDUCER) {  // models/inducer_constant.py:106-114: [OD, OD*RFP, OD*(YFP+F530), OD*F480]
    xp[2] = y[0] * (y[2] + y[3]);
    xp[3] = y[0] * y[4];
  } else {  // models/auto_constant.py:89-97, models/dr_blackbox.py:112-121
    xp[2] = y[0] * y[2];
    xp[3] = y[0] * y[3];
  }
}
template <int OBS>
__device__ __forceinline__ void observe_vjp(const float* y, const float* xpb, float* yb) {
  static_assert(OBS != OBS_CUSTOM, "a custom observation map is the model's own member observe_vjp(y, p, xpb, yb, pb)");
  if (OBS == OBS_DEFAULT) {
    yb[0] += xpb[0] + xpb[1] * y[1] + xpb[2] * (y[2] + y[4]) + xpb[3] * (y[3] + y[5]);
    yb[1] += xpb[1] * y[0];
    yb[2] += xpb[2] * y[0];
    yb[4] += xpb[2] * y[0];
    yb[3] += xpb[3] * y[0];
    yb[5] += xpb[3] * y[0];
  } else if (OBS == OBS_INDUCER) {
    yb[0] += xpb[0] + xpb[1] * y[1] + xpb[2] * (y[2] + y[3]) + xpb[3] * y[4];
    yb[1] += xpb[1] * y[0];
    yb[2] += xpb[2] * y[0];
    yb[3] += xpb[2] * y[0];
    yb[4] += xpb[3] * y[0];
  } else {
    yb[0] += xpb[0] + xpb[1] * y[1] + xpb[2] * y[2] + xpb[3] * y[3];
    yb[1] += xpb[1] * y[0];
    yb[2] += xpb[2] * y[0];
    yb[3] += xpb[3] * y[0];
  }
}

// backward context per model kind
struct NoCtx {};
template <int NW>
struct WeightGradCtx {
  static constexpr bool DUMP = false;
  float wb[NW];
};
// white-box + neural precisions with an aux buffer: instead of 2*4*NIN register accumulators per thread (which spill:
// 0.4-0.5 KB of scratch per lane and a third of the adjoint's time for relay_constant_precisions) the adjoint stores,
// per RHS evaluation, the 8 pre-activation adjoints and the NIN layer inputs field-major [8+NIN][E][n]; the weight
// gradients are then two rectangles of vihds_gram_blocks over that dump.  Only the 8 bias sums stay in registers.
struct PrecDumpCtx {
  static constexpr bool DUMP = true;
  float* dump;     // &aux[i]
  size_t n;        // trajectories
  size_t fstride;  // floats between consecutive fields = E * n
  int e;           // evaluation counter
  float bsum[8];
};
// a generated core with networks of its own (net_fields<M> > 0), with constant precisions or inside WithPrec<>: the aux
// buffer holds the networks' fields [NET_FIELDS][E][n] first, then (WithPrec<>) the precision network's [8 + NIN (+ 2 H)][E][n].
// Nothing of the networks stays in registers: their bias gradients are row sums of the dump (vihds/ops.py).
struct GenDumpCtx {
  static constexpr bool DUMP = true;
  float* dump;  // precision section (PrecDumpCtx's members, for WithPrec::rhs_vjp)
  size_t n, fstride;
  int e;
  float bsum[8];
  float* net_dump;  // &aux[i]
  int net_e;
};
// ... without an aux buffer: state / theta adjoints only, no weight gradient of either section (as a hidden precision
// layer without aux; vihds_ode_bwd refuses g_weights without aux for these models)
struct NetSkipCtx {
  static constexpr bool DUMP = false;
};
// RHS evaluations the adjoint of one step dumps, explicit schemes (the dump contexts below ask on the device: a model with
// weights of any kind has no implicit scheme, so their code is what it was)
__host__ __device__ inline int explicit_stages(int solver) {
  if (solver_is_adaptive(solver)) return adaptive_stages(solver);
  return solver == VIHDS_SOLVER_EULER ? 1 : (solver == VIHDS_SOLVER_RK4 ? 4 : 2);
}
// ... of every solver: the adjoint of an implicit step has one vector-Jacobian product, at (t1, y_k+1)
__host__ __device__ inline int ode_stages(int solver) { return solver_is_implicit(solver) ? 1 : explicit_stages(solver); }
template <class M, bool BB = is_blackbox<M>::value, bool HAS_W = (M::NW > 0)>
struct bwd_ctx {  // white-box
  using type = NoCtx;
  __device__ static void init(type&, const OdeArgs&, int) {}
};
template <class M>
struct bwd_ctx<M, false, true> {  // white-box + neural precisions
  using type = WeightGradCtx<M::NW>;
  __device__ static void init(type& c, const OdeArgs&, int) {
    VIHDS_UNROLL for (int q = 0; q < M::NW; ++q) c.wb[q] = 0.f;
  }
};
template <class M>
struct bwd_ctx<M, true, true> {  // dr_blackbox
  using type = BlackboxCtx;
  __device__ static void init(type& c, const OdeArgs& a, int i) {
    c.dump = a.aux + i;
    c.n = (size_t)a.n;
    c.fstride = (size_t)(a.T - 1) * M::stages(a.solver) * a.n;
    c.e = 0;
    VIHDS_UNROLL for (int k = 0; k < 2 * M::NX + 8; ++k) c.bsum[k] = 0.f;
  }
};

template <class M, bool DUMP, bool NET = (net_fields<M>::value > 0)>
struct bwd_ctx_sel {
  using impl = bwd_ctx<M>;
};
template <class M>
struct bwd_ctx_sel<M, false, true> {
  struct impl {
    using type = NetSkipCtx;
    __device__ static void init(type&, const OdeArgs&, int) {}
  };
};
template <class M>
struct bwd_ctx_sel<M, true, true> {
  struct impl {
    using type = GenDumpCtx;
    __device__ static void init(type& c, const OdeArgs& a, int i) {
      c.n = (size_t)a.n;
      c.fstride = (size_t)(a.T - 1) * explicit_stages(a.solver) * a.n;
      c.net_dump = a.aux + i;
      c.dump = a.aux + (size_t)net_fields<M>::value * c.fstride + i;
      c.e = 0;
      c.net_e = 0;
      VIHDS_UNROLL for (int k = 0; k < 8; ++k) c.bsum[k] = 0.f;
    }
  };
};
template <class M>
struct bwd_ctx_sel<M, true, false> {
  struct impl {
    using type = PrecDumpCtx;
    __device__ static void init(type& c, const OdeArgs& a, int i) {
      c.dump = a.aux + i;
      c.n = (size_t)a.n;
      c.fstride = (size_t)(a.T - 1) * explicit_stages(a.solver) * a.n;
      c.e = 0;
      VIHDS_UNROLL for (int k = 0; k < 8; ++k) c.bsum[k] = 0.f;
    }
  };
};

// ---- one step of each scheme ---------------------------------------------------------------------
template <class M, int SOLVER>
__device__ __forceinline__ void ode_step(float t0, float t1, float h0, float* y, const float* p, const float* wts) {
  constexpr int N = M::N;
  if constexpr (solver_is_implicit(SOLVER)) {  // backward Euler by M::NEWTON Newton iterations from y (vihds_implicit.hpp)
    static_assert(has_jacobian<M>::value, "an implicit solver needs a model generated with implicit = True");
    if constexpr (implicit_order<M>::value == 2) {  // ... or the model's two-stage SDIRK, M::NEWTON iterations per stage
      sdirk2_step<N, M::NEWTON, M::JAC_NZ>(
          t0, t1, y, [&](float t, const float* z, float* fz) { M::rhs(t, z, p, wts, fz); },
          [&](float t, const float* z, float* J) { M::rhs_jac(t, z, p, wts, J); });
      return;
    }
    beuler_step<N, M::NEWTON, M::JAC_NZ>(
        t1 - t0, y, [&](const float* z, float* fz) { M::rhs(t1, z, p, wts, fz); },
        [&](const float* z, float* J) { M::rhs_jac(t1, z, p, wts, J); });
    return;
  }
  if constexpr (solver_is_adaptive(SOLVER)) {  // the accepted grid of an adaptive pair, its higher-order tableau
    rk_step_generic<M, Tableau<SOLVER>>(t0, t1 - t0, y, p, wts, nullptr);
    return;
  }
  float k1[N], k2[N], ya[N];
  if (SOLVER == VIHDS_SOLVER_MODEULER || SOLVER == VIHDS_SOLVER_MODEULERWHILE) {
    // vihds/solvers.py:12-16 / :21-25
    const float h = (SOLVER == VIHDS_SOLVER_MODEULER) ? h0 : (t1 - t0);
    M::rhs(t0, y, p, wts, k1);
    VIHDS_UNROLL for (int j = 0; j < N; ++j) ya[j] = y[j] + h * k1[j];
    M::rhs(t1, ya, p, wts, k2);
    const float hh = 0.5f * h;
    VIHDS_UNROLL for (int j = 0; j < N; ++j) y[j] = y[j] + hh * (k1[j] + k2[j]);
  } else if (SOLVER == VIHDS_SOLVER_EULER) {
    const float dt = t1 - t0;
    M::rhs(t0, y, p, wts, k1);
    VIHDS_UNROLL for (int j = 0; j < N; ++j) y[j] = y[j] + dt * k1[j];
  } else if (SOLVER == VIHDS_SOLVER_MIDPOINT) {
    // torchdiffeq 0.1 Midpoint.step_func: y_mid = y + f(t,y)*dt/2 ; dy = dt*f(t+dt/2, y_mid)
    const float dt = t1 - t0;
    M::rhs(t0, y, p, wts, k1);
    VIHDS_UNROLL for (int j = 0; j < N; ++j) ya[j] = y[j] + k1[j] * dt * 0.5f;
    M::rhs(t0 + dt * 0.5f, ya, p, wts, k2);
    VIHDS_UNROLL for (int j = 0; j < N; ++j) y[j] = y[j] + dt * k2[j];
  } else {
    // torchdiffeq 0.1 rk4_alt_step_func (3/8 rule)
    const float dt = t1 - t0;
    const float d3 = dt * (1.f / 3.f);  // the per-element k/3 of torchdiffeq become multiplies (1-ulp difference)
    float k3[N], k4[N];
    M::rhs(t0, y, p, wts, k1);
    VIHDS_UNROLL for (int j = 0; j < N; ++j) ya[j] = y[j] + d3 * k1[j];
    M::rhs(t0 + d3, ya, p, wts, k2);
    VIHDS_UNROLL for (int j = 0; j < N; ++j) ya[j] = y[j] + (dt * k2[j] - d3 * k1[j]);
    M::rhs(t0 + 2.f * d3, ya, p, wts, k3);
    VIHDS_UNROLL for (int j = 0; j < N; ++j) ya[j] = y[j] + dt * (k1[j] - k2[j] + k3[j]);
    M::rhs(t0 + dt, ya, p, wts, k4);
    const float d8 = dt * 0.125f;
    VIHDS_UNROLL for (int j = 0; j < N; ++j) y[j] = y[j] + (k1[j] + 3.f * k2[j] + 3.f * k3[j] + k4[j]) * d8;
  }
}

template <class M, class Ctx>
__device__ __forceinline__ void call_vjp(float t, const float* y, const float* p, const float* w, const float* v,
                                         float* yb, float* pb, Ctx& ctx) {
  if constexpr (std::is_same<Ctx, NoCtx>::value) M::rhs_vjp(t, y, p, w, v, yb, pb);
  else M::rhs_vjp(t, y, p, w, v, yb, pb, ctx);
}

// reverse of one step: lam (adjoint of y_{k+1}) -> adjoint of y_k ; pb += parameter adjoint
template <class M, int SOLVER, class Ctx>
__device__ __forceinline__ void ode_step_vjp(float t0, float t1, float h0, const float* y, const float* p,
                                             const float* wts, float* lam, float* pb, Ctx& wtsb) {
  constexpr int N = M::N;
  if constexpr (solver_is_adaptive(SOLVER)) {
    rk_step_generic_vjp<M, Tableau<SOLVER>>(t0, t1 - t0, y, p, wts, lam, [&](float t, const float* ys, const float* v,
                                                                             float* yb) {
      call_vjp<M>(t, ys, p, wts, v, yb, pb, wtsb);
    });
    return;
  }
  float k1[N], ya[N], v[N], w[N];
  if (SOLVER == VIHDS_SOLVER_MODEULER || SOLVER == VIHDS_SOLVER_MODEULERWHILE) {
    const float h = (SOLVER == VIHDS_SOLVER_MODEULER) ? h0 : (t1 - t0);
    const float hh = 0.5f * h;
    M::rhs(t0, y, p, wts, k1);
    VIHDS_UNROLL for (int j = 0; j < N; ++j) ya[j] = y[j] + h * k1[j];
    // y' = y + hh*(f1 + f2)
    VIHDS_UNROLL for (int j = 0; j < N; ++j) { v[j] = hh * lam[j]; w[j] = 0.f; }
    call_vjp<M>(t1, ya, p, wts, v, w, pb, wtsb);  // w = ya_bar
    VIHDS_UNROLL for (int j = 0; j < N; ++j) { lam[j] += w[j]; v[j] += h * w[j]; }
    call_vjp<M>(t0, y, p, wts, v, lam, pb, wtsb);
  } else if (SOLVER == VIHDS_SOLVER_EULER) {
    const float dt = t1 - t0;
    VIHDS_UNROLL for (int j = 0; j < N; ++j) v[j] = dt * lam[j];
    call_vjp<M>(t0, y, p, wts, v, lam, pb, wtsb);
  } else if (SOLVER == VIHDS_SOLVER_MIDPOINT) {
    const float dt = t1 - t0;
    M::rhs(t0, y, p, wts, k1);
    VIHDS_UNROLL for (int j = 0; j < N; ++j) ya[j] = y[j] + k1[j] * dt * 0.5f;
    VIHDS_UNROLL for (int j = 0; j < N; ++j) { v[j] = dt * lam[j]; w[j] = 0.f; }
    call_vjp<M>(t0 + dt * 0.5f, ya, p, wts, v, w, pb, wtsb);  // w = ymid_bar
    VIHDS_UNROLL for (int j = 0; j < N; ++j) { lam[j] += w[j]; v[j] = 0.5f * dt * w[j]; }
    call_vjp<M>(t0, y, p, wts, v, lam, pb, wtsb);
  } else {
    const float dt = t1 - t0;
    const float d3 = dt * (1.f / 3.f);
    float k2[N], k3[N], y2[N], y3[N];
    M::rhs(t0, y, p, wts, k1);
    VIHDS_UNROLL for (int j = 0; j < N; ++j) y2[j] = y[j] + d3 * k1[j];
    M::rhs(t0 + d3, y2, p, wts, k2);
    VIHDS_UNROLL for (int j = 0; j < N; ++j) y3[j] = y[j] + (dt * k2[j] - d3 * k1[j]);
    M::rhs(t0 + 2.f * d3, y3, p, wts, k3);
    VIHDS_UNROLL for (int j = 0; j < N; ++j) ya[j] = y[j] + dt * (k1[j] - k2[j] + k3[j]);  // y4
    const float d8 = dt * 0.125f;
    float k1b[N], k2b[N], k3b[N];
    VIHDS_UNROLL for (int j = 0; j < N; ++j) {
      v[j] = d8 * lam[j];  // k4_bar
      k1b[j] = v[j];
      k2b[j] = 3.f * v[j];
      k3b[j] = 3.f * v[j];
      w[j] = 0.f;
    }
    call_vjp<M>(t0 + dt, ya, p, wts, v, w, pb, wtsb);  // w = y4_bar
    VIHDS_UNROLL for (int j = 0; j < N; ++j) {
      lam[j] += w[j];
      k1b[j] += dt * w[j];
      k2b[j] -= dt * w[j];
      k3b[j] += dt * w[j];
      w[j] = 0.f;
    }
    call_vjp<M>(t0 + 2.f * d3, y3, p, wts, k3b, w, pb, wtsb);  // w = y3_bar
    VIHDS_UNROLL for (int j = 0; j < N; ++j) {
      lam[j] += w[j];
      k1b[j] -= d3 * w[j];
      k2b[j] += dt * w[j];
      w[j] = 0.f;
    }
    call_vjp<M>(t0 + d3, y2, p, wts, k2b, w, pb, wtsb);  // w = y2_bar
    VIHDS_UNROLL for (int j = 0; j < N; ++j) {
      lam[j] += w[j];
      k1b[j] += d3 * w[j];
    }
    call_vjp<M>(t0, y, p, wts, k1b, lam, pb, wtsb);
  }
}

// reverse of one implicit step, at the stored y_next = y_k+1 (no Newton iteration runs here): lam <- A^-T lam with
// A = I - h J(t1, y_next), then pb += (h lam)^T df/dp by one rhs_vjp whose state output is discarded
template <class M, class Ctx>
__device__ __forceinline__ void ode_step_vjp_implicit(float t0, float t1, const float* y_next, const float* p,
                                                      const float* wts, float* lam, float* pb, Ctx& wtsb) {
  constexpr int N = M::N;
  static_assert(has_jacobian<M>::value, "an implicit solver needs a model generated with implicit = True");
  const float h = t1 - t0;
  beuler_step_vjp<N, M::JAC_NZ>(h, y_next, lam, [&](const float* z, float* J) { M::rhs_jac(t1, z, p, wts, J); });
  float v[N], unused[N];
  VIHDS_UNROLL for (int j = 0; j < N; ++j) { v[j] = h * lam[j]; unused[j] = 0.f; }
  call_vjp<M>(t1, y_next, p, wts, v, unused, pb, wtsb);
}

// reverse of one step of the two-stage SDIRK (implicit_order<M> = 2), from the step's start state y = y_k and the stored
// y_next = y_k+1: the stage value z1 is recomputed by the forward's stage-1 call into registers (no Newton iteration runs on the
// adjoint itself), lam <- (1 - c) mu2 + mu1, then pb += (a mu2)^T df/dp at (t1, y_next) + (a mu1)^T df/dp at (tg, z1) by two
// rhs_vjp calls whose state output is discarded.  Instantiated for such a model only.
template <class M, class Ctx>
__device__ __forceinline__ void ode_step_vjp_sdirk2(float t0, float t1, const float* y, const float* y_next, const float* p,
                                                    const float* wts, float* lam, float* pb, Ctx& wtsb) {
  constexpr int N = M::N;
  static_assert(implicit_order<M>::value == 2, "the two-stage scheme needs a model generated with implicit_order = 2");
  const float h = t1 - t0;
  const float a = kSdirk2Gamma * h;
  const float tg = __builtin_fmaf(kSdirk2Gamma, h, t0);
  float z1[N], mu1[N], mu2[N], unused[N];
  sdirk2_step_vjp<N, M::NEWTON, M::JAC_NZ>(
      t0, t1, y, y_next, lam, z1, mu1, mu2, [&](float t, const float* z, float* fz) { M::rhs(t, z, p, wts, fz); },
      [&](float t, const float* z, float* J) { M::rhs_jac(t, z, p, wts, J); });
  VIHDS_UNROLL for (int j = 0; j < N; ++j) { mu2[j] = a * mu2[j]; unused[j] = 0.f; }
  call_vjp<M>(t1, y_next, p, wts, mu2, unused, pb, wtsb);
  VIHDS_UNROLL for (int j = 0; j < N; ++j) { mu1[j] = a * mu1[j]; unused[j] = 0.f; }
  call_vjp<M>(tg, z1, p, wts, mu1, unused, pb, wtsb);
}
// ... of one step of the model's implicit scheme, whichever it is: y (the step's start state) is read by the two-stage scheme
// only (backward Euler's adjoint needs no start state: a caller may pass nullptr for such a model)
template <class M, class Ctx>
__device__ __forceinline__ void ode_step_vjp_implicit_any(float t0, float t1, const float* y, const float* y_next,
                                                          const float* p, const float* wts, float* lam, float* pb, Ctx& wtsb) {
  if constexpr (implicit_order<M>::value == 2) ode_step_vjp_sdirk2<M>(t0, t1, y, y_next, p, wts, lam, pb, wtsb);
  else ode_step_vjp_implicit<M>(t0, t1, y_next, p, wts, lam, pb, wtsb);
}

// ---- sub-steps per observation interval (substeps<M> = MS > 1, vihds_substeps.hpp) -----------------------------------
// Everything below is instantiated for a generated model with `substeps` above 1 only: the time loops reach it behind
// `if constexpr (substeps<M>::value > 1)`, so every other model's kernels are what they were.

// the forward's interval: MS steps of the scheme, a rolled loop (the code does not grow with MS)
// (k, key: the interval's index and the thread's noise stream, read by a model with process noise only -- vihds_sde.hpp)
template <class M, int SOLVER>
__device__ __forceinline__ void ode_substeps(float t0, float t1, float h0, float* y, const float* p, const float* wts,
                                             int k = 0, const SdeKey& key = SdeKey{}) {
  constexpr int MS = substeps<M>::value;
  const SubGrid<MS> sg(t0, t1);
  const float hm = SubGrid<MS>::fixed_step(h0);
#pragma unroll 1
  for (int j = 0; j < MS; ++j) {
    if constexpr (has_diffusion<M>::value) noisy_step<M, SOLVER>(sg.at(j), sg.at(j + 1), hm, sde_step_index(k, MS, j), key, y, p, wts);
    else ode_step<M, SOLVER>(sg.at(j), sg.at(j + 1), hm, y, p, wts);
  }
}

// Where the adjoint keeps an interval's intermediate states u_1 .. u_MS-1: ROWS = (MS - 1) * N rows of 256 floats in LDS.
// Thread t reads and writes column t alone: no barrier, and the lanes of a wavefront touch consecutive banks.  Declared by
// the kernels that call column() only (a launcher of any other model asks for no shared memory of this kind).
template <int ROWS>
struct SubstateLds {
  static_assert(ROWS >= 1 && ROWS * 256 * sizeof(float) < 64 * 1024, "(substeps - 1) * N rows of 256 floats: under 64 KB");
  __device__ static __forceinline__ float* column() {
    __shared__ float rows[ROWS * 256];
    return rows + threadIdx.x;
  }
};
// the rows a model's adjoint asks for: the sub-states of an interval and those of the lead-in phase (lead_in<M>, below) are
// never live at once, so they share one block of max(substeps - 1, lead-in steps - 1) * N rows
template <class M>
constexpr int substate_rows() {
  constexpr int ms = substeps<M>::value - 1, nl = lead_in<M>::value - 1;
  return (ms > nl ? ms : nl) * M::N;
}

// reverse of one observation interval of MS sub-steps.  y is the stored y_k = u_0; y_next the stored y_k+1 = u_MS (read by an
// implicit scheme only).  The intermediate states are stored nowhere: MS - 1 forward sub-steps from u_0 recompute them --
// ode_step with SubGrid's times, exactly the forward's calls -- into LDS, then the step adjoints run for j = MS-1 down to 0.
// An explicit scheme's adjoint starts from u_j, the implicit one's from u_j+1.  Both loops stay rolled.
// (sg, MS: the interval's sub-grid and its step count -- SubGrid<substeps<M>> and that constant, or, for a model with step
// control, SubGridN and the count its forward chose, at most substeps<M>: the rows of SubstateLds are sized by that ceiling)
template <class M, int SOLVER, class Grid, class Ctx>
__device__ __forceinline__ void ode_substeps_vjp_on(const Grid& sg, const int MS, float hm, const float* y, const float* y_next,
                                                    const float* p, const float* wts, float* lam, float* pb, Ctx& wtsb,
                                                    int k, const SdeKey& key) {
  constexpr int N = M::N;
  float* col = SubstateLds<substate_rows<M>()>::column();
  float u[N];
  VIHDS_UNROLL for (int q = 0; q < N; ++q) u[q] = y[q];
#pragma unroll 1
  for (int j = 0; j < MS - 1; ++j) {  // u_j -> u_j+1, kept as row block j
    // (a model with process noise: the forward's noisy step with the forward's step index, so the forward's draws and bits)
    if constexpr (has_diffusion<M>::value) noisy_step<M, SOLVER>(sg.at(j), sg.at(j + 1), hm, sde_step_index(k, MS, j), key, u, p, wts);
    else ode_step<M, SOLVER>(sg.at(j), sg.at(j + 1), hm, u, p, wts);
    VIHDS_UNROLL for (int q = 0; q < N; ++q) col[(j * N + q) * 256] = u[q];
  }
  if constexpr (solver_is_implicit(SOLVER)) {
    VIHDS_UNROLL for (int q = 0; q < N; ++q) u[q] = y_next[q];  // u_MS
#pragma unroll 1
    for (int j = MS - 1; j >= 0; --j) {
      if constexpr (implicit_order<M>::value == 2) {  // (the two-stage scheme's adjoint also reads the sub-step's start u_j)
        float us[N];
        if (j > 0) {
          VIHDS_UNROLL for (int q = 0; q < N; ++q) us[q] = col[((j - 1) * N + q) * 256];
        } else {
          VIHDS_UNROLL for (int q = 0; q < N; ++q) us[q] = y[q];
        }
        ode_step_vjp_sdirk2<M>(sg.at(j), sg.at(j + 1), us, u, p, wts, lam, pb, wtsb);
        VIHDS_UNROLL for (int q = 0; q < N; ++q) u[q] = us[q];
      } else {
        ode_step_vjp_implicit<M>(sg.at(j), sg.at(j + 1), u, p, wts, lam, pb, wtsb);
        if (j > 0) {  // u_j for the sub-step below
          VIHDS_UNROLL for (int q = 0; q < N; ++q) u[q] = col[((j - 1) * N + q) * 256];
        }
      }
    }
  } else {  // (u holds u_MS-1)
#pragma unroll 1
    for (int j = MS - 1; j >= 0; --j) {
      if constexpr (has_diffusion<M>::value)
        noisy_step_vjp<M, SOLVER>(sg.at(j), sg.at(j + 1), hm, sde_step_index(k, MS, j), key, u, p, wts, lam, pb, wtsb);
      else ode_step_vjp<M, SOLVER>(sg.at(j), sg.at(j + 1), hm, u, p, wts, lam, pb, wtsb);
      if (j > 1) {  // u_j-1 for the sub-step below
        VIHDS_UNROLL for (int q = 0; q < N; ++q) u[q] = col[((j - 2) * N + q) * 256];
      } else {
        VIHDS_UNROLL for (int q = 0; q < N; ++q) u[q] = y[q];
      }
    }
  }
}
template <class M, int SOLVER, class Ctx>
__device__ __forceinline__ void ode_substeps_vjp(float t0, float t1, float h0, const float* y, const float* y_next,
                                                 const float* p, const float* wts, float* lam, float* pb, Ctx& wtsb,
                                                 int k = 0, const SdeKey& key = SdeKey{}) {
  constexpr int MS = substeps<M>::value;
  ode_substeps_vjp_on<M, SOLVER>(SubGrid<MS>(t0, t1), MS, SubGrid<MS>::fixed_step(h0), y, y_next, p, wts, lam, pb, wtsb, k, key);
}

// ---- error-controlled sub-steps (step_control<M>, vihds_stepctl.hpp) ---------------------------------------------------
// Instantiated for a generated model with `step_tolerance` only: the time loops reach it behind
// `if constexpr (step_control<M>::value)`.  substeps<M> = MS is the ceiling of the ladder.

// the forward's interval: Phi^1, Phi^2, Phi^4 .. from y = y_k until the acceptance test passes or the count reaches MS; y
// becomes the accepted state and the row's code is returned.  y_k, coarse and fine stay in registers; one rolled loop holds the
// one inlined step of the scheme, so the code does not grow with MS.  (The solvers in scope do not read modeuler's fixed step.)
template <class M, int SOLVER>
__device__ __forceinline__ float ode_stepctl(float t0, float t1, float* y, const float* p, const float* wts) {
  constexpr int N = M::N, MS = substeps<M>::value;
  static_assert(MS == 2 || MS == 4 || MS == 8, "step control: the ceiling of the ladder is 2, 4 or 8");
  float coarse[N], fine[N];
  float code = 0.f;
#pragma unroll 1
  for (int c = 1;; c *= 2) {  // c = 1: coarse = Phi^1(y_k), no test
    const SubGridN sg(t0, t1, c);
    VIHDS_UNROLL for (int q = 0; q < N; ++q) fine[q] = y[q];
#pragma unroll 1
    for (int j = 0; j < c; ++j) ode_step<M, SOLVER>(sg.at(j), sg.at(j + 1), 0.f, fine, p, wts);
    if (c > 1) {
      const bool passed = step_ratio<N>(fine, coarse, M::STEP_RTOL, M::STEP_ATOL) <= 1.f;
      if (passed || c == MS) {
        code = step_code(c, passed);
        break;
      }
    }
    VIHDS_UNROLL for (int q = 0; q < N; ++q) coarse[q] = fine[q];
  }
  VIHDS_UNROLL for (int q = 0; q < N; ++q) y[q] = fine[q];
  return code;
}
// reverse of such an interval: the existing interval adjoint with the count the forward stored (code: the row's float at the
// interval's end point, clamped into 1 .. MS before it bounds a loop or indexes LDS).  The ladder is not repeated
template <class M, int SOLVER, class Ctx>
__device__ __forceinline__ void ode_stepctl_vjp(float t0, float t1, float code, const float* y, const float* y_next,
                                                const float* p, const float* wts, float* lam, float* pb, Ctx& wtsb) {
  const int cnt = step_count_of(code, substeps<M>::value);
  ode_substeps_vjp_on<M, SOLVER>(SubGridN(t0, t1, cnt), cnt, 0.f, y, y_next, p, wts, lam, pb, wtsb, 0, SdeKey{});
}

// ---- the lead-in phase (lead_in<M> = NL > 0: LEAD_STEPS steps over LEAD_TIME before the first observation point) -------
// Instantiated for a generated model with `lead_in` only (behind `if constexpr (lead_in<M>::value > 0)`).  The grid is
// SubGrid<NL>(t_0 - L, t_0): s_j = fmaf(j, hl, tl), s_NL = t_0 exactly; modeuler's fixed step is hl there; sub-steps do not
// divide these steps and no jump is applied.  The caller has put the first forcing samples in place with slope 0
// (set_interval(p, tl, 0, u_0, u_0)).  Nothing is stored: y goes from y_start to y_0.
template <class M, int SOLVER>
__device__ __forceinline__ void ode_lead_in(float t_first, float* y, const float* p, const float* wts) {
  constexpr int NL = lead_in<M>::value;
  const SubGrid<NL> sg(t_first - M::LEAD_TIME, t_first);
#pragma unroll 1
  for (int j = 0; j < NL; ++j) ode_step<M, SOLVER>(sg.at(j), sg.at(j + 1), sg.hs, y, p, wts);
}

// reverse of the lead-in phase: lam (the adjoint of y_0 = u_NL) -> the adjoint of y_start = u_0; pb += the parameter part.
// u_1 .. u_NL-1 are recomputed from y_start with exactly the forward's calls into LDS (the rows of SubstateLds, which no
// interval's sub-states occupy any more), then the step adjoints run last to first; an implicit step's at u_j+1, with
// u_NL = y_first, the stored y_0 (read by an implicit scheme only).  NL = 1 keeps nothing and declares no LDS.
template <class M, int SOLVER, class Ctx>
__device__ __forceinline__ void ode_lead_in_vjp(float t_first, const float* y_start, const float* y_first, const float* p,
                                                const float* wts, float* lam, float* pb, Ctx& wtsb) {
  constexpr int N = M::N, NL = lead_in<M>::value;
  const SubGrid<NL> sg(t_first - M::LEAD_TIME, t_first);
  float u[N];
  VIHDS_UNROLL for (int q = 0; q < N; ++q) u[q] = y_start[q];
  if constexpr (NL > 1) {
    float* col = SubstateLds<substate_rows<M>()>::column();
#pragma unroll 1
    for (int j = 0; j < NL - 1; ++j) {  // u_j -> u_j+1, kept as row block j
      ode_step<M, SOLVER>(sg.at(j), sg.at(j + 1), sg.hs, u, p, wts);
      VIHDS_UNROLL for (int q = 0; q < N; ++q) col[(j * N + q) * 256] = u[q];
    }
    if constexpr (solver_is_implicit(SOLVER)) {
      VIHDS_UNROLL for (int q = 0; q < N; ++q) u[q] = y_first[q];  // u_NL
#pragma unroll 1
      for (int j = NL - 1; j >= 0; --j) {
        if constexpr (implicit_order<M>::value == 2) {  // (the two-stage scheme's adjoint also reads the step's start u_j)
          float us[N];
          if (j > 0) {
            VIHDS_UNROLL for (int q = 0; q < N; ++q) us[q] = col[((j - 1) * N + q) * 256];
          } else {
            VIHDS_UNROLL for (int q = 0; q < N; ++q) us[q] = y_start[q];
          }
          ode_step_vjp_sdirk2<M>(sg.at(j), sg.at(j + 1), us, u, p, wts, lam, pb, wtsb);
          VIHDS_UNROLL for (int q = 0; q < N; ++q) u[q] = us[q];
        } else {
          ode_step_vjp_implicit<M>(sg.at(j), sg.at(j + 1), u, p, wts, lam, pb, wtsb);
          if (j > 0) {  // u_j for the step below
            VIHDS_UNROLL for (int q = 0; q < N; ++q) u[q] = col[((j - 1) * N + q) * 256];
          }
        }
      }
    } else {  // (u holds u_NL-1)
#pragma unroll 1
      for (int j = NL - 1; j >= 0; --j) {
        ode_step_vjp<M, SOLVER>(sg.at(j), sg.at(j + 1), sg.hs, u, p, wts, lam, pb, wtsb);
        if (j > 1) {  // u_j-1 for the step below
          VIHDS_UNROLL for (int q = 0; q < N; ++q) u[q] = col[((j - 2) * N + q) * 256];
        } else {
          VIHDS_UNROLL for (int q = 0; q < N; ++q) u[q] = y_start[q];
        }
      }
    }
  } else if constexpr (solver_is_implicit(SOLVER)) {
    ode_step_vjp_implicit_any<M>(sg.at(0), sg.at(1), u, y_first, p, wts, lam, pb, wtsb);
  } else {
    ode_step_vjp<M, SOLVER>(sg.at(0), sg.at(1), sg.hs, u, p, wts, lam, pb, wtsb);
  }
}

template <class M>
__device__ __forceinline__ void load_theta(const OdeArgs& a, int i, int b, float* th, float* prec, float* c) {
  VIHDS_UNROLL for (int q = 0; q < M::NSLOT; ++q) th[q] = a.theta[(size_t)a.slot_row[q] * a.n + i];
  if constexpr (!own_prec<M>::value) {  // (a precision map of the model's own has no precision slot rows: prec stays unset)
    if (!M::NEURAL_PREC) {  // constant precisions: four more theta rows (reference precisions.py:31-35)
      VIHDS_UNROLL for (int j = 0; j < 4; ++j) prec[j] = a.theta[(size_t)a.slot_row[M::NSLOT + j] * a.n + i];
    }
  }
  VIHDS_UNROLL for (int q = 0; q < M::NC; ++q) c[q] = clampf(expf(a.cond[b * a.C + q]) - 1.f, 1e-12f, 1e6f);
}

// Shared neural weights: dr_blackbox stages them in LDS once per block (every lane reads the same address:
// broadcast); the white-box models with neural precisions read them as scalars straight from the caller's buffer
// (WithPrec::weights_ptr).
template <class M>
__device__ __forceinline__ const float* stage_weights(const OdeArgs& a, float* lds) {
  if constexpr (M::NW == 0) {
    return nullptr;
  } else if constexpr (is_blackbox<M>::value) {
    M::stage(a, lds);
    __syncthreads();
    return lds;
  } else {
    return a.weights;
  }
}

#ifndef VIHDS_NT_TRAJ
#define VIHDS_NT_TRAJ 1
#endif
// What the time loops keep for a model with forcings (n_forcings<M> = NF > 0, vihds_models.hpp): where the thread's data row
// has its samples -- cond[b * C + (C - NF T) + j * T + k], or the block's staged copy -- and the samples at the two ends of
// the current interval and at the point requested one iteration ahead.  Empty for every other model: their kernels declare
// nothing and every use sits behind `if constexpr (NF > 0)`.
template <int NF>
struct ForcingFeed {
  const float* src;  // the row's samples in cond (the unstaged forward, the adjoint)
  int lds;           // ... in in_lds (the staged forward)
  float lo[NF], hi[NF], ahead[NF];
};
template <>
struct ForcingFeed<0> {};
// what the adjoint's time loop keeps for an implicit solver beside its forcing feed: the state of the previous iteration,
// y_k+1 (N registers).  An explicit solver's loop declares the feed alone, as it did (bwd_feed_t), so its code is what it was.
template <class Feed, int N>
struct WithNextState : Feed {
  float y_next[N];
};
template <int NF, int N, bool IMPLICIT>
using bwd_feed_t = std::conditional_t<IMPLICIT, WithNextState<ForcingFeed<NF>, N>, ForcingFeed<NF>>;
// what the time loops keep for a model with delayed reads (n_delays<M> = ND > 0, vihds_delay.hpp) beside their feed: per read
// the stored state of its species at t_0 (the constant history) and the search cursor, the index of s_lo's interval, which
// climbs in the forward and descends in the adjoint.  Every other model's loop declares the feed alone, as it did
// (delay_feed_t), so its code is what it was.
template <class Feed, int ND>
struct WithDelayState : Feed {
  float y0[ND];
  int cur[ND];
};
template <class Feed, int ND>
using delay_feed_t = std::conditional_t<(ND > 0), WithDelayState<Feed, ND>, Feed>;
// what the time loops keep for a model with process noise (has_diffusion<M>, vihds_sde.hpp) beside their feed: the row's key and
// the trajectory's index, loaded once ahead of the loop.  Every other model's loop declares the feed alone, as it did
// (noise_feed_t), so its code is what it was.
template <class Feed>
struct WithNoiseKey : Feed {
  SdeKey key;
};
template <class Feed, bool ON>
using noise_feed_t = std::conditional_t<ON, WithNoiseKey<Feed>, Feed>;
// what the time loops keep for a model with missing observations (masked_obs<M>, vihds_mask.hpp) beside their feed: where the
// thread's data row has its mask words -- cond[b * C + (C - cond_tail - T) + k], or the block's staged copy -- and the word
// requested one iteration ahead, as the observations are.  Every other model's loop declares the feed alone, as it did
// (mask_feed_t), so its code is what it was.
template <class Feed>
struct WithObsMask : Feed {
  const float* msrc;  // the row's mask words in cond (the unstaged forward, the adjoint)
  int mlds;           // ... in in_lds (the staged forward)
  float word, word_ahead;
};
template <class Feed, bool ON>
using mask_feed_t = std::conditional_t<ON, WithObsMask<Feed>, Feed>;
// what the time loops keep for a model with step control (step_control<M>, vihds_stepctl.hpp) beside their feed: the float of
// the count row -- in the forward the code of the interval that just ended, in the adjoint the code of the interval above the
// point k and the one requested one iteration ahead, as the stored states are.  Every other model's loop declares the feed
// alone, as it did (ctl_feed_t), so its code is what it was.
template <class Feed>
struct WithStepCode : Feed {
  float code, code_ahead;
};
template <class Feed, bool ON>
using ctl_feed_t = std::conditional_t<ON, WithStepCode<Feed>, Feed>;
// ---- forward -------------------------------------------------------------------------------------
// LDS_IN: the time grid and the observation rows of the data rows this block spans are staged in LDS once, so the
// time loop holds no vector-memory loads and its trajectory / x_predict stores are never waited on (see
// vihds_dr_lanes.hpp: with a global load in the loop every s_waitcnt vmcnt(0) for it also waits for the stores).
template <class M, int SOLVER, bool LDS_IN>
__global__ void __launch_bounds__(256) ode_fwd_kernel(OdeArgs a) {
  constexpr int N = M::N;
  constexpr int NT = traj_rows<M>::value;  // rows per time point of traj: N, + 4 precision rows of a model with its own map
  constexpr bool OWN_PREC = own_prec<M>::value;
  constexpr bool OWN_LIK = own_lik<M>::value;  // the log density is the model's own member (vihds_models.hpp)
  constexpr int NF = n_forcings<M>::value;     // forcings: K series of T samples per data row behind its treatments in cond
  constexpr int ND = n_delays<M>::value;       // delayed reads: looked up in the rows of traj this thread stored earlier
  constexpr bool MASKED = masked_obs<M>::value;  // missing observations: one mask word per time point in the row of cond
  __shared__ float wlds[M::NW > 0 ? M::NW : 1];
  extern __shared__ float in_lds[];  // [T] times | [nb][4][T] observations | [nb][NF][T] forcing samples | [nb][T] mask words
  const float* wts = stage_weights<M>(a, wlds);
  int ob_off = 0;
  // (ForcingFeed<NF>; a model with delayed reads also keeps y_0 and its cursors, one with process noise its key, one with
  // missing observations its mask words, one with step control the code of the interval that just ended)
  ctl_feed_t<mask_feed_t<noise_feed_t<delay_feed_t<ForcingFeed<NF>, ND>, has_diffusion<M>::value>, MASKED>, step_control<M>::value> ff;
  if constexpr (step_control<M>::value) ff.code = 0.f;
  if (LDS_IN) {
    const int first = blockIdx.x * blockDim.x, last = min(first + (int)blockDim.x, a.n) - 1;
    const int b0 = first / a.S, nb = last / a.S - b0 + 1;
    for (int q = threadIdx.x; q < a.T; q += blockDim.x) in_lds[q] = a.times[q];
    const float* src = a.obs + (size_t)b0 * 4 * a.T;
    for (int q = threadIdx.x; q < nb * 4 * a.T; q += blockDim.x) in_lds[a.T + q] = src[q];
    if constexpr (NF > 0) {  // (a row's samples are contiguous, the rows are C apart)
      const int per_row = NF * a.T, f_base = a.T + nb * 4 * a.T;
      const float* fsrc = a.cond + (size_t)b0 * a.C + (a.C - cond_tail<M>() - cond_mask_words<M>(a.T) - per_row);
      for (int q = threadIdx.x; q < nb * per_row; q += blockDim.x)
        in_lds[f_base + q] = fsrc[(size_t)(q / per_row) * a.C + q % per_row];
    }
    if constexpr (MASKED) {  // (a row's T words are contiguous behind its forcing samples, the rows are C apart)
      const int m_base = a.T + nb * (4 + NF) * a.T;
      const float* msrc = a.cond + (size_t)b0 * a.C + (a.C - cond_tail<M>() - a.T);
      for (int q = threadIdx.x; q < nb * a.T; q += blockDim.x) in_lds[m_base + q] = msrc[(size_t)(q / a.T) * a.C + q % a.T];
    }
    __syncthreads();
    const int ii = min((int)(blockIdx.x * blockDim.x + threadIdx.x), a.n - 1);
    ob_off = a.T + (ii / a.S - b0) * 4 * a.T;
    if constexpr (NF > 0) ff.lds = a.T + nb * 4 * a.T + (ii / a.S - b0) * NF * a.T;
    if constexpr (MASKED) ff.mlds = a.T + nb * (4 + NF) * a.T + (ii / a.S - b0) * a.T;
  }
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  const int b = i / a.S;
  float th[M::NSLOT], prec[4], c[M::NC > 0 ? M::NC : 1], p[M::NP], y[N];
  load_theta<M>(a, i, b, th, prec, c);
  if constexpr (is_blackbox<M>::value) {
    M::prepare_bb(th, a, b, p);
    M::init_bb(th, a, y);
  } else {
    M::prepare(th, c, p);
    if constexpr (M::NEURAL_PREC) p[M::NP - 1] = __int_as_float(a.n_hidden_prec);
    M::init(th, c, y);
  }

  float lc[4], lp[4];
  VIHDS_UNROLL for (int j = 0; j < 4; ++j) {
    if constexpr (OWN_LIK) lc[j] = 0.f;  // (unused: the model's own log density takes the precisions as they are)
    else if constexpr (OWN_PREC) lc[j] = 0.f;  // (unused: the own branch of the time loop forms the term from its values)
    else lc[j] = M::NEURAL_PREC ? 0.f : LOG2PI_F - logf(prec[j]);
    lp[j] = 0.f;
  }
  const float* ob = a.obs + (size_t)b * 4 * a.T;
  auto time_at = [&](int k) { return LDS_IN ? in_lds[k] : a.times[k]; };
  auto obs_at = [&](int j, int k) { return LDS_IN ? in_lds[ob_off + j * a.T + k] : ob[j * a.T + k]; };
  const float h0 = a.times[1] - a.times[0];
  const size_t n = a.n;

  // A trajectory larger than the chip's caches (the evaluation shape: 644 MB at B=234, S=1000) is written with streaming
  // (non-temporal) stores: its lines are not kept dirty in L2 / Infinity Cache, so the summaries launch that follows does not
  // share HBM with their write-back.  Training shapes keep ordinary stores (the adjoint re-reads them from cache).
  const bool nt_traj = VIHDS_NT_TRAJ && (size_t)a.n * NT * a.T * sizeof(float) > ((size_t)256 << 20);
  // times / observations are fetched one step ahead so their latency is off the dependent chain
  float tA = time_at(0), tB = time_at(1);
  float obc[4], obn[4];
  VIHDS_UNROLL for (int j = 0; j < 4; ++j) { obc[j] = a.logp ? obs_at(j, 0) : 0.f; obn[j] = 0.f; }
  // forcing samples travel with the times: ff.lo / ff.hi at tA / tB, the next point's requested one iteration ahead like tC
  if constexpr (NF > 0) {
    ff.src = a.cond + (size_t)b * a.C + (a.C - cond_tail<M>() - cond_mask_words<M>(a.T) - NF * a.T);
    VIHDS_UNROLL for (int j = 0; j < NF; ++j) {
      ff.lo[j] = LDS_IN ? in_lds[ff.lds + j * a.T] : ff.src[j * a.T];
      ff.hi[j] = LDS_IN ? in_lds[ff.lds + j * a.T + 1] : ff.src[j * a.T + 1];
    }
  }
  // mask words travel with the observations: ff.word at the current point, the next point's requested one iteration ahead
  if constexpr (MASKED) {
    ff.msrc = a.cond + (size_t)b * a.C + (a.C - cond_tail<M>() - a.T);
    ff.word = LDS_IN ? in_lds[ff.mlds] : ff.msrc[0];
    ff.word_ahead = ff.word;
  }
  if constexpr (has_start<M>::value || lead_in<M>::value > 0 || has_steady<M>::value > 0) {
    // where the trajectory starts, for a generated model that says so (a branch of its own: every other model's code stays what
    // it was).  start maps what init returned, with the first forcing samples in p (set_point); steady then takes the steady
    // species from that guess to a steady state of the pre-culture system (vihds_steady.hpp); the lead-in phase then takes
    // the scheme from t_0 - L to t_0 with those samples held (slope 0) and rhs seeing the true t < t_0.  Nothing of it is
    // stored, observed or scored: the time loop below begins at y_0
    if constexpr (NF > 0) M::set_point(p, ff.lo);
    if constexpr (has_start<M>::value) {
      float ys[N];
      M::start(y, p, ys);
      VIHDS_UNROLL for (int j = 0; j < N; ++j) y[j] = ys[j];
    }
    if constexpr (has_steady<M>::value > 0) M::steady(y, p);
    if constexpr (lead_in<M>::value > 0) {
      if constexpr (NF > 0) M::set_interval(p, tA - M::LEAD_TIME, 0.f, ff.lo, ff.lo);
      ode_lead_in<M, SOLVER>(tA, y, p, wts);
    }
  }
  if constexpr (has_diffusion<M>::value) ff.key = sde_load_key(a.cond, a.C, b, i);
  if constexpr (ND > 0) {  // the history before t_0 is the state stored at t_0 (after start, where the model has one)
    VIHDS_UNROLL for (int e = 0; e < ND; ++e) {
      ff.y0[e] = y[M::delay_species(e)];
      ff.cur[e] = 0;
    }
  }
  for (int k = 0; k < a.T; ++k) {
    const float tC = (k + 1 < a.T) ? time_at(k + 1) : tB;
    if (a.logp && k + 1 < a.T) {
      VIHDS_UNROLL for (int j = 0; j < 4; ++j) obn[j] = obs_at(j, k + 1);
    }
    if constexpr (MASKED) {
      if (k + 1 < a.T) ff.word_ahead = LDS_IN ? in_lds[ff.mlds + k + 1] : ff.msrc[k + 1];
    }
    if constexpr (NF > 0) {
      VIHDS_UNROLL for (int j = 0; j < NF; ++j) {
        ff.ahead[j] = ff.hi[j];
        if (k + 1 < a.T) ff.ahead[j] = LDS_IN ? in_lds[ff.lds + j * a.T + k + 1] : ff.src[j * a.T + k + 1];
      }
    }
    if (k > 0) {
      if constexpr (NF > 0) M::set_interval(p, tA, 1.f / (tB - tA), ff.lo, ff.hi);
      if constexpr (ND > 0) {
        // delayed reads of the interval k - 1 = [tA, tB]: the two lookups per read into the points 0 .. k - 1, which this
        // thread stored in its earlier iterations (vihds_delay.hpp: the indices are clamped into that range before any load)
        float d_lo[ND], d_hi[ND];
        const float t0 = time_at(0);
        VIHDS_UNROLL for (int e = 0; e < ND; ++e) {
          const float tau = p[M::delay_param(e)];
          auto y_at = [&](int q) { return a.traj[((size_t)q * NT + M::delay_species(e)) * n + i]; };
          const DelayEnds en = delay_ends(tA, tB, tau);
          ff.cur[e] = delay_seek_up(time_at, ff.cur[e], k - 1, en.s_lo);
          d_lo[e] = delay_lookup(time_at, y_at, ff.cur[e], en.s_lo, t0, ff.y0[e], tau).value;
          const int jh = delay_seek_up(time_at, ff.cur[e], k - 1, en.s_hi);
          d_hi[e] = delay_lookup(time_at, y_at, jh, en.s_hi, t0, ff.y0[e], tau).value;
        }
        M::set_delay(p, tA, 1.f / (tB - tA), d_lo, d_hi);
      }
      if constexpr (has_diffusion<M>::value) {
        // process noise (a branch of its own: every other model's code stays what it was): every step of the interval k - 1 adds
        // g(u) sqrt(h) xi, its draws counted by the trajectory, the species and the step (vihds_sde.hpp)
        if constexpr (substeps<M>::value > 1) ode_substeps<M, SOLVER>(tA, tB, h0, y, p, wts, k - 1, ff.key);
        else noisy_step<M, SOLVER>(tA, tB, h0, sde_step_index(k - 1, 1, 0), ff.key, y, p, wts);
      } else if constexpr (step_control<M>::value) ff.code = ode_stepctl<M, SOLVER>(tA, tB, y, p, wts);  // (the trajectory's own count)
      else if constexpr (substeps<M>::value > 1) ode_substeps<M, SOLVER>(tA, tB, h0, y, p, wts);  // (one interval, several steps)
      else ode_step<M, SOLVER>(tA, tB, h0, y, p, wts);
      tA = tB;
      if constexpr (NF > 0) {
        VIHDS_UNROLL for (int j = 0; j < NF; ++j) ff.lo[j] = ff.hi[j];
      }
    }
    tB = tC;
    if constexpr (NF > 0) {  // the hooks of this time point read the sample itself
      VIHDS_UNROLL for (int j = 0; j < NF; ++j) ff.hi[j] = ff.ahead[j];
      M::set_point(p, ff.lo);
    }
    if (a.traj) {
      if (nt_traj) {  // (streaming stores at evaluation-sized launches: see nt_traj)
        VIHDS_UNROLL for (int j = 0; j < N; ++j) __builtin_nontemporal_store(y[j], &a.traj[((size_t)k * NT + j) * n + i]);
      } else {
        VIHDS_UNROLL for (int j = 0; j < N; ++j) a.traj[((size_t)k * NT + j) * n + i] = y[j];
      }
      if constexpr (step_control<M>::value) {  // the count row, the last of the point's rows: the interval that ended here (0 at k = 0)
        if (nt_traj) __builtin_nontemporal_store(ff.code, &a.traj[((size_t)k * NT + (NT - 1)) * n + i]);
        else a.traj[((size_t)k * NT + (NT - 1)) * n + i] = ff.code;
      }
    }
    float xp[4];
    if constexpr (M::OBS == OBS_CUSTOM) M::observe(y, p, xp);
    else observe<M::OBS>(y, xp);
    if (a.xpred) {
      VIHDS_UNROLL for (int j = 0; j < 4; ++j) a.xpred[((size_t)k * 4 + j) * n + i] = xp[j];
    }
    if constexpr (MASKED) {
      // missing observations (vihds_mask.hpp; a branch of its own: every other model's code stays what it was).  The three
      // branches below in one: the precisions are the model's own map's (stored behind the species as there), the precision
      // states or the constant slots; every term is formed from obu = ob', the read where the point's mask word has one and the
      // predicted signal where it has none -- the placeholder never enters the arithmetic --, and joins lp by a select
      const ObsMask om(ff.word);
      ff.word = ff.word_ahead;
      float prl[4];
      if constexpr (OWN_PREC) {
        M::precision(y, xp, p, prl);
        if (a.traj) {
          if (nt_traj) {
            VIHDS_UNROLL for (int j = 0; j < 4; ++j) __builtin_nontemporal_store(prl[j], &a.traj[((size_t)k * NT + N + j) * n + i]);
          } else {
            VIHDS_UNROLL for (int j = 0; j < 4; ++j) a.traj[((size_t)k * NT + N + j) * n + i] = prl[j];
          }
        }
      } else {
        VIHDS_UNROLL for (int j = 0; j < 4; ++j) prl[j] = M::NEURAL_PREC ? y[(M::N - 4) + j] : prec[j];
      }
      if (a.logp) {
        float obu[4], ll[4];
        VIHDS_UNROLL for (int j = 0; j < 4; ++j) obu[j] = om.read(j, obc[j], xp[j]);
        if constexpr (OWN_LIK) {
          M::loglik(xp, obu, prl, p, ll);
        } else {
          VIHDS_UNROLL for (int j = 0; j < 4; ++j) {
            const float e = xp[j] - obu[j];
            if (OWN_PREC || M::NEURAL_PREC) ll[j] = -0.5f * (LOG2PI_F - logf(prl[j]) + prl[j] * e * e);
            else ll[j] = -0.5f * (lc[j] + prl[j] * e * e);
          }
        }
        VIHDS_UNROLL for (int j = 0; j < 4; ++j) {
          lp[j] += om.gate(j, ll[j]);
          obc[j] = obn[j];
        }
      }
    } else if constexpr (OWN_LIK) {
      // an observation log density of the model's own (a branch of its own: every other model's code stays what it was).  Its
      // precisions are the constant slots, or the values of the model's own map, which are stored as in the branch below
      float prl[4];
      if constexpr (OWN_PREC) {
        M::precision(y, xp, p, prl);
        if (a.traj) {
          if (nt_traj) {
            VIHDS_UNROLL for (int j = 0; j < 4; ++j) __builtin_nontemporal_store(prl[j], &a.traj[((size_t)k * NT + N + j) * n + i]);
          } else {
            VIHDS_UNROLL for (int j = 0; j < 4; ++j) a.traj[((size_t)k * NT + N + j) * n + i] = prl[j];
          }
        }
      } else {
        VIHDS_UNROLL for (int j = 0; j < 4; ++j) prl[j] = prec[j];
      }
      if (a.logp) {
        float ll[4];
        M::loglik(xp, obc, prl, p, ll);
        VIHDS_UNROLL for (int j = 0; j < 4; ++j) {
          lp[j] += ll[j];
          obc[j] = obn[j];
        }
      }
    } else if constexpr (OWN_PREC) {
      // a precision map of the model's own: evaluated on the species and the predicted signals of this time point, stored
      // as the four rows behind the species (where a *_precisions model keeps its precision states); the log-likelihood
      // term is the neural branch's.  (A branch of its own: every other model's code stays what it was.)
      float pr4[4];
      M::precision(y, xp, p, pr4);
      if (a.traj) {
        if (nt_traj) {
          VIHDS_UNROLL for (int j = 0; j < 4; ++j) __builtin_nontemporal_store(pr4[j], &a.traj[((size_t)k * NT + N + j) * n + i]);
        } else {
          VIHDS_UNROLL for (int j = 0; j < 4; ++j) a.traj[((size_t)k * NT + N + j) * n + i] = pr4[j];
        }
      }
      if (a.logp) {
        VIHDS_UNROLL for (int j = 0; j < 4; ++j) {
          const float e = xp[j] - obc[j];
          const float pr = pr4[j];
          lp[j] += -0.5f * (LOG2PI_F - logf(pr) + pr * e * e);
          obc[j] = obn[j];
        }
      }
    } else if (a.logp) {
      VIHDS_UNROLL for (int j = 0; j < 4; ++j) {
        const float e = xp[j] - obc[j];
        if (M::NEURAL_PREC) {  // precisions are ODE states (reference precisions.py:89-94)
          const float pr = y[(M::N - 4) + j];
          lp[j] += -0.5f * (LOG2PI_F - logf(pr) + pr * e * e);
        } else {
          lp[j] += -0.5f * (lc[j] + prec[j] * e * e);
        }
        obc[j] = obn[j];
      }
    }
    if constexpr (has_jump<M>::value) {
      // a state jump of the model's own (a branch of its own: every other model's code stays what it was): what was stored,
      // observed and scored above is the left limit y_k; the step of the next iteration starts from jump(y_k), evaluated
      // while p still holds the point's forcing samples (set_point).  A jump at the last point has no effect: not evaluated
      if (k + 1 < a.T) {
        float yj[N];
        M::jump(y, p, yj);
        VIHDS_UNROLL for (int j = 0; j < N; ++j) y[j] = yj[j];
      }
    }
  }
  if (a.logp) {
    VIHDS_UNROLL for (int j = 0; j < 4; ++j) a.logp[(size_t)j * n + i] = lp[j];
  }
}

// ---- evaluation summaries without the trajectory's round trip through HBM (round 5) -------------------------------------
// Results.init (reference vihds/utils.py:79-99) needs, per data row and time point, sums over the row's samples weighted with
// the NORMALISED importance weights -- which exist only when every sample's last time point does.  The evaluation pass used
// to write the trajectory (644 MB at B = 234, S = 1 000) and stream it back through vihds_iw_summaries_states; now a first
// forward launch writes the log-likelihoods only (traj == NULL), the weights are formed, and THIS kernel integrates again
// and adds up on the way: per time point NV = n_species + 12 weighted values per lane, summed over the wavefront with
// gfx950's row swaps (2.5 instructions per value instead of 6 DPP additions), one partial row per wavefront and time point
// (26 MB at that size), which summ_finish_kernel adds up in a fixed order.  The integration is ode_fwd_kernel's (same
// ode_step, same operands): the trajectory summed here is bit for bit the one the weights were computed from.
// grid: (ceil(S / 256), B), 256 threads: every wavefront's 64 samples belong to one data row.

// v[0 .. NVP): per-lane values -> u[p] (p < NVP / 4): in the lanes of row r (lanes 16 r .. 16 r + 15) the wavefront's total of
// value 4 p + {0, 2, 1, 3}[r]
// (NR <= NVP / 4 output registers: only the first 4 NR values are summed.  A swap costs the issuing wavefront 15 cycles, 23
// with a nop of its own -- tests/micro/permlane_rate.hip)
template <int NVP, int NR>
__device__ __forceinline__ void wave_sum_rows(const float (&v)[NVP], float (&u)[NVP / 4]) {
  static_assert(NVP % 4 == 0 && NR <= NVP / 4, "pad the values to a multiple of four");
  float a[2 * NR], b[2 * NR];
#pragma unroll
  for (int p = 0; p < 2 * NR; ++p) { a[p] = v[2 * p]; b[p] = v[2 * p + 1]; }
  // lanes l and l ^ 32: rows 0, 1 keep value 2 p, rows 2, 3 value 2 p + 1
  // (two swaps per asm block behind ONE s_nop: the compiler may put the copies that feed a swap right in front of its
  // block, and the swap reads a VALU result two wait states late at the earliest)
#pragma unroll
  for (int p = 0; p < 2 * NR; p += 2)
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\tv_permlane32_swap_b32 %2, %3"
                 : "+v"(a[p]), "+v"(b[p]), "+v"(a[p + 1]), "+v"(b[p + 1]));
  float c[NR], d[NR];
#pragma unroll
  for (int p = 0; p < NR; ++p) { c[p] = a[2 * p] + b[2 * p]; d[p] = a[2 * p + 1] + b[2 * p + 1]; }
  // rows 0 + 1 and 2 + 3 of each: one value per row
#pragma unroll
  for (int p = 0; p + 1 < NR; p += 2)
    asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1\n\tv_permlane16_swap_b32 %2, %3"
                 : "+v"(c[p]), "+v"(d[p]), "+v"(c[p + 1]), "+v"(d[p + 1]));
  if (NR & 1) asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(c[NR - 1]), "+v"(d[NR - 1]));
#pragma unroll
  for (int p = 0; p < NR; ++p) u[p] = c[p] + d[p];
  // all 16 lanes of a row: rotations by 8, 4, 2, 1 (every lane ends with the row's total), the registers side by side
#pragma unroll
  for (int p = 0; p < NR; ++p) u[p] += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, u[p]), 0x128, 0xf, 0xf, false));
#pragma unroll
  for (int p = 0; p < NR; ++p) u[p] += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, u[p]), 0x124, 0xf, 0xf, false));
#pragma unroll
  for (int p = 0; p < NR; ++p) u[p] += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, u[p]), 0x122, 0xf, 0xf, false));
#pragma unroll
  for (int p = 0; p < NR; ++p) u[p] += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, u[p]), 0x121, 0xf, 0xf, false));
}

template <class M>
struct SummLayout {
  static constexpr int NS = M::NEURAL_PREC ? M::N - 4 : M::N;  // species (the last four states of a neural-precision model are the precisions)
  static constexpr int NV = NS + 12, NVP = (NV + 3) & ~3;      // states | w x | w (x^2 + 1 / prec) | w / prec
};

template <class M, int SOLVER>
__global__ void __launch_bounds__(256) ode_fwd_summ_kernel(OdeArgs a, SummArgs sa) {
  constexpr int N = M::N;
  using L = SummLayout<M>;
  constexpr int NS = L::NS, NVP = L::NVP;
  __shared__ float wlds[M::NW > 0 ? M::NW : 1];
  extern __shared__ float in_lds[];  // [T] times
  const float* wts = stage_weights<M>(a, wlds);
  for (int q = threadIdx.x; q < a.T; q += blockDim.x) in_lds[q] = a.times[q];
  __syncthreads();
  const int b = blockIdx.y;
  const int s0 = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = s0 < a.S;
  const int i = b * a.S + (live ? s0 : a.S - 1);  // (idle lanes shadow the row's last sample at weight 0)
  float th[M::NSLOT], prec[4], c[M::NC > 0 ? M::NC : 1], p[M::NP], y[N];
  load_theta<M>(a, i, b, th, prec, c);
  M::prepare(th, c, p);
  if constexpr (M::NEURAL_PREC) p[M::NP - 1] = __int_as_float(a.n_hidden_prec);
  M::init(th, c, y);
  const float w = live ? expf(sa.log_w[i] - sa.lse[b]) : 0.f;
  float ivc[4];  // 1 / precision (constant precisions)
  VIHDS_UNROLL for (int j = 0; j < 4; ++j) ivc[j] = M::NEURAL_PREC ? 0.f : 1.f / prec[j];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // the wavefront's partial rows [T][NVP]; lane 16 r writes the values of row r (wave_sum_rows)
  float* out = sa.partial + ((size_t)b * sa.nch + (size_t)blockIdx.x * (blockDim.x >> 6) + wave) * (size_t)a.T * NVP;
  const int row = lane >> 4;
  const int slot = row == 1 ? 2 : (row == 2 ? 1 : row);
  const bool writer = (lane & 15) == 0;
  float* p_out = out + slot;
  const float h0 = a.times[1] - a.times[0];
  float tA = in_lds[0], tB = in_lds[a.T > 1 ? 1 : 0];
  __builtin_amdgcn_s_waitcnt(0);  // (nothing loaded before the loop is waited for inside it, behind the loop's stores)
  for (int k = 0; k < a.T; ++k) {
    const float tC = (k + 1 < a.T) ? in_lds[k + 1] : tB;
    if (k > 0) {
      ode_step<M, SOLVER>(tA, tB, h0, y, p, wts);
      tA = tB;
    }
    tB = tC;
    float xp[4];
    observe<M::OBS>(y, xp);
    float v[NVP];
    VIHDS_UNROLL for (int j = 0; j < NVP; ++j) v[j] = 0.f;
    VIHDS_UNROLL for (int j = 0; j < NS; ++j) v[j] = w * y[j];
    VIHDS_UNROLL for (int j = 0; j < 4; ++j) {
      const float iv = M::NEURAL_PREC ? 1.f / y[NS + j] : ivc[j];  // (per-sample terms as vihds_iw_summaries forms them)
      v[NS + j] = w * xp[j];
      v[NS + 4 + j] = w * (xp[j] * xp[j] + iv);
      v[NS + 8 + j] = w * iv;
    }
    // constant precisions: the four sums of w / precision do not depend on the time point -- they are taken at the first one
    // only (summ_finish_kernel hands them to every time point)
    constexpr int NR_ALL = NVP / 4, NR_STEP = M::NEURAL_PREC ? NR_ALL : (NS + 8 + 3) / 4;
    float u[NVP / 4];
    if (k == 0) {
      wave_sum_rows<NVP, NR_ALL>(v, u);
      if (writer) {
        VIHDS_UNROLL for (int q = 0; q < NR_ALL; ++q) p_out[4 * q] = u[q];
      }
    } else {
      wave_sum_rows<NVP, NR_STEP>(v, u);
      if (writer) {
        VIHDS_UNROLL for (int q = 0; q < NR_STEP; ++q) p_out[4 * q] = u[q];
      }
    }
    p_out += NVP;
  }
}
template <class M, int ONLY>
inline int launch_fwd_summ(int solver, const OdeArgs& a, const SummArgs& sa, hipStream_t st) {
  if constexpr (is_blackbox<M>::value) return VIHDS_E_UNSUPPORTED;
  else {
    if (sa.nvp != SummLayout<M>::NVP || sa.nch != ((a.S + 255) / 256) * 4) return VIHDS_E_BADARG;
    const dim3 grid((a.S + 255) / 256, a.B);
    const size_t lds = (size_t)a.T * sizeof(float);
#define VIHDS_SUMM_CASE(SV)                                                                                         \
  case SV:                                                                                                        \
    if constexpr (ONLY < 0 || SV == ONLY) {                                                                       \
      hipLaunchKernelGGL((ode_fwd_summ_kernel<M, SV>), grid, dim3(256), lds, st, a, sa);                           \
      return VIHDS_OK;                                                                                            \
    }                                                                                                             \
    break;
    switch (solver) {
      VIHDS_SUMM_CASE(VIHDS_SOLVER_MODEULER)
      VIHDS_SUMM_CASE(VIHDS_SOLVER_MODEULERWHILE)
      VIHDS_SUMM_CASE(VIHDS_SOLVER_EULER)
      VIHDS_SUMM_CASE(VIHDS_SOLVER_MIDPOINT)
      VIHDS_SUMM_CASE(VIHDS_SOLVER_RK4)
    }
#undef VIHDS_SUMM_CASE
    return VIHDS_E_UNSUPPORTED;  // (the adaptive pairs keep the two-kernel form)
  }
}

// ---- backward ------------------------------------------------------------------------------------
template <class M, int SOLVER, bool DUMP = false>
__global__ void __launch_bounds__(256) ode_bwd_kernel(OdeArgs a) {
  constexpr int N = M::N;
  constexpr int NT = traj_rows<M>::value;  // rows per time point of traj_in / g_traj (the precision rows of traj_in are never read)
  constexpr bool OWN_PREC = own_prec<M>::value;
  constexpr bool OWN_LIK = own_lik<M>::value;  // the log density's adjoint is the model's own member (vihds_models.hpp)
  constexpr int NF = n_forcings<M>::value;     // forcings: K series of T samples per data row behind its treatments in cond
  constexpr int ND = n_delays<M>::value;       // delayed reads: looked up in traj_in, their adjoint scattered into aux
  constexpr bool MASKED = masked_obs<M>::value;  // missing observations: one mask word per time point in the row of cond
  __shared__ float wlds[M::NW > 0 ? M::NW : 1];
  const float* wts = stage_weights<M>(a, wlds);
  const int i0 = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = i0 < a.n;
  const int i = live ? i0 : a.n - 1;  // tail lanes shadow the last trajectory (they take part in the reductions)
  const int b = i / a.S;
  float th[M::NSLOT], prec[4], c[M::NC > 0 ? M::NC : 1], p[M::NP];
  load_theta<M>(a, i, b, th, prec, c);
  if constexpr (is_blackbox<M>::value) {
    M::prepare_bb(th, a, b, p);
  } else {
    M::prepare(th, c, p);
    if constexpr (M::NEURAL_PREC) p[M::NP - 1] = __int_as_float(a.n_hidden_prec);
  }

  float lam[N], pb[M::NP], precb[4], glp[4];
  VIHDS_UNROLL for (int j = 0; j < N; ++j) lam[j] = 0.f;
  VIHDS_UNROLL for (int j = 0; j < M::NP; ++j) pb[j] = 0.f;
  // backward context: per-thread shared-weight gradient accumulators (white-box + neural precisions), or the
  // evaluation dump cursor (dr_blackbox)
  using CtxImpl = typename bwd_ctx_sel<M, DUMP>::impl;
  typename CtxImpl::type wtsb;
  CtxImpl::init(wtsb, a, i);
  const size_t n = a.n;
  const float w_iw = a.iw_logp ? iw_wave_weight(a, i, b) : 0.f;
  VIHDS_UNROLL for (int j = 0; j < 4; ++j) {
    precb[j] = 0.f;
    glp[j] = ode_logp_grad(a, w_iw, i, j);
  }
  const float* ob = a.obs + (size_t)b * 4 * a.T;
  const float h0 = a.times[1] - a.times[0];

  // software pipeline: the stored state, observations and times of step k-1 are requested while step k computes
  float yn[N], obn[4];
  VIHDS_UNROLL for (int j = 0; j < N; ++j) yn[j] = a.traj_in[((size_t)(a.T - 1) * NT + j) * n + i];
  VIHDS_UNROLL for (int j = 0; j < 4; ++j) obn[j] = ob[j * a.T + a.T - 1];
  float tHi = a.times[a.T - 1], tLo = tHi;
  // forcing samples travel with the times: ff.hi at tHi, ff.lo at tK, the next lower point's (ff.ahead) requested one
  // iteration ahead like tLo
  // (ForcingFeed<NF>; an implicit solver's also keeps y_k+1, a model with delayed reads y_0 and its cursors, one with process
  // noise its key, one with missing observations its mask words, one with step control the codes of the count row)
  ctl_feed_t<mask_feed_t<noise_feed_t<delay_feed_t<bwd_feed_t<NF, N, solver_is_implicit(SOLVER)>, ND>, has_diffusion<M>::value>, MASKED>,
             step_control<M>::value> ff;
  // the count row travels with the stored states: the code of the point k (the interval below it) requested one iteration ahead
  if constexpr (step_control<M>::value) ff.code_ahead = 0.f;
  // mask words travel with the observations: the word of the point k - 1 (ff.word_ahead) requested one iteration ahead like obn
  if constexpr (MASKED) {
    ff.msrc = a.cond + (size_t)b * a.C + (a.C - cond_tail<M>() - a.T);
    ff.word_ahead = ff.msrc[a.T - 1];
  }
  if constexpr (ND > 0) {
    // the history adjoint A[entry][T] of this trajectory: its own column of aux, zeroed here and touched by no other thread
    // (a tail lane shadows the last trajectory: it reads that column and never writes it)
    VIHDS_UNROLL for (int e = 0; e < ND; ++e) {
      ff.y0[e] = a.traj_in[(size_t)M::delay_species(e) * n + i];
      ff.cur[e] = a.T - 2;
      if (live) {
        for (int q = 0; q < a.T; ++q) a.aux[((size_t)e * a.T + q) * n + i] = 0.f;
      }
    }
  }
  if constexpr (has_diffusion<M>::value) ff.key = sde_load_key(a.cond, a.C, b, i);
  if constexpr (NF > 0) {
    ff.src = a.cond + (size_t)b * a.C + (a.C - cond_tail<M>() - cond_mask_words<M>(a.T) - NF * a.T);
    VIHDS_UNROLL for (int j = 0; j < NF; ++j) { ff.ahead[j] = ff.src[j * a.T + a.T - 1]; ff.hi[j] = ff.ahead[j]; }
  }
  for (int k = a.T - 1; k >= 0; --k) {
    float y[N], obk[4];
    VIHDS_UNROLL for (int j = 0; j < N; ++j) y[j] = yn[j];
    VIHDS_UNROLL for (int j = 0; j < 4; ++j) obk[j] = obn[j];
    const float tK = tLo;
    if constexpr (NF > 0) {
      VIHDS_UNROLL for (int j = 0; j < NF; ++j) ff.lo[j] = ff.ahead[j];
    }
    if constexpr (MASKED) {
      ff.word = ff.word_ahead;
      if (k > 0) ff.word_ahead = ff.msrc[k - 1];
    }
    if constexpr (step_control<M>::value) {  // (ff.code: the count of the interval k, stored at the point k + 1)
      ff.code = ff.code_ahead;
      if (k > 0) ff.code_ahead = a.traj_in[((size_t)k * NT + (NT - 1)) * n + i];
    }
    if (k > 0) {
      VIHDS_UNROLL for (int j = 0; j < N; ++j) yn[j] = a.traj_in[((size_t)(k - 1) * NT + j) * n + i];
      VIHDS_UNROLL for (int j = 0; j < 4; ++j) obn[j] = ob[j * a.T + k - 1];
      tLo = a.times[k - 1];
      if constexpr (NF > 0) {
        VIHDS_UNROLL for (int j = 0; j < NF; ++j) ff.ahead[j] = ff.src[j * a.T + k - 1];
      }
    }
    if constexpr (NF > 0) {  // the interval (k, k + 1) ...
      if (k < a.T - 1) M::set_interval(p, tK, 1.f / (tHi - tK), ff.lo, ff.hi);
    }
    if constexpr (ND > 0) {
      // delayed reads (a branch of its own: every other model's code stays what it was; such a model has no jump, sub-steps
      // or implicit scheme).  The interval k = [tK, tHi] repeats the forward's two lookups per read on the forward's operands
      // (the same bits), runs the step adjoint, then takes and clears the read's value and slope adjoints and scatters them
      // into the history adjoint at the points the lookups read -- which may be the point k itself: A[.][k] joins lam below
      if (k < a.T - 1) {
        float d_lo[ND], d_hi[ND];
        DelayHit lo[ND], hi[ND];
        bool moves[ND];
        const float t0 = a.times[0], inv_dt = 1.f / (tHi - tK);
        auto time_at = [&](int q) { return a.times[q]; };
        VIHDS_UNROLL for (int e = 0; e < ND; ++e) {
          const float tau = p[M::delay_param(e)];
          auto y_at = [&](int q) { return a.traj_in[((size_t)q * NT + M::delay_species(e)) * n + i]; };
          const DelayEnds en = delay_ends(tK, tHi, tau);
          ff.cur[e] = delay_seek_down(time_at, ff.cur[e], k, en.s_lo);
          lo[e] = delay_lookup(time_at, y_at, ff.cur[e], en.s_lo, t0, ff.y0[e], tau);
          hi[e] = delay_lookup(time_at, y_at, delay_seek_up(time_at, ff.cur[e], k, en.s_hi), en.s_hi, t0, ff.y0[e], tau);
          moves[e] = !en.clamped;
          d_lo[e] = lo[e].value;
          d_hi[e] = hi[e].value;
        }
        M::set_delay(p, tK, inv_dt, d_lo, d_hi);
        ode_step_vjp<M, SOLVER>(tK, tHi, h0, y, p, wts, lam, pb, wtsb);
        VIHDS_UNROLL for (int e = 0; e < ND; ++e) {
          const float g_hi = pb[M::DELAY_SLOT + ND + e] * inv_dt, g_lo = pb[M::DELAY_SLOT + e] - g_hi;
          pb[M::DELAY_SLOT + e] = 0.f;
          pb[M::DELAY_SLOT + ND + e] = 0.f;
          if (live) {
            auto a_at = [&](int q) -> float& { return a.aux[((size_t)e * a.T + q) * n + i]; };
            const float taub = delay_scatter(a_at, lo[e], g_lo, true) + delay_scatter(a_at, hi[e], g_hi, moves[e]);
            if (p[M::delay_param(e)] > 0.f) pb[M::delay_param(e)] += taub;  // (taue = fmaxf(tau, 0))
          }
        }
      }
    } else if constexpr (has_diffusion<M>::value) {
      // process noise (a branch of its own: every other model's code stays what it was; such a model has no implicit scheme, no
      // delays and no lead-in).  The interval k started from the stored y_k, or from jump(y_k) recomputed as below; every step
      // adjoint regenerates its draws from the forward's counters (noisy_step_vjp), a sub-stepped interval recomputes its
      // sub-states by the forward's noisy steps (ode_substeps_vjp)
      if (k < a.T - 1) {
        float ys[N];
        if constexpr (has_jump<M>::value) {
          M::jump(y, p, ys);
        } else {
          VIHDS_UNROLL for (int j = 0; j < N; ++j) ys[j] = y[j];
        }
        if constexpr (substeps<M>::value > 1) ode_substeps_vjp<M, SOLVER>(tK, tHi, h0, ys, nullptr, p, wts, lam, pb, wtsb, k, ff.key);
        else noisy_step_vjp<M, SOLVER>(tK, tHi, h0, sde_step_index(k, 1, 0), ff.key, ys, p, wts, lam, pb, wtsb);
        if constexpr (has_jump<M>::value) {
          float lamk[N];
          VIHDS_UNROLL for (int j = 0; j < N; ++j) lamk[j] = 0.f;
          M::jump_vjp(y, p, lam, lamk, pb);
          VIHDS_UNROLL for (int j = 0; j < N; ++j) lam[j] = lamk[j];
        }
      }
    } else if constexpr (has_jump<M>::value) {
      // a state jump of the model's own (a branch of its own: every other model's code stays what it was).  The stored y is the
      // left limit y_k and the interval started from yj = jump(y_k): recomputed here by the forward's call on the forward's
      // operands (the value entries of p are u_k after set_interval), so the same bits.  The step adjoint runs from yj -- an
      // implicit step's at the stored y_k+1, which needs no start state --, then jump_vjp takes lam (the adjoint of yj) to the
      // adjoint of y_k and adds its parameter part to pb, ahead of the hook adjoints of the point, which add into that lam
      if (k < a.T - 1) {
        float yj[N], lamk[N];
        if constexpr (step_control<M>::value) {  // (the count the forward chose for this interval: ode_stepctl_vjp)
          M::jump(y, p, yj);
          if constexpr (solver_is_implicit(SOLVER)) ode_stepctl_vjp<M, SOLVER>(tK, tHi, ff.code, yj, ff.y_next, p, wts, lam, pb, wtsb);
          else ode_stepctl_vjp<M, SOLVER>(tK, tHi, ff.code, yj, nullptr, p, wts, lam, pb, wtsb);
        } else if constexpr (substeps<M>::value > 1) {
          M::jump(y, p, yj);
          if constexpr (solver_is_implicit(SOLVER)) ode_substeps_vjp<M, SOLVER>(tK, tHi, h0, yj, ff.y_next, p, wts, lam, pb, wtsb);
          else ode_substeps_vjp<M, SOLVER>(tK, tHi, h0, yj, nullptr, p, wts, lam, pb, wtsb);
        } else if constexpr (solver_is_implicit(SOLVER)) {
          if constexpr (implicit_order<M>::value == 2) {  // (the two-stage scheme's adjoint starts from yj as well)
            M::jump(y, p, yj);
            ode_step_vjp_sdirk2<M>(tK, tHi, yj, ff.y_next, p, wts, lam, pb, wtsb);
          } else {
            ode_step_vjp_implicit<M>(tK, tHi, ff.y_next, p, wts, lam, pb, wtsb);
          }
        } else {
          M::jump(y, p, yj);
          ode_step_vjp<M, SOLVER>(tK, tHi, h0, yj, p, wts, lam, pb, wtsb);
        }
        VIHDS_UNROLL for (int j = 0; j < N; ++j) lamk[j] = 0.f;
        M::jump_vjp(y, p, lam, lamk, pb);
        VIHDS_UNROLL for (int j = 0; j < N; ++j) lam[j] = lamk[j];
      }
      if constexpr (solver_is_implicit(SOLVER)) {  // (the interval below ends on the stored left limit y_k)
        VIHDS_UNROLL for (int j = 0; j < N; ++j) ff.y_next[j] = y[j];
      }
    } else if constexpr (step_control<M>::value) {  // (the existing interval adjoint at the count the forward chose: ode_stepctl_vjp)
      if constexpr (solver_is_implicit(SOLVER)) {
        if (k < a.T - 1) ode_stepctl_vjp<M, SOLVER>(tK, tHi, ff.code, y, ff.y_next, p, wts, lam, pb, wtsb);
        VIHDS_UNROLL for (int j = 0; j < N; ++j) ff.y_next[j] = y[j];
      } else {
        if (k < a.T - 1) ode_stepctl_vjp<M, SOLVER>(tK, tHi, ff.code, y, nullptr, p, wts, lam, pb, wtsb);
      }
    } else if constexpr (substeps<M>::value > 1) {  // (the interval's sub-states are recomputed from y = y_k: ode_substeps_vjp)
      if constexpr (solver_is_implicit(SOLVER)) {
        if (k < a.T - 1) ode_substeps_vjp<M, SOLVER>(tK, tHi, h0, y, ff.y_next, p, wts, lam, pb, wtsb);
        VIHDS_UNROLL for (int j = 0; j < N; ++j) ff.y_next[j] = y[j];
      } else {
        if (k < a.T - 1) ode_substeps_vjp<M, SOLVER>(tK, tHi, h0, y, nullptr, p, wts, lam, pb, wtsb);
      }
    } else if constexpr (solver_is_implicit(SOLVER)) {
      if (k < a.T - 1) ode_step_vjp_implicit_any<M>(tK, tHi, y, ff.y_next, p, wts, lam, pb, wtsb);
      VIHDS_UNROLL for (int j = 0; j < N; ++j) ff.y_next[j] = y[j];
    } else {
      if (k < a.T - 1) ode_step_vjp<M, SOLVER>(tK, tHi, h0, y, p, wts, lam, pb, wtsb);
    }
    tHi = tK;
    if constexpr (NF > 0) {  // ... then the point k, whose hook adjoints follow
      VIHDS_UNROLL for (int j = 0; j < NF; ++j) ff.hi[j] = ff.lo[j];
      M::set_point(p, ff.lo);
    }
    // gradient injected at time k: log-likelihood term, x_predict and trajectory upstream grads
    float xp[4], xpb[4];
    if constexpr (M::OBS == OBS_CUSTOM) M::observe(y, p, xp);
    else observe<M::OBS>(y, xp);
    if constexpr (MASKED) {
      // missing observations (vihds_mask.hpp; a branch of its own: every other model's code stays what it was).  The three
      // branches below in one, in their order of adjoints: the residuals are formed from obu = ob', as the forward's were, and the
      // log-likelihood's seed of an unobserved signal is 0 by a select; what arrives for x_predict and for the precision rows of
      // the trajectory is not masked.  On the in-kernel importance-weight route glp holds the trajectory's weight as before
      const ObsMask om(ff.word);
      float prl[4], prb4[4], obu[4], sd[4];
      if constexpr (OWN_PREC) {
        M::precision(y, xp, p, prl);
      } else {
        VIHDS_UNROLL for (int j = 0; j < 4; ++j) prl[j] = M::NEURAL_PREC ? y[(M::N - 4) + j] : prec[j];
      }
      VIHDS_UNROLL for (int j = 0; j < 4; ++j) {
        obu[j] = om.read(j, obk[j], xp[j]);
        sd[j] = om.gate(j, glp[j]);
        xpb[j] = 0.f;
        prb4[j] = 0.f;
      }
      if constexpr (OWN_LIK) {
        if (a.g_logp || a.iw_logp) M::loglik_vjp(xp, obu, prl, p, sd, xpb, prb4, pb);  // (skipped as below where no gradient arrives)
      } else {
        VIHDS_UNROLL for (int j = 0; j < 4; ++j) {
          const float e = xp[j] - obu[j];
          xpb[j] = -sd[j] * prl[j] * e;
          prb4[j] = sd[j] * (0.5f / prl[j] - 0.5f * e * e);
        }
      }
      VIHDS_UNROLL for (int j = 0; j < 4; ++j) {
        if constexpr (OWN_PREC) {
          if (a.g_traj) prb4[j] += a.g_traj[((size_t)k * NT + N + j) * n + i];
        } else if constexpr (M::NEURAL_PREC) {
          lam[(M::N - 4) + j] += prb4[j];
        } else {
          precb[j] += prb4[j];
        }
        if (a.g_xpred) xpb[j] += a.g_xpred[((size_t)k * 4 + j) * n + i];
      }
      if constexpr (OWN_PREC) M::precision_vjp(y, xp, p, prb4, lam, xpb, pb);
    } else if constexpr (OWN_LIK) {
      // an observation log density of the model's own (a branch of its own: every other model's code stays what it was).
      // Three adjoints in this order: the log density's (seeded with glp; it adds into xpb, prb4 and pb), then the precision
      // map's where the model has one (prb4 plus what arrives for the precision rows of the trajectory; into lam, xpb and
      // pb) -- constant precisions take prb4 into precb --, then the observation map's below, which pulls xpb back.  The
      // parameter parts join pb ahead of prepare_vjp.  Forward values are recomputed; nothing is buffered
      float prl[4], llb[4], prb4[4];
      if constexpr (OWN_PREC) {
        M::precision(y, xp, p, prl);
      } else {
        VIHDS_UNROLL for (int j = 0; j < 4; ++j) prl[j] = prec[j];
      }
      VIHDS_UNROLL for (int j = 0; j < 4; ++j) {
        llb[j] = glp[j];
        xpb[j] = 0.f;
        prb4[j] = 0.f;
      }
      // (no log-likelihood gradient arrives -- the host-driven adaptive route integrates on placeholder observations and forms
      // the log-likelihood itself: the adjoint is skipped, uniformly over the launch, not multiplied by zero: a density that is
      // singular at the placeholder would give 0 * inf)
      if (a.g_logp || a.iw_logp) M::loglik_vjp(xp, obk, prl, p, llb, xpb, prb4, pb);
      VIHDS_UNROLL for (int j = 0; j < 4; ++j) {
        if constexpr (OWN_PREC) {
          if (a.g_traj) prb4[j] += a.g_traj[((size_t)k * NT + N + j) * n + i];
        } else {
          precb[j] += prb4[j];
        }
        if (a.g_xpred) xpb[j] += a.g_xpred[((size_t)k * 4 + j) * n + i];
      }
      if constexpr (OWN_PREC) M::precision_vjp(y, xp, p, prb4, lam, xpb, pb);
    } else if constexpr (OWN_PREC) {
      // a precision map of the model's own (a branch of its own: every other model's code stays what it was).  The forward
      // values are recomputed, never read from traj_in; prb is the log-likelihood's part plus what arrives for the four
      // precision rows of the trajectory.  The precision adjoint goes into lam, xpb and pb BEFORE the observation map's
      // adjoint runs: a precision that depends on the predicted signals chains through observe_vjp; its parameter part joins
      // pb ahead of prepare_vjp like the map's
      float pr4[4], prb4[4];
      M::precision(y, xp, p, pr4);
      VIHDS_UNROLL for (int j = 0; j < 4; ++j) {
        const float e = xp[j] - obk[j];
        const float pr = pr4[j];
        xpb[j] = -glp[j] * pr * e;
        prb4[j] = glp[j] * (0.5f / pr - 0.5f * e * e);
        if (a.g_traj) prb4[j] += a.g_traj[((size_t)k * NT + N + j) * n + i];
        if (a.g_xpred) xpb[j] += a.g_xpred[((size_t)k * 4 + j) * n + i];
      }
      M::precision_vjp(y, xp, p, prb4, lam, xpb, pb);
    } else {
      VIHDS_UNROLL for (int j = 0; j < 4; ++j) {
        const float e = xp[j] - obk[j];
        const float pr = M::NEURAL_PREC ? y[(M::N - 4) + j] : prec[j];
        xpb[j] = -glp[j] * pr * e;
        const float prb = glp[j] * (0.5f / pr - 0.5f * e * e);
        if (M::NEURAL_PREC) lam[(M::N - 4) + j] += prb;
        else precb[j] += prb;
        if (a.g_xpred) xpb[j] += a.g_xpred[((size_t)k * 4 + j) * n + i];
      }
    }
    // (a custom map also has a parameter adjoint: it joins pb ahead of prepare_vjp and reaches g_theta through the epilogue)
    if constexpr (M::OBS == OBS_CUSTOM) M::observe_vjp(y, p, xpb, lam, pb);
    else observe_vjp<M::OBS>(y, xpb, lam);
    if (a.g_traj) {
      VIHDS_UNROLL for (int j = 0; j < N; ++j) lam[j] += a.g_traj[((size_t)k * NT + j) * n + i];
    }
    if constexpr (ND > 0) {  // what the later intervals' delayed reads took from the stored y_k
      VIHDS_UNROLL for (int e = 0; e < ND; ++e) lam[M::delay_species(e)] += a.aux[((size_t)e * a.T + k) * n + i];
    }
  }
  if constexpr (has_start<M>::value || lead_in<M>::value > 0 || has_steady<M>::value > 0) {
    // where the trajectory started (a branch of its own: every other model's code stays what it was).  lam is the adjoint of
    // y_0 and tHi is t_0; ff.lo holds the first forcing samples.  init, start and steady are recomputed by the forward's calls
    // on the forward's operands; the lead-in's step adjoints run last to first from the state steady returned (an implicit
    // scheme's last one at the stored y_0, which ff.y_next holds), then steady_vjp applies the implicit-function step at that
    // state and clears the steady species' adjoint, then start_vjp takes lam to the adjoint of what init returned and adds its
    // parameter part to pb ahead of prepare_vjp; init_vjp below is handed that state adjoint
    float yi[N];
    M::init(th, c, yi);
    if constexpr (NF > 0) M::set_point(p, ff.lo);
    if constexpr (lead_in<M>::value > 0 || has_steady<M>::value > 0) {
      float ys[N];
      if constexpr (has_start<M>::value) {
        M::start(yi, p, ys);
      } else {
        VIHDS_UNROLL for (int j = 0; j < N; ++j) ys[j] = yi[j];
      }
      if constexpr (has_steady<M>::value > 0) M::steady(ys, p);
      if constexpr (lead_in<M>::value > 0) {
        if constexpr (NF > 0) M::set_interval(p, tHi - M::LEAD_TIME, 0.f, ff.lo, ff.lo);  // (the value entries stay u_0)
        if constexpr (solver_is_implicit(SOLVER)) ode_lead_in_vjp<M, SOLVER>(tHi, ys, ff.y_next, p, wts, lam, pb, wtsb);
        else ode_lead_in_vjp<M, SOLVER>(tHi, ys, nullptr, p, wts, lam, pb, wtsb);
      }
      if constexpr (has_steady<M>::value > 0) M::steady_vjp(ys, p, lam, pb);
    }
    if constexpr (has_start<M>::value) {
      float lami[N];
      VIHDS_UNROLL for (int j = 0; j < N; ++j) lami[j] = 0.f;
      M::start_vjp(yi, p, lam, lami, pb);
      VIHDS_UNROLL for (int j = 0; j < N; ++j) lam[j] = lami[j];
    }
  }
  float thb[M::NSLOT];
  VIHDS_UNROLL for (int q = 0; q < M::NSLOT; ++q) thb[q] = 0.f;
  if constexpr (is_blackbox<M>::value) {
    M::prepare_vjp_bb(th, a, b, pb, thb);
    if (live) M::store_delta(a, i, pb, wtsb);
  } else {
    M::prepare_vjp(th, c, p, pb, thb);
  }
  M::init_vjp(lam, thb);
  if (live) {
    VIHDS_UNROLL for (int q = 0; q < M::NSLOT; ++q) a.g_theta[(size_t)a.slot_row[q] * n + i] = thb[q];
    if constexpr (!OWN_PREC) {  // (a precision map of the model's own has no precision slot rows: nothing to store)
      if (!M::NEURAL_PREC) {
        VIHDS_UNROLL for (int j = 0; j < 4; ++j) a.g_theta[(size_t)a.slot_row[M::NSLOT + j] * n + i] = precb[j];
      }
    }
  }
  if constexpr (!is_blackbox<M>::value && M::NEURAL_PREC) {
    if (a.g_weights) {
      if constexpr (DUMP && net_fields<M>::value > 0) {
        // a generated core with networks: nothing is added here -- the precision network's bias gradients are row sums of
        // its dump fields 0..7 like the networks' own (vihds/ops.py), so the whole weight gradient is the same bits run to run
      } else if constexpr (DUMP) {
        // only the biases are accumulated here; the weight matrices come from the dump (vihds_gram_blocks)
        VIHDS_UNROLL for (int q = 0; q < 8; ++q) {
          float v = live ? wtsb.bsum[q] : 0.f;
          VIHDS_UNROLL for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
          if ((threadIdx.x & 63) == 0)
            atomicAdd(&a.g_weights[M::W0 + (q < 4 ? M::o_bp(a.n_hidden_prec) + q : M::o_bd(a.n_hidden_prec) + (q - 4))], v);
        }
      } else if constexpr (ctx_has_wb<typename CtxImpl::type>::value) {
        if (a.n_hidden_prec < 1) {
          // shared-weight gradient: per-thread register accumulators -> wave shuffle tree -> one atomic per wave
          VIHDS_UNROLL for (int q = 0; q < M::NW; ++q) {
            float v = live ? wtsb.wb[q] : 0.f;
            VIHDS_UNROLL for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
            if ((threadIdx.x & 63) == 0) atomicAdd(&a.g_weights[M::W0 + q], v);
          }
        }
      }
    }
  }
}

inline int pick_block(int n) { return n >= (1 << 18) ? 256 : 64; }
// VIHDS_LANE_SPLIT_MAX_N (default 16 384): up to this many trajectories kernel_variant 0 means dr_constant's lane-split
// kernels, above it the thread-per-trajectory kernels (whose integration vihds_ode_fwd_summaries repeats)
inline long long lane_split_max_n() {
  static const long long v = [] {
    const char* e = std::getenv("VIHDS_LANE_SPLIT_MAX_N");
    return e ? std::atoll(e) : 16384LL;
  }();
  return v;
}

template <class M, int SOLVER>
inline void launch_fwd_s(const OdeArgs& a, hipStream_t st) {
  const int blk = pick_block(a.n);
  const int nb = min(a.B, (blk - 1) / a.S + 2);
  size_t lds = ((size_t)a.T + (size_t)nb * 4 * a.T) * sizeof(float);
  lds += (size_t)nb * n_forcings<M>::value * a.T * sizeof(float);  // (the rows' forcing samples behind the observations)
  lds += (size_t)nb * cond_mask_words<M>(a.T) * sizeof(float);     // (... and the mask words of a model with missing observations)
  if (lds <= 32 * 1024)
    hipLaunchKernelGGL((ode_fwd_kernel<M, SOLVER, true>), dim3((a.n + blk - 1) / blk), dim3(blk), lds, st, a);
  else
    hipLaunchKernelGGL((ode_fwd_kernel<M, SOLVER, false>), dim3((a.n + blk - 1) / blk), dim3(blk), 0, st, a);
}
template <class M, int SOLVER>
inline void launch_bwd_s(const OdeArgs& a, hipStream_t st) {
  const int blk = pick_block(a.n);
  if constexpr ((M::NEURAL_PREC || net_fields<M>::value > 0) && !is_blackbox<M>::value) {
    if (a.aux) {  // dump mode: the caller contracts the weight gradients (vihds_ode_bwd, include/vihds_hip.h)
      hipLaunchKernelGGL((ode_bwd_kernel<M, SOLVER, true>), dim3((a.n + blk - 1) / blk), dim3(blk), 0, st, a);
      return;
    }
  }
  hipLaunchKernelGGL((ode_bwd_kernel<M, SOLVER>), dim3((a.n + blk - 1) / blk), dim3(blk), 0, st, a);
}

// Request block of vihds_ode_adaptive_grid (LaunchMode::grid): the model's launcher runs the step-size controller instead
// of a forward / adjoint launch and leaves the grid length (or an error code) in `result`.
struct AdaptiveCtl {
  const float* times_host;
  float rtol, atol;
  float* workspace;
  float* grid_host;
  int max_grid;
  int* index_host;
  int result;
};
template <class M, int ONLY>
inline int adaptive_grid(int solver, const OdeArgs& a, const float* times_host, float rtol, float atol, float* workspace,
                         float* grid_host, int max_grid, int* index_host, hipStream_t st);

// -DVIHDS_ONLY_SOLVER=<id>: this translation unit holds the kernels of one solver only (the per-size dr_blackbox side
// libraries compile their eight solvers as eight objects in parallel: sized/ode_dr_blackbox_sized.hip)
// (ONLY is a template parameter of the dispatchers so that the eight objects hold eight DIFFERENT functions: the same
// inline function with different bodies would be folded into one by the linker)
#ifdef VIHDS_ONLY_SOLVER
constexpr int kOnlySolver = VIHDS_ONLY_SOLVER;
#else
constexpr int kOnlySolver = -1;
#endif
template <int ONLY>
constexpr bool solver_built_in(int sv) { return ONLY < 0 || sv == ONLY; }

}  // namespace vihds
#include "vihds_rk_adaptive_device.hpp"
namespace vihds {

template <class M, int ONLY>
inline int launch_ode_any(bool backward, int solver, const OdeArgs& a, hipStream_t st, const LaunchMode& mode);
// An implicit solver: its forward and adjoint kernels exist for a model with a generated Jacobian only -- every other
// launcher holds exactly the kernels it held without them and answers VIHDS_E_UNSUPPORTED.  The step-size controllers and the
// one-pass summaries are declined: an implicit step is taken on the observation grid.
template <class M, int ONLY>
inline int launch_ode_implicit(bool backward, int solver, const OdeArgs& a, hipStream_t st, const LaunchMode& mode) {
  if constexpr (has_jacobian<M>::value) {
    if (mode.summ || mode.dev || mode.grid) return VIHDS_E_UNSUPPORTED;
    if constexpr (solver_built_in<ONLY>(VIHDS_SOLVER_BEULER)) {
      if (solver == VIHDS_SOLVER_BEULER) {
        if (backward) launch_bwd_s<M, VIHDS_SOLVER_BEULER>(a, st);
        else launch_fwd_s<M, VIHDS_SOLVER_BEULER>(a, st);
        return VIHDS_OK;
      }
    }
    return VIHDS_E_BADARG;
  } else {
    return VIHDS_E_UNSUPPORTED;
  }
}
// the fixed-grid solvers a model with step control takes (vihds_stepctl.hpp): every one but the modeuler family
template <class M>
constexpr bool step_control_takes(int sv) {
  return !step_control<M>::value || (sv != VIHDS_SOLVER_MODEULER && sv != VIHDS_SOLVER_MODEULERWHILE);
}
template <class M, int ONLY = kOnlySolver>
inline int launch_ode(bool backward, int solver, const OdeArgs& a, hipStream_t st, const LaunchMode& mode) {
  if (solver_is_implicit(solver)) return launch_ode_implicit<M, ONLY>(backward, solver, a, st, mode);
  if constexpr (n_forcings<M>::value > 0 || substeps<M>::value > 1 || has_jump<M>::value || has_start<M>::value ||
                lead_in<M>::value > 0 || has_steady<M>::value > 0 || n_delays<M>::value > 0 || has_diffusion<M>::value || masked_obs<M>::value ||
                step_control<M>::value) {
    // a model with forcings: its samples live on the observation grid, so only the fixed-grid schemes integrate it -- the
    // adaptive pairs (either controller) and the one-pass summaries are declined here, and none of their kernels
    // (ode_trial_kernel, the device-resident solver, ode_fwd_summ_kernel) is instantiated for it.  A model with sub-steps
    // likewise: they divide the intervals of a fixed-grid scheme, an adaptive pair chooses its own steps.  A model with a state
    // jump likewise: the jump is applied between two intervals of the observation grid, which only these time loops walk.  A
    // model with a start map or a lead-in phase likewise: only these kernels call start and run the steps before t_0.  A model
    // with delayed reads likewise: its history is the trajectory these kernels store on the observation grid.  A model with
    // process noise likewise: its draws are counted by the steps of the observation grid (vihds_sde.hpp).  A model with missing
    // observations likewise: its mask words live on the observation grid (vihds_mask.hpp)
    if (mode.summ || mode.dev || mode.grid || solver_is_adaptive(solver)) return VIHDS_E_UNSUPPORTED;
    // (a model with step control: modeuler's fixed step is not the interval -- neither kernel of that family is instantiated)
    if constexpr (step_control<M>::value) {
      if (solver == VIHDS_SOLVER_MODEULER || solver == VIHDS_SOLVER_MODEULERWHILE) return VIHDS_E_UNSUPPORTED;
    }
#define VIHDS_CASE(SV)                                           \
  case SV:                                                       \
    if constexpr (solver_built_in<ONLY>(SV) && step_control_takes<M>(SV)) { \
      if (backward) launch_bwd_s<M, SV>(a, st);                  \
      else launch_fwd_s<M, SV>(a, st);                           \
      return VIHDS_OK;                                           \
    }                                                            \
    break;
    switch (solver) {
      VIHDS_CASE(VIHDS_SOLVER_MODEULER)
      VIHDS_CASE(VIHDS_SOLVER_MODEULERWHILE)
      VIHDS_CASE(VIHDS_SOLVER_EULER)
      VIHDS_CASE(VIHDS_SOLVER_MIDPOINT)
      VIHDS_CASE(VIHDS_SOLVER_RK4)
    }
#undef VIHDS_CASE
    return VIHDS_E_BADARG;
  } else {
    return launch_ode_any<M, ONLY>(backward, solver, a, st, mode);
  }
}
template <class M, int ONLY>
inline int launch_ode_any(bool backward, int solver, const OdeArgs& a, hipStream_t st, const LaunchMode& mode) {
  if (solver_is_implicit(solver)) return launch_ode_implicit<M, ONLY>(backward, solver, a, st, mode);
  if constexpr (net_fields<M>::value > 0 || M::OBS == OBS_CUSTOM || own_prec<M>::value || own_lik<M>::value) {
    // (a generated core with networks: neither family is instantiated -- their adjoints keep weight gradients in registers;
    // a model with an observation map of its own: the one-pass summaries know the fixed maps only; a model with a precision
    // map of its own: both families know the constant precisions and the precision states only; a model with a log density
    // of its own: both families form the Gaussian term)
    if (mode.summ || mode.dev) return VIHDS_E_UNSUPPORTED;
  } else {
    if (const SummArgs* sm = mode.summ) {  // vihds_ode_fwd_summaries: the evaluation's second forward pass
      return backward ? VIHDS_E_BADARG : launch_fwd_summ<M, ONLY>(solver, a, *sm, st);
    }
    if (AdaptiveDevCtl* dc = mode.dev) {  // vihds_ode_adaptive_fwd / _bwd: the device-resident controller and its adjoint
      dc->result = adaptive_device<M, ONLY>(solver, a, *dc, st);
      return dc->result;
    }
  }
  if (AdaptiveCtl* ctl = mode.grid) {
    ctl->result = adaptive_grid<M, ONLY>(solver, a, ctl->times_host, ctl->rtol, ctl->atol, ctl->workspace, ctl->grid_host,
                                   ctl->max_grid, ctl->index_host, st);
    return ctl->result < 0 ? ctl->result : VIHDS_OK;
  }
#define VIHDS_CASE(SV)                                           \
  case SV:                                                       \
    if constexpr (solver_built_in<ONLY>(SV)) {                            \
      if (backward) launch_bwd_s<M, SV>(a, st);                  \
      else launch_fwd_s<M, SV>(a, st);                           \
      return VIHDS_OK;                                           \
    }                                                            \
    break;
  switch (solver) {
    VIHDS_CASE(VIHDS_SOLVER_MODEULER)
    VIHDS_CASE(VIHDS_SOLVER_MODEULERWHILE)
    VIHDS_CASE(VIHDS_SOLVER_EULER)
    VIHDS_CASE(VIHDS_SOLVER_MIDPOINT)
    VIHDS_CASE(VIHDS_SOLVER_RK4)
    VIHDS_CASE(VIHDS_SOLVER_DOPRI5)
    VIHDS_CASE(VIHDS_SOLVER_BOSH3)
    VIHDS_CASE(VIHDS_SOLVER_ADAPTIVE_HEUN)
    VIHDS_CASE(VIHDS_SOLVER_DOPRI8)
  }
#undef VIHDS_CASE
  return VIHDS_E_BADARG;
}

// ---- step-size controller of the adaptive pairs (vihds_rk_adaptive.hpp) ---------------------------------------------
// State of the whole batch in a caller-provided workspace Y [N][n]; every launch writes one float per block to
// `partial` (sums of squares), which the host adds up in block order (deterministic).
// MODE 0: Y <- initial state; partial[0][blk] = sum (y0 / scale)^2, partial[1][blk] = sum (f0 / scale)^2   (scale = atol + rtol |y0|)
// MODE 1: partial[0][blk] = sum ((f(t + h, y0 + h f0) - f0) / scale)^2                                     (initial step)
// MODE 2: trial step of size h from Yin at t: Yout <- y', partial[0][blk] = sum (err / (atol + rtol max(|y|, |y'|)))^2
template <class M, int SOLVER, int MODE>
__global__ void __launch_bounds__(256) ode_trial_kernel(OdeArgs a, const float* Yin, float* Yout, float t, float h,
                                                        float rtol, float atol, float* partial) {
  constexpr int N = M::N;
  __shared__ float wlds[M::NW > 0 ? M::NW : 1];
  __shared__ float red[2][256];
  const float* wts = stage_weights<M>(a, wlds);
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  float s0 = 0.f, s1 = 0.f;
  if (i < a.n) {
    const int b = i / a.S;
    float th[M::NSLOT], prec[4], c[M::NC > 0 ? M::NC : 1], p[M::NP], y[N];
    load_theta<M>(a, i, b, th, prec, c);
    if constexpr (is_blackbox<M>::value) {
      M::prepare_bb(th, a, b, p);
      M::init_bb(th, a, y);
    } else {
      M::prepare(th, c, p);
      if constexpr (M::NEURAL_PREC) p[M::NP - 1] = __int_as_float(a.n_hidden_prec);
      M::init(th, c, y);
    }
    const size_t n = a.n;
    if (MODE == 0) {
      float f0[N];
      M::rhs(t, y, p, wts, f0);
      VIHDS_UNROLL for (int j = 0; j < N; ++j) {
        Yout[(size_t)j * n + i] = y[j];
        const float sc = atol + rtol * fabsf(y[j]);
        s0 += (y[j] / sc) * (y[j] / sc);
        s1 += (f0[j] / sc) * (f0[j] / sc);
      }
    } else if (MODE == 1) {
      float f0[N], f1[N], y1[N];
      M::rhs(t, y, p, wts, f0);
      VIHDS_UNROLL for (int j = 0; j < N; ++j) y1[j] = y[j] + h * f0[j];
      M::rhs(t + h, y1, p, wts, f1);
      VIHDS_UNROLL for (int j = 0; j < N; ++j) {
        const float sc = atol + rtol * fabsf(y[j]);
        const float d = (f1[j] - f0[j]) / sc;
        s0 += d * d;
      }
    } else {
      float err[N], y0[N];
      VIHDS_UNROLL for (int j = 0; j < N; ++j) { y[j] = Yin[(size_t)j * n + i]; y0[j] = y[j]; }
      rk_step_generic<M, Tableau<SOLVER>>(t, h, y, p, wts, err);
      VIHDS_UNROLL for (int j = 0; j < N; ++j) {
        Yout[(size_t)j * n + i] = y[j];
        const float tol = atol + rtol * fmaxf(fabsf(y0[j]), fabsf(y[j]));
        const float r = err[j] / tol;
        s0 += r * r;
      }
    }
  }
  red[0][threadIdx.x] = s0;
  red[1][threadIdx.x] = s1;
  __syncthreads();
  for (int w = blockDim.x / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      red[0][threadIdx.x] += red[0][threadIdx.x + w];
      red[1][threadIdx.x] += red[1][threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    partial[blockIdx.x] = red[0][0];
    partial[gridDim.x + blockIdx.x] = red[1][0];
  }
}

// Host-driven controller (synchronous on `st`).  Workspace: 2 N n floats of state + 2 blocks floats of partial sums.
// Returns the number of grid points written to grid_host (<= max_grid), or a negative error code.
template <class M, int SOLVER>
inline int adaptive_grid_s(const OdeArgs& a, const float* times_host, float rtol, float atol, float* workspace,
                           float* grid_host, int max_grid, int* index_host, hipStream_t st) {
  using TB = Tableau<SOLVER>;
  constexpr int N = M::N;
  const int blk = 256, nblk = (a.n + blk - 1) / blk;
  float* Y0 = workspace;
  float* Y1 = Y0 + (size_t)N * a.n;
  float* partial = Y1 + (size_t)N * a.n;
  std::vector<float> hp(2 * (size_t)nblk);
  auto sums = [&](double* s0, double* s1) -> bool {
    if (hipMemcpyAsync(hp.data(), partial, hp.size() * sizeof(float), hipMemcpyDeviceToHost, st) != hipSuccess) return false;
    if (hipStreamSynchronize(st) != hipSuccess) return false;
    double u = 0.0, v = 0.0;
    for (int q = 0; q < nblk; ++q) { u += hp[q]; v += hp[nblk + q]; }
    *s0 = u;
    if (s1) *s1 = v;
    return true;
  };
  const double cnt = (double)N * (double)a.n;
  const float t0 = times_host[0];
  // initial step (torchdiffeq 0.1 _select_initial_step) [recalled]
  double q0, q1, q2;
  hipLaunchKernelGGL((ode_trial_kernel<M, SOLVER, 0>), dim3(nblk), dim3(blk), 0, st, a, nullptr, Y0, t0, 0.f, rtol, atol, partial);
  if (!sums(&q0, &q1)) return VIHDS_E_HIP;
  const double d0 = std::sqrt(q0 / cnt), d1 = std::sqrt(q1 / cnt);
  double h0 = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * d0 / d1;
  hipLaunchKernelGGL((ode_trial_kernel<M, SOLVER, 1>), dim3(nblk), dim3(blk), 0, st, a, nullptr, Y0, t0, (float)h0, rtol, atol, partial);
  if (!sums(&q2, nullptr)) return VIHDS_E_HIP;
  const double d2 = std::sqrt(q2 / cnt) / h0;
  double h1 = (d1 <= 1e-15 && d2 <= 1e-15) ? std::max(1e-6, h0 * 1e-3) : std::pow(0.01 / std::max(d1, d2), 1.0 / (TB::ORDER + 1));
  double h = std::min(100.0 * h0, h1);
  // accepted steps, clipped to the output times
  int ng = 0;
  grid_host[ng++] = t0;
  index_host[0] = 0;
  float t = t0;
  for (int k = 1; k < a.T; ++k) {
    const float t_out = times_host[k];
    while (t < t_out) {
      if (ng >= max_grid) return VIHDS_E_UNSUPPORTED;
      const bool clip = t + (float)h >= t_out;
      const float t_next = clip ? t_out : t + (float)h;
      const float hs = t_next - t;
      if (!(hs > 0.f)) return VIHDS_E_BADARG;  // step size underflow
      hipLaunchKernelGGL((ode_trial_kernel<M, SOLVER, 2>), dim3(nblk), dim3(blk), 0, st, a, Y0, Y1, t, hs, rtol, atol, partial);
      double e2;
      if (!sums(&e2, nullptr)) return VIHDS_E_HIP;
      const double ratio = e2 / cnt;  // mean squared error ratio
      if (!(ratio == ratio)) return VIHDS_E_BADARG;
      const bool accept = ratio <= 1.0;
      // torchdiffeq 0.1 _optimal_step_size(last_step, mean_error_ratio, safety 0.9, ifactor 10, dfactor 0.2, order)
      double hn;
      if (ratio == 0.0) hn = (double)hs * 10.0;
      else {
        const double dfactor = ratio < 1.0 ? 1.0 : 0.2;
        const double er = std::sqrt(ratio);
        const double factor = std::max(1.0 / 10.0, std::min(std::pow(er, 1.0 / TB::ORDER) / 0.9, 1.0 / dfactor));
        hn = (double)hs / factor;
      }
      if (accept) {
        t = t_next;
        std::swap(Y0, Y1);
        grid_host[ng++] = t;
        // a clipped step says little about the step the controller wanted: keep the larger proposal
        h = clip ? std::max(h, hn) : hn;
      } else {
        h = hn;
      }
    }
    index_host[k] = ng - 1;
  }
  return ng;
}

template <class M, int ONLY>
inline int adaptive_grid(int solver, const OdeArgs& a, const float* times_host, float rtol, float atol, float* workspace,
                         float* grid_host, int max_grid, int* index_host, hipStream_t st) {
#define VIHDS_CASE(SV)       \
  case SV:                   \
    if constexpr (solver_built_in<ONLY>(SV)) return adaptive_grid_s<M, SV>(a, times_host, rtol, atol, workspace, grid_host, max_grid, index_host, st); \
    break;
  switch (solver) {
    VIHDS_CASE(VIHDS_SOLVER_DOPRI5)
    VIHDS_CASE(VIHDS_SOLVER_BOSH3)
    VIHDS_CASE(VIHDS_SOLVER_ADAPTIVE_HEUN)
    VIHDS_CASE(VIHDS_SOLVER_DOPRI8)
  }
#undef VIHDS_CASE
  return VIHDS_E_BADARG;
}

}  // namespace vihds
