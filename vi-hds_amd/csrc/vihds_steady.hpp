// Pre-equilibration of generated models (vihds/modelgen.py: `steady_species`, `steady_rate`): the trajectory starts at a steady
// state of the model itself under the pre-culture conditions.  M <= 8 of the species, E, are solved for; the others are inputs
// held fixed.  With F(y, p) = steady_rate (d y_E / dt before t_0) and J = dF / dy_E, the value, defined exactly -- from the guess
// y (what init, then start returned), with delta_0 = STEADY_DELTA0 and for k = 0 .. STEPS - 1:
//     solve (I - delta_k J(y)) d = delta_k F(y);   y_E <- y_E + d;   delta_k+1 = delta_k * STEADY_GROWTH        (all float32)
// Each iteration is one Newton iteration of a backward-Euler step in pseudo-time (pseudo-transient continuation): while delta is
// small the iterate follows the flow from the guess, so a bistable model lands in the basin its guess is in; once delta is large
// the iteration is Newton's on F = 0, up to 1 / delta.  The count is fixed: no convergence test, no data-dependent branch.
//
// The adjoint is the implicit-function theorem's at the final state y*: with lam the adjoint of y*, solve J(y*)^T mu = lam_E --
// a plain solve with J, not with I - delta J --, add the vector-Jacobian product of F seeded with -mu into the adjoints of the
// other species and of p, and set lam_E = 0.  Nothing is differentiated through the iteration: the guess of a steady species
// receives exactly 0.  Too few steps leave a y* that is not a root, and the adjoint is then not the gradient of what was computed.
//
// The forward solve is implicit_solve of vihds_implicit.hpp (A = I - delta J on J's 64-bit pattern).  The adjoint's solve is
// steady_solve_t below: Gaussian elimination WITHOUT pivoting on J^T itself, fully unrolled, the matrix in registers, the
// fill-in worked out at compile time from the structural pattern (STEADY_NZ, bit i M + j) and every operation on a structural
// zero left out; a structurally zero pivot does not compile.  A pivot that vanishes numerically gives inf or NaN, which travels
// to the non-finite-loss exit like any other blow-up.
//
// Everything here is a __host__ __device__ template and uses no HIP intrinsic; every multiply-subtract is a fused one
// (__builtin_fmaf), so a host build computes the kernels' bits (tests/test_modelgen_steady_host.py runs a stand-alone host
// program under the address and undefined-behaviour sanitizers).
#pragma once
#include "vihds_implicit.hpp"

#if defined(__clang__)
#define VIHDS_STEADY_UNROLL _Pragma("unroll")
#define VIHDS_STEADY_LOOP _Pragma("nounroll")
#else
#define VIHDS_STEADY_UNROLL
#define VIHDS_STEADY_LOOP
#endif

namespace vihds {

// the species a generated model may solve for (vihds.modelgen.MAX_STEADY): the matrix lives in registers beside the states, its
// pattern is one 64-bit constant; and the iterations it may ask for (vihds.modelgen.MAX_STEADY_STEPS)
constexpr int kMaxSteady = 8;
constexpr int kMaxSteadySteps = 16;
static_assert(kMaxSteady <= kMaxImplicitStates, "the forward solve is implicit_solve");

// which entries of J^T are not structurally zero once the elimination has run: its own pattern and the fill-in of every step
template <int M>
constexpr SolvePattern<M> steady_pattern_t(unsigned long long nz) {
  SolvePattern<M> p{};
  for (int i = 0; i < M; ++i)
    for (int j = 0; j < M; ++j) p.nz[i * M + j] = ((nz >> (j * M + i)) & 1ull) != 0;
  for (int k = 0; k < M; ++k)
    for (int i = k + 1; i < M; ++i)
      if (p.nz[i * M + k])
        for (int j = k + 1; j < M; ++j)
          if (p.nz[k * M + j]) p.nz[i * M + j] = true;
  return p;
}
template <int M>
constexpr bool steady_pivots_present(unsigned long long nz) {
  const SolvePattern<M> p = steady_pattern_t<M>(nz);
  for (int k = 0; k < M; ++k)
    if (!p.nz[k * M + k]) return false;
  return true;
}

// b <- J^-T b for J row-major [M][M] with the structural pattern NZ (an entry outside it is not read).  Elimination without
// pivoting; the reciprocal of each pivot is taken once.
template <int M, unsigned long long NZ>
VIHDS_HD void steady_solve_t(const float* J, float* b) {
  static_assert(M >= 1 && M <= kMaxSteady, "at most 8 steady species: the pattern is 64 bits, the matrix lives in registers");
  static_assert(steady_pivots_present<M>(NZ), "a pivot of the elimination is structurally zero: reorder steady_species or the residuals");
  constexpr SolvePattern<M> P = steady_pattern_t<M>(NZ);
  float a[M * M], rinv[M];
  VIHDS_STEADY_UNROLL for (int i = 0; i < M; ++i) {
    VIHDS_STEADY_UNROLL for (int j = 0; j < M; ++j) {
      a[i * M + j] = ((NZ >> (j * M + i)) & 1ull) != 0 ? J[j * M + i] : 0.f;
    }
  }
  VIHDS_STEADY_UNROLL for (int k = 0; k < M; ++k) {
    rinv[k] = 1.f / a[k * M + k];
    VIHDS_STEADY_UNROLL for (int i = k + 1; i < M; ++i) {
      if (P.nz[i * M + k]) {
        const float m = a[i * M + k] * rinv[k];
        VIHDS_STEADY_UNROLL for (int j = k + 1; j < M; ++j) {
          if (P.nz[k * M + j]) a[i * M + j] = __builtin_fmaf(-m, a[k * M + j], a[i * M + j]);
        }
        b[i] = __builtin_fmaf(-m, b[k], b[i]);
      }
    }
  }
  VIHDS_STEADY_UNROLL for (int i = M - 1; i >= 0; --i) {
    float s = b[i];
    VIHDS_STEADY_UNROLL for (int j = i + 1; j < M; ++j) {
      if (P.nz[i * M + j]) s = __builtin_fmaf(-a[i * M + j], b[j], s);
    }
    b[i] = s * rinv[i];
  }
}

// STEPS iterations from z (the guess of the steady species on entry, the solution on return).  f(z, F[M]) is steady_rate with the
// other species held and jac(z, J[M M]) its Jacobian, J[i M + j] = d F_i / d z_j (entries outside NZ need not be written).  The
// loop is kept a loop: it runs once per trajectory, and STEPS copies of an 8 x 8 elimination would only cost instruction cache.
template <int M, int STEPS, unsigned long long NZ, class F, class JF>
VIHDS_HD void steady_iterate(float delta0, float growth, float* z, F&& f, JF&& jac) {
  static_assert(STEPS >= 1 && STEPS <= kMaxSteadySteps, "steady_steps: 1 .. 16");
  float delta = delta0;
  VIHDS_STEADY_LOOP for (int k = 0; k < STEPS; ++k) {
    float d[M], J[M * M];
    f(z, d);
    jac(z, J);
    VIHDS_STEADY_UNROLL for (int i = 0; i < M; ++i) d[i] = delta * d[i];
    implicit_solve<M, NZ, false>(delta, J, d);
    VIHDS_STEADY_UNROLL for (int i = 0; i < M; ++i) z[i] += d[i];
    delta = delta * growth;
  }
}

// The adjoint's solve at the final state: mu (lam_E on entry) <- -J^-T lam_E.  The caller then adds steady_rate's
// vector-Jacobian product seeded with it into the adjoints of the other species and of p, and clears lam_E.
template <int M, unsigned long long NZ, class JF>
VIHDS_HD void steady_adjoint(float* mu, JF&& jac) {
  float J[M * M];
  jac(J);
  steady_solve_t<M, NZ>(J, mu);
  VIHDS_STEADY_UNROLL for (int i = 0; i < M; ++i) mu[i] = -mu[i];
}

}  // namespace vihds
