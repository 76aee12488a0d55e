// Implicit fixed-grid schemes for generated models with a Jacobian (vihds/modelgen.py: implicit = True; vihds_models.hpp:
// has_jacobian<M>).  Solver VIHDS_SOLVER_BEULER is the implicit scheme of the model: backward Euler, or Alexander's two-stage
// SDIRK for a model generated with implicit_order = 2 (below, sdirk2_step).  Backward Euler, defined exactly -- with
// h = t1 - t0 and z = y_k, NEWTON times:
//     F = z - y_k - h f(t1, z);   A = I - h J(t1, z);   solve A d = -F;   z <- z + d
// then y_k+1 = z.  The count is fixed: no convergence test, no data-dependent branch.  The adjoint is the implicit-function
// theorem's at the stored y_k+1 (the exact derivative of the converged step; first derivatives only, no Newton in the
// backward pass):  A = I - h J(t1, y_k+1);  solve A^T mu = lambda;  lambda <- mu;  parameter adjoint += (h mu)^T df/dp.
//
// The linear solve is Gaussian elimination WITHOUT pivoting, fully unrolled, the matrix in registers.  A zero pivot gives
// inf or NaN, which travels to the non-finite-loss exit like any other blow-up.  The structural zeros of J are known when the
// model is generated (the struct's JAC_NZ, bit i N + j): the fill-in pattern of the elimination is worked out at compile
// time from it and every operation on a structural zero is left out.  (A literal 0.f in J does not do that by itself: under
// IEEE rules h * 0.f is not 0.f for every h, so the compiler keeps the arithmetic.)
//
// Everything here is a __host__ __device__ template on N and uses no HIP intrinsic: a stand-alone host program can run it
// (tests/test_modelgen_implicit_host.py compiles one with the address and undefined-behaviour sanitizers).
#pragma once
#include "../../include/vihds_hip.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VIHDS_HD __host__ __device__ __forceinline__
#else
#define VIHDS_HD inline
#endif
#if defined(__clang__)
#define VIHDS_IMPLICIT_UNROLL _Pragma("unroll")
#else
#define VIHDS_IMPLICIT_UNROLL
#endif

namespace vihds {

constexpr bool solver_is_implicit(int solver) { return solver == VIHDS_SOLVER_BEULER; }
// the states an implicit generated model may have (the matrix lives in registers; vihds.modelgen.MAX_IMPLICIT_STATES): the
// 64 bits of JAC_NZ
constexpr int kMaxImplicitStates = 8;

// which entries of A = I - h J (TRANSPOSE: of its transpose) are not structurally zero once the elimination has run: the
// diagonal, J's pattern, and the fill-in of every elimination step
template <int N>
struct SolvePattern {
  bool nz[N * N];
};
template <int N>
constexpr SolvePattern<N> solve_pattern(unsigned long long jac_nz, bool transpose) {
  SolvePattern<N> p{};
  for (int i = 0; i < N; ++i)
    for (int j = 0; j < N; ++j) {
      const int bit = transpose ? j * N + i : i * N + j;
      p.nz[i * N + j] = i == j || ((jac_nz >> bit) & 1ull) != 0;
    }
  for (int k = 0; k < N; ++k)
    for (int i = k + 1; i < N; ++i)
      if (p.nz[i * N + k])
        for (int j = k + 1; j < N; ++j)
          if (p.nz[k * N + j]) p.nz[i * N + j] = true;
  return p;
}
constexpr unsigned long long dense_pattern(int n) { return n * n >= 64 ? ~0ull : (1ull << (n * n)) - 1ull; }

// b <- A^-1 b (TRANSPOSE: A^-T b) for A = I - h J, J row-major [N][N] with the structural pattern JAC_NZ.  Elimination
// without pivoting; the reciprocal of each pivot is taken once.  Every multiply-subtract is written as a fused one
// (__builtin_fmaf, a compiler builtin on the host and the device): A's entries and the updates are rounded once, and a host
// build computes bit for bit what the kernels do whatever its contraction flags are.
template <int N, unsigned long long JAC_NZ, bool TRANSPOSE>
VIHDS_HD void implicit_solve(float h, const float* J, float* b) {
  static_assert(N >= 1 && N <= kMaxImplicitStates, "the pattern is 64 bits: at most 8 states");
  constexpr SolvePattern<N> P = solve_pattern<N>(JAC_NZ, TRANSPOSE);
  float a[N * N], rinv[N];
  VIHDS_IMPLICIT_UNROLL for (int i = 0; i < N; ++i) {
    VIHDS_IMPLICIT_UNROLL for (int j = 0; j < N; ++j) {
      const float d = i == j ? 1.f : 0.f;
      const bool in_j = ((JAC_NZ >> (TRANSPOSE ? j * N + i : i * N + j)) & 1ull) != 0;
      a[i * N + j] = in_j ? __builtin_fmaf(-h, TRANSPOSE ? J[j * N + i] : J[i * N + j], d) : d;
    }
  }
  VIHDS_IMPLICIT_UNROLL for (int k = 0; k < N; ++k) {
    rinv[k] = 1.f / a[k * N + k];
    VIHDS_IMPLICIT_UNROLL for (int i = k + 1; i < N; ++i) {
      if (P.nz[i * N + k]) {
        const float m = a[i * N + k] * rinv[k];
        VIHDS_IMPLICIT_UNROLL for (int j = k + 1; j < N; ++j) {
          if (P.nz[k * N + j]) a[i * N + j] = __builtin_fmaf(-m, a[k * N + j], a[i * N + j]);
        }
        b[i] = __builtin_fmaf(-m, b[k], b[i]);
      }
    }
  }
  VIHDS_IMPLICIT_UNROLL for (int i = N - 1; i >= 0; --i) {
    float s = b[i];
    VIHDS_IMPLICIT_UNROLL for (int j = i + 1; j < N; ++j) {
      if (P.nz[i * N + j]) s = __builtin_fmaf(-a[i * N + j], b[j], s);
    }
    b[i] = s * rinv[i];
  }
}

// One backward-Euler step y (= y_k) -> y_k+1 over h.  f(z, out[N]) is the right-hand side at t1, jac(z, J[N N]) its
// Jacobian there, J[i N + j] = d f_i / d z_j.
template <int N, int NEWTON, unsigned long long JAC_NZ, class F, class JF>
VIHDS_HD void beuler_step(float h, float* y, F&& f, JF&& jac) {
  static_assert(NEWTON >= 1, "at least one Newton iteration");
  float z[N];
  VIHDS_IMPLICIT_UNROLL for (int j = 0; j < N; ++j) z[j] = y[j];
  for (int it = 0; it < NEWTON; ++it) {
    float fz[N], J[N * N], d[N];
    f(z, fz);
    jac(z, J);
    VIHDS_IMPLICIT_UNROLL for (int j = 0; j < N; ++j) d[j] = __builtin_fmaf(h, fz[j], y[j] - z[j]);  // -F
    implicit_solve<N, JAC_NZ, false>(h, J, d);
    VIHDS_IMPLICIT_UNROLL for (int j = 0; j < N; ++j) z[j] += d[j];
  }
  VIHDS_IMPLICIT_UNROLL for (int j = 0; j < N; ++j) y[j] = z[j];
}

// The step's adjoint at the stored y_k+1: lam (adjoint of y_k+1) <- adjoint of y_k = A^-T lam.  The caller then adds the
// parameter adjoint with one vector-Jacobian product of f at (t1, y_k+1) seeded with h * lam.
template <int N, unsigned long long JAC_NZ, class JF>
VIHDS_HD void beuler_step_vjp(float h, const float* y_next, float* lam, JF&& jac) {
  float J[N * N];
  jac(y_next, J);
  implicit_solve<N, JAC_NZ, true>(h, J, lam);
}

// ---- Alexander's two-stage SDIRK (implicit_order = 2: order 2, L-stable, stiffly accurate) ------------------------------------
// gamma = 1 - sqrt(2)/2 and c = 1 + sqrt(2) = (1 - gamma) / gamma, each the nearest float.  With h = t1 - t0, a = gamma h and
// tg = fmaf(gamma, h, t0):
//     stage 1   z = y_k;  NEWTON times  F = z - y_k - a f(tg, z);  A = I - a J(tg, z);  solve A d = -F;  z <- z + d   -> z1
//     base      w = fmaf(c, z1 - y_k, y_k)      (= y_k + (1 - gamma) h f(tg, z1) without evaluating a stiff f again)
//     stage 2   z = z1;   NEWTON times  F = z - w - a f(t1, z);     A = I - a J(t1, z);   solve A d = -F;  z <- z + d   -> y_k+1
// The count is fixed as for backward Euler.  The adjoint is the converged step's (first derivatives, no Newton iteration on the
// adjoint): with z1 recomputed by the forward's stage-1 call,  A2 = I - a J(t1, y_k+1), A2^T mu2 = lambda;
// A1 = I - a J(tg, z1), A1^T mu1 = c mu2;  parameter adjoint += (a mu2)^T df/dp at (t1, y_k+1) + (a mu1)^T df/dp at (tg, z1);
// lambda <- (1 - c) mu2 + mu1.
constexpr float kSdirk2Gamma = 0.29289323f;
constexpr float kSdirk2C = 2.4142137f;

// NEWTON iterations of z = base + a f(z) from z (= the start on entry, the stage value on return).  f(z, out[N]) and
// jac(z, J[N N]) are the right-hand side and its Jacobian at the stage's time.
template <int N, int NEWTON, unsigned long long JAC_NZ, class F, class JF>
VIHDS_HD void sdirk_stage(float a, const float* base, float* z, F&& f, JF&& jac) {
  static_assert(NEWTON >= 1, "at least one Newton iteration");
  for (int it = 0; it < NEWTON; ++it) {
    float fz[N], J[N * N], d[N];
    f(z, fz);
    jac(z, J);
    VIHDS_IMPLICIT_UNROLL for (int j = 0; j < N; ++j) d[j] = __builtin_fmaf(a, fz[j], base[j] - z[j]);  // -F
    implicit_solve<N, JAC_NZ, false>(a, J, d);
    VIHDS_IMPLICIT_UNROLL for (int j = 0; j < N; ++j) z[j] += d[j];
  }
}

// the stage-1 value z1 of the step from y over [t0, t0 + h]; f(t, z, out) and jac(t, z, J) take the stage time
template <int N, int NEWTON, unsigned long long JAC_NZ, class F, class JF>
VIHDS_HD void sdirk2_stage1(float t0, float h, const float* y, float* z1, F&& f, JF&& jac) {
  const float a = kSdirk2Gamma * h;
  const float tg = __builtin_fmaf(kSdirk2Gamma, h, t0);
  VIHDS_IMPLICIT_UNROLL for (int j = 0; j < N; ++j) z1[j] = y[j];
  sdirk_stage<N, NEWTON, JAC_NZ>(
      a, y, z1, [&](const float* z, float* fz) { f(tg, z, fz); }, [&](const float* z, float* J) { jac(tg, z, J); });
}

// One step y (= y_k) -> y_k+1 from t0 to t1.
template <int N, int NEWTON, unsigned long long JAC_NZ, class F, class JF>
VIHDS_HD void sdirk2_step(float t0, float t1, float* y, F&& f, JF&& jac) {
  const float h = t1 - t0;
  const float a = kSdirk2Gamma * h;
  float z[N], w[N];
  sdirk2_stage1<N, NEWTON, JAC_NZ>(t0, h, y, z, f, jac);
  VIHDS_IMPLICIT_UNROLL for (int j = 0; j < N; ++j) w[j] = __builtin_fmaf(kSdirk2C, z[j] - y[j], y[j]);
  sdirk_stage<N, NEWTON, JAC_NZ>(
      a, w, z, [&](const float* u, float* fz) { f(t1, u, fz); }, [&](const float* u, float* J) { jac(t1, u, J); });
  VIHDS_IMPLICIT_UNROLL for (int j = 0; j < N; ++j) y[j] = z[j];
}

// The step's adjoint at the start state y (= y_k) and the stored y_next (= y_k+1): lam (adjoint of y_k+1) <- adjoint of y_k.
// z1 (the recomputed stage value), mu1 and mu2 are returned for the caller's two parameter products: rhs_vjp at (t1, y_next)
// seeded with a mu2 and at (tg, z1) seeded with a mu1.
template <int N, int NEWTON, unsigned long long JAC_NZ, class F, class JF>
VIHDS_HD void sdirk2_step_vjp(float t0, float t1, const float* y, const float* y_next, float* lam, float* z1, float* mu1,
                              float* mu2, F&& f, JF&& jac) {
  const float h = t1 - t0;
  const float a = kSdirk2Gamma * h;
  const float tg = __builtin_fmaf(kSdirk2Gamma, h, t0);
  sdirk2_stage1<N, NEWTON, JAC_NZ>(t0, h, y, z1, f, jac);
  {
    float J[N * N];
    jac(t1, y_next, J);
    VIHDS_IMPLICIT_UNROLL for (int j = 0; j < N; ++j) mu2[j] = lam[j];
    implicit_solve<N, JAC_NZ, true>(a, J, mu2);
  }
  {
    float J[N * N];
    jac(tg, z1, J);
    VIHDS_IMPLICIT_UNROLL for (int j = 0; j < N; ++j) mu1[j] = kSdirk2C * mu2[j];
    implicit_solve<N, JAC_NZ, true>(a, J, mu1);
  }
  VIHDS_IMPLICIT_UNROLL for (int j = 0; j < N; ++j) lam[j] = __builtin_fmaf(1.f - kSdirk2C, mu2[j], mu1[j]);
}

}  // namespace vihds
