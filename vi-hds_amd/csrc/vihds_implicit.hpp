// Implicit fixed-grid schemes for generated models with a Jacobian (vihds/modelgen.py: implicit = True; vihds_models.hpp:
// has_jacobian<M>).  One scheme: backward Euler (VIHDS_SOLVER_BEULER), defined exactly -- with h = t1 - t0 and z = y_k,
// NEWTON times:
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

}  // namespace vihds
