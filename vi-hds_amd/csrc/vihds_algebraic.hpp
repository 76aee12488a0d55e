// Algebraic variables of generated models (vihds/modelgen.py: `algebraic`, `constraint`, `algebraic_start`): a fast reaction
// held at its equilibrium.  The model keeps the totals as ODE states y and defines M <= 4 unknowns z by a constraint
// g(y, z, p) = 0 (a semi-explicit index-1 DAE).  The closure lives inside the generated struct: its rhs and its observe open
// with the solve, so every explicit scheme of vihds_ode_kernels.hpp runs such a model unchanged.  The value, defined exactly:
//     z = algebraic_start(y, p);   ALG_ITER times:  G = g(y, z, p);  A = dg/dz (y, z, p);  solve A d = -G;  z <- z + d
// then rhs / observe are evaluated with that z.  The count is fixed: no convergence test, no data-dependent branch.  The adjoint
// repeats the value pass (the same iteration, so forward and adjoint see the same bits), takes zb = the adjoint of z from reverse
// mode over rhs / observe, and with A at the final z solves A^T mu = zb; then yb -= (dg/dy)^T mu and pb -= (dg/dp)^T mu, which
// is one vector-Jacobian product of the constraint seeded with -mu.  That is the implicit-function derivative of the converged
// solution: nothing is differentiated through the iteration or through algebraic_start, and no Newton iteration runs on the
// adjoint.  Too few iterations leave a z that is not the root, and the adjoint is then not the gradient of what was computed.
//
// The linear solve is Gaussian elimination WITHOUT pivoting, fully unrolled, the matrix in registers (vihds_implicit.hpp does
// the same for I - h J).  A zero pivot gives inf or NaN, which travels to the non-finite-loss exit like any other blow-up.  The
// structural non-zeros of dg/dz are known when the model is generated (the struct's ALG_NZ, bit i M + j): the fill-in of the
// elimination is worked out at compile time from it and every operation on a structural zero is left out.
//
// Everything here is a __host__ __device__ template and uses no HIP intrinsic; every multiply-subtract is a fused one
// (__builtin_fmaf), so a host build computes the kernels' bits (tests/test_modelgen_algebraic_host.py runs a stand-alone host
// program under the address and undefined-behaviour sanitizers).
#pragma once

#ifndef VIHDS_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define VIHDS_HD __host__ __device__ __forceinline__
#else
#define VIHDS_HD inline
#endif
#endif
#if defined(__clang__)
#define VIHDS_ALGEBRAIC_UNROLL _Pragma("unroll")
#else
#define VIHDS_ALGEBRAIC_UNROLL
#endif

namespace vihds {

// the unknowns a generated model may have (vihds.modelgen.MAX_ALGEBRAIC): the matrix lives in registers beside the states
constexpr int kMaxAlgebraic = 4;

// which entries of A (TRANSPOSE: of its transpose) are not structurally zero once the elimination has run: A's own pattern
// and the fill-in of every elimination step
template <int M>
struct DensePattern {
  bool nz[M * M];
};
template <int M>
constexpr DensePattern<M> dense_solve_pattern(unsigned nz, bool transpose) {
  DensePattern<M> p{};
  for (int i = 0; i < M; ++i)
    for (int j = 0; j < M; ++j) p.nz[i * M + j] = ((nz >> (transpose ? j * M + i : i * M + j)) & 1u) != 0;
  for (int k = 0; k < M; ++k)
    for (int i = k + 1; i < M; ++i)
      if (p.nz[i * M + k])
        for (int j = k + 1; j < M; ++j)
          if (p.nz[k * M + j]) p.nz[i * M + j] = true;
  return p;
}
template <int M>
constexpr bool dense_pivots_present(unsigned nz) {
  const DensePattern<M> p = dense_solve_pattern<M>(nz, false);
  for (int k = 0; k < M; ++k)
    if (!p.nz[k * M + k]) return false;
  return true;
}
constexpr unsigned dense_algebraic_pattern(int m) { return (1u << (m * m)) - 1u; }

// b <- A^-1 b (TRANSPOSE: A^-T b) for A row-major [M][M] with the structural pattern NZ (bit i M + j; an entry outside it is
// not read).  Elimination without pivoting; the reciprocal of each pivot is taken once.
template <int M, unsigned NZ, bool TRANSPOSE>
VIHDS_HD void dense_solve(const float* A, float* b) {
  static_assert(M >= 1 && M <= kMaxAlgebraic, "at most 4 unknowns: the pattern is 16 bits, the matrix lives in registers");
  static_assert(dense_pivots_present<M>(NZ), "a pivot of the elimination is structurally zero: reorder unknowns or residuals");
  constexpr DensePattern<M> P = dense_solve_pattern<M>(NZ, TRANSPOSE);
  float a[M * M], rinv[M];
  VIHDS_ALGEBRAIC_UNROLL for (int i = 0; i < M; ++i) {
    VIHDS_ALGEBRAIC_UNROLL for (int j = 0; j < M; ++j) {
      const int src = TRANSPOSE ? j * M + i : i * M + j;
      a[i * M + j] = ((NZ >> src) & 1u) != 0 ? A[src] : 0.f;
    }
  }
  VIHDS_ALGEBRAIC_UNROLL for (int k = 0; k < M; ++k) {
    rinv[k] = 1.f / a[k * M + k];
    VIHDS_ALGEBRAIC_UNROLL for (int i = k + 1; i < M; ++i) {
      if (P.nz[i * M + k]) {
        const float m = a[i * M + k] * rinv[k];
        VIHDS_ALGEBRAIC_UNROLL for (int j = k + 1; j < M; ++j) {
          if (P.nz[k * M + j]) a[i * M + j] = __builtin_fmaf(-m, a[k * M + j], a[i * M + j]);
        }
        b[i] = __builtin_fmaf(-m, b[k], b[i]);
      }
    }
  }
  VIHDS_ALGEBRAIC_UNROLL for (int i = M - 1; i >= 0; --i) {
    float s = b[i];
    VIHDS_ALGEBRAIC_UNROLL for (int j = i + 1; j < M; ++j) {
      if (P.nz[i * M + j]) s = __builtin_fmaf(-a[i * M + j], b[j], s);
    }
    b[i] = s * rinv[i];
  }
}

// ITER Newton iterations of g(z) = 0 from z (the start on entry, the solution on return).  g(z, G[M]) is the constraint and
// jac(z, A[M M]) its Jacobian, A[i M + j] = d g_i / d z_j (entries outside NZ need not be written).
template <int M, int ITER, unsigned NZ, class GF, class JF>
VIHDS_HD void algebraic_newton(float* z, GF&& g, JF&& jac) {
  static_assert(ITER >= 1, "at least one Newton iteration");
  for (int it = 0; it < ITER; ++it) {
    float d[M], A[M * M];
    g(z, d);
    jac(z, A);
    VIHDS_ALGEBRAIC_UNROLL for (int i = 0; i < M; ++i) d[i] = -d[i];
    dense_solve<M, NZ, false>(A, d);
    VIHDS_ALGEBRAIC_UNROLL for (int i = 0; i < M; ++i) z[i] += d[i];
  }
}

// The adjoint's solve at the final z: zb (the adjoint of z) <- -mu with A^T mu = zb.  The caller then adds the constraint's
// vector-Jacobian product seeded with it into the adjoints of y and p.
template <int M, unsigned NZ, class JF>
VIHDS_HD void algebraic_adjoint(float* zb, JF&& jac) {
  float A[M * M];
  jac(A);
  dense_solve<M, NZ, true>(A, zb);
  VIHDS_ALGEBRAIC_UNROLL for (int i = 0; i < M; ++i) zb[i] = -zb[i];
}

}  // namespace vihds
