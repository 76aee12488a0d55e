// Delayed state reads of generated models (vihds/modelgen.py: delays = {name: (species, effective parameter)}; vihds_models.hpp:
// n_delays<M>).  The right-hand side reads y_i(t - tau) from the trajectory the forward kernel itself stored at the earlier
// observation points.  The value, defined exactly, per observation interval k = [t_k, t_k+1] and per read, taue = fmaxf(tau, 0):
//     s_lo = t_k - taue,   s_hi = fminf(t_k+1 - taue, t_k)          (the history is known up to the start of the step only)
//     H(s) = y_0                                     for s <= t_0   (a constant history: the stored state at t_0)
//     H(s) = fmaf(w, y_j+1 - y_j, y_j),  w = (s - t_j) / (t_j+1 - t_j),  j the largest index of [0, k-1] with t_j <= s
//     d_lo = H(s_lo),  d_hi = H(s_hi);  every stage of the step reads the chord d_lo + (t - t_k) (d_hi - d_lo) / (t_k+1 - t_k)
// y_* are the float32 values of the trajectory buffer.  The index j is clamped into [0, k-1] before any load whatever tau is;
// a delay that is not finite (NaN, +-inf) makes the value NaN, which travels to the non-finite-loss exit like any blow-up --
// it never becomes an address.  The searches are cursor walks bounded by k: s_lo grows with k along a trajectory, so the
// forward's cursor only climbs and the adjoint's only descends, and s_hi is searched upwards from s_lo's index.
//
// The adjoint is the exact derivative of that map (first derivatives only, no atomics): with g the adjoint of H(s),
//     s <= t_0:  A[0] += g;     otherwise  A[j] += (1 - w) g,  A[j+1] += w g,
//     taue's adjoint += -(y_j+1 - y_j) / (t_j+1 - t_j) g   where s > t_0 and s was not clamped to t_k
// A is the thread's own column of the history adjoint.
//
// Everything here is a __host__ __device__ template and uses no HIP intrinsic; every multiply-add is __builtin_fmaf: a
// stand-alone host program can run it (tests/test_modelgen_delay_host.py compiles one with the address and
// undefined-behaviour sanitizers).  TimeAt / YAt / AAt are callables: time_at(j) -> t_j, y_at(j) -> y_j of the read's species,
// a_at(j) -> a reference to A[j].
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VIHDS_DELAY_HD __host__ __device__ __forceinline__
#else
#define VIHDS_DELAY_HD inline
#endif

namespace vihds {

// one lookup H(s): where it landed and what the adjoint needs of it
struct DelayHit {
  float value;  // H(s) (NaN for a delay that is not finite)
  float w;      // the interpolation weight (0 where past)
  float slope;  // (y_j+1 - y_j) / (t_j+1 - t_j) (0 where past)
  int j;        // the interval of the history, in [0, max(k - 1, 0)]
  bool past;    // s <= t_0 (or s not a number): the constant history
};

VIHDS_DELAY_HD float delay_effective(float tau) { return __builtin_fmaxf(tau, 0.f); }
VIHDS_DELAY_HD bool delay_finite(float tau) { return __builtin_fabsf(tau) <= 3.402823466e+38f; }  // (false for NaN)

// the largest index of [0, k - 1] with t_j <= s (0 where there is none, or k == 0), climbing from a cursor that is the answer
// of a smaller s and a smaller k.  At most k comparisons; a NaN s moves nothing
template <class TimeAt>
VIHDS_DELAY_HD int delay_seek_up(TimeAt time_at, int j, int k, float s) {
  j = j < 0 ? 0 : j;
  while (j + 1 < k && time_at(j + 1) <= s) ++j;
  return j < k - 1 ? j : (k > 0 ? k - 1 : 0);
}
// ... descending from a cursor that is the answer of a larger s (and a larger k)
template <class TimeAt>
VIHDS_DELAY_HD int delay_seek_down(TimeAt time_at, int j, int k, float s) {
  j = j > k - 1 ? k - 1 : j;
  j = j < 0 ? 0 : j;
  while (j > 0 && time_at(j) > s) --j;
  return j;
}

// H(s) for the interval index j the seeks returned (j + 1 <= k is only loaded where s > t_0, which needs k >= 1)
template <class TimeAt, class YAt>
VIHDS_DELAY_HD DelayHit delay_lookup(TimeAt time_at, YAt y_at, int j, float s, float t0, float y0, float tau) {
  DelayHit h;
  h.j = j;
  h.past = !(s > t0);
  h.w = 0.f;
  h.slope = 0.f;
  h.value = y0;
  if (!h.past) {
    const float tj = time_at(j), dt = time_at(j + 1) - tj;
    const float yj = y_at(j), dy = y_at(j + 1) - yj;
    h.w = (s - tj) / dt;
    h.slope = dy / dt;
    h.value = __builtin_fmaf(h.w, dy, yj);
  }
  if (!delay_finite(tau)) h.value = tau - tau;  // (inf - inf and NaN - NaN: NaN)
  return h;
}

// the adjoint g of one lookup into the history adjoint; returns its part of the adjoint of taue (`moves`: s follows taue --
// false for an s_hi that was clamped to t_k)
template <class AAt>
VIHDS_DELAY_HD float delay_scatter(AAt a_at, const DelayHit& h, float g, bool moves) {
  if (h.past) {
    a_at(0) += g;
    return 0.f;
  }
  a_at(h.j) += __builtin_fmaf(-h.w, g, g);
  a_at(h.j + 1) += h.w * g;
  return moves ? -h.slope * g : 0.f;
}

// the two ends of interval k: s_lo = t_k - taue and s_hi = fminf(t_k+1 - taue, t_k); `clamped` says which s_hi is
struct DelayEnds {
  float s_lo, s_hi;
  bool clamped;
};
VIHDS_DELAY_HD DelayEnds delay_ends(float t_k, float t_k1, float tau) {
  const float taue = delay_effective(tau);
  DelayEnds e;
  e.s_lo = t_k - taue;
  const float s = t_k1 - taue;
  e.clamped = !(s < t_k);
  e.s_hi = e.clamped ? t_k : s;
  return e;
}

}  // namespace vihds
