// Process noise for generated models (vihds/modelgen.py: diffusion(self, y, p, c); vihds_models.hpp: has_diffusion<M>).
// Diagonal Ito noise, one independent Wiener process per species.  Every step a fixed-grid scheme takes -- every sub-step of a
// model with substeps > 1 -- from the state u over a step of length h becomes
//     u' = Phi_h(u) + g(u, p) * (sqrt(h) * xi),        xi ~ N(0, 1) per species,
// Phi the unchanged step of the scheme (ode_step), g the model's diffusion at the step's START state, h the length the scheme
// itself advances by: modeuler's fixed step as ode_step uses it, t1 - t0 for every other solver.  Euler-Maruyama for euler; a
// drift / noise splitting of the same strong order 1/2 for the others.
//
// The draws are stored nowhere.  xi of species q at step `step` of trajectory `traj` under the row's key (k0, k1) is normal
// q & 3 of philox_normal4 (vihds_rng.hpp) at the counter
//     (traj, q >> 2, step, kSdeStreamTag)
// with traj = b * S + s of the launch and step = k * substeps + j for sub-step j of observation interval k.  The theta stream
// has 0 in the fourth counter word and kSdeStreamTag is not 0: the two never share a counter.  The adjoint regenerates each
// draw from its counter; nothing is kept for it.  The key is two integer-valued floats in [0, 2^24), the last two floats of the
// thread's data row of cond ([treatments | forcing samples | key lo, key hi]), converted by truncation: the forward and the
// adjoint launch are given the same cond, so they agree by construction.
//
// Reaction channels (vihds/modelgen.py: noise_channels, channel_noise(self, y, p, c); vihds_models.hpp: noise_channels<M>).  A
// model may instead give every reaction channel r = 0 .. R-1 a Wiener process of its own, which enters every species q the
// channel touches with the amplitude G[q][r] (the chemical Langevin equation: G[q][r] = nu_r[q] sqrt(a_r)):
//     dw[r] = sqrtf(h) * xi_r;   for r ascending, for q ascending in the channel's pattern:  y[q] = fmaf(G[q][r], dw[r], y[q])
// after the unchanged step Phi_h, G at the step's start state.  xi_r is normal r & 3 of the block at the counter
// (traj, r >> 2, step, kSdeStreamTag): the layout above with the channel index where the species index stood, so a model with one
// channel per species and a diagonal G repeats the per-species model bit for bit.  G is the flat array G[q * R + r]; an entry
// outside the pattern M::channel_species(r) is a structural zero, never written and never read.  The adjoint regenerates dw,
// seeds Gb[q][r] = lam'[q] * dw[r] on the pattern, runs channel_noise_vjp into a temporary yb, then the scheme's own step
// adjoint on lam, then lam += yb.
//
// The first part below (which h a solver uses, the counter, block and lane of a species, the step index of a sub-step) uses
// no HIP intrinsic and is __host__ __device__: a stand-alone host program can run it (tests/test_modelgen_sde_host.py compiles
// one with the address and undefined-behaviour sanitizers).  The wrappers around the step follow under __HIPCC__.
#pragma once

#include "../../include/vihds_hip.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VIHDS_SDE_HD __host__ __device__ __forceinline__
#else
#define VIHDS_SDE_HD inline
#endif

namespace vihds {

// the fourth counter word of the process-noise stream ("SDE1"); the theta stream's is 0
constexpr unsigned int kSdeStreamTag = 0x53444531u;
// floats of a row of cond behind the treatments and the forcing samples: key lo, key hi
constexpr int kSdeKeyFloats = 2;
static_assert(kSdeStreamTag != 0u, "the theta stream has 0 in the fourth counter word");

// what a thread knows about its noise stream: the row's key and the trajectory's index in the launch
struct SdeKey {
  unsigned int k0, k1, traj;
};
// a key word from its float in cond: an integer-valued float in [0, 2^24), by truncation (anything else is clamped into range:
// the host refuses it before upload)
VIHDS_SDE_HD unsigned int sde_key_word(float v) {
  return v >= 0.f ? (v < 16777216.f ? (unsigned int)v : 16777215u) : 0u;
}
struct SdeCounter {
  unsigned int c0, c1, c2, c3;
};
// the Philox block that holds the draw of a species and the draw's place in it
VIHDS_SDE_HD unsigned int sde_block(int species) { return (unsigned int)species >> 2; }
VIHDS_SDE_HD int sde_lane(int species) { return species & 3; }
VIHDS_SDE_HD SdeCounter sde_counter(unsigned int traj, int species, unsigned int step) {
  return SdeCounter{traj, sde_block(species), step, kSdeStreamTag};
}
// the step index of sub-step j of observation interval k (substeps = 1: k itself)
VIHDS_SDE_HD unsigned int sde_step_index(int k, int substeps, int j) { return (unsigned int)k * (unsigned int)substeps + (unsigned int)j; }
// the length h the scheme advances by over [t0, t1]: modeuler's fixed step h0 (already divided by substeps where the model has
// them, SubGrid::fixed_step), t1 - t0 for every other solver -- as ode_step forms it
VIHDS_SDE_HD float sde_step_length(int solver, float t0, float t1, float h0) {
  return solver == VIHDS_SOLVER_MODEULER ? h0 : t1 - t0;
}
// whether any species of Philox block q is noisy under `mask` (bit j: species j has a non-zero amplitude)
VIHDS_SDE_HD constexpr bool sde_block_drawn(unsigned int mask, int q) { return ((mask >> (4 * q)) & 0xfu) != 0u; }


// ---- reaction channels: the draw of channel r sits where the draw of species r sits in the per-species layout
VIHDS_SDE_HD unsigned int sde_channel_block(int channel) { return sde_block(channel); }
VIHDS_SDE_HD int sde_channel_lane(int channel) { return sde_lane(channel); }
VIHDS_SDE_HD SdeCounter sde_channel_counter(unsigned int traj, int channel, unsigned int step) {
  return sde_counter(traj, channel, step);
}
// the channels 0 .. R-1 as a mask for sde_block_drawn: a Philox block none of whose channels exist draws nothing
VIHDS_SDE_HD constexpr unsigned int sde_channel_mask(int R) { return R >= 32 ? 0xffffffffu : ((1u << R) - 1u); }
// whether channel r enters species q under the model's pattern (M::channel_species(r): bit q)
template <class M>
VIHDS_SDE_HD constexpr bool sde_channel_enters(int r, int q) {
  return ((M::channel_species(r) >> q) & 1u) != 0u;
}
// y[q] = fmaf(G[q][r], dw[r], y[q]) for r ascending and, within a channel, q ascending over the channel's pattern: the order is
// part of the definition (two channels that enter one species add in this order).  M gives N, NOISE_CHANNELS, channel_species
template <class M>
VIHDS_SDE_HD void sde_channel_accumulate(const float* G, const float* dw, float* y) {
  constexpr int N = M::N, R = M::NOISE_CHANNELS;
#pragma unroll
  for (int r = 0; r < R; ++r) {
#pragma unroll
    for (int q = 0; q < N; ++q) {
      if (sde_channel_enters<M>(r, q)) y[q] = __builtin_fmaf(G[q * R + r], dw[r], y[q]);
    }
  }
}
// the seeds of channel_noise_vjp: Gb[q][r] = lam[q] * dw[r] on the pattern (nothing else of Gb is written or read)
template <class M>
VIHDS_SDE_HD void sde_channel_seed(const float* lam, const float* dw, float* Gb) {
  constexpr int N = M::N, R = M::NOISE_CHANNELS;
#pragma unroll
  for (int r = 0; r < R; ++r) {
#pragma unroll
    for (int q = 0; q < N; ++q) {
      if (sde_channel_enters<M>(r, q)) Gb[q * R + r] = lam[q] * dw[r];
    }
  }
}

}  // namespace vihds

#if defined(__HIPCC__)
#include "vihds_rng.hpp"

namespace vihds {

// (defined in vihds_ode_kernels.hpp, which includes this header ahead of them)
template <class M, int SOLVER>
__device__ __forceinline__ void ode_step(float t0, float t1, float h0, float* y, const float* p, const float* wts);
template <class M, int SOLVER, class Ctx>
__device__ __forceinline__ void ode_step_vjp(float t0, float t1, float h0, const float* y, const float* p, const float* wts,
                                             float* lam, float* pb, Ctx& wtsb);

// the key of the thread's data row b: the last two floats of its row of cond
__device__ __forceinline__ SdeKey sde_load_key(const float* cond, int C, int b, int traj) {
  const float* row = cond + (size_t)b * C + (C - kSdeKeyFloats);
  return SdeKey{sde_key_word(row[0]), sde_key_word(row[1]), (unsigned int)traj};
}

// dw[j] = sqrt(h) * xi_j for the noisy species of M (M::NOISE_MASK), 0 for the others; a block of four species without a
// noisy one draws nothing.  The forward and the adjoint both call this: the same counters, the same instructions, the same bits
template <class M>
__device__ __forceinline__ void sde_increments(const SdeKey& key, unsigned int step, float h, float* dw) {
  constexpr int N = M::N;
  const float sh = sqrtf(h);
#pragma unroll
  for (int q = 0; q < (N + 3) / 4; ++q) {
    if (sde_block_drawn(M::NOISE_MASK, q)) {  // (a constant of the model: the branch folds)
      float z[4];
      const SdeCounter c = sde_counter(key.traj, 4 * q, step);
      philox_normal4(c.c0, c.c1, c.c2, c.c3, key.k0, key.k1, z);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (4 * q + r < N) dw[4 * q + r] = ((M::NOISE_MASK >> (4 * q + r)) & 1u) ? sh * z[r] : 0.f;
      }
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (4 * q + r < N) dw[4 * q + r] = 0.f;
      }
    }
  }
}

// dw[r] = sqrt(h) * xi_r for the R channels of M: the instructions of sde_increments with the channel index where the species
// index stood.  The forward and the adjoint both call this
template <class M>
__device__ __forceinline__ void sde_channel_increments(const SdeKey& key, unsigned int step, float h, float* dw) {
  constexpr int R = noise_channels<M>::value;
  const float sh = sqrtf(h);
#pragma unroll
  for (int q = 0; q < (R + 3) / 4; ++q) {
    if (sde_block_drawn(sde_channel_mask(R), q)) {  // (a constant of the model: the branch folds)
      float z[4];
      const SdeCounter c = sde_channel_counter(key.traj, 4 * q, step);
      philox_normal4(c.c0, c.c1, c.c2, c.c3, key.k0, key.k1, z);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (4 * q + r < R) dw[4 * q + r] = sh * z[r];
      }
    }
  }
}

// one noisy step: y <- Phi_h(y) + g(y, p) * dw, g at the start state.  The amplitudes are evaluated first and live across the
// scheme's step; the draws live only after it
template <class M, int SOLVER>
__device__ __forceinline__ void noisy_step(float t0, float t1, float h0, unsigned int step_index, const SdeKey& key, float* y,
                                           const float* p, const float* wts) {
  constexpr int N = M::N;
  if constexpr (noise_channels<M>::value > 0) {
    // reaction channels: the amplitudes of the pattern live across the scheme's step, the R increments only after it
    constexpr int R = noise_channels<M>::value;
    float G[N * R];
    M::channel_noise(y, p, G);
    ode_step<M, SOLVER>(t0, t1, h0, y, p, wts);
    float dw[R];
    sde_channel_increments<M>(key, step_index, sde_step_length(SOLVER, t0, t1, h0), dw);
    sde_channel_accumulate<M>(G, dw, y);
  } else {
    float g[N];
#pragma unroll
    for (int j = 0; j < N; ++j) g[j] = 0.f;
    M::diffusion(y, p, g);
    ode_step<M, SOLVER>(t0, t1, h0, y, p, wts);
    float dw[N];
    sde_increments<M>(key, step_index, sde_step_length(SOLVER, t0, t1, h0), dw);
#pragma unroll
    for (int j = 0; j < N; ++j) {
      if ((M::NOISE_MASK >> j) & 1u) y[j] = __builtin_fmaf(g[j], dw[j], y[j]);
    }
  }
}

// reverse of one noisy step from its start state u: lam (the adjoint of u') -> the adjoint of u; pb += the parameter part.
// gb = lam * dw with the regenerated draws, diffusion_vjp into a temporary yb, the scheme's own step adjoint on lam, then
// lam += yb.  No atomics: gradients repeat bit for bit
template <class M, int SOLVER, class Ctx>
__device__ __forceinline__ void noisy_step_vjp(float t0, float t1, float h0, unsigned int step_index, const SdeKey& key,
                                               const float* u, const float* p, const float* wts, float* lam, float* pb,
                                               Ctx& wtsb) {
  constexpr int N = M::N;
  if constexpr (noise_channels<M>::value > 0) {
    constexpr int R = noise_channels<M>::value;
    float yb[N];
    {
      float dw[R], Gb[N * R];
      sde_channel_increments<M>(key, step_index, sde_step_length(SOLVER, t0, t1, h0), dw);
      sde_channel_seed<M>(lam, dw, Gb);
#pragma unroll
      for (int j = 0; j < N; ++j) yb[j] = 0.f;
      M::channel_noise_vjp(u, p, Gb, yb, pb);
    }
    ode_step_vjp<M, SOLVER>(t0, t1, h0, u, p, wts, lam, pb, wtsb);
#pragma unroll
    for (int j = 0; j < N; ++j) lam[j] += yb[j];
  } else {
    float gb[N], yb[N];
    sde_increments<M>(key, step_index, sde_step_length(SOLVER, t0, t1, h0), gb);
#pragma unroll
    for (int j = 0; j < N; ++j) {
      gb[j] *= lam[j];
      yb[j] = 0.f;
    }
    M::diffusion_vjp(u, p, gb, yb, pb);
    ode_step_vjp<M, SOLVER>(t0, t1, h0, u, p, wts, lam, pb, wtsb);
#pragma unroll
    for (int j = 0; j < N; ++j) lam[j] += yb[j];
  }
}

}  // namespace vihds
#endif
