// optim.hpp — Flux 0.13.4 Optimiser(ClipNorm(thresh), Adam(η, (0.9, 0.999), 1e-8)) stated once (oracle: orc_clipnorm_adam): the per-element
// arithmetic every optimiser kernel calls (clipnorm_adam_kernel, adam_slice_kernel: optim.hip; reduce_optim_kernel: update.hip; dqn_adam_kernel: dqn.hip),
// the Flux-order table of the 12 parameter arrays and the arguments the PPO / A2C launches share. The kernels differ only in the order they add Σg².
#pragma once
#include <hip/hip_runtime.h>

namespace crl {

constexpr double ADAM_B1 = 0.9, ADAM_B2 = 0.999, ADAM_EPS = 1e-8;
constexpr double CLIPNORM_THRESH = 0.5;   // ppo.jl:93, a2c.jl:36

// Flat layout of the parameters (and of the gradient, m, v): actor W1 b1 W2 b2 W3 b3, then the critic's six; array a = [off[a], off[a + 1])
struct ParamTable { int off[13]; };
inline ParamTable param_table(int obs_dim, int n_act, int hidden) {
  const int D = obs_dim, A = n_act, H = hidden;
  const int sizes[12] = {H * D, H, H * H, H, A * H, A, H * D, H, H * H, H, H, 1};
  ParamTable t;
  t.off[0] = 0;
  for (int i = 0; i < 12; ++i) t.off[i + 1] = t.off[i] + sizes[i];
  return t;
}

// What every ClipNorm + Adam launch needs besides its gradient; betap = [12][2] running powers β₁ᵗ, β₂ᵗ per array
struct OptimCore {
  ParamTable tab;
  float* params; float* m; float* v; double* betap;
  double eta, thresh;
};

// The helpers carry the pragma themselves: it is lexical, and a contracted b1·m + (1 − b1)·g rounds once where the oracle rounds twice.

// ClipNorm of one array from its Float64 Σg²: the norm is rounded to Float32 (Flux: norm of a Float32 array), sc = thresh / norm where it clips
__device__ __forceinline__ bool clipnorm_scale(double ss, double thresh, double& sc) {
#pragma clang fp contract(off)
  const float nrm = (float)sqrt(ss);
  const bool clip = (double)nrm > thresh;
  sc = clip ? thresh / (double)nrm : 1.0;
  return clip;
}

// Adam on one entry: Float64 scalar math on Float32 state; bp0 / bp1 are the β powers BEFORE this step's advance
__device__ __forceinline__ void adam_entry(double g, float m_old, float v_old, float p_old, double bp0, double bp1, double eta, bool clip, double sc,
                                           float& mi, float& vi, float& pi) {
#pragma clang fp contract(off)
  if (clip) g = (double)(float)(g * sc);
  mi = (float)(ADAM_B1 * (double)m_old + (1 - ADAM_B1) * g);
  vi = (float)(ADAM_B2 * (double)v_old + (1 - ADAM_B2) * g * g);
  const double delta = (double)mi / (1 - bp0) / (sqrt((double)vi / (1 - bp1)) + ADAM_EPS) * eta;
  pi = p_old - (float)delta;
}

// the running powers of array `arr` after a step that used (bp0, bp1)
__device__ __forceinline__ void betap_advance(double* betap, int arr, double bp0, double bp1) {
#pragma clang fp contract(off)
  betap[2 * arr] = bp0 * ADAM_B1; betap[2 * arr + 1] = bp1 * ADAM_B2;
}

}  // namespace crl
