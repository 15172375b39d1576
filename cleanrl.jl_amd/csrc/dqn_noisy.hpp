// dqn_noisy.hpp — noisy linear layers (Fortunato et al. 2018, factorised Gaussian noise) for dqn.hip. Every DQN kernel reads its network as a flat
// float image through a.q / a.t, so a noisy handle learns mu and sigma per parameter (NoisyDev.pq / pt: [2P], mu in the twin's layout, then sigma in
// the same layout), materialises the effective image w = mu + sigma·eps into a.q / a.t on the device, and lets every forward, pullback and
// weight-gradient kernel run on that image unchanged; the effective-weight gradient is split into g_mu = g and g_sigma = g·eps where Adam reads it.
// The expressions are pinned in include/cleanrl_hip.h ("Noisy linear layers" block); tests/noisy_ref.py restates them in numpy.
//
// The noise table lists the layers in parameter-array order, each layer xi_in[in] then xi_out[out]; the position in the table is the Philox component
// word. Plain / categorical: 3 layers, 412 + rows3 floats (414 with the scalar head); dueling: 5 layers, 700 + 3·R floats (892 at R = 64).
#pragma once
#include "common.hpp"
#include "normal_bm.hpp"
#include "dqn_duel.hpp"

namespace crl {

constexpr uint32_t S_NOISY_Q = 0x22u, S_NOISY_T = 0x23u;   // Philox streams "noisy online net" / "noisy target net" (DQN's others: 0, 1, 2, 4, 0x20, 0x21, 0xD9, 0xDA)
constexpr int NOISY_MAX_LAYERS = 5;
constexpr int NOISY_MAX_XI = 892;                          // the dueling table at R = 64: 124 + 204 + 148 + 204 + 212

struct NoisyDev {
  int32_t on, P;                 // P = the twin's parameter count = the length of the images a.q / a.t
  float *pq, *pt;                // [2P] each: mu then sigma of the online and of the target net
};

struct NoisyLayer { int in, out, oW, ob, xi; };            // weights at oW (out fastest), bias at ob, xi_in at table position xi, xi_out at xi + in
struct NoisyTable { int n_layers, n_xi; NoisyLayer l[NOISY_MAX_LAYERS]; };

// the layer table of a net: rows3 = the plain head's row count (2, or 2N on a categorical handle); duel: R rows per stream output
__host__ __device__ __forceinline__ NoisyTable noisy_table(bool duel, int R, int rows3) {
  NoisyTable t;
  int x = 0;
  const auto put = [&](int i, int in, int out, int oW, int ob) { t.l[i] = {in, out, oW, ob, x}; x += in + out; };
  if (duel) {
    const DuelOff o = duel_off(R);
    t.n_layers = 5;
    put(0, DUEL_D, DUEL_H1, o.W1, o.b1); put(1, DUEL_H1, DUEL_H2, o.W2v, o.b2v); put(2, DUEL_H2, R, o.W3v, o.b3v);
    put(3, DUEL_H1, DUEL_H2, o.W2a, o.b2a); put(4, DUEL_H2, 2 * R, o.W3a, o.b3a);
  } else {
    t.n_layers = 3;
    put(0, 4, 120, 0, 480); put(1, 120, 84, 600, 10680); put(2, 84, rows3, 10764, 10764 + rows3 * 84);
    for (int i = 3; i < NOISY_MAX_LAYERS; ++i) t.l[i] = {0, 0, 0, 0, 0};
  }
  t.n_xi = x;
  return t;
}
static_assert(DUEL_D == 4 && DUEL_H1 == 120 && DUEL_H2 == 84, "the plain offsets above are dqn_loops.hpp's");

// xi = (float)(sgn(z)·sqrt(|z|)), z the Float64 normal of Philox block (seed, component, gen, stream)
__device__ __forceinline__ float noisy_xi(uint64_t seed, uint32_t comp, uint64_t gen, uint32_t stream) {
#pragma clang fp contract(off)
  const double z = box_muller(philox_env(seed, comp, gen, stream));
  return (float)(z < 0.0 ? -sqrt(-z) : sqrt(z));
}
// the whole table of one net and generation into xi[0 .. n_xi) (LDS or global), the block's threads striding it; no barrier: the caller's
__device__ __forceinline__ void noisy_build_xi(float* xi, int n_xi, uint64_t seed, uint64_t gen, uint32_t stream) {
  for (int c = threadIdx.x; c < n_xi; c += blockDim.x) xi[c] = noisy_xi(seed, (uint32_t)c, gen, stream);
}
// eps of parameter p: weight (i, j) = xi_out[i] * xi_in[j], one Float32 multiply; bias i = xi_out[i]
__device__ __forceinline__ float noisy_eps(const NoisyTable& t, const float* xi, int p) {
#pragma clang fp contract(off)
  int li = 0;
  while (li + 1 < t.n_layers && p >= t.l[li + 1].oW) ++li;
  const NoisyLayer& l = t.l[li];
  if (p >= l.ob) return xi[l.xi + l.in + (p - l.ob)];
  const int r = p - l.oW, j = r / l.out, i = r - j * l.out;
  return xi[l.xi + l.in + i] * xi[l.xi + j];
}
// w = mu + sigma * eps: a Float32 multiply, then a Float32 add
__device__ __forceinline__ float noisy_weight(float mu, float sigma, float eps) {
#pragma clang fp contract(off)
  const float se = sigma * eps;
  return mu + se;
}

}  // namespace crl
