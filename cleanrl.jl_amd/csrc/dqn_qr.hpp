// dqn_qr.hpp — the quantile-regression value distribution of Dabney et al. 2018 (QR-DQN) for dqn.hip: N quantile locations θ_i per action at the fixed
// fractions τ_i = (i + 0.5) / N, a head of 2·N rows like the categorical one (row a·N + i = quantile i of action a), no support and no projection:
// the loss is the quantile Huber loss over all N × N pairs of (target T_j, quantile θ_i). The expressions are pinned in include/cleanrl_hip.h
// ("Quantile-regression DQN" block); tests/qr_ref.py restates them in numpy. Float64, contraction off, nothing transcendental: + − × ÷ |·| and
// comparisons only, so a uniform-replay run has no rounding freedom at all.
//
// As in dqn_c51.hpp the functions are called by ALL 64 lanes of ONE wave; lane i < N owns quantile i, lanes >= N carry +0.0 into every cross-lane
// sum (c51_sum: lanes ascending through a scalar register, so N = 2..64 is one code path). The pair loop is the other way round: lane i keeps θ_i
// and τ_i in registers and walks j = 0..N−1, taking T_j out of lane j by v_readlane with the loop counter as the (scalar) lane select — N trips
// instead of 64, no LDS, no atomics, no barrier — and both of its sums (Σ_j wt·h/κ and G_i = Σ_j wt·c) are private register chains in j order.
// The TD kernel, the collect kernels, the evaluation kernels, crl_dqn_q_values / crl_dqn_qr_quantiles and crl_dqn_qr_loss_probe run these same
// functions, which is why their bits agree.
#pragma once
#include "common.hpp"
#include "dqn_c51.hpp"

namespace crl {

__device__ __forceinline__ double qr_tau(int i, int N) {
#pragma clang fp contract(off)
  return ((double)i + 0.5) / (double)N;
}

// Q = (Σ_i θ_i, i ascending from 0.0) / N; the same bits in every lane. Lanes >= N must hold 0.0.
__device__ __forceinline__ double qr_value(double theta, int N) {
#pragma clang fp contract(off)
  return c51_sum(theta) / (double)N;
}

// lane j's v in every lane, j wave-uniform but not a compile-time constant: the scalar-register broadcast of c51_lane with an SGPR lane select
__device__ __forceinline__ double qr_lane(double v, int j) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), j), __builtin_amdgcn_readlane(__double2loint(v), j));
}

// The N × N pair loss seen from quantile `lane`: theta = θ_lane, T = T_lane (what lanes >= N hold in either is never read into a sum).
// → rho = (Σ_j (wt·h)/κ) / N and G = Σ_j wt·c, j ascending from 0.0; rho is 0.0 in the lanes past N so that c51_sum(rho) is loss_s.
__device__ __forceinline__ void qr_pair(double theta, double T, double kappa, int N, int lane, double& rho, double& G) {
#pragma clang fp contract(off)
  const double tau = qr_tau(lane, N), half_kappa = 0.5 * kappa;
  double sh = 0.0, sg = 0.0;
  for (int j = 0; j < N; ++j) {   // N trips, not unrolled: v_readlane with a scalar lane select is convergent, and the chain below is what bounds a trip
    const double u = qr_lane(T, j) - theta;
    const double au = u < 0.0 ? -u : u;
    const bool quad = au <= kappa, neg = u < 0.0;
    const double h = quad ? (0.5 * u) * u : kappa * (au - half_kappa);
    const double c = quad ? u : (neg ? -kappa : kappa);
    const double d = tau - (neg ? 1.0 : 0.0);
    const double wt = d < 0.0 ? -d : d;
    sh += (wt * h) / kappa;
    sg += wt * c;
  }
  rho = lane < N ? sh / (double)N : 0.0;
  G = sg;
}

// the cotangent of loss_s on θ_lane, weighted: (w · (−(G / κ))) / N; the TD kernel divides by k behind it, the probe passes w = 1.0
__device__ __forceinline__ double qr_dtheta(double G, double kappa, int N, double w) {
#pragma clang fp contract(off)
  return (w * (-(G / kappa))) / (double)N;
}

// T_lane = R + ((disc · θ'_lane) · (1 − term))
__device__ __forceinline__ double qr_target(double R, double disc, double theta_next, uint8_t term) {
#pragma clang fp contract(off)
  return R + ((disc * theta_next) * (1.0 - (double)term));
}

// crl_dqn_qr_loss_probe: the pair loss alone on caller-supplied rows, one wave per sample; theta, target and dtheta are (N, k), quantile fastest
__global__ void __launch_bounds__(64 * C51_TD_WAVES) dqn_qr_loss_probe_kernel(const double* theta, const double* target, int k, int N, double kappa,
                                                                              double* loss, double* dtheta) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int s = blockIdx.x * C51_TD_WAVES + w; s < k; s += gridDim.x * C51_TD_WAVES) {   // s is wave-uniform: whole waves take a sample or leave
    const double th = lane < N ? theta[(size_t)N * s + lane] : 0.0, T = lane < N ? target[(size_t)N * s + lane] : 0.0;
    double rho, G;
    qr_pair(th, T, kappa, N, lane, rho, G);
    const double l = c51_sum(rho);
    if (lane < N) dtheta[(size_t)N * s + lane] = qr_dtheta(G, kappa, N, 1.0);
    if (lane == 0) loss[s] = l;
  }
}

}  // namespace crl
