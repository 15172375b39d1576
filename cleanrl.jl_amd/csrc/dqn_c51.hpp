// dqn_c51.hpp — the categorical value distribution of Bellemare et al. 2017 (C51) for dqn.hip: N atoms on [v_min, v_max], a softmax head of 2·N rows,
// the projection of the shifted target distribution back onto the atoms, the cross-entropy and its cotangent. The expressions are pinned in
// include/cleanrl_hip.h ("Categorical DQN" block); tests/c51_ref.py restates them in numpy. Everything here is Float64 with contraction off; every sum
// starts from 0.0 and runs in ascending atom order.
//
// The functions below are called by ALL 64 lanes of ONE wave with the whole wave active; lane i < N owns atom i, lanes >= N carry +0.0. A sum over
// the atoms reads lane 0, 1, … 63 in turn (v_readlane: the value goes through a scalar register to every lane, no LDS and no wait on it) and adds
// them in that order, so the result is wave-uniform and has no tree order in it; the reads do not depend on each other, only the adds do. The 64 − N
// trailing adds of +0.0 change no bit (x + 0.0 = x for every x but −0.0, which a sum that starts from +0.0 never holds), and a trip count known at
// compile time lets the loop unroll into straight-line code. The update's TD kernel, the collect kernel, the evaluation kernel, crl_dqn_q_values /
// crl_dqn_c51_probs and crl_dqn_c51_project_probe all run these same functions, which is why their bits agree.
#pragma once
#include "common.hpp"

namespace crl {

constexpr int C51_MAX_ATOMS = 64;      // a lane owns an atom
constexpr int C51_TD_WAVES = 4;        // samples per block of the TD kernel: one wave per SIMD, ⌈k / 4⌉ blocks

struct C51Dev {
  int32_t on, N, P, pad;               // P = 10764 + 85·2N parameters
  double v_min, v_max;
  double* L;                           // [nets][k][2N] logits, row a·N + i = atom i of action a
  double *dl, *proj;                   // [k][N] cotangent on the taken action's logits, projected target m
  double* sloss;                       // [k] loss_j
};

__device__ __forceinline__ double c51_delta(double v_min, double v_max, int N) {
#pragma clang fp contract(off)
  return (v_max - v_min) / (double)(N - 1);
}
__device__ __forceinline__ double c51_atom(double v_min, double delta, int i) {
#pragma clang fp contract(off)
  return v_min + (double)i * delta;
}

// lane i's v in every lane; i is a compile-time constant at every use (the loops below are fully unrolled)
__device__ __forceinline__ double c51_lane(double v, int i) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), i), __builtin_amdgcn_readlane(__double2loint(v), i));
}

// Σ_i v_i, i ascending from 0.0; the same bits in every lane. Lanes >= N must hold 0.0.
__device__ __forceinline__ double c51_sum(double v) {
#pragma clang fp contract(off)
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < C51_MAX_ATOMS; ++i) s += c51_lane(v, i);
  return s;
}

// mx = max l; d = l − mx; e = exp(d); S = Σ e; p = e / S; logp = d − log(S)
__device__ __forceinline__ void c51_softmax(double l, int N, int lane, double& p, double& logp) {
#pragma clang fp contract(off)
  const double mx = wave_max(lane < N ? l : -__builtin_huge_val());   // a maximum is exact in any order
  const double d = lane < N ? l - mx : 0.0;
  const double e = lane < N ? exp(d) : 0.0;
  const double S = c51_sum(e);
  p = e / S;
  logp = d - log(S);
}

// Q = Σ_i z_i·p_i (p is 0.0 in the lanes past N)
__device__ __forceinline__ double c51_expect(double p, double v_min, double delta, int lane) {
#pragma clang fp contract(off)
  return c51_sum(c51_atom(v_min, delta, lane) * p);
}

// The projection: source atom `lane` carries pp = p'_lane to Tz = clamp(R + ((disc·z)·(1 − term))), which lies between atoms lo and up; target atom
// `lane` then GATHERS what it receives, sources ascending (a source that sends it nothing adds an exact 0.0) — no atomics, so the bits do not depend
// on scheduling. pp must be 0.0 in the lanes past N: their atoms lie above v_max, so they send that 0.0 to atom N − 1. → m_lane, 0.0 past N
__device__ __forceinline__ double c51_project(double pp, double R, double disc, uint8_t term, double v_min, double v_max, double delta, int N, int lane) {
#pragma clang fp contract(off)
  const double top = (double)(N - 1);
  double Tz = R + ((disc * c51_atom(v_min, delta, lane)) * (1.0 - (double)term));
  Tz = Tz < v_min ? v_min : (Tz > v_max ? v_max : Tz);
  double b = (Tz - v_min) / delta;
  b = b > top ? top : b;
  const double lo = floor(b), up = ceil(b);
  const int lo_i = (int)lo, up_i = (int)up;
  const double wl = lo == up ? pp : pp * (up - b), wu = lo == up ? 0.0 : pp * (b - lo);
  double m = 0.0;
#pragma unroll
  for (int i = 0; i < C51_MAX_ATOMS; ++i) {
    const int l = __builtin_amdgcn_readlane(lo_i, i), u = __builtin_amdgcn_readlane(up_i, i);
    const double a = c51_lane(wl, i), c = c51_lane(wu, i);
    m += l == lane ? a : (u == lane ? c : 0.0);
  }
  return m;
}

// crl_dqn_c51_project_probe: the projection alone on caller-supplied rows, one wave per sample; probs and proj are (N, k), atom fastest
__global__ void __launch_bounds__(64 * C51_TD_WAVES) dqn_c51_project_probe_kernel(const double* probs, const double* nret, const double* ndisc,
                                                                                  const uint8_t* terminal, int k, int N, double v_min, double v_max,
                                                                                  double* proj) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const double delta = c51_delta(v_min, v_max, N);
  for (int j = w; j < k; j += C51_TD_WAVES) {
    const double pp = lane < N ? probs[(size_t)N * j + lane] : 0.0;
    const double m = c51_project(pp, nret[j], ndisc[j], terminal[j], v_min, v_max, delta, N, lane);
    if (lane < N) proj[(size_t)N * j + lane] = m;
  }
}

}  // namespace crl
