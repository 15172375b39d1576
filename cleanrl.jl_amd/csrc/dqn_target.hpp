// dqn_target.hpp — how dqn.hip forms the TD target on a crl_dqn_create_with handle: uncorrected n-step returns and double Q-learning (van Hasselt
// et al. 2016), the two Rainbow components that change the target and nothing else. The expressions are pinned in include/cleanrl_hip.h ("DQN target
// options" block); tests/dqn_target_ref.py restates them in numpy. Everything here is Float64 with contraction off.
//
// nstep_walk is ONE thread's walk for ONE sample: at most n_step dependent ring reads. dqn_tgt_sample_kernel (dqn.hip) runs it at the tail of the
// sampling launch, in the block that drew; dqn_nstep_probe_kernel below runs the same function on a ring the host wrote.
#pragma once
#include "common.hpp"

namespace crl {

constexpr int TGT_MAX_N_STEP = 16;

struct TgtDev {
  int32_t on, n_step, double_q, pad;
  int32_t *last, *m, *astar;     // [k] the slot the bootstrap reads, the steps summed, the bootstrap action of the last update
  double *nret, *ndisc, *td;     // [k] R, disc = gamma^m, the TD target
};

// From slot s forward in time: R = Σ_i disc_i·reward, disc = gamma^m by repeated multiplication; stops after a terminal transition, after n_step
// transitions, or at the newest transition (the one before ptr, the slot the next add takes): the horizon is cut there, never wrapped into the oldest.
__device__ __forceinline__ void nstep_walk(const double* __restrict__ reward, const uint8_t* __restrict__ terminal, int cap, int ptr, int s, int n_step,
                                           double gamma, int& last, int& m, double& R, double& disc) {
#pragma clang fp contract(off)
  R = 0.0; disc = 1.0; m = 0;
  int c = s;
  while (true) {
    R = R + disc * reward[c];
    disc = disc * gamma;
    m += 1; last = c;
    if (terminal[last] != 0 || m == n_step) break;
    const int nx = last + 1 == cap ? 0 : last + 1;
    if (nx == ptr) break;
    c = nx;
  }
}

// the bootstrap action: the first maximum of q_net(x) under double_q, of target_net(x) otherwise (sq = q_net(x), tq = target_net(x))
__device__ __forceinline__ int tgt_astar(int double_q, double sq0, double sq1, double tq0, double tq1) {
  return double_q ? (sq1 > sq0 ? 1 : 0) : (tq1 > tq0 ? 1 : 0);
}

// td = R + ((disc·next_q)·(1 − terminal[last]))
__device__ __forceinline__ double tgt_td(double R, double disc, double next_q, uint8_t term) {
#pragma clang fp contract(off)
  return R + disc * next_q * (1.0 - (double)term);
}

// crl_dqn_nstep_probe: the walk alone, one sample per thread, on a scratch ring
__global__ void __launch_bounds__(1024) dqn_nstep_probe_kernel(const double* reward, const uint8_t* terminal, int cap, int ptr, const int32_t* idx, int k,
                                                               int n_step, double gamma, int32_t* last, int32_t* m, double* nret, double* ndisc) {
  for (int j = threadIdx.x; j < k; j += blockDim.x) {
    int l, mm; double R, disc;
    nstep_walk(reward, terminal, cap, ptr, (int)idx[j], n_step, gamma, l, mm, R, disc);
    last[j] = l; m[j] = mm; nret[j] = R; ndisc[j] = disc;
  }
}

}  // namespace crl
