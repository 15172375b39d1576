// rollout_env.hpp — the per-lane env owner of the 4 / 2 / 64 rollout kernels (policy.hip): what a rollout step does besides the forward pass, stated once.
// One lane owns one CartPole env for all num_steps steps of the launch: load its state; per step sample, step the env, Buffer.add!, episode bookkeeping
// (ppo.jl:125-165); store the state back; then the fused compat-GAE tail and the wave's episode statistics. How the forward pass is spread over waves,
// which wave stores `value`, and where the step's uniform and reset state come from stay with the kernel.
#pragma once
#include "common.hpp"
#include "env.hpp"
#include "ppo_ctx.hpp"
#include "stats.hpp"

namespace crl {

struct RolloutArgs {
  DevCfg c;
  const float* params;
  float* obs; int32_t* action; float* logprob; float* reward; uint8_t* terminal; float* value;
  float* env_state; int32_t* env_t; float* cur_obs; uint8_t* next_done; float* ep_return; int32_t* ep_length;
  double* ep_stats;
  crl_episode_record* ring; uint32_t* ring_count; int ring_cap;   // per-episode records (ring_cap = 0: off)
  uint64_t iteration;
  int stagger;  // s_sleep units (64 clocks) by which waves 4-7 of an 8-wave block start late
  // GAE fused into the tail of the rollout (crl_ppo_iterate, compat mode): the wave that stepped 32 envs for num_steps steps
  // scans their value / reward / terminal columns — which it has just written and which still sit in L2 — backwards and
  // writes advantages and returns (ppo.jl:48-73,173-181): no separate launch, no HBM read of the scan's inputs.
  float* adv; float* ret; int fuse_gae; float gamma, gl;
  double* range_err = nullptr;   // fp16x2 weight-window error word (CX2 kernels)
};

// gae(values, rewards, terminals, γ, λ) for ONE env (this lane), compat mode (ppo.jl:66: the loop starts at k-1, the last slot
// is defined as 0 — Q1): the reference's serial Float64 recurrence, step by step ⇒ bit-identical to orc_gae.
__device__ __forceinline__ void gae_tail_compat(const RolloutArgs& a, int e) {
#pragma clang fp contract(off)
  const int nt = a.c.nt, k = a.c.k;
  size_t idx = (size_t)e + (size_t)nt * (k - 1);
  float vnext = a.value[idx];
  uint32_t tnext = a.terminal[idx];
  a.adv[idx] = 0.0f; a.ret[idx] = 0.0f + vnext;
  double A = 0.0;
  // eight steps' inputs are loaded together (the loads cannot be hoisted above the stores by the compiler: it must assume
  // adv / ret alias the inputs), then the serial recurrence runs on registers: one L2 round trip per eight steps
  constexpr int CH = 8;
  for (int t0 = k - 2; t0 >= 0; t0 -= CH) {
    float v[CH], r[CH]; uint32_t tm[CH];
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const bool ok = t0 - i >= 0;
      const size_t ix = ok ? (size_t)e + (size_t)nt * (t0 - i) : (size_t)e;
      v[i] = a.value[ix]; r[i] = a.reward[ix]; tm[i] = a.terminal[ix];
    }
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      if (t0 - i < 0) break;
      const size_t ix = (size_t)e + (size_t)nt * (t0 - i);
      const double nonterm = 1.0 - (double)(tnext ? 1 : 0);
      const double delta = (double)r[i] + ((double)a.gamma * nonterm) * (double)vnext - (double)v[i];
      const double cc = (double)a.gl * nonterm;
      A = delta + (cc * A);
      const float a32 = (float)A;
      a.adv[ix] = a32; a.ret[ix] = a32 + v[i];
      vnext = v[i]; tnext = tm[i];
    }
  }
}

// One env's registers for the launch. A wave that owns no env keeps the zeros.
struct EnvOwner {
  float s[4] = {0, 0, 0, 0}, co[4] = {0, 0, 0, 0};   // env state, current observation (the network's input)
  int t_env = 0;
  uint8_t nd = 0;
  float ep_ret = 0.0f;
  int ep_len = 0;
  double st_n = 0.0, st_ret = 0.0, st_len = 0.0, st_max = 0.0;   // this lane's finished episodes
};

__device__ __forceinline__ void env_owner_load(EnvOwner& o, const RolloutArgs& a, int ee) {
  const float4 sv = reinterpret_cast<const float4*>(a.env_state)[ee];
  const float4 cv = reinterpret_cast<const float4*>(a.cur_obs)[ee];
  o.s[0] = sv.x; o.s[1] = sv.y; o.s[2] = sv.z; o.s[3] = sv.w;
  o.co[0] = cv.x; o.co[1] = cv.y; o.co[2] = cv.z; o.co[3] = cv.w;
  o.t_env = a.env_t[ee]; o.nd = a.next_done[ee]; o.ep_ret = a.ep_return[ee]; o.ep_len = a.ep_length[ee];
}

// ppo.jl:127 get_action, after the logits: softmax, the categorical draw from the uniform u, the action's log-probability
template <int A>
__device__ __forceinline__ int env_owner_sample(const float (&z)[A], double u, float& lpa) {
  float p[A], lp[A];
  softmax_logsoftmax<A>(z, p, lp);
  const int act = sample_weights<A>(p, u);
  lpa = lp[0];
#pragma unroll
  for (int i = 1; i < A; ++i) lpa = (act == i) ? lp[i] : lpa;
  return act;
}

// ppo.jl:125,130-165 for the sampled action: env step, Buffer.add! (all fields but `value`), next_obs / next_done, and at an episode end the statistics,
// the record and reset!(env). reset: the env's reset state of this step where another wave has computed it ahead (rollout_split6_kernel: read only at
// an episode end), nullptr: computed here (cartpole_reset, Philox stream 1).
__device__ __forceinline__ void env_owner_advance(EnvOwner& o, const RolloutArgs& a, int act, float lpa, uint32_t gid, uint64_t gstep, int step, size_t b,
                                                  bool writer, const float4* reset = nullptr) {
  const DevCfg& c = a.c;
  o.ep_len += 1;                                                     // ppo.jl:125
  const bool done = cartpole_step(o.s, o.t_env, act);                // ppo.jl:130
  const float rew = done ? 0.0f : 1.0f;                              // ppo.jl:132 (RLEnvs: reward 0 on the terminal step)
  if (writer) {                                                      // ppo.jl:133-140 Buffer.add!
    // obs/action/logprob are next read by the update pass, a full GAE + shuffle later: stream them past the caches
    // (nontemporal) so the 75 MB the GAE scan needs (value, reward, terminal) stay resident in L2 / Infinity Cache
    store_nt4(reinterpret_cast<f32x4*>(a.obs) + b, o.co[0], o.co[1], o.co[2], o.co[3]);
    __builtin_nontemporal_store(act, a.action + b); __builtin_nontemporal_store(lpa, a.logprob + b);
    a.reward[b] = rew; a.terminal[b] = o.nd;
  }
  o.co[0] = o.s[0]; o.co[1] = o.s[1]; o.co[2] = o.s[2]; o.co[3] = o.s[3];   // ppo.jl:143 next_obs (before reset!, Q7)
  o.nd = done ? 1 : 0;                                               // ppo.jl:144
  o.ep_ret += rew;                                                   // ppo.jl:145
  if (done) {                                                        // ppo.jl:147-165
    if (writer) {
      o.st_n += 1.0; o.st_ret += (double)o.ep_ret; o.st_len += (double)o.ep_len; o.st_max = fmax(o.st_max, (double)o.ep_ret);
      episode_ring_push(a.ring, a.ring_count, a.ring_cap, o.ep_ret, o.ep_len, gid, step);
    }
    o.ep_ret = 0.0f; o.ep_len = 0;
    if (reset) { const float4 rv = *reset; o.s[0] = rv.x; o.s[1] = rv.y; o.s[2] = rv.z; o.s[3] = rv.w; }
    else cartpole_reset(o.s, c.seed, gid, gstep, 1);                 // ppo.jl:164 reset!(env)
    o.t_env = 0;
    if (!c.stale_obs) { o.co[0] = o.s[0]; o.co[1] = o.s[1]; o.co[2] = o.s[2]; o.co[3] = o.s[3]; }
  }
}

// one step from the logits on: the two pieces above (rollout_cartpole_kernel calls them apart: its critic runs between them)
template <int A>
__device__ __forceinline__ void env_owner_step(EnvOwner& o, const RolloutArgs& a, const float (&z)[A], double u, uint32_t gid, uint64_t gstep, int step, size_t b,
                                               bool writer, const float4* reset = nullptr) {
  float lpa;
  const int act = env_owner_sample<A>(z, u, lpa);
  env_owner_advance(o, a, act, lpa, gid, gstep, step, b, writer, reset);
}

__device__ __forceinline__ void env_owner_store(const EnvOwner& o, const RolloutArgs& a, int e) {
  reinterpret_cast<float4*>(a.env_state)[e] = make_float4(o.s[0], o.s[1], o.s[2], o.s[3]);
  reinterpret_cast<float4*>(a.cur_obs)[e] = make_float4(o.co[0], o.co[1], o.co[2], o.co[3]);
  a.env_t[e] = o.t_env; a.next_done[e] = o.nd; a.ep_return[e] = o.ep_ret; a.ep_length[e] = o.ep_len;
}

// after the last step, by the whole env wave: the fused GAE tail (value[] must be visible to this lane: the caller's barrier or fence), then the
// episode statistics of this rollout ("Episode Statistics" record, aggregated)
__device__ __forceinline__ void env_owner_finish(const EnvOwner& o, const RolloutArgs& a, int e, bool writer) {
  if (writer && a.fuse_gae) gae_tail_compat(a, e);
  episode_stats_flush(a.ep_stats, o.st_n, o.st_ret, o.st_len, o.st_max);
}

}  // namespace crl
