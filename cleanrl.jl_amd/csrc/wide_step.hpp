// wide_step.hpp — one rollout step of one env after the two forward passes: sampling, env step, Buffer.add!, episode bookkeeping (ppo.jl:125-165).
// Every rollout flavour of the layer-wise path calls wide_step_env (wide.hip: per-step, persistent and producer / consumer kernels; ppo_gauss.hip: the
// Gaussian per-step kernel). What the actor's head means is a compile-time tag: HeadSoftmax samples an index from softmax(z) (int32 action plane),
// HeadGauss draws a = μ + σ·ξ from the diagonal Gaussian of ppo_gauss.hpp (float action plane, act_dim words per sample) and steps a continuous env.
#pragma once
#include "common.hpp"
#include "env.hpp"
#include "policy_rt.hpp"
#include "ppo_ctx.hpp"
#include "ppo_gauss.hpp"
#include "stats.hpp"

namespace crl {

// softmax_rt / sample_rt: policy_rt.hpp (shared with eval.hip)
__device__ __forceinline__ float pick_rt(const float (&v)[AMAX], int A, int i) {
  float r = v[0];
#pragma unroll
  for (int a = 1; a < AMAX; ++a) if (a < A) r = (i == a) ? v[a] : r;
  return r;
}
__device__ __forceinline__ void load_logits(const float* Z, int A8, int A, size_t m, float (&z)[AMAX]) {
#pragma unroll
  for (int a = 0; a < AMAX; ++a) z[a] = a < A ? Z[(size_t)A8 * m + a] : 0.0f;
}

struct WStepArgs {
  DevCfg c; const float* Z; int A8; const float* V;
  float* obs; int32_t* action; float* logprob; float* reward; uint8_t* terminal; float* value;
  float* env_state; int32_t* env_t; float* cur_obs; uint8_t* next_done; float* ep_return; int32_t* ep_length; double* ep_stats;
  crl_episode_record* ring; uint32_t* ring_count; int ring_cap;
  uint64_t iteration; int step;
};

// the discrete head: nothing to carry (the logits' meaning is softmax_rt / sample_rt / pick_rt)
struct HeadSoftmax {};
template <class Head> struct head_is_gauss { static constexpr bool value = false; };
template <> struct head_is_gauss<HeadGauss> { static constexpr bool value = true; };
// episode returns can be negative: the discrete kinds of env_signed_returns, and the Pendulum on a Gaussian handle
template <class Head>
__device__ __host__ __forceinline__ bool head_signed_returns(int kind) {
  if (head_is_gauss<Head>::value) return env_continuous(kind);
  return env_signed_returns(kind);
}

// A lane's running return_max. CartPole / synthetic keep max(0, ·) (their accumulator is ordered as an unsigned bit pattern, which holds for values >= 0);
// kinds whose returns can be negative (env_signed_returns) keep the true maximum of the lane's finished episodes: st_n says whether there was one yet.
__device__ __forceinline__ double step_stat_max_s(bool is_signed, double st_n, double st_max, double ep_ret) {
  if (!is_signed) return fmax(st_max, fmax(0.0, ep_ret));
  return st_n > 1.0 ? fmax(st_max, ep_ret) : ep_ret;
}
__device__ __forceinline__ double step_stat_max(int kind, double st_n, double st_max, double ep_ret) {
  return step_stat_max_s(env_signed_returns(kind), st_n, st_max, ep_ret);
}

// HeadGauss: the action of env e at buffer slot b — act_dim floats into the action plane and act[] — and its logπ (ppo_gauss.hpp's expressions, index order)
__device__ __forceinline__ float gauss_step_act(const WStepArgs& a, const HeadGauss& hd, int e, size_t b, uint32_t gid, uint64_t gstep, float (&act)[GAUSS_AMAX]) {
  const int ad = hd.g.ad;
  const float* z = a.Z + (size_t)a.A8 * e;
  float lpa = 0.0f;
#pragma unroll
  for (int i = 0; i < GAUSS_AMAX; ++i) {
    act[i] = 0.0f;
    if (i < ad) {
      float th;
      const float ls = gauss_log_std(hd.g, z[ad + i], th);
      const float xi = gauss_xi(a.c.seed, gid, gstep, i);
      act[i] = gauss_action(z[i], expf(ls), xi);
      lpa += gauss_lp_term(xi, ls);
      hd.action_f[b * (size_t)ad + i] = act[i];
    }
  }
  return lpa;
}

// one env, one step; the episode statistics of a finished episode are added to the caller's running sums. zreg: the env's logits when the caller holds them
// in registers (else they come from a.Z); xout: receives the env's next observation (16 floats, zero beyond obs_dim) besides cur_obs; a.V may be null (the
// caller fills the value buffer later: wide_rs_rollout_kernel). zreg / xout are the discrete head's (the Gaussian head runs on the per-step route only).
template <class Head>
__device__ __forceinline__ void wide_step_env(const WStepArgs& a, const Head& hd, int e, int step, double& st_n, double& st_ret, double& st_len, double& st_max,
                                              const float* zreg = nullptr, float* xout = nullptr) {
  constexpr bool GAUSS = head_is_gauss<Head>::value;
  const DevCfg& c = a.c;
  const int D = c.D, A = c.A;
  const uint32_t gid = c.env_id_offset + (uint32_t)e;
  const uint64_t gstep = a.iteration * (uint64_t)c.k + (uint64_t)step;
  const size_t b = (size_t)e + (size_t)c.nt * step;
  int ep_len = a.ep_length[e] + 1;                                   // ppo.jl:125
  int act = 0; float actf[GAUSS_AMAX]; float lpa;
  if constexpr (GAUSS) {
    lpa = gauss_step_act(a, hd, e, b, gid, gstep, actf);
  } else {
    float z[AMAX], p[AMAX], lp[AMAX];
    if (zreg) {
#pragma unroll
      for (int i = 0; i < AMAX; ++i) z[i] = (i < A && i < 8) ? zreg[i & 7] : 0.0f;
    } else load_logits(a.Z, a.A8, A, (size_t)e, z);
    softmax_rt(z, A, p, lp);                                          // ppo.jl:127 get_action
    const double u = u53(philox_env(c.seed, gid, gstep, 0));
    act = sample_rt(p, A, u);
    lpa = pick_rt(lp, A, act);
  }
  float* co = a.cur_obs + (size_t)D * e;
  float* es = a.env_state + (size_t)D * e;
  float* ob = a.obs + b * (size_t)D;
  for (int i = 0; i < D; ++i) ob[i] = co[i];                        // ppo.jl:133-140 Buffer.add!
  if constexpr (!GAUSS) a.action[b] = act;
  a.logprob[b] = lpa; a.terminal[b] = a.next_done[e]; if (a.V) a.value[b] = a.V[e];
  bool done; float rew;
  if (GAUSS ? env_continuous(c.env_kind) : env_stateful(c.env_kind)) {
    const int ns = GAUSS ? PENDULUM_STATE : env_state_dim(c.env_kind);
    float s[4], so[ENV_OBS_MAX];
#pragma unroll
    for (int i = 0; i < 4; ++i) s[i] = i < ns ? es[i] : 0.0f;
    int t_env = a.env_t[e];
    if constexpr (GAUSS) env_transition_c(c.env_kind, c.stale_obs, s, t_env, actf, c.seed, gid, gstep, so, rew, done);
    else env_transition(c.env_kind, c.stale_obs, s, t_env, act, c.seed, gid, gstep, so, rew, done);   // ppo.jl:130-132,143,164
#pragma unroll
    for (int i = 0; i < ENV_OBS_MAX; ++i) if (i < D) { co[i] = so[i]; es[i] = i < ns ? s[i] : 0.0f; }
    a.env_t[e] = t_env;
    if (xout) {
#pragma unroll
      for (int i = 0; i < 16; ++i) xout[i] = (i < ENV_OBS_MAX && i < D) ? so[i] : 0.0f;
    }
  } else {
    if (xout) {
#pragma unroll
      for (int i = 0; i < 16; ++i) xout[i] = 0.0f;
    }
    for (int q = 0; 4 * q < D; ++q) {
      float o4[4];
      synth_obs4(c.seed, gid, gstep, q, o4);
      for (int i = 0; i < 4 && 4 * q + i < D; ++i) { es[4 * q + i] = o4[i]; co[4 * q + i] = o4[i]; }
      if (xout) {                                                    // constant indices: the caller's array stays in registers
#pragma unroll
        for (int qq = 0; qq < 4; ++qq)
          if (q == qq) {
#pragma unroll
            for (int i = 0; i < 4; ++i) xout[4 * qq + i] = 4 * qq + i < D ? o4[i] : 0.0f;
          }
      }
    }
    synth_reward_done(c.seed, gid, gstep, rew, done);
  }
  a.reward[b] = rew;
  a.next_done[e] = done ? 1 : 0;                                     // ppo.jl:144
  float ep_ret = a.ep_return[e] + rew;                               // ppo.jl:145
  if (done) {                                                        // ppo.jl:147-165
    st_n += 1.0; st_ret += (double)ep_ret; st_len += (double)ep_len; st_max = step_stat_max_s(head_signed_returns<Head>(c.env_kind), st_n, st_max, (double)ep_ret);
    episode_ring_push(a.ring, a.ring_count, a.ring_cap, ep_ret, ep_len, gid, step);
    ep_ret = 0.0f; ep_len = 0;
  }
  a.ep_return[e] = ep_ret; a.ep_length[e] = ep_len;
}

}  // namespace crl
