// stats.hpp — the "Training Statistics" record (ppo.jl:243-247) from the four loss sums of one optimiser step, the key return_max travels as, and
// the two pieces every rollout kernel ends an episode with: the per-episode record and the per-wave flush of the "Episode Statistics" sums.
#pragma once
#include "common.hpp"
#include "ppo_ctx.hpp"

namespace crl {

// "Training Statistics" (ppo.jl:247) from the (all-reduced) sums msg[P..P+3]; mode 0 also raises the value-loss
// speculation flag (u > 0), mode 1 is the re-evaluation after the exact critic pass.
__device__ __forceinline__ void compute_stats4(float s0, float s1, float s2, float s3, const DevCfg& c, double Mglobal, const double* adv_ms,
                                               int mb, double* vfix, crl_ppo_stats* out, int mode) {
  const double pg = (double)s0 / Mglobal;
  const double ent = (double)(float)((double)s1 / ((double)c.A * Mglobal));
  const double u = (double)(float)((double)s2 / Mglobal);
  const double vl = 0.5 * (double)(float)((double)s3 / Mglobal);
  if (mode == 0) {
    vfix[0] = u;
    vfix[3] = (c.clip_vloss && u > 0.0) ? 1.0 : 0.0;
    if (vfix[3] != 0.0) vfix[4] = 1.0;  // sticky: lets a data-parallel run fail loudly (no exact pass there yet)
    out->n_unclipped_wins = 0.0;
  } else {
    out->n_unclipped_wins = vfix[1];
  }
  out->pg_loss = pg; out->entropy_loss = ent; out->v_loss = vl; out->u_value = u;
  out->loss = pg - (double)(c.ent_coeff * (float)ent) + (double)c.v_coef * vl;
  out->adv_mean = (double)(float)adv_ms[2 * mb]; out->adv_std = (double)(float)adv_ms[2 * mb + 1];
}

__device__ __forceinline__ void compute_stats(const float* msg, int P, const DevCfg& c, double Mglobal, const double* adv_ms,
                                              int mb, double* vfix, crl_ppo_stats* out, int mode) {
  compute_stats4(msg[P], msg[P + 1], msg[P + 2], msg[P + 3], c, Mglobal, adv_ms, mb, vfix, out, mode);
}

// return_max of the env kinds whose episode returns can be negative (env_signed_returns, and CRL_ENV_EXTERNAL): ep_stats[3] holds an order-preserving map of
// the double onto u64 (never 0 for a number: 0 = "no episode yet", which is what the accumulator is cleared to), so one unsigned atomicMax keeps the maximum;
// the host maps what it reads back
__device__ __host__ __forceinline__ unsigned long long stat_max_key(double x) {
  unsigned long long b; __builtin_memcpy(&b, &x, 8);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __host__ __forceinline__ double stat_max_unkey(unsigned long long k) {
  if (k == 0) return 0.0;
  k = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  double x; __builtin_memcpy(&x, &k, 8);
  return x;
}

// ppo.jl:147-165 per-episode records (opt-in, ring_cap = 0: off): every episode end takes a slot; past the capacity it is counted, not stored
__device__ __forceinline__ void episode_ring_push(crl_episode_record* ring, uint32_t* ring_count, int ring_cap, float ep_ret, int ep_len, uint32_t gid, int step) {
  if (ring_cap > 0) {
    const uint32_t slot = atomicAdd(ring_count, 1u);
    if (slot < (uint32_t)ring_cap) ring[slot] = crl_episode_record{ep_ret, ep_len, (int32_t)gid, step};
  }
}

// A wave's episode statistics into the handle's four accumulators: one atomic set per wave that finished an episode. Called by whole waves; lanes without
// an env bring zeros. return_max: returns of the non-negative kinds (CartPole, synthetic) are ordered by their f64 bit pattern read as u64; is_signed (the
// env kind's returns can be negative: env_signed_returns, CRL_ENV_EXTERNAL) — lanes without a finished episode stand aside and the accumulator holds
// stat_max_key of the maximum, which the host maps back (api.cpp return_max_of).
__device__ __forceinline__ void episode_stats_flush(double* ep_stats, double st_n, double st_ret, double st_len, double st_max, bool is_signed = false) {
  if (is_signed && !(st_n > 0.0)) st_max = -__builtin_inf();
  st_n = wave_sum(st_n);
  if (st_n > 0.0) {
    st_ret = wave_sum(st_ret); st_len = wave_sum(st_len); st_max = wave_max(st_max);
    if ((threadIdx.x & 63) == 0) {
      atomicAdd(&ep_stats[0], st_n); atomicAdd(&ep_stats[1], st_ret); atomicAdd(&ep_stats[2], st_len);
      atomicMax(reinterpret_cast<unsigned long long*>(&ep_stats[3]), is_signed ? stat_max_key(st_max) : (unsigned long long)__double_as_longlong(st_max));
    }
  }
}

struct StatsArgs {
  DevCfg c; double Mglobal; const double* adv_ms; int mb; double* vfix; crl_ppo_stats* out;
  int fused;  // 1: the last block of reduce_kernel also writes the statistics (single-GPU: sums are already global)
  float* dscale;   // [4]: G actor, G critic, then (as unsigned) the launch's largest |δ2| per role — fp16x2 weight gradient
};

}  // namespace crl
