// ppo_gauss.hpp — the diagonal Gaussian policy of a crl_ppo_create_gaussian handle, stated once: every expression include/cleanrl_hip.h pins for
// it, the Philox stream its rollout noise comes from, and the launchers of the kernels that use them (ppo_gauss.hip). The actor head has 2·act_dim
// rows, z = (μ, s) — as sac.hpp's — so the twelve-array parameter table, the forward / backward GEMMs, the reduce and the optimiser never learn what the
// head means. Float32 throughout, contraction off: a numpy Float32 restatement differs only by the device's tanhf / expf / log / cos.
#pragma once
#include "common.hpp"
#include "normal_bm.hpp"
#include "ppo_ctx.hpp"

namespace crl {

constexpr int GAUSS_AMAX = 8;                        // act_dim ≤ 8: the head's 2·act_dim rows fit AMAX = 16
constexpr uint32_t GAUSS_STREAM0 = 0x20u;            // ξ_i of (env, step) = Box–Muller of Philox block (seed, env id, gstep, 0x20 + i): streams 0x20 … 0x27
constexpr float GAUSS_HALF_LOG_2PI = 0.918938533204672742f;    // 0.5·log 2π
constexpr float GAUSS_ENT_CONST = 1.418938533204672742f;       // 0.5·(1 + log 2π)

struct GaussDist { int ad; float ls_min, ls_half; };  // act_dim, log_std_min, 0.5f·(log_std_max − log_std_min) as a Float32 product

// log_std = min + 0.5·(max − min)·(tanh(s) + 1); th receives tanh(s) (the update's 1 − tanh²). tanhf is the HIP device library's.
__device__ __forceinline__ float gauss_log_std(const GaussDist& g, float s, float& th) {
#pragma clang fp contract(off)
  th = tanhf(s);
  return g.ls_min + g.ls_half * (th + 1.0f);
}
// one component's term of logπ: −0.5·ξ² − log_std − 0.5·log 2π
__device__ __forceinline__ float gauss_lp_term(float xi, float ls) {
#pragma clang fp contract(off)
  return (-0.5f * (xi * xi) - ls) - GAUSS_HALF_LOG_2PI;
}
__device__ __forceinline__ float gauss_ent_term(float ls) { return ls + GAUSS_ENT_CONST; }
// a = μ + σ·ξ
__device__ __forceinline__ float gauss_action(float mu, float sigma, float xi) {
#pragma clang fp contract(off)
  return mu + sigma * xi;
}
// the rollout's ξ_i: normal_bm.hpp's Float64 Box–Muller on all four words of the env's own block, rounded to Float32
// — in two halves, so a caller may put other work between the integer block and the Float64 chain (wide_rs_rollout_gauss_kernel)
__device__ __forceinline__ u32x4 gauss_xi_block(uint64_t seed, uint32_t gid, uint64_t gstep, int i) {
  return philox_env(seed, gid, gstep, GAUSS_STREAM0 + (uint32_t)i);
}
__device__ __forceinline__ float gauss_xi_of(const u32x4& block) { return (float)box_muller(block); }
__device__ __forceinline__ float gauss_xi(uint64_t seed, uint32_t gid, uint64_t gstep, int i) { return gauss_xi_of(gauss_xi_block(seed, gid, gstep, i)); }

// the Gaussian head tag of wide_step_env (wide_step.hpp): where the float actions go and the distribution's constants
struct HeadGauss { GaussDist g; float* action_f; };

// the loss kernel's view (wide_loss_gauss_kernel): WLossArgs of wide.hip with the 64-byte records and the distribution
struct GaussLossArgs {
  int M, A8; float clip, ent_coeff, v_coef; int clip_vloss;
  const int32_t* perm; float* Z; const float* V; float* dv8; const float* rec;
  const double* adv_ms; int mb; const double* vfix; double Mglobal; double* lpart;
  GaussDist g;
};

inline GaussDist gauss_dist(const crl_ppo* h) { return GaussDist{h->act_dim, h->ls_min, 0.5f * (h->ls_max - h->ls_min)}; }

struct WStepArgs;
// launchers (ppo_gauss.hip); each returns after the enqueue
int gauss_env_reset(crl_ppo* h);                                                                              // crl_env_reset on CRL_ENV_PENDULUM
int gauss_env_step(crl_ppo* h, const float* action_d, uint64_t gstep, float* reward_d, uint8_t* done_d);      // crl_env_step_gaussian
void gauss_launch_step(hipStream_t st, const WStepArgs& a, const HeadGauss& hd);
void gauss_launch_sample(hipStream_t st, const GaussDist& g, const float* Z, int A8, const float* V, const float* xi, int n, float* action, float* logprob,
                         float* value);
void gauss_launch_logprob(hipStream_t st, const GaussDist& g, const float* Z, int A8, const float* actions, int n, float* logprob, float* entropy);
void gauss_launch_pack_rec(hipStream_t st, int B, int ad, const float* action_f, const float* logprob, const float* value, const float* adv, const float* ret,
                           float* rec);
void gauss_launch_loss(hipStream_t st, const GaussLossArgs& a, int nlb);

}  // namespace crl
