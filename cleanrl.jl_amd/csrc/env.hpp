// env.hpp — on-device environments: CartPoleEnv{Float32} (RLEnvs 0.6.12 semantics, ppo.jl:82), MountainCarEnv{Float32} and
// AcrobotEnv{Float32} (the two other discrete classic-control envs of the package ppo.jl:82 takes CartPoleEnv from), and the synthetic
// obs-d / reward / done generator used for shapes the reference has no env for (BASELINE config C3). env_transition is the one
// entry every stateful caller goes through (rollout kernels of the layer-wise path, crl_env_step, crl_env_reset).
#pragma once
#include "common.hpp"
#include "../../include/cleanrl_hip.h"

namespace crl {

// ------------------------------------------------------------------------------------------------------
// CartPoleEnv{Float32} step (RLEnvs 0.6.12 semantics; oracle/ppo_oracle.c:orc_cartpole_step is the restatement).
// Contraction is off and the promotions to Float64 follow the reference expression (`4 / 3` is a Float64 literal),
// so this is bit-identical to the CPU oracle.
// ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void store_nt4(f32x4* p, float a, float b, float c, float d) {
  f32x4 v; v[0] = a; v[1] = b; v[2] = c; v[3] = d;
  __builtin_nontemporal_store(v, p);
}

__device__ __forceinline__ float sin_poly(float x) {
  float x2 = x * x;
  float p = __builtin_fmaf(x2, __builtin_fmaf(x2, __builtin_fmaf(x2, 2.7557319e-6f, -1.9841270e-4f), 8.3333333e-3f), -1.6666667e-1f);
  return __builtin_fmaf(x * x2, p, x);
}
__device__ __forceinline__ float cos_poly(float x) {
  float x2 = x * x;
  float p = __builtin_fmaf(x2, __builtin_fmaf(x2, __builtin_fmaf(x2, 2.4801587e-5f, -1.3888889e-3f), 4.1666667e-2f), -0.5f);
  return __builtin_fmaf(x2, p, 1.0f);
}

__device__ __forceinline__ bool cartpole_step(float (&s)[4], int& t, int action) {
#pragma clang fp contract(off)
  const float gravity = 9.8f, masspole = 0.1f, totalmass = 1.1f, halflength = 0.5f, pml = 0.05f;
  const float forcemag = 10.0f, dt = 0.02f, ththr = 0.20943951f, xthr = 2.4f;
  t += 1;
  const float force = action == 1 ? forcemag : -forcemag;
  const float xdot = s[1], theta = s[2], thetadot = s[3];
  const float costheta = cos_poly(theta), sintheta = sin_poly(theta);
  const float tmp = (force + (pml * (thetadot * thetadot)) * sintheta) / totalmass;
  const float num = gravity * sintheta - costheta * tmp;
  const double den = (double)halflength * (4.0 / 3.0 - (double)((masspole * (costheta * costheta)) / totalmass));
  const double thetaacc = (double)num / den;
  const double xacc = (double)tmp - (((double)pml * thetaacc) * (double)costheta) / (double)totalmass;
  s[0] = s[0] + dt * xdot;
  s[1] = (float)((double)s[1] + (double)dt * xacc);
  s[2] = s[2] + dt * thetadot;
  s[3] = (float)((double)s[3] + (double)dt * thetaacc);
  return (fabsf(s[0]) > xthr) || (fabsf(s[2]) > ththr) || (t > 500);
}

__device__ __forceinline__ void cartpole_reset(float (&s)[4], uint64_t seed, uint32_t gid, uint64_t gstep, uint32_t stream) {
#pragma clang fp contract(off)
  u32x4 o = philox_env(seed, gid, gstep, stream);
  s[0] = 0.1f * ((float)(o.x >> 8) * 0x1.0p-24f) - 0.05f;
  s[1] = 0.1f * ((float)(o.y >> 8) * 0x1.0p-24f) - 0.05f;
  s[2] = 0.1f * ((float)(o.z >> 8) * 0x1.0p-24f) - 0.05f;
  s[3] = 0.1f * ((float)(o.w >> 8) * 0x1.0p-24f) - 0.05f;
}

// ------------------------------------------------------------------------------------------------------
// sin / cos for the two envs below: Cody–Waite reduction by π/2 (three FMA steps: exact for the |x| < ~1e3 an RK4 stage can reach from
// wrapped angles and clamped velocities) + the degree-7 / degree-8 minimax polynomials on [-π/4, π/4]; ≤ ~1.5 ulp. Plain Float32, one env
// per lane, no libm. (sin_poly / cos_poly above are CartPole's: valid near zero only, and pinned bit for bit by the oracle.)
// ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void sincos_f32(float x, float& sn, float& cs) {
  const float kf = __builtin_rintf(x * 0.63661977236758134f);
  float r = __builtin_fmaf(-kf, 1.5707962513e+0f, x);
  r = __builtin_fmaf(-kf, 7.5497894159e-8f, r);
  r = __builtin_fmaf(-kf, 5.3903029534e-15f, r);
  const int k = (int)kf;
  const float r2 = r * r;
  const float ps = __builtin_fmaf(r2, __builtin_fmaf(r2, -1.9515295891e-4f, 8.3321608736e-3f), -1.6666654611e-1f);
  const float s = __builtin_fmaf(r * r2, ps, r);
  const float pc = __builtin_fmaf(r2, __builtin_fmaf(r2, 2.443315711809948e-5f, -1.388731625493765e-3f), 4.166664568298827e-2f);
  const float c = __builtin_fmaf(r2 * r2, pc, __builtin_fmaf(r2, -0.5f, 1.0f));
  const float ss = (k & 1) ? c : s, cc = (k & 1) ? s : c;
  sn = (k & 2) ? -ss : ss;
  cs = ((k + 1) & 2) ? -cc : cc;
}
__device__ __forceinline__ float sin_f32(float x) { float s, c; sincos_f32(x, s, c); return s; }
__device__ __forceinline__ float cos_f32(float x) { float s, c; sincos_f32(x, s, c); return c; }

// ------------------------------------------------------------------------------------------------------
// MountainCarEnv{Float32} / AcrobotEnv{Float32}: discrete actions {0, 1, 2} -> command a - 1, max_steps = 200, done = goal || t >= max_steps,
// reward = done ? 0 : -1 (CartPole's `done ? 0 : 1` pattern). PARITY UNPINNED: the RLEnvs source is not available to this project; the
// contracts are restated from RLEnvs 0.6.12 / Gym MountainCar-v0 / Acrobot-v1 as recalled (tests/envs_ref.py is the independent Float64
// restatement the kernels are tested against; VERIFY_WITH_JULIA.md lists what a Julia owner must compare). Contraction off, as in cartpole_step.
// ------------------------------------------------------------------------------------------------------
constexpr int ENV_MAX_STEPS_CC = 200;

// state (x, v) = observation
__device__ __forceinline__ bool mountaincar_step(float (&s)[4], int& t, int action) {
#pragma clang fp contract(off)
  t += 1;
  float x = s[0], v = s[1];
  v = v + ((float)(action - 1) * 0.001f + cos_f32(3.0f * x) * -0.0025f);
  v = fminf(fmaxf(v, -0.07f), 0.07f);
  x = x + v;
  x = fminf(fmaxf(x, -1.2f), 0.6f);
  if (x == -1.2f && v < 0.0f) v = 0.0f;
  s[0] = x; s[1] = v;
  return (x >= 0.5f && v >= 0.0f) || t >= ENV_MAX_STEPS_CC;
}
__device__ __forceinline__ void mountaincar_reset(float (&s)[4], uint64_t seed, uint32_t gid, uint64_t gstep, uint32_t stream) {
#pragma clang fp contract(off)
  const u32x4 o = philox_env(seed, gid, gstep, stream);
  s[0] = 0.2f * ((float)(o.x >> 8) * 0x1.0p-24f) - 0.6f;
  s[1] = 0.0f; s[2] = 0.0f; s[3] = 0.0f;
}

// state (θ1, θ2, ω1, ω2); the "book" equations of motion with link lengths, masses and the moment of inertia 1, centres of mass at 0.5
__device__ __forceinline__ void acrobot_dsdt(const float (&y)[4], float tau, float (&d)[4]) {
#pragma clang fp contract(off)
  const float m1 = 1.0f, m2 = 1.0f, l1 = 1.0f, lc1 = 0.5f, lc2 = 0.5f, I1 = 1.0f, I2 = 1.0f, g = 9.8f, hpi = 1.57079632679489662f;
  const float th1 = y[0], th2 = y[1], w1 = y[2], w2 = y[3];
  float s2, c2;
  sincos_f32(th2, s2, c2);
  const float d1 = m1 * (lc1 * lc1) + m2 * (l1 * l1 + lc2 * lc2 + 2.0f * l1 * lc2 * c2) + I1 + I2;
  const float d2 = m2 * (lc2 * lc2 + l1 * lc2 * c2) + I2;
  const float phi2 = m2 * lc2 * g * cos_f32(th1 + th2 - hpi);
  const float phi1 = -m2 * l1 * lc2 * (w2 * w2) * s2 - 2.0f * m2 * l1 * lc2 * w2 * w1 * s2 + (m1 * lc1 + m2 * l1) * g * cos_f32(th1 - hpi) + phi2;
  const float dw2 = (tau + d2 / d1 * phi1 - m2 * l1 * lc2 * (w1 * w1) * s2 - phi2) / (m2 * (lc2 * lc2) + I2 - (d2 * d2) / d1);
  const float dw1 = -(d2 * dw2 + phi1) / d1;
  d[0] = w1; d[1] = w2; d[2] = dw1; d[3] = dw2;
}
__device__ __forceinline__ float wrap_pi(float x) {            // into [-π, π)
#pragma clang fp contract(off)
  const float pi = 3.14159265358979324f, two_pi = 6.28318530717958648f;
  x = x - two_pi * floorf((x + pi) / two_pi);
  if (x >= pi) x = x - two_pi;
  if (x < -pi) x = x + two_pi;
  return x;
}
__device__ __forceinline__ bool acrobot_step(float (&s)[4], int& t, int action) {
#pragma clang fp contract(off)
  const float dt = 0.2f, hdt = 0.1f, dt6 = 0.2f / 6.0f, w1max = 12.5663706143591730f, w2max = 28.2743338823081391f;
  t += 1;
  const float tau = (float)(action - 1);
  float k1[4], k2[4], k3[4], k4[4], y[4];
  acrobot_dsdt(s, tau, k1);                                    // one classical RK4 step, torque held constant
#pragma unroll
  for (int i = 0; i < 4; ++i) y[i] = s[i] + hdt * k1[i];
  acrobot_dsdt(y, tau, k2);
#pragma unroll
  for (int i = 0; i < 4; ++i) y[i] = s[i] + hdt * k2[i];
  acrobot_dsdt(y, tau, k3);
#pragma unroll
  for (int i = 0; i < 4; ++i) y[i] = s[i] + dt * k3[i];
  acrobot_dsdt(y, tau, k4);
#pragma unroll
  for (int i = 0; i < 4; ++i) y[i] = s[i] + dt6 * (k1[i] + 2.0f * k2[i] + 2.0f * k3[i] + k4[i]);
  s[0] = wrap_pi(y[0]); s[1] = wrap_pi(y[1]);
  s[2] = fminf(fmaxf(y[2], -w1max), w1max); s[3] = fminf(fmaxf(y[3], -w2max), w2max);
  const bool goal = -cos_f32(s[0]) - cos_f32(s[0] + s[1]) > 1.0f;
  return goal || t >= ENV_MAX_STEPS_CC;
}
__device__ __forceinline__ void acrobot_reset(float (&s)[4], uint64_t seed, uint32_t gid, uint64_t gstep, uint32_t stream) {
#pragma clang fp contract(off)
  const u32x4 o = philox_env(seed, gid, gstep, stream);
  s[0] = 0.2f * ((float)(o.x >> 8) * 0x1.0p-24f) - 0.1f;
  s[1] = 0.2f * ((float)(o.y >> 8) * 0x1.0p-24f) - 0.1f;
  s[2] = 0.2f * ((float)(o.z >> 8) * 0x1.0p-24f) - 0.1f;
  s[3] = 0.2f * ((float)(o.w >> 8) * 0x1.0p-24f) - 0.1f;
}

// ------------------------------------------------------------------------------------------------------
// The dispatcher. A stateful env keeps at most four state words (the first words of its CRL_F_ENV_STATE column) and shows at most
// ENV_OBS_MAX observation words. `kind` is uniform over a launch, so the switch is a scalar branch; for CRL_ENV_CARTPOLE every function
// below reduces to the call it replaced (observation = state, reward = done ? 0 : 1).
// ------------------------------------------------------------------------------------------------------
constexpr int ENV_OBS_MAX = 8;
__device__ __host__ __forceinline__ bool env_stateful(int kind) { return kind == CRL_ENV_CARTPOLE || kind == CRL_ENV_MOUNTAINCAR || kind == CRL_ENV_ACROBOT; }
__device__ __host__ __forceinline__ int env_state_dim(int kind) { return kind == CRL_ENV_MOUNTAINCAR ? 2 : 4; }
// episode returns of these kinds can be negative: return_max travels as an order-preserving key (stats.hpp: episode_stats_flush)
__device__ __host__ __forceinline__ bool env_signed_returns(int kind) { return kind == CRL_ENV_MOUNTAINCAR || kind == CRL_ENV_ACROBOT; }

__device__ __forceinline__ void env_observe(int kind, const float (&s)[4], float (&o)[ENV_OBS_MAX]) {
#pragma unroll
  for (int i = 0; i < ENV_OBS_MAX; ++i) o[i] = i < 4 ? s[i] : 0.0f;
  if (kind == CRL_ENV_ACROBOT) {
    float s1, c1, s2, c2;
    sincos_f32(s[0], s1, c1); sincos_f32(s[1], s2, c2);
    o[0] = c1; o[1] = s1; o[2] = c2; o[3] = s2; o[4] = s[2]; o[5] = s[3];
  }
}
__device__ __forceinline__ void env_reset(int kind, float (&s)[4], uint64_t seed, uint32_t gid, uint64_t gstep, uint32_t stream) {
  if (kind == CRL_ENV_ACROBOT) acrobot_reset(s, seed, gid, gstep, stream);
  else if (kind == CRL_ENV_MOUNTAINCAR) mountaincar_reset(s, seed, gid, gstep, stream);
  else cartpole_reset(s, seed, gid, gstep, stream);
}
// env(action); reward; is_terminated (ppo.jl:130-132)
__device__ __forceinline__ void env_step(int kind, float (&s)[4], int& t, int action, float& reward, bool& done) {
  if (kind == CRL_ENV_ACROBOT) { done = acrobot_step(s, t, action); reward = done ? 0.0f : -1.0f; }
  else if (kind == CRL_ENV_MOUNTAINCAR) { done = mountaincar_step(s, t, action); reward = done ? 0.0f : -1.0f; }
  else { done = cartpole_step(s, t, action); reward = done ? 0.0f : 1.0f; }
}
// One transition as the rollout loop sees it (ppo.jl:130-132,143,164): step, observe, and reset!(env) of a terminated env from its own Philox
// stream (gstep keys it). The observation handed on is the one taken BEFORE the reset when stale_obs is set (Q7), else the fresh state's.
__device__ __forceinline__ void env_transition(int kind, int stale_obs, float (&s)[4], int& t, int action, uint64_t seed, uint32_t gid,
                                               uint64_t gstep, float (&obs)[ENV_OBS_MAX], float& reward, bool& done) {
  env_step(kind, s, t, action, reward, done);
  env_observe(kind, s, obs);
  if (done) {
    env_reset(kind, s, seed, gid, gstep, 1);
    t = 0;
    if (!stale_obs) env_observe(kind, s, obs);
  }
}

// Synthetic env (oracle: synth_step): obs ~ U(-1,1)^d, reward ~ U(-1,1), done ~ Bernoulli(1/200), all from the env's
// own Philox stream (streams 8+q for the observation quads, 3 for reward/done). Stateless: a "reset" is a no-op.
__device__ __forceinline__ float synth_unit(uint32_t o) { return (float)(o >> 8) * 0x1.0p-23f - 1.0f; }
__device__ __forceinline__ void synth_obs4(uint64_t seed, uint32_t gid, uint64_t gstep, int q, float (&o4)[4]) {
  const u32x4 o = philox_env(seed, gid, gstep, 8u + (uint32_t)q);
  o4[0] = synth_unit(o.x); o4[1] = synth_unit(o.y); o4[2] = synth_unit(o.z); o4[3] = synth_unit(o.w);
}
__device__ __forceinline__ void synth_reward_done(uint64_t seed, uint32_t gid, uint64_t gstep, float& reward, bool& done) {
  const u32x4 o = philox_env(seed, gid, gstep, 3u);
  reward = synth_unit(o.x);
  done = (o.y % 200u) == 0u;
}

}  // namespace crl
