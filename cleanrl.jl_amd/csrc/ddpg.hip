// ddpg.hip — src/algorithms/ddpg.jl on the GPU (C ABI: the crl_ddpg_* block of include/cleanrl_hip.h).
//
// The reference steps ONE env and, once global_step > max(min_buff_size, warmup_steps), runs one 120-sample update per env step
// (ddpg.jl:76-135). As in dqn.hip the loop body is a fixed sequence of launches, every decision is taken on the device (kernels
// early-exit on the control block) and crl_ddpg_run enqueues the cycles of a chunk without reading anything back. One cycle:
//   A ddpg_sample_kernel   Buffer.sample (ddpg.jl:106): replay_sample.hpp, the draw dqn.hip uses
//   B ddpg_critic_kernel   one wave per sample, lane = hidden unit: target actor → target critic → TD target (:108-110); critic
//                          forward, (td − q)², ∂loss/∂q, δ2, δ1 (:114-117)
//   C ddpg_critic_step     one critic parameter per thread: gradient summed over the samples in sample order, Float32 projection, Adam
//                          (:118) and polyak (:129) on that element; thread 0 sums the loss in sample order
//   D ddpg_actor_kernel    one wave per sample: actor forward → UPDATED critic forward → back through the critic to ∂Q/∂a → actor δ3,
//                          δ2, δ1 (:122-124); tanh_fast' = 1 − y² from the stored activation
//   E ddpg_actor_step      one actor parameter per thread: as C (:125, :128)
//   F ddpg_collect_kernel  closes the update (β powers, n_updates, loss record :131-133, train_pending = 0 — by ONE thread, after every block
//                          of C and E is done), then env steps (:77-101) until an update is due; the warm-up runs inside one launch
// Six dependent launches per env step; ordering between phases is by launch boundaries only (no cooperative grid, no Float64 atomics).
// Float32 weights, Float64 arithmetic like a2c.hip / dqn.hip; contraction is off wherever a sum is formed; every sum has a fixed order:
// dot products in input order with the bias last, sums over the batch in sample order ⇒ two runs from one seed are bit-identical.
//
// Philox streams (counter = philox_env(seed, component, global_step, stream)): 0x10 behaviour noise (:79), 0x11 warm-up rand(act_space) (:79),
// 0x12 target-actor noise (:108), 0x13 actor-loss noise (:123), 0x14 Pendulum reset in the loop (:100), 0x15 the first reset (:74), 0x16 the
// resets of crl_ddpg_evaluate's private envs (no reference counterpart), 0x17 TD3's target smoothing (per sample: component word 16·b + c), 0x18 / 0x19 the
// ε of SAC's next action / actor pass (sac.hpp, the same component word), 0xD9 the minibatch draw. A normal is Box–Muller in Float64 from the two
// u53 halves of ONE Philox block: sqrt(−2·log(1 − u_xy))·cos(2π·u_zw).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "common.hpp"
#include "normal_bm.hpp"
#include "optim.hpp"
#include "ppo_ctx.hpp"
#include "replay_sample.hpp"
#include "tanh64.hpp"

struct crl_ddpg;

namespace crl {

constexpr int GH = 64;                          // hidden width, ddpg.jl:24-25,31-32
constexpr int DDPG_MAX_OBS = 64, DDPG_MAX_ACT = 16, DDPG_MAX_IN = DDPG_MAX_OBS + DDPG_MAX_ACT;
constexpr int DDPG_MAX_EPS = 8192, DDPG_MAX_LOSSES = 4096, DDPG_MAX_BATCH = 1024, DDPG_MAX_CAP = 1 << 17;   // ring: reference default 1e5
constexpr uint32_t S_BEHAVE = 0x10u, S_WARMUP = 0x11u, S_TARGET = 0x12u, S_ACTOR = 0x13u, S_RESET = 0x14u, S_RESET0 = 0x15u, S_EVAL = 0x16u, S_SMOOTH = 0x17u;

// Dense(n_in, 64, ·) → Dense(64, 64, ·) → Dense(64, n_out, ·), flat in Flux.params order, (out,in) column-major
struct NetOff { int W1, b1, W2, b2, W3, b3, N; };
__host__ __device__ inline NetOff net_off(int n_in, int n_out) {
  NetOff o;
  o.W1 = 0; o.b1 = GH * n_in; o.W2 = o.b1 + GH; o.b2 = o.W2 + GH * GH; o.W3 = o.b2 + GH; o.b3 = o.W3 + n_out * GH; o.N = o.b3 + n_out;
  return o;
}
__host__ __device__ inline int net_array(const NetOff& o, int p) { return p < o.b1 ? 0 : p < o.W2 ? 1 : p < o.b2 ? 2 : p < o.W3 ? 3 : p < o.b3 ? 4 : 5; }

struct DDPGCtl {
  double env[2]; double episode_return, actor_loss, critic_loss;
  int64_t global_step, episode_length, n_updates, taken, ptr, size, budget;
  int32_t env_t, n_eps, n_losses, train_pending;
};

struct DDPGDev {
  crl_ddpg_config cfg;
  float *actor, *critic, *actor_t, *critic_t, *ma, *va, *mc, *vc; double* betap;   // betap: [12][2], the actor's six arrays then the critic's
  DDPGCtl* ctl; crl_ddpg_episode* eps; crl_ddpg_loss_record* losses;
  double *rb_state, *rb_action, *rb_reward, *rb_next; uint8_t* rb_terminal;
  int32_t* idx;                                                   // [k] minibatch slots
  double *X, *cH1, *cH2, *cD1, *cD2, *dz, *sq;                    // critic pass: [k][obs+act] input, [k][64] each, [k], [k]
  double *aH1, *aH2, *aY, *aD1, *aD2, *aD3, *Qa;                  // actor pass: [k][64], [k][64], [k][act] tanh outputs, δ1, δ2, δ3, [k] Q(s, μ(s))
  double* stage;                                                  // external env: obs | action | reward | next_obs | terminal, then act's output
};

// ------------------------------------------------------------------------------------------------------
// Pendulum, Float64 (beside env64.hpp's cartpole_step64; dynamics "parity unpinned"). sin / cos are Taylor polynomials in Horner form with PLAIN
// multiplies and adds (no fma: a numpy restatement is then bit-for-bit). 14 terms each: the first dropped term at |θ| = π is π³¹/31! ≈ 3.1e-19
// (sin) and π³⁰/30! ≈ 3.1e-18 (cos) — below one ulp of 1; the error that remains is the rounding of the Horner steps, whose terms reach ≈ 5 near π.
// ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double pend_sin(double x) {
#pragma clang fp contract(off)
  const double c[14] = {-1.0 / 6.0, 1.0 / 120.0, -1.0 / 5040.0, 1.0 / 362880.0, -1.0 / 39916800.0, 1.0 / 6227020800.0, -1.0 / 1307674368000.0,
                        1.0 / 355687428096000.0, -1.0 / 121645100408832000.0, 1.0 / 51090942171709440000.0, -1.0 / 25852016738884976640000.0,
                        1.0 / 15511210043330985984000000.0, -1.0 / 10888869450418352160768000000.0, 1.0 / 8841761993739701954543616000000.0};
  const double x2 = x * x;
  double p = c[13];
#pragma unroll
  for (int i = 12; i >= 0; --i) p = p * x2 + c[i];
  return x + (x * x2) * p;
}
__device__ __forceinline__ double pend_cos(double x) {
#pragma clang fp contract(off)
  const double c[14] = {-1.0 / 2.0, 1.0 / 24.0, -1.0 / 720.0, 1.0 / 40320.0, -1.0 / 3628800.0, 1.0 / 479001600.0, -1.0 / 87178291200.0,
                        1.0 / 20922789888000.0, -1.0 / 6402373705728000.0, 1.0 / 2432902008176640000.0, -1.0 / 1124000727777607680000.0,
                        1.0 / 620448401733239439360000.0, -1.0 / 403291461126605635584000000.0, 1.0 / 304888344611713860501504000000.0};
  const double x2 = x * x;
  double p = c[13];
#pragma unroll
  for (int i = 12; i >= 0; --i) p = p * x2 + c[i];
  return 1.0 + x2 * p;
}
// s = (θ, θ̇), θ held in [−π, π); returns done = terminal = t >= max_steps; reward = −cost of the state BEFORE the step
__device__ __forceinline__ bool pendulum_step64(double* s, int& t, double a0, int max_steps, double& reward) {
#pragma clang fp contract(off)
  const double PI = 3.141592653589793, dt = 0.05;
  const double th = s[0], thd = s[1];
  const double u = a0 < -2.0 ? -2.0 : (a0 > 2.0 ? 2.0 : a0);
  const double cost = th * th + 0.1 * (thd * thd) + 0.001 * (u * u);
  double nthd = thd + (15.0 * pend_sin(th) + 3.0 * u) * dt;
  nthd = nthd < -8.0 ? -8.0 : (nthd > 8.0 ? 8.0 : nthd);
  double nth = th + nthd * dt;
  if (nth >= PI) nth -= 2.0 * PI; else if (nth < -PI) nth += 2.0 * PI;
  s[0] = nth; s[1] = nthd;
  t += 1;
  reward = -cost;
  return t >= max_steps;
}
__device__ __forceinline__ void pendulum_reset64(double* s, uint64_t seed, uint64_t gstep, uint32_t stream) {
#pragma clang fp contract(off)
  const double PI = 3.141592653589793;
  s[0] = -PI + (2.0 * PI) * u53(philox_env(seed, 0u, gstep, stream));
  s[1] = -1.0 + 2.0 * u53(philox_env(seed, 1u, gstep, stream));
}

// randn() for component `comp` of the draw (gstep, stream)
__device__ __forceinline__ double ddpg_normal(uint64_t seed, uint32_t comp, uint64_t gstep, uint32_t stream) {
#pragma clang fp contract(off)
  return box_muller(philox_env(seed, comp, gstep, stream));   // normal_bm.hpp
}

// ------------------------------------------------------------------------------------------------------
// One sample on one wave, lane = unit. x, hs: LDS. Every dot product adds its terms in input order and the bias last.
// ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double dense_row(const float* __restrict__ W, const float* __restrict__ b, int n_in, const double* x, int lane) {
#pragma clang fp contract(off)
  double acc = 0.0;
  for (int k = 0; k < n_in; ++k) acc += (double)W[lane + GH * k] * x[k];
  acc += (double)b[lane];
  return acc;
}
__device__ __forceinline__ double head_row(const float* __restrict__ W3, const float* __restrict__ b3, int n_out, const double* h, int a) {
#pragma clang fp contract(off)
  double acc = 0.0;
#pragma unroll 8
  for (int k = 0; k < GH; ++k) acc += (double)W3[a + n_out * k] * h[k];
  return acc + (double)b3[a];
}
// Σ_j W2[j, i]·d[j] on lane i, j ascending: the pullback of the hidden Dense(64, 64)
__device__ __forceinline__ double w2t_row(const float* __restrict__ W2, const double* d, int lane) {
#pragma clang fp contract(off)
  double s = 0.0;
#pragma unroll 8
  for (int j = 0; j < GH; ++j) s += (double)W2[j + GH * lane] * d[j];
  return s;
}
// the two tanh_fast layers of an actor whose offsets are o (ddpg.jl:24-25): h1, h2 returned per lane and left in h1s / h2s
__device__ __forceinline__ void actor_hidden(const float* __restrict__ P, const NetOff& o, int D, const double* x, double* h1s, double* h2s, int lane,
                                             double& h1, double& h2) {
  h1 = tanh_fast64(dense_row(P + o.W1, P + o.b1, D, x, lane));
  h1s[lane] = h1;
  __syncthreads();
  h2 = tanh_fast64(dense_row(P + o.W2, P + o.b2, GH, h1s, lane));
  h2s[lane] = h2;
  __syncthreads();
}
// actor(x) without the ·2 + noise: h1, h2 (returned per lane and left in h1s / h2s), ys[a] = tanh_fast(z3[a])   (ddpg.jl:24-26)
__device__ __forceinline__ void actor_forward(const float* __restrict__ P, int D, int A, const double* x, double* h1s, double* h2s, double* ys,
                                              int lane, double& h1, double& h2) {
  const NetOff o = net_off(D, A);
  actor_hidden(P, o, D, x, h1s, h2s, lane, h1, h2);
  if (lane < A) ys[lane] = tanh_fast64(head_row(P + o.W3, P + o.b3, A, h2s, lane));
  __syncthreads();
}
// what stands between two layers of a forward: the block's barrier where the wave is the whole block; where several waves share a block and each
// owns its x / h1s / h2s / qs, a wave-private fence (a wave's LDS instructions execute in issue order), so that no wave waits for another
template <bool BLOCK>
__device__ __forceinline__ void layer_sync() {
  if constexpr (BLOCK) __syncthreads(); else wave_lds_fence();
}
// critic(vcat(obs, act)) (ddpg.jl:31-33,45): x holds the D + A inputs; the value lands in *qs (LDS) for every lane
template <bool BLOCK = true>
__device__ __forceinline__ double critic_forward(const float* __restrict__ P, int n_in, const double* x, double* h1s, double* h2s, double* qs,
                                                 int lane, double& h1, double& h2) {
  const NetOff o = net_off(n_in, 1);
  double z = dense_row(P + o.W1, P + o.b1, n_in, x, lane);
  h1 = z > 0.0 ? z : 0.0;
  h1s[lane] = h1;
  layer_sync<BLOCK>();
  z = dense_row(P + o.W2, P + o.b2, GH, h1s, lane);
  h2 = z > 0.0 ? z : 0.0;
  h2s[lane] = h2;
  layer_sync<BLOCK>();
  if (lane == 0) *qs = head_row(P + o.W3, P + o.b3, 1, h2s, 0);
  layer_sync<BLOCK>();
  return *qs;
}

__global__ void ddpg_begin_kernel(DDPGDev a, int64_t max_env_steps) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  a.ctl->n_eps = 0; a.ctl->n_losses = 0; a.ctl->taken = 0; a.ctl->budget = max_env_steps;
}
__global__ void ddpg_clear_losses_kernel(DDPGDev a) {
  if (threadIdx.x == 0 && blockIdx.x == 0) a.ctl->n_losses = 0;
}

// A. Buffer.sample(rb, batch_size) (ddpg.jl:106)
__global__ void __launch_bounds__(1024) ddpg_sample_kernel(DDPGDev a) {
  if (!a.ctl->train_pending) return;
  replay_sample<DDPG_MAX_CAP>(a.cfg.seed, (uint64_t)a.ctl->global_step, (int)a.ctl->size, (int)a.cfg.batch_size, a.idx);
}

// B. ddpg.jl:108-117 for sample blockIdx.x
__global__ void __launch_bounds__(64) ddpg_critic_kernel(DDPGDev a) {
#pragma clang fp contract(off)
  if (!a.ctl->train_pending) return;
  __shared__ double xs[DDPG_MAX_IN], h1s[GH], h2s[GH], ys[DDPG_MAX_ACT], qs, d2s[GH];
  const int lane = threadIdx.x, b = blockIdx.x, D = a.cfg.obs_dim, A = a.cfg.act_dim, NI = D + A, k = (int)a.cfg.batch_size;
  const uint64_t gstep = (uint64_t)a.ctl->global_step;
  const size_t s = (size_t)a.idx[b];
  double h1, h2;
  // next_acts = target_actor(next_state) (:108), next_q = get_q(target_critic, next_state, next_acts) (:109)
  for (int i = lane; i < D; i += GH) xs[i] = a.rb_next[D * s + i];
  __syncthreads();
  actor_forward(a.actor_t, D, A, xs, h1s, h2s, ys, lane, h1, h2);
  if (lane < A) {
    const double nz = a.cfg.noise_in_update ? ddpg_normal(a.cfg.seed, (uint32_t)lane, gstep, S_TARGET) * a.cfg.exploration_noise : 0.0;
    xs[D + lane] = ys[lane] * 2.0 + nz;                                               // ddpg.jl:28
  }
  __syncthreads();
  const double next_q = critic_forward(a.critic_t, NI, xs, h1s, h2s, &qs, lane, h1, h2);
  const double td = a.rb_reward[s] + a.cfg.gamma * next_q * (1.0 - (double)a.rb_terminal[s]);   // :110
  __syncthreads();
  // q = get_q(critic, state, action); Flux.mse(td_target, q) (:115-116)
  for (int i = lane; i < NI; i += GH) {
    const double v = i < D ? a.rb_state[D * s + i] : a.rb_action[A * s + (i - D)];
    xs[i] = v; a.X[(size_t)NI * b + i] = v;
  }
  __syncthreads();
  const double q = critic_forward(a.critic, NI, xs, h1s, h2s, &qs, lane, h1, h2);
  const double diff = td - q;
  const double dq = -2.0 * diff / (double)k;
  const NetOff o = net_off(NI, 1);
  const double d2 = h2 > 0.0 ? (double)a.critic[o.W3 + lane] * dq : 0.0;
  d2s[lane] = d2;
  __syncthreads();
  const double t1 = w2t_row(a.critic + o.W2, d2s, lane);
  const double d1 = h1 > 0.0 ? t1 : 0.0;
  const size_t r = (size_t)GH * b + lane;
  a.cH1[r] = h1; a.cH2[r] = h2; a.cD1[r] = d1; a.cD2[r] = d2;
  if (lane == 0) { a.sq[b] = diff * diff; a.dz[b] = dq; }
}

// Adam(lr) on element p (ddpg.jl:55-56,118,125: optim.hpp's entry step without the clip) and polyak_update! on the same element (:39-43)
__device__ __forceinline__ void ddpg_step_entry(double g, float* w, float* t, float* m, float* v, const double* bp, double lr, double tau, int p) {
#pragma clang fp contract(off)
  float mi, vi, wi;
  adam_entry((double)(float)g, m[p], v[p], w[p], bp[0], bp[1], lr, /*clip=*/false, 1.0, mi, vi, wi);
  m[p] = mi; v[p] = vi; w[p] = wi;
  t[p] = (float)(tau * (double)wi + (1.0 - tau) * (double)t[p]);
}

// the gradient of critic parameter p from one critic pass's buffers: act = offset of its [k][64] blocks, row = offset of its [k] rows (both 0 for DDPG;
// TD3's second critic sits one block further). Every loop is unrolled 30x as in dqn_wgrad_kernel: the operands were written by the launch before,
// 30 loads in flight per round trip; the Float64 adds stay in sample order
__device__ __forceinline__ double critic_param_grad(const DDPGDev& a, const NetOff& o, int NI, int k, int p, size_t act, size_t row) {
#pragma clang fp contract(off)
  const double *cH1 = a.cH1 + act, *cH2 = a.cH2 + act, *cD1 = a.cD1 + act, *cD2 = a.cD2 + act, *dz = a.dz + row;
  double g = 0.0;
  if (p < o.b1) {
    const int i = p % GH, kk = p / GH;
#pragma unroll 30
    for (int b = 0; b < k; ++b) g += cD1[(size_t)GH * b + i] * a.X[(size_t)NI * b + kk];
  } else if (p < o.W2) {
    const int i = p - o.b1;
#pragma unroll 30
    for (int b = 0; b < k; ++b) g += cD1[(size_t)GH * b + i];
  } else if (p < o.b2) {
    const int r = p - o.W2, j = r % GH, kk = r / GH;
#pragma unroll 30
    for (int b = 0; b < k; ++b) g += cD2[(size_t)GH * b + j] * cH1[(size_t)GH * b + kk];
  } else if (p < o.W3) {
    const int j = p - o.b2;
#pragma unroll 30
    for (int b = 0; b < k; ++b) g += cD2[(size_t)GH * b + j];
  } else if (p < o.b3) {
    const int j = p - o.W3;
#pragma unroll 30
    for (int b = 0; b < k; ++b) g += dz[b] * cH2[(size_t)GH * b + j];
  } else {
#pragma unroll 30
    for (int b = 0; b < k; ++b) g += dz[b];
  }
  return g;
}

// C. critic gradient, Adam, polyak: one parameter per thread, samples in sample order
__global__ void __launch_bounds__(64) ddpg_critic_step(DDPGDev a) {
#pragma clang fp contract(off)
  if (!a.ctl->train_pending) return;
  const int k = (int)a.cfg.batch_size, NI = a.cfg.obs_dim + a.cfg.act_dim, p = blockIdx.x * 64 + threadIdx.x;
  const NetOff o = net_off(NI, 1);
  if (p == 0) {                                                                        // critic_loss = mean((td − q)²) (:114-116)
    double loss = 0.0;
    for (int b = 0; b < k; ++b) loss += a.sq[b];
    a.ctl->critic_loss = loss / (double)k;
  }
  if (p >= o.N) return;
  const double g = critic_param_grad(a, o, NI, k, p, 0, 0);
  ddpg_step_entry(g, a.critic, a.critic_t, a.mc, a.vc, a.betap + 2 * (6 + net_array(o, p)), a.cfg.lr, a.cfg.tau, p);
}

// D. ddpg.jl:122-124 for sample blockIdx.x: −mean(get_q(critic, state, actor(state))) through the updated critic, gradient w.r.t. the actor
__device__ __forceinline__ void ddpg_actor_pass(const DDPGDev& a) {
#pragma clang fp contract(off)
  __shared__ double xs[DDPG_MAX_IN], h1s[GH], h2s[GH], ys[DDPG_MAX_ACT], qs, ds[GH], d3s[DDPG_MAX_ACT];
  const int lane = threadIdx.x, b = blockIdx.x, D = a.cfg.obs_dim, A = a.cfg.act_dim, NI = D + A, k = (int)a.cfg.batch_size;
  const uint64_t gstep = (uint64_t)a.ctl->global_step;
  const NetOff oa = net_off(D, A), oc = net_off(NI, 1);
  double ah1, ah2, ch1, ch2;
  for (int i = lane; i < D; i += GH) xs[i] = a.X[(size_t)NI * b + i];
  __syncthreads();
  actor_forward(a.actor, D, A, xs, h1s, h2s, ys, lane, ah1, ah2);
  double y3 = 0.0;
  if (lane < A) {
    y3 = ys[lane];
    const double nz = a.cfg.noise_in_update ? ddpg_normal(a.cfg.seed, (uint32_t)lane, gstep, S_ACTOR) * a.cfg.exploration_noise : 0.0;
    xs[D + lane] = y3 * 2.0 + nz;
  }
  __syncthreads();
  const double q = critic_forward(a.critic, NI, xs, h1s, h2s, &qs, lane, ch1, ch2);
  // back through the critic: ∂loss/∂Q = −1/k, δ2, δ1, then ∂loss/∂a[c] = Σ_i W1[i, D + c]·δ1[i], i ascending
  const double dq = -1.0 / (double)k;
  ds[lane] = ch2 > 0.0 ? (double)a.critic[oc.W3 + lane] * dq : 0.0;
  __syncthreads();
  const double t1 = w2t_row(a.critic + oc.W2, ds, lane);
  __syncthreads();
  ds[lane] = ch1 > 0.0 ? t1 : 0.0;
  __syncthreads();
  if (lane < A) {
    double ga = 0.0;
#pragma unroll 8
    for (int i = 0; i < GH; ++i) ga += (double)a.critic[oc.W1 + i + GH * (D + lane)] * ds[i];
    const double d3 = (ga * 2.0) * (1.0 - y3 * y3);                                   // x·2, then tanh_fast' = 1 − y²
    d3s[lane] = d3;
    a.aD3[(size_t)A * b + lane] = d3; a.aY[(size_t)A * b + lane] = y3;
  }
  __syncthreads();
  // actor δ2[j] = (Σ_c W3[c, j]·δ3[c])·(1 − h2[j]²), δ1[i] = (Σ_j W2[j, i]·δ2[j])·(1 − h1[i]²)
  double s2 = 0.0;
  for (int c = 0; c < A; ++c) s2 += (double)a.actor[oa.W3 + c + A * lane] * d3s[c];
  const double d2 = s2 * (1.0 - ah2 * ah2);
  ds[lane] = d2;
  __syncthreads();
  const double d1 = w2t_row(a.actor + oa.W2, ds, lane) * (1.0 - ah1 * ah1);
  const size_t r = (size_t)GH * b + lane;
  a.aH1[r] = ah1; a.aH2[r] = ah2; a.aD1[r] = d1; a.aD2[r] = d2;
  if (lane == 0) a.Qa[b] = q;
}
__global__ void __launch_bounds__(64) ddpg_actor_kernel(DDPGDev a) {
  if (!a.ctl->train_pending) return;
  ddpg_actor_pass(a);
}

// the gradient of actor parameter p from the actor pass's buffers, samples in sample order; HR = head rows (o = net_off(D, HR), aD3 is [k][HR]:
// act_dim for DDPG and TD3, 2·act_dim for SAC), NI = the row length of X
__device__ __forceinline__ double actor_param_grad(const DDPGDev& a, const NetOff& o, int NI, int HR, int k, int p) {
#pragma clang fp contract(off)
  double g = 0.0;
  if (p < o.b1) {
    const int i = p % GH, kk = p / GH;
#pragma unroll 30
    for (int b = 0; b < k; ++b) g += a.aD1[(size_t)GH * b + i] * a.X[(size_t)NI * b + kk];
  } else if (p < o.W2) {
    const int i = p - o.b1;
#pragma unroll 30
    for (int b = 0; b < k; ++b) g += a.aD1[(size_t)GH * b + i];
  } else if (p < o.b2) {
    const int r = p - o.W2, j = r % GH, kk = r / GH;
#pragma unroll 30
    for (int b = 0; b < k; ++b) g += a.aD2[(size_t)GH * b + j] * a.aH1[(size_t)GH * b + kk];
  } else if (p < o.W3) {
    const int j = p - o.b2;
#pragma unroll 30
    for (int b = 0; b < k; ++b) g += a.aD2[(size_t)GH * b + j];
  } else if (p < o.b3) {
    const int r = p - o.W3, c = r % HR, j = r / HR;
#pragma unroll 30
    for (int b = 0; b < k; ++b) g += a.aD3[(size_t)HR * b + c] * a.aH2[(size_t)GH * b + j];
  } else {
    const int c = p - o.b3;
#pragma unroll 30
    for (int b = 0; b < k; ++b) g += a.aD3[(size_t)HR * b + c];
  }
  return g;
}

// E. actor gradient, Adam, polyak for actor parameter p (p >= the actor's size: only p = 0's loss)
__device__ __forceinline__ void ddpg_actor_step_entry(const DDPGDev& a, int p) {
#pragma clang fp contract(off)
  const int k = (int)a.cfg.batch_size, D = a.cfg.obs_dim, A = a.cfg.act_dim, NI = D + A;
  const NetOff o = net_off(D, A);
  if (p == 0) {                                                                        // actor_loss = −mean(Q) (:123)
    double sum = 0.0;
    for (int b = 0; b < k; ++b) sum += a.Qa[b];
    a.ctl->actor_loss = -(sum / (double)k);
  }
  if (p >= o.N) return;
  const double g = actor_param_grad(a, o, NI, A, k, p);
  ddpg_step_entry(g, a.actor, a.actor_t, a.ma, a.va, a.betap + 2 * net_array(o, p), a.cfg.lr, a.cfg.tau, p);
}
__global__ void __launch_bounds__(64) ddpg_actor_step(DDPGDev a) {
  if (!a.ctl->train_pending) return;
  ddpg_actor_step_entry(a, blockIdx.x * 64 + threadIdx.x);
}

// ddpg.jl:79 for step `gstep` on one wave: act[0..A) = rand(act_space) while gstep <= warmup_steps, else actor(obs) with its noise. obs in xs (LDS).
__device__ __forceinline__ void ddpg_select_action(const DDPGDev& a, uint64_t gstep, const double* xs, double* h1s, double* h2s, double* ys, double* act,
                                                   int lane) {
#pragma clang fp contract(off)
  const int D = a.cfg.obs_dim, A = a.cfg.act_dim;
  if ((int64_t)gstep <= a.cfg.warmup_steps) {
    if (lane < A) act[lane] = a.cfg.act_low + (a.cfg.act_high - a.cfg.act_low) * u53(philox_env(a.cfg.seed, (uint32_t)lane, gstep, S_WARMUP));
  } else {
    double h1, h2;
    actor_forward(a.actor, D, A, xs, h1s, h2s, ys, lane, h1, h2);
    if (lane < A) act[lane] = ys[lane] * 2.0 + ddpg_normal(a.cfg.seed, (uint32_t)lane, gstep, S_BEHAVE) * a.cfg.exploration_noise;
  }
  __syncthreads();
}

// ddpg_select_action as the `select` of ddpg_collect / ddpg_act: DDPG's and TD3's behaviour policy
__device__ __forceinline__ auto ddpg_selector(const DDPGDev& a) {
  return [&a](uint64_t gstep, const double* xs, double* h1s, double* h2s, double* ys, double* act, int lane) {
    ddpg_select_action(a, gstep, xs, h1s, h2s, ys, act, lane);
  };
}

// one thread: counts the update, writes its loss record when the step is a multiple of log_frequency (ddpg.jl:131-133) and clears train_pending;
// → the index of the record it wrote, −1 if none
__device__ __forceinline__ int ddpg_log_update(const DDPGDev& a, DDPGCtl& c) {
  int rec = -1;
  c.n_updates += 1;
  if (c.global_step % a.cfg.log_frequency == 0) {
    if (c.n_losses < DDPG_MAX_LOSSES) {
      rec = c.n_losses;
      a.losses[rec].global_step = c.global_step; a.losses[rec].actor_loss = c.actor_loss; a.losses[rec].critic_loss = c.critic_loss;
    }
    c.n_losses += 1;
  }
  c.train_pending = 0;
  return rec;
}
// closes the update the launches before this one ran: the only writer of the β powers, n_updates, the loss records and train_pending
__device__ __forceinline__ void ddpg_finish_update(const DDPGDev& a, DDPGCtl& c, int lane) {
  if (lane < 12) betap_advance(a.betap, lane, a.betap[2 * lane], a.betap[2 * lane + 1]);
  if (lane == 0) ddpg_log_update(a, c);
}

// F. close the pending update, then ddpg.jl:77-105 on the Pendulum until an update is due, the budget or total_timesteps is used up
template <class Finish, class Select>
__device__ __forceinline__ void ddpg_collect(const DDPGDev& a, Finish finish, Select select) {
#pragma clang fp contract(off)
  __shared__ DDPGCtl c;
  __shared__ double xs[DDPG_MAX_IN], h1s[GH], h2s[GH], ys[DDPG_MAX_ACT], act[DDPG_MAX_ACT];
  __shared__ int go;
  const int lane = threadIdx.x;
  if (lane == 0) c = *a.ctl;
  __syncthreads();
  if (c.train_pending) finish(c, lane);
  __syncthreads();
  while (a.cfg.env_kind == CRL_DDPG_ENV_PENDULUM) {
    if (lane == 0) {
      go = (!c.train_pending && c.taken < c.budget && c.global_step < a.cfg.total_timesteps) ? 1 : 0;
      if (go) {
        c.global_step += 1; c.taken += 1;                                              // ddpg.jl:76
        xs[0] = pend_cos(c.env[0]); xs[1] = pend_sin(c.env[0]); xs[2] = c.env[1];      // :77 obs = state(env)
      }
    }
    __syncthreads();
    if (!go) break;
    const uint64_t gstep = (uint64_t)c.global_step;
    select(gstep, xs, h1s, h2s, ys, act, lane);                                        // :79
    if (lane == 0) {
      double rew;
      const bool done = pendulum_step64(c.env, c.env_t, act[0], a.cfg.max_steps, rew); // :80
      const size_t p = (size_t)c.ptr;                                                  // :83-90 Buffer.add!, the action unclipped
      for (int i = 0; i < 3; ++i) a.rb_state[3 * p + i] = xs[i];
      a.rb_action[p] = act[0]; a.rb_reward[p] = rew; a.rb_terminal[p] = done ? 1 : 0;
      a.rb_next[3 * p + 0] = pend_cos(c.env[0]); a.rb_next[3 * p + 1] = pend_sin(c.env[0]); a.rb_next[3 * p + 2] = c.env[1];
      c.ptr = c.ptr + 1 >= a.cfg.buffer_size ? 0 : c.ptr + 1;
      c.size = c.size + 1 > a.cfg.buffer_size ? a.cfg.buffer_size : c.size + 1;
      c.episode_return += rew; c.episode_length += 1;                                  // :93-94
      if (done) {                                                                      // :95-101
        if (c.n_eps < DDPG_MAX_EPS) {
          a.eps[c.n_eps].episode_return = c.episode_return; a.eps[c.n_eps].episode_length = c.episode_length; a.eps[c.n_eps].global_step = c.global_step;
        }
        c.n_eps += 1;
        c.episode_length = 0; c.episode_return = 0.0;
        pendulum_reset64(c.env, a.cfg.seed, gstep, S_RESET); c.env_t = 0;
      }
      c.train_pending = (c.global_step > a.cfg.min_buff_size && c.global_step > a.cfg.warmup_steps) ? 1 : 0;   // :105
    }
    __syncthreads();
  }
  if (lane == 0) *a.ctl = c;
}
__global__ void __launch_bounds__(64) ddpg_collect_kernel(DDPGDev a) {
  ddpg_collect(a, [&a](DDPGCtl& c, int lane) { ddpg_finish_update(a, c, lane); }, ddpg_selector(a));
}

// ------------------------------------------------------------------------------------------------------
// TD3 (the crl_td3_* block of include/cleanrl_hip.h) on the DDPG handle: the same six launches, the same ring, draw, env loop and act / observe
// kernels. A TD3 handle's critic, critic_t, mc and vc hold [2][nc] floats (critic 1 first, so every DDPG kernel that reads a.critic reads critic 1),
// its cH1 / cH2 / cD1 / cD2 hold [2][k][64], dz / sq [2][k], betap [18][2]: the actor's six arrays, critic 1's, critic 2's. X is stored once.
//   A  ddpg_sample_kernel  unchanged
//   B' td3_critic_kernel   one block per sample, two waves, wave w = critic w: target actor + smoothing noise (both waves, each into its own LDS),
//                          target critic w, min of the two through LDS, then forward and backward of online critic w on the shared TD target
//   C' td3_critic_step     one thread per parameter of the 2·nc: gradient in sample order, Adam; no polyak
//   D' td3_actor_kernel    ddpg_actor_pass (critic 1, no noise: noise_in_update is 0 on a TD3 handle) when the actor is due
//   E' td3_actor_step      when the actor is due: ddpg_actor_step_entry (gradient, Adam, polyak) in the first blocks, polyak of both critics in the rest
//   F' td3_collect_kernel  ddpg_collect with TD3's close: 18 β-power pairs, the actor's six only when it stepped
// "The actor is due" is global_step % policy_delay == 0: global_step is the control block's and no kernel of A–E' writes it, so every block of a
// cycle takes the same decision (it is the flag a cycle would otherwise carry next to train_pending, derived instead of stored).
// ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool td3_actor_due(const DDPGCtl* c, const crl_td3_options& o) { return c->global_step % (int64_t)o.policy_delay == 0; }

// forward and backward of online critic w (wave w of a two-wave block) on the shared TD target, for sample b = ring slot s: what the critic pass of
// a twin-critic update (TD3, SAC) does once td is known. Both waves take every barrier alike; each wave's x / h1s / h2s / qs / d2s are its own.
__device__ __forceinline__ void twin_critic_pass(const DDPGDev& a, const float* __restrict__ critic, double td, double* x, double* h1s, double* h2s,
                                                 double* qs, double* d2s, int lane, int w, int b, size_t s) {
#pragma clang fp contract(off)
  const int D = a.cfg.obs_dim, A = a.cfg.act_dim, NI = D + A, k = (int)a.cfg.batch_size;
  const NetOff o = net_off(NI, 1);
  double h1, h2;
  for (int i = lane; i < NI; i += GH) {
    const double v = i < D ? a.rb_state[D * s + i] : a.rb_action[A * s + (i - D)];
    x[i] = v;
    if (w == 0) a.X[(size_t)NI * b + i] = v;
  }
  __syncthreads();
  const double q = critic_forward(critic, NI, x, h1s, h2s, qs, lane, h1, h2);
  const double diff = td - q;
  const double dq = -2.0 * diff / (double)k;
  const double d2 = h2 > 0.0 ? (double)critic[o.W3 + lane] * dq : 0.0;
  d2s[lane] = d2;
  __syncthreads();
  const double t1 = w2t_row(critic + o.W2, d2s, lane);
  const double d1 = h1 > 0.0 ? t1 : 0.0;
  const size_t r = (size_t)GH * ((size_t)w * k + b) + lane;
  a.cH1[r] = h1; a.cH2[r] = h2; a.cD1[r] = d1; a.cD2[r] = d2;
  if (lane == 0) { a.sq[(size_t)w * k + b] = diff * diff; a.dz[(size_t)w * k + b] = dq; }
}

// B'. Every barrier below is reached by both waves: the one exit is the block-uniform one at the top, and both waves take every call alike.
__global__ void __launch_bounds__(128) td3_critic_kernel(DDPGDev a, crl_td3_options opt) {
#pragma clang fp contract(off)
  if (!a.ctl->train_pending) return;
  __shared__ double xs[2][DDPG_MAX_IN], h1s[2][GH], h2s[2][GH], ys[2][DDPG_MAX_ACT], qs[2], d2s[2][GH];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, b = blockIdx.x, D = a.cfg.obs_dim, A = a.cfg.act_dim, NI = D + A;
  const uint64_t gstep = (uint64_t)a.ctl->global_step;
  const size_t s = (size_t)a.idx[b];
  const NetOff o = net_off(NI, 1);
  const float* const critic = a.critic + (size_t)w * o.N;
  const float* const critic_t = a.critic_t + (size_t)w * o.N;
  double h1, h2;
  for (int i = lane; i < D; i += GH) xs[w][i] = a.rb_next[D * s + i];
  __syncthreads();
  actor_forward(a.actor_t, D, A, xs[w], h1s[w], h2s[w], ys[w], lane, h1, h2);
  if (lane < A) {
    // target policy smoothing: a per-SAMPLE draw, component word 16·b + c
    const double z = ddpg_normal(a.cfg.seed, (uint32_t)(16 * b + lane), gstep, S_SMOOTH);
    const double nz0 = opt.policy_noise * z;
    const double nz = nz0 < -opt.noise_clip ? -opt.noise_clip : (nz0 > opt.noise_clip ? opt.noise_clip : nz0);
    const double a0 = ys[w][lane] * 2.0 + nz;
    xs[w][D + lane] = a0 < a.cfg.act_low ? a.cfg.act_low : (a0 > a.cfg.act_high ? a.cfg.act_high : a0);
  }
  __syncthreads();
  critic_forward(critic_t, NI, xs[w], h1s[w], h2s[w], &qs[w], lane, h1, h2);       // its last barrier publishes both qs
  const double q1 = qs[0], q2 = qs[1];
  const double next_q = q2 < q1 ? q2 : q1;
  const double td = a.rb_reward[s] + a.cfg.gamma * next_q * (1.0 - (double)a.rb_terminal[s]);
  __syncthreads();
  twin_critic_pass(a, critic, td, xs[w], h1s[w], h2s[w], &qs[w], d2s[w], lane, w, b, s);
}

// C'. thread p: parameter p % nc of critic p / nc. critic_loss = loss_1 + loss_2
__global__ void __launch_bounds__(64) td3_critic_step(DDPGDev a) {
#pragma clang fp contract(off)
  if (!a.ctl->train_pending) return;
  const int k = (int)a.cfg.batch_size, NI = a.cfg.obs_dim + a.cfg.act_dim, t = blockIdx.x * 64 + threadIdx.x;
  const NetOff o = net_off(NI, 1);
  if (t == 0) {
    double l1 = 0.0, l2 = 0.0;
    for (int b = 0; b < k; ++b) l1 += a.sq[b];
    for (int b = 0; b < k; ++b) l2 += a.sq[(size_t)k + b];
    a.ctl->critic_loss = l1 / (double)k + l2 / (double)k;
  }
  if (t >= 2 * o.N) return;
  const int w = t / o.N, p = t - w * o.N;
  const double g = critic_param_grad(a, o, NI, k, p, (size_t)w * k * GH, (size_t)w * k);
  const double* bp = a.betap + 2 * (6 + 6 * w + net_array(o, p));
  float mi, vi, wi;
  adam_entry((double)(float)g, a.mc[t], a.vc[t], a.critic[t], bp[0], bp[1], a.cfg.lr, /*clip=*/false, 1.0, mi, vi, wi);
  a.mc[t] = mi; a.vc[t] = vi; a.critic[t] = wi;
}

// D'.
__global__ void __launch_bounds__(64) td3_actor_kernel(DDPGDev a, crl_td3_options opt) {
  if (!a.ctl->train_pending || !td3_actor_due(a.ctl, opt)) return;
  ddpg_actor_pass(a);
}

// E'. blocks 0..actor_blocks−1: the actor; the blocks after them: polyak_update! of the 2·nc critic elements (the critics stepped in C')
__global__ void __launch_bounds__(64) td3_actor_step(DDPGDev a, crl_td3_options opt, int actor_blocks, int nc2) {
#pragma clang fp contract(off)
  if (!a.ctl->train_pending || !td3_actor_due(a.ctl, opt)) return;
  if ((int)blockIdx.x < actor_blocks) { ddpg_actor_step_entry(a, blockIdx.x * 64 + threadIdx.x); return; }
  const int t = ((int)blockIdx.x - actor_blocks) * 64 + threadIdx.x;
  if (t < nc2) a.critic_t[t] = (float)(a.cfg.tau * (double)a.critic[t] + (1.0 - a.cfg.tau) * (double)a.critic_t[t]);
}

// closes a TD3 update: critic β powers always, the actor's only when it stepped; the rest is ddpg_finish_update's
__device__ __forceinline__ void td3_finish_update(const DDPGDev& a, const crl_td3_options& opt, DDPGCtl& c, int lane) {
  const bool due = td3_actor_due(&c, opt);
  if (lane < 18 && (lane >= 6 || due)) betap_advance(a.betap, lane, a.betap[2 * lane], a.betap[2 * lane + 1]);
  if (lane == 0) ddpg_log_update(a, c);
}
// F'.
__global__ void __launch_bounds__(64) td3_collect_kernel(DDPGDev a, crl_td3_options opt) {
  ddpg_collect(a, [&a, &opt](DDPGCtl& c, int lane) { td3_finish_update(a, opt, c, lane); }, ddpg_selector(a));
}

// host-driven env: the action of step global_step + 1 for the staged observation (advances nothing)
template <class Select>
__device__ __forceinline__ void ddpg_act(const DDPGDev& a, Select select) {
  __shared__ double xs[DDPG_MAX_IN], h1s[GH], h2s[GH], ys[DDPG_MAX_ACT], act[DDPG_MAX_ACT];
  const int lane = threadIdx.x, D = a.cfg.obs_dim, A = a.cfg.act_dim;
  for (int i = lane; i < D; i += GH) xs[i] = a.stage[i];
  __syncthreads();
  select((uint64_t)(a.ctl->global_step + 1), xs, h1s, h2s, ys, act, lane);
  if (lane < A) a.stage[2 * D + A + 2 + lane] = act[lane];
}
__global__ void __launch_bounds__(64) ddpg_act_kernel(DDPGDev a) { ddpg_act(a, ddpg_selector(a)); }
// host-driven env: global_step += 1, Buffer.add! of the staged transition (ddpg.jl:76,83-90), is an update due (:105)
__global__ void __launch_bounds__(64) ddpg_add_kernel(DDPGDev a) {
  __shared__ int64_t ptr;
  const int lane = threadIdx.x, D = a.cfg.obs_dim, A = a.cfg.act_dim;
  if (lane == 0) ptr = a.ctl->ptr;
  __syncthreads();
  const size_t p = (size_t)ptr;
  const double* s = a.stage;
  for (int i = lane; i < D; i += GH) { a.rb_state[D * p + i] = s[i]; a.rb_next[D * p + i] = s[D + A + 1 + i]; }
  if (lane < A) a.rb_action[A * p + lane] = s[D + lane];
  if (lane == 0) {
    DDPGCtl* c = a.ctl;
    a.rb_reward[p] = s[D + A]; a.rb_terminal[p] = s[2 * D + A + 1] != 0.0 ? 1 : 0;
    c->global_step += 1;
    c->ptr = ptr + 1 >= a.cfg.buffer_size ? 0 : ptr + 1;
    c->size = c->size + 1 > a.cfg.buffer_size ? a.cfg.buffer_size : c->size + 1;
    c->train_pending = (c->global_step > a.cfg.min_buff_size && c->global_step > a.cfg.warmup_steps) ? 1 : 0;
  }
}

__global__ void ddpg_init_kernel(DDPGDev a) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  DDPGCtl c;
  memset(&c, 0, sizeof(c));
  if (a.cfg.env_kind == CRL_DDPG_ENV_PENDULUM) pendulum_reset64(c.env, a.cfg.seed, 0, S_RESET0);   // ddpg.jl:74 reset!(env)
  *a.ctl = c;
}

// the noise-free 2·tanh_fast(·) of actor(obs) / get_q(critic, obs, act) on caller-supplied inputs, one wave per column
__global__ void __launch_bounds__(64) ddpg_actor_eval_kernel(DDPGDev a, const double* __restrict__ obs, int n, double* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ double xs[DDPG_MAX_IN], h1s[GH], h2s[GH], ys[DDPG_MAX_ACT];
  const int lane = threadIdx.x, b = blockIdx.x, D = a.cfg.obs_dim, A = a.cfg.act_dim;
  if (b >= n) return;
  for (int i = lane; i < D; i += GH) xs[i] = obs[(size_t)D * b + i];
  __syncthreads();
  double h1, h2;
  actor_forward(a.actor, D, A, xs, h1s, h2s, ys, lane, h1, h2);
  if (lane < A) out[(size_t)A * b + lane] = ys[lane] * 2.0;
}
__global__ void __launch_bounds__(64) ddpg_q_eval_kernel(DDPGDev a, const double* __restrict__ obs, const double* __restrict__ act, int n,
                                                         double* __restrict__ out) {
  __shared__ double xs[DDPG_MAX_IN], h1s[GH], h2s[GH], qs;
  const int lane = threadIdx.x, b = blockIdx.x, D = a.cfg.obs_dim, A = a.cfg.act_dim;
  if (b >= n) return;
  for (int i = lane; i < D + A; i += GH) xs[i] = i < D ? obs[(size_t)D * b + i] : act[(size_t)A * b + (i - D)];
  __syncthreads();
  double h1, h2;
  const double q = critic_forward(a.critic, D + A, xs, h1s, h2s, &qs, lane, h1, h2);
  if (lane == 0) out[b] = q;
}

}  // namespace crl

#include "sac.hpp"   // SAC on this handle: its kernels, built from the pieces above

namespace crl {

// ------------------------------------------------------------------------------------------------------
// crl_ddpg_evaluate: the frozen actor on n private Pendulums, `episodes` episodes each, in ONE launch. One wave owns one env from its first reset to
// its last step, lane = hidden unit, EVAL_WAVES envs per block. The actor stays on the chip for the whole launch: the lane's rows of W1 and W2 and
// its two biases are registers, W3 / b3 (which every lane reads in input order) are staged once per block into LDS, so the step loop reads no global
// memory. Env state, sums and the action are computed by every lane alike (wave-uniform: no broadcast). The arithmetic is dense_row's and head_row's
// — products in input order, bias last, contraction off —, so an action has the bits crl_ddpg_actor gives for the same observation; the critic runs
// once per episode through critic_forward itself. After the staging barrier a wave never meets a block barrier again (a wave past n leaves there):
// layers are separated by wave_lds_fence on wave-private h1s / h2s. Pendulum handles only (obs 3, act 1 — crl_ddpg_create pins that shape).
// head_rows = 1: DDPG's and TD3's actor, action 2·tanh_fast(head). head_rows = 2: SAC's, whose head row 0 is μ: action scale·tanh_fast(μ) + bias, what
// sac_actor_eval_kernel gives.
// ------------------------------------------------------------------------------------------------------
#ifndef CRL_EVAL_WAVES
#define CRL_EVAL_WAVES 4      // envs per block; experiment builds (csrc/Makefile, EXTRA=-DCRL_EVAL_WAVES=n) measured 1, 2, 4, 8: DESIGN.md §3e
#endif
constexpr int EVAL_WAVES = CRL_EVAL_WAVES, PEND_OBS = 3;
struct DDPGEvalArgs {
  int32_t n, episodes, trace_steps, head_rows; uint64_t seed;
  double *ret, *disc_ret, *q0, *trace;      // [episodes][n] each, [trace_steps][n]
};
__global__ void __launch_bounds__(64 * EVAL_WAVES) ddpg_eval_kernel(DDPGDev a, DDPGEvalArgs ev) {
#pragma clang fp contract(off)
  __shared__ float w3s[GH], b3s;
  __shared__ double xs[EVAL_WAVES][PEND_OBS + 1], h1s[EVAL_WAVES][GH], h2s[EVAL_WAVES][GH], qs[EVAL_WAVES];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, env = blockIdx.x * EVAL_WAVES + w, max_steps = a.cfg.max_steps;
  const int HR = ev.head_rows;
  const NetOff o = net_off(PEND_OBS, HR);
  if (threadIdx.x < GH) w3s[threadIdx.x] = a.actor[o.W3 + HR * threadIdx.x];
  if (threadIdx.x == 0) b3s = a.actor[o.b3];
  __syncthreads();
  if (env >= ev.n) return;
  float w1[PEND_OBS], w2[GH];
#pragma unroll
  for (int k = 0; k < PEND_OBS; ++k) w1[k] = a.actor[o.W1 + lane + GH * k];
#pragma unroll
  for (int k = 0; k < GH; ++k) w2[k] = a.actor[o.W2 + lane + GH * k];
  const double b1 = (double)a.actor[o.b1 + lane], b2 = (double)a.actor[o.b2 + lane], gamma = a.cfg.gamma;
  double* const h1w = h1s[w];
  double* const h2w = h2s[w];
  for (int j = 0; j < ev.episodes; ++j) {
    double s[2], ret = 0.0, disc_ret = 0.0, disc = 1.0;
    int t = 0;
    pendulum_reset64(s, ev.seed, (uint64_t)j * (uint64_t)ev.n + (uint64_t)env, S_EVAL);
    for (int step = 0; step < max_steps; ++step) {
      const double x[PEND_OBS] = {pend_cos(s[0]), pend_sin(s[0]), s[1]};
      double acc = 0.0;
#pragma unroll
      for (int k = 0; k < PEND_OBS; ++k) acc += (double)w1[k] * x[k];
      acc += b1;
      h1w[lane] = tanh_fast64(acc);
      wave_lds_fence();
      acc = 0.0;
#pragma unroll
      for (int k = 0; k < GH; ++k) acc += (double)w2[k] * h1w[k];
      acc += b2;
      h2w[lane] = tanh_fast64(acc);
      wave_lds_fence();
      acc = 0.0;
#pragma unroll 8
      for (int k = 0; k < GH; ++k) acc += (double)w3s[k] * h2w[k];
      const double y = tanh_fast64(acc + (double)b3s);
      const double act = HR == 2 ? sac_scale(a.cfg) * y + sac_bias(a.cfg) : y * 2.0;
      if (step == 0) {                                                                 // Q(s0, μ(s0)): what crl_ddpg_q_values gives for (x, act)
        if (lane == 0) { xs[w][0] = x[0]; xs[w][1] = x[1]; xs[w][2] = x[2]; xs[w][3] = act; }
        wave_lds_fence();
        double c1, c2;
        const double q = critic_forward<false>(a.critic, PEND_OBS + 1, xs[w], h1w, h2w, &qs[w], lane, c1, c2);
        if (lane == 0) ev.q0[(size_t)j * ev.n + env] = q;
      }
      const int64_t row = (int64_t)j * max_steps + step;
      if (lane == 0 && row < ev.trace_steps) ev.trace[(size_t)row * ev.n + env] = act;
      double rew;
      const bool done = pendulum_step64(s, t, act, max_steps, rew);
      ret += rew;
      disc_ret += disc * rew;
      disc = disc * gamma;
      if (done) break;
    }
    if (lane == 0) { ev.ret[(size_t)j * ev.n + env] = ret; ev.disc_ret[(size_t)j * ev.n + env] = disc_ret; }
  }
}

}  // namespace crl

struct crl_ddpg {
  crl_ddpg_config cfg;
  int device = 0;
  bool params_set = false;       // ddpg.jl:52 has happened (a fresh handle holds zeros)
  int64_t host_step = 0;         // global_step as of the last call (the schedule of ddpg.jl:105 is deterministic)
  int na = 0, nc = 0;
  bool td3 = false;              // created by crl_td3_create: two critics ([2][nc] in d.critic / critic_t / mc / vc), the TD3 cycle
  crl_td3_options topt{};
  bool sac = false;              // created by crl_sac_create: critics as a TD3 handle's, an actor with a head of 2·act_dim rows, the SAC cycle
  crl::SACDev sd{};
  std::vector<crl_sac_alpha_record> arecs;   // the alpha records of the loss records the last crl_ddpg_run / crl_ddpg_read_losses returned
  hipStream_t stream = nullptr;
  crl::DDPGDev d;
  double* pinned = nullptr;      // external env: the staging slot's host side
  void* scratch = nullptr; size_t scratch_bytes = 0;   // crl_ddpg_actor / crl_ddpg_q_values
};

using namespace crl;

#define DDPG_GUARD(h)                                          \
  if (!(h)) { set_error("null crl_ddpg handle"); return 1; }   \
  CRL_HIP_CHECK(hipSetDevice((h)->device));

template <typename T>
static int galloc(T** p, size_t n) {
  CRL_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(p), n * sizeof(T)));
  CRL_HIP_CHECK(hipMemset(*p, 0, n * sizeof(T)));
  return 0;
}

// one cycle: launches A–E, then the collect launch F (which closes the update and, on a Pendulum handle, steps the env)
static void enqueue_cycle(const crl_ddpg* h) {
  hipStream_t st = h->stream;
  const DDPGDev& d = h->d;
  const int k = (int)h->cfg.batch_size, na = h->na, nc = h->nc;
  hipLaunchKernelGGL(ddpg_sample_kernel, dim3(1), dim3(1024), 0, st, d);
  if (h->sac) {
    const int ab = (na + 63) / 64;
    hipLaunchKernelGGL(sac_critic_kernel, dim3(k), dim3(128), 0, st, d, h->sd);
    hipLaunchKernelGGL(td3_critic_step, dim3((2 * nc + 63) / 64), dim3(64), 0, st, d);
    hipLaunchKernelGGL(sac_actor_kernel, dim3(k), dim3(128), 0, st, d, h->sd);
    hipLaunchKernelGGL(sac_actor_step, dim3(ab + (2 * nc + 63) / 64), dim3(64), 0, st, d, h->sd, ab, 2 * nc);
    hipLaunchKernelGGL(sac_collect_kernel, dim3(1), dim3(64), 0, st, d, h->sd);
    return;
  }
  if (h->td3) {
    const int ab = (na + 63) / 64;
    hipLaunchKernelGGL(td3_critic_kernel, dim3(k), dim3(128), 0, st, d, h->topt);
    hipLaunchKernelGGL(td3_critic_step, dim3((2 * nc + 63) / 64), dim3(64), 0, st, d);
    hipLaunchKernelGGL(td3_actor_kernel, dim3(k), dim3(64), 0, st, d, h->topt);
    hipLaunchKernelGGL(td3_actor_step, dim3(ab + (2 * nc + 63) / 64), dim3(64), 0, st, d, h->topt, ab, 2 * nc);
    hipLaunchKernelGGL(td3_collect_kernel, dim3(1), dim3(64), 0, st, d, h->topt);
    return;
  }
  hipLaunchKernelGGL(ddpg_critic_kernel, dim3(k), dim3(64), 0, st, d);
  hipLaunchKernelGGL(ddpg_critic_step, dim3((nc + 63) / 64), dim3(64), 0, st, d);
  hipLaunchKernelGGL(ddpg_actor_kernel, dim3(k), dim3(64), 0, st, d);
  hipLaunchKernelGGL(ddpg_actor_step, dim3((na + 63) / 64), dim3(64), 0, st, d);
  hipLaunchKernelGGL(ddpg_collect_kernel, dim3(1), dim3(64), 0, st, d);
}

static int ddpg_scratch(crl_ddpg* h, size_t need) {
  if (h->scratch_bytes >= need) return 0;
  if (h->scratch) CRL_HIP_CHECK(hipFree(h->scratch));
  h->scratch = nullptr; h->scratch_bytes = 0;
  CRL_HIP_CHECK(hipMalloc(&h->scratch, need));
  h->scratch_bytes = need;
  return 0;
}

extern "C" {

int32_t crl_ddpg_param_count(int32_t obs_dim, int32_t act_dim, int64_t* actor_n, int64_t* critic_n) {
  if (obs_dim < 1 || obs_dim > DDPG_MAX_OBS) { set_error("crl_ddpg_param_count: obs_dim must be in 1..64"); return 1; }
  if (act_dim < 1 || act_dim > DDPG_MAX_ACT) { set_error("crl_ddpg_param_count: act_dim must be in 1..16"); return 1; }
  if (actor_n) *actor_n = net_off(obs_dim, act_dim).N;
  if (critic_n) *critic_n = net_off(obs_dim + act_dim, 1).N;
  return 0;
}

}  // extern "C"

// crl_ddpg_create (topt = sopt = nullptr), crl_td3_create and crl_sac_create: a TD3 or SAC handle holds two critics and two critic passes' buffers
// where a DDPG handle holds one; a SAC handle's actor has a head of 2·act_dim rows, and it owns log_alpha, its β-power pair and the alpha records
static int32_t ddpg_create(const crl_ddpg_config* cfg, const crl_td3_options* topt, const crl_sac_options* sopt, int32_t device, crl_ddpg** out) {
  if (cfg->obs_dim < 1 || cfg->obs_dim > DDPG_MAX_OBS) { set_error("crl_ddpg_create: obs_dim must be in 1..64"); return 1; }
  if (cfg->act_dim < 1 || cfg->act_dim > DDPG_MAX_ACT) { set_error("crl_ddpg_create: act_dim must be in 1..16"); return 1; }
  if (cfg->env_kind != CRL_DDPG_ENV_PENDULUM && cfg->env_kind != CRL_DDPG_ENV_EXTERNAL) { set_error("crl_ddpg_create: env_kind must be CRL_DDPG_ENV_PENDULUM or CRL_DDPG_ENV_EXTERNAL"); return 1; }
  if (cfg->env_kind == CRL_DDPG_ENV_PENDULUM && (cfg->obs_dim != 3 || cfg->act_dim != 1)) { set_error("crl_ddpg_create: the Pendulum needs obs_dim = 3 and act_dim = 1"); return 1; }
  if (cfg->batch_size < 1 || cfg->batch_size > DDPG_MAX_BATCH) { set_error("crl_ddpg_create: batch_size must be in 1..1024"); return 1; }
  if (cfg->buffer_size < cfg->batch_size || cfg->buffer_size > DDPG_MAX_CAP) { set_error("crl_ddpg_create: buffer_size must be in batch_size..131072"); return 1; }
  if (cfg->min_buff_size < 0 || cfg->warmup_steps < 0 ||
      (cfg->min_buff_size > cfg->warmup_steps ? cfg->min_buff_size : cfg->warmup_steps) + 1 < cfg->batch_size) {
    set_error("crl_ddpg_create: max(min_buff_size, warmup_steps) + 1 must be >= batch_size (Buffer.sample asserts n <= rb.size, replay_buffer.jl:41)"); return 1;
  }
  if (!(cfg->act_low < cfg->act_high)) { set_error("crl_ddpg_create: act_low must be < act_high"); return 1; }
  if (!(cfg->tau > 0.0 && cfg->tau <= 1.0)) { set_error("crl_ddpg_create: tau must be in (0, 1]"); return 1; }
  if (cfg->log_frequency < 1) { set_error("crl_ddpg_create: log_frequency must be >= 1"); return 1; }
  if (cfg->max_steps < 1) { set_error("crl_ddpg_create: max_steps must be >= 1"); return 1; }
  if (cfg->total_timesteps < 0) { set_error("crl_ddpg_create: total_timesteps must be >= 0"); return 1; }
  int ndev = 0;
  CRL_HIP_CHECK(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) { set_error("crl_ddpg_create: no such HIP device (no GPU → no CPU fallback)"); return 1; }
  CRL_HIP_CHECK(hipSetDevice(device));
  crl_ddpg* h = new (std::nothrow) crl_ddpg();
  if (!h) { set_error("out of host memory"); return 1; }
  h->cfg = *cfg; h->device = device;
  if (topt) { h->td3 = true; h->topt = *topt; }
  if (sopt) { h->sac = true; h->sd.opt = *sopt; }
  const size_t Q = topt || sopt ? 2 : 1;   // critics
  memset(&h->d, 0, sizeof(h->d));
  h->d.cfg = *cfg;
  hipError_t se = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
  if (se != hipSuccess) { set_error(std::string("hipStreamCreate: ") + hipGetErrorString(se)); delete h; return 1; }
  const size_t cap = (size_t)cfg->buffer_size, k = (size_t)cfg->batch_size, D = (size_t)cfg->obs_dim, A = (size_t)cfg->act_dim;
  const size_t HR = sopt ? 2 * A : A;   // head rows of the actor
  h->na = net_off((int)D, (int)HR).N; h->nc = net_off((int)(D + A), 1).N;
  const size_t na = (size_t)h->na, nc = (size_t)h->nc;
  DDPGDev& d = h->d;
  int rc = 0;
  rc |= galloc(&d.actor, na); rc |= galloc(&d.ma, na); rc |= galloc(&d.va, na);
  rc |= galloc(&d.critic, Q * nc); rc |= galloc(&d.critic_t, Q * nc); rc |= galloc(&d.mc, Q * nc); rc |= galloc(&d.vc, Q * nc);
  rc |= galloc(&d.betap, 12 * (Q + 1) + (sopt ? 2 : 0)); rc |= galloc(&d.ctl, 1); rc |= galloc(&d.eps, DDPG_MAX_EPS); rc |= galloc(&d.losses, DDPG_MAX_LOSSES);
  rc |= galloc(&d.rb_state, cap * D); rc |= galloc(&d.rb_next, cap * D); rc |= galloc(&d.rb_action, cap * A); rc |= galloc(&d.rb_reward, cap);
  rc |= galloc(&d.rb_terminal, cap); rc |= galloc(&d.idx, k);
  rc |= galloc(&d.X, k * (D + A)); rc |= galloc(&d.cH1, Q * k * GH); rc |= galloc(&d.cH2, Q * k * GH);
  rc |= galloc(&d.cD1, Q * k * GH); rc |= galloc(&d.cD2, Q * k * GH); rc |= galloc(&d.dz, Q * k); rc |= galloc(&d.sq, Q * k);
  rc |= galloc(&d.aH1, k * GH); rc |= galloc(&d.aH2, k * GH); rc |= galloc(&d.aD1, k * GH); rc |= galloc(&d.aD2, k * GH);
  rc |= galloc(&d.aD3, k * HR); rc |= galloc(&d.Qa, k);
  if (!sopt) { rc |= galloc(&d.actor_t, na); rc |= galloc(&d.aY, k * A); }   // SAC has no target actor and keeps no tanh outputs: both stay null
  if (sopt) {
    rc |= galloc(&h->sd.log_alpha, 3); rc |= galloc(&h->sd.lp, k); rc |= galloc(&h->sd.sctl, 1); rc |= galloc(&h->sd.arecs, DDPG_MAX_LOSSES);
  }
  rc |= galloc(&d.stage, 2 * D + 2 * A + 2);
  if (!rc && hipHostMalloc(reinterpret_cast<void**>(&h->pinned), (2 * D + 2 * A + 2) * sizeof(double), hipHostMallocDefault) != hipSuccess) {
    set_error("crl_ddpg_create: hipHostMalloc failed"); h->pinned = nullptr; rc = 1;
  }
  if (rc) { crl_ddpg_destroy(h); return 1; }
  double bp[38];
  for (int i = 0; i < 19; ++i) { bp[2 * i] = ADAM_B1; bp[2 * i + 1] = ADAM_B2; }
  CRL_HIP_CHECK(hipMemcpy(d.betap, bp, (12 * (Q + 1) + (sopt ? 2 : 0)) * sizeof(double), hipMemcpyHostToDevice));
  if (sopt) {
    const float la = (float)std::log(sopt->alpha);
    const SACCtl sc{sopt->alpha, 0.0, 0.0};
    CRL_HIP_CHECK(hipMemcpy(h->sd.log_alpha, &la, sizeof(la), hipMemcpyHostToDevice));
    CRL_HIP_CHECK(hipMemcpy(h->sd.sctl, &sc, sizeof(sc), hipMemcpyHostToDevice));
  }
  hipLaunchKernelGGL(ddpg_init_kernel, dim3(1), dim3(1), 0, h->stream, d);
  CRL_HIP_CHECK(hipStreamSynchronize(h->stream));
  *out = h;
  return 0;
}

// the three kinds of handle: 0 DDPG, 1 TD3, 2 SAC
static const char* const KIND[3] = {"ddpg", "td3", "sac"};
static int kind_of(const crl_ddpg* h) { return h->sac ? 2 : h->td3 ? 1 : 0; }
static const char NO_TWIN[] = "";
// the DDPG parameter calls know one critic, the crl_td3_* ones two, the crl_sac_* ones two and another actor: each refuses the other kinds of handle
// and names its twin: the call of the same name for the handle's kind, or `twin` where that call has another name (NO_TWIN: a call only SAC has).
// fn = "crl_<kind>_<call>"; want: the kind the call is for
static bool wrong_kind(const crl_ddpg* h, int want, const char* fn, const char* twin = nullptr) {
  static const char* const names[3] = {"DDPG", "TD3", "SAC"};
  const int is = kind_of(h);
  if (is == want) return false;
  const std::string call = std::string(fn).substr(4 + strlen(KIND[want]));           // "_<call>"
  const std::string what = std::string(fn) + ": this is a " + names[is] + " handle (crl_" + KIND[is] + "_create) — ";
  if (twin == NO_TWIN) set_error(what + "only a " + names[want] + " handle (crl_" + KIND[want] + "_create) has this call");
  else set_error(what + "use " + (twin ? std::string(twin) : std::string("crl_") + KIND[is] + call));
  return true;
}
// the calls every kind of handle takes refuse one whose parameters were never written, and name the parameter calls of the handle's own kind
static bool params_unset(const crl_ddpg* h, const char* fn, const char* more = "") {
  if (h->params_set) return false;
  const std::string k = std::string("crl_") + KIND[kind_of(h)];
  set_error(std::string(fn) + ": parameters not set — " + k + "_write_params or " + k + "_init_params first (ddpg.jl:52" + more + ")");
  return true;
}

extern "C" {

int32_t crl_ddpg_create(const crl_ddpg_config* cfg, int32_t device, crl_ddpg** out) {
  if (!cfg || !out) { set_error("crl_ddpg_create: null argument"); return 1; }
  *out = nullptr;
  return ddpg_create(cfg, nullptr, nullptr, device, out);
}

int32_t crl_td3_create(const crl_ddpg_config* cfg, const crl_td3_options* opt, int32_t device, crl_ddpg** out) {
  if (!cfg || !out) { set_error("crl_td3_create: null argument"); return 1; }
  *out = nullptr;
  if (!opt) { set_error("crl_td3_create: options must not be NULL (crl_td3_options: policy_delay, policy_noise, noise_clip)"); return 1; }
  if (opt->policy_delay < 1) { set_error("crl_td3_create: policy_delay must be >= 1"); return 1; }
  if (!(opt->policy_noise >= 0.0)) { set_error("crl_td3_create: policy_noise must be >= 0"); return 1; }
  if (!(opt->noise_clip >= 0.0)) { set_error("crl_td3_create: noise_clip must be >= 0"); return 1; }
  if (cfg->noise_in_update != 0) {
    set_error("crl_td3_create: noise_in_update must be 0 (TD3 has its own target noise, policy_noise / noise_clip, and none in the actor loss)"); return 1;
  }
  return ddpg_create(cfg, opt, nullptr, device, out);
}

int32_t crl_ddpg_destroy(crl_ddpg* h) {
  if (!h) return 0;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  DDPGDev& d = h->d;
  void* ptrs[] = {d.actor, d.actor_t, d.ma, d.va, d.critic, d.critic_t, d.mc, d.vc, d.betap, d.ctl, d.eps, d.losses, d.rb_state, d.rb_next, d.rb_action,
                  d.rb_reward, d.rb_terminal, d.idx, d.X, d.cH1, d.cH2, d.cD1, d.cD2, d.dz, d.sq, d.aH1, d.aH2, d.aD1, d.aD2, d.aY, d.aD3, d.Qa, d.stage,
                  h->scratch, h->sd.log_alpha, h->sd.lp, h->sd.sctl, h->sd.arecs};
  for (void* p : ptrs) if (p) (void)hipFree(p);
  if (h->pinned) (void)hipHostFree(h->pinned);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
  return 0;
}

int32_t crl_ddpg_write_params(crl_ddpg* h, const float* actor, size_t actor_n, const float* critic, size_t critic_n) {
  DDPG_GUARD(h);
  if (wrong_kind(h, 0, "crl_ddpg_write_params")) return 1;
  if (!actor || !critic || actor_n != (size_t)h->na || critic_n != (size_t)h->nc) {
    set_error("crl_ddpg_write_params: expected " + std::to_string(h->na) + " actor and " + std::to_string(h->nc) + " critic floats"); return 1;
  }
  CRL_HIP_CHECK(hipStreamSynchronize(h->stream));
  CRL_HIP_CHECK(hipMemcpy(h->d.actor, actor, actor_n * 4, hipMemcpyHostToDevice));
  CRL_HIP_CHECK(hipMemcpy(h->d.actor_t, actor, actor_n * 4, hipMemcpyHostToDevice));     // ddpg.jl:53 deepcopy(actor)
  CRL_HIP_CHECK(hipMemcpy(h->d.critic, critic, critic_n * 4, hipMemcpyHostToDevice));
  CRL_HIP_CHECK(hipMemcpy(h->d.critic_t, critic, critic_n * 4, hipMemcpyHostToDevice));  // ddpg.jl:54 deepcopy(critic)
  h->params_set = true;
  return 0;
}
int32_t crl_ddpg_init_params(crl_ddpg* h, uint64_t seed) {
  DDPG_GUARD(h);
  if (wrong_kind(h, 0, "crl_ddpg_init_params")) return 1;
  std::vector<float> wa((size_t)h->na), wc((size_t)h->nc);
  if (crl_ddpg_make_nn(h->cfg.obs_dim, h->cfg.act_dim, seed, wa.data(), wa.size(), wc.data(), wc.size())) return 1;
  return crl_ddpg_write_params(h, wa.data(), wa.size(), wc.data(), wc.size());
}
int32_t crl_ddpg_read_params(crl_ddpg* h, float* actor, float* critic, float* target_actor, float* target_critic) {
  DDPG_GUARD(h);
  if (wrong_kind(h, 0, "crl_ddpg_read_params")) return 1;
  CRL_HIP_CHECK(hipStreamSynchronize(h->stream));
  if (actor) CRL_HIP_CHECK(hipMemcpy(actor, h->d.actor, (size_t)h->na * 4, hipMemcpyDeviceToHost));
  if (critic) CRL_HIP_CHECK(hipMemcpy(critic, h->d.critic, (size_t)h->nc * 4, hipMemcpyDeviceToHost));
  if (target_actor) CRL_HIP_CHECK(hipMemcpy(target_actor, h->d.actor_t, (size_t)h->na * 4, hipMemcpyDeviceToHost));
  if (target_critic) CRL_HIP_CHECK(hipMemcpy(target_critic, h->d.critic_t, (size_t)h->nc * 4, hipMemcpyDeviceToHost));
  return 0;
}

static int ddpg_read_ctl(crl_ddpg* h, DDPGCtl& c) {
  CRL_HIP_CHECK(hipMemcpyAsync(&c, h->d.ctl, sizeof(c), hipMemcpyDeviceToHost, h->stream));
  CRL_HIP_CHECK(hipStreamSynchronize(h->stream));
  return 0;
}

int32_t crl_ddpg_status_read(crl_ddpg* h, crl_ddpg_status* out) {
  DDPG_GUARD(h);
  if (!out) { set_error("null argument"); return 1; }
  DDPGCtl c;
  if (ddpg_read_ctl(h, c)) return 1;
  out->theta = c.env[0]; out->theta_dot = c.env[1]; out->env_t = c.env_t; out->global_step = c.global_step; out->rb_size = c.size; out->rb_ptr = c.ptr;
  out->n_updates = c.n_updates; out->actor_loss = c.actor_loss; out->critic_loss = c.critic_loss;
  return 0;
}

// copies the first min(n_losses, cap, max_losses) records out; c was just read
static int ddpg_copy_losses(crl_ddpg* h, const DDPGCtl& c, crl_ddpg_loss_record* losses, int32_t max_losses, int32_t* n_losses) {
  int nl = c.n_losses < DDPG_MAX_LOSSES ? c.n_losses : DDPG_MAX_LOSSES; if (nl > max_losses) nl = max_losses;
  if (nl > 0) {
    CRL_HIP_CHECK(hipMemcpyAsync(losses, h->d.losses, sizeof(crl_ddpg_loss_record) * (size_t)nl, hipMemcpyDeviceToHost, h->stream));
    CRL_HIP_CHECK(hipStreamSynchronize(h->stream));
  }
  if (h->sac) {                                                                        // what crl_sac_alpha_records hands out
    h->arecs.resize((size_t)(nl > 0 ? nl : 0));
    if (nl > 0) CRL_HIP_CHECK(hipMemcpy(h->arecs.data(), h->sd.arecs, sizeof(crl_sac_alpha_record) * (size_t)nl, hipMemcpyDeviceToHost));
  }
  *n_losses = nl;
  return 0;
}

int32_t crl_ddpg_run(crl_ddpg* h, int64_t max_env_steps, crl_ddpg_episode* eps, int32_t max_eps, int32_t* n_eps,
                     crl_ddpg_loss_record* losses, int32_t max_losses, int32_t* n_losses, int64_t* steps_taken) {
  DDPG_GUARD(h);
  if (h->cfg.env_kind != CRL_DDPG_ENV_PENDULUM) { set_error("crl_ddpg_run: the env of this handle lives in the host process — crl_ddpg_act / crl_ddpg_observe"); return 1; }
  if (params_unset(h, "crl_ddpg_run", "; a fresh handle holds zeros")) return 1;
  if (!n_eps || !n_losses || max_eps < 0 || max_losses < 0 || (max_eps > 0 && !eps) || (max_losses > 0 && !losses)) {
    set_error("crl_ddpg_run: bad arguments"); return 1;
  }
  *n_eps = 0; *n_losses = 0;
  h->arecs.clear();
  if (steps_taken) *steps_taken = 0;
  if (max_env_steps <= 0) return 0;
  const DDPGDev& d = h->d;
  hipStream_t st = h->stream;
  // steps this call can take; the ones up to max(min_buff_size, warmup_steps) run inside ONE collect launch, every later one is a cycle of its own,
  // and one more cycle closes the last update
  const int64_t left = h->cfg.total_timesteps - h->host_step;
  const int64_t limit = left < max_env_steps ? (left > 0 ? left : 0) : max_env_steps;
  const int64_t thr = h->cfg.min_buff_size > h->cfg.warmup_steps ? h->cfg.min_buff_size : h->cfg.warmup_steps;
  const int64_t quiet = thr > h->host_step ? thr - h->host_step : 0;
  const int64_t cycles = (limit > quiet ? limit - quiet : 0) + 2;
  hipLaunchKernelGGL(ddpg_begin_kernel, dim3(1), dim3(1), 0, st, d, max_env_steps);
  for (int64_t cy = 0; cy < cycles; ++cy) {
    enqueue_cycle(h);
    if ((cy & 4095) == 4095) CRL_HIP_CHECK(hipStreamSynchronize(st));   // bound the queue depth of very long calls
  }
  CRL_HIP_CHECK(hipGetLastError());
  DDPGCtl c;
  if (ddpg_read_ctl(h, c)) return 1;
  h->host_step = c.global_step;
  if (steps_taken) *steps_taken = c.taken;
  int ne = c.n_eps < DDPG_MAX_EPS ? c.n_eps : DDPG_MAX_EPS; if (ne > max_eps) ne = max_eps;
  if (ne > 0) CRL_HIP_CHECK(hipMemcpyAsync(eps, h->d.eps, sizeof(crl_ddpg_episode) * (size_t)ne, hipMemcpyDeviceToHost, h->stream));
  CRL_HIP_CHECK(hipStreamSynchronize(h->stream));
  *n_eps = ne;
  return ddpg_copy_losses(h, c, losses, max_losses, n_losses);
}

int32_t crl_ddpg_act(crl_ddpg* h, const double* obs, double* action_out) {
  DDPG_GUARD(h);
  if (h->cfg.env_kind != CRL_DDPG_ENV_EXTERNAL) { set_error("crl_ddpg_act: this handle steps its own Pendulum — crl_ddpg_run"); return 1; }
  if (params_unset(h, "crl_ddpg_act")) return 1;
  if (!obs || !action_out) { set_error("crl_ddpg_act: null argument"); return 1; }
  const size_t D = (size_t)h->cfg.obs_dim, A = (size_t)h->cfg.act_dim;
  CRL_HIP_CHECK(hipStreamSynchronize(h->stream));                      // the pinned slot is free again
  memcpy(h->pinned, obs, D * 8);
  CRL_HIP_CHECK(hipMemcpyAsync(h->d.stage, h->pinned, D * 8, hipMemcpyHostToDevice, h->stream));
  if (h->sac) hipLaunchKernelGGL(sac_act_kernel, dim3(1), dim3(64), 0, h->stream, h->d);
  else hipLaunchKernelGGL(ddpg_act_kernel, dim3(1), dim3(64), 0, h->stream, h->d);
  CRL_HIP_CHECK(hipGetLastError());
  CRL_HIP_CHECK(hipMemcpyAsync(h->pinned + 2 * D + A + 2, h->d.stage + 2 * D + A + 2, A * 8, hipMemcpyDeviceToHost, h->stream));
  CRL_HIP_CHECK(hipStreamSynchronize(h->stream));
  memcpy(action_out, h->pinned + 2 * D + A + 2, A * 8);
  return 0;
}

int32_t crl_ddpg_observe(crl_ddpg* h, const double* obs, const double* action, double reward, const double* next_obs, int32_t terminal) {
  DDPG_GUARD(h);
  if (h->cfg.env_kind != CRL_DDPG_ENV_EXTERNAL) { set_error("crl_ddpg_observe: this handle steps its own Pendulum — crl_ddpg_run"); return 1; }
  if (params_unset(h, "crl_ddpg_observe")) return 1;
  if (!obs || !action || !next_obs) { set_error("crl_ddpg_observe: null argument"); return 1; }
  if (h->host_step >= h->cfg.total_timesteps) { set_error("crl_ddpg_observe: total_timesteps steps were already taken"); return 1; }
  const size_t D = (size_t)h->cfg.obs_dim, A = (size_t)h->cfg.act_dim;
  CRL_HIP_CHECK(hipStreamSynchronize(h->stream));                      // the pinned slot is free again
  double* s = h->pinned;
  memcpy(s, obs, D * 8); memcpy(s + D, action, A * 8); s[D + A] = reward; memcpy(s + D + A + 1, next_obs, D * 8); s[2 * D + A + 1] = terminal ? 1.0 : 0.0;
  CRL_HIP_CHECK(hipMemcpyAsync(h->d.stage, s, (2 * D + A + 2) * 8, hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(ddpg_add_kernel, dim3(1), dim3(64), 0, h->stream, h->d);
  h->host_step += 1;
  if (h->host_step > h->cfg.min_buff_size && h->host_step > h->cfg.warmup_steps) {    // ddpg.jl:105 (the kernels check train_pending themselves)
    enqueue_cycle(h);                                                                  // external: the collect launch closes the update only
  }
  CRL_HIP_CHECK(hipGetLastError());
  return 0;
}

int32_t crl_ddpg_read_losses(crl_ddpg* h, crl_ddpg_loss_record* losses, int32_t max_losses, int32_t* n_losses) {
  DDPG_GUARD(h);
  if (!n_losses || max_losses < 0 || (max_losses > 0 && !losses)) { set_error("crl_ddpg_read_losses: bad arguments"); return 1; }
  DDPGCtl c;
  if (ddpg_read_ctl(h, c)) return 1;
  if (ddpg_copy_losses(h, c, losses, max_losses, n_losses)) return 1;
  hipLaunchKernelGGL(ddpg_clear_losses_kernel, dim3(1), dim3(1), 0, h->stream, h->d);
  CRL_HIP_CHECK(hipStreamSynchronize(h->stream));
  return 0;
}

int32_t crl_ddpg_read_buffer(crl_ddpg* h, double* state, double* action, double* reward, double* next_state, uint8_t* terminal, int64_t cap,
                             int64_t* ptr, int64_t* size) {
  DDPG_GUARD(h);
  if (cap != h->cfg.buffer_size) { set_error("crl_ddpg_read_buffer: cap must be buffer_size"); return 1; }
  const size_t n = (size_t)cap, D = (size_t)h->cfg.obs_dim, A = (size_t)h->cfg.act_dim;
  DDPGCtl c;
  if (ddpg_read_ctl(h, c)) return 1;
  if (state) CRL_HIP_CHECK(hipMemcpy(state, h->d.rb_state, n * D * 8, hipMemcpyDeviceToHost));
  if (action) CRL_HIP_CHECK(hipMemcpy(action, h->d.rb_action, n * A * 8, hipMemcpyDeviceToHost));
  if (reward) CRL_HIP_CHECK(hipMemcpy(reward, h->d.rb_reward, n * 8, hipMemcpyDeviceToHost));
  if (next_state) CRL_HIP_CHECK(hipMemcpy(next_state, h->d.rb_next, n * D * 8, hipMemcpyDeviceToHost));
  if (terminal) CRL_HIP_CHECK(hipMemcpy(terminal, h->d.rb_terminal, n, hipMemcpyDeviceToHost));
  if (ptr) *ptr = c.ptr;
  if (size) *size = c.size;
  return 0;
}

int32_t crl_ddpg_actor(crl_ddpg* h, const double* obs, int32_t n, double* out) {
  DDPG_GUARD(h);
  if (params_unset(h, "crl_ddpg_actor")) return 1;
  if (n < 0 || (n > 0 && (!obs || !out))) { set_error("crl_ddpg_actor: bad arguments"); return 1; }
  if (n == 0) return 0;
  const size_t N = (size_t)n, D = (size_t)h->cfg.obs_dim, A = (size_t)h->cfg.act_dim;
  if (ddpg_scratch(h, N * (D + A) * 8)) return 1;
  double* so = static_cast<double*>(h->scratch);
  double* sa = so + N * D;
  CRL_HIP_CHECK(hipMemcpyAsync(so, obs, N * D * 8, hipMemcpyHostToDevice, h->stream));
  if (h->sac) hipLaunchKernelGGL(sac_actor_eval_kernel, dim3(n), dim3(64), 0, h->stream, h->d, so, n, sa);
  else hipLaunchKernelGGL(ddpg_actor_eval_kernel, dim3(n), dim3(64), 0, h->stream, h->d, so, n, sa);
  CRL_HIP_CHECK(hipGetLastError());
  CRL_HIP_CHECK(hipMemcpyAsync(out, sa, N * A * 8, hipMemcpyDeviceToHost, h->stream));
  CRL_HIP_CHECK(hipStreamSynchronize(h->stream));
  return 0;
}

}  // extern "C"

// get_q of critic `which` (0; 1 on a TD3 handle) for n staged pairs
static int32_t ddpg_q_eval(crl_ddpg* h, int which, const double* obs, const double* act, int32_t n, double* out) {
  const size_t N = (size_t)n, D = (size_t)h->cfg.obs_dim, A = (size_t)h->cfg.act_dim;
  if (ddpg_scratch(h, N * (D + A + 1) * 8)) return 1;
  double* so = static_cast<double*>(h->scratch);
  double* sa = so + N * D;
  double* sq = sa + N * A;
  CRL_HIP_CHECK(hipMemcpyAsync(so, obs, N * D * 8, hipMemcpyHostToDevice, h->stream));
  CRL_HIP_CHECK(hipMemcpyAsync(sa, act, N * A * 8, hipMemcpyHostToDevice, h->stream));
  DDPGDev d = h->d;
  d.critic += (size_t)which * (size_t)h->nc;
  hipLaunchKernelGGL(ddpg_q_eval_kernel, dim3(n), dim3(64), 0, h->stream, d, so, sa, n, sq);
  CRL_HIP_CHECK(hipGetLastError());
  CRL_HIP_CHECK(hipMemcpyAsync(out, sq, N * 8, hipMemcpyDeviceToHost, h->stream));
  CRL_HIP_CHECK(hipStreamSynchronize(h->stream));
  return 0;
}

extern "C" {

int32_t crl_ddpg_q_values(crl_ddpg* h, const double* obs, const double* act, int32_t n, double* out) {
  DDPG_GUARD(h);
  if (params_unset(h, "crl_ddpg_q_values")) return 1;
  if (n < 0 || (n > 0 && (!obs || !act || !out))) { set_error("crl_ddpg_q_values: bad arguments"); return 1; }
  if (n == 0) return 0;
  return ddpg_q_eval(h, 0, obs, act, n, out);
}

int32_t crl_td3_q_values(crl_ddpg* h, const double* obs, const double* act, int32_t n, double* q1, double* q2) {
  DDPG_GUARD(h);
  if (wrong_kind(h, 1, "crl_td3_q_values")) return 1;
  if (!h->params_set) { set_error("crl_td3_q_values: parameters not set — crl_td3_write_params or crl_td3_init_params first"); return 1; }
  if (n < 0 || (n > 0 && (!obs || !act))) { set_error("crl_td3_q_values: bad arguments"); return 1; }
  if (n == 0) return 0;
  if (q1 && ddpg_q_eval(h, 0, obs, act, n, q1)) return 1;
  if (q2 && ddpg_q_eval(h, 1, obs, act, n, q2)) return 1;
  return 0;
}

int32_t crl_td3_write_params(crl_ddpg* h, const float* actor, size_t actor_n, const float* critic1, size_t critic1_n, const float* critic2,
                             size_t critic2_n) {
  DDPG_GUARD(h);
  if (wrong_kind(h, 1, "crl_td3_write_params")) return 1;
  const size_t na = (size_t)h->na, nc = (size_t)h->nc;
  if (!actor || !critic1 || !critic2 || actor_n != na || critic1_n != nc || critic2_n != nc) {
    set_error("crl_td3_write_params: expected " + std::to_string(na) + " actor floats and " + std::to_string(nc) + " floats for each critic"); return 1;
  }
  CRL_HIP_CHECK(hipStreamSynchronize(h->stream));
  for (float* dst : {h->d.actor, h->d.actor_t}) CRL_HIP_CHECK(hipMemcpy(dst, actor, na * 4, hipMemcpyHostToDevice));
  for (float* dst : {h->d.critic, h->d.critic_t}) {                                       // the targets are copies, as ddpg.jl:53-54
    CRL_HIP_CHECK(hipMemcpy(dst, critic1, nc * 4, hipMemcpyHostToDevice));
    CRL_HIP_CHECK(hipMemcpy(dst + nc, critic2, nc * 4, hipMemcpyHostToDevice));
  }
  h->params_set = true;
  return 0;
}
int32_t crl_td3_init_params(crl_ddpg* h, uint64_t seed) {
  DDPG_GUARD(h);
  if (wrong_kind(h, 1, "crl_td3_init_params")) return 1;
  std::vector<float> wa((size_t)h->na), wc1((size_t)h->nc), wa2((size_t)h->na), wc2((size_t)h->nc);
  if (crl_ddpg_make_nn(h->cfg.obs_dim, h->cfg.act_dim, seed, wa.data(), wa.size(), wc1.data(), wc1.size())) return 1;
  if (crl_ddpg_make_nn(h->cfg.obs_dim, h->cfg.act_dim, seed + 1, wa2.data(), wa2.size(), wc2.data(), wc2.size())) return 1;   // its actor is dropped
  return crl_td3_write_params(h, wa.data(), wa.size(), wc1.data(), wc1.size(), wc2.data(), wc2.size());
}
int32_t crl_td3_read_params(crl_ddpg* h, float* actor, float* critic1, float* critic2, float* target_actor, float* target_critic1,
                            float* target_critic2) {
  DDPG_GUARD(h);
  if (wrong_kind(h, 1, "crl_td3_read_params")) return 1;
  CRL_HIP_CHECK(hipStreamSynchronize(h->stream));
  const size_t na = (size_t)h->na, nc = (size_t)h->nc;
  if (actor) CRL_HIP_CHECK(hipMemcpy(actor, h->d.actor, na * 4, hipMemcpyDeviceToHost));
  if (critic1) CRL_HIP_CHECK(hipMemcpy(critic1, h->d.critic, nc * 4, hipMemcpyDeviceToHost));
  if (critic2) CRL_HIP_CHECK(hipMemcpy(critic2, h->d.critic + nc, nc * 4, hipMemcpyDeviceToHost));
  if (target_actor) CRL_HIP_CHECK(hipMemcpy(target_actor, h->d.actor_t, na * 4, hipMemcpyDeviceToHost));
  if (target_critic1) CRL_HIP_CHECK(hipMemcpy(target_critic1, h->d.critic_t, nc * 4, hipMemcpyDeviceToHost));
  if (target_critic2) CRL_HIP_CHECK(hipMemcpy(target_critic2, h->d.critic_t + nc, nc * 4, hipMemcpyDeviceToHost));
  return 0;
}

// ---- SAC: the crl_sac_* block
int32_t crl_sac_param_count(int32_t obs_dim, int32_t act_dim, int64_t* actor_n, int64_t* critic_n) {
  if (obs_dim < 1 || obs_dim > DDPG_MAX_OBS) { set_error("crl_sac_param_count: obs_dim must be in 1..64"); return 1; }
  if (act_dim < 1 || act_dim > DDPG_MAX_ACT) { set_error("crl_sac_param_count: act_dim must be in 1..16"); return 1; }
  if (actor_n) *actor_n = net_off(obs_dim, 2 * act_dim).N;
  if (critic_n) *critic_n = net_off(obs_dim + act_dim, 1).N;
  return 0;
}

int32_t crl_sac_create(const crl_ddpg_config* cfg, const crl_sac_options* opt, int32_t device, crl_ddpg** out) {
  if (!cfg || !out) { set_error("crl_sac_create: null argument"); return 1; }
  *out = nullptr;
  if (!opt) { set_error("crl_sac_create: options must not be NULL (crl_sac_options: autotune, alpha, target_entropy)"); return 1; }
  if (opt->autotune != 0 && opt->autotune != 1) { set_error("crl_sac_create: autotune must be 0 or 1"); return 1; }
  if (!(opt->alpha > 0.0) || !std::isfinite(opt->alpha)) { set_error("crl_sac_create: alpha must be > 0 and finite"); return 1; }
  if (!std::isfinite(opt->target_entropy)) { set_error("crl_sac_create: target_entropy must be finite"); return 1; }
  if (cfg->noise_in_update != 0) {
    set_error("crl_sac_create: noise_in_update must be 0 (SAC samples its actions from the policy; exploration_noise is not read)"); return 1;
  }
  return ddpg_create(cfg, nullptr, opt, device, out);
}

int32_t crl_sac_write_params(crl_ddpg* h, const float* actor, size_t actor_n, const float* critic1, size_t critic1_n, const float* critic2,
                             size_t critic2_n) {
  DDPG_GUARD(h);
  if (wrong_kind(h, 2, "crl_sac_write_params")) return 1;
  const size_t na = (size_t)h->na, nc = (size_t)h->nc;
  if (!actor || !critic1 || !critic2 || actor_n != na || critic1_n != nc || critic2_n != nc) {
    set_error("crl_sac_write_params: expected " + std::to_string(na) + " actor floats and " + std::to_string(nc) + " floats for each critic"); return 1;
  }
  CRL_HIP_CHECK(hipStreamSynchronize(h->stream));
  CRL_HIP_CHECK(hipMemcpy(h->d.actor, actor, na * 4, hipMemcpyHostToDevice));
  for (float* dst : {h->d.critic, h->d.critic_t}) {                                       // the targets are copies
    CRL_HIP_CHECK(hipMemcpy(dst, critic1, nc * 4, hipMemcpyHostToDevice));
    CRL_HIP_CHECK(hipMemcpy(dst + nc, critic2, nc * 4, hipMemcpyHostToDevice));
  }
  h->params_set = true;
  return 0;
}
int32_t crl_sac_init_params(crl_ddpg* h, uint64_t seed) {
  DDPG_GUARD(h);
  if (wrong_kind(h, 2, "crl_sac_init_params")) return 1;
  std::vector<float> wa((size_t)h->na), wc1((size_t)h->nc), wc2((size_t)h->nc);
  if (crl_sac_make_nn(h->cfg.obs_dim, h->cfg.act_dim, seed, wa.data(), wa.size(), wc1.data(), wc1.size(), wc2.data(), wc2.size())) return 1;
  return crl_sac_write_params(h, wa.data(), wa.size(), wc1.data(), wc1.size(), wc2.data(), wc2.size());
}
int32_t crl_sac_read_params(crl_ddpg* h, float* actor, float* critic1, float* critic2, float* target_critic1, float* target_critic2, float* log_alpha) {
  DDPG_GUARD(h);
  if (wrong_kind(h, 2, "crl_sac_read_params")) return 1;
  CRL_HIP_CHECK(hipStreamSynchronize(h->stream));
  const size_t na = (size_t)h->na, nc = (size_t)h->nc;
  if (actor) CRL_HIP_CHECK(hipMemcpy(actor, h->d.actor, na * 4, hipMemcpyDeviceToHost));
  if (critic1) CRL_HIP_CHECK(hipMemcpy(critic1, h->d.critic, nc * 4, hipMemcpyDeviceToHost));
  if (critic2) CRL_HIP_CHECK(hipMemcpy(critic2, h->d.critic + nc, nc * 4, hipMemcpyDeviceToHost));
  if (target_critic1) CRL_HIP_CHECK(hipMemcpy(target_critic1, h->d.critic_t, nc * 4, hipMemcpyDeviceToHost));
  if (target_critic2) CRL_HIP_CHECK(hipMemcpy(target_critic2, h->d.critic_t + nc, nc * 4, hipMemcpyDeviceToHost));
  if (log_alpha) CRL_HIP_CHECK(hipMemcpy(log_alpha, h->sd.log_alpha, 4, hipMemcpyDeviceToHost));
  return 0;
}
int32_t crl_sac_q_values(crl_ddpg* h, const double* obs, const double* act, int32_t n, double* q1, double* q2) {
  DDPG_GUARD(h);
  if (wrong_kind(h, 2, "crl_sac_q_values")) return 1;
  if (!h->params_set) { set_error("crl_sac_q_values: parameters not set — crl_sac_write_params or crl_sac_init_params first"); return 1; }
  if (n < 0 || (n > 0 && (!obs || !act))) { set_error("crl_sac_q_values: bad arguments"); return 1; }
  if (n == 0) return 0;
  if (q1 && ddpg_q_eval(h, 0, obs, act, n, q1)) return 1;
  if (q2 && ddpg_q_eval(h, 1, obs, act, n, q2)) return 1;
  return 0;
}
int32_t crl_sac_status_read(crl_ddpg* h, crl_sac_status* out) {
  DDPG_GUARD(h);
  if (wrong_kind(h, 2, "crl_sac_status_read", "crl_ddpg_status_read")) return 1;
  if (!out) { set_error("crl_sac_status_read: null argument"); return 1; }
  SACCtl sc;
  CRL_HIP_CHECK(hipStreamSynchronize(h->stream));
  CRL_HIP_CHECK(hipMemcpy(&sc, h->sd.sctl, sizeof(sc), hipMemcpyDeviceToHost));
  CRL_HIP_CHECK(hipMemcpy(&out->log_alpha, h->sd.log_alpha, 4, hipMemcpyDeviceToHost));
  out->alpha = sc.alpha; out->alpha_loss = sc.alpha_loss; out->entropy = sc.entropy; out->pad = 0;
  return 0;
}
int32_t crl_sac_alpha_records(crl_ddpg* h, crl_sac_alpha_record* records, int32_t max_records, int32_t* n_records) {
  DDPG_GUARD(h);
  if (wrong_kind(h, 2, "crl_sac_alpha_records", NO_TWIN)) return 1;
  if (!n_records || max_records < 0 || (max_records > 0 && !records)) { set_error("crl_sac_alpha_records: bad arguments"); return 1; }
  const size_t n = h->arecs.size() < (size_t)max_records ? h->arecs.size() : (size_t)max_records;
  if (n > 0) memcpy(records, h->arecs.data(), n * sizeof(crl_sac_alpha_record));
  *n_records = (int32_t)n;
  return 0;
}

// Held-out evaluation: argument checks, scratch, ONE launch (ddpg_eval_kernel), the per-episode arrays back to the host, the report in Float64
int32_t crl_ddpg_evaluate(crl_ddpg* h, const crl_ddpg_eval_config* cfg, crl_ddpg_eval_report* report, double* returns, double* disc_returns,
                          double* q0, double* trace_action) {
#pragma clang fp contract(off)
  DDPG_GUARD(h);
  if (!cfg || !report) { set_error("crl_ddpg_evaluate: null cfg or report"); return 1; }
  if (h->cfg.env_kind != CRL_DDPG_ENV_PENDULUM) {
    set_error("crl_ddpg_evaluate: the env of this handle lives in the host process — step it there and take the noise-free actions from crl_ddpg_actor");
    return 1;
  }
  if (params_unset(h, "crl_ddpg_evaluate")) return 1;
  const int64_t n = cfg->num_envs, E = cfg->episodes_per_env, T = cfg->trace_steps, steps = E * (int64_t)h->cfg.max_steps;
  if (n < 1 || n > 65536) { set_error("crl_ddpg_evaluate: num_envs must be in 1..65536, got " + std::to_string(n)); return 1; }
  if (E < 1 || E > 1024) { set_error("crl_ddpg_evaluate: episodes_per_env must be in 1..1024, got " + std::to_string(E)); return 1; }
  if (n * E > (1 << 20)) { set_error("crl_ddpg_evaluate: num_envs * episodes_per_env must be <= 1048576, got " + std::to_string(n * E)); return 1; }
  if (T < 0 || T > steps) {
    set_error("crl_ddpg_evaluate: trace_steps must be in 0..episodes_per_env * max_steps = " + std::to_string(steps) + ", got " + std::to_string(T)); return 1;
  }
  if ((T > 0) != (trace_action != nullptr)) { set_error("crl_ddpg_evaluate: trace_action must be given exactly when trace_steps > 0"); return 1; }
  if (T * n > (1 << 24)) { set_error("crl_ddpg_evaluate: trace_steps * num_envs must be <= 16777216, got " + std::to_string(T * n)); return 1; }
  const size_t ne = (size_t)(n * E), nt = (size_t)(T * n);
  if (ddpg_scratch(h, (3 * ne + nt) * 8)) return 1;
  DDPGEvalArgs ev;
  ev.n = (int32_t)n; ev.episodes = (int32_t)E; ev.trace_steps = (int32_t)T; ev.head_rows = h->sac ? 2 : 1; ev.seed = cfg->seed;
  ev.ret = static_cast<double*>(h->scratch); ev.disc_ret = ev.ret + ne; ev.q0 = ev.disc_ret + ne; ev.trace = ev.q0 + ne;
  // every slot of the four arrays is written: each env runs episodes_per_env episodes of exactly max_steps steps
  hipLaunchKernelGGL(ddpg_eval_kernel, dim3((unsigned)((n + EVAL_WAVES - 1) / EVAL_WAVES)), dim3(64 * EVAL_WAVES), 0, h->stream, h->d, ev);
  CRL_HIP_CHECK(hipGetLastError());
  std::vector<double> host(3 * ne);
  CRL_HIP_CHECK(hipMemcpyAsync(host.data(), ev.ret, 3 * ne * 8, hipMemcpyDeviceToHost, h->stream));
  if (T > 0) CRL_HIP_CHECK(hipMemcpyAsync(trace_action, ev.trace, nt * 8, hipMemcpyDeviceToHost, h->stream));
  CRL_HIP_CHECK(hipStreamSynchronize(h->stream));   // host buffers are only borrowed for the call
  const double *ret = host.data(), *disc = ret + ne, *q = disc + ne;
  double rsum = 0.0, dsum = 0.0, qsum = 0.0, bsum = 0.0, rmin = ret[0], rmax = ret[0];
  for (size_t i = 0; i < ne; ++i) {
    rsum += ret[i]; dsum += disc[i]; qsum += q[i]; bsum += q[i] - disc[i];
    rmin = ret[i] < rmin ? ret[i] : rmin; rmax = ret[i] > rmax ? ret[i] : rmax;
  }
  const double mean = rsum / (double)ne;
  double var = 0.0;
  for (size_t i = 0; i < ne; ++i) { const double d = ret[i] - mean; var += d * d; }
  report->episodes = (int64_t)ne; report->env_steps = (int64_t)ne * h->cfg.max_steps;
  report->return_mean = mean; report->return_std = std::sqrt(var / (double)ne); report->return_min = rmin; report->return_max = rmax;
  report->disc_return_mean = dsum / (double)ne; report->q0_mean = qsum / (double)ne; report->q_bias_mean = bsum / (double)ne;
  if (returns) memcpy(returns, ret, ne * 8);
  if (disc_returns) memcpy(disc_returns, disc, ne * 8);
  if (q0) memcpy(q0, q, ne * 8);
  return 0;
}

}  // extern "C"
