// sac.hpp — SAC on the DDPG handle (the crl_sac_* block of include/cleanrl_hip.h), included by ddpg.hip: the kernels of what SAC adds. The ring, the
// draw, the env loop, the act / add kernels, the critic step and every building block (actor_hidden, head_row, critic_forward, w2t_row,
// twin_critic_pass, critic_param_grad, actor_param_grad, adam_entry, ddpg_collect, ddpg_act) are ddpg.hip's, called here. A SAC handle's critic,
// critic_t, mc, vc, cH1 .. sq are laid out as a TD3 handle's ([2][...]); its actor has a head of 2·act_dim rows (aD3 is [k][2A]); actor_t and aY are not allocated;
// betap holds 19 pairs: the actor's six arrays, critic 1's, critic 2's, log_alpha's. One cycle:
//   A   ddpg_sample_kernel  unchanged
//   B'' sac_critic_kernel   one block per sample, two waves, wave w = critic w: the actor on next_state and the sampled a', logπ' (both waves, each
//                           into its own LDS), target critic w, the min through LDS, the entropy term, then twin_critic_pass
//   C'' td3_critic_step     unchanged
//   D'' sac_actor_kernel    one block per sample, two waves: the actor on state and the sampled a, logπ (both waves); wave w runs the UPDATED critic w
//                           and its pullback to ∂(−Q_w/k)/∂a; the selected one goes through LDS; then δ3 (2A wide), δ2, δ1 (both waves alike, wave 0
//                           stores)
//   E'' sac_actor_step      first blocks: one actor parameter per thread (gradient in sample order, Adam, no polyak); thread 0 sums actor_loss,
//                           alpha_loss and the entropy in sample order and takes the log_alpha step. Following blocks: polyak of the 2·nc critic targets
//   F'' sac_collect_kernel  ddpg_collect with SAC's close (19 β-power pairs, log_alpha's only with autotune; the loss and alpha records) and SAC's
//                           behaviour policy
// Every __syncthreads() is reached by both waves of a block: the only early exit is the block-uniform one at the top, and both waves take every call
// alike. α of an update is read from log_alpha by B'', D'' and E'' before E'' writes it: ordering is by launch boundaries, as everywhere in ddpg.hip.
#pragma once

namespace crl {

constexpr uint32_t S_SAC_NEXT = 0x18u, S_SAC_PI = 0x19u;
constexpr int SAC_MAX_HEAD = 2 * DDPG_MAX_ACT, SAC_ALPHA_PAIR = 18;

struct SACCtl { double alpha, alpha_loss, entropy; };   // of the last update
struct SACDev {
  crl_sac_options opt;
  float* log_alpha;                  // [3]: log_alpha, its Adam m, its Adam v
  double* lp;                        // [k] logπ of the actor pass
  SACCtl* sctl;
  crl_sac_alpha_record* arecs;       // [DDPG_MAX_LOSSES], index = the loss record's
};

__device__ __forceinline__ double sac_alpha(const SACDev& sd) { return exp((double)sd.log_alpha[0]); }
__device__ __forceinline__ double sac_scale(const crl_ddpg_config& c) { return (c.act_high - c.act_low) / 2.0; }
__device__ __forceinline__ double sac_bias(const crl_ddpg_config& c) { return (c.act_high + c.act_low) / 2.0; }

// one component of the squashed Gaussian for head outputs (mu, s) and the normal eps: the header's expressions in the header's order
struct SacDraw { double t, sigma, y, act, lp; };
__device__ __forceinline__ SacDraw sac_squash(double mu, double s, double eps, double scale, double bias) {
#pragma clang fp contract(off)
  SacDraw d;
  d.t = tanh_fast64(s);
  const double log_std = -5.0 + 3.5 * (d.t + 1.0);
  d.sigma = exp(log_std);
  d.y = tanh_fast64(mu + d.sigma * eps);
  d.act = scale * d.y + bias;
  d.lp = ((-0.5 * (eps * eps) - log_std) - 0.9189385332046727) - log(scale * (1.0 - d.y * d.y) + 1e-6);
  return d;
}

// the SAC actor up to its linear head: zs[0..A) = μ, zs[A..2A) = s; h1, h2 per lane. Ends on the block's barrier.
__device__ __forceinline__ void sac_actor_head(const float* __restrict__ P, int D, int A, const double* x, double* h1s, double* h2s, double* zs, int lane,
                                               double& h1, double& h2) {
  const NetOff o = net_off(D, 2 * A);
  actor_hidden(P, o, D, x, h1s, h2s, lane, h1, h2);
  if (lane < 2 * A) zs[lane] = head_row(P + o.W3, P + o.b3, 2 * A, h2s, lane);
  __syncthreads();
}

// lane c < A: the sampled component for the draw (comp, gstep, stream), its action into act_out[c] and its logπ term into lps[c]; every lane returns
// logπ = Σ_c lps[c] (c ascending) after the block's barrier
__device__ __forceinline__ double sac_sample(const DDPGDev& a, const double* zs, uint32_t comp0, uint64_t gstep, uint32_t stream, double* act_out,
                                             double* lps, int lane, SacDraw& d, double& eps) {
#pragma clang fp contract(off)
  const int A = a.cfg.act_dim;
  if (lane < A) {
    eps = ddpg_normal(a.cfg.seed, comp0 + (uint32_t)lane, gstep, stream);
    d = sac_squash(zs[lane], zs[A + lane], eps, sac_scale(a.cfg), sac_bias(a.cfg));
    act_out[lane] = d.act; lps[lane] = d.lp;
  }
  __syncthreads();
  double lp = 0.0;
  for (int c = 0; c < A; ++c) lp += lps[c];
  return lp;
}

// B''.
__global__ void __launch_bounds__(128) sac_critic_kernel(DDPGDev a, SACDev sd) {
#pragma clang fp contract(off)
  if (!a.ctl->train_pending) return;
  __shared__ double xs[2][DDPG_MAX_IN], h1s[2][GH], h2s[2][GH], zs[2][SAC_MAX_HEAD], lps[2][DDPG_MAX_ACT], qs[2], d2s[2][GH];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, b = blockIdx.x, D = a.cfg.obs_dim, NI = D + a.cfg.act_dim;
  const uint64_t gstep = (uint64_t)a.ctl->global_step;
  const size_t s = (size_t)a.idx[b];
  const NetOff o = net_off(NI, 1);
  const float* const critic = a.critic + (size_t)w * o.N;
  const float* const critic_t = a.critic_t + (size_t)w * o.N;
  const double alpha = sac_alpha(sd);
  double h1, h2, eps = 0.0;
  SacDraw d{};
  for (int i = lane; i < D; i += GH) xs[w][i] = a.rb_next[D * s + i];
  __syncthreads();
  sac_actor_head(a.actor, D, a.cfg.act_dim, xs[w], h1s[w], h2s[w], zs[w], lane, h1, h2);
  const double lp = sac_sample(a, zs[w], (uint32_t)(16 * b), gstep, S_SAC_NEXT, xs[w] + D, lps[w], lane, d, eps);
  critic_forward(critic_t, NI, xs[w], h1s[w], h2s[w], &qs[w], lane, h1, h2);          // its last barrier publishes both qs
  const double q1 = qs[0], q2 = qs[1];
  const double next_q = q2 < q1 ? q2 : q1;
  const double td = a.rb_reward[s] + (a.cfg.gamma * (1.0 - (double)a.rb_terminal[s])) * (next_q - alpha * lp);
  __syncthreads();
  twin_critic_pass(a, critic, td, xs[w], h1s[w], h2s[w], &qs[w], d2s[w], lane, w, b, s);
}

// D''.
__global__ void __launch_bounds__(128) sac_actor_kernel(DDPGDev a, SACDev sd) {
#pragma clang fp contract(off)
  if (!a.ctl->train_pending) return;
  __shared__ double xs[2][DDPG_MAX_IN], h1s[2][GH], h2s[2][GH], zs[2][SAC_MAX_HEAD], lps[2][DDPG_MAX_ACT], qs[2], ds[2][GH], gas[2][DDPG_MAX_ACT],
      d3s[2][SAC_MAX_HEAD];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, b = blockIdx.x, D = a.cfg.obs_dim, A = a.cfg.act_dim, NI = D + A, k = (int)a.cfg.batch_size;
  const uint64_t gstep = (uint64_t)a.ctl->global_step;
  const NetOff oa = net_off(D, 2 * A), oc = net_off(NI, 1);
  const float* const critic = a.critic + (size_t)w * oc.N;
  const double alpha = sac_alpha(sd), scale = sac_scale(a.cfg);
  double ah1, ah2, ch1, ch2, eps = 0.0;
  SacDraw d{};
  for (int i = lane; i < D; i += GH) xs[w][i] = a.X[(size_t)NI * b + i];
  __syncthreads();
  sac_actor_head(a.actor, D, A, xs[w], h1s[w], h2s[w], zs[w], lane, ah1, ah2);
  const double lp = sac_sample(a, zs[w], (uint32_t)(16 * b), gstep, S_SAC_PI, xs[w] + D, lps[w], lane, d, eps);
  critic_forward(critic, NI, xs[w], h1s[w], h2s[w], &qs[w], lane, ch1, ch2);          // the updated critic w; publishes both qs
  const double q1 = qs[0], q2 = qs[1];
  const int sel = q2 < q1 ? 1 : 0;
  // back through critic w: ∂(−Q_w/k)/∂Q_w = −1/k, δ2, δ1, then ∂/∂a[c] = Σ_i W1[i, D + c]·δ1[i], i ascending
  const double dq = -1.0 / (double)k;
  ds[w][lane] = ch2 > 0.0 ? (double)critic[oc.W3 + lane] * dq : 0.0;
  __syncthreads();
  const double t1 = w2t_row(critic + oc.W2, ds[w], lane);
  __syncthreads();
  ds[w][lane] = ch1 > 0.0 ? t1 : 0.0;
  __syncthreads();
  if (lane < A) {
    double ga = 0.0;
#pragma unroll 8
    for (int i = 0; i < GH; ++i) ga += (double)critic[oc.W1 + i + GH * (D + lane)] * ds[w][i];
    gas[w][lane] = ga;
  }
  __syncthreads();
  if (lane < A) {                                                                     // the selected critic's ∂/∂a, then through the squash to μ and s
    const double ga = gas[sel][lane], ak = alpha / (double)k;
    const double omy = 1.0 - d.y * d.y;
    const double den = scale * omy + 1e-6;
    const double dy = ga * scale + ak * ((2.0 * scale * d.y) / den);
    const double du = dy * omy;
    const double dls = du * (d.sigma * eps) - ak;
    const double dsr = (dls * 3.5) * (1.0 - d.t * d.t);
    d3s[w][lane] = du; d3s[w][A + lane] = dsr;
    if (w == 0) { a.aD3[(size_t)(2 * A) * b + lane] = du; a.aD3[(size_t)(2 * A) * b + A + lane] = dsr; }
  }
  __syncthreads();
  double s2 = 0.0;
  for (int r = 0; r < 2 * A; ++r) s2 += (double)a.actor[oa.W3 + r + 2 * A * lane] * d3s[w][r];
  const double d2 = s2 * (1.0 - ah2 * ah2);
  ds[w][lane] = d2;
  __syncthreads();
  const double d1 = w2t_row(a.actor + oa.W2, ds[w], lane) * (1.0 - ah1 * ah1);
  if (w == 0) {
    const size_t r = (size_t)GH * b + lane;
    a.aH1[r] = ah1; a.aH2[r] = ah2; a.aD1[r] = d1; a.aD2[r] = d2;
    if (lane == 0) { a.Qa[b] = sel ? q2 : q1; sd.lp[b] = lp; }
  }
}

// E''. blocks 0..actor_blocks−1: the actor (and thread 0: the losses and the log_alpha step); the blocks after them: polyak of the 2·nc critic targets
__global__ void __launch_bounds__(64) sac_actor_step(DDPGDev a, SACDev sd, int actor_blocks, int nc2) {
#pragma clang fp contract(off)
  if (!a.ctl->train_pending) return;
  if ((int)blockIdx.x >= actor_blocks) {
    const int t = ((int)blockIdx.x - actor_blocks) * 64 + threadIdx.x;
    if (t < nc2) a.critic_t[t] = (float)(a.cfg.tau * (double)a.critic[t] + (1.0 - a.cfg.tau) * (double)a.critic_t[t]);
    return;
  }
  const int k = (int)a.cfg.batch_size, D = a.cfg.obs_dim, A = a.cfg.act_dim, p = blockIdx.x * 64 + threadIdx.x;
  const NetOff o = net_off(D, 2 * A);
  if (p == 0) {
    const double alpha = sac_alpha(sd), te = sd.opt.target_entropy;
    double sl = 0.0, se = 0.0, sp = 0.0;
    for (int b = 0; b < k; ++b) {
      const double lp = sd.lp[b];
      sl += alpha * lp - a.Qa[b]; se += lp + te; sp += lp;
    }
    const double al = -(alpha * (se / (double)k));
    a.ctl->actor_loss = sl / (double)k;
    sd.sctl->alpha = alpha; sd.sctl->alpha_loss = al; sd.sctl->entropy = -(sp / (double)k);
    if (sd.opt.autotune) {                                                             // ∂alpha_loss/∂log_alpha = alpha_loss
      const double* bp = a.betap + 2 * SAC_ALPHA_PAIR;
      float mi, vi, wi;
      adam_entry((double)(float)al, sd.log_alpha[1], sd.log_alpha[2], sd.log_alpha[0], bp[0], bp[1], a.cfg.lr, /*clip=*/false, 1.0, mi, vi, wi);
      sd.log_alpha[1] = mi; sd.log_alpha[2] = vi; sd.log_alpha[0] = wi;
    }
  }
  if (p >= o.N) return;
  const double g = actor_param_grad(a, o, D + A, 2 * A, k, p);
  const double* bp = a.betap + 2 * net_array(o, p);
  float mi, vi, wi;
  adam_entry((double)(float)g, a.ma[p], a.va[p], a.actor[p], bp[0], bp[1], a.cfg.lr, /*clip=*/false, 1.0, mi, vi, wi);
  a.ma[p] = mi; a.va[p] = vi; a.actor[p] = wi;
}

// the behaviour policy: DDPG's warm-up draw, then a sample from the actor with ε on stream 0x10, component word c
__device__ __forceinline__ auto sac_selector(const DDPGDev& a) {
  return [&a](uint64_t gstep, const double* xs, double* h1s, double* h2s, double* ys, double* act, int lane) {
    if ((int64_t)gstep <= a.cfg.warmup_steps) { ddpg_select_action(a, gstep, xs, h1s, h2s, ys, act, lane); return; }
    __shared__ double zs[SAC_MAX_HEAD], lps[DDPG_MAX_ACT];
    double h1, h2, eps = 0.0;
    SacDraw d{};
    sac_actor_head(a.actor, a.cfg.obs_dim, a.cfg.act_dim, xs, h1s, h2s, zs, lane, h1, h2);
    sac_sample(a, zs, 0u, gstep, S_BEHAVE, act, lps, lane, d, eps);
  };
}

// F''. 19 β-power pairs, log_alpha's only when it stepped; the alpha record beside the loss record
__global__ void __launch_bounds__(64) sac_collect_kernel(DDPGDev a, SACDev sd) {
  ddpg_collect(a, [&a, &sd](DDPGCtl& c, int lane) {
    if (lane <= SAC_ALPHA_PAIR && (lane < SAC_ALPHA_PAIR || sd.opt.autotune)) betap_advance(a.betap, lane, a.betap[2 * lane], a.betap[2 * lane + 1]);
    if (lane == 0) {
      const int rec = ddpg_log_update(a, c);
      if (rec >= 0) {
        sd.arecs[rec].global_step = c.global_step; sd.arecs[rec].alpha = sd.sctl->alpha; sd.arecs[rec].alpha_loss = sd.sctl->alpha_loss;
        sd.arecs[rec].entropy = sd.sctl->entropy;
      }
    }
  }, sac_selector(a));
}

__global__ void __launch_bounds__(64) sac_act_kernel(DDPGDev a) { ddpg_act(a, sac_selector(a)); }

// crl_ddpg_actor on a SAC handle: scale·tanh_fast(μ) + bias, one wave per column
__global__ void __launch_bounds__(64) sac_actor_eval_kernel(DDPGDev a, const double* __restrict__ obs, int n, double* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ double xs[DDPG_MAX_IN], h1s[GH], h2s[GH], zs[SAC_MAX_HEAD];
  const int lane = threadIdx.x, b = blockIdx.x, D = a.cfg.obs_dim, A = a.cfg.act_dim;
  if (b >= n) return;
  for (int i = lane; i < D; i += GH) xs[i] = obs[(size_t)D * b + i];
  __syncthreads();
  double h1, h2;
  sac_actor_head(a.actor, D, A, xs, h1s, h2s, zs, lane, h1, h2);
  if (lane < A) out[(size_t)A * b + lane] = sac_scale(a.cfg) * tanh_fast64(zs[lane]) + sac_bias(a.cfg);
}

}  // namespace crl
