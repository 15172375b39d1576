// ppo_gauss.hip — the kernels of a Gaussian PPO handle (crl_ppo_create_gaussian) on the layer-wise path: everything that knows what the actor's
// 2·act_dim head rows mean. The GEMMs, weight gradients, reduce, ClipNorm + Adam, GAE and shuffle of wide.hip run unchanged around them.
//   wide_step_gauss_kernel      one rollout step per env after the two forwards (wide_step_env<HeadGauss>, wide_step.hpp): a = μ + σ·ξ, Pendulum / synthetic env
//   wide_pack_rec_gauss_kernel  the batch as 64-byte records: a[8] | old logprob, old value, advantage, return | 16 B pad
//   wide_loss_gauss_kernel<G>   loss terms and head cotangents of one minibatch; G lanes per sample (below)
//   wide_sample_gauss_kernel / wide_logprob_gauss_kernel   the two probes on precomputed head outputs
//   pendulum_reset_kernel / pendulum_step_kernel           crl_env_reset / crl_env_step_gaussian
// The distribution's expressions live in ppo_gauss.hpp and are pinned in include/cleanrl_hip.h.
#include "env.hpp"
#include "ppo_ctx.hpp"
#include "ppo_gauss.hpp"
#include "stats.hpp"
#include "wide_step.hpp"

namespace crl {

__global__ void __launch_bounds__(256) wide_step_gauss_kernel(WStepArgs a, HeadGauss hd) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  double st_n = 0.0, st_ret = 0.0, st_len = 0.0, st_max = 0.0;
  if (e < a.c.nt) wide_step_env(a, hd, e, a.step, st_n, st_ret, st_len, st_max);
  episode_stats_flush(a.ep_stats, st_n, st_ret, st_len, st_max, head_signed_returns<HeadGauss>(a.c.env_kind));
}

// ------------------------------------------------------------------------------------------------------
// Record pack: what the loss kernel reads of a sample as ONE 64-byte piece (the discrete path's is 32 bytes: one action word instead of eight)
// ------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) wide_pack_rec_gauss_kernel(int B, int ad, const float* __restrict__ action_f, const float* __restrict__ logprob,
                                                                 const float* __restrict__ value, const float* __restrict__ adv,
                                                                 const float* __restrict__ ret, float* __restrict__ rec) {
  for (int b = blockIdx.x * 256 + threadIdx.x; b < B; b += gridDim.x * 256) {
    f32x4 r[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) r[q] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int i = 0; i < GAUSS_AMAX; ++i) if (i < ad) r[i >> 2][i & 3] = action_f[(size_t)ad * b + i];
    r[2][0] = logprob[b]; r[2][1] = value[b]; r[2][2] = adv[b]; r[2][3] = ret[b];
#pragma unroll
    for (int q = 0; q < 4; ++q) reinterpret_cast<f32x4*>(rec)[4 * (size_t)b + q] = r[q];
  }
}

// ------------------------------------------------------------------------------------------------------
// Loss terms and head cotangents of one minibatch on the Gaussian head (the policy half of ppo.jl:213-244 for a = μ + σ·ξ; the value half is
// wide_loss_kernel's). The split: a sample is up to 16 head values, 8 action words and — per component — one tanhf, one expf and one division, so one
// thread per sample would walk eight dependent transcendental chains over 16-register arrays. Here G = the power of two >= act_dim lanes share a
// sample, lane i owns component i: it reads μ_i, s_i and a_i (the group's loads are contiguous pieces of the sample's Z row and of its record), forms
// its two terms, and the group's logπ and H come from log2(G) cross-lane adds — pairwise: (i, i^1), then ^2, ^4. Every lane then holds the sample's
// ratio and dnlp and writes its own two cotangents (and the zero padding columns up to A8). A block still owns 256 consecutive minibatch positions —
// the lpart layout, the grid and wide_reduce_kernel stay wide_loss_kernel's — and walks them in G passes of 256 / G samples.
// ------------------------------------------------------------------------------------------------------
template <int G>
__global__ void __launch_bounds__(256) wide_loss_gauss_kernel(GaussLossArgs a) {
  constexpr int SPB = 256 / G;
  const int ad = a.g.ad, i = threadIdx.x % G, sl = threadIdx.x / G;
  const bool comp = i < ad;
  const double invM = 1.0 / a.Mglobal;
  const float mean_f = (float)a.adv_ms[2 * a.mb];
  const double inv_denom = 1.0 / ((double)(float)a.adv_ms[2 * a.mb + 1] + 1e-8);
  const float eps = a.clip, lo = 1.0f - a.clip, hi = 1.0f + a.clip;
  const double entk = (double)a.ent_coeff * invM;
  double sums[4] = {0.0, 0.0, 0.0, 0.0}, dmu_s = 0.0, ds_s = 0.0, dv_s = 0.0;
  for (int p = 0; p < G; ++p) {
    const int pos = blockIdx.x * 256 + p * SPB + sl;
    if (pos < a.M) {
      const int smp = a.perm[pos];
      const float* rec = a.rec + 16 * (size_t)smp;
      float* z = a.Z + (size_t)a.A8 * pos;
      // policy half: this lane's component, then the group's sums
      float lpt = 0.0f, ent = 0.0f, xi = 0.0f, sg = 1.0f, th = 0.0f;
      if (comp) {
        const float ls = gauss_log_std(a.g, z[ad + i], th);
        sg = expf(ls);
        xi = (rec[i] - z[i]) / sg;
        lpt = gauss_lp_term(xi, ls);
        ent = gauss_ent_term(ls);
      }
#pragma unroll
      for (int o = 1; o < G; o <<= 1) { lpt += __shfl_xor(lpt, o, 64); ent += __shfl_xor(ent, o, 64); }
      const float old_lp = rec[8], ov = rec[9], adv = rec[10], R = rec[11];
      const double Ahat = (double)(adv - mean_f) * inv_denom;
      const float ratio = expf(lpt - old_lp);
      const float rc = fminf(fmaxf(ratio, lo), hi);
      const double pg1 = -Ahat * (double)ratio, pg2 = -Ahat * (double)rc;
      double dnlp, pg;
      if (pg1 > pg2) { pg = pg1; dnlp = pg1; }
      else { pg = pg2; dnlp = (ratio >= lo && ratio <= hi) ? pg1 : 0.0; }
      dnlp *= invM;
      if (comp) {
        const float dmu = (float)(dnlp * (double)(xi / sg));
        const float dsr = (float)((dnlp * ((double)(xi * xi) - 1.0) - entk) * (double)(a.g.ls_half * (1.0f - th * th)));
        z[i] = dmu; z[ad + i] = dsr;
        dmu_s += (double)dmu; ds_s += (double)dsr;
      }
      for (int cpad = 2 * ad + i; cpad < a.A8; cpad += G) z[cpad] = 0.0f;   // K of the head's backward GEMM is padded to A8
      if (i == 0) {
        // value loss (ppo.jl:214,231-240), as wide_loss_kernel
        const float v = a.V[pos];
        const double vk = (double)a.v_coef * 0.5 * invM;
        double dv, term;
        if (a.clip_vloss) {
          const float u = (float)a.vfix[0];
          const double nwin = a.vfix[1];
          const float dvv = v - ov;
          const float cl = fminf(fmaxf(dvv, -eps), eps);
          const float vc = ov + cl;
          const float q = (vc - R) * (vc - R);
          const bool q_wins = !(u > q);  // max.(u, q): ties → q
          term = q_wins ? (double)q : (double)u;
          const double inner = (q_wins && dvv >= -eps && dvv <= eps) ? 2.0 * (double)(vc - R) : 0.0;
          dv = vk * (nwin * invM + inner);
        } else {
          const float e = v - R;
          term = (double)(e * e);
          dv = vk * 2.0 * (double)e;
        }
        const float dvf = (float)dv;
        sums[0] += pg; sums[1] += (double)ent; sums[2] += (double)(v - R * R); sums[3] += term; dv_s += (double)dvf;
        f32x4 d0 = {dvf, 0.0f, 0.0f, 0.0f}, d1 = {0.0f, 0.0f, 0.0f, 0.0f};
        reinterpret_cast<f32x4*>(a.dv8)[2 * (size_t)pos] = d0;
        reinterpret_cast<f32x4*>(a.dv8)[2 * (size_t)pos + 1] = d1;
      }
    }
  }
  // block partials in wide_loss_kernel's slots: 4 loss sums, db3 of the actor (2·act_dim of the 16 slots: μ rows, then s rows), db3 of the critic
  __shared__ double sm[4][24];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int q = 0; q < 4; ++q) { const double s = wave_sum(sums[q]); if (lane == 0) sm[wave][q] = s; }
  { const double s = wave_sum(dv_s); if (lane == 0) sm[wave][4 + 16] = s; }
#pragma unroll
  for (int o = G; o < 64; o <<= 1) { dmu_s += __shfl_xor(dmu_s, o, 64); ds_s += __shfl_xor(ds_s, o, 64); }   // lanes of the same component
  if (lane < G && comp) { sm[wave][4 + lane] = dmu_s; sm[wave][4 + ad + lane] = ds_s; }
  __syncthreads();
  if (threadIdx.x < 4 + 16 + 1) {
    const int q = threadIdx.x;
    const bool live = q < 4 || q == 4 + 16 || (q - 4) < 2 * ad;
    a.lpart[(size_t)blockIdx.x * 24 + q] = live ? (sm[0][q] + sm[1][q]) + (sm[2][q] + sm[3][q]) : 0.0;
  }
}

// ------------------------------------------------------------------------------------------------------
// Probes on precomputed head outputs: one thread per sample, the terms added in index order
// ------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) wide_sample_gauss_kernel(GaussDist g, const float* __restrict__ Z, int A8, const float* __restrict__ V,
                                                               const float* __restrict__ xi, int n, float* __restrict__ action,
                                                               float* __restrict__ logprob, float* __restrict__ value) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= n) return;
  const float* z = Z + (size_t)A8 * b;
  float lp = 0.0f;
  for (int i = 0; i < g.ad; ++i) {
    float th;
    const float ls = gauss_log_std(g, z[g.ad + i], th), x = xi[(size_t)g.ad * b + i];
    action[(size_t)g.ad * b + i] = gauss_action(z[i], expf(ls), x);
    lp += gauss_lp_term(x, ls);
  }
  logprob[b] = lp;
  if (value) value[b] = V[b];
}

__global__ void __launch_bounds__(256) wide_logprob_gauss_kernel(GaussDist g, const float* __restrict__ Z, int A8, const float* __restrict__ actions,
                                                                int n, float* __restrict__ logprob, float* __restrict__ entropy) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= n) return;
  const float* z = Z + (size_t)A8 * b;
  float lp = 0.0f, H = 0.0f;
  for (int i = 0; i < g.ad; ++i) {
    float th;
    const float ls = gauss_log_std(g, z[g.ad + i], th);
    const float x = (actions[(size_t)g.ad * b + i] - z[i]) / expf(ls);
    lp += gauss_lp_term(x, ls);
    H += gauss_ent_term(ls);
  }
  logprob[b] = lp; entropy[b] = H;
}

// ------------------------------------------------------------------------------------------------------
// CRL_ENV_PENDULUM outside the rollout: construction (reset stream 2 at gstep 0, like env_reset_kind_kernel) and one step with the caller's actions
// ------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) pendulum_reset_kernel(DevCfg c, float* __restrict__ env_state, int32_t* __restrict__ env_t, float* __restrict__ cur_obs,
                                                            uint8_t* __restrict__ next_done, float* __restrict__ ep_return, int32_t* __restrict__ ep_length,
                                                            double* ep_stats) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e == 0) { ep_stats[0] = ep_stats[1] = ep_stats[2] = ep_stats[3] = 0.0; }
  if (e >= c.nt) return;
  float s[4], o[ENV_OBS_MAX];
  pendulum_reset(s, c.seed, c.env_id_offset + (uint32_t)e, 0, 2);
  pendulum_observe(s, o);
#pragma unroll
  for (int i = 0; i < PENDULUM_OBS; ++i) { env_state[(size_t)c.D * e + i] = i < PENDULUM_STATE ? s[i] : 0.0f; cur_obs[(size_t)c.D * e + i] = o[i]; }
  env_t[e] = 0; next_done[e] = 0; ep_return[e] = 0.0f; ep_length[e] = 0;
}

__global__ void __launch_bounds__(256) pendulum_step_kernel(DevCfg c, const float* __restrict__ action, uint64_t gstep, float* __restrict__ env_state,
                                                           int32_t* __restrict__ env_t, float* __restrict__ cur_obs, uint8_t* __restrict__ next_done,
                                                           float* __restrict__ reward, uint8_t* __restrict__ done_out) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= c.nt) return;
  float* es = env_state + (size_t)c.D * e;
  float* co = cur_obs + (size_t)c.D * e;
  float s[4] = {es[0], es[1], 0.0f, 0.0f}, so[ENV_OBS_MAX];
  int t_env = env_t[e];
  bool done; float rew;
  env_transition_c(c.env_kind, c.stale_obs, s, t_env, action + e, c.seed, c.env_id_offset + (uint32_t)e, gstep, so, rew, done);   // act_dim = 1
#pragma unroll
  for (int i = 0; i < PENDULUM_OBS; ++i) { co[i] = so[i]; es[i] = i < PENDULUM_STATE ? s[i] : 0.0f; }
  env_t[e] = t_env; next_done[e] = done ? 1 : 0;
  reward[e] = rew; done_out[e] = done ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------------
// Launchers
// ------------------------------------------------------------------------------------------------------
int gauss_env_reset(crl_ppo* h) {
  hipLaunchKernelGGL(pendulum_reset_kernel, dim3((h->dc.nt + 255) / 256), dim3(256), 0, h->stream, h->dc, h->env_state, h->env_t, h->cur_obs,
                     h->next_done, h->ep_return, h->ep_length, h->ep_stats);
  CRL_HIP_CHECK(hipGetLastError());
  return 0;
}
int gauss_env_step(crl_ppo* h, const float* action_d, uint64_t gstep, float* reward_d, uint8_t* done_d) {
  hipLaunchKernelGGL(pendulum_step_kernel, dim3((h->dc.nt + 255) / 256), dim3(256), 0, h->stream, h->dc, action_d, gstep, h->env_state, h->env_t,
                     h->cur_obs, h->next_done, reward_d, done_d);
  CRL_HIP_CHECK(hipGetLastError());
  return 0;
}
void gauss_launch_step(hipStream_t st, const WStepArgs& a, const HeadGauss& hd) {
  hipLaunchKernelGGL(wide_step_gauss_kernel, dim3((a.c.nt + 255) / 256), dim3(256), 0, st, a, hd);
}
void gauss_launch_sample(hipStream_t st, const GaussDist& g, const float* Z, int A8, const float* V, const float* xi, int n, float* action, float* logprob,
                         float* value) {
  hipLaunchKernelGGL(wide_sample_gauss_kernel, dim3((n + 255) / 256), dim3(256), 0, st, g, Z, A8, V, xi, n, action, logprob, value);
}
void gauss_launch_logprob(hipStream_t st, const GaussDist& g, const float* Z, int A8, const float* actions, int n, float* logprob, float* entropy) {
  hipLaunchKernelGGL(wide_logprob_gauss_kernel, dim3((n + 255) / 256), dim3(256), 0, st, g, Z, A8, actions, n, logprob, entropy);
}
void gauss_launch_pack_rec(hipStream_t st, int B, int ad, const float* action_f, const float* logprob, const float* value, const float* adv, const float* ret,
                           float* rec) {
  int nb = (B + 255) / 256; if (nb > 4096) nb = 4096;
  hipLaunchKernelGGL(wide_pack_rec_gauss_kernel, dim3(nb), dim3(256), 0, st, B, ad, action_f, logprob, value, adv, ret, rec);
}
void gauss_launch_loss(hipStream_t st, const GaussLossArgs& a, int nlb) {
  const int ad = a.g.ad;
  if (ad == 1) hipLaunchKernelGGL(wide_loss_gauss_kernel<1>, dim3(nlb), dim3(256), 0, st, a);
  else if (ad == 2) hipLaunchKernelGGL(wide_loss_gauss_kernel<2>, dim3(nlb), dim3(256), 0, st, a);
  else if (ad <= 4) hipLaunchKernelGGL(wide_loss_gauss_kernel<4>, dim3(nlb), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(wide_loss_gauss_kernel<8>, dim3(nlb), dim3(256), 0, st, a);
}

}  // namespace crl
