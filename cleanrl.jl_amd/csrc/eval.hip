// eval.hip — crl_ppo_evaluate: the handle's actor, frozen, on a private set of on-device envs until every env has finished its quota of
// episodes; one launch, nothing but the per-episode (return, length) pairs and the optional action trace leaves the CU. No reference
// counterpart (ppo.jl never evaluates): the trajectory is DEFINED by the public calls — crl_env_reset, then crl_env_step(actions, gstep = g)
// on a twin handle with num_envs = n, seed = S, env_id_offset = 0, stale_obs = 0, the action of env e at step g chosen from the actor's
// logits at the twin's CRL_F_CUR_OBS: greedy = lowest index of the largest logit, sampled = get_action's sampler (ppo.jl:21-32) on
// u53(philox_env(S, e, g, 0)), the draw of step g of iteration 0 of a training rollout.
//
// eval_rollout_kernel<H, DP>: a block of H / 32 waves owns a tile of 32 envs for their whole evaluation. The forward is the register-stationary bf16x3 block
// of fwd_rs_x3.hpp (W2 staging, layer-1 epilogue, layer 2, head partials, logits); what is this kernel's own:
//   weights   W1 (row-major, padded to DP columns) sits in LDS next to the block's biases and head rows.
//   per step  layer 1's dot product with the env's observation in registers | barrier | layer 2 and the wave's head partials (their own LDS region: no
//             barrier between the two) | barrier | lanes 0-31 of wave 0 pick the action, run env_transition and the episode bookkeeping (env state, t,
//             running return, length, episode index: eight LDS words per env, in registers for the step) and write the next observation to LDS | barrier.
//   exit      wave 0 publishes "any env of the tile still has episodes to finish" through LDS in front of the third barrier; every thread
//             reads it behind the barrier, so the exit is block-uniform, and the loop is bounded by episodes_per_env x the env's longest
//             episode whatever the flag says.
#include "common.hpp"
#include "env.hpp"
#include "fwd_rs_x3.hpp"

namespace crl {

struct EvalArgs {
  const float* actor;        // W1(H,D) b1(H) W2(H,H) b2(H) W3(A,H) b3(A), (out,in) column-major
  int D, A, n, episodes, mode, kind, max_steps, trace_steps;
  uint64_t seed;
  float* returns; int32_t* lengths; int32_t* trace;   // (episodes, n) / (episodes, n) / (trace_steps, n), env fastest; trace may be null
};

// LDS (floats): the block's prefix (h1 pieces | W2 fragments of the k-steps that are not in registers) | env state | observations | W1 rows | b1 | b2 (C-fragment order) | b3 | flag | head partials | W3 (C-fragment order)
__host__ __device__ constexpr int eval_lds_fixed(int H, int DP) {
  return rs_lds_prefix(H) + 32 * 8 + 32 * DP + H * DP + H + H + AMAX + 4 + (H / 32) * AMAX * 32;
}
static inline size_t eval_lds_bytes(int H, int DP, int A) { return sizeof(float) * (size_t)(eval_lds_fixed(H, DP) + A * H); }

template <int H, int DP>
__global__ void __launch_bounds__(2 * H) eval_rollout_kernel(EvalArgs a) {
  constexpr int NW = RsGeom<H>::NW, KS = RsGeom<H>::KS, NT = RsGeom<H>::NT, KR = RsGeom<H>::KR;
  extern __shared__ __attribute__((aligned(16))) float sm[];
  bf16x8* h1p = reinterpret_cast<bf16x8*>(sm);
  bf16x8* wl = h1p + 3 * KS * 64;
  float* es = sm + rs_lds_prefix(H);                            // [32 envs][8]: state[4], t, running return, length, episode index
  float* xt = es + 32 * 8;                                      // [32 envs][DP]
  float* w1l = xt + 32 * DP;                                    // [H][DP]
  float* b1l = w1l + H * DP;
  float* b2c = b1l + H;
  float* b3l = b2c + H;
  int* flag = reinterpret_cast<int*>(b3l + AMAX);
  float* zp = b3l + AMAX + 4;                                   // [wave][AMAX][32 envs]
  float* w3c = zp + NW * AMAX * 32;                             // [A][wave][hf][16]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int D = a.D, A = a.A, n = a.n;
  const RsNet net = rs_net<H>(a.actor, D, A);

  for (int idx = tid; idx < H * DP; idx += NT) { const int r = idx / DP, k = idx % DP; w1l[idx] = k < D ? net.W1[r + H * k] : 0.0f; }
  rs_stage_head<H>(net, A, b1l, b2c, w3c, b3l, tid);
  if (tid == 0) flag[0] = 1;                                     // the grid has no empty tile
  P3 wr[KR];
  rs_stage_w2<H>(net.W2, wr, wl, w, lane);

  // env state of lane's env (lanes 0-31 of wave 0): crl_env_reset's draw — stream 2 at gstep 0 of global id e
  const int e = blockIdx.x * 32 + lane;
  if (w == 0 && lane < 32) {
    float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    float o[ENV_OBS_MAX];
#pragma unroll
    for (int k = 0; k < ENV_OBS_MAX; ++k) o[k] = 0.0f;
    if (e < n) { env_reset(a.kind, s, a.seed, (uint32_t)e, 0, 2); env_observe(a.kind, s, o); }
    float* st = es + lane * 8;
    st[0] = s[0]; st[1] = s[1]; st[2] = s[2]; st[3] = s[3];
    reinterpret_cast<int*>(st)[4] = 0; st[5] = 0.0f; reinterpret_cast<int*>(st)[6] = 0;
    reinterpret_cast<int*>(st)[7] = e < n ? 0 : a.episodes;      // a lane beyond num_envs has nothing to finish
#pragma unroll
    for (int k = 0; k < DP; ++k) xt[lane * DP + k] = k < D ? o[k] : 0.0f;
  }
  __syncthreads();

  for (int g = 0; g < a.max_steps; ++g) {
    if (flag[0] == 0) break;                                     // block-uniform: written in front of the last barrier
    {                                                            // layer 1: env m, hidden rows 8 oct … 8 oct + 7
      const int m = tid & 31, g8 = tid >> 5;
      float x[DP];
#pragma unroll
      for (int q = 0; q < DP / 4; ++q) {
        const f32x4 v = reinterpret_cast<const f32x4*>(xt + m * DP)[q];
        x[4 * q] = v[0]; x[4 * q + 1] = v[1]; x[4 * q + 2] = v[2]; x[4 * q + 3] = v[3];
      }
#pragma unroll 1
      for (int half = 0; half < 2; ++half) {
        const int oct = g8 + half * (H / 16);
        float hv[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int r = 8 * oct + j;
          float acc = 0.0f;
#pragma unroll
          for (int q = 0; q < DP / 4; ++q) {
            const f32x4 wv = reinterpret_cast<const f32x4*>(w1l + r * DP)[q];
            acc = __builtin_fmaf(wv[0], x[4 * q], acc); acc = __builtin_fmaf(wv[1], x[4 * q + 1], acc);
            acc = __builtin_fmaf(wv[2], x[4 * q + 2], acc); acc = __builtin_fmaf(wv[3], x[4 * q + 3], acc);
          }
          hv[j] = acc;
          if (j & 1) __builtin_amdgcn_sched_barrier(0);          // two rows of W1 in flight, not sixteen: the registers belong to W2
        }
        rs_l1_epilogue<H>(hv, b1l, oct, m, h1p);
      }
    }
    __syncthreads();
    rs_head_partials<H>(rs_layer2<H>(wr, wl, h1p, b2c, w, lane), w3c, A, zp, w, lane);
    __syncthreads();
    if (w == 0) {                                                // action, env, episode bookkeeping: one lane per env
      float* st = es + (lane & 31) * 8;
      int ep_idx = reinterpret_cast<int*>(st)[7];
      bool active = lane < 32 && ep_idx < a.episodes;
      if (active) {
        float s[4] = {st[0], st[1], st[2], st[3]};
        int t = reinterpret_cast<int*>(st)[4], ep_len = reinterpret_cast<int*>(st)[6];
        float ep_ret = st[5];
        float z[AMAX];
        rs_logits<H>(zp, b3l, A, lane, z);
        int act = 0;
        if (a.mode == CRL_EVAL_GREEDY) {
          float best = z[0];
#pragma unroll
          for (int aa = 1; aa < AMAX; ++aa) { const bool up = aa < A && z[aa] > best; act = up ? aa : act; best = up ? z[aa] : best; }
        } else {
          float p[AMAX], lp[AMAX];
          softmax_rt(z, A, p, lp);
          act = sample_rt(p, A, u53(philox_env(a.seed, (uint32_t)e, (uint64_t)g, 0)));
        }
        if (g < a.trace_steps) a.trace[(size_t)g * n + e] = act;
        float o[ENV_OBS_MAX], rew; bool done;
        env_transition(a.kind, /*stale_obs=*/0, s, t, act, a.seed, (uint32_t)e, (uint64_t)g, o, rew, done);
        ep_ret += rew; ep_len += 1;
        if (done) {
          a.returns[(size_t)ep_idx * n + e] = ep_ret; a.lengths[(size_t)ep_idx * n + e] = ep_len;
          ep_idx += 1; ep_ret = 0.0f; ep_len = 0;
          active = ep_idx < a.episodes;
        }
        st[0] = s[0]; st[1] = s[1]; st[2] = s[2]; st[3] = s[3];
        reinterpret_cast<int*>(st)[4] = t; st[5] = ep_ret; reinterpret_cast<int*>(st)[6] = ep_len; reinterpret_cast<int*>(st)[7] = ep_idx;
#pragma unroll
        for (int k = 0; k < DP; ++k) xt[lane * DP + k] = k < D ? o[k] : 0.0f;
      }
      const unsigned long long live = __ballot(active);
      if (lane == 0) flag[0] = live != 0ull;
    }
    __syncthreads();
  }
}

template <int H>
static int eval_launch_h(crl_ppo* h, const EvalArgs& a, int DP) {
  const dim3 grid((a.n + 31) / 32), block(2 * H);
  const size_t lds = eval_lds_bytes(H, DP, a.A);
  if (lds > 160 * 1024) { set_error("crl_ppo_evaluate: n_act = " + std::to_string(a.A) + " at hidden " + std::to_string(H) + " needs more LDS than a CU has"); return 1; }
  if (DP == 4) hipLaunchKernelGGL((eval_rollout_kernel<H, 4>), grid, block, lds, h->stream, a);
  else hipLaunchKernelGGL((eval_rollout_kernel<H, 8>), grid, block, lds, h->stream, a);
  CRL_HIP_CHECK(hipGetLastError());
  return 0;
}

// the longest episode an env can produce: CartPole ends at t > 500 (the 501st step), the other two at t >= 200
int eval_episode_cap(int kind) { return kind == CRL_ENV_CARTPOLE ? 501 : ENV_MAX_STEPS_CC; }

int launch_eval(crl_ppo* h, const crl_eval_config* c, float* returns_d, int32_t* lengths_d, int32_t* trace_d) {
  const int H = h->cfg.hidden, D = h->dc.D, A = h->dc.A;
  if (!env_stateful(h->cfg.env_kind) || D > ENV_OBS_MAX || A > AMAX || (H != 64 && H != 128 && H != 256)) {
    set_error("crl_ppo_evaluate: no evaluation kernel for this shape (stateful env, obs_dim <= 8, n_act <= 16, hidden 64 / 128 / 256)");
    return 1;
  }
  EvalArgs a;
  a.actor = h->params; a.D = D; a.A = A; a.n = c->num_envs; a.episodes = c->episodes_per_env; a.mode = c->mode; a.kind = h->cfg.env_kind;
  a.max_steps = c->episodes_per_env * eval_episode_cap(h->cfg.env_kind); a.trace_steps = trace_d ? c->trace_steps : 0; a.seed = c->seed;
  a.returns = returns_d; a.lengths = lengths_d; a.trace = trace_d;
  const int DP = D <= 4 ? 4 : 8;
  return rs_dispatch_h(H, [&](auto hc) { return eval_launch_h<decltype(hc)::value>(h, a, DP); });
}

}  // namespace crl
