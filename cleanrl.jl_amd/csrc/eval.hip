// eval.hip — crl_ppo_evaluate: the handle's actor, frozen, on a private set of on-device envs until every env has finished its quota of
// episodes; one launch, nothing but the per-episode (return, length) pairs and the optional action trace leaves the CU. No reference
// counterpart (ppo.jl never evaluates): the trajectory is DEFINED by the public calls — crl_env_reset, then crl_env_step(actions, gstep = g)
// on a twin handle with num_envs = n, seed = S, env_id_offset = 0, stale_obs = 0, the action of env e at step g chosen from the actor's
// logits at the twin's CRL_F_CUR_OBS: greedy = lowest index of the largest logit, sampled = get_action's sampler (ppo.jl:21-32) on
// u53(philox_env(S, e, g, 0)), the draw of step g of iteration 0 of a training rollout.
//
// eval_rollout_kernel<H, DP>: a block of H / 32 waves owns a tile of 32 envs for their whole evaluation.
//   weights   W2 as bf16x3 A-fragments is REGISTER-STATIONARY for every width: wave w keeps rows 32w … 32w + 31 over all H columns, 12
//             registers per 16-wide k-step (48 / 96 registers at H = 64 / 128). At 256 the 384 KB of pieces fit neither LDS nor, at 192
//             registers a lane, the file next to everything else: 13 of the 16 k-steps live in registers (156), the last three in LDS
//             (72 KB, written once, read as three 16-byte fragments per k-step like the activations). W1 (padded to DP columns), the
//             biases and the head rows sit in LDS, read straight from the flat Flux-ordered actor parameters once per launch — no pack,
//             no option, no route of the handle is involved.
//   per step  layer 1 on the vector pipe (a thread forms two octets of hidden rows of one env: tanh_fast, bf16x3 split, three 16-byte
//             LDS stores in B-fragment order) | barrier | layer 2 on the matrix pipe (6 v_mfma_f32_32x32x16_bf16 per k-step, f32
//             accumulation), tanh_fast, the wave's head partials to LDS | barrier | lanes 0-31 of wave 0 add the partials in wave order,
//             pick the action, run env_transition and the episode bookkeeping (env state, t, running return, length, episode index: eight
//             LDS words per env, in registers for the step) and write the next observation to LDS | barrier.
//   exit      wave 0 publishes "any env of the tile still has episodes to finish" through LDS in front of the third barrier; every thread
//             reads it behind the barrier, so the exit is block-uniform, and the loop is bounded by episodes_per_env x the env's longest
//             episode whatever the flag says.
#include "common.hpp"
#include "env.hpp"
#include "mlp_x3.hpp"
#include "policy_rt.hpp"
#include "ppo_ctx.hpp"

namespace crl {

struct EvalArgs {
  const float* actor;        // W1(H,D) b1(H) W2(H,H) b2(H) W3(A,H) b3(A), (out,in) column-major
  int D, A, n, episodes, mode, kind, max_steps, trace_steps;
  uint64_t seed;
  float* returns; int32_t* lengths; int32_t* trace;   // (episodes, n) / (episodes, n) / (trace_steps, n), env fastest; trace may be null
};

// LDS (floats): h1 pieces | W2 fragments of the k-steps that are not in registers | env state | observations | W1 rows | b1 | b2 (C-fragment order) | b3 | flag | head partials | W3 (C-fragment order)
// (the partials are laid out for AMAX actions whatever n_act is: every address of the step loop is then the block's base plus a constant)
__host__ __device__ constexpr int eval_ks_lds(int H) { return H == 256 ? 3 : 0; }   // k-steps of W2 whose A fragments sit in LDS, not in registers
__host__ __device__ constexpr int eval_lds_fixed(int H, int DP) {
  return 3 * H * 16 + eval_ks_lds(H) * 3 * (H / 32) * 64 * 4 + 32 * 8 + 32 * DP + H * DP + H + H + AMAX + 4 + (H / 32) * AMAX * 32;
}
static inline size_t eval_lds_bytes(int H, int DP, int A) { return sizeof(float) * (size_t)(eval_lds_fixed(H, DP) + A * H); }

template <int H, int DP>
__global__ void __launch_bounds__(2 * H) eval_rollout_kernel(EvalArgs a) {
  constexpr int NW = H / 32, KS = H / 16, NT = 2 * H, KL = eval_ks_lds(H), KR = KS - KL;
  extern __shared__ __attribute__((aligned(16))) float sm[];
  bf16x8* h1p = reinterpret_cast<bf16x8*>(sm);                  // [piece][ks][lane]: B fragments of h1, k = 16 ks + 8 (lane >> 5) + j
  bf16x8* wl = h1p + 3 * KS * 64;                               // [KL][piece][wave][lane]: A fragments of the last KL k-steps of W2
  float* es = sm + 3 * H * 16 + KL * 3 * NW * 64 * 4;           // [32 envs][8]: state[4], t, running return, length, episode index
  float* xt = es + 32 * 8;                                      // [32 envs][DP]
  float* w1l = xt + 32 * DP;                                    // [H][DP]
  float* b1l = w1l + H * DP;
  float* b2c = b1l + H;                                         // [wave][hf][16]: b2[32 wave + rowmap(r, hf)]
  float* b3l = b2c + H;
  int* flag = reinterpret_cast<int*>(b3l + AMAX);
  float* zp = b3l + AMAX + 4;                                   // [wave][AMAX][32 envs]
  float* w3c = zp + NW * AMAX * 32;                             // [A][wave][hf][16]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, hf = lane >> 5, i = lane & 31;
  const int D = a.D, A = a.A, n = a.n;
  const float* W1 = a.actor; const float* b1 = W1 + H * D; const float* W2 = b1 + H; const float* b2 = W2 + H * H;
  const float* W3 = b2 + H; const float* b3 = W3 + A * H;

  for (int idx = tid; idx < H * DP; idx += NT) { const int r = idx / DP, k = idx % DP; w1l[idx] = k < D ? W1[r + H * k] : 0.0f; }
  for (int idx = tid; idx < H; idx += NT) {
    b1l[idx] = b1[idx];
    b2c[idx] = b2[32 * (idx >> 5) + rowmap(idx & 15, (idx >> 4) & 1)];
  }
  for (int idx = tid; idx < A * H; idx += NT) {
    const int aa = idx / H, q = idx % H;
    w3c[idx] = W3[aa + A * (32 * (q >> 5) + rowmap(q & 15, (q >> 4) & 1))];
  }
  if (tid < AMAX) b3l[tid] = tid < A ? b3[tid] : 0.0f;
  if (tid == 0) flag[0] = 1;                                     // the grid has no empty tile
  P3 wr[KR];                                                     // this wave's 32 rows of W2: A fragments, row = 32 w + i
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = W2[(32 * w + i) + H * (16 * ks + 8 * hf + j)];
    if (ks < KR) wr[ks] = split3(v);
    else { const P3 p = split3(v); bf16x8* q = wl + ((ks - KR) * 3 * NW + w) * 64 + lane; q[0] = p.hi; q[NW * 64] = p.mid; q[2 * NW * 64] = p.lo; }
    if (ks & 1) __builtin_amdgcn_sched_barrier(0);               // raw rows of two k-steps in flight: the split pieces fill the file
  }

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
          hv[j] = tanh_fast(acc + b1l[r]);
          if (j & 1) __builtin_amdgcn_sched_barrier(0);          // two rows of W1 in flight, not sixteen: the registers belong to W2
        }
        const P3 p = split3(hv);
        const int slot = (oct >> 1) * 64 + (oct & 1) * 32 + m;
        h1p[slot] = p.hi; h1p[KS * 64 + slot] = p.mid; h1p[2 * KS * 64 + slot] = p.lo;
      }
    }
    __syncthreads();
    {                                                            // layer 2 + the wave's head partials
      f32x16 acc = load16(b2c + (2 * w + hf) * 16);
      const bf16x8* hb = h1p + lane;
      asm volatile("" : "+v"(hb));                               // one base per step, constant offsets behind it (see zl below)
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        P3 b;
        b.hi = hb[ks * 64]; b.mid = hb[(KS + ks) * 64]; b.lo = hb[(2 * KS + ks) * 64];
        if (ks < KR) acc = mfma_x3(wr[ks], b, acc);
        else {
          const bf16x8* q = wl + ((ks - KR) * 3 * NW + w) * 64 + lane;
          P3 aw; aw.hi = q[0]; aw.mid = q[NW * 64]; aw.lo = q[2 * NW * 64];
          acc = mfma_x3(aw, b, acc);
        }
        if (ks & 1) __builtin_amdgcn_sched_barrier(0);           // at most two k-steps of B fragments in flight
      }
      float h2[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) h2[r] = tanh_fast(acc[r]);
      for (int aa = 0; aa < A; ++aa) {
        const f32x4* wv = reinterpret_cast<const f32x4*>(w3c + aa * H + (2 * w + hf) * 16);
        float p = 0.0f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const f32x4 v = wv[q];
#pragma unroll
          for (int c = 0; c < 4; ++c) p = __builtin_fmaf(v[c], h2[4 * q + c], p);
        }
        p = add32(p);
        if (hf == 0) zp[(w * AMAX + aa) * 32 + i] = p;
      }
    }
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
        const float* zl = zp + lane;
        asm volatile("" : "+v"(zl));                             // formed per step: 128 hoisted addresses would cost W2 its registers
#pragma unroll
        for (int aa = 0; aa < AMAX; ++aa) {
          float v = 0.0f;
          if (aa < A) {
            v = b3l[aa];
            for (int ww = 0; ww < NW; ++ww) v += zl[(ww * AMAX + aa) * 32];
          }
          z[aa] = v;
        }
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
  if (H == 64) return eval_launch_h<64>(h, a, DP);
  if (H == 128) return eval_launch_h<128>(h, a, DP);
  return eval_launch_h<256>(h, a, DP);
}

}  // namespace crl
