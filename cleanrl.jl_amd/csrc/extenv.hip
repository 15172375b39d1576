// extenv.hip — device-resident external envs: the two per-step launches of crl_rollout_act_device / crl_rollout_record_device. The caller's simulator
// lives on the same GPU and hands over device pointers; nothing is staged and the host never waits inside the rollout loop.
//
// ext_act_kernel<H>: ppo.jl:127-128 plus the state / action / logprob / terminal / value fields of Buffer.add! (:133-140) for ONE step of all envs: the
// register-stationary bf16x3 forward block and the role-pair frame of fwd_rs_x3.hpp (even blocks hold the actor, odd blocks the critic, both persistent over
// 32-env tiles). One kernel family for the 4 / 2 / 64 shape and every layer-wise shape; no option and no route of the handle is read.
//   per tile  the 32 x obs_dim observations (contiguous in obs_d) to LDS — the ACTOR block also copies them to slot `step` of the buffer, it has them in
//             flight anyway | barrier | layer 1 | barrier | layer 2 | barrier | the wave's head partials | barrier | lanes 0-31 of wave 0, one env each:
//             actor  softmax_rt (policy_rt.hpp), u = u53(philox_env(seed, env_id_offset + e, iteration * num_steps + step, 0)) — the draw every on-device
//                    rollout kernel takes for that env and step —, sample_rt, the logprob of the drawn action; action to the buffer and to action_d, logprob
//             critic the value; terminal <- done_d
//   stores    plain vector stores to the (·, num_envs, num_steps) layout, env fastest; a partial last tile reads and writes nothing past num_envs.
//
// ext_record_kernel: ppo.jl:132,137,143-165 for one step, one thread per env: reward to the slot, CRL_F_CUR_OBS / CRL_F_NEXT_DONE <- next_obs_d / next_done_d
// (what the fixed-mode bootstrap reads), ep_length += 1, ep_return += reward (Float32, step order); where next_done: the four ep_stats doubles (wave sums, one
// atomic set per wave like the rollout kernels), a record {return, length, env_id_offset + e, step} to the episode ring through the same atomic counter, and
// zeroed accumulators. return_max keeps the order-preserving key of the signed env kinds (stat_max_key; api.cpp maps it back).
#include "fwd_rs_x3.hpp"
#include "stats.hpp"

namespace crl {

struct ExtActArgs {
  const float* params; int64_t Pa;   // actor | critic, each W1(H,D) b1(H) W2(H,H) b2(H) W3(n_out,H) b3(n_out), (out,in) column-major
  const float* obs_in; const uint8_t* done_in; int32_t* action_out;   // the caller's: (D, N), [N], [N]
  float* obs; int32_t* action; float* logprob; float* value; uint8_t* terminal;   // slot `step` of the resident buffer: (D, N), [N] each
  int D, A, N;
  int w1_lds;                        // 1 = W1 fits LDS next to everything else, 0 = layer 1 reads it from the parameters (hidden 256 with a wide observation)
  uint64_t seed, gstep; uint32_t gid0;
};

template <int H>
__global__ void __launch_bounds__(2 * H) ext_act_kernel(ExtActArgs a) {
  constexpr int NT = RsGeom<H>::NT, KR = RsGeom<H>::KR;
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int D = a.D, XS = rs_xs(D), N = a.N;
  const int role = blockIdx.x & 1, rb = blockIdx.x >> 1, nrb = gridDim.x >> 1;   // 0 = actor, 1 = critic
  const int A = role ? 1 : a.A;
  const RsRoleLds l = rs_role_lds<H>(sm, 0, D, a.A);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const RsNet net = rs_net<H>(a.params + (role ? a.Pa : 0), D, A);

  if (a.w1_lds) for (int idx = tid; idx < H * D; idx += NT) l.w1l[idx] = net.W1[idx];
  rs_stage_head<H>(net, A, l.b1l, l.b2c, l.w3c, l.b3l, tid);
  P3 wr[KR];
  rs_stage_w2<H>(net.W2, wr, l.wl, w, lane);
  __syncthreads();

  for (int tile = rb; tile * 32 < N; tile += nrb) {
    const int e0 = tile * 32, ne = N - e0 < 32 ? N - e0 : 32;
    const bool mine = w == 0 && lane < ne;
    for (int idx = tid; idx < 32 * D; idx += NT) {               // obs (D, N): the tile's 32 D floats are contiguous; nothing at or past env N is touched
      const int m = idx / D, k = idx - m * D;
      float x = 0.0f;
      if (m < ne) {
        x = a.obs_in[(size_t)e0 * D + idx];
        if (role == 0) a.obs[(size_t)e0 * D + idx] = x;          // Buffer.add!'s state field: written once, by the actor's block
      }
      l.xt[m * XS + k] = x;
    }
    __syncthreads();
    rs_layer1_stream<H>(l, net.W1, a.w1_lds, D, tid);
    __syncthreads();
    const f32x16 acc = rs_layer2<H>(wr, l.wl, l.h1p, l.b2c, w, lane);
    __syncthreads();                                             // every wave has read its h1 fragments: the region now takes the head partials
    rs_head_partials<H>(acc, l.w3c, A, l.zp, w, lane);
    __syncthreads();
    if (mine) {                                                  // one lane per env; the next tile's first barrier stands between these reads of zp and layer 1's writes of h1
      const int e = e0 + lane;
      float z[AMAX];
      rs_logits<H>(l.zp, l.b3l, A, lane, z);
      if (role == 0) {                                           // ppo.jl:21-32 get_action
        float p[AMAX], lp[AMAX];
#pragma unroll
        for (int aa = 0; aa < AMAX; ++aa) { p[aa] = 0.0f; lp[aa] = 0.0f; }
        softmax_rt(z, A, p, lp);
        const double u = u53(philox_env(a.seed, a.gid0 + (uint32_t)e, a.gstep, 0));
        const int act = sample_rt(p, A, u);
        float lpa = lp[0];
#pragma unroll
        for (int aa = 1; aa < AMAX; ++aa) lpa = (act == aa) ? lp[aa] : lpa;
        a.action[e] = act; a.action_out[e] = act; a.logprob[e] = lpa;
      } else {
        a.value[e] = z[0];
        a.terminal[e] = a.done_in[e];
      }
    }
  }
}

struct ExtRecArgs {
  const float* reward_in; const float* next_obs_in; const uint8_t* next_done_in;
  float* reward;                                   // slot `step`
  float* cur_obs; uint8_t* next_done; float* ep_return; int32_t* ep_length; double* ep_stats;
  crl_episode_record* ring; uint32_t* ring_count; int ring_cap;
  int D, N, step; uint32_t gid0;
};

__global__ void __launch_bounds__(256) ext_record_kernel(ExtRecArgs a) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  const bool live = e < a.N;
  double st_n = 0.0, st_ret = 0.0, st_len = 0.0, st_max = 0.0;
  if (live) {
    const float rew = a.reward_in[e];
    a.reward[e] = rew;                                            // ppo.jl:132,137
    for (int k = 0; k < a.D; ++k) a.cur_obs[(size_t)e * a.D + k] = a.next_obs_in[(size_t)e * a.D + k];   // ppo.jl:143
    const uint8_t nd = a.next_done_in[e];
    a.next_done[e] = nd;                                          // ppo.jl:144
    int ep_len = a.ep_length[e] + 1;                              // ppo.jl:125
    float ep_ret = a.ep_return[e] + rew;                          // ppo.jl:145
    if (nd) {                                                     // ppo.jl:147-165
      st_n = 1.0; st_ret = (double)ep_ret; st_len = (double)ep_len; st_max = (double)ep_ret;
      episode_ring_push(a.ring, a.ring_count, a.ring_cap, ep_ret, ep_len, a.gid0 + (uint32_t)e, a.step);
      ep_ret = 0.0f; ep_len = 0;
    }
    a.ep_return[e] = ep_ret; a.ep_length[e] = ep_len;
  }
  episode_stats_flush(a.ep_stats, st_n, st_ret, st_len, st_max, true);   // lanes past num_envs bring the neutral elements
}

// The launch of crl_rollout_act_device on the handle's stream.
int launch_ext_act(crl_ppo* h, int step, const float* obs_d, const uint8_t* done_d, int32_t* action_d) {
  const int H = h->cfg.hidden, D = h->dc.D, A = h->dc.A, N = h->dc.nt;
  bool w1_lds; size_t lds;
  if (rs_role_shape(h, 0, "crl_rollout_act_device: no kernel for this shape (obs_dim <= 64, n_act <= 16, hidden 64 / 128 / 256)",
                    "crl_rollout_act_device: this shape needs more LDS than a CU has", &w1_lds, &lds)) return 1;
  // the shape is fixed for the life of the handle: asked once, not per step
  if (h->ext_per_cu == 0 && rs_dispatch_h(H, [&](auto hc) { return rs_role_per_cu(ext_act_kernel<decltype(hc)::value>, H, lds, &h->ext_per_cu); })) return 1;
  const int nrb = rs_role_pairs(h, h->ext_per_cu, N);
  const size_t off = (size_t)N * (size_t)step;
  ExtActArgs a;
  a.params = h->params; a.Pa = h->Pa;
  a.obs_in = obs_d; a.done_in = done_d; a.action_out = action_d;
  a.obs = h->obs + off * (size_t)D; a.action = h->action + off; a.logprob = h->logprob + off; a.value = h->value + off; a.terminal = h->terminal + off;
  a.D = D; a.A = A; a.N = N; a.w1_lds = w1_lds ? 1 : 0;
  a.seed = h->dc.seed; a.gstep = (uint64_t)h->iteration * (uint64_t)h->dc.k + (uint64_t)step; a.gid0 = h->dc.env_id_offset;
  const dim3 grid(2 * nrb), block(2 * H);
  rs_dispatch_h(H, [&](auto hc) { hipLaunchKernelGGL(ext_act_kernel<decltype(hc)::value>, grid, block, lds, h->stream, a); return 0; });
  CRL_HIP_CHECK(hipGetLastError());
  return 0;
}

int launch_ext_record(crl_ppo* h, int step, const float* reward_d, const float* next_obs_d, const uint8_t* next_done_d) {
  ExtRecArgs a;
  a.reward_in = reward_d; a.next_obs_in = next_obs_d; a.next_done_in = next_done_d;
  a.reward = h->reward + (size_t)h->dc.nt * (size_t)step;
  a.cur_obs = h->cur_obs; a.next_done = h->next_done; a.ep_return = h->ep_return; a.ep_length = h->ep_length; a.ep_stats = h->ep_stats;
  a.ring = h->ep_ring; a.ring_count = h->ep_ring_count; a.ring_cap = h->ep_ring_cap;
  a.D = h->dc.D; a.N = h->dc.nt; a.step = step; a.gid0 = h->dc.env_id_offset;
  hipLaunchKernelGGL(ext_record_kernel, dim3((h->dc.nt + 255) / 256), dim3(256), 0, h->stream, a);
  CRL_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace crl
