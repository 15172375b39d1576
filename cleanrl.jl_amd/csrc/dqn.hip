// dqn.hip — src/algorithms/dqn.jl on the GPU (C ABI: the crl_dqn_* block of include/cleanrl_hip.h).
//
// The reference interleaves ONE CartPoleEnv{Float64} step with a 120-sample update every train_freq steps. The
// `for global_step` body (dqn.jl:57-119) runs here as a fixed sequence of launches per train_freq steps, enqueued without
// any host read-back in between: dqn_collect_kernel (ε-greedy action — q_net forward only on greedy steps —, env step,
// ring-buffer add, episode bookkeeping, up to the next training step), then the minibatch draw without replacement, both
// forwards, TD target, Flux.mse, the pullbacks, Adam (the entry step PPO's optimiser kernels share: optim.hpp) and the hard target copy as multi-CU kernels.
// Float64 arithmetic with Float32 weights like the reference (see a2c.hip; both step the CartPoleEnv{Float64} of env64.hpp); relu has no transcendental, every sum runs
// in the oracle's order with contraction off ⇒ the run is BIT-IDENTICAL to oracle/dqn_oracle.c.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <new>
#include <string>

#include "common.hpp"
#include "env64.hpp"
#include "optim.hpp"
#include "ppo_ctx.hpp"
#include "dqn_per.hpp"
#include "dqn_target.hpp"
#include "dqn_c51.hpp"
#include "dqn_duel.hpp"
#include "dqn_loops.hpp"   // the net's shape, DQNCtl, DQNDev, and the loops the heads share
#include "replay_sample.hpp"
#include "value_eval.hpp"

struct crl_dqn;

namespace crl {

// ------------------------------------------------------------------------------------------------------
// One cycle = [collect: env steps up to and including the next training step] → [update phases]. The schedule is
// deterministic (dqn.jl:93), every decision is taken on the device (kernels early-exit on the control block), so the
// host simply enqueues ⌈steps / train_freq⌉ + 1 identical cycles without ever reading anything back in between.
// The update phases are ordinary multi-CU launches: an update is ≈5 M Float64 multiply-adds, ≈0.5 ms on ONE CU but a
// few µs per phase on the whole chip. Per-element arithmetic and summation order are exactly the oracle's.
// ------------------------------------------------------------------------------------------------------
__global__ void dqn_begin_kernel(DQNDev a, int64_t max_env_steps) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  a.ctl->n_eps = 0; a.ctl->n_losses = 0; a.ctl->taken = 0; a.ctl->budget = max_env_steps;
}

// dqn.jl:57-93: env steps until a training step is due (train_pending = 1), the budget or total_timesteps is used up. This kernel keeps ITS OWN text of
// the loop that dqn_collect_loop (dqn_loops.hpp) states for the categorical and the dueling head, and its own static arrays: around the shared loop,
// with the scratch gathered into one DQNCollectLds, it measured 44.2 us per launch against 43.1 us (the plain cycle 172.3 us against the parent's
// 170.0-170.4: DESIGN.md §3k). A change to the ring, the episode record or the train_pending rule is made here AND in dqn_collect_loop. The greedy
// forward is the shared dqn_block_trunk + dqn_head_row: with them the kernel's instructions are the parent's but for where one loop base is folded.
__global__ void __launch_bounds__(128) dqn_collect_kernel(DQNDev a) {
#pragma clang fp contract(off)
  __shared__ DQNCtl c;
  __shared__ double obs[QD], h1s[QH1], h2s[QH2], qs[QA];
  __shared__ int go, need_q, action_s;
  __shared__ double eps_s;
  __shared__ float wq[QP];   // q_net for the greedy steps of this launch (its dot products read one weight per term)
  const int tid = threadIdx.x;
  if (tid == 0) c = *a.ctl;
  __syncthreads();
  // nothing to do (budget used up / training still pending): skip the 44 KB weight load
  if (c.train_pending || c.taken >= c.budget || c.global_step >= a.cfg.total_timesteps) return;
  for (int p = tid; p < QP; p += 128) wq[p] = a.q[p];
  __syncthreads();
  while (true) {
    if (tid == 0) {
      go = (!c.train_pending && c.taken < c.budget && c.global_step < a.cfg.total_timesteps) ? 1 : 0;
      if (go) {
        c.global_step += 1; c.taken += 1;                                            // dqn.jl:57
        const uint64_t gstep = (uint64_t)c.global_step;
        for (int i = 0; i < QD; ++i) obs[i] = c.env[i];                              // dqn.jl:58
        eps_s = dq_linear_schedule(a.cfg.epsilon_start, a.cfg.epsilon_end, a.cfg.epsilon_duration, (double)c.global_step);
        if (u53(philox_env(a.cfg.seed, 0u, gstep, 0u)) < eps_s) {                    // dqn.jl:61-62
          need_q = 0;
          action_s = (int)(philox_env(a.cfg.seed, 0u, gstep, 4u).x >> 31);
        } else need_q = 1;
      }
    }
    __syncthreads();
    if (!go) break;
    if (need_q) {                                                                    // dqn.jl:64 qs = q_net(obs)
      dqn_block_trunk(wq, obs, h1s, h2s);
      if (tid < QA) qs[tid] = dqn_head_row(wq, QA, tid, h2s);
      __syncthreads();
    }
    if (tid == 0) {
      const uint64_t gstep = (uint64_t)c.global_step;
      const int action = need_q ? (qs[1] > qs[0] ? 1 : 0) : action_s;               // dqn.jl:65 argmax: first maximum
      const bool done = cartpole_step64(c.env, c.env_t, action, a.cfg.max_steps);  // dqn.jl:68
      const double rew = done ? 0.0 : 1.0;
      const size_t p = (size_t)c.ptr;                                                // dqn.jl:71-78 Buffer.add!
      for (int i = 0; i < QD; ++i) { a.rb_state[QD * p + i] = obs[i]; a.rb_next[QD * p + i] = c.env[i]; }
      a.rb_action[p] = action; a.rb_reward[p] = rew; a.rb_terminal[p] = done ? 1 : 0;
      c.ptr = c.ptr + 1 >= a.cfg.buffer_size ? 0 : c.ptr + 1;
      c.size = c.size + 1 > a.cfg.buffer_size ? a.cfg.buffer_size : c.size + 1;
      c.episode_return += rew; c.episode_length += 1;                               // dqn.jl:81-82
      if (done) {                                                                    // dqn.jl:83-90
        if (c.n_eps < DQN_MAX_EPS) {
          a.eps[c.n_eps].episode_return = c.episode_return; a.eps[c.n_eps].episode_length = c.episode_length;
          a.eps[c.n_eps].global_step = c.global_step; a.eps[c.n_eps].epsilon = eps_s;
        }
        c.n_eps += 1;
        c.episode_length = 0; c.episode_return = 0.0;
        env_reset64(c.env, a.cfg.seed, gstep, 1); c.env_t = 0;
      }
      c.train_pending = (c.global_step > a.cfg.min_buff_size && c.global_step % a.cfg.train_freq == 0) ? 1 : 0;   // dqn.jl:93
    }
    __syncthreads();
  }
  if (tid == 0) *a.ctl = c;
}

// Buffer.sample(rb, batch_size) (dqn.jl:94): replay_sample.hpp's self-avoiding draws (oracle: dqn_sample_indices)
__global__ void __launch_bounds__(1024) dqn_sample_kernel(DQNDev a) {
  if (!a.ctl->train_pending) return;
  replay_sample<DQN_MAX_CAP>(a.cfg.seed, (uint64_t)a.ctl->global_step, (int)a.ctl->size, (int)a.cfg.batch_size, a.idx);
}

// forward of q_net(state) (net 0), target_net(x) (net 1) and, on a double_q handle, q_net(x) (net 2), x = next_state[boot], one output element per
// thread (dqn.jl:99,104)
__global__ void __launch_bounds__(256) dqn_fwd1_kernel(DQNDev a) {
#pragma clang fp contract(off)
  if (!a.ctl->train_pending) return;
  const int k = (int)a.cfg.batch_size, o = blockIdx.x * 256 + threadIdx.x;
  if (o >= a.nets * QH1 * k) return;
  const int net = o / (QH1 * k), r = o - net * (QH1 * k), b = r / QH1, i = r - b * QH1;
  const float* p = net == 1 ? a.t : a.q;
  const double* x = net ? a.rb_next + (size_t)QD * a.boot[b] : a.rb_state + (size_t)QD * a.idx[b];
  double acc = 0.0;
  for (int kk = 0; kk < QD; ++kk) acc += (double)p[QoW1 + i + QH1 * kk] * x[kk];
  acc += (double)p[Qob1 + i];
  a.H1[(size_t)net * QH1 * k + r] = acc > 0.0 ? acc : 0.0;
}
__global__ void __launch_bounds__(256) dqn_fwd2_kernel(DQNDev a) {
#pragma clang fp contract(off)
  if (!a.ctl->train_pending) return;
  const int k = (int)a.cfg.batch_size, o = blockIdx.x * 256 + threadIdx.x;
  if (o >= a.nets * QH2 * k) return;
  const int net = o / (QH2 * k), r = o - net * (QH2 * k), b = r / QH2, j = r - b * QH2;
  const float* p = net == 1 ? a.t : a.q;
  const double* h = a.H1 + (size_t)net * QH1 * k + (size_t)QH1 * b;
  double acc = 0.0;
#pragma unroll 8
  for (int kk = 0; kk < QH1; ++kk) acc += (double)p[QoW2 + j + QH2 * kk] * h[kk];
  acc += (double)p[Qob2 + j];
  a.H2[(size_t)net * QH2 * k + r] = acc > 0.0 ? acc : 0.0;
}
// the head's `rows` outputs of every pass → dst [nets][k][rows]: one output element per thread, input order, bias last. The scalar head's two Q(a)
// go to Q (rows is a compile-time 2 there), the categorical head's 2N logits to c51.L: two kernels, so that neither branches on its caller.
__device__ __forceinline__ void dqn_fwd3_rows(const DQNDev& a, int rows, double* dst) {
#pragma clang fp contract(off)
  const int k = (int)a.cfg.batch_size, o = blockIdx.x * 256 + threadIdx.x;
  if (o >= a.nets * rows * k) return;
  const int net = o / (rows * k), r = o - net * (rows * k), b = r / rows, row = r - b * rows;
  dst[(size_t)net * rows * k + r] = dqn_head_row(net == 1 ? a.t : a.q, rows, row, a.H2 + (size_t)net * QH2 * k + (size_t)QH2 * b);
}
__global__ void __launch_bounds__(256) dqn_fwd3_kernel(DQNDev a) {
  if (!a.ctl->train_pending) return;
  dqn_fwd3_rows(a, QA, a.Q);
}
// The TD launch of the scalar heads, one block: TD target, mse, output cotangent (dqn.jl:99-107), the loss summed in sample order by thread 0.
// TGT = false is dqn.jl's target, td = reward + gamma·max target_net(x)·(1 − terminal) at the sampled slot, and touches nothing of a.tgt. TGT = true
// (crl_dqn_create_with and the scalar dueling handles) is dqn_target.hpp's: a* from q_net(x) (plane 2) under double_q, next_q = target_net(x)[a*],
// td = R + disc·next_q·(1 − terminal[last]); at n_step = 1 without double_q that is the same arithmetic. PER = true takes the place of the mse by the
// importance-weighted one, loss = (Σ_b w_b·δ_b², sample order)/k, dz_b = −2·w_b·δ_b/k, and adds the priority write-back of dqn_per.hpp: the new
// leaves of idx_b, max_leaf raised to the batch's largest new leaf, the ancestors repaired.
template <bool TGT, bool PER>
__global__ void __launch_bounds__(1024) dqn_td_kernel(DQNDev a) {
#pragma clang fp contract(off)
  if (!a.ctl->train_pending) return;
  __shared__ float lmax[16];
  const PerDev& p = a.per;
  const int k = (int)a.cfg.batch_size;
  float mine = 0.0f;
  for (int b = threadIdx.x; b < k; b += blockDim.x) {
    const double tq0 = a.Q[(size_t)QA * k + QA * b], tq1 = a.Q[(size_t)QA * k + QA * b + 1];
    const int s = a.idx[b];
    double td;
    if constexpr (TGT) {
      const TgtDev& t = a.tgt;
      const double sq0 = t.double_q ? a.Q[(size_t)2 * QA * k + QA * b] : 0.0, sq1 = t.double_q ? a.Q[(size_t)2 * QA * k + QA * b + 1] : 0.0;
      const int astar = tgt_astar(t.double_q, sq0, sq1, tq0, tq1);
      td = tgt_td(t.nret[b], t.ndisc[b], astar ? tq1 : tq0, a.rb_terminal[t.last[b]]);
      t.astar[b] = astar; t.td[b] = td;
    } else {
      const double next_q = tq1 > tq0 ? tq1 : tq0;
      td = a.rb_reward[s] + a.cfg.gamma * next_q * (1.0 - (double)a.rb_terminal[s]);
    }
    const double diff = td - a.Q[QA * b + a.rb_action[s]];
    if constexpr (PER) {
      const double w = p.w[b];
      a.sq[b] = w * (diff * diff);
      a.dz[b] = -2.0 * w * diff / (double)k;
      per_td_writeback(p, b, s, diff < 0.0 ? -diff : diff, mine);
    } else {
      a.sq[b] = diff * diff;
      a.dz[b] = -2.0 * diff / (double)k;
    }
  }
  if constexpr (PER) per_block_max(mine, lmax);
  __syncthreads();
  if (threadIdx.x == 0) dqn_loss_in_sample_order(a);
  if constexpr (PER) per_batch_tail(p, a.idx, k, lmax);
}

// ------------------------------------------------------------------------------------------------------
// Prioritized replay (crl_dqn_per_create; dqn_per.hpp): dqn_per_sample_kernel takes the place of dqn_sample_kernel and the TD launch is a PER = true
// instantiation of dqn_td_kernel, so the cycle stays ten launches. One block of 1024 each.
// ------------------------------------------------------------------------------------------------------
// Add (the slots the ring took since the last update get max_leaf, their ancestors are repaired), beta(g), the draw, the weights
__device__ __forceinline__ void dqn_per_sample_body(const DQNDev& a) {
#pragma clang fp contract(off)
  const PerDev& p = a.per;
  const int C = p.C, cap = (int)a.cfg.buffer_size, k = (int)a.cfg.batch_size, n = (int)a.ctl->size, ptr = (int)a.ctl->ptr;
  const int64_t g = a.ctl->global_step, behind = g - p.ctl->synced_step;
  const int fresh = behind < (int64_t)cap ? (int)behind : cap;
  const double fill = (double)p.ctl->max_leaf;              // as of the last completed update
  const auto slot_of = [=](int i) { const int s = ptr - 1 - i; return s < 0 ? s + cap : s; };   // the i-th slot behind ptr
  for (int i = threadIdx.x; i < fresh; i += blockDim.x) p.tree[C + slot_of(i)] = fill;
  per_repair(p.tree, C, fresh, slot_of);
  const double beta = per_beta(p.beta_start, p.beta_end, p.beta_duration, (double)g);
  per_draw(p.tree, C, k, a.cfg.seed, (uint64_t)g, a.idx);
  per_weights(p.tree, C, n, k, beta, a.idx, p.w);
  if (threadIdx.x == 0) { p.ctl->synced_step = g; p.ctl->beta = beta; }
}
__global__ void __launch_bounds__(1024) dqn_per_sample_kernel(DQNDev a) {
  if (!a.ctl->train_pending) return;
  dqn_per_sample_body(a);
}
// crl_dqn_per_probe: the sampler alone on a scratch tree whose leaves the host wrote (every inner node is rebuilt first)
__global__ void __launch_bounds__(1024) dqn_per_probe_kernel(double* tree, int C, int n, int k, uint64_t seed, uint64_t g, double beta, int32_t* idx,
                                                             double* w) {
  per_repair(tree, C, C, [](int i) { return i; });
  per_draw(tree, C, k, seed, g, idx);
  per_weights(tree, C, n, k, beta, idx, w);
}

// ------------------------------------------------------------------------------------------------------
// n-step / double-Q targets (crl_dqn_create_with; dqn_target.hpp): dqn_tgt_sample_kernel takes the place of the sampling launch and the TD launch is
// a TGT = true instantiation of dqn_td_kernel, PER or uniform, so the cycle stays ten launches. One block of 1024 each.
// ------------------------------------------------------------------------------------------------------
// The draw of the handle's replay, then each sample's n-step walk in the block that drew: both samplers end on a block barrier, after which idx is
// visible to every thread; the ring and its write pointer are those the collect launch left.
template <bool PER>
__global__ void __launch_bounds__(1024) dqn_tgt_sample_kernel(DQNDev a) {
  if (!a.ctl->train_pending) return;
  if constexpr (PER) dqn_per_sample_body(a);
  else replay_sample<DQN_MAX_CAP>(a.cfg.seed, (uint64_t)a.ctl->global_step, (int)a.ctl->size, (int)a.cfg.batch_size, a.idx);
  __syncthreads();
  const TgtDev& t = a.tgt;
  const int k = (int)a.cfg.batch_size, cap = (int)a.cfg.buffer_size, ptr = (int)a.ctl->ptr;
  for (int j = threadIdx.x; j < k; j += blockDim.x) {
    int last, m; double R, disc;
    nstep_walk(a.rb_reward, a.rb_terminal, cap, ptr, (int)a.idx[j], t.n_step, a.cfg.gamma, last, m, R, disc);
    t.last[j] = last; t.m[j] = m; t.nret[j] = R; t.ndisc[j] = disc;
  }
}

__global__ void __launch_bounds__(256) dqn_bwd2_kernel(DQNDev a) {
#pragma clang fp contract(off)
  if (!a.ctl->train_pending) return;
  const int k = (int)a.cfg.batch_size, o = blockIdx.x * 256 + threadIdx.x;
  if (o >= QH2 * k) return;
  const int b = o / QH2, j = o - b * QH2;
  const double s = (double)a.q[QoW3 + a.rb_action[a.idx[b]] + QA * j] * a.dz[b];
  a.d2[o] = a.H2[o] > 0.0 ? s : 0.0;
}
__global__ void __launch_bounds__(256) dqn_bwd1_kernel(DQNDev a) {
#pragma clang fp contract(off)
  if (!a.ctl->train_pending) return;
  const int k = (int)a.cfg.batch_size, o = blockIdx.x * 256 + threadIdx.x;
  if (o >= QH1 * k) return;
  const int b = o / QH1, kk = o - b * QH1;
  const double* dd = a.d2 + (size_t)QH2 * b;
  double s = 0.0;
#pragma unroll 6
  for (int j = 0; j < QH2; ++j) s += (double)a.q[QoW2 + j + QH2 * kk] * dd[j];
  a.d1[o] = a.H1[o] > 0.0 ? s : 0.0;
}
// the weight gradients of the trunk (W1 b1 W2 b2, p < QoW3): shared by dqn_wgrad_kernel and dqn_c51_wgrad_kernel, whose trunks are the same arrays
// every loop is unrolled 30x: the operands were written by the previous launches, so they come from the Infinity Cache
// at ≈2 µs per dependent round trip — 4 rounds of 60 loads in flight instead of 15 of 16. The Float64 adds stay in
// sample order.
__device__ __forceinline__ double dqn_wgrad_trunk(const DQNDev& a, int p, int k) {
#pragma clang fp contract(off)
  double g = 0.0;
  if (p < Qob1) {
    const int i = p % QH1, kk = p / QH1;
#pragma unroll 30
    for (int b = 0; b < k; ++b) g += a.d1[(size_t)QH1 * b + i] * a.rb_state[(size_t)QD * a.idx[b] + kk];
  } else if (p < QoW2) {
    const int i = p - Qob1;
#pragma unroll 30
    for (int b = 0; b < k; ++b) g += a.d1[(size_t)QH1 * b + i];
  } else if (p < Qob2) {
    const int r = p - QoW2, j = r % QH2, kk = r / QH2;
#pragma unroll 30
    for (int b = 0; b < k; ++b) g += a.d2[(size_t)QH2 * b + j] * a.H1[(size_t)QH1 * b + kk];
  } else {
    const int j = p - Qob2;
#pragma unroll 30
    for (int b = 0; b < k; ++b) g += a.d2[(size_t)QH2 * b + j];
  }
  return g;
}
// one parameter per thread, samples summed in sample order, Float32 projection
__global__ void __launch_bounds__(64) dqn_wgrad_kernel(DQNDev a) {
#pragma clang fp contract(off)
  if (!a.ctl->train_pending) return;
  const int k = (int)a.cfg.batch_size, p = blockIdx.x * 64 + threadIdx.x;
  if (p >= QP) return;
  // Adding an exact 0.0 for samples of the other action leaves the sum unchanged.
  double g = 0.0;
  if (p < QoW3) {
    g = dqn_wgrad_trunk(a, p, k);
  } else if (p < Qob3) {
    const int r = p - QoW3, aa = r % QA, j = r / QA;
#pragma unroll 30
    for (int b = 0; b < k; ++b) {
      const double t = a.dz[b] * a.H2[(size_t)QH2 * b + j];
      if (a.rb_action[a.idx[b]] == aa) g += t;
    }
  } else {
    const int aa = p - Qob3;
#pragma unroll 30
    for (int b = 0; b < k; ++b) {
      const double t = a.dz[b];
      if (a.rb_action[a.idx[b]] == aa) g += t;
    }
  }
  a.grads[p] = (float)g;
}
// the Adam launch of the plain net: dqn_adam_step over the six arrays W1 b1 W2 b2 W3 b3, whose bounds are compile-time here; one block
__global__ void __launch_bounds__(1024) dqn_adam_kernel(DQNDev a) {
  if (!a.ctl->train_pending) return;
  dqn_adam_step(a, QP, 6, [](int p) { return dqn_array_of(p, Qob3); });
}

// ------------------------------------------------------------------------------------------------------
// Categorical DQN (crl_dqn_c51_create; dqn_c51.hpp). The trunk W1 b1 W2 b2 sits at the scalar net's offsets, so dqn_fwd1_kernel, dqn_fwd2_kernel and
// dqn_bwd1_kernel run unchanged; the sampling launch is dqn_tgt_sample_kernel (a C51 handle always carries target options, {1, 0} by default). The
// head W3(2N, 84) b3(2N) starts at QoW3; its kernels below take the places of collect, fwd3, TD, bwd2, wgrad and Adam: the cycle stays ten launches.
// ------------------------------------------------------------------------------------------------------
// What the collect kernel keeps in LDS besides the weights. All of it lives in the dynamic region (the weights alone pass the 64 KB static limit at
// N >= 36), the struct first so that the float image behind it starts 16-byte aligned.
struct C51CollectLds {
  DQNCollectLds s;
  double h1s[QH1], h2s[QH2], ls[2 * C51_MAX_ATOMS];
};
constexpr size_t C51_COLLECT_LDS = (sizeof(C51CollectLds) + 15) / 16 * 16;
extern __shared__ __attribute__((aligned(16))) char c51_smem[];

// Q(a) = Σ z·softmax(ls[a·N ..]) for both actions by a block of 128 = two waves, wave a taking action a; ends on a block barrier
__device__ __forceinline__ void c51_block_q(const double* ls, double* qs, const C51Dev& c, double* probs) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const double delta = c51_delta(c.v_min, c.v_max, c.N);
  double p, logp;
  c51_softmax(lane < c.N ? ls[w * c.N + lane] : 0.0, c.N, lane, p, logp);
  const double Q = c51_expect(p, c.v_min, delta, lane);
  if (lane == 0) qs[w] = Q;
  if (probs && lane < c.N) probs[w * c.N + lane] = p;
  __syncthreads();
}

// dqn_collect_kernel with the categorical head: a greedy step forms the 2N logits (one row per thread), then Q(a) as above
__global__ void __launch_bounds__(DQN_OBS_BLOCK) dqn_c51_collect_kernel(DQNDev a) {
#pragma clang fp contract(off)
  C51CollectLds& l = *reinterpret_cast<C51CollectLds*>(c51_smem);
  DQNCollectLds& s = l.s;
  float* const wq = reinterpret_cast<float*>(c51_smem + C51_COLLECT_LDS);
  const int tid = threadIdx.x, P = a.c51.P, NA = 2 * a.c51.N;
  if (tid == 0) s.c = *a.ctl;
  __syncthreads();
  if (s.c.train_pending || s.c.taken >= s.c.budget || s.c.global_step >= a.cfg.total_timesteps) return;   // as dqn_collect_kernel: no weight load
  for (int p = tid; p < P; p += DQN_OBS_BLOCK) wq[p] = a.q[p];
  __syncthreads();
  dqn_collect_loop(a, s, [&] {
#pragma clang fp contract(off)
    dqn_block_trunk(wq, s.obs, l.h1s, l.h2s);
    if (tid < NA) l.ls[tid] = dqn_head_row(wq, NA, tid, l.h2s);
    __syncthreads();
    c51_block_q(l.ls, s.qs, a.c51, nullptr);
  });
  if (tid == 0) *a.ctl = s.c;
}

// the 2N logits of every pass → c51.L: dqn_fwd3_rows with the categorical head's row count
__global__ void __launch_bounds__(256) dqn_c51_fwd3_kernel(DQNDev a) {
  if (!a.ctl->train_pending) return;
  dqn_fwd3_rows(a, 2 * a.c51.N, a.c51.L);
}

// The TD launch of a C51 handle: one wave per sample, one lane per atom, C51_TD_WAVES samples per block, ⌈k / C51_TD_WAVES⌉ blocks — the per-sample work
// is a few thousand wave instructions that all 64 lanes issue alike, so one CU would be bound by issue slots while the others idle. Per sample: Q of
// both actions at x from the a* net, a*, p' = softmax(target_net(x)[a*]), the projection m, softmax of the taken action's logits, loss_j = −Σ m·logp,
// dl; under PER the new leaf from loss_j (duplicates write identical values). What needs the whole batch — the loss in sample order, max_leaf, the
// tree's repair — is dqn_c51_adam_kernel's, the cycle's one-block launch: a launch boundary orders it behind every block here at no extra cost.
template <bool PER>
__global__ void __launch_bounds__(64 * C51_TD_WAVES) dqn_c51_td_kernel(DQNDev a) {
#pragma clang fp contract(off)
  if (!a.ctl->train_pending) return;
  const PerDev& p = a.per;
  const TgtDev& t = a.tgt;
  const C51Dev& c = a.c51;
  const int k = (int)a.cfg.batch_size, N = c.N, lane = threadIdx.x & 63, b = blockIdx.x * C51_TD_WAVES + (threadIdx.x >> 6);
  if (b >= k) return;                                                        // whole waves leave: the wave functions below see all 64 lanes
  const size_t plane = (size_t)2 * N * k;
  const double delta = c51_delta(c.v_min, c.v_max, N);
  const int s = a.idx[b], act = a.rb_action[s];
  const double* Lt = c.L + plane + (size_t)2 * N * b;                        // target_net(x)
  const double* Lx = t.double_q ? c.L + 2 * plane + (size_t)2 * N * b : Lt;   // the net a* is taken from
  double p0, p1, lp;
  c51_softmax(lane < N ? Lx[lane] : 0.0, N, lane, p0, lp);
  const double Q0 = c51_expect(p0, c.v_min, delta, lane);
  c51_softmax(lane < N ? Lx[N + lane] : 0.0, N, lane, p1, lp);
  const double Q1 = c51_expect(p1, c.v_min, delta, lane);
  const int astar = Q1 > Q0 ? 1 : 0;
  double pp = astar ? p1 : p0, Qt = astar ? Q1 : Q0;
  if (t.double_q) {
    c51_softmax(lane < N ? Lt[astar * N + lane] : 0.0, N, lane, pp, lp);
    Qt = c51_expect(pp, c.v_min, delta, lane);
  }
  const int last = t.last[b];
  const double m = c51_project(pp, t.nret[b], t.ndisc[b], a.rb_terminal[last], c.v_min, c.v_max, delta, N, lane);
  double pi, logp;
  c51_softmax(lane < N ? c.L[(size_t)2 * N * b + act * N + lane] : 0.0, N, lane, pi, logp);
  const double loss_j = -c51_sum(m * logp);
  const double wj = PER ? p.w[b] : 1.0;
  if (lane < N) {
    c.dl[(size_t)N * b + lane] = wj * (pi - m) / (double)k;
    c.proj[(size_t)N * b + lane] = m;
  }
  if (lane == 0) {
    c.sloss[b] = loss_j;
    a.sq[b] = wj * loss_j;
    t.astar[b] = astar; t.td[b] = tgt_td(t.nret[b], t.ndisc[b], Qt, a.rb_terminal[last]);
    if constexpr (PER) {
      p.abs_td[b] = loss_j;
      p.tree[p.C + s] = (double)per_leaf(loss_j, p.eps, p.alpha);
    }
  }
}

// d2_j = relu'(H2_j) · Σ_i W3[a·N + i, j] · dl_i, atoms ascending
__global__ void __launch_bounds__(256) dqn_c51_bwd2_kernel(DQNDev a) {
#pragma clang fp contract(off)
  if (!a.ctl->train_pending) return;
  const int k = (int)a.cfg.batch_size, N = a.c51.N, o = blockIdx.x * 256 + threadIdx.x;
  if (o >= QH2 * k) return;
  const int b = o / QH2, j = o - b * QH2;
  const float* w3 = a.q + QoW3 + a.rb_action[a.idx[b]] * N + 2 * N * j;
  const double* dl = a.c51.dl + (size_t)N * b;
  double s = 0.0;
#pragma unroll 4
  for (int i = 0; i < N; ++i) s += (double)w3[i] * dl[i];
  a.d2[o] = a.H2[o] > 0.0 ? s : 0.0;
}
// dqn_wgrad_kernel with the head's 2N rows: row a·N + i takes dl_i of the samples whose action is a, an exact 0.0 of the others
__global__ void __launch_bounds__(64) dqn_c51_wgrad_kernel(DQNDev a) {
#pragma clang fp contract(off)
  if (!a.ctl->train_pending) return;
  const int k = (int)a.cfg.batch_size, N = a.c51.N, NA = 2 * N, ob3 = QoW3 + NA * QH2, p = blockIdx.x * 64 + threadIdx.x;
  if (p >= a.c51.P) return;
  double g = 0.0;
  if (p < QoW3) {
    g = dqn_wgrad_trunk(a, p, k);
  } else if (p < ob3) {
    const int r = p - QoW3, row = r % NA, j = r / NA, aa = row / N, i = row - aa * N;
#pragma unroll 30
    for (int b = 0; b < k; ++b) {
      const double t = a.c51.dl[(size_t)N * b + i] * a.H2[(size_t)QH2 * b + j];
      if (a.rb_action[a.idx[b]] == aa) g += t;
    }
  } else {
    const int row = p - ob3, aa = row / N, i = row - aa * N;
#pragma unroll 30
    for (int b = 0; b < k; ++b) {
      const double t = a.c51.dl[(size_t)N * b + i];
      if (a.rb_action[a.idx[b]] == aa) g += t;
    }
  }
  a.grads[p] = (float)g;
}
// dqn_adam_kernel over the C51 handle's P parameters: the same six arrays, the head's two being longer. Being the cycle's one-block launch behind the
// TD launch, it first does what needs the whole batch: loss = (Σ_b sq_b, sample order) / k, and under PER max_leaf raised to the batch's largest new
// leaf and the ancestors of the written leaves repaired (dqn_td_kernel<·, true>'s tail; here the maximum is taken over the leaves that
// dqn_c51_td_kernel wrote): dqn_c51_batch_tail, which dqn_duel_adam_kernel runs as well.
__device__ __forceinline__ void dqn_c51_batch_tail(const DQNDev& a) {
#pragma clang fp contract(off)
  if (threadIdx.x == 0) dqn_loss_in_sample_order(a);
  if (a.per.on) {
    __shared__ float lmax[16];
    const PerDev& p = a.per;
    const int k = (int)a.cfg.batch_size;
    float mine = 0.0f;
    for (int b = threadIdx.x; b < k; b += blockDim.x) { const float leaf = (float)p.tree[p.C + a.idx[b]]; mine = leaf > mine ? leaf : mine; }
    per_block_max(mine, lmax);
    __syncthreads();
    per_batch_tail(p, a.idx, k, lmax);
  }
}
__global__ void __launch_bounds__(1024) dqn_c51_adam_kernel(DQNDev a) {
  if (!a.ctl->train_pending) return;
  dqn_c51_batch_tail(a);
  const int ob3 = QoW3 + 2 * a.c51.N * QH2;
  dqn_adam_step(a, a.c51.P, 6, [=](int p) { return dqn_array_of(p, ob3); });
}

// crl_dqn_q_values and crl_dqn_c51_probs on a C51 handle: dqn_q_kernel's trunk, the 2N logits, then Q(a) and / or the probabilities (N, 2, n)
__global__ void __launch_bounds__(DQN_OBS_BLOCK) dqn_c51_q_kernel(const float* __restrict__ q, C51Dev c, const double* __restrict__ obs, int n,
                                                        double* __restrict__ out_q, double* __restrict__ out_p) {
#pragma clang fp contract(off)
  __shared__ double h1s[QH1], h2s[QH2], ls[2 * C51_MAX_ATOMS], qs[QA];
  const int b = blockIdx.x, tid = threadIdx.x, NA = 2 * c.N;
  if (b >= n) return;
  dqn_block_trunk(q, obs + (size_t)QD * b, h1s, h2s);
  if (tid < NA) ls[tid] = dqn_head_row(q, NA, tid, h2s);
  __syncthreads();
  c51_block_q(ls, qs, c, out_p ? out_p + (size_t)NA * b : nullptr);
  if (out_q && tid < QA) out_q[(size_t)QA * b + tid] = qs[tid];
}

__global__ void dqn_init_kernel(DQNDev a) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  DQNCtl c;
  memset(&c, 0, sizeof(c));
  env_reset64(c.env, a.cfg.seed, 0, 2);                                             // dqn.jl:56 reset!(env)
  *a.ctl = c;
}

// q_net(obs) on caller-supplied observations: one thread per (observation, layer unit) would be overkill — a wave per
// observation, lanes striding the units
__global__ void __launch_bounds__(DQN_OBS_BLOCK) dqn_q_kernel(const float* __restrict__ q, const double* __restrict__ obs, int n, double* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ double h1s[QH1], h2s[QH2];
  const int b = blockIdx.x, tid = threadIdx.x;
  if (b >= n) return;
  dqn_block_trunk(q, obs + (size_t)QD * b, h1s, h2s);
  if (tid < QA) out[(size_t)QA * b + tid] = dqn_head_row(q, QA, tid, h2s);
}

// ------------------------------------------------------------------------------------------------------
// crl_dqn_evaluate: the frozen q_net, greedy, on n private CartPoles, `episodes` episodes each, in ONE launch. One wave owns one env from its first
// reset to its last step, DQN_EVAL_WAVES envs per block. The whole q_net (43.7 KB) is staged once per block into LDS as float and widened at use, so
// the step loop reads no global memory; a wave takes the 120 and the 84 units as two units per lane (lane and lane + 64: two independent chains side by
// side, which halves the dependent adds of a step) through its private h1 / h2 strips, and every lane forms both head sums, env state, episode sums and the action alike (wave-uniform: no broadcast). Each unit's dot product is
// dqn_q_kernel's — input order, bias last, contraction off —, so an action has the bits crl_dqn_q_values gives for the same observation.
// Episodes end at different steps: after the ONE staging barrier no wave meets a block barrier again — a wave past n, or one whose env has played
// its quota, simply leaves; layers are separated by wave_lds_fence on the wave-private strips.
// ------------------------------------------------------------------------------------------------------
#ifndef CRL_DQN_EVAL_WAVES
#define CRL_DQN_EVAL_WAVES 4  // envs per block; experiment builds (csrc/Makefile, EXTRA=-DCRL_DQN_EVAL_WAVES=n) measured 1, 2, 4, 8: DESIGN.md §3f
#endif
constexpr int DQN_EVAL_WAVES = CRL_DQN_EVAL_WAVES;
static_assert(QP * 4 + DQN_EVAL_WAVES * (QH1 + QH2) * 8 <= 64 * 1024, "q_net + the waves' strips must fit the 64 KB static LDS limit");
__global__ void __launch_bounds__(64 * DQN_EVAL_WAVES) dqn_eval_kernel(const float* __restrict__ q, int max_steps, double gamma, ValueEvalArgs ev) {
#pragma clang fp contract(off)
  __shared__ float wq[QP];
  __shared__ double h1s[DQN_EVAL_WAVES][QH1], h2s[DQN_EVAL_WAVES][QH2];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, env = blockIdx.x * DQN_EVAL_WAVES + w;
  for (int p = threadIdx.x; p < QP; p += 64 * DQN_EVAL_WAVES) wq[p] = q[p];
  __syncthreads();                       // the only block barrier of the kernel
  if (env >= ev.n) return;
  double* const h1w = h1s[w];
  double* const h2w = h2s[w];
  dqn_eval_episodes(ev, env, lane, max_steps, gamma, [&](const double* s, double& q0, double& q1) {
#pragma clang fp contract(off)
    eval_layer1_pair(wq, QoW1, Qob1, s, h1w, lane);
    wave_lds_fence();
    eval_layer2_pair(wq, h1w, h2w, lane);
    wave_lds_fence();
    eval_head_pair(wq, QA, 0, 1, h2w, q0, q1);   // every lane forms both head sums alike
  });
}

// dqn_eval_kernel with the categorical head: the same one-wave-per-env structure with ONE staging barrier. The net (up to 86.6 KB at N = 64) and the
// waves' strips live in dynamic LDS. Lane i < N forms the logits of atom i for both actions (rows i and N + i: two chains side by side), then the two
// softmaxes and expectations run wave-wide (dqn_c51.hpp: no LDS in them); Q(a) has the bits crl_dqn_q_values gives.
struct C51EvalWaveLds { double h1[QH1], h2[QH2]; };
__global__ void __launch_bounds__(64 * DQN_EVAL_WAVES) dqn_c51_eval_kernel(const float* __restrict__ q, C51Dev c, int max_steps, double gamma,
                                                                           ValueEvalArgs ev) {
#pragma clang fp contract(off)
  C51EvalWaveLds* const wl = reinterpret_cast<C51EvalWaveLds*>(c51_smem);
  float* const wq = reinterpret_cast<float*>(c51_smem + sizeof(C51EvalWaveLds) * DQN_EVAL_WAVES);
  static_assert(sizeof(C51EvalWaveLds) % 16 == 0, "the weight image starts 16-byte aligned");
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, env = blockIdx.x * DQN_EVAL_WAVES + w, N = c.N;
  for (int p = threadIdx.x; p < c.P; p += 64 * DQN_EVAL_WAVES) wq[p] = q[p];
  __syncthreads();                       // the only block barrier of the kernel
  if (env >= ev.n) return;
  double* const h1w = wl[w].h1;
  double* const h2w = wl[w].h2;
  const double delta = c51_delta(c.v_min, c.v_max, N);
  const int r0 = lane < N ? lane : 0, r1 = N + r0;   // a lane past N repeats atom 0 and its results are masked by the wave functions
  dqn_eval_episodes(ev, env, lane, max_steps, gamma, [&](const double* s, double& q0, double& q1) {
#pragma clang fp contract(off)
    eval_layer1_pair(wq, QoW1, Qob1, s, h1w, lane);
    wave_lds_fence();
    eval_layer2_pair(wq, h1w, h2w, lane);
    wave_lds_fence();
    double l0, l1, p0, p1, lp;
    eval_head_pair(wq, 2 * N, r0, r1, h2w, l0, l1);
    c51_softmax(l0, N, lane, p0, lp);
    q0 = c51_expect(p0, c.v_min, delta, lane);
    c51_softmax(l1, N, lane, p1, lp);
    q1 = c51_expect(p1, c.v_min, delta, lane);
  });
}

// ------------------------------------------------------------------------------------------------------
// Dueling heads (crl_dqn_dueling_create; dqn_duel.hpp). One family for both heads, R = 1 (scalar) or N (categorical) at run time. W1 b1 sit at the
// plain net's offsets, so dqn_fwd1_kernel runs unchanged, and such a handle always carries target options, so the sampling launch is
// dqn_tgt_sample_kernel. The two streams are combined where the head's output is written (dqn_duel_fwd3_kernel): the combined Q or logits land in the
// buffers the TD kernels read (Q, c51.L), so dqn_td_kernel<true, ·> / dqn_c51_td_kernel run as they are and what they leave (dz, c51.dl) is the cotangent g
// of out_{act,·}. The kernels below take the places of collect, fwd2, fwd3, bwd2, bwd1, wgrad and Adam: the cycle stays ten launches.
// ------------------------------------------------------------------------------------------------------
struct DuelCollectLds {
  DQNCollectLds s;
  double h1s[DUEL_H1], h2s[DUEL_U2], raw[3 * DUEL_MAX_R], ls[2 * DUEL_MAX_R];   // raw: V (R), then A (2R), before they are combined
};
constexpr size_t DUEL_COLLECT_LDS = (sizeof(DuelCollectLds) + 15) / 16 * 16;
struct DuelEvalWaveLds { double h1[DUEL_H1], h2[DUEL_U2]; };
constexpr int DUEL_EVAL_WAVES = DQN_EVAL_WAVES < 4 ? DQN_EVAL_WAVES : 4;   // four waves' strips beside the largest net are what the CU's LDS holds
constexpr size_t DUEL_LDS_LIMIT = 160 * 1024;                              // one workgroup may take the whole CU's LDS
static_assert(DUEL_MAX_R == C51_MAX_ATOMS && DUEL_H1 == QH1 && DUEL_H2 == QH2 && DUEL_D == QD, "one net shape");
static_assert(DUEL_COLLECT_LDS + (size_t)duel_param_count(DUEL_MAX_R) * 4 <= DUEL_LDS_LIMIT, "collect: the largest net + the block's strips fit the CU's LDS");
static_assert(sizeof(DuelEvalWaveLds) * DUEL_EVAL_WAVES + (size_t)duel_param_count(DUEL_MAX_R) * 4 <= DUEL_LDS_LIMIT,
              "evaluation: the largest net + the waves' strips fit the CU's LDS");
static_assert(sizeof(DuelEvalWaveLds) % 16 == 0, "the weight image starts 16-byte aligned");

// the block's forward for one observation, layers separated by block barriers: h1 (120), h2 (168), raw (V then A), ls = the combined head (2R). Ends on
// a block barrier. The q kernel and the collect kernel run it, 128 threads each.
__device__ __forceinline__ void duel_block_forward(const float* W, const DuelOff& o, int R, const double* obs, double* h1s, double* h2s, double* raw,
                                                   double* ls) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x, nth = blockDim.x;
  dqn_block_layer1(W, obs, h1s);   // W1 b1 sit at the plain net's offsets; one unit per thread: both callers are DQN_OBS_BLOCK-thread kernels
  for (int u = tid; u < DUEL_U2; u += nth) h2s[u] = duel_hidden2(W, o, u, h1s);
  __syncthreads();
  for (int r = tid; r < 3 * R; r += nth) raw[r] = duel_head_row(W, o, R, r, h2s);
  __syncthreads();
  for (int i = tid; i < R; i += nth) duel_combine(raw[i], raw[R + i], raw[2 * R + i], ls[i], ls[R + i]);
  __syncthreads();
}

// dqn_c51_collect_kernel with the dueling heads: the whole net in dynamic LDS (84.7 KB at R = 1, 149.0 KB at R = 64)
__global__ void __launch_bounds__(DQN_OBS_BLOCK) dqn_duel_collect_kernel(DQNDev a) {
#pragma clang fp contract(off)
  DuelCollectLds& l = *reinterpret_cast<DuelCollectLds*>(c51_smem);
  DQNCollectLds& s = l.s;
  float* const wq = reinterpret_cast<float*>(c51_smem + DUEL_COLLECT_LDS);
  const int tid = threadIdx.x, P = a.duel.P, R = a.duel.R;
  const DuelOff o = duel_off(R);
  if (tid == 0) s.c = *a.ctl;
  __syncthreads();
  if (s.c.train_pending || s.c.taken >= s.c.budget || s.c.global_step >= a.cfg.total_timesteps) return;   // as dqn_collect_kernel: no weight load
  for (int p = tid; p < P; p += DQN_OBS_BLOCK) wq[p] = a.q[p];
  __syncthreads();
  dqn_collect_loop(a, s, [&] {
#pragma clang fp contract(off)
    duel_block_forward(wq, o, R, s.obs, l.h1s, l.h2s, l.raw, l.ls);
    if (a.c51.on) c51_block_q(l.ls, s.qs, a.c51, nullptr);
    else {
      if (tid < QA) s.qs[tid] = l.ls[tid];
      __syncthreads();
    }
  });
  if (tid == 0) *a.ctl = s.c;
}

// the two-stream hidden layer of every pass: 168 units per sample, one per thread
__global__ void __launch_bounds__(256) dqn_duel_fwd2_kernel(DQNDev a) {
#pragma clang fp contract(off)
  if (!a.ctl->train_pending) return;
  const int k = (int)a.cfg.batch_size, o = blockIdx.x * 256 + threadIdx.x;
  if (o >= a.nets * DUEL_U2 * k) return;
  const int net = o / (DUEL_U2 * k), r = o - net * (DUEL_U2 * k), b = r / DUEL_U2, u = r - b * DUEL_U2;
  const float* p = net == 1 ? a.t : a.q;
  a.H2[(size_t)net * DUEL_U2 * k + r] = duel_hidden2(p, duel_off(a.duel.R), u, a.H1 + (size_t)net * QH1 * k + (size_t)QH1 * b);
}
// V_i, A_{0,i}, A_{1,i} and the combined out_{a,i} of every pass, one i per thread, written where the TD kernels read: Q (R = 1) or c51.L (R = N)
__global__ void __launch_bounds__(256) dqn_duel_fwd3_kernel(DQNDev a) {
#pragma clang fp contract(off)
  if (!a.ctl->train_pending) return;
  const int k = (int)a.cfg.batch_size, R = a.duel.R, o = blockIdx.x * 256 + threadIdx.x;
  if (o >= a.nets * R * k) return;
  const int net = o / (R * k), r = o - net * (R * k), b = r / R, i = r - b * R;
  const float* p = net == 1 ? a.t : a.q;
  const DuelOff off = duel_off(R);
  const double* h = a.H2 + (size_t)net * DUEL_U2 * k + (size_t)DUEL_U2 * b;
  const double V = duel_head_row(p, off, R, i, h), A0 = duel_head_row(p, off, R, R + i, h), A1 = duel_head_row(p, off, R, 2 * R + i, h);
  double* dst = (a.c51.on ? a.c51.L : a.Q) + (size_t)net * 2 * R * k + (size_t)2 * R * b;
  duel_combine(V, A0, A1, dst[i], dst[R + i]);
}
// d2v_j = relu'(h2v_j) · Σ_i W3v[i,j]·g_i; d2a_j = relu'(h2a_j) · Σ_row W3a[row,j]·dA_row, row = a·R + i ascending; g = dz (R = 1) or dl (R = N)
__global__ void __launch_bounds__(256) dqn_duel_bwd2_kernel(DQNDev a) {
#pragma clang fp contract(off)
  if (!a.ctl->train_pending) return;
  const int k = (int)a.cfg.batch_size, R = a.duel.R, o = blockIdx.x * 256 + threadIdx.x;
  if (o >= DUEL_U2 * k) return;
  const int b = o / DUEL_U2, u = o - b * DUEL_U2, act = a.rb_action[a.idx[b]];
  const DuelOff off = duel_off(R);
  const double* g = a.c51.on ? a.c51.dl + (size_t)R * b : a.dz + b;
  double s = 0.0;
  if (u < QH2) {
    const float* w = a.q + off.W3v + R * u;
#pragma unroll 4
    for (int i = 0; i < R; ++i) s += (double)w[i] * g[i];
  } else {
    const float* w = a.q + off.W3a + 2 * R * (u - QH2);
    for (int aa = 0; aa < QA; ++aa) {
#pragma unroll 4
      for (int i = 0; i < R; ++i) s += (double)w[aa * R + i] * duel_dadv(g[i], act, aa);
    }
  }
  a.d2[o] = a.H2[o] > 0.0 ? s : 0.0;
}
// d1_k = relu'(h1_k) · (Σ_j W2v[j,k]·d2v_j, then the same accumulator on with Σ_j W2a[j,k]·d2a_j)
__global__ void __launch_bounds__(256) dqn_duel_bwd1_kernel(DQNDev a) {
#pragma clang fp contract(off)
  if (!a.ctl->train_pending) return;
  const int k = (int)a.cfg.batch_size, o = blockIdx.x * 256 + threadIdx.x;
  if (o >= QH1 * k) return;
  const int b = o / QH1, kk = o - b * QH1;
  const DuelOff off = duel_off(a.duel.R);
  const double* dd = a.d2 + (size_t)DUEL_U2 * b;
  double s = 0.0;
#pragma unroll 6
  for (int j = 0; j < QH2; ++j) s += (double)a.q[off.W2v + j + QH2 * kk] * dd[j];
#pragma unroll 6
  for (int j = 0; j < QH2; ++j) s += (double)a.q[off.W2a + j + QH2 * kk] * dd[QH2 + j];
  a.d1[o] = a.H1[o] > 0.0 ? s : 0.0;
}
// dqn_wgrad_kernel over the ten arrays: one parameter per thread, samples in sample order, Float32 projection. Both rows of W3a / b3a get a term
// from every sample (±g·0.5), unlike the plain head.
__global__ void __launch_bounds__(64) dqn_duel_wgrad_kernel(DQNDev a) {
#pragma clang fp contract(off)
  if (!a.ctl->train_pending) return;
  const int k = (int)a.cfg.batch_size, R = a.duel.R, p = blockIdx.x * 64 + threadIdx.x;
  if (p >= a.duel.P) return;
  const DuelOff off = duel_off(R);
  const double* g = a.c51.on ? a.c51.dl : a.dz;       // [k][R]
  double s = 0.0;
  if (p < off.W2v) {
    s = dqn_wgrad_trunk(a, p, k);                      // W1 b1: the plain trunk's offsets and sums
  } else if (p < off.W3v || (p >= off.W2a && p < off.W3a)) {
    const bool adv = p >= off.W2a;
    const int r = p - (adv ? off.W2a : off.W2v), u0 = adv ? QH2 : 0;
    if (r < QH2 * QH1) {
      const int j = r % QH2, kk = r / QH2;
#pragma unroll 30
      for (int b = 0; b < k; ++b) s += a.d2[(size_t)DUEL_U2 * b + u0 + j] * a.H1[(size_t)QH1 * b + kk];
    } else {
      const int j = r - QH2 * QH1;
#pragma unroll 30
      for (int b = 0; b < k; ++b) s += a.d2[(size_t)DUEL_U2 * b + u0 + j];
    }
  } else if (p < off.b3v) {
    const int r = p - off.W3v, i = r % R, j = r / R;
#pragma unroll 30
    for (int b = 0; b < k; ++b) s += g[(size_t)R * b + i] * a.H2[(size_t)DUEL_U2 * b + j];
  } else if (p < off.W2a) {
    const int i = p - off.b3v;
#pragma unroll 30
    for (int b = 0; b < k; ++b) s += g[(size_t)R * b + i];
  } else if (p < off.b3a) {
    const int r = p - off.W3a, row = r % (2 * R), j = r / (2 * R), aa = row / R, i = row - aa * R;
#pragma unroll 30
    for (int b = 0; b < k; ++b) s += duel_dadv(g[(size_t)R * b + i], a.rb_action[a.idx[b]], aa) * a.H2[(size_t)DUEL_U2 * b + QH2 + j];
  } else {
    const int row = p - off.b3a, aa = row / R, i = row - aa * R;
#pragma unroll 30
    for (int b = 0; b < k; ++b) s += duel_dadv(g[(size_t)R * b + i], a.rb_action[a.idx[b]], aa);
  }
  a.grads[p] = (float)s;
}
// dqn_adam_kernel over ten arrays, one β-power pair each; on a categorical handle it first does what needs the whole batch, as dqn_c51_adam_kernel
__global__ void __launch_bounds__(1024) dqn_duel_adam_kernel(DQNDev a) {
  if (!a.ctl->train_pending) return;
  if (a.c51.on) dqn_c51_batch_tail(a);
  const DuelOff off = duel_off(a.duel.R);
  dqn_adam_step(a, a.duel.P, DUEL_ARRAYS, [&](int p) { return duel_array_of(off, p); });
}

// ------------------------------------------------------------------------------------------------------
// Noisy linear layers (crl_dqn_noisy_create; dqn_noisy.hpp). a.q / a.t are the effective images of the current generation, so the first nine launches
// of the cycle, the collect kernels among them, are the twin's with nothing changed. The Adam slot is dqn_noisy_adam_kernel, one kernel for all heads:
// dqn_noisy_adam_step with the head's array table and layer table. Evaluation, crl_dqn_q_values, crl_dqn_c51_probs and crl_dqn_dueling_streams get the
// mu half (noisy.pq, the twin's layout) as their image: the noise is off there. The images of the next generation are formed by an eleventh launch,
// dqn_noisy_materialise_kernel, on every CU: in the Adam launch's one block they measured slower, so a noisy cycle is eleven launches.
// ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ NoisyTable dqn_noisy_table(const DQNDev& a) {
  return noisy_table(a.duel.on != 0, a.duel.R, a.c51.on ? 2 * a.c51.N : QA);
}
__global__ void __launch_bounds__(1024) dqn_noisy_adam_kernel(DQNDev a) {
  if (!a.ctl->train_pending) return;
  __shared__ float xs[(CRL_NOISY_SPLIT_TAIL ? 1 : 2) * NOISY_MAX_XI];   // generation u's online table; the one-block experiment build adds the next generation's two
  if (a.c51.on) dqn_c51_batch_tail(a);   // as dqn_c51_adam_kernel / dqn_duel_adam_kernel: what needs the whole batch
  const NoisyTable tab = dqn_noisy_table(a);
  if (a.duel.on) {
    const DuelOff off = duel_off(a.duel.R);
    dqn_noisy_adam_step(a, DUEL_ARRAYS, [&](int p) { return duel_array_of(off, p); }, tab, xs);
  } else {
    const int ob3 = tab.l[2].ob;
    dqn_noisy_adam_step(a, 6, [=](int p) { return dqn_array_of(p, ob3); }, tab, xs);
  }
}
// create, crl_dqn_write_params and crl_dqn_init_params: both images at the current generation (n_updates) from mu and sigma
__global__ void __launch_bounds__(256) dqn_noisy_materialise_kernel(DQNDev a) {
  __shared__ float xs[2 * NOISY_MAX_XI];
  dqn_noisy_materialise(a, dqn_noisy_table(a), (uint64_t)a.ctl->n_updates, xs);
}
// crl_dqn_noisy_noise: the xi table of any generation and either net, by the function the Adam launch builds its tables with; one block
__global__ void __launch_bounds__(256) dqn_noisy_noise_kernel(DQNDev a, uint64_t gen, uint32_t stream, float* out) {
  noisy_build_xi(out, dqn_noisy_table(a).n_xi, a.cfg.seed, gen, stream);
}

// crl_dqn_q_values, crl_dqn_c51_probs and crl_dqn_dueling_streams on a dueling handle: the block's forward, then whichever outputs are asked for.
// out_q (2, n); out_p (N, 2, n); out_v (R, n); out_a (R, 2, n), i fastest
__global__ void __launch_bounds__(DQN_OBS_BLOCK) dqn_duel_q_kernel(const float* __restrict__ q, DuelDev du, C51Dev c, const double* __restrict__ obs, int n,
                                                         double* __restrict__ out_q, double* __restrict__ out_p, double* __restrict__ out_v,
                                                         double* __restrict__ out_a) {
#pragma clang fp contract(off)
  __shared__ double h1s[DUEL_H1], h2s[DUEL_U2], raw[3 * DUEL_MAX_R], ls[2 * DUEL_MAX_R], qs[QA];
  const int b = blockIdx.x, tid = threadIdx.x, R = du.R;
  if (b >= n) return;
  duel_block_forward(q, duel_off(R), R, obs + (size_t)QD * b, h1s, h2s, raw, ls);
  if (out_v && tid < R) out_v[(size_t)R * b + tid] = raw[tid];
  if (out_a) for (int r = tid; r < 2 * R; r += DQN_OBS_BLOCK) out_a[(size_t)2 * R * b + r] = raw[R + r];
  if (c.on) {
    c51_block_q(ls, qs, c, out_p ? out_p + (size_t)2 * R * b : nullptr);
    if (out_q && tid < QA) out_q[(size_t)QA * b + tid] = qs[tid];
  } else if (out_q && tid < QA) out_q[(size_t)QA * b + tid] = ls[tid];
}

// dqn_c51_eval_kernel with the dueling heads: one wave per env, ONE staging barrier, the net (up to 149.0 KB) and the waves' strips in dynamic LDS.
// The 168 hidden units are three per lane (lane, lane + 64, lane + 128: three chains side by side); lane i < R forms V_i, A_{0,i} and A_{1,i} side by
// side and combines them, then on a categorical handle the two softmaxes and expectations run wave-wide. With R = 1 every lane forms row 0 alike.
__global__ void __launch_bounds__(64 * DUEL_EVAL_WAVES) dqn_duel_eval_kernel(const float* __restrict__ q, DuelDev du, C51Dev c, int max_steps, double gamma,
                                                                             ValueEvalArgs ev) {
#pragma clang fp contract(off)
  DuelEvalWaveLds* const wl = reinterpret_cast<DuelEvalWaveLds*>(c51_smem);
  float* const wq = reinterpret_cast<float*>(c51_smem + sizeof(DuelEvalWaveLds) * DUEL_EVAL_WAVES);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, env = blockIdx.x * DUEL_EVAL_WAVES + w, R = du.R;
  const DuelOff o = duel_off(R);
  for (int p = threadIdx.x; p < du.P; p += 64 * DUEL_EVAL_WAVES) wq[p] = q[p];
  __syncthreads();                       // the only block barrier of the kernel
  if (env >= ev.n) return;
  double* const h1w = wl[w].h1;
  double* const h2w = wl[w].h2;
  const double delta = c.on ? c51_delta(c.v_min, c.v_max, R) : 0.0;
  // the lane's three units of the two-stream layer: lane is a value unit, lane + 64 one of either stream, lane + 128 an advantage unit (lanes 0..39)
  const int ua = lane, ub = lane + 64, uc = lane + 128 < DUEL_U2 ? lane + 128 : lane;
  const auto wof = [&](int u) { return u >= QH2 ? o.W2a + u - QH2 : o.W2v + u; };
  const auto bof = [&](int u) { return u >= QH2 ? o.b2a + u - QH2 : o.b2v + u; };
  const int wa = wof(ua), wb = wof(ub), wc = wof(uc), ba = bof(ua), bb = bof(ub), bc = bof(uc);
  const int r0 = lane < R ? lane : 0;    // a lane past R repeats row 0; on a categorical handle its results are masked by the wave functions
  dqn_eval_episodes(ev, env, lane, max_steps, gamma, [&](const double* s, double& q0, double& q1) {
#pragma clang fp contract(off)
    eval_layer1_pair(wq, o.W1, o.b1, s, h1w, lane);
    wave_lds_fence();
    {
      double acc = 0.0, acc2 = 0.0, acc3 = 0.0;
#pragma unroll 8
      for (int kk = 0; kk < QH1; ++kk) {
        const double h = h1w[kk];
        acc += (double)wq[wa + QH2 * kk] * h;
        acc2 += (double)wq[wb + QH2 * kk] * h;
        acc3 += (double)wq[wc + QH2 * kk] * h;
      }
      acc += (double)wq[ba];
      acc2 += (double)wq[bb];
      acc3 += (double)wq[bc];
      h2w[ua] = acc > 0.0 ? acc : 0.0;
      h2w[ub] = acc2 > 0.0 ? acc2 : 0.0;
      if (lane + 128 < DUEL_U2) h2w[lane + 128] = acc3 > 0.0 ? acc3 : 0.0;
    }
    wave_lds_fence();
    double av = 0.0, a0 = 0.0, a1 = 0.0;
#pragma unroll 4
    for (int kk = 0; kk < QH2; ++kk) {
      const double hv = h2w[kk], ha = h2w[QH2 + kk];
      av += (double)wq[o.W3v + r0 + R * kk] * hv;
      a0 += (double)wq[o.W3a + r0 + 2 * R * kk] * ha;
      a1 += (double)wq[o.W3a + R + r0 + 2 * R * kk] * ha;
    }
    duel_combine(av + (double)wq[o.b3v + r0], a0 + (double)wq[o.b3a + r0], a1 + (double)wq[o.b3a + R + r0], q0, q1);
    if (c.on) {                          // q0, q1 are the logits of atom `lane`
      double p0, p1, lp;
      c51_softmax(q0, R, lane, p0, lp);
      const double e0 = c51_expect(p0, c.v_min, delta, lane);
      c51_softmax(q1, R, lane, p1, lp);
      q1 = c51_expect(p1, c.v_min, delta, lane);
      q0 = e0;
    }
  });
}

}  // namespace crl

struct crl_dqn {
  crl_dqn_config cfg;
  int device = 0;
  bool params_set = false;   // dqn.jl:39-40 has happened: q_net was uploaded or crl_dqn_init_params ran (a fresh handle holds zeros)
  hipStream_t stream = nullptr;
  crl::DQNDev d;
  void* stage = nullptr; size_t stage_bytes = 0;
  crl::ValueEvalScratch eval;   // crl_dqn_evaluate
  hipGraphExec_t cycle_exec = nullptr; bool graph_failed = false;   // CRL_DQN_GRAPH=1 replays the cycle as a hipGraph
  bool per = false;                                                 // made by crl_dqn_per_create
  double* probe_tree = nullptr; int32_t* probe_idx = nullptr; double* probe_w = nullptr;   // crl_dqn_per_probe's scratch
  bool tgt = false;                                                 // made by crl_dqn_create_with
  void* walk_scratch = nullptr;                                     // crl_dqn_nstep_probe's scratch
  bool c51 = false;                                                 // made by crl_dqn_c51_create
  size_t P = (size_t)crl::QP;                                       // the handle's parameter count: 10934, 10764 + 85·2N on a C51 handle, 20928 + 255·R on a dueling one
  void* proj_scratch = nullptr;                                     // crl_dqn_c51_project_probe's scratch
  bool duel = false;                                                // made by crl_dqn_dueling_create: P = 20928 + 255·R, R = 1 or n_atoms
  bool noisy = false;                                               // made by crl_dqn_noisy_create: P is still the twin's count = the images' length
  size_t n_params = (size_t)crl::QP;                                // what crl_dqn_param_count reports and write / read take: P, or 2P (mu, sigma) on a noisy handle
  double sigma0 = 0.5;                                              // crl_dqn_init_params on a noisy handle
  float* xi_scratch = nullptr;                                      // crl_dqn_noisy_noise's table, NOISY_MAX_XI floats
  // the image the noise-free calls read (crl_dqn_q_values, crl_dqn_c51_probs, crl_dqn_dueling_streams, crl_dqn_evaluate): q_net, or its mu half
  const float* greedy_image() const { return noisy ? d.noisy.pq : d.q; }
};

using namespace crl;

#define DQN_GUARD(h)                                          \
  if (!(h)) { set_error("null crl_dqn handle"); return 1; }   \
  CRL_HIP_CHECK(hipSetDevice((h)->device));

template <typename T>
static int qalloc(T** p, size_t n) {
  CRL_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(p), n * sizeof(T)));
  CRL_HIP_CHECK(hipMemset(*p, 0, n * sizeof(T)));
  return 0;
}

// dynamic LDS of the collect and the evaluation launch of a categorical / a dueling handle with P parameters
static size_t c51_collect_lds(int P) { return C51_COLLECT_LDS + (size_t)P * 4; }
static size_t c51_eval_lds(int P) { return sizeof(C51EvalWaveLds) * DQN_EVAL_WAVES + (size_t)P * 4; }
static size_t duel_collect_lds(int P) { return DUEL_COLLECT_LDS + (size_t)P * 4; }
static size_t duel_eval_lds(int P) { return sizeof(DuelEvalWaveLds) * DUEL_EVAL_WAVES + (size_t)P * 4; }
// The attribute belongs to the kernel, not to the handle, so callers set it to what the largest head needs: handles of different sizes live side by side.
template <typename K>
static bool set_dyn_lds(K* kernel, size_t bytes) {
  return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) == hipSuccess;
}

// The ten launches of a cycle (eleven on a noisy handle), each slot named once with the kernel the handle's head puts there. The trunk's kernels (fwd1, fwd2, bwd1) are shared
// where the arrays sit at the plain offsets; a categorical or a dueling handle always carries target options, so tgt.on holds for them.
using DQNKernel = void (*)(DQNDev);
// the sampling launch and the TD launch come as a uniform-replay and a PER instantiation
static DQNKernel by_replay(const DQNDev& d, DQNKernel uniform, DQNKernel per) { return d.per.on ? per : uniform; }
static void enqueue_cycle(hipStream_t st, const DQNDev& d, int k) {
  const bool duel = d.duel.on, c51 = d.c51.on, tgt = d.tgt.on;
  const int nets = d.nets, U2 = duel ? DUEL_U2 : QH2, P = duel ? d.duel.P : c51 ? d.c51.P : QP;
  const int rows3 = duel ? d.duel.R : c51 ? 2 * d.c51.N : QA;   // threads per sample and pass of the fwd3 slot
  const auto launch = [&](DQNKernel kernel, int threads, int block, size_t lds = 0) {   // ⌈threads / block⌉ blocks
    hipLaunchKernelGGL(kernel, dim3((threads + block - 1) / block), dim3(block), lds, st, d);
  };
  launch(duel ? dqn_duel_collect_kernel : c51 ? dqn_c51_collect_kernel : dqn_collect_kernel, DQN_OBS_BLOCK, DQN_OBS_BLOCK,
         duel ? duel_collect_lds(P) : c51 ? c51_collect_lds(P) : 0);
  launch(tgt ? by_replay(d, dqn_tgt_sample_kernel<false>, dqn_tgt_sample_kernel<true>) : by_replay(d, dqn_sample_kernel, dqn_per_sample_kernel), 1024, 1024);
  launch(dqn_fwd1_kernel, nets * QH1 * k, 256);
  launch(duel ? dqn_duel_fwd2_kernel : dqn_fwd2_kernel, nets * U2 * k, 256);
  launch(duel ? dqn_duel_fwd3_kernel : c51 ? dqn_c51_fwd3_kernel : dqn_fwd3_kernel, nets * rows3 * k, 256);
  if (c51) launch(by_replay(d, dqn_c51_td_kernel<false>, dqn_c51_td_kernel<true>), 64 * k, 64 * C51_TD_WAVES);   // one wave per sample
  else launch(tgt ? by_replay(d, dqn_td_kernel<true, false>, dqn_td_kernel<true, true>) : by_replay(d, dqn_td_kernel<false, false>, dqn_td_kernel<false, true>),
              1024, 1024);
  launch(duel ? dqn_duel_bwd2_kernel : c51 ? dqn_c51_bwd2_kernel : dqn_bwd2_kernel, U2 * k, 256);
  launch(duel ? dqn_duel_bwd1_kernel : dqn_bwd1_kernel, QH1 * k, 256);
  launch(duel ? dqn_duel_wgrad_kernel : c51 ? dqn_c51_wgrad_kernel : dqn_wgrad_kernel, P, 64);
  launch(d.noisy.on ? dqn_noisy_adam_kernel : duel ? dqn_duel_adam_kernel : c51 ? dqn_c51_adam_kernel : dqn_adam_kernel, 1024, 1024);
  // a noisy handle's eleventh launch: both images at generation n_updates on every CU (idempotent, so a cycle without an update rewrites the same
  // bits); in dqn_noisy_adam_kernel's one block the same work measured 12 us (plain net) to 53 us (dueling + C51) slower per cycle: DESIGN.md §3l
  if (CRL_NOISY_SPLIT_TAIL && d.noisy.on) launch(dqn_noisy_materialise_kernel, P, 256);
}

// crl_dqn_create, crl_dqn_per_create, crl_dqn_create_with, crl_dqn_c51_create, crl_dqn_dueling_create and crl_dqn_noisy_create: one body; `per` is null for uniform replay,
// `tgt` for the 1-step max target of dqn.jl, `c51` for the scalar head; `duel` splits layers 2 and 3 into a value and an advantage stream
static int32_t dqn_create(const crl_dqn_config* cfg, const crl_dqn_per_options* per, const crl_dqn_target_options* tgt, int32_t device, crl_dqn** out,
                          const crl_dqn_c51_options* c51 = nullptr, bool duel = false, const crl_dqn_noisy_options* noisy = nullptr) {
  if (cfg->batch_size < 1 || cfg->batch_size > DQN_MAX_BATCH) { set_error("crl_dqn_create: batch_size must be in 1..1024"); return 1; }
  if (cfg->buffer_size < cfg->batch_size || cfg->buffer_size > DQN_MAX_CAP) { set_error("crl_dqn_create: buffer_size must be in batch_size..65536"); return 1; }
  if (cfg->min_buff_size < cfg->batch_size) {
    set_error("crl_dqn_create: min_buff_size must be >= batch_size (Buffer.sample asserts n <= rb.size, replay_buffer.jl:41)"); return 1;
  }
  if (cfg->train_freq < 1 || cfg->target_net_freq < 1 || cfg->log_frequency < 1 || cfg->max_steps < 1 || cfg->total_timesteps < 0 ||
      !(cfg->epsilon_duration > 0.0)) { set_error("crl_dqn_create: bad frequencies / sizes"); return 1; }
  int ndev = 0;
  CRL_HIP_CHECK(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) { set_error("crl_dqn_create: no such HIP device (no GPU → no CPU fallback)"); return 1; }
  CRL_HIP_CHECK(hipSetDevice(device));
  crl_dqn* h = new (std::nothrow) crl_dqn();
  if (!h) { set_error("out of host memory"); return 1; }
  h->cfg = *cfg; h->device = device;
  { const char* e = getenv("CRL_DQN_GRAPH"); h->graph_failed = !(e && atoi(e) != 0); }   // hipGraph replay is opt-in: measured no faster
  memset(&h->d, 0, sizeof(h->d));
  h->d.cfg = *cfg;
  hipError_t se = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
  if (se != hipSuccess) { set_error(std::string("hipStreamCreate: ") + hipGetErrorString(se)); delete h; return 1; }
  const size_t cap = (size_t)cfg->buffer_size, k = (size_t)cfg->batch_size;
  DQNDev& d = h->d;
  int rc = 0;
  const size_t NP = duel ? (size_t)duel_param_count(c51 ? c51->n_atoms : 1) : c51 ? (size_t)QoW3 + 85 * 2 * (size_t)c51->n_atoms : (size_t)QP;
  const size_t U2 = duel ? DUEL_U2 : QH2, NARR = duel ? DUEL_ARRAYS : 6;   // hidden units of layer 2 per sample; arrays Adam keeps a β-power pair for
  const size_t NZ = noisy ? 2 : 1;   // a noisy handle keeps Adam state for mu and sigma: 2P entries, twice the arrays
  h->P = NP; h->n_params = NZ * NP;
  rc |= qalloc(&d.q, NP); rc |= qalloc(&d.t, NP); rc |= qalloc(&d.grads, NP); rc |= qalloc(&d.m, NZ * NP); rc |= qalloc(&d.v, NZ * NP);
  rc |= qalloc(&d.betap, 2 * NZ * NARR); rc |= qalloc(&d.ctl, 1); rc |= qalloc(&d.eps, DQN_MAX_EPS); rc |= qalloc(&d.losses, DQN_MAX_LOSSES);
  rc |= qalloc(&d.rb_state, cap * QD); rc |= qalloc(&d.rb_next, cap * QD); rc |= qalloc(&d.rb_reward, cap);
  rc |= qalloc(&d.rb_action, cap); rc |= qalloc(&d.rb_terminal, cap);
  const size_t nets = tgt && tgt->double_q ? 3 : 2;
  d.nets = (int32_t)nets;
  rc |= qalloc(&d.H1, nets * QH1 * k); rc |= qalloc(&d.H2, nets * U2 * k); rc |= qalloc(&d.Q, nets * QA * k);
  rc |= qalloc(&d.dz, k); rc |= qalloc(&d.sq, k); rc |= qalloc(&d.d2, U2 * k); rc |= qalloc(&d.d1, QH1 * k); rc |= qalloc(&d.idx, k);
  d.boot = d.idx;
  if (tgt) {
    h->tgt = true;
    TgtDev& t = d.tgt;
    t.on = 1; t.n_step = tgt->n_step; t.double_q = tgt->double_q;
    rc |= qalloc(&t.last, k); rc |= qalloc(&t.m, k); rc |= qalloc(&t.astar, k); rc |= qalloc(&t.nret, k); rc |= qalloc(&t.ndisc, k); rc |= qalloc(&t.td, k);
    d.boot = t.last;
  }
  if (per) {
    h->per = true;
    PerDev& p = d.per;
    p.on = 1; p.C = per_tree_leaves(cfg->buffer_size);
    p.alpha = per->alpha; p.beta_start = per->beta_start; p.beta_end = per->beta_end; p.beta_duration = per->beta_duration; p.eps = per->eps;
    rc |= qalloc(&p.tree, 2 * (size_t)p.C); rc |= qalloc(&p.ctl, 1); rc |= qalloc(&p.w, k); rc |= qalloc(&p.abs_td, k);
    if (!rc) {
      PerCtl pc;
      memset(&pc, 0, sizeof(pc));
      pc.beta = per->beta_start; pc.max_leaf = 1.0f;
      if (hipMemcpy(p.ctl, &pc, sizeof(pc), hipMemcpyHostToDevice) != hipSuccess) { set_error("hipMemcpy of the PER control block failed"); rc = 1; }
    }
  }
  if (c51) {
    h->c51 = true;
    C51Dev& c = d.c51;
    const size_t N = (size_t)c51->n_atoms;
    c.on = 1; c.N = c51->n_atoms; c.P = (int32_t)NP; c.v_min = c51->v_min; c.v_max = c51->v_max;
    rc |= qalloc(&c.L, nets * 2 * N * k); rc |= qalloc(&c.dl, N * k); rc |= qalloc(&c.proj, N * k); rc |= qalloc(&c.sloss, k);
    // the net in LDS passes the 64 KB a launch gets without asking at N >= 36; the CU has 160 KB. Set for the largest head (set_dyn_lds).
    constexpr int PMAX = QoW3 + 85 * 2 * C51_MAX_ATOMS;
    if (!rc && !(set_dyn_lds(dqn_c51_collect_kernel, c51_collect_lds(PMAX)) && set_dyn_lds(dqn_c51_eval_kernel, c51_eval_lds(PMAX)))) {
      set_error("crl_dqn_c51_create: the device refused the dynamic LDS size of the collect / evaluation kernels"); rc = 1;
    }
  }
  if (duel) {
    h->duel = true;
    d.duel.on = 1; d.duel.R = c51 ? c51->n_atoms : 1; d.duel.P = (int32_t)NP;
    // both kernels keep the whole net in LDS, past the 64 KB a launch gets without asking at every R; set for the largest head, as above
    constexpr int PMAX = duel_param_count(DUEL_MAX_R);
    if (!rc && !(set_dyn_lds(dqn_duel_collect_kernel, duel_collect_lds(PMAX)) && set_dyn_lds(dqn_duel_eval_kernel, duel_eval_lds(PMAX)))) {
      set_error("crl_dqn_dueling_create: the device refused the dynamic LDS size of the collect / evaluation kernels"); rc = 1;
    }
  }
  if (noisy) {
    h->noisy = true; h->sigma0 = noisy->sigma0;
    d.noisy.on = 1; d.noisy.P = (int32_t)NP;
    rc |= qalloc(&d.noisy.pq, 2 * NP); rc |= qalloc(&d.noisy.pt, 2 * NP); rc |= qalloc(&h->xi_scratch, (size_t)NOISY_MAX_XI);
  }
  if (rc) { crl_dqn_destroy(h); return 1; }
  double bp[2 * 2 * DUEL_ARRAYS];
  for (size_t i = 0; i < NZ * NARR; ++i) { bp[2 * i] = 0.9; bp[2 * i + 1] = 0.999; }
  CRL_HIP_CHECK(hipMemcpy(d.betap, bp, 2 * NZ * NARR * sizeof(double), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(dqn_init_kernel, dim3(1), dim3(1), 0, h->stream, d);
  CRL_HIP_CHECK(hipStreamSynchronize(h->stream));
  *out = h;
  return 0;
}

#define DQN_TGT_GUARD(h, name)                                                                                           \
  DQN_GUARD(h);                                                                                                          \
  if (!(h)->tgt) { set_error(name ": the handle was not made by crl_dqn_create_with (only such a handle forms n-step / double-Q targets)"); return 1; }

static int per_options_check(const char* who, const crl_dqn_per_options* per) {
  const std::string w(who);
  if (!(per->alpha >= 0.0 && per->alpha <= 1.0)) { set_error(w + ": alpha must be in 0..1"); return 1; }
  if (!(per->beta_start >= 0.0 && per->beta_start <= 1.0)) { set_error(w + ": beta_start must be in 0..1"); return 1; }
  if (!(per->beta_end >= 0.0 && per->beta_end <= 1.0)) { set_error(w + ": beta_end must be in 0..1"); return 1; }
  if (!(per->beta_duration > 0.0) || !(per->beta_duration < 1e300)) { set_error(w + ": beta_duration must be > 0 and finite"); return 1; }
  if (!(per->eps >= 1e-6 && per->eps <= 1.0)) { set_error(w + ": eps must be in 1e-6..1"); return 1; }
  return 0;
}

#define DQN_NOISY_GUARD(h, name)                                                                                         \
  DQN_GUARD(h);                                                                                                          \
  if (!(h)->noisy) { set_error(name ": the handle's layers are not noisy; crl_dqn_noisy_create makes a NoisyNet handle"); return 1; }

// both images of a noisy handle at its current generation, from the mu and sigma it holds
static int noisy_materialise(crl_dqn* h) {
  hipLaunchKernelGGL(dqn_noisy_materialise_kernel, dim3((unsigned)((h->P + 255) / 256)), dim3(256), 0, h->stream, h->d);
  CRL_HIP_CHECK(hipGetLastError());
  return 0;
}

// the categorical head's options and the target options, checked once for every creator that takes them; `who` names the creator in the message
static int c51_options_check(const char* who, const crl_dqn_c51_options* c51) {
  const std::string w(who);
  if (c51->n_atoms < 2 || c51->n_atoms > C51_MAX_ATOMS) { set_error(w + ": n_atoms must be in 2..64"); return 1; }
  if (!(c51->v_min > -1e300 && c51->v_min < 1e300)) { set_error(w + ": v_min must be finite"); return 1; }
  if (!(c51->v_max > -1e300 && c51->v_max < 1e300)) { set_error(w + ": v_max must be finite"); return 1; }
  if (!(c51->v_min < c51->v_max)) { set_error(w + ": v_min must be < v_max"); return 1; }
  return 0;
}
// t = *tgt, or {1, 0} (dqn.jl's 1-step max) for NULL
static int target_options_check(const char* who, const crl_dqn_target_options* tgt, crl_dqn_target_options& t) {
  const std::string w(who);
  t = {1, 0};
  if (tgt) t = *tgt;
  if (t.n_step < 1 || t.n_step > TGT_MAX_N_STEP) { set_error(w + ": n_step must be in 1..16"); return 1; }
  if (t.double_q != 0 && t.double_q != 1) { set_error(w + ": double_q must be 0 or 1"); return 1; }
  return 0;
}

#define DQN_C51_GUARD(h, name)                                                                                           \
  DQN_GUARD(h);                                                                                                          \
  if (!(h)->c51) { set_error(name ": the handle has a scalar head; crl_dqn_c51_create makes a categorical (C51) handle"); return 1; }

#define DQN_PER_GUARD(h, name)                                                                                           \
  DQN_GUARD(h);                                                                                                          \
  if (!(h)->per) { set_error(name ": the handle was made by crl_dqn_create (uniform replay); crl_dqn_per_create makes a PER handle"); return 1; }

extern "C" {

int32_t crl_dqn_create(const crl_dqn_config* cfg, int32_t device, crl_dqn** out) {
  if (!cfg || !out) { set_error("crl_dqn_create: null argument"); return 1; }
  *out = nullptr;
  return dqn_create(cfg, nullptr, nullptr, device, out);
}

int32_t crl_dqn_per_create(const crl_dqn_config* cfg, const crl_dqn_per_options* per, int32_t device, crl_dqn** out) {
  if (!cfg || !per || !out) { set_error("crl_dqn_per_create: null argument"); return 1; }
  *out = nullptr;
  if (per_options_check("crl_dqn_per_create", per)) return 1;
  return dqn_create(cfg, per, nullptr, device, out);
}

int32_t crl_dqn_create_with(const crl_dqn_config* cfg, const crl_dqn_per_options* per, const crl_dqn_target_options* tgt, int32_t device, crl_dqn** out) {
  if (!cfg || !out) { set_error("crl_dqn_create_with: null argument (cfg and out are required)"); return 1; }
  *out = nullptr;
  if (per && per_options_check("crl_dqn_create_with", per)) return 1;
  crl_dqn_target_options t;
  if (target_options_check("crl_dqn_create_with", tgt, t)) return 1;
  return dqn_create(cfg, per, &t, device, out);
}

int32_t crl_dqn_c51_create(const crl_dqn_config* cfg, const crl_dqn_c51_options* c51, const crl_dqn_per_options* per, const crl_dqn_target_options* tgt,
                           int32_t device, crl_dqn** out) {
  if (!cfg || !c51 || !out) { set_error("crl_dqn_c51_create: null argument (cfg, c51 and out are required)"); return 1; }
  *out = nullptr;
  if (c51_options_check("crl_dqn_c51_create", c51)) return 1;
  if (per && per_options_check("crl_dqn_c51_create", per)) return 1;
  crl_dqn_target_options t;
  if (target_options_check("crl_dqn_c51_create", tgt, t)) return 1;
  return dqn_create(cfg, per, &t, device, out, c51);
}

int32_t crl_dqn_dueling_create(const crl_dqn_config* cfg, const crl_dqn_c51_options* c51, const crl_dqn_per_options* per, const crl_dqn_target_options* tgt,
                               int32_t device, crl_dqn** out) {
  if (!cfg || !out) { set_error("crl_dqn_dueling_create: null argument (cfg and out are required)"); return 1; }
  *out = nullptr;
  if (c51 && c51_options_check("crl_dqn_dueling_create", c51)) return 1;
  if (per && per_options_check("crl_dqn_dueling_create", per)) return 1;
  crl_dqn_target_options t;
  if (target_options_check("crl_dqn_dueling_create", tgt, t)) return 1;
  return dqn_create(cfg, per, &t, device, out, c51, /*duel=*/true);
}

int32_t crl_dqn_noisy_create(const crl_dqn_config* cfg, const crl_dqn_noisy_options* noisy, int32_t dueling, const crl_dqn_c51_options* c51,
                             const crl_dqn_per_options* per, const crl_dqn_target_options* tgt, int32_t device, crl_dqn** out) {
  if (!cfg || !noisy || !out) { set_error("crl_dqn_noisy_create: null argument (cfg, noisy and out are required)"); return 1; }
  *out = nullptr;
  if (!(noisy->sigma0 >= 0.0 && noisy->sigma0 <= 10.0)) { set_error("crl_dqn_noisy_create: sigma0 must be in 0..10"); return 1; }
  if (dueling != 0 && dueling != 1) { set_error("crl_dqn_noisy_create: dueling must be 0 or 1"); return 1; }
  if (c51 && c51_options_check("crl_dqn_noisy_create", c51)) return 1;
  if (per && per_options_check("crl_dqn_noisy_create", per)) return 1;
  crl_dqn_target_options t;
  if (target_options_check("crl_dqn_noisy_create", tgt, t)) return 1;
  // the twin's kind: a categorical or a dueling handle always carries target options; the plain one only when they were given
  if (dqn_create(cfg, per, (tgt || c51 || dueling) ? &t : nullptr, device, out, c51, dueling != 0, noisy)) return 1;
  if (noisy_materialise(*out) || hipStreamSynchronize((*out)->stream) != hipSuccess) {
    set_error("crl_dqn_noisy_create: the materialise launch failed"); crl_dqn_destroy(*out); *out = nullptr; return 1;
  }
  return 0;
}

int32_t crl_dqn_noisy_weights(crl_dqn* h, int32_t net, float* out, size_t n) {
  DQN_NOISY_GUARD(h, "crl_dqn_noisy_weights");
  if (net != 0 && net != 1) { set_error("crl_dqn_noisy_weights: net must be 0 (q_net) or 1 (target_net)"); return 1; }
  if (!out || n != h->P) { set_error("crl_dqn_noisy_weights: expected " + std::to_string(h->P) + " floats"); return 1; }
  CRL_HIP_CHECK(hipMemcpyAsync(out, net ? h->d.t : h->d.q, n * 4, hipMemcpyDeviceToHost, h->stream));
  CRL_HIP_CHECK(hipStreamSynchronize(h->stream));
  return 0;
}

int32_t crl_dqn_noisy_noise_count(crl_dqn* h, size_t* n) {
  DQN_NOISY_GUARD(h, "crl_dqn_noisy_noise_count");
  if (!n) { set_error("crl_dqn_noisy_noise_count: null argument"); return 1; }
  *n = (size_t)noisy_table(h->duel, h->d.duel.R, h->c51 ? 2 * h->d.c51.N : QA).n_xi;
  return 0;
}

int32_t crl_dqn_noisy_noise(crl_dqn* h, uint64_t gen, int32_t net, float* xi, size_t n) {
  DQN_NOISY_GUARD(h, "crl_dqn_noisy_noise");
  if (net != 0 && net != 1) { set_error("crl_dqn_noisy_noise: net must be 0 (q_net) or 1 (target_net)"); return 1; }
  const size_t want = (size_t)noisy_table(h->duel, h->d.duel.R, h->c51 ? 2 * h->d.c51.N : QA).n_xi;
  if (!xi || n != want) { set_error("crl_dqn_noisy_noise: expected " + std::to_string(want) + " floats"); return 1; }
  hipLaunchKernelGGL(dqn_noisy_noise_kernel, dim3(1), dim3(256), 0, h->stream, h->d, gen, net ? S_NOISY_T : S_NOISY_Q, h->xi_scratch);
  CRL_HIP_CHECK(hipGetLastError());
  CRL_HIP_CHECK(hipMemcpyAsync(xi, h->xi_scratch, n * 4, hipMemcpyDeviceToHost, h->stream));
  CRL_HIP_CHECK(hipStreamSynchronize(h->stream));
  return 0;
}

// the stage buffer of the forward-only calls, grown on demand
static int dqn_stage(crl_dqn* h, size_t need) {
  if (h->stage_bytes < need) {
    if (h->stage) CRL_HIP_CHECK(hipFree(h->stage));
    h->stage = nullptr; h->stage_bytes = 0;
    CRL_HIP_CHECK(hipMalloc(&h->stage, need));
    h->stage_bytes = need;
  }
  return 0;
}

int32_t crl_dqn_dueling_streams(crl_dqn* h, const double* obs, int32_t n, double* value, double* adv) {
  DQN_GUARD(h);
  if (!h->duel) { set_error("crl_dqn_dueling_streams: the handle has one head; crl_dqn_dueling_create makes a dueling handle"); return 1; }
  if (!h->params_set) { set_error("crl_dqn_dueling_streams: parameters not set — crl_dqn_write_params or crl_dqn_init_params first"); return 1; }
  if (n < 0 || (n > 0 && !obs)) { set_error("crl_dqn_dueling_streams: bad arguments"); return 1; }
  if (n == 0) return 0;
  const size_t N = (size_t)n, R = (size_t)h->d.duel.R;
  if (dqn_stage(h, N * (QD + 3 * R) * 8)) return 1;
  double* so = static_cast<double*>(h->stage);
  double *sv = so + N * QD, *sa = sv + N * R;
  CRL_HIP_CHECK(hipMemcpyAsync(so, obs, N * QD * 8, hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(dqn_duel_q_kernel, dim3(n), dim3(DQN_OBS_BLOCK), 0, h->stream, h->greedy_image(), h->d.duel, h->d.c51, (const double*)so, n, (double*)nullptr,
                     (double*)nullptr, sv, sa);
  CRL_HIP_CHECK(hipGetLastError());
  if (value) CRL_HIP_CHECK(hipMemcpyAsync(value, sv, N * R * 8, hipMemcpyDeviceToHost, h->stream));
  if (adv) CRL_HIP_CHECK(hipMemcpyAsync(adv, sa, N * 2 * R * 8, hipMemcpyDeviceToHost, h->stream));
  CRL_HIP_CHECK(hipStreamSynchronize(h->stream));
  return 0;
}

int32_t crl_dqn_param_count(crl_dqn* h, size_t* n) {
  DQN_GUARD(h);
  if (!n) { set_error("crl_dqn_param_count: null argument"); return 1; }
  *n = h->n_params;
  return 0;
}

int32_t crl_dqn_c51_probs(crl_dqn* h, const double* obs, int32_t n, double* probs) {
  DQN_C51_GUARD(h, "crl_dqn_c51_probs");
  if (!h->params_set) { set_error("crl_dqn_c51_probs: parameters not set — crl_dqn_write_params or crl_dqn_init_params first"); return 1; }
  if (n < 0 || (n > 0 && (!obs || !probs))) { set_error("crl_dqn_c51_probs: bad arguments"); return 1; }
  if (n == 0) return 0;
  const size_t N = (size_t)n, NA = 2 * (size_t)h->d.c51.N, need = N * (QD + NA) * 8;
  if (dqn_stage(h, need)) return 1;
  double* so = static_cast<double*>(h->stage);
  double* sp = so + N * QD;
  CRL_HIP_CHECK(hipMemcpyAsync(so, obs, N * QD * 8, hipMemcpyHostToDevice, h->stream));
  if (h->duel) hipLaunchKernelGGL(dqn_duel_q_kernel, dim3(n), dim3(DQN_OBS_BLOCK), 0, h->stream, h->greedy_image(), h->d.duel, h->d.c51, (const double*)so, n,
                                  (double*)nullptr, sp, (double*)nullptr, (double*)nullptr);
  else hipLaunchKernelGGL(dqn_c51_q_kernel, dim3(n), dim3(DQN_OBS_BLOCK), 0, h->stream, h->greedy_image(), h->d.c51, (const double*)so, n, (double*)nullptr, sp);
  CRL_HIP_CHECK(hipGetLastError());
  CRL_HIP_CHECK(hipMemcpyAsync(probs, sp, N * NA * 8, hipMemcpyDeviceToHost, h->stream));
  CRL_HIP_CHECK(hipStreamSynchronize(h->stream));
  return 0;
}

int32_t crl_dqn_c51_read(crl_dqn* h, double* proj, double* sample_loss) {
  DQN_C51_GUARD(h, "crl_dqn_c51_read");
  const size_t k = (size_t)h->cfg.batch_size, N = (size_t)h->d.c51.N;
  if (proj) CRL_HIP_CHECK(hipMemcpyAsync(proj, h->d.c51.proj, k * N * 8, hipMemcpyDeviceToHost, h->stream));
  if (sample_loss) CRL_HIP_CHECK(hipMemcpyAsync(sample_loss, h->d.c51.sloss, k * 8, hipMemcpyDeviceToHost, h->stream));
  CRL_HIP_CHECK(hipStreamSynchronize(h->stream));
  return 0;
}

int32_t crl_dqn_c51_project_probe(crl_dqn* h, const double* probs, const double* nret, const double* ndisc, const uint8_t* terminal, int32_t k,
                                  double* proj) {
  DQN_C51_GUARD(h, "crl_dqn_c51_project_probe");
  if (!probs || !nret || !ndisc || !terminal || !proj) { set_error("crl_dqn_c51_project_probe: null argument"); return 1; }
  if (k < 1 || k > DQN_MAX_BATCH) { set_error("crl_dqn_c51_project_probe: k must be in 1..1024"); return 1; }
  // one allocation: probs [1024·64] f64 | proj [1024·64] f64 | nret [1024] f64 | ndisc [1024] f64 | terminal [1024] u8
  constexpr size_t rows = (size_t)DQN_MAX_BATCH * C51_MAX_ATOMS * 8, oP = 0, oM = oP + rows, oR = oM + rows, oD = oR + (size_t)DQN_MAX_BATCH * 8,
                   oT = oD + (size_t)DQN_MAX_BATCH * 8, total = oT + DQN_MAX_BATCH;
  if (!h->proj_scratch) CRL_HIP_CHECK(hipMalloc(&h->proj_scratch, total));
  char* base = static_cast<char*>(h->proj_scratch);
  double *dP = reinterpret_cast<double*>(base + oP), *dM = reinterpret_cast<double*>(base + oM), *dR = reinterpret_cast<double*>(base + oR),
         *dD = reinterpret_cast<double*>(base + oD);
  uint8_t* dT = reinterpret_cast<uint8_t*>(base + oT);
  const C51Dev& c = h->d.c51;
  const size_t K = (size_t)k, N = (size_t)c.N;
  CRL_HIP_CHECK(hipMemcpyAsync(dP, probs, K * N * 8, hipMemcpyHostToDevice, h->stream));
  CRL_HIP_CHECK(hipMemcpyAsync(dR, nret, K * 8, hipMemcpyHostToDevice, h->stream));
  CRL_HIP_CHECK(hipMemcpyAsync(dD, ndisc, K * 8, hipMemcpyHostToDevice, h->stream));
  CRL_HIP_CHECK(hipMemcpyAsync(dT, terminal, K, hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(dqn_c51_project_probe_kernel, dim3(1), dim3(64 * C51_TD_WAVES), 0, h->stream, (const double*)dP, (const double*)dR, (const double*)dD,
                     (const uint8_t*)dT, (int)k, (int)c.N, c.v_min, c.v_max, dM);
  CRL_HIP_CHECK(hipGetLastError());
  CRL_HIP_CHECK(hipMemcpyAsync(proj, dM, K * N * 8, hipMemcpyDeviceToHost, h->stream));
  CRL_HIP_CHECK(hipStreamSynchronize(h->stream));
  return 0;
}

int32_t crl_dqn_target_read(crl_dqn* h, int32_t* last, int32_t* m, double* nret, double* ndisc, int32_t* astar, double* td) {
  DQN_TGT_GUARD(h, "crl_dqn_target_read");
  const TgtDev& t = h->d.tgt;
  const size_t k = (size_t)h->cfg.batch_size;
  if (last) CRL_HIP_CHECK(hipMemcpyAsync(last, t.last, k * 4, hipMemcpyDeviceToHost, h->stream));
  if (m) CRL_HIP_CHECK(hipMemcpyAsync(m, t.m, k * 4, hipMemcpyDeviceToHost, h->stream));
  if (nret) CRL_HIP_CHECK(hipMemcpyAsync(nret, t.nret, k * 8, hipMemcpyDeviceToHost, h->stream));
  if (ndisc) CRL_HIP_CHECK(hipMemcpyAsync(ndisc, t.ndisc, k * 8, hipMemcpyDeviceToHost, h->stream));
  if (astar) CRL_HIP_CHECK(hipMemcpyAsync(astar, t.astar, k * 4, hipMemcpyDeviceToHost, h->stream));
  if (td) CRL_HIP_CHECK(hipMemcpyAsync(td, t.td, k * 8, hipMemcpyDeviceToHost, h->stream));
  CRL_HIP_CHECK(hipStreamSynchronize(h->stream));
  return 0;
}

int32_t crl_dqn_nstep_probe(crl_dqn* h, const double* reward, const uint8_t* terminal, int32_t cap, int32_t ptr, const int32_t* idx, int32_t k,
                            int32_t n_step, double gamma, int32_t* last, int32_t* m, double* nret, double* ndisc) {
  DQN_TGT_GUARD(h, "crl_dqn_nstep_probe");
  if (!reward || !terminal || !idx || !last || !m || !nret || !ndisc) { set_error("crl_dqn_nstep_probe: null argument"); return 1; }
  if (cap < 1 || cap > DQN_MAX_CAP) { set_error("crl_dqn_nstep_probe: cap must be in 1..65536"); return 1; }
  if (k < 1 || k > DQN_MAX_BATCH) { set_error("crl_dqn_nstep_probe: k must be in 1..1024"); return 1; }
  if (ptr < 0 || ptr >= cap) { set_error("crl_dqn_nstep_probe: ptr must be in 0..cap-1"); return 1; }
  if (n_step < 1 || n_step > TGT_MAX_N_STEP) { set_error("crl_dqn_nstep_probe: n_step must be in 1..16"); return 1; }
  for (int32_t j = 0; j < k; ++j)
    if (idx[j] < 0 || idx[j] >= cap) { set_error("crl_dqn_nstep_probe: every idx must be in 0..cap-1"); return 1; }
  // one allocation: reward [65536] f64 | nret [1024] f64 | ndisc [1024] f64 | idx, last, m [1024] i32 each | terminal [65536] u8
  constexpr size_t oR = 0, oN = oR + (size_t)DQN_MAX_CAP * 8, oD = oN + (size_t)DQN_MAX_BATCH * 8, oI = oD + (size_t)DQN_MAX_BATCH * 8,
                   oL = oI + (size_t)DQN_MAX_BATCH * 4, oM = oL + (size_t)DQN_MAX_BATCH * 4, oT = oM + (size_t)DQN_MAX_BATCH * 4, total = oT + DQN_MAX_CAP;
  if (!h->walk_scratch) CRL_HIP_CHECK(hipMalloc(&h->walk_scratch, total));
  char* base = static_cast<char*>(h->walk_scratch);
  double *dR = reinterpret_cast<double*>(base + oR), *dN = reinterpret_cast<double*>(base + oN), *dD = reinterpret_cast<double*>(base + oD);
  int32_t *dI = reinterpret_cast<int32_t*>(base + oI), *dL = reinterpret_cast<int32_t*>(base + oL), *dM = reinterpret_cast<int32_t*>(base + oM);
  uint8_t* dT = reinterpret_cast<uint8_t*>(base + oT);
  CRL_HIP_CHECK(hipMemcpyAsync(dR, reward, (size_t)cap * 8, hipMemcpyHostToDevice, h->stream));
  CRL_HIP_CHECK(hipMemcpyAsync(dT, terminal, (size_t)cap, hipMemcpyHostToDevice, h->stream));
  CRL_HIP_CHECK(hipMemcpyAsync(dI, idx, (size_t)k * 4, hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(dqn_nstep_probe_kernel, dim3(1), dim3(1024), 0, h->stream, (const double*)dR, (const uint8_t*)dT, (int)cap, (int)ptr, (const int32_t*)dI,
                     (int)k, (int)n_step, gamma, dL, dM, dN, dD);
  CRL_HIP_CHECK(hipGetLastError());
  CRL_HIP_CHECK(hipMemcpyAsync(last, dL, (size_t)k * 4, hipMemcpyDeviceToHost, h->stream));
  CRL_HIP_CHECK(hipMemcpyAsync(m, dM, (size_t)k * 4, hipMemcpyDeviceToHost, h->stream));
  CRL_HIP_CHECK(hipMemcpyAsync(nret, dN, (size_t)k * 8, hipMemcpyDeviceToHost, h->stream));
  CRL_HIP_CHECK(hipMemcpyAsync(ndisc, dD, (size_t)k * 8, hipMemcpyDeviceToHost, h->stream));
  CRL_HIP_CHECK(hipStreamSynchronize(h->stream));
  return 0;
}

int32_t crl_dqn_per_status_read(crl_dqn* h, crl_dqn_per_status* out) {
  DQN_PER_GUARD(h, "crl_dqn_per_status_read");
  if (!out) { set_error("crl_dqn_per_status_read: null argument"); return 1; }
  PerCtl pc; double total = 0.0;
  CRL_HIP_CHECK(hipMemcpyAsync(&pc, h->d.per.ctl, sizeof(pc), hipMemcpyDeviceToHost, h->stream));
  CRL_HIP_CHECK(hipMemcpyAsync(&total, h->d.per.tree + 1, sizeof(double), hipMemcpyDeviceToHost, h->stream));
  CRL_HIP_CHECK(hipStreamSynchronize(h->stream));
  out->beta = pc.beta; out->total = total; out->max_leaf = pc.max_leaf; out->tree_leaves = h->d.per.C;
  return 0;
}

int32_t crl_dqn_per_read(crl_dqn* h, float* leaves, double* tree, int32_t* idx, double* weight, double* abs_td) {
  DQN_PER_GUARD(h, "crl_dqn_per_read");
  const PerDev& p = h->d.per;
  const size_t C = (size_t)p.C, cap = (size_t)h->cfg.buffer_size, k = (size_t)h->cfg.batch_size;
  std::vector<double> t;
  if (leaves) {
    t.resize(cap);
    CRL_HIP_CHECK(hipMemcpyAsync(t.data(), p.tree + C, cap * 8, hipMemcpyDeviceToHost, h->stream));
  }
  if (tree) CRL_HIP_CHECK(hipMemcpyAsync(tree, p.tree, 2 * C * 8, hipMemcpyDeviceToHost, h->stream));
  if (idx) CRL_HIP_CHECK(hipMemcpyAsync(idx, h->d.idx, k * 4, hipMemcpyDeviceToHost, h->stream));
  if (weight) CRL_HIP_CHECK(hipMemcpyAsync(weight, p.w, k * 8, hipMemcpyDeviceToHost, h->stream));
  if (abs_td) CRL_HIP_CHECK(hipMemcpyAsync(abs_td, p.abs_td, k * 8, hipMemcpyDeviceToHost, h->stream));
  CRL_HIP_CHECK(hipStreamSynchronize(h->stream));
  if (leaves) for (size_t s = 0; s < cap; ++s) leaves[s] = (float)t[s];   // stored widened: the conversion back is exact
  return 0;
}

int32_t crl_dqn_per_probe(crl_dqn* h, const float* leaves, int32_t n, uint64_t gstep, int32_t k, double beta, int32_t* idx, double* weight,
                          double* tree) {
  DQN_PER_GUARD(h, "crl_dqn_per_probe");
  if (!leaves || !idx || !weight) { set_error("crl_dqn_per_probe: null argument (leaves, idx and weight are required)"); return 1; }
  if (n < 1 || n > DQN_MAX_CAP) { set_error("crl_dqn_per_probe: n must be in 1..65536"); return 1; }
  if (k < 1 || k > DQN_MAX_BATCH) { set_error("crl_dqn_per_probe: k must be in 1..1024"); return 1; }
  if (!(beta >= 0.0 && beta <= 1.0)) { set_error("crl_dqn_per_probe: beta must be in 0..1"); return 1; }
  for (int32_t i = 0; i < n; ++i)
    if (!((double)leaves[i] >= PER_LEAF_MIN && (double)leaves[i] <= PER_LEAF_MAX)) { set_error("crl_dqn_per_probe: every leaf must be in 2^-100..2^100"); return 1; }
  if (!h->probe_tree) {
    CRL_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&h->probe_tree), 2 * (size_t)DQN_MAX_CAP * 8));
    CRL_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&h->probe_idx), (size_t)DQN_MAX_BATCH * 4));
    CRL_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&h->probe_w), (size_t)DQN_MAX_BATCH * 8));
  }
  const int C = per_tree_leaves(n);
  std::vector<double> t(2 * (size_t)C, 0.0);                 // leaves widened, slots >= n and the inner nodes 0.0 (the kernel rebuilds the inner nodes)
  for (int32_t i = 0; i < n; ++i) t[(size_t)C + (size_t)i] = (double)leaves[i];
  CRL_HIP_CHECK(hipMemcpyAsync(h->probe_tree, t.data(), t.size() * 8, hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(dqn_per_probe_kernel, dim3(1), dim3(1024), 0, h->stream, h->probe_tree, C, (int)n, (int)k, h->cfg.seed, gstep, beta, h->probe_idx,
                     h->probe_w);
  CRL_HIP_CHECK(hipGetLastError());
  CRL_HIP_CHECK(hipMemcpyAsync(idx, h->probe_idx, (size_t)k * 4, hipMemcpyDeviceToHost, h->stream));
  CRL_HIP_CHECK(hipMemcpyAsync(weight, h->probe_w, (size_t)k * 8, hipMemcpyDeviceToHost, h->stream));
  if (tree) CRL_HIP_CHECK(hipMemcpyAsync(tree, h->probe_tree, t.size() * 8, hipMemcpyDeviceToHost, h->stream));
  CRL_HIP_CHECK(hipStreamSynchronize(h->stream));
  return 0;
}

int32_t crl_dqn_destroy(crl_dqn* h) {
  if (!h) return 0;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  if (h->cycle_exec) (void)hipGraphExecDestroy(h->cycle_exec);
  DQNDev& d = h->d;
  void* ptrs[] = {d.q, d.t, d.grads, d.m, d.v, d.betap, d.ctl, d.eps, d.losses, d.rb_state, d.rb_next, d.rb_reward, d.rb_action,
                  d.rb_terminal, d.H1, d.H2, d.Q, d.dz, d.sq, d.d2, d.d1, d.idx, h->stage, h->eval.p,
                  d.per.tree, d.per.ctl, d.per.w, d.per.abs_td, h->probe_tree, h->probe_idx, h->probe_w,
                  d.tgt.last, d.tgt.m, d.tgt.astar, d.tgt.nret, d.tgt.ndisc, d.tgt.td, h->walk_scratch,
                  d.c51.L, d.c51.dl, d.c51.proj, d.c51.sloss, h->proj_scratch, d.noisy.pq, d.noisy.pt, h->xi_scratch};
  for (void* p : ptrs) if (p) (void)hipFree(p);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
  return 0;
}

int32_t crl_dqn_write_params(crl_dqn* h, const float* q_params, size_t n) {
  DQN_GUARD(h);
  if (!q_params || n != h->n_params) { set_error("crl_dqn_write_params: expected " + std::to_string(h->n_params) + " floats"); return 1; }
  // dqn.jl:40 deepcopy(q_net); a noisy handle takes mu then sigma for both nets and rebuilds both images at its current generation
  CRL_HIP_CHECK(hipMemcpyAsync(h->noisy ? h->d.noisy.pq : h->d.q, q_params, n * 4, hipMemcpyHostToDevice, h->stream));
  CRL_HIP_CHECK(hipMemcpyAsync(h->noisy ? h->d.noisy.pt : h->d.t, q_params, n * 4, hipMemcpyHostToDevice, h->stream));
  if (h->noisy && noisy_materialise(h)) return 1;
  CRL_HIP_CHECK(hipStreamSynchronize(h->stream));
  h->params_set = true;
  return 0;
}
int32_t crl_dqn_init_params(crl_dqn* h, uint64_t seed) {
  DQN_GUARD(h);
  std::vector<float> w(h->n_params);
  if (h->noisy ? crl_dqn_noisy_make_nn(seed, h->sigma0, h->duel ? 1 : 0, h->c51 ? h->d.c51.N : 0, w.data(), w.size())
      : h->duel ? crl_dqn_dueling_make_nn(seed, h->c51 ? h->d.c51.N : 0, w.data(), w.size())
              : h->c51 ? crl_dqn_c51_make_nn(seed, h->d.c51.N, w.data(), w.size()) : crl_dqn_make_nn(seed, w.data(), w.size())) return 1;
  return crl_dqn_write_params(h, w.data(), w.size());
}

int32_t crl_dqn_read_params(crl_dqn* h, float* q_params, float* target_params, size_t n) {
  DQN_GUARD(h);
  if (!q_params || n != h->n_params) { set_error("crl_dqn_read_params: expected " + std::to_string(h->n_params) + " floats"); return 1; }
  CRL_HIP_CHECK(hipMemcpyAsync(q_params, h->noisy ? h->d.noisy.pq : h->d.q, n * 4, hipMemcpyDeviceToHost, h->stream));
  if (target_params) CRL_HIP_CHECK(hipMemcpyAsync(target_params, h->noisy ? h->d.noisy.pt : h->d.t, n * 4, hipMemcpyDeviceToHost, h->stream));
  CRL_HIP_CHECK(hipStreamSynchronize(h->stream));
  return 0;
}
int32_t crl_dqn_status_read(crl_dqn* h, crl_dqn_status* out) {
  DQN_GUARD(h);
  if (!out) { set_error("null argument"); return 1; }
  DQNCtl c;
  CRL_HIP_CHECK(hipMemcpyAsync(&c, h->d.ctl, sizeof(c), hipMemcpyDeviceToHost, h->stream));
  CRL_HIP_CHECK(hipStreamSynchronize(h->stream));
  for (int i = 0; i < 4; ++i) out->env_state[i] = c.env[i];
  out->global_step = c.global_step; out->rb_size = c.size; out->n_updates = c.n_updates; out->last_loss = c.last_loss;
  return 0;
}

int32_t crl_dqn_run(crl_dqn* h, int64_t max_env_steps, crl_dqn_episode* eps, int32_t max_eps, int32_t* n_eps,
                    crl_dqn_loss_record* losses, int32_t max_losses, int32_t* n_losses, int64_t* steps_taken) {
  DQN_GUARD(h);
  if (!h->params_set) { set_error("crl_dqn_run: parameters not set — crl_dqn_write_params or crl_dqn_init_params first (dqn.jl:39; a fresh handle holds zeros)"); return 1; }
  if (!n_eps || !n_losses || max_eps < 0 || max_losses < 0 || (max_eps > 0 && !eps) || (max_losses > 0 && !losses)) {
    set_error("crl_dqn_run: bad arguments"); return 1;
  }
  *n_eps = 0; *n_losses = 0;
  if (steps_taken) *steps_taken = 0;
  if (max_env_steps <= 0) return 0;
  {
    const DQNDev& d = h->d;
    hipStream_t st = h->stream;
    const int k = (int)h->cfg.batch_size;
    // a cycle ends at the next multiple of train_freq; one spare cycle covers a call that starts mid-cycle
    const int64_t limit = h->cfg.total_timesteps < max_env_steps ? h->cfg.total_timesteps : max_env_steps;
    const int64_t cycles = limit / h->cfg.train_freq + 2;
    hipLaunchKernelGGL(dqn_begin_kernel, dim3(1), dim3(1), 0, st, d, max_env_steps);
    if (!h->cycle_exec && !h->graph_failed) {
      // one cycle = ten (a noisy handle: eleven) dependent launches with constant arguments: captured once, replayed as a hipGraph (the cycle is
      // bound by the dependent kernels themselves — 52.7 K vs 53.1 K steps/s without the graph — so this stays opt-in)
      hipGraph_t g = nullptr;
      bool ok = hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) == hipSuccess;
      if (ok) {
        enqueue_cycle(st, d, k);
        ok = hipStreamEndCapture(st, &g) == hipSuccess && g != nullptr;
        if (ok) ok = hipGraphInstantiate(&h->cycle_exec, g, nullptr, nullptr, 0) == hipSuccess;
        if (g) (void)hipGraphDestroy(g);
      }
      if (!ok) { h->cycle_exec = nullptr; h->graph_failed = true; (void)hipGetLastError(); }
    }
    for (int64_t cy = 0; cy < cycles; ++cy) {
      if (h->cycle_exec) CRL_HIP_CHECK(hipGraphLaunch(h->cycle_exec, st));
      else enqueue_cycle(st, d, k);
      if ((cy & 4095) == 4095) CRL_HIP_CHECK(hipStreamSynchronize(st));   // bound the queue depth of very long calls
    }
    CRL_HIP_CHECK(hipGetLastError());
  }
  DQNCtl c;
  CRL_HIP_CHECK(hipMemcpyAsync(&c, h->d.ctl, sizeof(c), hipMemcpyDeviceToHost, h->stream));
  CRL_HIP_CHECK(hipStreamSynchronize(h->stream));
  if (steps_taken) *steps_taken = c.taken;
  int ne = c.n_eps < DQN_MAX_EPS ? c.n_eps : DQN_MAX_EPS; if (ne > max_eps) ne = max_eps;
  int nl = c.n_losses < DQN_MAX_LOSSES ? c.n_losses : DQN_MAX_LOSSES; if (nl > max_losses) nl = max_losses;
  if (ne > 0) CRL_HIP_CHECK(hipMemcpyAsync(eps, h->d.eps, sizeof(crl_dqn_episode) * (size_t)ne, hipMemcpyDeviceToHost, h->stream));
  if (nl > 0) CRL_HIP_CHECK(hipMemcpyAsync(losses, h->d.losses, sizeof(crl_dqn_loss_record) * (size_t)nl, hipMemcpyDeviceToHost, h->stream));
  CRL_HIP_CHECK(hipStreamSynchronize(h->stream));
  *n_eps = ne; *n_losses = nl;
  return 0;
}

int32_t crl_dqn_q_values(crl_dqn* h, const double* obs, int32_t n, double* q) {
  DQN_GUARD(h);
  if (!h->params_set) { set_error("crl_dqn_q_values: parameters not set — crl_dqn_write_params or crl_dqn_init_params first (dqn.jl:39)"); return 1; }
  if (n < 0 || (n > 0 && (!obs || !q))) { set_error("crl_dqn_q_values: bad arguments"); return 1; }
  if (n == 0) return 0;
  const size_t N = (size_t)n, need = N * (QD + QA) * 8;
  if (dqn_stage(h, need)) return 1;
  double* so = static_cast<double*>(h->stage);
  double* sq = so + N * QD;
  CRL_HIP_CHECK(hipMemcpyAsync(so, obs, N * QD * 8, hipMemcpyHostToDevice, h->stream));
  if (h->duel) hipLaunchKernelGGL(dqn_duel_q_kernel, dim3(n), dim3(DQN_OBS_BLOCK), 0, h->stream, h->greedy_image(), h->d.duel, h->d.c51, (const double*)so, n, sq,
                                  (double*)nullptr, (double*)nullptr, (double*)nullptr);
  else if (h->c51) hipLaunchKernelGGL(dqn_c51_q_kernel, dim3(n), dim3(DQN_OBS_BLOCK), 0, h->stream, h->greedy_image(), h->d.c51, (const double*)so, n, sq, (double*)nullptr);
  else hipLaunchKernelGGL(dqn_q_kernel, dim3(n), dim3(DQN_OBS_BLOCK), 0, h->stream, h->greedy_image(), (const double*)so, n, sq);
  CRL_HIP_CHECK(hipGetLastError());
  CRL_HIP_CHECK(hipMemcpyAsync(q, sq, N * QA * 8, hipMemcpyDeviceToHost, h->stream));
  CRL_HIP_CHECK(hipStreamSynchronize(h->stream));
  return 0;
}

// Held-out evaluation: argument checks, scratch, ONE launch (dqn_eval_kernel), the per-episode arrays back to the host, the report in Float64
int32_t crl_dqn_evaluate(crl_dqn* h, const crl_eval_config* cfg, crl_value_eval_report* report, double* returns, int32_t* lengths,
                         double* disc_returns, double* v0, int32_t* trace_action) {
  DQN_GUARD(h);
  if (value_eval_check("crl_dqn_evaluate", cfg, report, h->params_set, "crl_dqn_write_params or crl_dqn_init_params first (dqn.jl:39)",
                       h->cfg.max_steps, /*has_sampler=*/false, trace_action)) return 1;
  ValueEvalArgs ev;
  if (value_eval_scratch(h->eval, cfg, ev)) return 1;
  // every slot of the arrays and of the trace is written: each env plays its quota and then fills the rest of its trace column
  const dim3 grid((unsigned)((ev.n + DQN_EVAL_WAVES - 1) / DQN_EVAL_WAVES)), block(64 * DQN_EVAL_WAVES);
  if (h->duel) hipLaunchKernelGGL(dqn_duel_eval_kernel, dim3((unsigned)((ev.n + DUEL_EVAL_WAVES - 1) / DUEL_EVAL_WAVES)), dim3(64 * DUEL_EVAL_WAVES),
                                  duel_eval_lds((int)h->P), h->stream, h->greedy_image(), h->d.duel, h->d.c51, (int)h->cfg.max_steps, h->cfg.gamma, ev);
  else if (h->c51) hipLaunchKernelGGL(dqn_c51_eval_kernel, grid, block, c51_eval_lds((int)h->P), h->stream, h->greedy_image(), h->d.c51,
                                 (int)h->cfg.max_steps, h->cfg.gamma, ev);
  else hipLaunchKernelGGL(dqn_eval_kernel, grid, block, 0, h->stream, h->greedy_image(), (int)h->cfg.max_steps, h->cfg.gamma, ev);
  CRL_HIP_CHECK(hipGetLastError());
  return value_eval_finish(h->stream, ev, report, returns, lengths, disc_returns, v0, trace_action);
}
int32_t crl_dqn_eval_envs_per_block(void) { return DQN_EVAL_WAVES; }

}  // extern "C"
