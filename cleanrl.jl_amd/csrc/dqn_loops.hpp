// dqn_loops.hpp — what dqn.hip's heads (plain, categorical, dueling) have in common, stated once: the device-side state (DQNCtl, DQNDev), the collect
// loop, the plain trunk per observation, the evaluation episode loop with its paired-chain layers, the loss sum and the Adam step. Each is a
// __device__ __forceinline__ function (template) that a kernel of dqn.hip calls with a functor for the part that differs by head; the kernels keep
// their own LDS placement, weight staging and early exits. Float64 arithmetic with contraction off, every sum in the oracle's order:
// the pragma is lexical, so every function body here carries its own.
#pragma once
#include "common.hpp"
#include "env64.hpp"
#include "optim.hpp"
#include "dqn_per.hpp"
#include "dqn_target.hpp"
#include "dqn_c51.hpp"
#include "dqn_duel.hpp"
#include "dqn_noisy.hpp"
#include "value_eval.hpp"

namespace crl {

constexpr int QH1 = 120, QH2 = 84, QD = 4, QA = 2;
constexpr int QoW1 = 0, Qob1 = QH1 * QD, QoW2 = Qob1 + QH1, Qob2 = QoW2 + QH2 * QH1, QoW3 = Qob2 + QH2, Qob3 = QoW3 + QA * QH2;
constexpr int QP = Qob3 + QA;
static_assert(QP == CRL_DQN_PARAM_COUNT, "parameter count");
constexpr int DQN_MAX_EPS = 8192, DQN_MAX_LOSSES = 4096, DQN_MAX_BATCH = 1024, DQN_MAX_CAP = 1 << 16;

struct DQNCtl {
  double env[4]; double episode_return, last_loss;
  int64_t global_step, episode_length, n_updates, taken, ptr, size, budget;
  int32_t env_t, n_eps, n_losses, train_pending;
};

struct DQNDev {
  crl_dqn_config cfg;
  float *q, *t, *grads, *m, *v; double* betap;
  DQNCtl* ctl; crl_dqn_episode* eps; crl_dqn_loss_record* losses;
  double *rb_state, *rb_next, *rb_reward; int32_t* rb_action; uint8_t* rb_terminal;
  double *H1, *H2, *Q, *dz, *sq, *d2, *d1;   // [nets][120·k], [nets][84·k], [nets][2·k], [k], [k], [84·k], [120·k]
  int32_t* idx;                               // [k] minibatch indices into the ring
  const int32_t* boot;                        // [k] the slots whose next_state the target bootstraps from: idx, or tgt.last on a crl_dqn_create_with handle
  int32_t nets, pad;                          // forward passes per update: q_net(state), target_net(x) and, under double_q, q_net(x)
  PerDev per;                                 // prioritized replay (crl_dqn_per_create); all zero on a crl_dqn_create handle
  TgtDev tgt;                                 // n-step / double-Q targets (crl_dqn_create_with); all zero on the other handles
  C51Dev c51;                                 // the categorical head (crl_dqn_c51_create; such a handle also has tgt.on); all zero on the other handles
  DuelDev duel;                               // the dueling heads (crl_dqn_dueling_create; such a handle also has tgt.on, and c51.on if categorical): then H2
                                              // and d2 hold 168 units per sample; all zero on the other handles
  NoisyDev noisy;                             // noisy linear layers (crl_dqn_noisy_create): q / t are then the effective images mu + sigma·eps of the current
                                              // generation, m / v hold 2P entries and betap twice the twin's pairs; all zero on the other handles
};

__device__ __forceinline__ double dq_linear_schedule(double start_e, double end_e, double duration, double t) {
#pragma clang fp contract(off)
  const double slope = (end_e - start_e) / duration;
  const double v = slope * t + start_e;
  return v > end_e ? v : end_e;
}

// ------------------------------------------------------------------------------------------------------
// The plain trunk for ONE observation by one block: one unit per thread, a block barrier after each layer. W is any float image of a net whose
// W1 b1 W2 b2 sit at the plain offsets (global or LDS; the dot products read one weight per term). The greedy step of dqn_collect_kernel, the collect
// functor of the categorical head, dqn_q_kernel and dqn_c51_q_kernel run both layers, duel_block_forward the first. The sums are serial chains in
// input order, bias last, so the unroll factors change no bit; they are the collect kernels', whose greedy steps are the hot users.
// One unit per thread means the block must bring at least 120 threads: every kernel that calls these is launched with DQN_OBS_BLOCK.
// ------------------------------------------------------------------------------------------------------
constexpr int DQN_OBS_BLOCK = 128;     // threads of the kernels that run one observation per block: collect, q_values / probs / streams
static_assert(DQN_OBS_BLOCK >= QH1 && DQN_OBS_BLOCK >= QH2, "dqn_block_trunk gives every hidden unit a thread of its own");
template <typename WP>
__device__ __forceinline__ void dqn_block_layer1(const WP W, const double* obs, double* h1s) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x;
  if (tid < QH1) {
    double acc = 0.0;
    for (int kk = 0; kk < QD; ++kk) acc += (double)W[QoW1 + tid + QH1 * kk] * obs[kk];
    acc += (double)W[Qob1 + tid];
    h1s[tid] = acc > 0.0 ? acc : 0.0;
  }
  __syncthreads();
}
template <typename WP>
__device__ __forceinline__ void dqn_block_trunk(const WP W, const double* obs, double* h1s, double* h2s) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x;
  dqn_block_layer1(W, obs, h1s);
  if (tid < QH2) {
    double acc = 0.0;
#pragma unroll 8
    for (int kk = 0; kk < QH1; ++kk) acc += (double)W[QoW2 + tid + QH2 * kk] * h1s[kk];
    acc += (double)W[Qob2 + tid];
    h2s[tid] = acc > 0.0 ? acc : 0.0;
  }
  __syncthreads();
}
// one row of a head of `rows` rows behind the plain trunk (W3 at QoW3, its bias behind it): the scalar head has 2 rows, the categorical one 2N
template <typename WP>
__device__ __forceinline__ double dqn_head_row(const WP W, int rows, int row, const double* h2) {
#pragma clang fp contract(off)
  double acc = 0.0;
#pragma unroll 4
  for (int kk = 0; kk < QH2; ++kk) acc += (double)W[QoW3 + row + rows * kk] * h2[kk];
  return acc + (double)W[QoW3 + rows * QH2 + row];
}

// ------------------------------------------------------------------------------------------------------
// dqn.jl:57-93: env steps until a training step is due (train_pending = 1), the budget or total_timesteps is used up. The block of 128 runs it; thread
// 0 owns the env, the ring and the control block, the others only join greedy_q. DQNCollectLds is the loop's state in LDS: C51CollectLds and
// DuelCollectLds start with it. dqn_collect_kernel (the plain head) keeps its own text of this loop and its own static variables: it was slower
// around this one (dqn.hip), so a change to the ring, the episode record or the train_pending rule is made in both. greedy_q() is block-wide: it reads s.obs, leaves s.qs[0..1] (dqn.jl:64
// qs = q_net(obs)) and ENDS ON A BLOCK BARRIER, behind which thread 0 reads them.
// ------------------------------------------------------------------------------------------------------
struct DQNCollectLds {
  DQNCtl c;
  double obs[QD], qs[QA], eps_s;
  int go, need_q, action_s, pad;
};
template <typename GreedyQ>
__device__ __forceinline__ void dqn_collect_loop(const DQNDev& a, DQNCollectLds& s, GreedyQ greedy_q) {
#pragma clang fp contract(off)
  DQNCtl& c = s.c;
  const int tid = threadIdx.x;
  while (true) {
    if (tid == 0) {
      s.go = (!c.train_pending && c.taken < c.budget && c.global_step < a.cfg.total_timesteps) ? 1 : 0;
      if (s.go) {
        c.global_step += 1; c.taken += 1;                                            // dqn.jl:57
        const uint64_t gstep = (uint64_t)c.global_step;
        for (int i = 0; i < QD; ++i) s.obs[i] = c.env[i];                            // dqn.jl:58
        s.eps_s = dq_linear_schedule(a.cfg.epsilon_start, a.cfg.epsilon_end, a.cfg.epsilon_duration, (double)c.global_step);
        if (u53(philox_env(a.cfg.seed, 0u, gstep, 0u)) < s.eps_s) {                  // dqn.jl:61-62
          s.need_q = 0;
          s.action_s = (int)(philox_env(a.cfg.seed, 0u, gstep, 4u).x >> 31);
        } else s.need_q = 1;
      }
    }
    __syncthreads();
    if (!s.go) break;
    if (s.need_q) greedy_q();                                                        // dqn.jl:64 qs = q_net(obs)
    if (tid == 0) {
      const uint64_t gstep = (uint64_t)c.global_step;
      const int action = s.need_q ? (s.qs[1] > s.qs[0] ? 1 : 0) : s.action_s;       // dqn.jl:65 argmax: first maximum
      const bool done = cartpole_step64(c.env, c.env_t, action, a.cfg.max_steps);  // dqn.jl:68
      const double rew = done ? 0.0 : 1.0;
      const size_t p = (size_t)c.ptr;                                                // dqn.jl:71-78 Buffer.add!
      for (int i = 0; i < QD; ++i) { a.rb_state[QD * p + i] = s.obs[i]; a.rb_next[QD * p + i] = c.env[i]; }
      a.rb_action[p] = action; a.rb_reward[p] = rew; a.rb_terminal[p] = done ? 1 : 0;
      c.ptr = c.ptr + 1 >= a.cfg.buffer_size ? 0 : c.ptr + 1;
      c.size = c.size + 1 > a.cfg.buffer_size ? a.cfg.buffer_size : c.size + 1;
      c.episode_return += rew; c.episode_length += 1;                               // dqn.jl:81-82
      if (done) {                                                                    // dqn.jl:83-90
        if (c.n_eps < DQN_MAX_EPS) {
          a.eps[c.n_eps].episode_return = c.episode_return; a.eps[c.n_eps].episode_length = c.episode_length;
          a.eps[c.n_eps].global_step = c.global_step; a.eps[c.n_eps].epsilon = s.eps_s;
        }
        c.n_eps += 1;
        c.episode_length = 0; c.episode_return = 0.0;
        env_reset64(c.env, a.cfg.seed, gstep, 1); c.env_t = 0;
      }
      c.train_pending = (c.global_step > a.cfg.min_buff_size && c.global_step % a.cfg.train_freq == 0) ? 1 : 0;   // dqn.jl:93
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------------
// crl_dqn_evaluate's episode loop for ONE env owned by ONE wave (every lane carries env state, episode sums and the action alike: wave-uniform, no
// broadcast): `episodes` episodes from reset to done, v0 / trace row / ret / disc_ret / len per episode, then the rest of the env's trace column.
// q_of(s, q0, q1) is the head's wave-level forward through the wave's private strips; it fences between its layers itself, and the fence at the end
// of the step here keeps the next step's strip writes behind this step's reads. Nothing here knows how many waves share a block: no block barrier.
// ------------------------------------------------------------------------------------------------------
template <typename QOf>
__device__ __forceinline__ void dqn_eval_episodes(const ValueEvalArgs& ev, int env, int lane, int max_steps, double gamma, QOf q_of) {
#pragma clang fp contract(off)
  int64_t row = 0;                       // the env's step count across its episodes
  for (int j = 0; j < ev.episodes; ++j) {
    double s[QD], ret = 0.0, disc_ret = 0.0, disc = 1.0;
    int t = 0, length = 0;
    const size_t slot = (size_t)j * ev.n + env;
    env_reset64(s, ev.seed, (uint64_t)j * (uint64_t)ev.n + (uint64_t)env, S_VEVAL_RESET);
    while (true) {
      double q0, q1;
      q_of(s, q0, q1);
      const int action = q1 > q0 ? 1 : 0;                                               // argmax: first maximum, as dqn_collect_loop
      if (lane == 0) {
        if (length == 0) ev.v0[slot] = action ? q1 : q0;
        if (row < ev.trace_steps) ev.trace[(size_t)row * ev.n + env] = action;
      }
      row += 1;
      const bool done = cartpole_step64(s, t, action, max_steps);
      const double rew = done ? 0.0 : 1.0;
      ret += rew;
      disc_ret += disc * rew;
      disc = disc * gamma;
      length += 1;
      wave_lds_fence();                  // the next step's strip writes stay behind this step's reads
      if (done) break;
    }
    if (lane == 0) { ev.ret[slot] = ret; ev.disc_ret[slot] = disc_ret; ev.len[slot] = length; }
  }
  value_eval_trace_tail(ev, env, row, lane);
}
// layer 1 by one wave: units `lane` and `lane + 64`, two independent chains side by side; a lane that has no second unit (lane + 64 past the layer)
// repeats its first and stores nothing. wq is the net's float image in LDS, W1 at oW1 and b1 at ob1; h1w the wave's strip. No fence: the caller's.
__device__ __forceinline__ void eval_layer1_pair(const float* wq, int oW1, int ob1, const double* s, double* h1w, int lane) {
#pragma clang fp contract(off)
  const int u1b = lane + 64 < QH1 ? lane + 64 : lane;
  double acc = 0.0, acc2 = 0.0;
#pragma unroll
  for (int kk = 0; kk < QD; ++kk) {
    acc += (double)wq[oW1 + lane + QH1 * kk] * s[kk];
    acc2 += (double)wq[oW1 + u1b + QH1 * kk] * s[kk];
  }
  acc += (double)wq[ob1 + lane];
  acc2 += (double)wq[ob1 + u1b];
  h1w[lane] = acc > 0.0 ? acc : 0.0;
  if (lane + 64 < QH1) h1w[lane + 64] = acc2 > 0.0 ? acc2 : 0.0;
}
// layer 2 of the plain trunk by one wave: the same pairing — 120 dependent adds per step, not 240
__device__ __forceinline__ void eval_layer2_pair(const float* wq, const double* h1w, double* h2w, int lane) {
#pragma clang fp contract(off)
  const int u2b = lane + 64 < QH2 ? lane + 64 : lane;
  double acc = 0.0, acc2 = 0.0;
#pragma unroll 8
  for (int kk = 0; kk < QH1; ++kk) {
    const double h = h1w[kk];
    acc += (double)wq[QoW2 + lane + QH2 * kk] * h;
    acc2 += (double)wq[QoW2 + u2b + QH2 * kk] * h;
  }
  acc += (double)wq[Qob2 + lane];
  acc2 += (double)wq[Qob2 + u2b];
  h2w[lane] = acc > 0.0 ? acc : 0.0;
  if (lane + 64 < QH2) h2w[lane + 64] = acc2 > 0.0 ? acc2 : 0.0;
}
// the plain trunk's head by one wave: rows r0 and r1 of a head of `rows` rows side by side, every lane alike or one atom per lane → the two sums
__device__ __forceinline__ void eval_head_pair(const float* wq, int rows, int r0, int r1, const double* h2w, double& out0, double& out1) {
#pragma clang fp contract(off)
  double a0 = 0.0, a1 = 0.0;
#pragma unroll 4
  for (int kk = 0; kk < QH2; ++kk) {
    const double h = h2w[kk];
    a0 += (double)wq[QoW3 + r0 + rows * kk] * h;
    a1 += (double)wq[QoW3 + r1 + rows * kk] * h;
  }
  out0 = a0 + (double)wq[QoW3 + rows * QH2 + r0];
  out1 = a1 + (double)wq[QoW3 + rows * QH2 + r1];
}

// ------------------------------------------------------------------------------------------------------
// The tail of an update. Flux.mse's mean (dqn.jl:106) or the head's own loss: (Σ_b sq_b, SAMPLE ORDER) / k, by ONE thread behind a barrier or a launch
// boundary that makes every sq_b visible.
// ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void dqn_loss_in_sample_order(const DQNDev& a) {
#pragma clang fp contract(off)
  const int k = (int)a.cfg.batch_size;
  double loss = 0.0;
  for (int b = 0; b < k; ++b) loss += a.sq[b];
  a.ctl->last_loss = loss / (double)k;
}
// which of the six arrays W1 b1 W2 b2 W3 b3 parameter p belongs to; ob3 = where b3 starts (Qob3, or behind the categorical head's longer W3)
__device__ __forceinline__ int dqn_array_of(int p, int ob3) {
#pragma clang fp contract(off)
  return p < Qob1 ? 0 : p < QoW2 ? 1 : p < Qob2 ? 2 : p < QoW3 ? 3 : p < ob3 ? 4 : 5;
}
// Flux Adam(lr) (dqn.jl:41,109: optim.hpp's entry step without the clip, one β-power pair per array) + hard target copy (dqn.jl:111-113) + loss record
// (dqn.jl:115-117) over P parameters in n_arrays arrays, array_of(p) naming p's; one block
template <typename ArrayOf>
__device__ __forceinline__ void dqn_adam_step(const DQNDev& a, int P, int n_arrays, ArrayOf array_of) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x, nth = blockDim.x;
  const int64_t gstep = a.ctl->global_step;
  const bool copy = gstep % a.cfg.target_net_freq == 0;
  for (int p = tid; p < P; p += nth) {
    const int arr = array_of(p);
    float mi, vi, w;
    adam_entry((double)a.grads[p], a.m[p], a.v[p], a.q[p], a.betap[2 * arr], a.betap[2 * arr + 1], a.cfg.lr, /*clip=*/false, 1.0, mi, vi, w);
    a.m[p] = mi; a.v[p] = vi; a.q[p] = w;
    if (copy) a.t[p] = w;
  }
  __syncthreads();
  if (tid < n_arrays) betap_advance(a.betap, tid, a.betap[2 * tid], a.betap[2 * tid + 1]);
  if (tid == 0) {
    DQNCtl* c = a.ctl;
    c->n_updates += 1;
    if (gstep % a.cfg.log_frequency == 0) {
      if (c->n_losses < DQN_MAX_LOSSES) { a.losses[c->n_losses].global_step = gstep; a.losses[c->n_losses].loss = c->last_loss; }
      c->n_losses += 1;
    }
    c->train_pending = 0;
  }
}

// ------------------------------------------------------------------------------------------------------
// dqn_adam_step on a noisy handle (dqn_noisy.hpp), one block: the update that is now completing was update u = n_updates, run on the images of generation
// u. (1) that generation's xi table of the online net is rebuilt in LDS; (2) adam_entry on mu[p] with g = grads[p] and on sigma[p] with g·eps_p, sigma's
// arrays taking the β-power pairs n_arrays + arr; (3) the hard copy of mu and sigma to the target; (4) β powers, loss record, train_pending as
// dqn_adam_step; (5) the xi tables of generation u + 1 for both nets; (6) both images. xs: 2·NOISY_MAX_XI floats of LDS. Steps 5 and 6 are what
// dqn_noisy_materialise does; by default the cycle runs them as a launch of their own over every CU (CRL_NOISY_SPLIT_TAIL), which the launch
// boundary orders behind the n_updates this block leaves.
// ------------------------------------------------------------------------------------------------------
#ifndef CRL_NOISY_SPLIT_TAIL
#define CRL_NOISY_SPLIT_TAIL 1   // 1: steps 5-6 are an eleventh, multi-block launch (dqn_noisy_materialise_kernel); 0 (experiment build, csrc/Makefile EXTRA=-DCRL_NOISY_SPLIT_TAIL=0): they run here, in the one block — measured slower, DESIGN.md §3l
#endif
template <typename ArrayOf>
__device__ __forceinline__ void dqn_noisy_adam_step(const DQNDev& a, int n_arrays, ArrayOf array_of, const NoisyTable& tab, float* xs) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x, nth = blockDim.x, P = a.noisy.P;
  const int64_t gstep = a.ctl->global_step;
  const uint64_t u = (uint64_t)a.ctl->n_updates;
  const bool copy = gstep % a.cfg.target_net_freq == 0;
  float* const pq = a.noisy.pq;
  float* const pt = a.noisy.pt;
  noisy_build_xi(xs, tab.n_xi, a.cfg.seed, u, S_NOISY_Q);
  __syncthreads();
  for (int p = tid; p < P; p += nth) {
    const int arr = array_of(p);
    const float g = a.grads[p], gs = g * noisy_eps(tab, xs, p);
    float mi, vi, w;
    adam_entry((double)g, a.m[p], a.v[p], pq[p], a.betap[2 * arr], a.betap[2 * arr + 1], a.cfg.lr, /*clip=*/false, 1.0, mi, vi, w);
    a.m[p] = mi; a.v[p] = vi; pq[p] = w;
    if (copy) pt[p] = w;
    const int sarr = n_arrays + arr;
    adam_entry((double)gs, a.m[P + p], a.v[P + p], pq[P + p], a.betap[2 * sarr], a.betap[2 * sarr + 1], a.cfg.lr, /*clip=*/false, 1.0, mi, vi, w);
    a.m[P + p] = mi; a.v[P + p] = vi; pq[P + p] = w;
    if (copy) pt[P + p] = w;
  }
  __syncthreads();                       // every read of the β powers and of generation u's table is done
  if (tid < 2 * n_arrays) betap_advance(a.betap, tid, a.betap[2 * tid], a.betap[2 * tid + 1]);
  if (tid == 0) {
    DQNCtl* c = a.ctl;
    c->n_updates += 1;
    if (gstep % a.cfg.log_frequency == 0) {
      if (c->n_losses < DQN_MAX_LOSSES) { a.losses[c->n_losses].global_step = gstep; a.losses[c->n_losses].loss = c->last_loss; }
      c->n_losses += 1;
    }
    c->train_pending = 0;
  }
#if !CRL_NOISY_SPLIT_TAIL                // the experiment build; by default the cycle's eleventh launch (dqn_noisy_materialise_kernel) does this on every CU
  noisy_build_xi(xs, tab.n_xi, a.cfg.seed, u + 1, S_NOISY_Q);
  noisy_build_xi(xs + NOISY_MAX_XI, tab.n_xi, a.cfg.seed, u + 1, S_NOISY_T);
  __syncthreads();
  for (int p = tid; p < P; p += nth) {   // the thread that wrote mu[p] / sigma[p] above reads them here
    a.q[p] = noisy_weight(pq[p], pq[P + p], noisy_eps(tab, xs, p));
    a.t[p] = noisy_weight(pt[p], pt[P + p], noisy_eps(tab, xs + NOISY_MAX_XI, p));
  }
#endif
}
// both images of generation gen from mu and sigma, any grid: every block builds the two tables in its LDS (xs: 2·NOISY_MAX_XI floats)
__device__ __forceinline__ void dqn_noisy_materialise(const DQNDev& a, const NoisyTable& tab, uint64_t gen, float* xs) {
  const int P = a.noisy.P;
  noisy_build_xi(xs, tab.n_xi, a.cfg.seed, gen, S_NOISY_Q);
  noisy_build_xi(xs + NOISY_MAX_XI, tab.n_xi, a.cfg.seed, gen, S_NOISY_T);
  __syncthreads();
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < P; p += gridDim.x * blockDim.x) {
    a.q[p] = noisy_weight(a.noisy.pq[p], a.noisy.pq[P + p], noisy_eps(tab, xs, p));
    a.t[p] = noisy_weight(a.noisy.pt[p], a.noisy.pt[P + p], noisy_eps(tab, xs + NOISY_MAX_XI, p));
  }
}

}  // namespace crl
