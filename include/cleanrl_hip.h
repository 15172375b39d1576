/*
 * cleanrl_hip.h — C ABI of libcleanrl_hip.so: the MI355X-native PPO rollout + GAE + update hot path.
 *
 * Drop-in boundary for sash-a/CleanRL.jl `src/algorithms/ppo.jl`. The reference has no FFI today (it is pure
 * Julia); each entry point below names the reference function / lines it replaces, and INTEGRATION.md shows the
 * `ccall` a maintainer adds on the Julia side. Plain pointers and sizes only; no C++ or torch types.
 *
 * Conventions
 *  - every call returns 0 on success, non-zero on error; crl_last_error() gives the message (thread-local).
 *    No exception crosses the boundary. Julia wrapper: `rc == 0 || error(unsafe_string(crl_last_error()))`.
 *  - host pointers are borrowed for the duration of the call only (Julia: GC.@preserve); device memory is owned by
 *    the library behind the opaque crl_ppo handle.
 *  - layouts are Julia column-major, passed without copies: obs (obs_dim, n); buffers (nt, k); flat sample index
 *    b = e + nt*t (ppo.jl:184-189). Actions are 0-based int32 here (Julia side adds 1); terminals are uint8
 *    (widen the env's BitArray to Vector{Bool} first, multi_thread_env.jl:18).
 *  - parameters travel as ONE flat float vector in Flux.params(actor, critic) order (ppo.jl:196):
 *    actor W1(h,obs) b1(h) W2(h,h) b2(h) W3(A,h) b3(A), critic W1 b1 W2 b2 W3(1,h) b3(1); W is (out,in) col-major.
 *  - calls on one handle must be serialised by the caller; work is asynchronous on the handle's HIP stream until
 *    crl_sync() or a call that copies results to the host.
 */
#ifndef CLEANRL_HIP_H
#define CLEANRL_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CRL_VERSION 100 /* 0.1.0 */

/* gae_mode */
#define CRL_GAE_COMPAT 0 /* ppo.jl:66 loop k-1:-1:1, carry 0, slot k defined as 0 (upstream leaves it uninitialised) */
#define CRL_GAE_FIXED 1  /* loop from k with the bootstrap value (CleanRL-python semantics) */
/* env_kind */
#define CRL_ENV_CARTPOLE 0 /* CartPoleEnv(T=Float32, max_steps=500) ppo.jl:82 */
#define CRL_ENV_SYNTHETIC 1 /* stateless generator for shapes the reference has no env for: obs ~ U(-1,1)^d, reward ~ U(-1,1), done ~ B(1/200) */
#define CRL_ENV_EXTERNAL 2 /* envs stepped by the caller: crl_policy_act + crl_rollout_store */
#define CRL_ENV_MOUNTAINCAR 3 /* MountainCarEnv(T=Float32, max_steps=200): obs_dim=2, n_act=3; on-device, layer-wise path (parity unpinned: csrc/env.hpp) */
#define CRL_ENV_ACROBOT 4     /* AcrobotEnv(T=Float32, max_steps=200): obs_dim=6, n_act=3, RK4 "book" dynamics; on-device, layer-wise path (parity unpinned) */
/* shuffle mode */
#define CRL_SHUFFLE_FISHER_YATES 0 /* exact serial Fisher–Yates on device (ppo.jl:194 semantics) */
#define CRL_SHUFFLE_BIJECTION 1     /* perm[p] = keyed bijection of [0,B): O(1) per element, pseudo-random (throughput path) */
#define CRL_SHUFFLE_BLOCKED_FY 2    /* exact parallel shuffle: random split into ~64-element buckets + Fisher–Yates in each */
/* rollout / state fields for crl_ppo_read / crl_ppo_write */
enum crl_field {
  CRL_F_OBS = 0,      /* float  (obs_dim, nt, k)  replay_buffer.jl:15-18 / ppo.jl:96 */
  CRL_F_ACTION = 1,   /* int32  (nt, k) 0-based   ppo.jl:97  */
  CRL_F_LOGPROB = 2,  /* float  (nt, k)           ppo.jl:98  */
  CRL_F_REWARD = 3,   /* float  (nt, k)           ppo.jl:99  */
  CRL_F_TERMINAL = 4, /* uint8  (nt, k)           ppo.jl:100 */
  CRL_F_VALUE = 5,    /* float  (nt, k)           ppo.jl:101 */
  CRL_F_ADVANTAGE = 6,/* float  (nt, k)           ppo.jl:180 */
  CRL_F_RETURN = 7,   /* float  (nt, k)           ppo.jl:181 */
  CRL_F_PERM = 8,     /* int32  (nt*k) 0-based    ppo.jl:194 b_inds */
  CRL_F_PARAMS = 9,   /* float  (P)               ppo.jl:196 */
  CRL_F_GRADS = 10,   /* float  (P) gradient of the last minibatch (after all-reduce, before ClipNorm) ppo.jl:202 */
  CRL_F_ADAM_M = 11,  /* float  (P) */
  CRL_F_ADAM_V = 12,  /* float  (P) */
  CRL_F_ENV_STATE = 13, /* float (obs_dim, nt) env-internal state */
  CRL_F_CUR_OBS = 14,   /* float (obs_dim, nt) next_obs of ppo.jl:114,143 */
  CRL_F_NEXT_DONE = 15, /* uint8 (nt)          next_done of ppo.jl:115,144 */
  CRL_F_ENV_T = 16,     /* int32 (nt) steps since reset */
  CRL_F_BETAP = 17,     /* double (24) Adam running beta powers per array */
  CRL_F_ADV_SUMS = 18   /* double (num_minibatches, 2) Σadv, Σadv² of the current permutation slices (what the ranks all-reduce) */
};

/* Mirror of PPOConfig (ppo.jl:1-19) + the shapes the reference hard-codes (networks.jl:36, CartPole) */
typedef struct crl_ppo_config {
  int64_t total_timesteps;      /* ppo.jl:2 */
  int32_t num_steps;            /* ppo.jl:3 */
  int32_t num_envs;             /* ppo.jl:4  — envs owned by THIS handle (one data-parallel shard) */
  int32_t num_minibatches;      /* ppo.jl:5 */
  int32_t update_epochs;        /* ppo.jl:6 */
  float lr;                     /* ppo.jl:8 */
  float gamma;                  /* ppo.jl:9 */
  float gae_lambda;             /* ppo.jl:10 */
  float clip_coef;              /* ppo.jl:12 */
  float ent_coeff;              /* ppo.jl:13 */
  float v_coef;                 /* ppo.jl:14 */
  int32_t normalize_advantages; /* ppo.jl:16 — must be 1 (0 is an error upstream too, ppo.jl:219-222) */
  int32_t clip_value_loss;      /* ppo.jl:17 */
  int32_t anneal_lr;            /* ppo.jl:18 */
  int32_t obs_dim;              /* 4 */
  int32_t n_act;                /* 2 */
  int32_t hidden;               /* 64 (networks.jl:36) */
  int32_t gae_mode;             /* CRL_GAE_* */
  int32_t env_kind;             /* CRL_ENV_* */
  int32_t stale_obs;            /* 1 = ppo.jl:143-164 behaviour: policy sees the terminal obs after a reset */
  int32_t env_id_offset;        /* global id of local env 0 (rank * num_envs under data parallelism) */
  int32_t shuffle_mode;         /* CRL_SHUFFLE_* */
  uint64_t seed;
} crl_ppo_config;

/* "Training Statistics" record of ppo.jl:247, one per optimiser step */
typedef struct crl_ppo_stats {
  double loss, pg_loss, v_loss, entropy_loss;
  double adv_mean, adv_std, u_value, n_unclipped_wins;
} crl_ppo_stats;

/* "Episode Statistics" of ppo.jl:147-162 aggregated over one rollout */
typedef struct crl_episode_stats {
  double episodes, return_sum, length_sum, return_max;
} crl_episode_stats;

typedef struct crl_ppo crl_ppo;

int32_t crl_version(void);
const char* crl_last_error(void);
int32_t crl_device_count(int32_t* n);

/* ppo.jl:75-115 setup: buffers, optimiser state, env state — all resident in HBM on `device`. */
int32_t crl_ppo_create(const crl_ppo_config* cfg, int32_t device, crl_ppo** out);
int32_t crl_ppo_destroy(crl_ppo* h);
int32_t crl_ppo_param_count(const crl_ppo* h, int64_t* n);
int32_t crl_sync(crl_ppo* h);

/* `actor, critic = Networks.make_actor_critic(single_act_space, single_obs_space) .|> Flux.f32` — ppo.jl:87 / networks.jl:36-49: separate
 * actor and critic Dense(in,h,tanh_fast) → Dense(h,h,tanh_fast) → Dense(h,out), Flux.orthogonal weights with gains √2 / √2 / 0.01 (actor
 * head) and √2 / √2 / 1.0 (critic head), zero biases, as one flat float vector in Flux.params(actor, critic) order. Stateless, host-only
 * (runs without a GPU). The random stream is the library's own (seeded; Flux's task-local Xoshiro stream is not reproducible outside
 * Julia) — the distribution is the reference's. n must be the parameter count of the shape (crl_ppo_param_count). */
int32_t crl_make_actor_critic(int32_t obs_dim, int32_t n_act, int32_t hidden, uint64_t seed, float* out, size_t n);
/* ppo.jl:87 for a handle: crl_make_actor_critic for its shape, uploaded like a CRL_F_PARAMS write. A FRESH HANDLE HOLDS ALL-ZERO
 * PARAMETERS (h1 = h2 = 0: every gradient but the head biases' is zero for ever), so every entry point that computes with the networks —
 * crl_policy_act, crl_logprob_actions, crl_rollout_run, crl_ppo_update_minibatch, crl_ppo_iterate, crl_compute_gae in fixed mode —
 * returns an error ("parameters not set") until CRL_F_PARAMS has been written or this call has run. */
int32_t crl_ppo_init_params(crl_ppo* h, uint64_t seed);

/* Raw field access (parity tests, checkpointing, Julia-side inspection). nbytes must match the field size. */
int32_t crl_ppo_write(crl_ppo* h, int32_t field, const void* host, size_t nbytes);
int32_t crl_ppo_read(crl_ppo* h, int32_t field, void* host, size_t nbytes);

/* get_action(obs, actor) + critic(obs) — ppo.jl:21-32,127-128. obs (obs_dim,n) f32, u[n] uniform f64 in [0,1)
 * (the rand() of StatsBase.sample); outputs action[n] (0-based), logprob[n], value[n] (may be NULL). */
int32_t crl_policy_act(crl_ppo* h, const float* obs, const double* u, int32_t n, int32_t* action, float* logprob,
                       float* value);
/* logprob_actions(obs, actor, actions) — ppo.jl:34-45. entropy is the (n_act,n) matrix -p.*logp. */
int32_t crl_logprob_actions(crl_ppo* h, const float* obs, const int32_t* actions, int32_t n, float* logprob,
                            float* entropy);
/* gae.(eachrow(...)) — ppo.jl:48-73,173-181 on host arrays: value/reward (nt,k) f32, terminal (nt,k) u8,
 * next_value[nt], next_done[nt]; writes adv (nt,k) and ret (nt,k) (ret may be NULL). Stateless. */
int32_t crl_gae(int32_t device, const float* value, const float* reward, const uint8_t* terminal,
                const float* next_value, const uint8_t* next_done, int32_t nt, int32_t k, float gamma, float lambda,
                int32_t mode, float* adv, float* ret);
/* The same stateless call with the kernel-flavour switches a handle carries as options (gae_seg / gae_tile / gae_nt_loads of
 * crl_ppo_set_option): gae_tile = 4 forces the streaming kernel (serial Float64 recurrence, four envs per thread), 0 lets the size
 * decide; gae_nt_loads = 2 is crl_gae's own rule (nontemporal loads from 4 M samples). ppo.jl:48-73,173-181. */
int32_t crl_gae_opt(int32_t device, const float* value, const float* reward, const uint8_t* terminal,
                    const float* next_value, const uint8_t* next_done, int32_t nt, int32_t k, float gamma, float lambda,
                    int32_t mode, float* adv, float* ret, int32_t gae_seg, int32_t gae_tile, int32_t gae_nt_loads);

/* Buffer.add!(rb, transition) — replay_buffer.jl:23-37 / ppo.jl:133-140, external-env path: slot = step (0-based). */
int32_t crl_rollout_store(crl_ppo* h, int32_t step, const float* obs, const int32_t* action, const float* logprob,
                          const float* reward, const uint8_t* terminal, const float* value);

/* reset!(env); next_obs = state(env) — ppo.jl:112-115 for the on-device vectorised env. */
int32_t crl_env_reset(crl_ppo* h);
/* The whole `for step in 1:num_steps` loop — ppo.jl:123-166 — in one launch (on-device env + policy + sampling). */
int32_t crl_rollout_run(crl_ppo* h);
/* env(actions) + reward / is_terminated / state + reset!(env) of the terminated — ppo.jl:130-165 without the policy: steps the handle's on-device envs
 * with the caller's actions; gstep keys the reset stream like step `gstep` of the training loop. Outputs may be NULL. Leaves the rollout buffer alone.
 * action[num_envs] 0-based (out of range is an error); next_obs (obs_dim, num_envs) is what CRL_F_CUR_OBS holds afterwards (stale_obs decides whether a
 * terminated env shows its last or its fresh state); CRL_F_ENV_STATE / CRL_F_ENV_T / CRL_F_NEXT_DONE advance, the episode counters and statistics do
 * not. CRL_ENV_CARTPOLE, CRL_ENV_MOUNTAINCAR and CRL_ENV_ACROBOT on both paths; an error for CRL_ENV_SYNTHETIC (stateless) and CRL_ENV_EXTERNAL. */
int32_t crl_env_step(crl_ppo* h, const int32_t* action, uint64_t gstep, float* next_obs, float* reward, uint8_t* done);
/* Held-out evaluation of the current policy — no reference counterpart (ppo.jl only ever sees the returns of its training rollouts): the handle's
 * actor, with frozen parameters, runs on a fresh, private set of cfg->num_envs on-device envs of the handle's env_kind until EVERY env has finished
 * cfg->episodes_per_env episodes (the first N episodes of each env, not the first N to finish: short episodes are not over-represented), in ONE launch
 * (csrc/eval.hip). The trajectory is the one a twin handle of the same shape with num_envs = cfg->num_envs, seed = cfg->seed, env_id_offset = 0 and
 * stale_obs = 0 sees under crl_env_reset followed by crl_env_step(actions, gstep = g), g = 0, 1, 2, …, where the action of env e at step g comes from
 * the actor's logits at the twin's CRL_F_CUR_OBS: CRL_EVAL_GREEDY = the lowest index of the largest logit; CRL_EVAL_SAMPLE = get_action's sampler
 * (ppo.jl:21-32) on the uniform of Philox stream 0 of (cfg->seed, e, g) — the draw a training rollout takes at step g of iteration 0. An episode's
 * return is the Float32 running sum of its rewards in step order (ppo.jl:145), its length its step count; an env that has finished its quota stops.
 * returns / lengths: (episodes_per_env, num_envs), env fastest; either may be NULL. trace_action: (trace_steps, num_envs), the action taken at each of
 * the first trace_steps steps, -1 once the env had finished its quota; NULL exactly when trace_steps = 0 (it exists so that tests can follow the
 * device's trajectory). The report is computed on the host in Float64 from the per-episode arrays, sums in array order: return_std is the population
 * standard deviation, env_steps = Σ lengths. Reads CRL_F_PARAMS and nothing else of the handle — rollout buffer, env state, CRL_F_CUR_OBS, episode
 * statistics and ring, iteration counter, optimiser state, options, a pending crl_ppo_iterate_async report and the communicator stay as they are (under
 * data parallelism every rank evaluates locally) — but, like every entry point that reads state, it first closes an open guard window, refuses a handle
 * whose parameters were never set, and synchronises before it returns. Every episode ends by itself (CartPole after at most 501 steps — RLEnvs ends it
 * at t > max_steps = 500 —, the other two after 200), so the launch is bounded by episodes_per_env times that. Errors: NULL cfg / report, num_envs or
 * episodes_per_env < 1, unknown mode, trace_steps < 0 or without a trace_action, CRL_ENV_SYNTHETIC / CRL_ENV_EXTERNAL, and sizes past the caps:
 * num_envs <= 1048576, episodes_per_env <= 4096, num_envs * episodes_per_env <= 16777216, trace_steps * num_envs <= 67108864. Device scratch is
 * allocated on first use, kept on the handle and freed by crl_ppo_destroy. */
#define CRL_EVAL_GREEDY 0
#define CRL_EVAL_SAMPLE 1
typedef struct crl_eval_config { int32_t num_envs, episodes_per_env, mode, trace_steps; uint64_t seed; } crl_eval_config;
typedef struct crl_eval_report { int64_t episodes, env_steps; double return_mean, return_std, return_min, return_max, length_mean; } crl_eval_report;
int32_t crl_ppo_evaluate(crl_ppo* h, const crl_eval_config* cfg, crl_eval_report* report, float* returns, int32_t* lengths, int32_t* trace_action);
/* Diagnostics of the update — no reference counterpart (ppo.jl:247 logs its four losses and nothing else): approximate KL between the behaviour policy
 * and the current one, clip fraction, policy entropy and the critic's explained variance, from ONE read-only, forward-only launch (csrc/diag.hip) over
 * whatever the resident rollout buffer currently holds — CRL_F_OBS, CRL_F_ACTION, CRL_F_LOGPROB, CRL_F_VALUE, CRL_F_RETURN — with the handle's CURRENT
 * CRL_F_PARAMS: after crl_ppo_iterate that is the last rollout against the post-update parameters; after crl_rollout_run + crl_compute_gae, the rollout
 * against the parameters that drew it (approx_kl ≈ 0, clipfrac = 0). Per sample b (flat index e + num_envs * t): lp_new = logsoftmax(actor(obs_b))[action_b]
 * (ppo.jl:34-45), H_b = Σ_a -p_a * log p_a from the Float32 elements of the reference's entropy matrix added in index order, v_new = critic(obs_b),
 * logratio = lp_new - logprob_b as a Float32 difference (ppo.jl:224); from there on Float64: r = logratio, ratio = exp(r), kl_b = (ratio - 1) - r,
 * clipped_b = |ratio - 1| > (double)clip_coef. The forward is the same for every handle: W2 as bf16x3 (24-bit operands) with Float32 accumulation, NNlib's
 * rational tanh_fast; no option (gemm, wide_gemm, wide_*) changes a bit of the result. The raw sums are part of the struct so that data-parallel ranks (or
 * the host) can add their shards' reports field by field (n, n_clipped and the sum_* fields; min / max of the ratio_* fields) and apply the formulas below;
 * the call itself is local to the shard, like crl_ppo_evaluate. With mean(s) = s / n:
 *   old_approx_kl = -sum_logratio / n          approx_kl = sum_kl / n          clipfrac = n_clipped / n
 *   entropy = sum_entropy / n — the policy entropy PER SAMPLE: n_act times the reference's entropy_loss (crl_ppo_stats), which is the mean over all
 *             n_act * n elements of the (n_act, B) matrix
 *   explained_variance = 1 - Var(ret - value) / Var(ret), Var(x) = sum_x2 / n - (sum_x / n)^2 (population variances, sum_res_old* = Σ(ret - value),
 *             Σ(ret - value)^2 in Float64); NaN when Var(ret) is not positive (constant returns)
 *   explained_variance_new = the same with v_new in place of value (sum_res_new*)
 * Every block of the launch adds its samples in Float64 and the host adds the blocks' records in block order: two calls on the same state return the
 * same bits. new_logprob / new_value: (num_envs, num_steps) host arrays receiving lp_new / v_new, either may be NULL (they exist so that tests can
 * locate a wrong tile; NULL = the launch stores nothing per sample). Works for every env_kind — CRL_ENV_EXTERNAL and CRL_ENV_SYNTHETIC included, no env
 * is stepped — and both paths: obs 4 / act 2 / hidden 64 and every layer-wise shape (obs_dim <= 64, n_act <= 16, hidden 64 / 128 / 256). Reads the buffer
 * and CRL_F_PARAMS and changes nothing: env state, permutations, records, optimiser state, options, a pending crl_ppo_iterate_async report and the
 * iteration counter stay as they are; like every entry point that reads state it first closes an open guard window, refuses a handle whose parameters
 * were never set, and synchronises before it returns. Errors: NULL h or out. Device scratch (one record per block, the two per-sample arrays when asked
 * for) is allocated on first use, kept on the handle and freed by crl_ppo_destroy. crl_ppo_get_option("diag_last_ns") (read-only) is the HIP-event time
 * of the last call's launch. */
typedef struct crl_ppo_diag {
  int64_t n, n_clipped;
  double sum_logratio, sum_kl, sum_entropy, ratio_min, ratio_max;
  double sum_ret, sum_ret2, sum_res_old, sum_res_old2, sum_res_new, sum_res_new2;
  double old_approx_kl, approx_kl, clipfrac, entropy, explained_variance, explained_variance_new;
} crl_ppo_diag;
int32_t crl_ppo_diagnose(crl_ppo* h, crl_ppo_diag* out, float* new_logprob, float* new_value);
/* return_max is the largest return among the rollout's finished episodes, 0 when none finished. (CRL_ENV_CARTPOLE / CRL_ENV_SYNTHETIC keep their
 * historical max(0, ·): CartPole's returns are >= 0 anyway.) */
int32_t crl_episode_stats_read(crl_ppo* h, crl_episode_stats* out);
/* Per-episode records of the last rollout (the fields of ppo.jl:157's "Episode Statistics"): off by default; once enabled
 * every episode end appends {return, length, global env id, step of the rollout} to a device ring of `capacity` records
 * (episodes beyond that are counted, not stored). Records come back in arrival order — sort by (step, env) for the
 * reference's logging order (ppo.jl:147-165 walks the done envs of one step in ascending order). The ring holds the LAST rollout only:
 * when a speculation guard window is replayed (crl_ppo_exact_reruns), the records are those of the replayed rollouts — the
 * speculative ones they overwrite are not kept. */
typedef struct crl_episode_record { float episode_return; int32_t episode_length; int32_t env; int32_t step; } crl_episode_record;
int32_t crl_episode_ring_enable(crl_ppo* h, int32_t capacity);
int32_t crl_episode_ring_read(crl_ppo* h, crl_episode_record* out, int32_t max_records, int32_t* n_stored, int64_t* n_episodes);
/* bootstrap + advantages + returns — ppo.jl:169-181 — on the resident buffer. */
int32_t crl_compute_gae(crl_ppo* h);
/* b_inds = shuffle(b_inds) — ppo.jl:194. epoch_id keys the counter-based stream. */
int32_t crl_shuffle(crl_ppo* h, uint64_t epoch_id);
/* per-minibatch advantage mean/std of the current permutation (ppo.jl:221), all num_minibatches at once;
 * all-reduced across ranks when a communicator is attached. Must follow crl_shuffle / a CRL_F_PERM write. */
int32_t crl_adv_stats(crl_ppo* h);
/* The two halves of crl_adv_stats for hosts that run the exchange themselves (and for the single-GPU test of the
 * data-parallel arithmetic): local sums → CRL_F_ADV_SUMS, then mean/std from whatever CRL_F_ADV_SUMS holds. */
int32_t crl_adv_stats_local(crl_ppo* h);
int32_t crl_adv_stats_finish(crl_ppo* h);
/* One `for start in 1:minibatch_size:batch_size` body — ppo.jl:197-251: loss, gradient, (all-reduce), per-array
 * ClipNorm(0.5) + Adam(eta). apply_update=0 stops after the gradient (parity tests). stats may be NULL (no sync). */
int32_t crl_ppo_update_minibatch(crl_ppo* h, int32_t mb, double eta, int32_t apply_update, crl_ppo_stats* stats);
/* n_iters passes of the ppo.jl:117-253 loop body, fully on device. stats (may be NULL) receives
 * update_epochs*num_minibatches records of the LAST iteration. */
int32_t crl_ppo_iterate(crl_ppo* h, int32_t n_iters, crl_ppo_stats* stats);
int32_t crl_ppo_iteration(const crl_ppo* h, int64_t* it);
/* The same loop body for a host that LOGS every update — ppo.jl:147-165 ("Episode Statistics") and :246-248 ("Training Statistics") — without making the GPU wait for
 * it. crl_ppo_iterate_async enqueues ONE iteration and hands back the records of the iteration BEFORE it (prev->iteration = its 0-based index; -1 on the first
 * call): at the end of every iteration one launch gathers its update_epochs * num_minibatches loss records, its episode statistics, its per-episode ring
 * (crl_episode_ring_enable; prev_ring receives up to max_ring records in arrival order), the value-loss speculation flag and the error words into a slot that
 * travels to pinned host memory on the stream; the host picks it up one call later, behind the launches of the next iteration. A host loop logs one iteration late
 * — the record stream (names, keys, order, global_step) is the reference's — and ends with crl_ppo_drain, which returns the last iteration's records (iteration =
 * -1: nothing pending). A failed speculation seen in a slot repeats the guard window exactly before the records are handed out, like every other read-back.
 * Measured against crl_ppo_iterate(h, 1, stats) + crl_episode_stats_read per update: 10.45 -> 10.21 ms per iteration at 65536 envs, 2.04 -> 1.86 at 8192, 1.65 -> 1.45 at 4096
 * (scripts/readback_cost.py). prev_stats may be NULL; the blocked shuffle limits update_epochs to 8 here. */
typedef struct crl_ppo_iteration_report {
  int64_t iteration;            /* which iteration the records belong to, -1 = none */
  crl_episode_stats episodes;   /* ppo.jl:147-162 aggregated over its rollout */
  int64_t n_episodes;           /* episodes that ended in its rollout */
  int32_t n_ring;               /* per-episode records copied to prev_ring */
  int32_t pad;
} crl_ppo_iteration_report;
int32_t crl_ppo_iterate_async(crl_ppo* h, crl_ppo_iteration_report* prev, crl_ppo_stats* prev_stats, crl_episode_record* prev_ring, int32_t max_ring);
int32_t crl_ppo_drain(crl_ppo* h, crl_ppo_iteration_report* last, crl_ppo_stats* last_stats, crl_episode_record* last_ring, int32_t max_ring);

/* ---- Device-resident external envs (csrc/extenv.hip): CRL_ENV_EXTERNAL for a simulator that lives on the handle's GPU (a torch-ROCm tensor env,
 * AMDGPU.jl arrays, the caller's own HIP kernels). Every `_d` pointer below is DEVICE memory on the handle's device; nothing is staged, the calls only
 * enqueue work on the handle's stream and never make the host wait (the one exception is stated at crl_ppo_update). The host-pointer pair
 * crl_policy_act + crl_rollout_store keeps working unchanged next to them.
 * The peer_stream rule, the same for every call that takes one. NULL (or the handle's own stream): the caller orders its work itself — it runs on the
 * stream of crl_ppo_stream, or it has synchronised. Any other hipStream_t: before its launch the call makes the handle's stream wait for everything
 * enqueued on peer_stream so far, and after its launch it makes peer_stream wait for that launch — an event record plus hipStreamWaitEvent each way, the
 * two events created once and kept on the handle. */
/* The handle's hipStream_t (non-blocking): run the env on it, or order another stream against it. */
int32_t crl_ppo_stream(crl_ppo* h, void** stream);
/* ppo.jl:127-128 plus the state / action / logprob / terminal / value fields of Buffer.add! (:133-140) in ONE launch: for env e, actor logits and critic
 * value of obs_d (obs_dim, num_envs), get_action's sampler (ppo.jl:21-32) on the uniform of Philox stream 0 of (seed, env_id_offset + e,
 * iteration * num_steps + step) — the draw every on-device rollout kernel takes for that env and step —, the 0-based action to action_d[e], and obs,
 * action, logprob, value and terminal = done_d[e] (next_done of ppo.jl:115,144) into slot `step` of the resident buffer. The forward is the one of
 * the diagnostics launch for every handle: W2 as bf16x3 with Float32 accumulation, NNlib's rational tanh_fast; no option changes a bit of it. step = 0
 * starts a rollout: the episode statistics and the ring count are cleared on the stream first. Shapes: obs_dim <= 64, n_act <= 16, hidden 64 / 128 / 256.
 * Errors: NULL pointers, step outside 0 … num_steps - 1, parameters never set. */
int32_t crl_rollout_act_device(crl_ppo* h, int32_t step, const float* obs_d, const uint8_t* done_d, int32_t* action_d, void* peer_stream);
/* ppo.jl:132,137,143-165 in one small launch: reward_d[num_envs] into slot `step`; CRL_F_CUR_OBS / CRL_F_NEXT_DONE <- next_obs_d (obs_dim, num_envs) /
 * next_done_d[num_envs] (what the fixed-mode bootstrap of crl_compute_gae reads); per env episode_length += 1 and episode_return += reward as a Float32
 * running sum in step order; where next_done is set the episode is added to the statistics of crl_episode_stats_read, appended as
 * {return, length, env_id_offset + e, step} to the ring of crl_episode_ring_enable, and the two accumulators restart at zero. The statistics are Float64
 * sums of the Float32 returns, added per wave and then atomically (exact, hence order-free, as long as the returns' binary exponents span less than
 * 29 - log2(episodes) bits); return_max is the true signed maximum, 0 when no episode ended. Errors: NULL pointers, step out of range. */
int32_t crl_rollout_record_device(crl_ppo* h, int32_t step, const float* reward_d, const float* next_obs_d, const uint8_t* next_done_d, void* peer_stream);
/* crl_env_step without the staging — one handle's built-in env as another handle's external env, entirely on device (ppo.jl:130-165 without the policy).
 * action_d / reward_d / done_d [num_envs] and next_obs_d (obs_dim, num_envs; may be NULL: CRL_F_CUR_OBS holds it) are device memory. An action outside
 * 0 … n_act - 1 leaves its env unstepped and raises a sticky device word instead of being read back here: the next crl_sync on this handle returns the
 * error and lowers the word. CRL_ENV_CARTPOLE, CRL_ENV_MOUNTAINCAR and CRL_ENV_ACROBOT. */
int32_t crl_env_step_device(crl_ppo* h, const int32_t* action_d, uint64_t gstep, float* next_obs_d, float* reward_d, uint8_t* done_d, void* peer_stream);
/* ppo.jl:168-253 on whatever the resident buffer holds — the loop body of crl_ppo_iterate without its rollout launch: bootstrap + GAE, all epoch
 * permutations, advantage statistics, update_epochs * num_minibatches optimiser steps with the annealed eta of the current iteration, then the
 * iteration counter advances. Every env_kind. On the 4 / 2 / 64 path the call is a value-loss speculation guard window of its own (see
 * crl_ppo_exact_reruns): snapshot, update phase, one read of the flag — the ONE host synchronisation of the device-pointer path, once per num_steps step
 * launches — and, when the speculation failed, the snapshot restored and the update phase repeated exactly; no rollout is replayed. The layer-wise path
 * does not synchronise. stats (may be NULL; non-NULL synchronises) receives the update_epochs * num_minibatches records of this update. Single rank
 * only: with an RCCL, peer or external communicator attached the call returns an error (multi-rank external envs are not supported). */
int32_t crl_ppo_update(crl_ppo* h, crl_ppo_stats* stats);
/* how many iterations had their update phase re-run with the exact value-loss pass under data parallelism: the fused
 * kernels speculate on u = mean(v - R^2) <= 0 (ppo.jl:232-237); with an RCCL communicator a failed speculation restores the
 * parameters / Adam state of the iteration's start and repeats its optimiser steps exactly (two more small all-reduces each) */
int32_t crl_ppo_exact_reruns(const crl_ppo* h, int64_t* n);

/* Data parallelism over num_envs: one RCCL communicator per handle (one process per GPU). The 128-byte id comes
 * from crl_comm_unique_id on rank 0 and is broadcast by the host launcher. Gradients (+ advantage statistics) are
 * all-reduced once per optimiser step (ppo.jl:250 cadence) and averaged; ClipNorm/Adam then run replicated. */
int32_t crl_comm_unique_id(uint8_t id[128]);
int32_t crl_comm_init(crl_ppo* h, const uint8_t id[128], int32_t world_size, int32_t rank);
/* Which RCCL the exchange runs on: the file the loaded ncclAllReduce lives in (dladdr; NUL-terminated into path[0..path_cap)) and ncclGetVersion's
 * code (e.g. 22203). Loads librccl if it is not loaded yet; stateless. A launcher records it per rank (bench.py: comm.rccl_path / rccl_version)
 * so that a multi-GPU run shows that every rank — and a host framework that maps its own copy — uses one library. No reference counterpart. */
int32_t crl_comm_info(char* path, size_t path_cap, int32_t* version);
/* The same data-parallel exchange without RCCL: a one-shot all-reduce over peer-mapped mailboxes (csrc/peer.hip) — every rank
 * pushes its message into every peer's mailbox over xGMI and adds the world_size slots in rank order, one launch per message
 * (the 36.6 KB gradient message of a 3 ms shard iteration is latency-bound on a ring). crl_comm_peer_export allocates this
 * rank's mailbox and returns its 64-byte hipIpcMemHandle_t; the host launcher all-gathers the handles (that all-gather is the
 * barrier the protocol needs) and hands all world_size * 64 bytes, in rank order, to crl_comm_peer_attach. world_size <= 16;
 * ranks may share a GPU (that is how a 1-GPU box runs the multi-rank tests). A rank that stops answering raises a sticky
 * time-out error (option peer_timeout_ms, default 20000) reported by crl_sync / crl_ppo_iterate instead of hanging the GPU. */
int32_t crl_comm_peer_export(crl_ppo* h, int32_t world_size, int32_t rank, uint8_t handle[64]);
int32_t crl_comm_peer_attach(crl_ppo* h, const uint8_t* handles);
/* Declares this handle one of `world_size` shards WITHOUT attaching a communicator: every 1/M uses the global
 * minibatch size and the host sums the per-shard gradient messages (CRL_F_GRADS) itself. */
int32_t crl_comm_init_external(crl_ppo* h, int32_t world_size, int32_t rank);

/* Detaches whatever exchange is attached (RCCL communicator, peer mailboxes, or the external-exchange declaration) and returns the
 * handle to a single-shard configuration; a launcher uses it to fall back from a partially failed RCCL initialisation to the peer
 * all-reduce (cleanrl.jl_amd/dist.py: attach_comm). No reference counterpart (the reference is single-process). */
int32_t crl_comm_destroy(crl_ppo* h);

/* Per-handle options: every switch that selects a kernel flavour or changes numerics (earlier rounds: process-wide CRL_*
 * environment variables). Integer-valued, by name; unknown names and out-of-range values are errors. The defaults are what
 * bench.py measures. crl_ppo_option_count / crl_ppo_option_name enumerate them.
 *   gemm                    2 = 64x64 products as fp16x2 split operands (default); 1 = bf16x3 everywhere — the fallback flavour, which
 *                           a launch also takes by itself, per role, when a hidden-layer weight leaves the fp16 window (|w| >= 255, or all of a network's |w| < 2^-11)
 *   rollout_split (4)       small-shard rollout kernel, waves per 32-env tile: 4 = by size (default) — six (the actor's hidden rows over four waves on 16x16x32 products,
 *                           the critic's over two: rollout_split6_kernel) for shards up to rollout_split_max_tiles; 3 = six, 1 = three, 2 = two, 0 = one
 *   rollout_split_max_tiles largest shard, in 32-env tiles, the split kernels take (512)
 *   rollout_stagger         start delay of waves 4-7 of an 8-wave rollout block, units of 1024 clocks (6)
 *   gae_fuse                1 = inside crl_ppo_iterate the compat-mode GAE is the tail of the rollout kernel (default), 0 = own launch
 *   shuffle_overlap         1 = epoch permutations are drawn on a second stream next to the rollout (default)
 *   guard_window            iterations crl_ppo_iterate enqueues between two read-backs of the value-loss speculation flag (8)
 *   update_stagger, actor_block_pct   launch-shape knobs of the update pass (3, 53)
 *   adv_seq (1)             per-minibatch advantage sums of crl_ppo_iterate: 1 = one sequential pass over the advantages that finds a sample's minibatch through
 *                           the blocked shuffle's bucket table, with the bucket digit the shuffle stored per sample and epoch; 2 = the same with the digit
 *                           recomputed (one Philox call per sample and epoch); 0 = gathers through the finished permutations
 *   comm_force              1 = crl_comm_init with world_size 1 still creates an RCCL communicator (1-GPU test of that path)
 *   peer_timeout_ms         in-kernel time-out of the peer all-reduce (20000)
 *   wide_gemm               layer-wise path, 256-wide layers: 2 = fp16x2 (default), 1 = bf16x3, 0 = f32 MFMA. fp16x2 stages W2 under ONE power of two
 *                           per network, taken from its largest |w|, and the observations of the h1 that wide_fuse = 3 regenerates in the weight gradient
 *                           under one per 32-sample slab: magnitude is free, DYNAMIC RANGE is not, and nothing detects it (no fallback, no flag). Within
 *                           1e-5 of Float64 up to a ratio of 2^16 between the largest W2 weight and the bulk, and between a sample's observations and the
 *                           largest of its slab; measured past that (tests/test_gpu_wide_range.py): 1.2e-5 / 1.9e-4 on the gradient and 6e-5 / 9e-4 on
 *                           values next to one weight of 2^20 / 2^24 among weights of 0.06, 3.5e-5 / 8e-3 / 1.2 on dW2 at an observation ratio of
 *                           2^24 / 2^32 / 2^40. wide_gemm = 1 and 0 have no such limit; set one of them for networks or observations like that
 *   wide_tanh_rational      1 = the layer-wise path evaluates NNlib's rational tanh_fast everywhere (default 0), saturating to exactly ±1 at x² >= 66 in the
 *                           forward of the update pass, whose 1 − h² the backward multiplies by the next layer's weights. The default is the exp2 form
 *                           1 − 2 / (2^(2·log2(e)·x) + 1) outside the actor's rollout forward, under every wide_gemm: ≈ 3e-8 ABSOLUTE near 0, where tanh_fast
 *                           is accurate relative to |x|. A hidden unit of size 2^-k carries that as 2^(k − 25) of itself: with first-layer activations of
 *                           2^-8 the weight gradient of the second layer is 5.5e-5 from Float64, 8e-4 at 2^-12, 1.5e-2 at 2^-16 (observations that small
 *                           with zero biases; tests/test_gpu_wide_range.py), and this option is what meets 1e-5 there
 *   gae_seg, gae_tile       standalone GAE kernel: steps per segment (8 / 16; 4 / 8 / 16 = window depth of the streaming kernel) / kernel shape, 0 = automatic:
 *                           gae_tile = 8 / 16 / 32 / 64 the segmented kernel with that many envs per block; 128 / 256 its two-envs-per-thread form (32 / 64 env
 *                           pairs per block, 8-byte accesses: what 4096 envs or more take by themselves when num_envs is even); 4 / 2 / 1 the streaming kernel
 *                           (that many envs per thread, serial Float64 recurrence: what batches of 33 M samples or more with >= 262144 envs take by themselves)
 *   gae_nt_loads (2)        standalone GAE kernel: 1 = nontemporal input loads (inputs not in the caches), 0 = cached, 2 = 1 for an external env with 4 M samples or more per rollout, else 0
 *   wide_rollout_persist (2)  layer-wise path, 2x256 fp16x2, obs_dim <= 16: the whole rollout as one launch — 2 = producer / consumer form (64 envs per
 *                           block, weight slabs by LDS-DMA, layer 1 on the matrix pipe; num_envs % 64 == 0, n_act <= 8, else 1), 1 = the first
 *                           one-launch kernel (32 envs per block), 0 = three launches per step
 *   update_xcd_align (1)    update kernel: tile t is worked on by blocks ≡ t (mod 8) of both roles (same XCD / L2 for a record's two readers)
 *   update_prio_small (0)   update kernel, launches with fewer than 16 tiles per wave (shards of 8192 envs and below): wave-priority rule of a
 *                           wave pair on one SIMD — 0 none (default), 1 the large-launch feedback rule, 2 static (younger wave first), 3 alternate
 *                           per tile.  Measured: 3 is -1..-2 % at 8192 envs and +1 % at 4096, the others neutral or worse
 *   wide_fuse (3)           layer-wise path, 2x256 fp16x2, obs_dim <= 16: the update pass runs the tile-resident fused kernels (csrc/wide_fused.hpp):
 *                           3 = forward, backward and a weight-gradient kernel that regenerates h1 (h1 is never stored), 2 = forward and backward,
 *                           1 = forward only, 0 = one launch per layer
 *   wide_wgrad_full (1)     the h1-regenerating weight-gradient kernel: 1 = one 256x256 tile per block, δ2 read once (default); 0 = 256x128 output tiles
 *   wide_fuse_pc (1)        the fused forward in its producer / consumer form (four MFMA-only waves, four staging waves, persistent blocks); 0 = the
 *                           symmetric first version
 *   wide_fwd_wbufs (2)      the producer / consumer forward's weight buffers in LDS: 2 = the producers fetch the next slab (default); 3 = the consumers fetch
 *                           the weight slab AFTER NEXT behind their own MFMAs (two slabs of lead for the LDS-DMA; n_act <= 6) — measured equal (DESIGN §3b:
 *                           the slab loop is bound by the SIMD's vector-issue slots, of which an LDS-DMA piece takes ~100-140 cycles whoever issues it)
 *   wide_d2_split (1)       wide_fuse = 3 with wide_wgrad_full = 1: the backward kernel hands δ2 to the weight-gradient kernel as the fp16x2 pieces it makes for
 *                           its own product (two f16 planes, one power-of-two scale per sample; the same bytes as the f32 array) and the weight-gradient kernel
 *                           multiplies straight from them (LDS-DMA + transposing LDS reads, no conversion); 0 = δ2 as f32, split again by its reader
 *   wide_rs (27)            2x256 fp16x2, register-stationary kernels (csrc/wide_rs.hpp: a network's 256 KB of W2 pieces live in the eight waves' registers
 *                           for the whole launch, nothing but the 32-sample activation tile moves): bit 0 = the update pass's forward (wide_rs_fwd_kernel,
 *                           obs_dim a multiple of 4; else the producer / consumer kernel), bit 1 = the rollout (wide_rs_rollout_kernel: the actor in the
 *                           step loop, env state in LDS; the critic as ONE batched forward over the stored observations behind it — ppo.jl:128 evaluates it
 *                           on the observation the buffer keeps), bit 2 = that critic pass on the register-stationary forward instead of the producer /
 *                           consumer kernel (measured slower), bit 3 = the update pass's backward (wide_rs_bwd_kernel: W2ᵀ stationary as the B operand, h2 /
 *                           δ3 / observations by LDS-DMA, layer 1 recomputed on the matrix pipe; with wide_d2_split = 1, obs_dim a multiple of 4), bit 4 = that kernel
 *                           also forms dW3 (h2 and δ3 are on chip: the two sweeps over h2 — 1.07 GB per optimiser step — are not launched); 0 = round 5's kernels
 *   wide_rs_actor_pct (52)  register-stationary backward: share of the CUs whose blocks take the actor's tiles (its δ2 staging costs n_act head rows against the
 *                           critic's one): 676 / 666 / 679 / 717 µs per launch at 50 / 52 / 54 / 56 % (C3)
 *   update_tile (0)         update pass of the 4 / 2 / 64 path: 32 = 32-sample tiles (update_x2_kernel), 16 = 16-sample tiles at three waves per SIMD (update16.hpp: one early-exit
 *                           repair launch redoes a minibatch as bf16x3 when a tile misses the carried weight-gradient scale or a weight leaves the fp16 window; 17 = the same with
 *                           every tile reporting a miss: test hook), 0 = by launch size — which currently means 32 everywhere: the 16-sample kernel measured slower at every
 *                           size it was built for (profiles/r06_update_tile16_ab.txt)
 *   fuse_optim (1)          speculative step of the 4 / 2 / 64 path: gradient reduction + ClipNorm + Adam as ONE launch (reduce_optim_kernel; 0 = two launches) — on one
 *                           GPU, and under data parallelism over the peer mailboxes, where the same launch also runs the exchange (reduce -> push -> wait ->
 *                           rank-order sum -> ClipNorm + Adam). Taken only where the launch's whole grid can be resident (checked at crl_ppo_create) and never
 *                           with an RCCL communicator, a host-side exchange or the inline value-loss fix-up
 * Read-only through crl_ppo_get_option: gemm_fallback_seen (1 once any launch of the fused 4/2/64 path took the bf16x3 fallback; the
 * layer-wise path needs none: it scales its fp16x2 weight pieces by the largest |w| of the layer at every optimiser step);
 * dw_scale_log2_actor / dw_scale_log2_critic (log2 of the power-of-two weight-gradient scale G that the next fp16x2 update launch of
 * that role uses: predicted from the previous launch's largest |δ2|, kept while it fits, clamped to [-100, 100]; see mlp_x2.hpp. Under
 * gemm = 1 no launch reads or moves it: the value is the one the next fp16x2 launch starts from. An error on a layer-wise handle, which
 * carries no such scale).
 * The environment variable CRL_OPTIONS="key=value,key=value" applies options at crl_ppo_create (shell-driven experiments). */
int32_t crl_ppo_set_option(crl_ppo* h, const char* key, int64_t value);
int32_t crl_ppo_get_option(crl_ppo* h, const char* key, int64_t* value);
int32_t crl_ppo_option_name(int32_t index, const char** name, int64_t* dflt);
int32_t crl_ppo_option_count(int32_t* n);   /* number of options: enumerate with crl_ppo_option_name(0 … n-1) */

/* Profiling: HIP-event timing of each kernel class on the handle's stream (bench.py roofline). on = 1: every class, events
 * recorded around the launches (extra packets between dependent kernels: a breakdown, not a throughput run); on = 2: only the
 * classes whose events ride on the dispatch itself — the update kernel of the fused path — which costs nothing, plus the gradient
 * all-reduces of a data-parallel run (recorded events: 32 packets per iteration); 0 = off. */
enum crl_kernel_id { CRL_K_ROLLOUT = 0, CRL_K_GAE = 1, CRL_K_SHUFFLE = 2, CRL_K_ADV_STATS = 3, CRL_K_UPDATE = 4,
                     CRL_K_REDUCE = 5, CRL_K_OPTIM = 6, CRL_K_ALLREDUCE = 7, CRL_K_PACK = 8, CRL_K_PERMUTE = 9,
                     CRL_K_COUNT = 10 };
/* Measurement entry (bench.py roofline_gae.beyond_cache, scripts/bench_gae.py): the standalone GAE scan (the kernel behind crl_gae /
 * crl_compute_gae, ppo.jl:48-73,173-181) on synthetic device-resident inputs of ANY size — value ~ U(-10,10), reward 0 with P 0.02,
 * terminal ~ B(0.02) — `reps` timed launches (HIP events on the dispatch), each followed by a timed launch of a hand-written float4
 * streaming copy that moves the same number of bytes (17 B per (env,step) + 5 B per env; half read, half written): the ceiling.
 * seg / tile / nt_loads as the options gae_seg / gae_tile / gae_nt_loads (0 / 0 / 0 or 1); flush_mb > 0 fills that many MiB before
 * every timed launch (sizes that fit the 256 MiB Infinity Cache); gae_ms / copy_ms receive `reps` values each. */
int32_t crl_gae_bench(int32_t device, int32_t nt, int32_t k, int32_t seg, int32_t tile, int32_t nt_loads, int32_t flush_mb,
                      int32_t reps, double* gae_ms, double* copy_ms);
/* Measurement entry (bench.py `clock`): the shader clock the GPU sustains under vector load — one 8-wave block per CU runs independent v_fma_f32 chains
 * for span_ms of the constant 100 MHz counter (s_memrealtime) and reports shader cycles (s_memtime) per microsecond: median / min / max over all waves,
 * in MHz. Boxes of one pool differ by more than a round's kernel work moves the headline; a line that carries its own clock can be normalised. */
int32_t crl_clock_probe(int32_t device, double span_ms, double* median_mhz, double* min_mhz, double* max_mhz);
/* Measurement entry (scripts/product_error.py → profiles/<tag>_product_error.json): C = A·B for the same Float32 host operands through every way the
 * hidden-layer products of networks.jl:6-13 could be multiplied on this GPU — flavour 0 = fp16x2 split operands (the default of option gemm; scale_a,
 * scale_b or a per-column col_scale[cols] are the exact powers of two the production kernels use), 1 = bf16x3 (gemm = 1), 2 = v_mfma_f32_32x32x2_f32,
 * 3 = a sequential v_fma_f32 chain per element (a scalar f32 matmul) — so that their errors against a Float64 product can be compared on real operands.
 * A [rows][K] row-major, B [cols][K]; K is cut into `chunks` pieces with one f32 accumulator each: C [chunks][cols][rows]. rows / cols multiples of 32,
 * K / chunks a multiple of 16. */
int32_t crl_product_probe(int32_t device, int32_t flavour, const float* A, const float* B, int32_t rows, int32_t cols, int32_t K, int32_t chunks,
                          float scale_a, float scale_b, const float* col_scale, float* C);
int32_t crl_prof_enable(crl_ppo* h, int32_t on);
int32_t crl_prof_read(crl_ppo* h, int32_t kernel_id, double* total_ms, int64_t* launches);
int32_t crl_prof_reset(crl_ppo* h);

/* =====================================================================================================
 * A2C: src/algorithms/a2c.jl on the GPU. One on-device CartPoleEnv{Float64}; the reference's
 * numeric regime (Float32 weights, Float64 observations ⇒ Float64 activations / losses / cotangents, a2c.jl:35,55-56)
 * is kept: these kernels are plain Float64 VALU code — a training batch is ≤ 2·min_replay_size samples of a 2x64 MLP
 * (≈0.1 GFLOP), nothing for the matrix pipes to win.
 * ===================================================================================================== */
typedef struct crl_a2c_config {   /* A2CConfig, a2c.jl:1-10 */
  double lr;                      /* a2c.jl:4 */
  int64_t total_timesteps;        /* a2c.jl:6 */
  int32_t min_replay_size;        /* a2c.jl:7; must be >= max_steps + 1 so the 2x buffer never wraps inside an update batch */
  int32_t max_steps;              /* a2c.jl:35 CartPoleEnv(max_steps=500) */
  double gamma;                   /* a2c.jl:9 */
  uint64_t seed;
} crl_a2c_config;
typedef struct crl_a2c_train_stats { double actor_loss, critic_loss; int32_t n, trained; } crl_a2c_train_stats;  /* a2c.jl:100 */
typedef struct crl_a2c_episode { double episode_return; int64_t episode_length, global_step; } crl_a2c_episode;  /* a2c.jl:106 */
typedef struct crl_a2c crl_a2c;
/* What crl_dqn_evaluate and crl_a2c_evaluate report: Float64 on the host from the per-episode arrays, sums in array order (80 bytes). */
typedef struct crl_value_eval_report { int64_t episodes, env_steps;
  double return_mean, return_std, return_min, return_max, length_mean, disc_return_mean, v0_mean, v_bias_mean; } crl_value_eval_report;

/* a2c.jl:32-52: networks (parameters are uploaded by crl_a2c_write_params, same flat layout as PPO: obs 4 / act 2 / 2x64),
 * Optimiser(ClipNorm(0.5), Adam(lr)) state, ReplayBuffer(capacity = 2*min_replay_size), reset!(env). */
int32_t crl_a2c_create(const crl_a2c_config* cfg, int32_t device, crl_a2c** out);
int32_t crl_a2c_destroy(crl_a2c* h);
int32_t crl_a2c_param_count(const crl_a2c* h, int64_t* n);
int32_t crl_a2c_write_params(crl_a2c* h, const float* params, size_t n);
int32_t crl_a2c_read_params(crl_a2c* h, float* params, size_t n);
/* The Float32 gradients of the last update (a2c.jl:87,97 `gradient(...)`, projected to the parameters' type) as the optimiser received them:
 * before ClipNorm, same flat layout as the parameters (the actor's six arrays, then the critic's). The optimiser reads them without changing
 * them, so they stay until the next update. Read-only; synchronises on the handle's stream. Errors: NULL grads; n != crl_a2c_param_count; no
 * update yet (no crl_a2c_run_until_update call of this handle has trained). */
int32_t crl_a2c_read_grads(crl_a2c* h, float* grads, size_t n);
/* `actor, critic = Networks.make_actor_critic(env)` — a2c.jl:37: crl_make_actor_critic(4, 2, 64, seed) uploaded. crl_a2c_run_until_update
 * on a handle whose parameters were neither written nor initialised is an error (a fresh handle holds zeros). */
int32_t crl_a2c_init_params(crl_a2c* h, uint64_t seed);
/* env state (4 doubles), global_step, current buffer size */
int32_t crl_a2c_read_env(crl_a2c* h, double* state4, int64_t* global_step, int32_t* rb_size);
/* replay buffer columns 1..size (a2c.jl:77 `x[:, 1:rb.size]`): state (4,size) Float64, action 0-based, reward, terminal */
int32_t crl_a2c_read_buffer(crl_a2c* h, double* state, int32_t* action, double* reward, uint8_t* terminal, int32_t capacity);
/* a2c.jl:53-111 `for global_step in 1:total_timesteps` body, run on the device until ONE training update has happened
 * (stats->trained = 1), max_env_steps were taken, or total_timesteps is reached. "Episode Statistics" records
 * (a2c.jl:106) of the episodes that ended are written to eps[0..*n_eps) (at most max_eps; later ones are dropped).
 * *steps_taken = env steps of this call. */
int32_t crl_a2c_run_until_update(crl_a2c* h, int64_t max_env_steps, crl_a2c_train_stats* stats, crl_a2c_episode* eps,
                                 int32_t max_eps, int32_t* n_eps, int64_t* steps_taken);
/* discounted_future_rewards(rewards, terminals, final_value, γ) (a2c.jl:13-24) on host vectors */
int32_t crl_a2c_discounted_future_rewards(int32_t device, const double* rewards, const uint8_t* terminals, int32_t n,
                                          double final_value, double gamma, double* out);
/* The missing public forward of A2C, the counterpart of crl_dqn_q_values. net 0: the actor's logits, (4, n) -> (2, n); net 1: the critic, (4, n) -> (n).
 * Float64, a2c.jl:55-56 / :82 arithmetic: Dense(tanh_fast) twice and the head, products in input order, bias last, no contraction — a wave per
 * observation through the forward kernel of the training batch. Errors: net outside {0, 1}; n < 0; NULL obs or out with n > 0; parameters never set. */
int32_t crl_a2c_forward(crl_a2c* h, int32_t net, const double* obs, int32_t n, double* out);
/* Held-out evaluation of the current actor, and of the critic's bias: see crl_dqn_evaluate below, whose definition it shares. A2C reads both networks,
 * accepts CRL_EVAL_GREEDY and CRL_EVAL_SAMPLE, and v0 is the critic's value of the reset state. csrc/a2c.hip, a2c_eval_kernel. */
int32_t crl_a2c_evaluate(crl_a2c* h, const crl_eval_config* cfg, crl_value_eval_report* report,
                         double* returns, int32_t* lengths, double* disc_returns, double* v0, int32_t* trace_action);
/* envs per block of a2c_eval_kernel (a compile-time constant of the library; tests choose their block-edge sizes from it) */
int32_t crl_a2c_eval_envs_per_block(void);

/* =====================================================================================================
 * DQN: src/algorithms/dqn.jl on the GPU. One on-device CartPoleEnv{Float64} (max_steps = 200),
 * q / target networks Chain(Dense(4,120,relu), Dense(120,84,relu), Dense(84,2)) (dqn.jl:22-26) with Float32 weights and
 * Float64 arithmetic like the reference, replay ring, ε-greedy schedule, minibatch drawn without replacement, TD target,
 * Flux.mse, Adam (no ClipNorm), hard target copy — a call enqueues the whole chunk of the `for global_step` loop (one fixed
 * ten-launch cycle per train_freq steps) and reads nothing back until it ends.
 * ===================================================================================================== */
typedef struct crl_dqn_config {   /* DQNConfig, dqn.jl:1-19 */
  int64_t log_frequency, total_timesteps, buffer_size, min_buff_size;
  double lr;
  int64_t train_freq, target_net_freq, batch_size;
  double gamma, epsilon_start, epsilon_end, epsilon_duration;
  int32_t max_steps;              /* dqn.jl:37 CartPoleEnv(): 200 */
  int32_t pad;
  uint64_t seed;
} crl_dqn_config;
typedef struct crl_dqn_episode { double episode_return; int64_t episode_length, global_step; double epsilon; } crl_dqn_episode; /* dqn.jl:88 */
typedef struct crl_dqn_loss_record { int64_t global_step; double loss; } crl_dqn_loss_record;                                  /* dqn.jl:116 */
typedef struct crl_dqn_status { double env_state[4]; int64_t global_step, rb_size, n_updates; double last_loss; } crl_dqn_status;
typedef struct crl_dqn crl_dqn;
#define CRL_DQN_PARAM_COUNT 10934 /* W1(120,4) b1 W2(84,120) b2 W3(2,84) b3 — Flux.params(q_net) order, (out,in) col-major */

int32_t crl_dqn_create(const crl_dqn_config* cfg, int32_t device, crl_dqn** out);          /* dqn.jl:34-56 */
int32_t crl_dqn_destroy(crl_dqn* h);
int32_t crl_dqn_write_params(crl_dqn* h, const float* q_params, size_t n);                  /* q_net; target_net = deepcopy(q_net) */
int32_t crl_dqn_read_params(crl_dqn* h, float* q_params, float* target_params, size_t n);   /* target_params may be NULL */
/* `q_net = make_nn(env)` — dqn.jl:22-26,39: Dense(4,120,relu) → Dense(120,84,relu) → Dense(84,2) with Flux's default glorot_uniform
 * weights and zero biases, flat in Flux.params(q_net) order; stateless and host-only. n must be CRL_DQN_PARAM_COUNT. */
int32_t crl_dqn_make_nn(uint64_t seed, float* out, size_t n);
/* dqn.jl:39-40 for a handle: crl_dqn_make_nn uploaded to q_net and target_net. crl_dqn_run / crl_dqn_q_values on a handle whose
 * parameters were neither written nor initialised are errors (a fresh handle holds zeros). */
int32_t crl_dqn_init_params(crl_dqn* h, uint64_t seed);
int32_t crl_dqn_status_read(crl_dqn* h, crl_dqn_status* out);
/* dqn.jl:57-119: up to max_env_steps iterations of the loop (or to total_timesteps), enqueued without host read-backs. Episode records
 * (dqn.jl:88) and the "Training Statistics" losses of steps that are multiples of log_frequency (dqn.jl:115-117) come
 * back in eps / losses (entries beyond max_* are dropped). */
int32_t crl_dqn_run(crl_dqn* h, int64_t max_env_steps, crl_dqn_episode* eps, int32_t max_eps, int32_t* n_eps,
                    crl_dqn_loss_record* losses, int32_t max_losses, int32_t* n_losses, int64_t* steps_taken);
/* q_net(obs) for n observations (4, n) Float64 → (2, n) Float64 (dqn.jl:64) */
int32_t crl_dqn_q_values(crl_dqn* h, const double* obs, int32_t n, double* q);
/* Held-out evaluation of the greedy policy, and of the value function's bias — no reference counterpart: dqn.jl:61-68 acts ε-greedily with
 * ε >= epsilon_end = 0.05 and a2c.jl:56-58 samples from the softmax, so their "Episode Statistics" score an exploring policy on the one training env,
 * and neither log can say whether the value function over-estimates — for DQN, whose TD target is a max over target-net Q-values (dqn.jl:99-100),
 * the first question anyone asks. Here the handle's current network(s), frozen, play cfg->episodes_per_env whole episodes on each of cfg->num_envs
 * fresh, private CartPoleEnv{Float64} in ONE read-only launch (csrc/dqn.hip dqn_eval_kernel, csrc/a2c.hip a2c_eval_kernel; one wave owns one env).
 * crl_eval_config is PPO's struct. The trajectory is defined by public calls. With n = num_envs, E = episodes_per_env and the handle's max_steps and
 * gamma, env e (0 <= e < n), episode j (0 <= j < E):
 *   reset    s[i] = 0.1·u53(Philox(key = cfg->seed, env = i, gstep = j·n + e, stream 0x20)) − 0.05, i = 0..3 — the loops' reset at the new stream 0x20,
 *            "evaluation reset" (the loops use 0, 1, 2 and 4, DDPG 0x10–0x16) —, t = 0.
 *   step     obs = the four doubles of s.
 *            DQN: q = exactly what crl_dqn_q_values returns for obs; action = q[1] > q[0] ? 1 : 0 (the first maximum, as the training loop's argmax).
 *                 Only CRL_EVAL_GREEDY is accepted: DQN has no sampling policy.
 *            A2C: z = exactly what crl_a2c_forward(net = 0) returns for obs. CRL_EVAL_GREEDY: action = z[1] > z[0] ? 1 : 0 (exp is never evaluated).
 *                 CRL_EVAL_SAMPLE: the training loop's own expressions, m = max(z0, z1), e0 = exp(z0 − m), e1 = exp(z1 − m), p0 = e0 / (e0 + e1),
 *                 action = p0 <= draw with draw = u53(Philox(key = cfg->seed, env = e, gstep = r, stream 0x21)), r = the env's step count across its
 *                 episodes; stream 0x21 is new, "evaluation draw".
 *   v0       on the first step of an episode. DQN: q[action]. A2C: exactly what crl_a2c_forward(net = 1) returns for obs.
 *   sums     done = the CartPole step with action (terminal by position, angle, or t > max_steps), rew = done ? 0.0 : 1.0 as in both training loops;
 *            ret += rew; disc_ret += disc·rew; disc = disc·gamma; length += 1, from 0.0, 0.0, 1.0 and 0 — Float64, in step order, a plain multiply
 *            then an add, no contraction. The episode ends at done: it has at most max_steps + 1 steps.
 * returns / lengths / disc_returns / v0: (E, n), env fastest (index j·n + e); each may be NULL. trace_action: (trace_steps, n), row r = the action of
 * the env's r-th step counted across its episodes, or −1 once the env has played its quota; NULL exactly when trace_steps = 0, and trace_steps <=
 * E·(max_steps + 1) (it exists so that tests can follow the device's trajectory). The report is computed on the host in Float64 from the arrays, sums
 * in array order: episodes = n·E, env_steps = Σ lengths, return_std the population standard deviation, length_mean = Σ lengths / episodes,
 * v0_mean = Σ v0 / episodes and v_bias_mean = Σ(v0 − disc_return) / episodes: positive = the value function promises more than the policy collects.
 * Reads the handle's parameters and config and nothing else — DQN the q-net, not the target; A2C both networks —: the target net, Adam state and β
 * powers, replay ring, env state and counters, episode sums and pending records stay bit for bit as they were. It synchronises before it returns. The
 * launch is bounded by E·(max_steps + 1) steps per env; no flags, no atomics, and after one staging barrier no block-wide synchronisation, so waves
 * whose episodes end early simply leave. Errors, each naming the field: NULL cfg / report; parameters never set; num_envs outside 1..65536;
 * episodes_per_env outside 1..1024; num_envs * episodes_per_env > 1048576; an unknown mode, or CRL_EVAL_SAMPLE on DQN; trace_steps < 0 or >
 * E·(max_steps + 1); trace_steps > 0 without a trace_action, or a trace_action with trace_steps = 0; trace_steps * num_envs > 16777216. Device scratch
 * is allocated on first use, kept on the handle and freed by crl_*_destroy. */
int32_t crl_dqn_evaluate(crl_dqn* h, const crl_eval_config* cfg, crl_value_eval_report* report,
                         double* returns, int32_t* lengths, double* disc_returns, double* v0, int32_t* trace_action);
/* envs per block of dqn_eval_kernel (a compile-time constant of the library; tests choose their block-edge sizes from it) */
int32_t crl_dqn_eval_envs_per_block(void);

/* -----------------------------------------------------------------------------------------------------
 * Prioritized experience replay for DQN (Schaul et al. 2016, proportional variant) — no reference counterpart: dqn.jl replays uniformly. A handle
 * made by crl_dqn_per_create runs the same ten-launch cycle with two kernels of its own in the places of the uniform draw and of the TD kernel
 * (csrc/dqn_per.hpp, csrc/dqn.hip: dqn_per_sample_kernel, dqn_td_kernel<false, true>); collect, the forwards, the pullbacks, the weight gradients, Adam and the
 * target copy are shared. crl_dqn_run, crl_dqn_status_read, crl_dqn_read_params / crl_dqn_write_params / crl_dqn_init_params, crl_dqn_q_values,
 * crl_dqn_evaluate and crl_dqn_destroy work on it unchanged; a crl_dqn_create handle is what it was, bit for bit, and the three per_* calls below fail
 * on it with a message. Everything is on the device; no call in between reads anything back.
 *
 * All arithmetic below is Float64, one operation per written operator, no contraction, unless a cast is written. n = the ring's size, k = batch_size,
 * g = the global step of the update, δ_j = td_j − Q(s_j, a_j) exactly as in the uniform loop (dqn.jl:99-107).
 *   Tree     C = the smallest power of two >= buffer_size. tree[1 .. 2C) in heap order (tree[0] is unused and 0.0); the leaf of ring slot s is
 *            tree[C + s]; leaves of slots >= n are 0.0; every inner node is exactly tree[2i] + tree[2i+1], one add, the left operand first. The tree is
 *            therefore a pure function of its leaves: any repair order gives the same bits, and a restatement may rebuild it whole.
 *   Leaves   are Float32 values, stored widened, so that the last bits of a Float64 pow do not reach the sampler:
 *            leaf = (float)clamp(pow(|δ| + eps, alpha), 2^-100, 2^100), clamp(p) = p >= 2^-100 ? (p > 2^100 ? 2^100 : p) : 2^-100 (a NaN becomes 2^-100).
 *            max_leaf starts at 1.0f and is the largest leaf any update has written.
 *   Add      A transition added to slot p gets leaf[p] = max_leaf, the value as of the last completed update. The collect kernel is not involved: the
 *            sample kernel keeps synced_step (0 on a fresh handle) and, before drawing, writes max_leaf into the min(g − synced_step, buffer_size) slots
 *            behind the ring's write pointer (ptr − 1, ptr − 2, … modulo buffer_size), repairs their ancestors and sets synced_step = g.
 *   Draw     seg = tree[1] / (double)k. For j = 0 .. k − 1: u_j = u53(Philox(counter (j, g lo, g hi, 0xDA), key = cfg.seed)) — stream 0xDA is new,
 *            "prioritized draw" (the uniform draw uses 0xD9) —, target = ((double)j + u_j) · seg. Descend from i = 1 while i < C: l = tree[2i]; go
 *            left (i = 2i) if target < l || tree[2i+1] == 0.0, otherwise target = target − l and go right (i = 2i + 1). idx[j] = i − C. Draws are
 *            with replacement. The zero test keeps every visited node positive, so no slot >= n and no empty leaf is ever returned.
 *   Weights  slope = (beta_end − beta_start) / beta_duration; v = slope · (double)g + beta_start; beta(g) = beta_end once v has passed it — v >
 *            beta_end for slope >= 0, v < beta_end for slope < 0 —, otherwise v. w_j = pow((double)n · leaf[idx_j] / tree[1], −beta(g)) (the product
 *            first), then w_j = w_j / max_j w_j: the batch maximum; there is no min tree.
 *   Update   sq_j = w_j · (δ_j · δ_j); loss = (Σ_j sq_j, in sample order from 0.0) / (double)k — this is what crl_dqn_run logs and last_loss holds;
 *            dz_j = −2.0 · w_j · δ_j / (double)k, evaluated left to right. The rest of the backward pass is the uniform one. The new leaf of idx_j
 *            follows the leaf expression (duplicate indices write identical values); max_leaf is raised to the batch's largest new leaf; the ancestors
 *            are repaired in the same launch. With beta = 0 every weight is exactly 1.0 and loss and gradient are the uniform loop's on that batch.
 * Errors of crl_dqn_per_create, beyond crl_dqn_create's: a NULL argument; alpha, beta_start or beta_end outside 0..1; beta_duration not > 0; eps
 * outside 1e-6..1.
 * ----------------------------------------------------------------------------------------------------- */
typedef struct crl_dqn_per_options { double alpha, beta_start, beta_end, beta_duration, eps; } crl_dqn_per_options;   /* 40 bytes */
int32_t crl_dqn_per_create(const crl_dqn_config* cfg, const crl_dqn_per_options* per, int32_t device, crl_dqn** out);
/* beta = beta(g) of the last update (beta_start before the first), total = tree[1], tree_leaves = C */
typedef struct crl_dqn_per_status { double beta, total; float max_leaf; int32_t tree_leaves; } crl_dqn_per_status;
int32_t crl_dqn_per_status_read(crl_dqn* h, crl_dqn_per_status* out);
/* The state after the last update; any pointer may be NULL: leaves[buffer_size], tree[2·C], idx[k], weight[k] (normalised), abs_td[k] (|δ_j|). */
int32_t crl_dqn_per_read(crl_dqn* h, float* leaves, double* tree, int32_t* idx, double* weight, double* abs_td);
/* The sampler alone, on the caller's leaves and a scratch tree (training state untouched): the tree of leaves[0 .. n) with C(n) = the smallest power
 * of two >= n is built, k draws are taken at update step gstep with the handle's seed, and their weights at beta — the same __device__ functions the
 * cycle runs. 1 <= n <= 65536, 1 <= k <= 1024, 0 <= beta <= 1, every leaf in 2^-100..2^100; tree receives 2·C(n) doubles and may be NULL. */
int32_t crl_dqn_per_probe(crl_dqn* h, const float* leaves, int32_t n, uint64_t gstep, int32_t k, double beta,
                          int32_t* idx, double* weight, double* tree);

/* -----------------------------------------------------------------------------------------------------
 * DQN target options: double Q-learning (van Hasselt et al. 2016) and uncorrected n-step returns (as Rainbow uses them) — no reference counterpart:
 * dqn.jl:99-100 forms a 1-step max over target_net. Both change how the TD target is formed and nothing else: the parameter layout, crl_dqn_q_values,
 * crl_dqn_evaluate and the collect kernel are what they were, and they compose with prioritized replay, whose priority is |δ| of the new target. A
 * handle made by crl_dqn_create_with runs the same ten-launch cycle with two kernels of its own in the places of the sampling launch and of the TD
 * launch (csrc/dqn_target.hpp, csrc/dqn.hip: dqn_tgt_sample_kernel, dqn_td_kernel<true, PER>); with double_q the three forward launches carry a third pass.
 * crl_dqn_create and crl_dqn_per_create handles keep every bit of their behaviour; the two calls below fail on them with a message naming
 * crl_dqn_create_with. With per != NULL the handle is also a PER handle: the crl_dqn_per_* calls work on it.
 *
 * For sample j with slot s = idx[j], ring capacity cap = buffer_size and ptr the slot the next add will take, all as of this update; all Float64, one
 * operation per written operator, no contraction:
 *   R = 0.0; disc = 1.0; c = s; m = 0
 *   repeat:  R = R + disc * reward[c];  disc = disc * gamma;  m = m + 1;  last = c
 *            stop if terminal[last] != 0 or m == n_step
 *            nx = (last + 1 == cap) ? 0 : last + 1
 *            stop if nx == ptr                 (`last` is the newest transition: the horizon is cut, never wrapped into the oldest)
 *            c = nx
 *   x      = next_state[last]
 *   a*     = double_q ? (q_net(x)[1] > q_net(x)[0] ? 1 : 0) : (target_net(x)[1] > target_net(x)[0] ? 1 : 0)      (the first maximum)
 *   next_q = target_net(x)[a*]
 *   td     = R + disc * next_q * (1.0 - (double)terminal[last])      (((disc·next_q)·(1−t)), then added to R)
 *   δ      = td - q_net(state[s])[action[s]]
 * disc is gamma^m by repeated multiplication; no pow is involved. Everything downstream is unchanged: the mse or the importance-weighted mse, dz, the
 * backward pass, the Float32 gradient projection, Adam, the target copy, the PER leaf from |δ|. Episodes never mix: the env stores terminal = 1 for
 * failure and for the step limit alike. With {n_step = 1, double_q = 0} the expressions reduce bit for bit to dqn.jl's: 0.0 + 1.0·r = r, 1.0·γ = γ.
 * Errors of crl_dqn_create_with, beyond crl_dqn_create's and (with per) crl_dqn_per_create's: cfg or out NULL; n_step outside 1..16; double_q not 0
 * or 1 — each names the field.
 * ----------------------------------------------------------------------------------------------------- */
typedef struct crl_dqn_target_options { int32_t n_step; int32_t double_q; } crl_dqn_target_options;   /* 8 bytes */
int32_t crl_dqn_create_with(const crl_dqn_config* cfg, const crl_dqn_per_options* per /* NULL = uniform */,
                            const crl_dqn_target_options* tgt /* NULL = {1, 0} */, int32_t device, crl_dqn** out);
/* The k values of the last completed update (zeros before the first); any pointer may be NULL: last[k] (the slot x was read from), m[k] (the steps
 * summed), nret[k] (R), ndisc[k] (disc), astar[k], td[k]. */
int32_t crl_dqn_target_read(crl_dqn* h, int32_t* last, int32_t* m, double* nret, double* ndisc, int32_t* astar, double* td);
/* The walk alone, on a ring the host wrote into scratch (training state untouched): the same __device__ function the update runs. reward[cap],
 * terminal[cap], idx[k]; 1 <= cap <= 65536, 0 <= ptr < cap, 1 <= k <= 1024, every idx in 0..cap-1, 1 <= n_step <= 16; no pointer may be NULL. */
int32_t crl_dqn_nstep_probe(crl_dqn* h, const double* reward, const uint8_t* terminal, int32_t cap, int32_t ptr, const int32_t* idx, int32_t k,
                            int32_t n_step, double gamma, int32_t* last, int32_t* m, double* nret, double* ndisc);

/* -----------------------------------------------------------------------------------------------------
 * Categorical DQN (C51, Bellemare et al. 2017) — no reference counterpart: dqn.jl's critic is a scalar. A handle made by crl_dqn_c51_create learns,
 * per action, a distribution over N fixed atoms instead of one number. The trunk is dqn.jl's, W1(120,4) b1 W2(84,120) b2; the head is W3(2N, 84)
 * b3(2N), row a·N + i = atom i of action a (Flux's reshape(…, N, 2, :) of a Dense(84, 2N)); one flat float vector, (out,in) column-major, 10764 +
 * 85·2N numbers (19434 at N = 51) — crl_dqn_param_count gives it, and crl_dqn_write_params / crl_dqn_read_params / crl_dqn_init_params take that n on
 * such a handle. The cycle stays ten launches (csrc/dqn_c51.hpp, csrc/dqn.hip: dqn_c51_*_kernel); sampler, ring, n-step walk, PER tree, Adam, target copy
 * and the loss record are the other handles', so crl_dqn_run, crl_dqn_status_read, crl_dqn_target_read and — with per != NULL — the crl_dqn_per_* calls
 * work unchanged. crl_dqn_q_values returns the expected values Q(a), (2, n); crl_dqn_evaluate acts greedily on them and reports q0 = Q(a): the bits
 * of crl_dqn_q_values for the same observation. crl_dqn_create, crl_dqn_per_create and crl_dqn_create_with handles keep every bit of their behaviour;
 * the c51_* calls below fail on them with a message naming crl_dqn_c51_create.
 *
 * All Float64, one operation per written operator, no contraction; every Σ starts from 0.0 and runs in ascending index order:
 *   Atoms     Δ = (v_max − v_min) / (double)(N − 1);  z_i = v_min + (double)i · Δ
 *   Softmax   of a row of N logits l:  mx = max_i l_i;  d_i = l_i − mx;  e_i = exp(d_i);  S = Σ_i e_i;  p_i = e_i / S;  logp_i = d_i − log(S)
 *   Value     Q(a) = Σ_i z_i · p_i; greedy = the first maximum (Q(1) > Q(0) ? 1 : 0) — in collect, in evaluation and for a*
 *   Target    for sample j: R, disc, last from the n-step walk above (n_step = 1: R = reward, disc = gamma, last = idx_j); x = next_state[last];
 *             a* = the first maximum of Q over q_net(x) under double_q, else over target_net(x);  p' = softmax(target_net(x)[a*])
 *   Project   for each source atom s = 0..N−1:  Tz = R + ((disc · z_s) · (1.0 − (double)terminal[last]));
 *             Tz = Tz < v_min ? v_min : (Tz > v_max ? v_max : Tz);  b = (Tz − v_min) / Δ;  b = b > (double)(N−1) ? (double)(N−1) : b;
 *             lo = floor(b); up = ceil(b); if lo == up atom lo receives p'_s, otherwise lo receives p'_s · ((double)up − b) and up receives
 *             p'_s · (b − (double)lo).  m_i = Σ of what atom i receives, over s ascending (each target atom gathers: no atomics)
 *   Loss      loss_j = −Σ_i m_i · logp_i(state_j, action_j)  (>= 0 exactly);  loss = (Σ_j w_j · loss_j, in sample order) / (double)k, w_j = 1.0 under
 *             uniform replay — what crl_dqn_run logs and last_loss holds;  dl_i = w_j · (p_i − m_i) / (double)k, left to right, on the taken action's
 *             logits; the other action's logits get exactly 0.0
 *   PER       the priority input is loss_j where the scalar handles use |δ_j|: leaf, max_leaf, repair and weights are PER's own; abs_td holds loss_j
 *   Backward  d2_j = relu'(H2_j) · Σ_i W3[a·N+i, j] · dl_i in atom order; weight gradients one parameter at a time over the samples in sample order,
 *             an exact 0.0 for samples of the other action, then the Float32 projection; Adam with six arrays, one β-power pair each
 * crl_dqn_target_read's td on such a handle is R + ((disc · Q_target(x)[a*]) · (1 − terminal[last])), the scalar the distribution's mean moves towards;
 * it enters nothing. exp and log are the device library's; how far they lie from a correctly rounded result has not been measured (tests/c51_bar.py).
 * n_atoms in 2..64 (a wavefront's lane owns an atom); v_min < v_max, both finite. Errors of crl_dqn_c51_create, beyond crl_dqn_create_with's: cfg, c51
 * or out NULL; n_atoms outside 2..64; v_min or v_max not finite; v_min >= v_max — each names the field.
 * ----------------------------------------------------------------------------------------------------- */
typedef struct crl_dqn_c51_options { int32_t n_atoms; int32_t pad; double v_min, v_max; } crl_dqn_c51_options;   /* 24 bytes */
int32_t crl_dqn_c51_create(const crl_dqn_config* cfg, const crl_dqn_c51_options* c51, const crl_dqn_per_options* per /* NULL = uniform */,
                           const crl_dqn_target_options* tgt /* NULL = {1, 0} */, int32_t device, crl_dqn** out);
/* the handle's parameter count: CRL_DQN_PARAM_COUNT on every handle but a C51 one (above) and a dueling one (20928 + 255·R, below) */
int32_t crl_dqn_param_count(crl_dqn* h, size_t* n);
/* crl_dqn_make_nn's rule (glorot_uniform weights, zero biases; the same trunk for the same seed) on the C51 shapes; n must be 10764 + 85·2·n_atoms */
int32_t crl_dqn_c51_make_nn(uint64_t seed, int32_t n_atoms, float* out, size_t n);
/* softmax of q_net(obs) per action for n observations (4, n) → (N, 2, n), atom fastest; crl_dqn_q_values is Σ_i z_i · probs[i, a, ·] of it, bit for bit */
int32_t crl_dqn_c51_probs(crl_dqn* h, const double* obs, int32_t n, double* probs);
/* the last completed update (zeros before the first): proj[k·N] the projected targets m, sample by sample, atom fastest; sample_loss[k] the loss_j.
 * Either may be NULL. */
int32_t crl_dqn_c51_read(crl_dqn* h, double* proj, double* sample_loss);
/* The projection alone with the handle's N, v_min, v_max on caller-supplied rows (training state untouched): the same __device__ function the update
 * runs. probs (N, k) p' rows, nret[k] R, ndisc[k] disc, terminal[k]; 1 <= k <= 1024; no pointer may be NULL. */
int32_t crl_dqn_c51_project_probe(crl_dqn* h, const double* probs, const double* nret, const double* ndisc, const uint8_t* terminal, int32_t k,
                                  double* proj);

/* -----------------------------------------------------------------------------------------------------
 * Dueling heads (Wang et al. 2016) — no reference counterpart: dqn.jl's critic has one head. A handle made by crl_dqn_dueling_create splits layers 2
 * and 3 into a state-value stream and an advantage stream and combines them where the head's output is written. R = 1 on a scalar handle (c51 NULL),
 * R = n_atoms on a categorical one (Rainbow's form: the combined rows are the logits the Softmax above takes, per action over i). Ten arrays, one flat
 * float vector, each (out,in) column-major, in this order:
 *   W1(120,4) b1  W2v(84,120) b2v  W3v(R,84) b3v  W2a(84,120) b2a  W3a(2R,84) b3a      20928 + 255·R numbers (21183 at R = 1, 33933 at R = 51)
 * crl_dqn_param_count gives it, and crl_dqn_write_params / crl_dqn_read_params / crl_dqn_init_params take that n on such a handle. Such a handle always
 * carries target options ({1, 0} by default), so crl_dqn_target_read works on it; the crl_dqn_c51_* calls work when c51 was given, the crl_dqn_per_*
 * calls when per was. The cycle stays ten launches (csrc/dqn_duel.hpp, csrc/dqn.hip: dqn_duel_*_kernel); sampler, ring, n-step walk, PER tree, the TD
 * kernels and the loss record are the other handles'. Every other crl_dqn_* call works unchanged; crl_dqn_create, crl_dqn_per_create,
 * crl_dqn_create_with and crl_dqn_c51_create handles keep every bit of their behaviour, and crl_dqn_dueling_streams fails on them with a message naming
 * crl_dqn_dueling_create.
 *
 * All Float64, one operation per written operator, no contraction; every dot product starts from 0.0, runs in input order and adds the bias last:
 *   Forward   h1 = relu(W1·x + b1);  h2v = relu(W2v·h1 + b2v);  h2a = relu(W2a·h1 + b2a)
 *             V_i = W3v[i,:]·h2v + b3v[i], i < R;  A_{a,i} = W3a[a·R+i,:]·h2a + b3a[a·R+i], a in {0, 1}
 *             mean_i = (A_{0,i} + A_{1,i}) * 0.5;  out_{a,i} = V_i + (A_{a,i} − mean_i)
 *             out is Q(a) on a scalar handle — halving is exact, so that path still runs no transcendental — and the logits on a categorical one.
 *             crl_dqn_q_values, crl_dqn_c51_probs, the collect step and crl_dqn_evaluate all act on these bits.
 *   Backward  g_i = the cotangent on out_{act,i} of the taken action (dz of the scalar update, dl_i of the categorical one, as pinned above):
 *             dV_i = g_i;  dA_{act,i} = g_i * 0.5;  dA_{1−act,i} = −(g_i * 0.5)
 *             d2v_j = relu'(h2v_j) · Σ_i W3v[i,j]·dV_i, i ascending;  d2a_j = relu'(h2a_j) · Σ_row W3a[row,j]·dA_row, row = a·R + i ascending
 *             d1_k = relu'(h1_k) · s, s = Σ_j W2v[j,k]·d2v_j (j ascending) and then, the same accumulator on, Σ_j W2a[j,k]·d2a_j (j ascending)
 *             weight gradients one parameter at a time over the samples in sample order from 0.0, then the Float32 projection; both rows of W3a
 *             and b3a receive a term from every sample. Adam with ten arrays, one β-power pair each.
 * Errors of crl_dqn_dueling_create are crl_dqn_c51_create's with c51 optional: cfg or out NULL; with c51, n_atoms outside 2..64, v_min or v_max not
 * finite, v_min >= v_max; bad per or tgt options — each names the field.
 * ----------------------------------------------------------------------------------------------------- */
int32_t crl_dqn_dueling_create(const crl_dqn_config* cfg, const crl_dqn_c51_options* c51 /* NULL = scalar */, const crl_dqn_per_options* per /* NULL = uniform */,
                               const crl_dqn_target_options* tgt /* NULL = {1, 0} */, int32_t device, crl_dqn** out);
/* crl_dqn_make_nn's rule (glorot_uniform weights, zero biases) on the ten arrays; for the same seed W1 and W2v get the draws crl_dqn_make_nn gives W1
 * and W2, then W3v, W2a, W3a draw in that order. n_atoms 0 = scalar (R = 1), else 2..64; n must be 20928 + 255·R. Stateless and host-only. */
int32_t crl_dqn_dueling_make_nn(uint64_t seed, int32_t n_atoms /* 0 = scalar */, float* out, size_t n);
/* the two streams before they are combined, for n observations (4, n): value (R, n), adv (R, 2, n) with i fastest. Either output may be NULL. */
int32_t crl_dqn_dueling_streams(crl_dqn* h, const double* obs, int32_t n, double* value, double* adv);

/* -----------------------------------------------------------------------------------------------------
 * Noisy linear layers (NoisyNets, Fortunato et al. 2018, factorised Gaussian noise) — no reference counterpart: dqn.jl explores ε-greedily. A handle
 * made by crl_dqn_noisy_create learns mu and sigma for every parameter of all its dense layers; its "twin" is the handle the other creators would make
 * from the same dueling / c51 / per / tgt arguments (crl_dqn_create when all are off; crl_dqn_per_create; crl_dqn_create_with when tgt is given;
 * crl_dqn_c51_create; crl_dqn_dueling_create), with P parameters. The effective image w = mu + sigma·eps of each net is materialised on the device,
 * and every kernel of the twin's cycle — collect, the forwards, the TD launch, the pullbacks, the weight gradients — runs on that image unchanged
 * (csrc/dqn_noisy.hpp, csrc/dqn.hip: the Adam slot is dqn_noisy_adam_kernel, and an eleventh launch, dqn_noisy_materialise_kernel, forms the next
 * generation's images on every CU: in the Adam launch's one block that measured slower). It composes with both heads,
 * dueling, both replays and every target option. The five older kinds of handle keep every bit of their behaviour; the crl_dqn_noisy_* calls below
 * fail on them with a message naming crl_dqn_noisy_create.
 *
 *   Table     The noise table lists the net's layers in parameter-array order — plain and categorical: (in, out) = (4,120) (120,84) (84,rows3), rows3 =
 *             2 or 2N; dueling: (4,120) (120,84) (84,R) (120,84) (84,2R) for W1, W2v, W3v, W2a, W3a — and each layer contributes xi_in[in] then
 *             xi_out[out]: 412 + rows3 or 700 + 3R floats (at most 892). The position c in the table is the Philox component word.
 *   Noise     z = sqrt(−2.0·log(1.0 − u_xy))·cos(6.283185307179586·u_zw), Float64, u_xy / u_zw the two 53-bit halves of ONE Philox block with counter
 *             (c, gen lo, gen hi, stream) and key cfg.seed — the Box–Muller form of DDPG's noise (csrc/normal_bm.hpp) —; stream 0x22 for q_net, 0x23
 *             for target_net (new: the loop uses 0, 1, 2, 4, evaluation 0x20 / 0x21, the draws 0xD9 / 0xDA).
 *             xi_c = (float)(z < 0.0 ? −sqrt(−z) : sqrt(z))                                      (f(x) = sgn(x)·sqrt|x|, rounded to Float32 once)
 *   eps       weight (i, j) of a layer: eps = xi_out[i] * xi_in[j], one Float32 multiply; bias i: eps = xi_out[i]
 *   Image     w = mu + sigma * eps: a Float32 multiply, then a Float32 add, no fma
 *   Gradient  g = the Float32 the twin's weight-gradient kernel leaves for parameter p (computed on the noisy image); g_mu = g;
 *             g_sigma = g * eps, one Float32 multiply. Adam (Flux's, as everywhere) runs over 2P entries, m and v likewise, with one β-power pair
 *             per array: the twin's arrays for mu, then as many again for sigma.
 *   Generations  The images in use after u completed updates (crl_dqn_status.n_updates) are generation gen = u, for both nets, each on its own
 *             stream word. The online image of generation u serves the collect steps up to the next update, that update's q_net(state) pass and its
 *             double-Q q_net(x) pass; the target image serves its target_net(x) pass. After the Adam step of that update (mu and sigma of q_net; the
 *             hard copy of mu and sigma to target_net when global_step % target_net_freq == 0) both images are rebuilt with generation u + 1 — the
 *             target image is redrawn every update, whether or not a copy happened. g_sigma of update u uses eps of generation u.
 *   Layout    2P floats: mu in the twin's layout, then sigma in the same layout. crl_dqn_param_count reports 2P; crl_dqn_write_params (mu, sigma of
 *             both nets, then both images rebuilt at the current generation), crl_dqn_read_params (mu, sigma of q_net / target_net) and
 *             crl_dqn_init_params take n = 2P.
 *   Init      per layer lim = 1.0 / sqrt((double)in); mu = (float)((u − 0.5) · (2.0 · lim)) ~ U(−1/√in, +1/√in) for weights, then biases, u in storage
 *             order from init.cpp's generator; sigma = (float)(sigma0 · lim).
 *   Noise off crl_dqn_evaluate, crl_dqn_q_values, crl_dqn_c51_probs and crl_dqn_dueling_streams read the mu half as their image: they are the twin's
 *             kernels on the twin's layout, so every evaluated action is still the argmax of crl_dqn_q_values on that observation, bit for bit.
 *             Collect acts on the noisy image.
 *   ε-greedy  is honoured as configured. The NoisyNet setting is epsilon_start = epsilon_end = 0: the draw u53 < 0 never fires and the agent explores
 *             by its noise alone.
 * Errors of crl_dqn_noisy_create: cfg, noisy or out NULL; sigma0 negative, not finite or above 10; dueling not 0 or 1; and the composed creators' own
 * (c51, per, tgt fields, crl_dqn_create's) — each names the field.
 * ----------------------------------------------------------------------------------------------------- */
typedef struct crl_dqn_noisy_options { double sigma0; } crl_dqn_noisy_options;   /* 8 bytes; Fortunato's default is 0.5 */
int32_t crl_dqn_noisy_create(const crl_dqn_config* cfg, const crl_dqn_noisy_options* noisy, int32_t dueling /* 0 | 1 */,
                             const crl_dqn_c51_options* c51 /* NULL = scalar */, const crl_dqn_per_options* per /* NULL = uniform */,
                             const crl_dqn_target_options* tgt /* NULL = the twin's default */, int32_t device, crl_dqn** out);
/* the Init rule above; n_atoms 0 = scalar, else 2..64; n must be 2P of that twin. Stateless and host-only. */
int32_t crl_dqn_noisy_make_nn(uint64_t seed, double sigma0, int32_t dueling, int32_t n_atoms /* 0 = scalar */, float* out, size_t n);
/* the effective image in use, net 0 = q_net, 1 = target_net; n must be P (half of crl_dqn_param_count) */
int32_t crl_dqn_noisy_weights(crl_dqn* h, int32_t net, float* out, size_t n);
/* the length of the handle's noise table: 412 + rows3, or 700 + 3R on a dueling handle */
int32_t crl_dqn_noisy_noise_count(crl_dqn* h, size_t* n);
/* the xi table of any generation and either net (stateless: training state untouched): one small launch of the __device__ function the Adam launch
 * builds its tables with. n must be crl_dqn_noisy_noise_count's. */
int32_t crl_dqn_noisy_noise(crl_dqn* h, uint64_t gen, int32_t net, float* xi, size_t n);

/* =====================================================================================================
 * DDPG: src/algorithms/ddpg.jl on the GPU — the reference's one continuous-action algorithm. Networks of ddpg.jl:19-37 with hidden width 64,
 * Float32 weights and Float64 arithmetic: actor Dense(obs,64,tanh_fast) → Dense(64,64,tanh_fast) → Dense(64,act,tanh_fast) → x·2 + randn(act)·
 * exploration_noise (one draw per CALL, broadcast over the batch, ddpg.jl:28), critic Dense(obs+act,64,relu) → Dense(64,64,relu) → Dense(64,1) on
 * vcat(obs, act). obs_dim 1..64 and act_dim 1..16 are runtime values. Each network is one flat float vector in Flux.params order, (out,in)
 * column-major. The loop of ddpg.jl:76-135 runs as a fixed six-launch cycle per env step (sample, critic pass, critic step, actor pass, actor
 * step, collect); a call enqueues the cycles of its chunk and reads nothing back until it ends. The env is either the built-in Float64 Pendulum
 * (g = 10, m = l = 1, dt = 0.05, torque ±2, obs (cos θ, sin θ, θ̇), reward −(θ² + 0.1·θ̇² + 0.001·u²), done = terminal = t >= max_steps) or lives
 * in the host process (ddpg.jl:50 is a MuJoCo env there): crl_ddpg_act / crl_ddpg_observe.
 * ===================================================================================================== */
#define CRL_DDPG_ENV_PENDULUM 0
#define CRL_DDPG_ENV_EXTERNAL 1
typedef struct crl_ddpg_config {   /* DDPGConfig, ddpg.jl:1-15 */
  int64_t total_timesteps, buffer_size, min_buff_size, batch_size, warmup_steps, log_frequency;
  double lr, tau, gamma, exploration_noise;
  int32_t obs_dim, act_dim;       /* Pendulum: 3, 1 */
  int32_t env_kind;               /* CRL_DDPG_ENV_* */
  int32_t max_steps;              /* Pendulum episode length: 200 */
  double act_low, act_high;       /* rand(act_space) of the warm-up (ddpg.jl:79): low + (high − low)·u per component */
  int32_t noise_in_update;        /* 1 (the reference): target_actor(next_state) (ddpg.jl:108) and actor(state) in the actor loss (:123) each add a
                                     fresh randn(act)·exploration_noise; 0: those two draws are zero (textbook DDPG). The behaviour draw (:79) stays. */
  int32_t pad;
  uint64_t seed;
} crl_ddpg_config;
typedef struct crl_ddpg_episode { double episode_return; int64_t episode_length, global_step; } crl_ddpg_episode;   /* ddpg.jl:97 */
typedef struct crl_ddpg_loss_record { int64_t global_step; double actor_loss, critic_loss; } crl_ddpg_loss_record;  /* ddpg.jl:132 */
typedef struct crl_ddpg_status {
  double theta, theta_dot;        /* Pendulum state (zeros on an external handle) */
  int64_t env_t, global_step, rb_size, rb_ptr, n_updates;   /* rb_ptr: 0-based slot of the next add (replay_buffer.jl:32) */
  double actor_loss, critic_loss; /* of the last update */
} crl_ddpg_status;
typedef struct crl_ddpg crl_ddpg;

/* lengths of Flux.params(actor) = W1(64,obs) b1 W2(64,64) b2 W3(act,64) b3 and Flux.params(critic) = W1(64,obs+act) b1 W2(64,64) b2 W3(1,64) b3 */
int32_t crl_ddpg_param_count(int32_t obs_dim, int32_t act_dim, int64_t* actor_n, int64_t* critic_n);
/* ddpg.jl:47-74. Rejected with a message that names the field: batch_size outside 1..1024, buffer_size outside batch_size..131072,
 * max(min_buff_size, warmup_steps) + 1 < batch_size (Buffer.sample asserts n <= size), obs_dim / act_dim out of range (Pendulum: 3 / 1),
 * act_low >= act_high, tau outside (0, 1]. */
int32_t crl_ddpg_create(const crl_ddpg_config* cfg, int32_t device, crl_ddpg** out);
int32_t crl_ddpg_destroy(crl_ddpg* h);
/* actor, critic; the targets are a deepcopy (ddpg.jl:53-54) */
int32_t crl_ddpg_write_params(crl_ddpg* h, const float* actor, size_t actor_n, const float* critic, size_t critic_n);
/* actor, critic, target_actor, target_critic (any may be NULL) */
int32_t crl_ddpg_read_params(crl_ddpg* h, float* actor, float* critic, float* target_actor, float* target_critic);
/* make_ddpg_nn (ddpg.jl:19-37): Flux's default glorot_uniform weights and zero biases; stateless and host-only */
int32_t crl_ddpg_make_nn(int32_t obs_dim, int32_t act_dim, uint64_t seed, float* actor, size_t actor_n, float* critic, size_t critic_n);
/* ddpg.jl:52-54 for a handle. Every call below that computes with the networks returns "parameters not set" on a handle whose parameters were
 * neither written nor initialised (a fresh handle holds zeros). */
int32_t crl_ddpg_init_params(crl_ddpg* h, uint64_t seed);
int32_t crl_ddpg_status_read(crl_ddpg* h, crl_ddpg_status* out);
/* ddpg.jl:76-135 on the Pendulum: up to max_env_steps iterations (or to total_timesteps). Episode records (ddpg.jl:97) and the losses of the
 * steps that are multiples of log_frequency (ddpg.jl:131-133) come back in eps / losses (entries beyond max_* are dropped). An error on an
 * external handle. */
int32_t crl_ddpg_run(crl_ddpg* h, int64_t max_env_steps, crl_ddpg_episode* eps, int32_t max_eps, int32_t* n_eps,
                     crl_ddpg_loss_record* losses, int32_t max_losses, int32_t* n_losses, int64_t* steps_taken);
/* Host-driven env (errors on a Pendulum handle). crl_ddpg_act: the action of step global_step + 1 for `obs` (ddpg.jl:79: rand(act_space) during
 * the warm-up, else actor(obs) with its noise), unclipped; advances nothing. crl_ddpg_observe: ddpg.jl:76-134 without the env — global_step += 1,
 * Buffer.add!(state, action, reward, next_state, terminal), and the update when it is due (the same kernels as crl_ddpg_run). Host pointers. */
int32_t crl_ddpg_act(crl_ddpg* h, const double* obs, double* action_out);
int32_t crl_ddpg_observe(crl_ddpg* h, const double* obs, const double* action, double reward, const double* next_obs, int32_t terminal);
/* the loss records (ddpg.jl:131-133) written since the last crl_ddpg_run / crl_ddpg_read_losses, oldest first; reading clears them */
int32_t crl_ddpg_read_losses(crl_ddpg* h, crl_ddpg_loss_record* losses, int32_t max_losses, int32_t* n_losses);
/* the ring: state (obs_dim, cap), action (act_dim, cap), reward (cap), next_state (obs_dim, cap), terminal (cap), cap = buffer_size slots;
 * ptr (0-based) and size as replay_buffer.jl:32-34 leave them */
int32_t crl_ddpg_read_buffer(crl_ddpg* h, double* state, double* action, double* reward, double* next_state, uint8_t* terminal, int64_t cap,
                             int64_t* ptr, int64_t* size);
/* the noise-free actor output 2·tanh_fast(·) for n observations (obs_dim, n) → (act_dim, n) */
int32_t crl_ddpg_actor(crl_ddpg* h, const double* obs, int32_t n, double* out);
/* get_q(critic, obs, act) (ddpg.jl:45) for n pairs → n values */
int32_t crl_ddpg_q_values(crl_ddpg* h, const double* obs, const double* act, int32_t n, double* out);
/* Held-out evaluation of the current actor, and of the critic's bias — no reference counterpart: ddpg.jl puts the exploration noise inside the actor
 * (:28), so its "Episode Statistics" score the noisy behaviour policy on the one training env. Here the handle's actor (not the target), frozen and
 * WITHOUT noise, plays cfg->episodes_per_env whole episodes on each of cfg->num_envs fresh, private Pendulums in ONE launch (csrc/ddpg.hip,
 * ddpg_eval_kernel). The trajectory is defined by public calls. With n = num_envs, E = episodes_per_env and the handle's max_steps and gamma, env e
 * (0 <= e < n), episode j (0 <= j < E): (θ, θ̇) = the Pendulum reset draw — components 0 and 1 of the Philox draw at (key = cfg->seed, gstep = j·n + e,
 * stream 0x16, "evaluation reset", beside the loop's 0x10–0x15): θ = −π + 2π·u0, θ̇ = −1 + 2·u1 —, t = 0. Per step: obs = (cos θ, sin θ, θ̇) as the
 * training loop forms it; a = exactly what crl_ddpg_actor returns for obs (2·tanh_fast(head), bit for bit); the Pendulum step with a (clipped to ±2
 * inside the step, as in training) gives the reward r; ret += r; disc_ret += disc·r, then disc = disc·gamma, from ret = disc_ret = 0.0 and disc = 1.0
 * — Float64, in step order, a plain multiply then an add, no contraction. On the first step of the episode q0 = exactly what crl_ddpg_q_values returns
 * for (obs, a), with the handle's current critic. The episode ends when the step reports terminal (t >= max_steps): every episode has max_steps steps.
 * returns / disc_returns / q0: (E, n), env fastest (index j·n + e); each may be NULL. trace_action: (trace_steps, n), row s = the action of the s-th
 * step of each env counted across its episodes (s = j·max_steps + t); NULL exactly when trace_steps = 0, and trace_steps <= E·max_steps (it exists so
 * that tests can follow the device's trajectory). The report is computed on the host in Float64 from the per-episode arrays, sums in array order:
 * episodes = n·E, env_steps = n·E·max_steps, return_std the population standard deviation, q0_mean = Σq0 / episodes and
 * q_bias_mean = Σ(q0 − disc_return) / episodes: positive = the critic promises more than the policy then collects. Reads the actor, the critic and the
 * handle's config and nothing else — targets, Adam state and β powers, the ring, env state, counters and episode sums, the loss records and the
 * external staging slot stay bit for bit as they were — and synchronises before it returns. The launch is bounded by E·max_steps steps per env; no
 * flags, no atomics, no cross-block synchronisation. Errors, each naming the field: NULL cfg / report; a handle whose env is external (step that env
 * on the host and take the actions from crl_ddpg_actor); parameters never set; num_envs outside 1..65536; episodes_per_env outside 1..1024;
 * num_envs * episodes_per_env > 1048576; trace_steps < 0 or > E·max_steps; trace_steps > 0 without a trace_action, or a trace_action with
 * trace_steps = 0; trace_steps * num_envs > 16777216. Device scratch is allocated on first use, kept on the handle and freed by crl_ddpg_destroy. */
typedef struct crl_ddpg_eval_config { int32_t num_envs, episodes_per_env, trace_steps, pad; uint64_t seed; } crl_ddpg_eval_config;   /* 24 bytes */
typedef struct crl_ddpg_eval_report { int64_t episodes, env_steps;
  double return_mean, return_std, return_min, return_max, disc_return_mean, q0_mean, q_bias_mean; } crl_ddpg_eval_report;           /* 72 bytes */
int32_t crl_ddpg_evaluate(crl_ddpg* h, const crl_ddpg_eval_config* cfg, crl_ddpg_eval_report* report,
                          double* returns, double* disc_returns, double* q0, double* trace_action);

/* =====================================================================================================
 * TD3 (Fujimoto et al. 2018) on the DDPG handle — no reference counterpart (the reference's README lists SAC and Rainbow as to-dos, no TD3; SAC: the block below). The
 * networks, the ring, the minibatch draw (stream 0xD9), the behaviour policy (one draw per call on stream 0x10, scaled by exploration_noise,
 * unclipped), the warm-up (rand(act_space), stream 0x11), the Pendulum, the host-driven mode, the records and the arithmetic conventions are
 * DDPG's: Float32 weights, Float64 arithmetic, contraction off wherever a sum is formed, dot products in input order with the bias last, sums over
 * the batch in sample order, gradients projected to Float32 before Adam. There are two critics of the DDPG critic's shape, each with its target,
 * its Adam(lr) state and its six β-power pairs. An update is due at step g exactly when DDPG's is (g > min_buff_size && g > warmup_steps). With
 * k = batch_size and the batch positions b = 0..k−1 of the draw:
 *   target action  a'[c] = clamp(2·tanh_fast(target_actor head)[c] + clamp(policy_noise·z(b, c), −noise_clip, +noise_clip), act_low, act_high), z(b, c)
 *                  = the Box–Muller normal of the DDPG block on Philox stream 0x17 ("target smoothing") at gstep = g, component word 16·b + c: one
 *                  draw per SAMPLE and component (not ddpg.jl:28's one draw per call). clamp(x, lo, hi) = x < lo ? lo : (x > hi ? hi : x).
 *   TD target      next_q = q2 < q1 ? q2 : q1 of target critic 1 / 2 on (next_state, a'); td = r + γ·next_q·(1 − terminal).
 *   critics        critic i takes mse(td, Q_i(s, a)) = Σ_b (td − q_i)² / k with its own gradient, Adam state and β powers; both step on every update.
 *                  The logged critic_loss is loss_1 + loss_2.
 *   actor          exactly when g % policy_delay == 0: −mean(Q_1(s, 2·tanh_fast(actor(s)))) through the UPDATED critic 1, no noise, Adam on the actor,
 *                  then polyak (tau) of the target actor and of both target critics — the targets move on those steps only, and the actor's β
 *                  powers advance on those steps only. actor_loss (status and records) is the value of the latest actor step, 0.0 before the first.
 * policy_delay = 1, policy_noise = 0, critic 2 = critic 1 and bounds that contain ±2 make every number DDPG's with noise_in_update = 0, bit for
 * bit (critic_loss = 2×). One cycle stays six launches (csrc/ddpg.hip): sample, td3_critic_kernel, td3_critic_step, actor pass, td3_actor_step
 * (+ all three polyaks), collect; the two actor launches return at once on a step where the actor is not due.
 * The handle type is crl_ddpg: crl_ddpg_run, _act, _observe, _read_losses, _read_buffer, _status_read, _actor, _q_values, _evaluate and _destroy
 * take a TD3 handle; crl_ddpg_q_values and the q0 of crl_ddpg_evaluate are critic 1's, and crl_ddpg_evaluate reads nothing of critic 2 (it, its
 * target and its Adam state stay bit for bit). The parameter calls come in twins, because the number of networks differs: crl_ddpg_write_params /
 * _init_params / _read_params refuse a TD3 handle and name the crl_td3_* call; every crl_td3_* call refuses a DDPG handle.
 * ===================================================================================================== */
typedef struct crl_td3_options { int32_t policy_delay, pad; double policy_noise, noise_clip; } crl_td3_options;  /* 24 bytes */
/* crl_ddpg_create's checks, and — each message naming its field — policy_delay < 1, policy_noise < 0, noise_clip < 0, noise_in_update != 0 (TD3
 * has its own target noise and none in the actor loss), NULL options. */
int32_t crl_td3_create(const crl_ddpg_config* cfg, const crl_td3_options* opt, int32_t device, crl_ddpg** out);
/* actor, critic 1, critic 2 (nc = nc2 = crl_ddpg_param_count's critic_n); the three targets are copies */
int32_t crl_td3_write_params(crl_ddpg* h, const float* actor, size_t na, const float* critic1, size_t nc, const float* critic2, size_t nc2);
/* any may be NULL */
int32_t crl_td3_read_params(crl_ddpg* h, float* actor, float* critic1, float* critic2, float* t_actor, float* t_critic1, float* t_critic2);
/* actor and critic 1 = crl_ddpg_make_nn(seed); critic 2 = the critic of crl_ddpg_make_nn(seed + 1), whose actor is dropped */
int32_t crl_td3_init_params(crl_ddpg* h, uint64_t seed);
/* get_q of critic 1 and of critic 2 for n pairs; either of q1 / q2 may be NULL. q1 = what crl_ddpg_q_values returns */
int32_t crl_td3_q_values(crl_ddpg* h, const double* obs, const double* act, int32_t n, double* q1, double* q2);

/* =====================================================================================================
 * SAC (Haarnoja et al. 2018: squashed-Gaussian actor, twin critics, entropy bonus, tuned temperature) on the DDPG handle — no reference
 * counterpart (the reference's README lists SAC as a to-do). The ring, the minibatch draw (stream 0xD9), the warm-up (rand(act_space), stream
 * 0x11), the Pendulum, the host-driven mode, the loss records, the critics' shape and the arithmetic conventions are DDPG's and TD3's: Float32
 * parameters, Float64 arithmetic, contraction off wherever a sum is formed, dot products in input order with the bias last, sums over the batch in
 * sample order, gradients projected to Float32 before Adam(lr). An update is due at step g exactly when DDPG's is. exploration_noise and
 * noise_in_update are not read (noise_in_update must be 0). With D = obs_dim, A = act_dim, k = batch_size, batch positions b = 0..k−1:
 *   actor          Dense(D,64,tanh_fast) → Dense(64,64,tanh_fast) → Dense(64,2A), the head LINEAR; flat in Flux.params order like every network
 *                  (W3 is (2A, 64) column-major). Head rows 0..A−1 are the mean μ, rows A..2A−1 the raw s. Per component c, in this order:
 *                    t = tanh_fast(s); log_std = −5 + 3.5·(t + 1)  ∈ [−5, 2]; σ = exp(log_std);
 *                    for a normal ε: u = μ + σ·ε; y = tanh_fast(u); a = scale·y + bias, scale = (act_high − act_low)/2, bias = (act_high + act_low)/2;
 *                    lp_c = ((−0.5·(ε·ε) − log_std) − 0.9189385332046727) − log(scale·(1 − y·y) + 1e-6);
 *                  logπ = Σ_c lp_c, c ascending, from 0.0. tanh_fast returns exactly ±1 past |x| > 30: 1 − y·y is then exactly 0 and the log sees 1e-6.
 *                  The deterministic action is scale·tanh_fast(μ) + bias. There is no target actor.
 *   temperature    log_alpha: one Float32 scalar with its own Adam(lr) moments and β-power pair. α of an update = exp((double)log_alpha) as it
 *                  stands BEFORE that update's alpha step; the critic pass, the actor pass, both logged losses and the alpha record use that α.
 *   next action    a', logπ' from the CURRENT actor on next_state, ε = the Box–Muller normal of the DDPG block on Philox stream 0x18 at gstep = g,
 *                  component word 16·b + c (one draw per sample and component).
 *   TD target      qmin' = q2 < q1 ? q2 : q1 of target critic 1 / 2 on (next_state, a'); td = r + (γ·(1 − terminal))·(qmin' − α·logπ').
 *   critics        as TD3: critic i takes Σ_b (td − q_i)² / k, both step on every update; critic_loss = loss_1 + loss_2.
 *   actor          on every update: a, logπ on state with ε on stream 0x19, same component word; q1, q2 of the UPDATED critics on (state, a);
 *                  qmin = q2 < q1 ? q2 : q1; actor_loss = (Σ_b (α·logπ_b − qmin_b)) / k. Its gradient, per sample: ga[c] = ∂(−Q_sel/k)/∂a[c] through the
 *                  selected critic (critic 2 where q2 < q1, else critic 1) by DDPG's pullback (cotangent −1/k, relu masks, Σ_i W1[i, D + c]·δ1[i]);
 *                    omy = 1 − y·y; den = scale·omy + 1e-6; ak = α/k;
 *                    dy = ga·scale + ak·((2·scale·y)/den); du = dy·omy;
 *                    δ3[c] = du (the μ row); dls = du·(σ·ε) − ak; δ3[A + c] = (dls·3.5)·(1 − t·t) (the s row);
 *                  δ2[j] = (Σ_r W3[r, j]·δ3[r], r = 0..2A−1 ascending)·(1 − h2[j]²), δ1 as DDPG's actor; Adam on the actor.
 *   alpha          alpha_loss = −(α·((Σ_b (logπ_b + target_entropy)) / k)) with the actor pass's logπ (no resampling); it is also its own derivative
 *                  with respect to log_alpha. With autotune = 1: Adam on log_alpha with that gradient (projected to Float32) — after the passes of
 *                  this update have read α. With autotune = 0 log_alpha, its moments and its β powers never change a bit; alpha_loss is still
 *                  reported. entropy = −((Σ_b logπ_b) / k).
 *   targets        polyak(tau) of both critic targets from the updated critics, on every update.
 *   behaviour      while global_step <= warmup_steps: the rand(act_space) draw; after that a sample a from the actor with ε on stream 0x10,
 *                  component word c, unclipped (it lies inside the bounds).
 * One cycle stays six launches (csrc/ddpg.hip, csrc/sac.hpp): sample, sac_critic_kernel, td3_critic_step, sac_actor_kernel, sac_actor_step (actor
 * Adam, both polyaks, the alpha step), sac_collect_kernel (19 β-power pairs, the alpha pair only with autotune = 1; the loss and alpha records).
 * crl_ddpg_run, _act, _observe, _read_losses, _read_buffer, _status_read, _actor (scale·tanh_fast(μ) + bias), _q_values (critic 1), _evaluate
 * (actions = crl_ddpg_actor's, q0 = critic 1's, bit for bit) and _destroy take a SAC handle. The crl_ddpg_* and crl_td3_* parameter calls refuse a
 * SAC handle and name the crl_sac_* twin; every crl_sac_* call refuses the other two kinds.
 * ===================================================================================================== */
typedef struct crl_sac_options { int32_t autotune, pad; double alpha, target_entropy; } crl_sac_options;   /* 24 bytes; log_alpha = (float)log(alpha) */
typedef struct crl_sac_status { double alpha, alpha_loss, entropy; float log_alpha; int32_t pad; } crl_sac_status;   /* α, losses of the last update (α =
                                     the option's alpha, the others 0.0 before the first); log_alpha as it stands now */
typedef struct crl_sac_alpha_record { int64_t global_step; double alpha, alpha_loss, entropy; } crl_sac_alpha_record;
/* lengths of the actor (head of 2·act_dim rows) and of one critic */
int32_t crl_sac_param_count(int32_t obs_dim, int32_t act_dim, int64_t* actor_n, int64_t* critic_n);
/* crl_ddpg_create's checks, and — each message naming its field — NULL options, alpha <= 0 (or not finite), a non-finite target_entropy, autotune
 * outside {0, 1}, noise_in_update != 0. */
int32_t crl_sac_create(const crl_ddpg_config* cfg, const crl_sac_options* opt, int32_t device, crl_ddpg** out);
/* host-only: glorot_uniform weights and zero biases. Critic 1 and critic 2 are crl_td3_init_params' for the same seed (the critics of
 * crl_ddpg_make_nn(seed) and of crl_ddpg_make_nn(seed + 1)); the actor is drawn layer by layer (64×D, 64×64, 2A×64) from the generator
 * crl_ddpg_make_nn uses, seeded with seed ^ 0x5AC. */
int32_t crl_sac_make_nn(int32_t obs_dim, int32_t act_dim, uint64_t seed, float* actor, size_t na, float* critic1, size_t nc, float* critic2, size_t nc2);
int32_t crl_sac_init_params(crl_ddpg* h, uint64_t seed);
/* actor, critic 1, critic 2; the two critic targets are copies */
int32_t crl_sac_write_params(crl_ddpg* h, const float* actor, size_t na, const float* critic1, size_t nc, const float* critic2, size_t nc2);
/* any may be NULL */
int32_t crl_sac_read_params(crl_ddpg* h, float* actor, float* critic1, float* critic2, float* t_critic1, float* t_critic2, float* log_alpha);
/* crl_td3_q_values' twin */
int32_t crl_sac_q_values(crl_ddpg* h, const double* obs, const double* act, int32_t n, double* q1, double* q2);
int32_t crl_sac_status_read(crl_ddpg* h, crl_sac_status* out);
/* one record for each loss record that the last crl_ddpg_run / crl_ddpg_read_losses call on this handle returned: same order, same count, same
 * global_step (entries beyond max_records are dropped) */
int32_t crl_sac_alpha_records(crl_ddpg* h, crl_sac_alpha_record* records, int32_t max_records, int32_t* n_records);

#ifdef __cplusplus
}
#endif
#endif
