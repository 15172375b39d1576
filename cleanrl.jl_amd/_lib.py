"""ctypes binding of libcleanrl_hip.so (include/cleanrl_hip.h).

There is NO CPU fallback anywhere in this package: if the HIP library is missing the import of this module raises,
and every compute entry point returns an error when no GPU is present.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CRL_LIB_PATH") or os.path.join(_HERE, "libcleanrl_hip.so")   # CRL_LIB_PATH: build-variant experiments


class CrlError(RuntimeError):
    pass


class CrlConfig(C.Structure):
    """crl_ppo_config — mirror of PPOConfig (ppo.jl:1-19) + shapes."""
    _fields_ = [
        ("total_timesteps", C.c_int64), ("num_steps", C.c_int32), ("num_envs", C.c_int32),
        ("num_minibatches", C.c_int32), ("update_epochs", C.c_int32), ("lr", C.c_float), ("gamma", C.c_float),
        ("gae_lambda", C.c_float), ("clip_coef", C.c_float), ("ent_coeff", C.c_float), ("v_coef", C.c_float),
        ("normalize_advantages", C.c_int32), ("clip_value_loss", C.c_int32), ("anneal_lr", C.c_int32),
        ("obs_dim", C.c_int32), ("n_act", C.c_int32), ("hidden", C.c_int32), ("gae_mode", C.c_int32),
        ("env_kind", C.c_int32), ("stale_obs", C.c_int32), ("env_id_offset", C.c_int32), ("shuffle_mode", C.c_int32),
        ("seed", C.c_uint64),
    ]


class CrlStats(C.Structure):
    _fields_ = [(n, C.c_double) for n in
                ("loss", "pg_loss", "v_loss", "entropy_loss", "adv_mean", "adv_std", "u_value", "n_unclipped_wins")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class CrlEpisodeRecord(C.Structure):
    _fields_ = [("episode_return", C.c_float), ("episode_length", C.c_int32), ("env", C.c_int32), ("step", C.c_int32)]


class CrlEpisodeStats(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("episodes", "return_sum", "length_sum", "return_max")]


class CrlIterationReport(C.Structure):
    """crl_ppo_iteration_report: whose records crl_ppo_iterate_async / crl_ppo_drain handed back."""
    _fields_ = [("iteration", C.c_int64), ("episodes", CrlEpisodeStats), ("n_episodes", C.c_int64), ("n_ring", C.c_int32), ("pad", C.c_int32)]


class CrlEvalConfig(C.Structure):
    """crl_eval_config: what crl_ppo_evaluate runs (mode: EVAL_GREEDY / EVAL_SAMPLE)."""
    _fields_ = [("num_envs", C.c_int32), ("episodes_per_env", C.c_int32), ("mode", C.c_int32), ("trace_steps", C.c_int32), ("seed", C.c_uint64)]


class CrlEvalReport(C.Structure):
    """crl_eval_report: Float64 summary of the per-episode arrays (population standard deviation; env_steps = sum of the lengths)."""
    _fields_ = [("episodes", C.c_int64), ("env_steps", C.c_int64), ("return_mean", C.c_double), ("return_std", C.c_double),
                ("return_min", C.c_double), ("return_max", C.c_double), ("length_mean", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class CrlValueEvalReport(C.Structure):
    """crl_value_eval_report: what crl_dqn_evaluate / crl_a2c_evaluate report (population standard deviation; v_bias_mean = mean(v0 - disc_return))."""
    _fields_ = [("episodes", C.c_int64), ("env_steps", C.c_int64)] + [(n, C.c_double) for n in (
        "return_mean", "return_std", "return_min", "return_max", "length_mean", "disc_return_mean", "v0_mean", "v_bias_mean")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class CrlDiag(C.Structure):
    """crl_ppo_diag: raw Float64 sums of crl_ppo_diagnose over the resident rollout buffer (shards add them field by field; min / max for ratio_*)
    and the fields derived from them (entropy = policy entropy per sample = n_act x the reference's entropy_loss)."""
    _fields_ = ([("n", C.c_int64), ("n_clipped", C.c_int64)] + [(n, C.c_double) for n in (
        "sum_logratio", "sum_kl", "sum_entropy", "ratio_min", "ratio_max",
        "sum_ret", "sum_ret2", "sum_res_old", "sum_res_old2", "sum_res_new", "sum_res_new2",
        "old_approx_kl", "approx_kl", "clipfrac", "entropy", "explained_variance", "explained_variance_new")])

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


# every symbol include/cleanrl_hip.h declares (tests check the library exports all of them)
EXPORTS = [
    "crl_version", "crl_last_error", "crl_device_count", "crl_ppo_create", "crl_ppo_destroy", "crl_ppo_param_count",
    "crl_sync", "crl_ppo_write", "crl_ppo_read", "crl_policy_act", "crl_logprob_actions", "crl_gae",
    "crl_rollout_store", "crl_env_reset", "crl_rollout_run", "crl_episode_stats_read", "crl_compute_gae",
    "crl_shuffle", "crl_adv_stats", "crl_ppo_update_minibatch", "crl_ppo_iterate", "crl_ppo_iteration",
    "crl_comm_unique_id", "crl_comm_init", "crl_comm_init_external", "crl_comm_peer_export", "crl_comm_peer_attach", "crl_adv_stats_local", "crl_adv_stats_finish",
    "crl_prof_enable", "crl_prof_read", "crl_prof_reset", "crl_ppo_exact_reruns", "crl_episode_ring_enable",
    "crl_episode_ring_read", "crl_comm_destroy", "crl_ppo_set_option", "crl_ppo_get_option", "crl_ppo_option_name", "crl_ppo_option_count", "crl_gae_bench", "crl_gae_opt",
    "crl_a2c_create", "crl_a2c_destroy", "crl_a2c_param_count", "crl_a2c_write_params", "crl_a2c_read_params", "crl_a2c_read_grads",
    "crl_a2c_read_env", "crl_a2c_read_buffer", "crl_a2c_run_until_update", "crl_a2c_discounted_future_rewards",
    "crl_dqn_create", "crl_dqn_destroy", "crl_dqn_write_params", "crl_dqn_read_params", "crl_dqn_status_read", "crl_dqn_run",
    "crl_dqn_q_values", "crl_dqn_evaluate", "crl_dqn_eval_envs_per_block", "crl_dqn_per_create", "crl_dqn_per_status_read", "crl_dqn_per_read",
    "crl_dqn_per_probe", "crl_dqn_create_with", "crl_dqn_target_read", "crl_dqn_nstep_probe",
    "crl_dqn_c51_create", "crl_dqn_param_count", "crl_dqn_c51_make_nn", "crl_dqn_c51_probs", "crl_dqn_c51_read", "crl_dqn_c51_project_probe",
    "crl_dqn_dueling_create", "crl_dqn_dueling_make_nn", "crl_dqn_dueling_streams",
    "crl_dqn_noisy_create", "crl_dqn_noisy_make_nn", "crl_dqn_noisy_weights", "crl_dqn_noisy_noise_count", "crl_dqn_noisy_noise", "crl_a2c_forward", "crl_a2c_evaluate", "crl_a2c_eval_envs_per_block",
    "crl_ddpg_param_count", "crl_ddpg_create", "crl_ddpg_destroy", "crl_ddpg_write_params", "crl_ddpg_read_params", "crl_ddpg_make_nn",
    "crl_ddpg_init_params", "crl_ddpg_status_read", "crl_ddpg_run", "crl_ddpg_act", "crl_ddpg_observe", "crl_ddpg_read_losses",
    "crl_ddpg_read_buffer", "crl_ddpg_actor", "crl_ddpg_q_values", "crl_ddpg_evaluate",
    "crl_td3_create", "crl_td3_write_params", "crl_td3_read_params", "crl_td3_init_params", "crl_td3_q_values",
    "crl_sac_param_count", "crl_sac_create", "crl_sac_make_nn", "crl_sac_init_params", "crl_sac_write_params", "crl_sac_read_params",
    "crl_sac_q_values", "crl_sac_status_read", "crl_sac_alpha_records",
    "crl_make_actor_critic", "crl_ppo_init_params", "crl_a2c_init_params", "crl_dqn_make_nn", "crl_dqn_init_params", "crl_comm_info", "crl_clock_probe", "crl_product_probe", "crl_ppo_iterate_async", "crl_ppo_drain",
    "crl_env_step", "crl_ppo_evaluate", "crl_ppo_diagnose",
    "crl_ppo_stream", "crl_rollout_act_device", "crl_rollout_record_device", "crl_env_step_device", "crl_ppo_update",
]

DQN_PARAM_COUNT = 10934


class CrlDQNConfig(C.Structure):
    """crl_dqn_config — mirror of DQNConfig (dqn.jl:1-19)."""
    _fields_ = [("log_frequency", C.c_int64), ("total_timesteps", C.c_int64), ("buffer_size", C.c_int64), ("min_buff_size", C.c_int64),
                ("lr", C.c_double), ("train_freq", C.c_int64), ("target_net_freq", C.c_int64), ("batch_size", C.c_int64),
                ("gamma", C.c_double), ("epsilon_start", C.c_double), ("epsilon_end", C.c_double), ("epsilon_duration", C.c_double),
                ("max_steps", C.c_int32), ("pad", C.c_int32), ("seed", C.c_uint64)]


class CrlDQNEpisode(C.Structure):
    _fields_ = [("episode_return", C.c_double), ("episode_length", C.c_int64), ("global_step", C.c_int64), ("epsilon", C.c_double)]


class CrlDQNLossRecord(C.Structure):
    _fields_ = [("global_step", C.c_int64), ("loss", C.c_double)]


class CrlDQNStatus(C.Structure):
    _fields_ = [("env_state", C.c_double * 4), ("global_step", C.c_int64), ("rb_size", C.c_int64), ("n_updates", C.c_int64),
                ("last_loss", C.c_double)]


class CrlDQNPEROptions(C.Structure):
    """crl_dqn_per_options: what prioritized replay adds to crl_dqn_config (40 bytes)."""
    _fields_ = [("alpha", C.c_double), ("beta_start", C.c_double), ("beta_end", C.c_double), ("beta_duration", C.c_double), ("eps", C.c_double)]


class CrlDQNPERStatus(C.Structure):
    _fields_ = [("beta", C.c_double), ("total", C.c_double), ("max_leaf", C.c_float), ("tree_leaves", C.c_int32)]


class CrlDQNTargetOptions(C.Structure):
    """crl_dqn_target_options: how the TD target is formed (8 bytes); {1, 0} is dqn.jl's 1-step max over target_net."""
    _fields_ = [("n_step", C.c_int32), ("double_q", C.c_int32)]


class CrlDQNC51Options(C.Structure):
    """crl_dqn_c51_options: the categorical head's support (24 bytes): n_atoms in 2..64 on [v_min, v_max]."""
    _fields_ = [("n_atoms", C.c_int32), ("pad", C.c_int32), ("v_min", C.c_double), ("v_max", C.c_double)]


def dqn_c51_param_count(n_atoms):
    """10764 + 85·2N: the trunk W1 b1 W2 b2 and the head W3(2N, 84) b3(2N)"""
    return 10764 + 85 * 2 * int(n_atoms)


class CrlDQNNoisyOptions(C.Structure):
    """crl_dqn_noisy_options: noisy linear layers (8 bytes): sigma = sigma0 / sqrt(in) at init, sigma0 in 0..10."""
    _fields_ = [("sigma0", C.c_double)]



DDPG_ENV_PENDULUM, DDPG_ENV_EXTERNAL = 0, 1


class CrlDDPGConfig(C.Structure):
    """crl_ddpg_config — mirror of DDPGConfig (ddpg.jl:1-15) + shapes, env, action bounds and the noise switch."""
    _fields_ = [("total_timesteps", C.c_int64), ("buffer_size", C.c_int64), ("min_buff_size", C.c_int64), ("batch_size", C.c_int64),
                ("warmup_steps", C.c_int64), ("log_frequency", C.c_int64),
                ("lr", C.c_double), ("tau", C.c_double), ("gamma", C.c_double), ("exploration_noise", C.c_double),
                ("obs_dim", C.c_int32), ("act_dim", C.c_int32), ("env_kind", C.c_int32), ("max_steps", C.c_int32),
                ("act_low", C.c_double), ("act_high", C.c_double), ("noise_in_update", C.c_int32), ("pad", C.c_int32), ("seed", C.c_uint64)]


class CrlTD3Options(C.Structure):
    """crl_td3_options: what TD3 adds to crl_ddpg_config."""
    _fields_ = [("policy_delay", C.c_int32), ("pad", C.c_int32), ("policy_noise", C.c_double), ("noise_clip", C.c_double)]


class CrlSACOptions(C.Structure):
    """crl_sac_options: what SAC adds to crl_ddpg_config (log_alpha starts at float32(log(alpha)))."""
    _fields_ = [("autotune", C.c_int32), ("pad", C.c_int32), ("alpha", C.c_double), ("target_entropy", C.c_double)]


class CrlSACStatus(C.Structure):
    _fields_ = [("alpha", C.c_double), ("alpha_loss", C.c_double), ("entropy", C.c_double), ("log_alpha", C.c_float), ("pad", C.c_int32)]


class CrlSACAlphaRecord(C.Structure):
    _fields_ = [("global_step", C.c_int64), ("alpha", C.c_double), ("alpha_loss", C.c_double), ("entropy", C.c_double)]


class CrlDDPGEpisode(C.Structure):
    _fields_ = [("episode_return", C.c_double), ("episode_length", C.c_int64), ("global_step", C.c_int64)]


class CrlDDPGLossRecord(C.Structure):
    _fields_ = [("global_step", C.c_int64), ("actor_loss", C.c_double), ("critic_loss", C.c_double)]


class CrlDDPGStatus(C.Structure):
    _fields_ = [("theta", C.c_double), ("theta_dot", C.c_double), ("env_t", C.c_int64), ("global_step", C.c_int64), ("rb_size", C.c_int64),
                ("rb_ptr", C.c_int64), ("n_updates", C.c_int64), ("actor_loss", C.c_double), ("critic_loss", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class CrlDDPGEvalConfig(C.Structure):
    """crl_ddpg_eval_config: what crl_ddpg_evaluate runs."""
    _fields_ = [("num_envs", C.c_int32), ("episodes_per_env", C.c_int32), ("trace_steps", C.c_int32), ("pad", C.c_int32), ("seed", C.c_uint64)]


class CrlDDPGEvalReport(C.Structure):
    """crl_ddpg_eval_report: Float64 summary of the per-episode arrays (population standard deviation; q_bias_mean = mean(q0 - disc_return))."""
    _fields_ = [("episodes", C.c_int64), ("env_steps", C.c_int64)] + [(n, C.c_double) for n in (
        "return_mean", "return_std", "return_min", "return_max", "disc_return_mean", "q0_mean", "q_bias_mean")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class CrlA2CConfig(C.Structure):
    """crl_a2c_config — mirror of A2CConfig (a2c.jl:1-10)."""
    _fields_ = [("lr", C.c_double), ("total_timesteps", C.c_int64), ("min_replay_size", C.c_int32), ("max_steps", C.c_int32),
                ("gamma", C.c_double), ("seed", C.c_uint64)]


class CrlA2CTrainStats(C.Structure):
    _fields_ = [("actor_loss", C.c_double), ("critic_loss", C.c_double), ("n", C.c_int32), ("trained", C.c_int32)]


class CrlA2CEpisode(C.Structure):
    _fields_ = [("episode_return", C.c_double), ("episode_length", C.c_int64), ("global_step", C.c_int64)]


# crl_field
F_OBS, F_ACTION, F_LOGPROB, F_REWARD, F_TERMINAL, F_VALUE, F_ADVANTAGE, F_RETURN, F_PERM, F_PARAMS, F_GRADS, F_ADAM_M, \
    F_ADAM_V, F_ENV_STATE, F_CUR_OBS, F_NEXT_DONE, F_ENV_T, F_BETAP, F_ADV_SUMS = range(19)
GAE_COMPAT, GAE_FIXED = 0, 1
ENV_CARTPOLE, ENV_SYNTHETIC, ENV_EXTERNAL, ENV_MOUNTAINCAR, ENV_ACROBOT = 0, 1, 2, 3, 4
EVAL_GREEDY, EVAL_SAMPLE = 0, 1
SHUFFLE_FISHER_YATES, SHUFFLE_BIJECTION, SHUFFLE_BLOCKED_FY = 0, 1, 2
K_ROLLOUT, K_GAE, K_SHUFFLE, K_ADV_STATS, K_UPDATE, K_REDUCE, K_OPTIM, K_ALLREDUCE, K_PACK, K_PERMUTE = range(10)
KERNEL_NAMES = ["rollout", "gae", "shuffle", "adv_stats", "update", "reduce", "optim", "allreduce", "pack", "permute"]

_lib = None


def load():
    """Loads the in-tree HIP library; raises (never falls back) when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise CrlError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    vp, fp, ip, dp, u8p = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_uint8)
    L.crl_version.restype = C.c_int32
    L.crl_last_error.restype = C.c_char_p
    L.crl_device_count.argtypes = [ip]
    L.crl_ppo_create.argtypes = [C.POINTER(CrlConfig), C.c_int32, C.POINTER(vp)]
    L.crl_ppo_destroy.argtypes = [vp]
    L.crl_ppo_param_count.argtypes = [vp, C.POINTER(C.c_int64)]
    L.crl_sync.argtypes = [vp]
    L.crl_ppo_write.argtypes = [vp, C.c_int32, vp, C.c_size_t]
    L.crl_ppo_read.argtypes = [vp, C.c_int32, vp, C.c_size_t]
    L.crl_policy_act.argtypes = [vp, fp, dp, C.c_int32, ip, fp, fp]
    L.crl_logprob_actions.argtypes = [vp, fp, ip, C.c_int32, fp, fp]
    L.crl_gae.argtypes = [C.c_int32, fp, fp, u8p, fp, u8p, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_int32, fp, fp]
    L.crl_gae_opt.argtypes = L.crl_gae.argtypes + [C.c_int32] * 3
    L.crl_rollout_store.argtypes = [vp, C.c_int32, fp, ip, fp, fp, u8p, fp]
    L.crl_env_reset.argtypes = [vp]
    L.crl_rollout_run.argtypes = [vp]
    L.crl_env_step.argtypes = [vp, ip, C.c_uint64, fp, fp, u8p]
    L.crl_ppo_evaluate.argtypes = [vp, C.POINTER(CrlEvalConfig), C.POINTER(CrlEvalReport), fp, ip, ip]
    L.crl_ppo_diagnose.argtypes = [vp, C.POINTER(CrlDiag), fp, fp]
    L.crl_episode_stats_read.argtypes = [vp, C.POINTER(CrlEpisodeStats)]
    L.crl_compute_gae.argtypes = [vp]
    L.crl_shuffle.argtypes = [vp, C.c_uint64]
    L.crl_adv_stats.argtypes = [vp]
    L.crl_ppo_update_minibatch.argtypes = [vp, C.c_int32, C.c_double, C.c_int32, C.POINTER(CrlStats)]
    L.crl_ppo_iterate.argtypes = [vp, C.c_int32, C.POINTER(CrlStats)]
    L.crl_ppo_iteration.argtypes = [vp, C.POINTER(C.c_int64)]
    L.crl_comm_unique_id.argtypes = [u8p]
    L.crl_comm_init.argtypes = [vp, u8p, C.c_int32, C.c_int32]
    L.crl_comm_init_external.argtypes = [vp, C.c_int32, C.c_int32]
    L.crl_comm_peer_export.argtypes = [vp, C.c_int32, C.c_int32, u8p]
    L.crl_comm_peer_attach.argtypes = [vp, u8p]
    L.crl_adv_stats_local.argtypes = [vp]
    L.crl_adv_stats_finish.argtypes = [vp]
    L.crl_prof_enable.argtypes = [vp, C.c_int32]
    L.crl_prof_read.argtypes = [vp, C.c_int32, dp, C.POINTER(C.c_int64)]
    L.crl_prof_reset.argtypes = [vp]
    i64p = C.POINTER(C.c_int64)
    L.crl_ppo_exact_reruns.argtypes = [vp, i64p]
    L.crl_episode_ring_enable.argtypes = [vp, C.c_int32]
    L.crl_episode_ring_read.argtypes = [vp, C.POINTER(CrlEpisodeRecord), C.c_int32, ip, i64p]
    L.crl_comm_destroy.argtypes = [vp]
    L.crl_ppo_set_option.argtypes = [vp, C.c_char_p, C.c_int64]
    L.crl_ppo_get_option.argtypes = [vp, C.c_char_p, i64p]
    L.crl_ppo_option_name.argtypes = [C.c_int32, C.POINTER(C.c_char_p), i64p]
    L.crl_ppo_option_count.argtypes = [ip]
    L.crl_gae_bench.argtypes = [C.c_int32] * 8 + [dp, dp]
    L.crl_a2c_create.argtypes = [C.POINTER(CrlA2CConfig), C.c_int32, C.POINTER(vp)]
    L.crl_a2c_destroy.argtypes = [vp]
    L.crl_a2c_param_count.argtypes = [vp, i64p]
    L.crl_a2c_write_params.argtypes = [vp, fp, C.c_size_t]
    L.crl_a2c_read_params.argtypes = [vp, fp, C.c_size_t]
    L.crl_a2c_read_grads.argtypes = [vp, fp, C.c_size_t]
    L.crl_a2c_read_env.argtypes = [vp, dp, i64p, ip]
    L.crl_a2c_read_buffer.argtypes = [vp, dp, ip, dp, u8p, C.c_int32]
    L.crl_a2c_run_until_update.argtypes = [vp, C.c_int64, C.POINTER(CrlA2CTrainStats), C.POINTER(CrlA2CEpisode), C.c_int32, ip, i64p]
    L.crl_a2c_discounted_future_rewards.argtypes = [C.c_int32, dp, u8p, C.c_int32, C.c_double, C.c_double, dp]
    L.crl_dqn_create.argtypes = [C.POINTER(CrlDQNConfig), C.c_int32, C.POINTER(vp)]
    L.crl_dqn_destroy.argtypes = [vp]
    L.crl_dqn_write_params.argtypes = [vp, fp, C.c_size_t]
    L.crl_dqn_read_params.argtypes = [vp, fp, fp, C.c_size_t]
    L.crl_dqn_status_read.argtypes = [vp, C.POINTER(CrlDQNStatus)]
    L.crl_dqn_run.argtypes = [vp, C.c_int64, C.POINTER(CrlDQNEpisode), C.c_int32, ip, C.POINTER(CrlDQNLossRecord), C.c_int32, ip, i64p]
    L.crl_dqn_q_values.argtypes = [vp, dp, C.c_int32, dp]
    L.crl_dqn_evaluate.argtypes = [vp, C.POINTER(CrlEvalConfig), C.POINTER(CrlValueEvalReport), dp, ip, dp, dp, ip]
    L.crl_dqn_eval_envs_per_block.argtypes = []
    L.crl_dqn_per_create.argtypes = [C.POINTER(CrlDQNConfig), C.POINTER(CrlDQNPEROptions), C.c_int32, C.POINTER(vp)]
    L.crl_dqn_per_status_read.argtypes = [vp, C.POINTER(CrlDQNPERStatus)]
    L.crl_dqn_per_read.argtypes = [vp, fp, dp, ip, dp, dp]
    L.crl_dqn_per_probe.argtypes = [vp, fp, C.c_int32, C.c_uint64, C.c_int32, C.c_double, ip, dp, dp]
    L.crl_dqn_create_with.argtypes = [C.POINTER(CrlDQNConfig), C.POINTER(CrlDQNPEROptions), C.POINTER(CrlDQNTargetOptions), C.c_int32, C.POINTER(vp)]
    L.crl_dqn_target_read.argtypes = [vp, ip, ip, dp, dp, ip, dp]
    L.crl_dqn_nstep_probe.argtypes = [vp, dp, C.POINTER(C.c_uint8), C.c_int32, C.c_int32, ip, C.c_int32, C.c_int32, C.c_double, ip, ip, dp, dp]
    L.crl_a2c_forward.argtypes = [vp, C.c_int32, dp, C.c_int32, dp]
    L.crl_dqn_c51_create.argtypes = [C.POINTER(CrlDQNConfig), C.POINTER(CrlDQNC51Options), C.POINTER(CrlDQNPEROptions), C.POINTER(CrlDQNTargetOptions),
                                     C.c_int32, C.POINTER(vp)]
    L.crl_dqn_param_count.argtypes = [vp, C.POINTER(C.c_size_t)]
    L.crl_dqn_c51_make_nn.argtypes = [C.c_uint64, C.c_int32, fp, C.c_size_t]
    L.crl_dqn_c51_probs.argtypes = [vp, dp, C.c_int32, dp]
    L.crl_dqn_c51_read.argtypes = [vp, dp, dp]
    L.crl_dqn_c51_project_probe.argtypes = [vp, dp, dp, dp, C.POINTER(C.c_uint8), C.c_int32, dp]
    L.crl_dqn_dueling_create.argtypes = L.crl_dqn_c51_create.argtypes
    L.crl_dqn_dueling_make_nn.argtypes = [C.c_uint64, C.c_int32, fp, C.c_size_t]
    L.crl_dqn_dueling_streams.argtypes = [vp, dp, C.c_int32, dp, dp]
    L.crl_dqn_noisy_create.argtypes = [C.POINTER(CrlDQNConfig), C.POINTER(CrlDQNNoisyOptions), C.c_int32, C.POINTER(CrlDQNC51Options),
                                       C.POINTER(CrlDQNPEROptions), C.POINTER(CrlDQNTargetOptions), C.c_int32, C.POINTER(vp)]
    L.crl_dqn_noisy_make_nn.argtypes = [C.c_uint64, C.c_double, C.c_int32, C.c_int32, fp, C.c_size_t]
    L.crl_dqn_noisy_weights.argtypes = [vp, C.c_int32, fp, C.c_size_t]
    L.crl_dqn_noisy_noise_count.argtypes = [vp, C.POINTER(C.c_size_t)]
    L.crl_dqn_noisy_noise.argtypes = [vp, C.c_uint64, C.c_int32, fp, C.c_size_t]
    L.crl_a2c_evaluate.argtypes = L.crl_dqn_evaluate.argtypes
    L.crl_a2c_eval_envs_per_block.argtypes = []
    L.crl_ddpg_param_count.argtypes = [C.c_int32, C.c_int32, i64p, i64p]
    L.crl_ddpg_create.argtypes = [C.POINTER(CrlDDPGConfig), C.c_int32, C.POINTER(vp)]
    L.crl_ddpg_destroy.argtypes = [vp]
    L.crl_ddpg_write_params.argtypes = [vp, fp, C.c_size_t, fp, C.c_size_t]
    L.crl_ddpg_read_params.argtypes = [vp, fp, fp, fp, fp]
    L.crl_ddpg_make_nn.argtypes = [C.c_int32, C.c_int32, C.c_uint64, fp, C.c_size_t, fp, C.c_size_t]
    L.crl_ddpg_init_params.argtypes = [vp, C.c_uint64]
    L.crl_ddpg_status_read.argtypes = [vp, C.POINTER(CrlDDPGStatus)]
    L.crl_ddpg_run.argtypes = [vp, C.c_int64, C.POINTER(CrlDDPGEpisode), C.c_int32, ip, C.POINTER(CrlDDPGLossRecord), C.c_int32, ip, i64p]
    L.crl_ddpg_act.argtypes = [vp, dp, dp]
    L.crl_ddpg_observe.argtypes = [vp, dp, dp, C.c_double, dp, C.c_int32]
    L.crl_ddpg_read_losses.argtypes = [vp, C.POINTER(CrlDDPGLossRecord), C.c_int32, ip]
    L.crl_ddpg_read_buffer.argtypes = [vp, dp, dp, dp, dp, u8p, C.c_int64, i64p, i64p]
    L.crl_ddpg_actor.argtypes = [vp, dp, C.c_int32, dp]
    L.crl_ddpg_q_values.argtypes = [vp, dp, dp, C.c_int32, dp]
    L.crl_ddpg_evaluate.argtypes = [vp, C.POINTER(CrlDDPGEvalConfig), C.POINTER(CrlDDPGEvalReport), dp, dp, dp, dp]
    L.crl_td3_create.argtypes = [C.POINTER(CrlDDPGConfig), C.POINTER(CrlTD3Options), C.c_int32, C.POINTER(vp)]
    L.crl_td3_write_params.argtypes = [vp, fp, C.c_size_t, fp, C.c_size_t, fp, C.c_size_t]
    L.crl_td3_read_params.argtypes = [vp, fp, fp, fp, fp, fp, fp]
    L.crl_td3_init_params.argtypes = [vp, C.c_uint64]
    L.crl_td3_q_values.argtypes = [vp, dp, dp, C.c_int32, dp, dp]
    L.crl_sac_param_count.argtypes = [C.c_int32, C.c_int32, i64p, i64p]
    L.crl_sac_create.argtypes = [C.POINTER(CrlDDPGConfig), C.POINTER(CrlSACOptions), C.c_int32, C.POINTER(vp)]
    L.crl_sac_make_nn.argtypes = [C.c_int32, C.c_int32, C.c_uint64, fp, C.c_size_t, fp, C.c_size_t, fp, C.c_size_t]
    L.crl_sac_init_params.argtypes = [vp, C.c_uint64]
    L.crl_sac_write_params.argtypes = [vp, fp, C.c_size_t, fp, C.c_size_t, fp, C.c_size_t]
    L.crl_sac_read_params.argtypes = [vp, fp, fp, fp, fp, fp, fp]
    L.crl_sac_q_values.argtypes = [vp, dp, dp, C.c_int32, dp, dp]
    L.crl_sac_status_read.argtypes = [vp, C.POINTER(CrlSACStatus)]
    L.crl_sac_alpha_records.argtypes = [vp, C.POINTER(CrlSACAlphaRecord), C.c_int32, ip]
    L.crl_make_actor_critic.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_uint64, fp, C.c_size_t]
    L.crl_ppo_init_params.argtypes = [vp, C.c_uint64]
    L.crl_a2c_init_params.argtypes = [vp, C.c_uint64]
    L.crl_dqn_make_nn.argtypes = [C.c_uint64, fp, C.c_size_t]
    L.crl_dqn_init_params.argtypes = [vp, C.c_uint64]
    L.crl_comm_info.argtypes = [C.c_char_p, C.c_size_t, ip]
    L.crl_clock_probe.argtypes = [C.c_int32, C.c_double, dp, dp, dp]
    L.crl_ppo_iterate_async.argtypes = [vp, C.POINTER(CrlIterationReport), C.POINTER(CrlStats), C.POINTER(CrlEpisodeRecord), C.c_int32]
    L.crl_ppo_drain.argtypes = [vp, C.POINTER(CrlIterationReport), C.POINTER(CrlStats), C.POINTER(CrlEpisodeRecord), C.c_int32]
    # device-pointer path: addresses travel as plain integers (devptr() below), never as host arrays
    L.crl_ppo_stream.argtypes = [vp, C.POINTER(vp)]
    L.crl_rollout_act_device.argtypes = [vp, C.c_int32, vp, vp, vp, vp]
    L.crl_rollout_record_device.argtypes = [vp, C.c_int32, vp, vp, vp, vp]
    L.crl_env_step_device.argtypes = [vp, vp, C.c_uint64, vp, vp, vp, vp]
    L.crl_ppo_update.argtypes = [vp, C.POINTER(CrlStats)]
    L.crl_product_probe.argtypes = [C.c_int32, C.c_int32, fp, fp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float, fp, fp]
    for name in EXPORTS:
        if name not in ("crl_version", "crl_last_error"):
            getattr(L, name).restype = C.c_int32
    _lib = L
    return L


def check(rc):
    if rc != 0:
        raise CrlError(load().crl_last_error().decode("utf-8", "replace"))


def device_count():
    n = C.c_int32(0)
    rc = load().crl_device_count(C.byref(n))
    return n.value if rc == 0 else 0


def _ptr(a, ct):
    return a.ctypes.data_as(C.POINTER(ct))


def devptr(x, what="pointer", optional=False):
    """The device address behind a pointer argument of the device-pointer calls: an int address or any object with data_ptr() (a torch tensor) —
    nothing else (a numpy array is HOST memory). 0 / None is a ValueError unless `optional`; raised before the library is touched."""
    if x is None or (isinstance(x, int) and not isinstance(x, bool) and x == 0):
        if optional:
            return None
        raise ValueError(f"{what}: a device pointer is required, got {x!r}")
    if isinstance(x, bool) or not (isinstance(x, int) or hasattr(x, "data_ptr")):
        raise TypeError(f"{what}: an int device address or an object with data_ptr() is expected, got {type(x).__name__}")
    a = x if isinstance(x, int) else int(x.data_ptr())
    if a <= 0 or a >= 1 << 64:
        raise ValueError(f"{what}: {a:#x} is not a device address")
    return a


_hip = None


def hip_runtime():
    """libamdhip64 through ctypes (hipMalloc / hipFree / hipMemcpy / hipMemset / hipSetDevice): by name, else through libcleanrl_hip.so, which links it."""
    global _hip
    if _hip is None:
        load()
        try:
            R = C.CDLL("libamdhip64.so")
        except OSError:
            R = C.CDLL(LIB_PATH)
        R.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        R.hipFree.argtypes = [C.c_void_p]
        R.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        R.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
        R.hipSetDevice.argtypes = [C.c_int]
        R.hipGetErrorString.argtypes = [C.c_int]; R.hipGetErrorString.restype = C.c_char_p
        _hip = R
    return _hip


class DeviceBuffer:
    """`nbytes` of device memory from hipMalloc, zeroed; data_ptr() makes it a pointer argument of the device-pointer calls. read() / write() are
    synchronous hipMemcpy (tests and set-up only — nothing on the stepping path uses them)."""

    def __init__(self, nbytes, device=0):
        self._R = hip_runtime()
        self.nbytes, self.device = int(nbytes), device
        self._p = C.c_void_p()
        self._ok(self._R.hipSetDevice(device))
        self._ok(self._R.hipMalloc(C.byref(self._p), max(self.nbytes, 1)))
        self._ok(self._R.hipMemset(self._p, 0, max(self.nbytes, 1)))

    def _ok(self, rc):
        if rc != 0:
            raise CrlError("HIP runtime: " + self._R.hipGetErrorString(rc).decode("utf-8", "replace"))

    def data_ptr(self):
        return self._p.value or 0

    def write(self, arr):
        a = np.ascontiguousarray(arr) if not arr.flags.f_contiguous else arr
        if a.nbytes != self.nbytes:
            raise ValueError(f"DeviceBuffer.write: {self.nbytes} bytes expected, got {a.nbytes}")
        self._ok(self._R.hipMemcpy(self._p, a.ctypes.data_as(C.c_void_p), a.nbytes, 1))

    def read(self, dtype, shape=None, order="F"):
        out = np.zeros(self.nbytes // np.dtype(dtype).itemsize if shape is None else shape, dtype, order=order)
        self._ok(self._R.hipMemcpy(out.ctypes.data_as(C.c_void_p), self._p, out.nbytes, 2))
        return out

    def close(self):
        if self._p.value:
            self._R.hipFree(self._p)
            self._p = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def product_probe(flavour, A, B, chunks=1, scale_a=1.0, scale_b=1.0, col_scale=None, device=0):
    """crl_product_probe: A [rows, K] (C order), B [cols, K] (C order) float32 → C [chunks, cols, rows] float32 partial products."""
    A = np.ascontiguousarray(A, np.float32); B = np.ascontiguousarray(B, np.float32)
    rows, K = A.shape; cols = B.shape[0]
    out = np.zeros((chunks, cols, rows), np.float32)
    cs = None if col_scale is None else np.ascontiguousarray(col_scale, np.float32)
    check(load().crl_product_probe(device, flavour, _ptr(A, C.c_float), _ptr(B, C.c_float), rows, cols, K, chunks, scale_a, scale_b,
                                   None if cs is None else _ptr(cs, C.c_float), _ptr(out, C.c_float)))
    return out


def clock_probe(device=0, span_ms=5.0):
    """crl_clock_probe: shader clock under vector load, MHz (median, min, max over all waves of a chip-filling launch)."""
    med, lo, hi = C.c_double(0), C.c_double(0), C.c_double(0)
    check(load().crl_clock_probe(device, span_ms, C.byref(med), C.byref(lo), C.byref(hi)))
    return med.value, lo.value, hi.value


def comm_info():
    """crl_comm_info: (path of the librccl the library's all-reduce resolves to, ncclGetVersion code). Raises when librccl cannot be loaded."""
    buf = C.create_string_buffer(4096)
    ver = C.c_int32(0)
    check(load().crl_comm_info(buf, len(buf), C.byref(ver)))
    return buf.value.decode("utf-8", "replace"), int(ver.value)


def make_actor_critic_host(obs_dim, n_act, hidden, seed=0):
    """crl_make_actor_critic: the library's host-side restatement of Networks.make_actor_critic (networks.jl:36-49) — the start
    crl_ppo_init_params gives a handle; runs without a GPU."""
    n = 2 * (hidden * obs_dim + hidden + hidden * hidden + hidden) + n_act * hidden + n_act + hidden + 1
    out = np.zeros(n, np.float32)
    check(load().crl_make_actor_critic(obs_dim, n_act, hidden, seed, _ptr(out, C.c_float), n))
    return out


def dqn_make_nn_host(seed=0):
    """crl_dqn_make_nn: make_nn(env) of dqn.jl:22-26 (glorot-uniform weights, zero biases), flat in Flux.params order."""
    out = np.zeros(DQN_PARAM_COUNT, np.float32)
    check(load().crl_dqn_make_nn(seed, _ptr(out, C.c_float), out.size))
    return out


_FIELD_DTYPES = {
    F_OBS: np.float32, F_ACTION: np.int32, F_LOGPROB: np.float32, F_REWARD: np.float32, F_TERMINAL: np.uint8,
    F_VALUE: np.float32, F_ADVANTAGE: np.float32, F_RETURN: np.float32, F_PERM: np.int32, F_PARAMS: np.float32,
    F_GRADS: np.float32, F_ADAM_M: np.float32, F_ADAM_V: np.float32, F_ENV_STATE: np.float32, F_CUR_OBS: np.float32,
    F_NEXT_DONE: np.uint8, F_ENV_T: np.int32, F_BETAP: np.float64, F_ADV_SUMS: np.float64,
}


class Handle:
    """Owns one crl_ppo (one GPU / one data-parallel shard)."""

    def __init__(self, cfg: CrlConfig, device: int = 0):
        self.cfg = cfg
        self._h = C.c_void_p()
        check(load().crl_ppo_create(C.byref(cfg), device, C.byref(self._h)))
        n = C.c_int64()
        check(load().crl_ppo_param_count(self._h, C.byref(n)))
        self.P = n.value
        self.nt, self.k, self.d, self.A = cfg.num_envs, cfg.num_steps, cfg.obs_dim, cfg.n_act
        self.device = device
        self.B = self.nt * self.k

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            load().crl_ppo_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _shape(self, f):
        nt, k, d, B, P = self.nt, self.k, self.d, self.B, self.P
        return {F_OBS: (d, nt, k), F_PERM: (B,), F_PARAMS: (P,), F_GRADS: (P,), F_ADAM_M: (P,), F_ADAM_V: (P,),
                F_ENV_STATE: (d, nt), F_CUR_OBS: (d, nt), F_NEXT_DONE: (nt,), F_ENV_T: (nt,), F_BETAP: (24,),
                F_ADV_SUMS: (2 * self.cfg.num_minibatches,)}.get(f, (nt, k))

    def read(self, f):
        out = np.zeros(self._shape(f), _FIELD_DTYPES[f], order="F")
        check(load().crl_ppo_read(self._h, f, out.ctypes.data_as(C.c_void_p), out.nbytes))
        return out

    def write(self, f, arr):
        a = np.asfortranarray(arr, _FIELD_DTYPES[f])
        if a.shape != self._shape(f):
            a = a.reshape(self._shape(f), order="F")
        a = np.asfortranarray(a)
        check(load().crl_ppo_write(self._h, f, a.ctypes.data_as(C.c_void_p), a.nbytes))

    def sync(self):
        check(load().crl_sync(self._h))

    def init_params(self, seed=0):
        """ppo.jl:87 through the library's own initialiser (crl_ppo_init_params)."""
        check(load().crl_ppo_init_params(self._h, seed))

    def policy_act(self, obs, u, with_value=True):
        obs = np.asfortranarray(obs, np.float32)
        n = obs.shape[1] if obs.ndim == 2 else 1
        u = np.ascontiguousarray(u, np.float64)
        action = np.zeros(n, np.int32); logprob = np.zeros(n, np.float32); value = np.zeros(n, np.float32)
        check(load().crl_policy_act(self._h, _ptr(obs, C.c_float), _ptr(u, C.c_double), n, _ptr(action, C.c_int32),
                                    _ptr(logprob, C.c_float), _ptr(value, C.c_float) if with_value else None))
        return action, logprob, value

    def logprob_actions(self, obs, actions):
        obs = np.asfortranarray(obs, np.float32)
        n = obs.shape[1]
        actions = np.ascontiguousarray(actions, np.int32)
        logprob = np.zeros(n, np.float32); ent = np.zeros((self.A, n), np.float32, order="F")
        check(load().crl_logprob_actions(self._h, _ptr(obs, C.c_float), _ptr(actions, C.c_int32), n, _ptr(logprob, C.c_float),
                                         _ptr(ent, C.c_float)))
        return logprob, ent

    def rollout_store(self, step, obs, action, logprob, reward, terminal, value):
        obs = np.asfortranarray(obs, np.float32); action = np.ascontiguousarray(action, np.int32)
        logprob = np.ascontiguousarray(logprob, np.float32); reward = np.ascontiguousarray(reward, np.float32)
        terminal = np.ascontiguousarray(terminal, np.uint8); value = np.ascontiguousarray(value, np.float32)
        check(load().crl_rollout_store(self._h, step, _ptr(obs, C.c_float), _ptr(action, C.c_int32), _ptr(logprob, C.c_float),
                                       _ptr(reward, C.c_float), _ptr(terminal, C.c_uint8), _ptr(value, C.c_float)))

    def env_reset(self):
        check(load().crl_env_reset(self._h))

    def rollout_run(self):
        check(load().crl_rollout_run(self._h))

    def env_step(self, action, gstep=0):
        """crl_env_step: the on-device envs take the caller's 0-based actions (ppo.jl:130-165 without the policy); gstep keys the reset stream like
        step `gstep` of the training loop. Returns (next_obs (obs_dim, nt), reward, done)."""
        action = np.ascontiguousarray(action, np.int32)
        if action.shape != (self.nt,):
            raise ValueError(f"env_step: {self.nt} actions expected, got shape {action.shape}")
        obs = np.zeros((self.d, self.nt), np.float32, order="F"); reward = np.zeros(self.nt, np.float32); done = np.zeros(self.nt, np.uint8)
        check(load().crl_env_step(self._h, _ptr(action, C.c_int32), int(gstep), _ptr(obs, C.c_float), _ptr(reward, C.c_float), _ptr(done, C.c_uint8)))
        return obs, reward, done

    # ---- device-resident external envs: every pointer is an int device address or an object with data_ptr(); no call below synchronises the host
    @property
    def stream(self):
        """crl_ppo_stream: the handle's hipStream_t as an int (e.g. for torch.cuda.ExternalStream)."""
        s = C.c_void_p()
        check(load().crl_ppo_stream(self._h, C.byref(s)))
        return s.value or 0

    def act_device(self, step, obs, done, action, peer_stream=None):
        """crl_rollout_act_device: ppo.jl:127-128 + the policy's share of Buffer.add! for slot `step`, one launch; the sampled 0-based actions land in `action`."""
        o, d, a = devptr(obs, "act_device: obs"), devptr(done, "act_device: done"), devptr(action, "act_device: action")
        ps = devptr(peer_stream, "peer_stream", optional=True)
        check(load().crl_rollout_act_device(self._h, int(step), o, d, a, ps))

    def record_device(self, step, reward, next_obs, next_done, peer_stream=None):
        """crl_rollout_record_device: ppo.jl:132,137,143-165 — reward into slot `step`, next_obs / next_done, episode bookkeeping."""
        r, o, d = devptr(reward, "record_device: reward"), devptr(next_obs, "record_device: next_obs"), devptr(next_done, "record_device: next_done")
        ps = devptr(peer_stream, "peer_stream", optional=True)
        check(load().crl_rollout_record_device(self._h, int(step), r, o, d, ps))

    def env_step_device(self, action, gstep, next_obs, reward, done, peer_stream=None):
        """crl_env_step_device: crl_env_step on device pointers (next_obs may be None: CRL_F_CUR_OBS holds it); a bad action surfaces at the next sync()."""
        a, r, d = devptr(action, "env_step_device: action"), devptr(reward, "env_step_device: reward"), devptr(done, "env_step_device: done")
        o, ps = devptr(next_obs, "env_step_device: next_obs", optional=True), devptr(peer_stream, "peer_stream", optional=True)
        check(load().crl_env_step_device(self._h, a, int(gstep), o, r, d, ps))

    def update(self, want_stats=True):
        """crl_ppo_update: ppo.jl:168-253 on the resident buffer (the update half of iterate)."""
        n = self.cfg.update_epochs * self.cfg.num_minibatches
        arr = (CrlStats * n)()
        check(load().crl_ppo_update(self._h, arr if want_stats else None))
        return [a.as_dict() for a in arr] if want_stats else None

    def evaluate(self, num_envs, episodes_per_env=1, mode=EVAL_GREEDY, seed=0, trace_steps=0, want_arrays=True):
        """crl_ppo_evaluate: the current actor, frozen, on `num_envs` fresh private envs until each has finished `episodes_per_env` episodes (one
        launch). Returns {"report": {...}, "returns": (episodes_per_env, num_envs) float32, "lengths": … int32[, "trace": (trace_steps, num_envs) int32,
        -1 once an env had finished its quota]}; want_arrays=False passes NULL for the arrays and returns the report only."""
        cfg = CrlEvalConfig(int(num_envs), int(episodes_per_env), int(mode), int(trace_steps), int(seed) & 0xFFFFFFFFFFFFFFFF)
        rep = CrlEvalReport()
        shape = (max(cfg.episodes_per_env, 0), max(cfg.num_envs, 0))
        ret = np.zeros(shape, np.float32) if want_arrays else None
        length = np.zeros(shape, np.int32) if want_arrays else None
        trace = np.zeros((cfg.trace_steps, max(cfg.num_envs, 0)), np.int32) if cfg.trace_steps > 0 else None
        check(load().crl_ppo_evaluate(self._h, C.byref(cfg), C.byref(rep), None if ret is None else _ptr(ret, C.c_float),
                                      None if length is None else _ptr(length, C.c_int32), None if trace is None else _ptr(trace, C.c_int32)))
        out = {"report": rep.as_dict()}
        if want_arrays:
            out["returns"] = ret; out["lengths"] = length
        if trace is not None:
            out["trace"] = trace
        return out

    def diagnose(self, per_sample=False):
        """crl_ppo_diagnose: approx-KL, clip fraction, entropy and explained variance of the resident rollout buffer under the current parameters (one
        read-only launch). Returns the struct's fields as a dict; per_sample=True adds "new_logprob" and "new_value", (num_envs, num_steps) float32."""
        d = CrlDiag()
        lp = np.zeros((self.nt, self.k), np.float32, order="F") if per_sample else None
        v = np.zeros((self.nt, self.k), np.float32, order="F") if per_sample else None
        check(load().crl_ppo_diagnose(self._h, C.byref(d), None if lp is None else _ptr(lp, C.c_float), None if v is None else _ptr(v, C.c_float)))
        out = d.as_dict()
        if per_sample:
            out["new_logprob"] = lp; out["new_value"] = v
        return out

    def episode_stats(self):
        st = CrlEpisodeStats()
        check(load().crl_episode_stats_read(self._h, C.byref(st)))
        return {"episodes": st.episodes, "return_sum": st.return_sum, "length_sum": st.length_sum, "return_max": st.return_max}

    def compute_gae(self):
        check(load().crl_compute_gae(self._h))

    def shuffle(self, epoch_id):
        check(load().crl_shuffle(self._h, epoch_id))

    def adv_stats(self):
        check(load().crl_adv_stats(self._h))

    def update_minibatch(self, mb, eta, apply_update=True, want_stats=True):
        st = CrlStats()
        check(load().crl_ppo_update_minibatch(self._h, mb, eta, int(apply_update), C.byref(st) if want_stats else None))
        return st.as_dict() if want_stats else None

    def iterate(self, n_iters=1, want_stats=True):
        n = self.cfg.update_epochs * self.cfg.num_minibatches
        arr = (CrlStats * n)()
        check(load().crl_ppo_iterate(self._h, n_iters, arr if want_stats else None))
        return [a.as_dict() for a in arr] if want_stats else None

    def _report(self, fn, want_stats):
        n = self.cfg.update_epochs * self.cfg.num_minibatches
        cap = getattr(self, "_ring_cap", 0)
        rep = CrlIterationReport(); arr = (CrlStats * n)(); ring = (CrlEpisodeRecord * max(cap, 1))()
        check(fn(self._h, C.byref(rep), arr if want_stats else None, ring if cap else None, cap))
        if rep.iteration < 0:
            return None
        recs = sorted((ring[i].step, ring[i].env, ring[i].episode_return, ring[i].episode_length) for i in range(rep.n_ring))
        return {"iteration": rep.iteration, "stats": [a.as_dict() for a in arr] if want_stats else None,
                "episodes": {"episodes": rep.episodes.episodes, "return_sum": rep.episodes.return_sum, "length_sum": rep.episodes.length_sum,
                             "return_max": rep.episodes.return_max},
                "records": recs, "n_episodes": rep.n_episodes}

    def iterate_async(self, want_stats=True):
        """crl_ppo_iterate_async: enqueues one iteration and returns the report of the iteration BEFORE it (None on the first call): its loss records,
        episode statistics and per-episode records (sorted by (step, env) like episode_records()) — read without making the GPU wait for the host."""
        return self._report(load().crl_ppo_iterate_async, want_stats)

    def drain(self, want_stats=True):
        """crl_ppo_drain: the report of the last iteration enqueued through iterate_async (None: nothing pending)."""
        return self._report(load().crl_ppo_drain, want_stats)

    @property
    def iteration(self):
        it = C.c_int64()
        check(load().crl_ppo_iteration(self._h, C.byref(it)))
        return it.value

    def episode_ring_enable(self, capacity):
        check(load().crl_episode_ring_enable(self._h, int(capacity)))
        self._ring_cap = int(capacity)

    def episode_records(self):
        """(records sorted by (step, env) — the reference's logging order —, number of episodes that ended)"""
        cap = getattr(self, "_ring_cap", 0)
        buf = (CrlEpisodeRecord * max(cap, 1))(); n = C.c_int32(); tot = C.c_int64()
        check(load().crl_episode_ring_read(self._h, buf, cap, C.byref(n), C.byref(tot)))
        recs = [(buf[i].step, buf[i].env, buf[i].episode_return, buf[i].episode_length) for i in range(n.value)]
        recs.sort()
        return recs, tot.value

    @property
    def exact_reruns(self):
        n = C.c_int64()
        check(load().crl_ppo_exact_reruns(self._h, C.byref(n)))
        return n.value

    def comm_init(self, unique_id: bytes, world_size: int, rank: int):
        buf = (C.c_uint8 * 128).from_buffer_copy(unique_id)
        check(load().crl_comm_init(self._h, buf, world_size, rank))

    def comm_peer_export(self, world_size: int, rank: int) -> bytes:
        """Allocates this rank's mailbox for the one-shot peer all-reduce; returns its 64-byte IPC handle."""
        buf = (C.c_uint8 * 64)()
        check(load().crl_comm_peer_export(self._h, world_size, rank, buf))
        return bytes(buf)

    def comm_peer_attach(self, handles: bytes):
        """handles: world_size x 64 bytes in rank order (every rank's crl_comm_peer_export result)."""
        buf = (C.c_uint8 * len(handles)).from_buffer_copy(handles)
        check(load().crl_comm_peer_attach(self._h, buf))

    def comm_init_external(self, world_size: int, rank: int):
        check(load().crl_comm_init_external(self._h, world_size, rank))

    def adv_stats_local(self):
        check(load().crl_adv_stats_local(self._h))

    def adv_stats_finish(self):
        check(load().crl_adv_stats_finish(self._h))

    def comm_destroy(self):
        check(load().crl_comm_destroy(self._h))

    def set_option(self, key: str, value: int):
        """crl_ppo_set_option: per-handle kernel-flavour / numerics switches (include/cleanrl_hip.h lists them)."""
        check(load().crl_ppo_set_option(self._h, key.encode(), int(value)))

    def get_option(self, key: str) -> int:
        v = C.c_int64()
        check(load().crl_ppo_get_option(self._h, key.encode(), C.byref(v)))
        return v.value

    def options(self) -> dict:
        return {k: self.get_option(k) for k in option_names()}

    def prof_enable(self, on=True):
        check(load().crl_prof_enable(self._h, int(on)))

    def prof_reset(self):
        check(load().crl_prof_reset(self._h))

    def prof_read(self):
        out = {}
        for kid, name in enumerate(KERNEL_NAMES):
            ms = C.c_double(); n = C.c_int64()
            check(load().crl_prof_read(self._h, kid, C.byref(ms), C.byref(n)))
            out[name] = (ms.value, n.value)
        return out


def option_names():
    """Names of every option crl_ppo_set_option accepts, in table order."""
    n = C.c_int32()
    check(load().crl_ppo_option_count(C.byref(n)))
    out = []
    for i in range(n.value):
        name = C.c_char_p(); d = C.c_int64()
        check(load().crl_ppo_option_name(i, C.byref(name), C.byref(d)))
        out.append(name.value.decode())
    return out


def comm_unique_id() -> bytes:
    buf = (C.c_uint8 * 128)()
    check(load().crl_comm_unique_id(buf))
    return bytes(buf)


def gae_host(value, reward, terminal, next_value, next_done, gamma, lam, mode=GAE_COMPAT, device=0, seg=0, tile=0, nt_loads=2):
    """crl_gae / crl_gae_opt on host arrays: value/reward/terminal are (nt,k) Fortran-ordered; seg / tile / nt_loads select the kernel
    flavour like the handle options gae_seg / gae_tile / gae_nt_loads (defaults: the library decides)."""
    value = np.asfortranarray(value, np.float32); reward = np.asfortranarray(reward, np.float32)
    terminal = np.asfortranarray(terminal, np.uint8)
    nt, k = value.shape
    nv = None if next_value is None else np.ascontiguousarray(next_value, np.float32)
    nd = None if next_done is None else np.ascontiguousarray(next_done, np.uint8)
    adv = np.zeros((nt, k), np.float32, order="F"); ret = np.zeros((nt, k), np.float32, order="F")
    args = (device, _ptr(value, C.c_float), _ptr(reward, C.c_float), _ptr(terminal, C.c_uint8),
            _ptr(nv, C.c_float) if nv is not None else None, _ptr(nd, C.c_uint8) if nd is not None else None,
            nt, k, gamma, lam, mode, _ptr(adv, C.c_float), _ptr(ret, C.c_float))
    if (seg, tile, nt_loads) == (0, 0, 2):
        check(load().crl_gae(*args))
    else:
        check(load().crl_gae_opt(*args, seg, tile, nt_loads))
    return adv, ret


def gae_bench(nt, k=128, seg=0, tile=0, nt_loads=0, flush_mb=0, reps=10, device=0):
    """crl_gae_bench: (gae launch times, same-byte-count float4 copy launch times), ms each, `reps` of them."""
    g = np.zeros(reps, np.float64); c = np.zeros(reps, np.float64)
    check(load().crl_gae_bench(device, nt, k, seg, tile, nt_loads, flush_mb, reps, _ptr(g, C.c_double), _ptr(c, C.c_double)))
    return g, c


class A2CHandle:
    """Owns one crl_a2c* (include/cleanrl_hip.h, A2C block): networks, optimiser state, replay buffer and env on one GPU."""

    def __init__(self, cfg: CrlA2CConfig, device=0):
        self._L = load()
        self.cfg = cfg
        self._h = C.c_void_p()
        check(self._L.crl_a2c_create(C.byref(cfg), device, C.byref(self._h)))
        n = C.c_int64()
        check(self._L.crl_a2c_param_count(self._h, C.byref(n)))
        self.param_count = n.value

    def close(self):
        if self._h:
            self._L.crl_a2c_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def write_params(self, p):
        p = np.ascontiguousarray(p, np.float32)
        check(self._L.crl_a2c_write_params(self._h, _ptr(p, C.c_float), p.size))

    def init_params(self, seed=0):
        check(self._L.crl_a2c_init_params(self._h, seed))

    def read_params(self):
        p = np.zeros(self.param_count, np.float32)
        check(self._L.crl_a2c_read_params(self._h, _ptr(p, C.c_float), p.size))
        return p

    def read_grads(self):
        """crl_a2c_read_grads: the last update's Float32 gradients before ClipNorm, in the parameters' layout; an error before the first update."""
        g = np.zeros(self.param_count, np.float32)
        check(self._L.crl_a2c_read_grads(self._h, _ptr(g, C.c_float), g.size))
        return g

    def env(self):
        s = np.zeros(4, np.float64); g = C.c_int64(); n = C.c_int32()
        check(self._L.crl_a2c_read_env(self._h, _ptr(s, C.c_double), C.byref(g), C.byref(n)))
        return s, g.value, n.value

    def buffer(self):
        cap = 2 * self.cfg.min_replay_size
        st = np.zeros((4, cap), np.float64, order="F"); a = np.zeros(cap, np.int32); r = np.zeros(cap, np.float64); t = np.zeros(cap, np.uint8)
        check(self._L.crl_a2c_read_buffer(self._h, _ptr(st, C.c_double), _ptr(a, C.c_int32), _ptr(r, C.c_double), _ptr(t, C.c_uint8), cap))
        n = self.env()[2]
        return st[:, :n], a[:n], r[:n], t[:n]

    def run_until_update(self, max_env_steps=1 << 40, max_eps=4096):
        ts = CrlA2CTrainStats(); eps = (CrlA2CEpisode * max_eps)(); n = C.c_int32(); taken = C.c_int64()
        check(self._L.crl_a2c_run_until_update(self._h, max_env_steps, C.byref(ts), eps, max_eps, C.byref(n), C.byref(taken)))
        episodes = [(eps[i].episode_return, eps[i].episode_length, eps[i].global_step) for i in range(n.value)]
        return taken.value, dict(actor_loss=ts.actor_loss, critic_loss=ts.critic_loss, n=ts.n, trained=bool(ts.trained)), episodes

    def forward(self, net, obs):
        """crl_a2c_forward: net 0 = the actor's logits, (4, n) → (2, n); net 1 = the critic, (4, n) → (n,). Float64."""
        obs = np.asfortranarray(obs, np.float64)
        if obs.ndim == 1:
            obs = obs[:, None]
        n = obs.shape[1]
        out = np.zeros(n, np.float64) if net == 1 else np.zeros((2, n), np.float64, order="F")
        check(self._L.crl_a2c_forward(self._h, int(net), _ptr(obs, C.c_double), n, _ptr(out, C.c_double)))
        return out

    def evaluate(self, num_envs, episodes_per_env=1, mode=EVAL_GREEDY, seed=0, trace_steps=0):
        """crl_a2c_evaluate: the current actor, frozen, greedy or sampled, on `num_envs` fresh private CartPoles x `episodes_per_env` episodes (one
        launch). Returns {"report": {...}, "returns", "disc_returns", "v0": (episodes_per_env, num_envs) float64, "lengths": int32[, "trace_action":
        (trace_steps, num_envs) int32, −1 after the env's quota]}."""
        return _value_evaluate(self._L.crl_a2c_evaluate, self._h, num_envs, episodes_per_env, mode, seed, trace_steps, "v0")


def _value_evaluate(fn, handle, num_envs, episodes_per_env, mode, seed, trace_steps, v0_name):
    """crl_dqn_evaluate / crl_a2c_evaluate → {"report", "returns", "lengths", "disc_returns", v0_name[, "trace_action"]}; the report's v0_mean /
    v_bias_mean carry v0_name's prefix (q0_mean / q_bias_mean for DQN, like DDPG's)."""
    cfg = CrlEvalConfig(int(num_envs), int(episodes_per_env), int(mode), int(trace_steps), int(seed) & 0xFFFFFFFFFFFFFFFF)
    rep = CrlValueEvalReport()
    shape = (max(cfg.episodes_per_env, 0), max(cfg.num_envs, 0))
    ret, disc, v0 = (np.zeros(shape, np.float64) for _ in range(3))
    lengths = np.zeros(shape, np.int32)
    trace = np.zeros((cfg.trace_steps, shape[1]), np.int32) if cfg.trace_steps > 0 else None
    check(fn(handle, C.byref(cfg), C.byref(rep), _ptr(ret, C.c_double), _ptr(lengths, C.c_int32), _ptr(disc, C.c_double), _ptr(v0, C.c_double),
             None if trace is None else _ptr(trace, C.c_int32)))
    report = rep.as_dict()
    if v0_name != "v0":
        report = {k.replace("v0_", "q0_").replace("v_bias", "q_bias"): v for k, v in report.items()}
    out = {"report": report, "returns": ret, "lengths": lengths, "disc_returns": disc, v0_name: v0}
    if trace is not None:
        out["trace_action"] = trace
    return out


def dqn_eval_envs_per_block():
    return load().crl_dqn_eval_envs_per_block()


def a2c_eval_envs_per_block():
    return load().crl_a2c_eval_envs_per_block()


def a2c_discounted_future_rewards_host(rewards, terminals, final_value, gamma, device=0):
    r = np.ascontiguousarray(rewards, np.float64); t = np.ascontiguousarray(terminals, np.uint8)
    out = np.zeros(r.size, np.float64)
    check(load().crl_a2c_discounted_future_rewards(device, _ptr(r, C.c_double), _ptr(t, C.c_uint8), r.size, float(final_value),
                                                   float(gamma), _ptr(out, C.c_double)))
    return out


def dqn_c51_make_nn_host(seed=0, n_atoms=51):
    """crl_dqn_c51_make_nn: crl_dqn_make_nn's rule on the C51 shapes (the same trunk for the same seed)."""
    out = np.zeros(dqn_c51_param_count(n_atoms), np.float32)
    check(load().crl_dqn_c51_make_nn(seed, int(n_atoms), _ptr(out, C.c_float), out.size))
    return out


def dqn_dueling_param_count(n_atoms=None):
    """20928 + 255·R floats: R = 1 on a scalar dueling handle (n_atoms None or 0), R = n_atoms on a categorical one"""
    return 20928 + 255 * (int(n_atoms) if n_atoms else 1)


def dqn_dueling_make_nn_host(seed=0, n_atoms=None):
    """crl_dqn_dueling_make_nn: crl_dqn_make_nn's rule on the ten arrays of a dueling net (the same W1 and W2v draws for the same seed)."""
    out = np.zeros(dqn_dueling_param_count(n_atoms), np.float32)
    check(load().crl_dqn_dueling_make_nn(seed, int(n_atoms) if n_atoms else 0, _ptr(out, C.c_float), out.size))
    return out


def dqn_noisy_make_nn_host(seed=0, sigma0=0.5, dueling=False, n_atoms=None):
    """crl_dqn_noisy_make_nn: Fortunato's factorised init, mu (P) then sigma (P) of the twin with these options."""
    P = dqn_dueling_param_count(n_atoms) if dueling else (dqn_c51_param_count(n_atoms) if n_atoms else DQN_PARAM_COUNT)
    out = np.zeros(2 * P, np.float32)
    check(load().crl_dqn_noisy_make_nn(seed, float(sigma0), int(bool(dueling)), int(n_atoms) if n_atoms else 0, _ptr(out, C.c_float), out.size))
    return out


class DQNHandle:
    """Owns one crl_dqn* (include/cleanrl_hip.h, DQN block). `per` (a CrlDQNPEROptions) makes it a prioritized-replay handle (crl_dqn_per_create):
    every method below works on it unchanged, and per_status / per_read / per_probe, which are errors on a uniform handle, become available.
    `target` (a CrlDQNTargetOptions) makes it a crl_dqn_create_with handle, with either replay: n-step / double-Q targets, and target_read /
    nstep_probe, which are errors on the other handles. `c51` (a CrlDQNC51Options) makes it a crl_dqn_c51_create handle, with either replay and any
    target options: the head is categorical, param_count is its own, q_values are expected values, and c51_probs / c51_read / c51_project_probe
    become available. `dueling=True` makes it a crl_dqn_dueling_create handle, with either head, either replay and any target options: layers 2 and 3
    are a value and an advantage stream (ten arrays, param_count is its own), and dueling_streams becomes available. `noisy` (a CrlDQNNoisyOptions)
    makes it a crl_dqn_noisy_create handle on top of any of the above: its parameters are mu then sigma (param_count is twice the twin's), q_values /
    evaluate / c51_probs / dueling_streams run with the noise off, and noisy_weights / noisy_noise become available."""

    def __init__(self, cfg: CrlDQNConfig, device=0, per=None, target=None, c51=None, dueling=False, noisy=None):
        self._L = load()
        self.cfg = cfg
        self.per = per
        self.target = target
        self.c51 = c51
        self.dueling = bool(dueling)
        self.noisy = noisy
        self._h = C.c_void_p()
        if noisy is not None:
            check(self._L.crl_dqn_noisy_create(C.byref(cfg), C.byref(noisy), int(self.dueling), None if c51 is None else C.byref(c51),
                                               None if per is None else C.byref(per), None if target is None else C.byref(target), device,
                                               C.byref(self._h)))
        elif self.dueling:
            check(self._L.crl_dqn_dueling_create(C.byref(cfg), None if c51 is None else C.byref(c51), None if per is None else C.byref(per),
                                                 None if target is None else C.byref(target), device, C.byref(self._h)))
        elif c51 is not None:
            check(self._L.crl_dqn_c51_create(C.byref(cfg), C.byref(c51), None if per is None else C.byref(per),
                                             None if target is None else C.byref(target), device, C.byref(self._h)))
        elif target is not None:
            check(self._L.crl_dqn_create_with(C.byref(cfg), None if per is None else C.byref(per), C.byref(target), device, C.byref(self._h)))
        elif per is None:
            check(self._L.crl_dqn_create(C.byref(cfg), device, C.byref(self._h)))
        else:
            check(self._L.crl_dqn_per_create(C.byref(cfg), C.byref(per), device, C.byref(self._h)))

    def close(self):
        if self._h:
            self._L.crl_dqn_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def write_params(self, p):
        p = np.ascontiguousarray(p, np.float32)
        check(self._L.crl_dqn_write_params(self._h, _ptr(p, C.c_float), p.size))

    def init_params(self, seed=0):
        check(self._L.crl_dqn_init_params(self._h, seed))

    def param_count(self):
        """crl_dqn_param_count: 10934, 10764 + 85·2N on a C51 handle, 20928 + 255·R on a dueling one"""
        n = C.c_size_t()
        check(self._L.crl_dqn_param_count(self._h, C.byref(n)))
        return int(n.value)

    def read_params(self):
        n = DQN_PARAM_COUNT if self.c51 is None and not self.dueling and self.noisy is None else self.param_count()
        q = np.zeros(n, np.float32); t = np.zeros(n, np.float32)
        check(self._L.crl_dqn_read_params(self._h, _ptr(q, C.c_float), _ptr(t, C.c_float), q.size))
        return q, t

    def status(self):
        st = CrlDQNStatus()
        check(self._L.crl_dqn_status_read(self._h, C.byref(st)))
        return dict(state=np.array(list(st.env_state)), global_step=st.global_step, rb_size=st.rb_size, n_updates=st.n_updates,
                    last_loss=st.last_loss)

    def run(self, max_env_steps, max_eps=8192, max_losses=4096):
        eps = (CrlDQNEpisode * max_eps)(); ls = (CrlDQNLossRecord * max_losses)(); ne = C.c_int32(); nl = C.c_int32(); taken = C.c_int64()
        check(self._L.crl_dqn_run(self._h, max_env_steps, eps, max_eps, C.byref(ne), ls, max_losses, C.byref(nl), C.byref(taken)))
        return (taken.value, [(eps[i].episode_return, eps[i].episode_length, eps[i].global_step, eps[i].epsilon) for i in range(ne.value)],
                [(ls[i].global_step, ls[i].loss) for i in range(nl.value)])

    def q_values(self, obs):
        obs = np.asfortranarray(obs, np.float64)
        if obs.ndim == 1:
            obs = obs[:, None]
        n = obs.shape[1]
        q = np.zeros((2, n), np.float64, order="F")
        check(self._L.crl_dqn_q_values(self._h, _ptr(obs, C.c_double), n, _ptr(q, C.c_double)))
        return q

    def evaluate(self, num_envs, episodes_per_env=1, seed=0, trace_steps=0):
        """crl_dqn_evaluate: the current q_net, frozen and greedy (no ε), on `num_envs` fresh private CartPoles x `episodes_per_env` episodes (one
        launch). Returns {"report": {..., q0_mean, q_bias_mean}, "returns", "disc_returns", "q0": (episodes_per_env, num_envs) float64, "lengths":
        int32[, "trace_action": (trace_steps, num_envs) int32, −1 after the env's quota]}."""
        return _value_evaluate(self._L.crl_dqn_evaluate, self._h, num_envs, episodes_per_env, EVAL_GREEDY, seed, trace_steps, "q0")

    def per_status(self):
        """crl_dqn_per_status_read → {beta, total, max_leaf, tree_leaves}"""
        st = CrlDQNPERStatus()
        check(self._L.crl_dqn_per_status_read(self._h, C.byref(st)))
        return dict(beta=st.beta, total=st.total, max_leaf=np.float32(st.max_leaf), tree_leaves=st.tree_leaves)

    def per_read(self):
        """crl_dqn_per_read → {leaves float32 [buffer_size], tree float64 [2·C], idx int32 [k], weight, abs_td float64 [k]} after the last update"""
        cap, k = int(self.cfg.buffer_size), int(self.cfg.batch_size)
        c = 1
        while c < cap:
            c *= 2
        out = dict(leaves=np.zeros(cap, np.float32), tree=np.zeros(2 * c, np.float64), idx=np.zeros(k, np.int32), weight=np.zeros(k, np.float64),
                   abs_td=np.zeros(k, np.float64))
        check(self._L.crl_dqn_per_read(self._h, _ptr(out["leaves"], C.c_float), _ptr(out["tree"], C.c_double), _ptr(out["idx"], C.c_int32),
                                       _ptr(out["weight"], C.c_double), _ptr(out["abs_td"], C.c_double)))
        return out

    def per_probe(self, leaves, gstep, k, beta, want_tree=True):
        """crl_dqn_per_probe: the device's sampler on `leaves` (float32, n of them) → (idx int32 [k], weight float64 [k], tree float64 [2·C(n)] or None)"""
        leaves = np.ascontiguousarray(leaves, np.float32)
        n = leaves.size
        c = 1
        while c < n:
            c *= 2
        idx, w = np.zeros(max(int(k), 1), np.int32), np.zeros(max(int(k), 1), np.float64)
        tree = np.zeros(2 * c, np.float64) if want_tree else None
        check(self._L.crl_dqn_per_probe(self._h, _ptr(leaves, C.c_float), n, int(gstep), int(k), float(beta), _ptr(idx, C.c_int32), _ptr(w, C.c_double),
                                        None if tree is None else _ptr(tree, C.c_double)))
        return idx, w, tree

    def target_read(self):
        """crl_dqn_target_read → {last, m, astar int32 [k], nret, ndisc, td float64 [k]} of the last completed update"""
        k = int(self.cfg.batch_size)
        out = dict(last=np.zeros(k, np.int32), m=np.zeros(k, np.int32), nret=np.zeros(k, np.float64), ndisc=np.zeros(k, np.float64),
                   astar=np.zeros(k, np.int32), td=np.zeros(k, np.float64))
        check(self._L.crl_dqn_target_read(self._h, _ptr(out["last"], C.c_int32), _ptr(out["m"], C.c_int32), _ptr(out["nret"], C.c_double),
                                          _ptr(out["ndisc"], C.c_double), _ptr(out["astar"], C.c_int32), _ptr(out["td"], C.c_double)))
        return out

    def noisy_weights(self, net=0):
        """crl_dqn_noisy_weights: the effective image mu + sigma·eps in use, net 0 = q_net, 1 = target_net → float32 [P]"""
        out = np.zeros(self.param_count() // 2 if self.noisy is not None else self.param_count(), np.float32)
        check(self._L.crl_dqn_noisy_weights(self._h, int(net), _ptr(out, C.c_float), out.size))
        return out

    def noisy_noise(self, gen, net=0):
        """crl_dqn_noisy_noise: the xi table of generation `gen` of either net (stateless) → float32 [412 + rows3, or 700 + 3R]"""
        n = C.c_size_t()
        check(self._L.crl_dqn_noisy_noise_count(self._h, C.byref(n)))
        out = np.zeros(int(n.value), np.float32)
        check(self._L.crl_dqn_noisy_noise(self._h, int(gen), int(net), _ptr(out, C.c_float), out.size))
        return out

    def dueling_streams(self, obs):
        """crl_dqn_dueling_streams: the two streams before they are combined, (4, n) → {value (R, n), adv (R, 2, n)} float64"""
        obs = np.asfortranarray(obs, np.float64)
        if obs.ndim == 1:
            obs = obs[:, None]
        n = obs.shape[1]
        R = 1 if self.c51 is None else int(self.c51.n_atoms)
        value = np.zeros((R, n), np.float64, order="F"); adv = np.zeros((R, 2, n), np.float64, order="F")
        check(self._L.crl_dqn_dueling_streams(self._h, _ptr(obs, C.c_double), n, _ptr(value, C.c_double), _ptr(adv, C.c_double)))
        return dict(value=value, adv=adv)

    def c51_probs(self, obs):
        """crl_dqn_c51_probs: softmax of q_net(obs) per action, (4, n) → (N, 2, n) float64"""
        obs = np.asfortranarray(obs, np.float64)
        if obs.ndim == 1:
            obs = obs[:, None]
        n = obs.shape[1]
        N = 0 if self.c51 is None else int(self.c51.n_atoms)
        probs = np.zeros((max(N, 1), 2, n), np.float64, order="F")
        check(self._L.crl_dqn_c51_probs(self._h, _ptr(obs, C.c_double), n, _ptr(probs, C.c_double)))
        return probs

    def c51_read(self):
        """crl_dqn_c51_read → {proj float64 (N, k) the projected targets, sample_loss float64 [k]} of the last completed update"""
        k = int(self.cfg.batch_size)
        N = 1 if self.c51 is None else int(self.c51.n_atoms)
        out = dict(proj=np.zeros((N, k), np.float64, order="F"), sample_loss=np.zeros(k, np.float64))
        check(self._L.crl_dqn_c51_read(self._h, _ptr(out["proj"], C.c_double), _ptr(out["sample_loss"], C.c_double)))
        return out

    def c51_project_probe(self, probs, nret, ndisc, terminal):
        """crl_dqn_c51_project_probe: the device's projection of the rows probs (N, k) → proj (N, k)"""
        probs = np.asfortranarray(probs, np.float64)
        nret = np.ascontiguousarray(nret, np.float64); ndisc = np.ascontiguousarray(ndisc, np.float64)
        terminal = np.ascontiguousarray(terminal, np.uint8)
        k = nret.size
        if self.c51 is not None and (probs.shape != (int(self.c51.n_atoms), k) or ndisc.size != k or terminal.size != k):
            raise ValueError("c51_project_probe: probs must be (n_atoms, k) and nret, ndisc, terminal of length k")
        proj = np.zeros(probs.shape, np.float64, order="F")
        check(self._L.crl_dqn_c51_project_probe(self._h, _ptr(probs, C.c_double), _ptr(nret, C.c_double), _ptr(ndisc, C.c_double),
                                                _ptr(terminal, C.c_uint8), k, _ptr(proj, C.c_double)))
        return proj

    def nstep_probe(self, reward, terminal, ptr, idx, n_step, gamma):
        """crl_dqn_nstep_probe: the device's n-step walk on a ring of len(reward) slots → {last, m int32 [k], nret, ndisc float64 [k]}"""
        reward = np.ascontiguousarray(reward, np.float64); terminal = np.ascontiguousarray(terminal, np.uint8)
        idx = np.ascontiguousarray(idx, np.int32)
        if terminal.size != reward.size:
            raise ValueError("nstep_probe: reward and terminal must have the same length")
        k = idx.size
        out = dict(last=np.zeros(max(k, 1), np.int32), m=np.zeros(max(k, 1), np.int32), nret=np.zeros(max(k, 1), np.float64),
                   ndisc=np.zeros(max(k, 1), np.float64))
        check(self._L.crl_dqn_nstep_probe(self._h, _ptr(reward, C.c_double), _ptr(terminal, C.c_uint8), reward.size, int(ptr), _ptr(idx, C.c_int32), k,
                                          int(n_step), float(gamma), _ptr(out["last"], C.c_int32), _ptr(out["m"], C.c_int32),
                                          _ptr(out["nret"], C.c_double), _ptr(out["ndisc"], C.c_double)))
        return out


def ddpg_param_count(obs_dim, act_dim):
    """crl_ddpg_param_count: (len of Flux.params(actor), len of Flux.params(critic)) flattened."""
    na, nc = C.c_int64(), C.c_int64()
    check(load().crl_ddpg_param_count(int(obs_dim), int(act_dim), C.byref(na), C.byref(nc)))
    return na.value, nc.value


def ddpg_make_nn_host(obs_dim, act_dim, seed=0):
    """crl_ddpg_make_nn: make_ddpg_nn of ddpg.jl:19-37 (glorot-uniform weights, zero biases) as two flat vectors in Flux.params order."""
    na, nc = ddpg_param_count(obs_dim, act_dim)
    a = np.zeros(na, np.float32); c = np.zeros(nc, np.float32)
    check(load().crl_ddpg_make_nn(int(obs_dim), int(act_dim), seed, _ptr(a, C.c_float), a.size, _ptr(c, C.c_float), c.size))
    return a, c


class DDPGHandle:
    """Owns one crl_ddpg* (include/cleanrl_hip.h, DDPG block)."""

    def __init__(self, cfg: CrlDDPGConfig, device=0):
        self._L = load()
        self.cfg = cfg
        self._h = C.c_void_p()
        self._create(device)
        self.obs_dim, self.act_dim = cfg.obs_dim, cfg.act_dim
        self.actor_n, self.critic_n = ddpg_param_count(cfg.obs_dim, cfg.act_dim)

    def _create(self, device):
        check(self._L.crl_ddpg_create(C.byref(self.cfg), device, C.byref(self._h)))

    def close(self):
        if self._h:
            self._L.crl_ddpg_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def write_params(self, actor, critic):
        a = np.ascontiguousarray(actor, np.float32); c = np.ascontiguousarray(critic, np.float32)
        check(self._L.crl_ddpg_write_params(self._h, _ptr(a, C.c_float), a.size, _ptr(c, C.c_float), c.size))

    def init_params(self, seed=0):
        check(self._L.crl_ddpg_init_params(self._h, seed))

    def read_params(self):
        """(actor, critic, target_actor, target_critic)"""
        out = [np.zeros(n, np.float32) for n in (self.actor_n, self.critic_n, self.actor_n, self.critic_n)]
        check(self._L.crl_ddpg_read_params(self._h, *[_ptr(o, C.c_float) for o in out]))
        return tuple(out)

    def status(self):
        st = CrlDDPGStatus()
        check(self._L.crl_ddpg_status_read(self._h, C.byref(st)))
        return st.as_dict()

    def run(self, max_env_steps, max_eps=8192, max_losses=4096):
        """crl_ddpg_run: (steps taken, [(episode_return, episode_length, global_step)], [(global_step, actor_loss, critic_loss)])"""
        eps = (CrlDDPGEpisode * max_eps)(); ls = (CrlDDPGLossRecord * max_losses)(); ne = C.c_int32(); nl = C.c_int32(); taken = C.c_int64()
        check(self._L.crl_ddpg_run(self._h, max_env_steps, eps, max_eps, C.byref(ne), ls, max_losses, C.byref(nl), C.byref(taken)))
        return (taken.value, [(eps[i].episode_return, eps[i].episode_length, eps[i].global_step) for i in range(ne.value)],
                [(ls[i].global_step, ls[i].actor_loss, ls[i].critic_loss) for i in range(nl.value)])

    def act(self, obs):
        o = np.ascontiguousarray(obs, np.float64)
        if o.shape != (self.obs_dim,):
            raise ValueError(f"act: {self.obs_dim} observation components expected, got shape {o.shape}")
        a = np.zeros(self.act_dim, np.float64)
        check(self._L.crl_ddpg_act(self._h, _ptr(o, C.c_double), _ptr(a, C.c_double)))
        return a

    def observe(self, obs, action, reward, next_obs, terminal):
        o = np.ascontiguousarray(obs, np.float64); a = np.ascontiguousarray(action, np.float64); n = np.ascontiguousarray(next_obs, np.float64)
        if o.shape != (self.obs_dim,) or n.shape != (self.obs_dim,) or a.shape != (self.act_dim,):
            raise ValueError("observe: obs / next_obs of obs_dim and action of act_dim components expected")
        check(self._L.crl_ddpg_observe(self._h, _ptr(o, C.c_double), _ptr(a, C.c_double), float(reward), _ptr(n, C.c_double), int(bool(terminal))))

    def read_losses(self, max_losses=4096):
        ls = (CrlDDPGLossRecord * max_losses)(); nl = C.c_int32()
        check(self._L.crl_ddpg_read_losses(self._h, ls, max_losses, C.byref(nl)))
        return [(ls[i].global_step, ls[i].actor_loss, ls[i].critic_loss) for i in range(nl.value)]

    def buffer(self):
        """The whole ring: dict(state (obs_dim, cap), action (act_dim, cap), reward, next_state, terminal, ptr, size)."""
        cap = self.cfg.buffer_size
        st = np.zeros((self.obs_dim, cap), np.float64, order="F"); nx = np.zeros((self.obs_dim, cap), np.float64, order="F")
        ac = np.zeros((self.act_dim, cap), np.float64, order="F"); r = np.zeros(cap, np.float64); t = np.zeros(cap, np.uint8)
        ptr, size = C.c_int64(), C.c_int64()
        check(self._L.crl_ddpg_read_buffer(self._h, _ptr(st, C.c_double), _ptr(ac, C.c_double), _ptr(r, C.c_double), _ptr(nx, C.c_double),
                                           _ptr(t, C.c_uint8), cap, C.byref(ptr), C.byref(size)))
        return dict(state=st, action=ac, reward=r, next_state=nx, terminal=t, ptr=ptr.value, size=size.value)

    def actor(self, obs):
        """crl_ddpg_actor: the noise-free 2·tanh_fast(·) output, (obs_dim, n) → (act_dim, n)."""
        obs = np.asfortranarray(obs, np.float64)
        if obs.ndim == 1:
            obs = obs[:, None]
        n = obs.shape[1]
        out = np.zeros((self.act_dim, n), np.float64, order="F")
        check(self._L.crl_ddpg_actor(self._h, _ptr(obs, C.c_double), n, _ptr(out, C.c_double)))
        return out

    def q_values(self, obs, act):
        """crl_ddpg_q_values: get_q(critic, obs, act) (ddpg.jl:45), (obs_dim, n), (act_dim, n) → (n,)."""
        obs = np.asfortranarray(obs, np.float64); act = np.asfortranarray(act, np.float64)
        if obs.ndim == 1:
            obs = obs[:, None]
        if act.ndim == 1:
            act = act.reshape(self.act_dim, -1, order="F")
        n = obs.shape[1]
        out = np.zeros(n, np.float64)
        check(self._L.crl_ddpg_q_values(self._h, _ptr(obs, C.c_double), _ptr(act, C.c_double), n, _ptr(out, C.c_double)))
        return out

    def evaluate(self, num_envs, episodes_per_env=1, seed=0, trace_steps=0):
        """crl_ddpg_evaluate: the current actor, frozen and without noise, on `num_envs` fresh private Pendulums x `episodes_per_env` episodes (one
        launch). Returns {"report": {...}, "returns", "disc_returns", "q0": (episodes_per_env, num_envs) float64[, "trace_action": (trace_steps,
        num_envs) float64]}."""
        cfg = CrlDDPGEvalConfig(int(num_envs), int(episodes_per_env), int(trace_steps), 0, int(seed) & 0xFFFFFFFFFFFFFFFF)
        rep = CrlDDPGEvalReport()
        shape = (max(cfg.episodes_per_env, 0), max(cfg.num_envs, 0))
        ret, disc, q0 = (np.zeros(shape, np.float64) for _ in range(3))
        trace = np.zeros((cfg.trace_steps, shape[1]), np.float64) if cfg.trace_steps > 0 else None
        check(self._L.crl_ddpg_evaluate(self._h, C.byref(cfg), C.byref(rep), _ptr(ret, C.c_double), _ptr(disc, C.c_double), _ptr(q0, C.c_double),
                                        None if trace is None else _ptr(trace, C.c_double)))
        out = {"report": rep.as_dict(), "returns": ret, "disc_returns": disc, "q0": q0}
        if trace is not None:
            out["trace_action"] = trace
        return out


def _twin_q_values(call, handle, obs, act):
    """crl_td3_q_values / crl_sac_q_values on `handle`: (Q_1, Q_2), each (n,), for (obs_dim, n), (act_dim, n)."""
    obs = np.asfortranarray(obs, np.float64); act = np.asfortranarray(act, np.float64)
    if obs.ndim == 1:
        obs = obs[:, None]
    if act.ndim == 1:
        act = act.reshape(handle.act_dim, -1, order="F")
    n = obs.shape[1]
    q1, q2 = np.zeros(n, np.float64), np.zeros(n, np.float64)
    check(call(handle._h, _ptr(obs, C.c_double), _ptr(act, C.c_double), n, _ptr(q1, C.c_double), _ptr(q2, C.c_double)))
    return q1, q2


class TD3Handle(DDPGHandle):
    """Owns one crl_ddpg* made by crl_td3_create (include/cleanrl_hip.h, TD3 block): run / act / observe / status / read_losses / buffer / actor /
    q_values (critic 1) / evaluate are DDPGHandle's; the parameter calls are the crl_td3_* twins, with two critics."""

    def __init__(self, cfg: CrlDDPGConfig, options: CrlTD3Options, device=0):
        self.options = options
        super().__init__(cfg, device)

    def _create(self, device):
        check(self._L.crl_td3_create(C.byref(self.cfg), None if self.options is None else C.byref(self.options), device, C.byref(self._h)))

    def write_params(self, actor, critic1, critic2):
        a, c1, c2 = (np.ascontiguousarray(x, np.float32) for x in (actor, critic1, critic2))
        check(self._L.crl_td3_write_params(self._h, _ptr(a, C.c_float), a.size, _ptr(c1, C.c_float), c1.size, _ptr(c2, C.c_float), c2.size))

    def init_params(self, seed=0):
        check(self._L.crl_td3_init_params(self._h, seed))

    def read_params(self):
        """(actor, critic1, critic2, target_actor, target_critic1, target_critic2)"""
        out = [np.zeros(n, np.float32) for n in (self.actor_n, self.critic_n, self.critic_n) * 2]
        check(self._L.crl_td3_read_params(self._h, *[_ptr(o, C.c_float) for o in out]))
        return tuple(out)

    def q_values_both(self, obs, act):
        """crl_td3_q_values: (Q_1, Q_2), each (n,), for (obs_dim, n), (act_dim, n)."""
        return _twin_q_values(self._L.crl_td3_q_values, self, obs, act)


def sac_param_count(obs_dim, act_dim):
    """crl_sac_param_count: (len of the actor with its head of 2·act_dim rows, len of one critic)."""
    na, nc = C.c_int64(), C.c_int64()
    check(load().crl_sac_param_count(int(obs_dim), int(act_dim), C.byref(na), C.byref(nc)))
    return na.value, nc.value


def sac_make_nn_host(obs_dim, act_dim, seed=0):
    """crl_sac_make_nn: (actor, critic1, critic2) — glorot-uniform weights, zero biases; the critics are crl_td3_init_params' for the same seed."""
    na, nc = sac_param_count(obs_dim, act_dim)
    a, c1, c2 = np.zeros(na, np.float32), np.zeros(nc, np.float32), np.zeros(nc, np.float32)
    check(load().crl_sac_make_nn(int(obs_dim), int(act_dim), seed, _ptr(a, C.c_float), a.size, _ptr(c1, C.c_float), c1.size, _ptr(c2, C.c_float), c2.size))
    return a, c1, c2


class SACHandle(DDPGHandle):
    """Owns one crl_ddpg* made by crl_sac_create (include/cleanrl_hip.h, SAC block): run / act / observe / status / read_losses / buffer / actor (the
    deterministic action) / q_values (critic 1) / evaluate are DDPGHandle's; the parameter calls are the crl_sac_* twins."""

    def __init__(self, cfg: CrlDDPGConfig, options: CrlSACOptions, device=0):
        self.options = options
        super().__init__(cfg, device)
        self.actor_n, self.critic_n = sac_param_count(cfg.obs_dim, cfg.act_dim)

    def _create(self, device):
        check(self._L.crl_sac_create(C.byref(self.cfg), None if self.options is None else C.byref(self.options), device, C.byref(self._h)))

    def write_params(self, actor, critic1, critic2):
        a, c1, c2 = (np.ascontiguousarray(x, np.float32) for x in (actor, critic1, critic2))
        check(self._L.crl_sac_write_params(self._h, _ptr(a, C.c_float), a.size, _ptr(c1, C.c_float), c1.size, _ptr(c2, C.c_float), c2.size))

    def init_params(self, seed=0):
        check(self._L.crl_sac_init_params(self._h, seed))

    def read_params(self):
        """(actor, critic1, critic2, target_critic1, target_critic2, log_alpha: float32 scalar)"""
        out = [np.zeros(n, np.float32) for n in (self.actor_n, self.critic_n, self.critic_n, self.critic_n, self.critic_n, 1)]
        check(self._L.crl_sac_read_params(self._h, *[_ptr(o, C.c_float) for o in out]))
        return tuple(out[:5]) + (out[5][0],)

    def q_values_both(self, obs, act):
        """crl_sac_q_values: (Q_1, Q_2), each (n,), for (obs_dim, n), (act_dim, n)."""
        return _twin_q_values(self._L.crl_sac_q_values, self, obs, act)

    def sac_status(self):
        st = CrlSACStatus()
        check(self._L.crl_sac_status_read(self._h, C.byref(st)))
        return dict(alpha=st.alpha, alpha_loss=st.alpha_loss, entropy=st.entropy, log_alpha=np.float32(st.log_alpha))

    def alpha_records(self, max_records=4096):
        """crl_sac_alpha_records: [(global_step, alpha, alpha_loss, entropy)], one per loss record the last run() / read_losses() returned."""
        rs = (CrlSACAlphaRecord * max_records)(); n = C.c_int32()
        check(self._L.crl_sac_alpha_records(self._h, rs, max_records, C.byref(n)))
        return [(rs[i].global_step, rs[i].alpha, rs[i].alpha_loss, rs[i].entropy) for i in range(n.value)]
