"""cleanrl.jl_amd — MI355X-native PPO rollout + GAE + update hot path behind the API of sash-a/CleanRL.jl's
src/algorithms/ppo.jl. Import as `cleanrl_jl_amd` (root shim) — the directory name is not a Python identifier.

Layout: csrc/ (HIP kernels + the C ABI of include/cleanrl_hip.h) and the host-side mirror of the reference interface.
"""
from . import _lib, config_parser
from ._lib import CrlError, Handle, comm_unique_id, device_count
from .logger import make_logger
from .networks import make_actor_critic
from .a2c import A2CAgent, A2CConfig, a2c, a2c_evaluate, discounted_future_rewards
from .dqn import C51Options, DQNAgent, DQNConfig, DQNTargetOptions, PEROptions, dqn, dqn_evaluate, linear_schedule, make_nn, make_nn_c51, make_nn_dueling, NoisyOptions, make_nn_noisy, noisy_sigma
from .ddpg import DDPGAgent, DDPGConfig, ddpg, ddpg_evaluate, get_q, make_ddpg_nn, polyak_update
from .td3 import TD3Agent, TD3Config, make_td3_nn, td3
from .sac import SACAgent, SACConfig, make_sac_nn, sac
from .ppo import Agent, LibraryEnv, Policy, PPOConfig, diagnose, evaluate, gae, get_action, logprob_actions, ppo, train, train_external

__all__ = ["_lib", "config_parser", "CrlError", "Handle", "comm_unique_id", "device_count", "make_logger", "make_actor_critic", "Agent",
           "Policy", "PPOConfig", "gae", "get_action", "logprob_actions", "ppo", "train", "train_external", "LibraryEnv", "evaluate", "diagnose", "A2CAgent", "A2CConfig", "a2c",
           "discounted_future_rewards", "DQNAgent", "DQNConfig", "PEROptions", "DQNTargetOptions", "C51Options", "make_nn_c51", "make_nn_dueling", "NoisyOptions", "make_nn_noisy", "noisy_sigma", "dqn", "linear_schedule", "make_nn",
           "DDPGAgent", "DDPGConfig", "ddpg", "ddpg_evaluate", "get_q", "make_ddpg_nn", "polyak_update", "dqn_evaluate", "a2c_evaluate",
           "TD3Agent", "TD3Config", "td3", "make_td3_nn",
           "SACAgent", "SACConfig", "sac", "make_sac_nn"]
