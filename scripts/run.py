#!/usr/bin/env python3
"""Runner in the style the reference README plans (`experiments/run_ppo`): every field of the algorithm's config struct is a
command line option (ConfigParser.argparse_struct), records go to the "CleanRL" logger sinks (Logger.make_logger).

    python scripts/run.py ppo --num_envs 4096 --num_steps 128 --total_timesteps 10485760
    python scripts/run.py ppo --env acrobot --hidden 256 --num_envs 256 --num_steps 128      (--env cartpole | mountaincar | acrobot: ppo.jl:82)
    python scripts/run.py ppo --env acrobot --eval_every 10 --eval_envs 256 --eval_episodes 1   ("Evaluation Statistics": a greedy held-out score every 10 updates)
    python scripts/run.py ppo --env acrobot --diag_every 10   ("Policy Diagnostics": approx-KL, clip fraction, entropy, explained variance every 10 updates)
    python scripts/run.py a2c --total_timesteps 100000
    python scripts/run.py dqn --total_timesteps 50000
    python scripts/run.py dqn --total_timesteps 50000 --eval_every 5000 --eval_envs 256 --eval_episodes 1   ("Evaluation Statistics": the greedy policy's held-out score and q_net's bias every 5000 steps)
    python scripts/run.py dqn --total_timesteps 50000 --per --per_alpha 0.6 --per_beta_start 0.4 --per_beta_end 1.0 --per_beta_duration 50000 --per_eps 1e-6   (prioritized replay; --per alone takes the defaults, beta_duration = total_timesteps)
    python scripts/run.py dqn --total_timesteps 50000 --double_q --n_step 3 [--per]   (double Q-learning and 3-step returns; either alone, both combine with --per)
    python scripts/run.py dqn --total_timesteps 50000 --c51 [--n_atoms 51 --v_min 0 --v_max 100] [--per] [--double_q --n_step 3]   (categorical C51 critic; combines with all of the above)
    python scripts/run.py dqn --total_timesteps 50000 --noisy [--sigma0 0.5] [--dueling --c51 --per --double_q --n_step 3]   (noisy linear layers; epsilon_start / epsilon_end default to 0 with --noisy; with all the others: Rainbow)
    python scripts/run.py a2c --total_timesteps 100000 --eval_every 10000   (the same for the actor's argmax and the critic's bias)
    python scripts/run.py ddpg --total_timesteps 20000 --warmup_steps 1000      (the library's Pendulum)
    python scripts/run.py ddpg --total_timesteps 20000 --eval_every 2000 --eval_envs 256 --eval_episodes 1   ("Evaluation Statistics": the noise-free actor's held-out score and the critic's bias every 2000 steps)
    python scripts/run.py td3 --total_timesteps 20000 --warmup_steps 1000 --policy_delay 2 --policy_noise 0.2 --noise_clip 0.5   (TD3 on the same Pendulum; --eval_* as for ddpg)
    python scripts/run.py sac --total_timesteps 20000 --warmup_steps 1000 --alpha 1.0 --autotune true --target_entropy -1   (SAC on the same Pendulum; --eval_* as for ddpg)
"""
import dataclasses
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cleanrl_jl_amd as crl  # noqa: E402
from cleanrl_jl_amd import config_parser  # noqa: E402


def main():
    if len(sys.argv) < 2 or sys.argv[1] not in ("ppo", "a2c", "dqn", "ddpg", "td3", "sac"):
        raise SystemExit(__doc__)
    algo, argv = sys.argv[1], sys.argv[2:]

    def take(flags):
        """the options that are not fields of the algorithm's config struct: removed from argv, returned as keywords"""
        nonlocal argv
        kw = {}
        for flag, cast in flags:
            if flag in argv:
                i = argv.index(flag)
                if i + 1 >= len(argv):
                    raise SystemExit(f"{flag} needs a value")
                kw[flag[2:]] = cast(argv[i + 1])
                argv = argv[:i] + argv[i + 2:]
        return kw

    if algo == "ppo":
        # not PPOConfig fields: the env of ppo.jl:82, the width of networks.jl:36 and the evaluation / diagnostics cadence (crl_ppo_evaluate, crl_ppo_diagnose)
        kw = take((("--env", str), ("--hidden", int), ("--eval_every", int), ("--eval_envs", int), ("--eval_episodes", int), ("--diag_every", int)))
        crl.ppo(config_parser.argparse_struct(crl.PPOConfig(), argv), logger_kw=dict(to_terminal=True, to_tensorboard=False), **kw)
    elif algo == "a2c":
        kw = take((("--eval_every", int), ("--eval_envs", int), ("--eval_episodes", int)))      # the evaluation cadence (crl_a2c_evaluate)
        crl.a2c(config_parser.argparse_struct(crl.A2CConfig(), argv), to_terminal=True, to_tensorboard=False, **kw).close()
    elif algo == "ddpg":
        kw = take((("--eval_every", int), ("--eval_envs", int), ("--eval_episodes", int)))      # the evaluation cadence (crl_ddpg_evaluate)
        crl.ddpg(config_parser.argparse_struct(crl.DDPGConfig(), argv), "pendulum", to_terminal=True, to_tensorboard=False, **kw).close()
    elif algo == "td3":
        kw = take((("--eval_every", int), ("--eval_envs", int), ("--eval_episodes", int)))      # the evaluation cadence (crl_ddpg_evaluate, critic 1)
        crl.td3(config_parser.argparse_struct(crl.TD3Config(), argv), "pendulum", to_terminal=True, to_tensorboard=False, **kw).close()
    elif algo == "sac":
        kw = take((("--eval_every", int), ("--eval_envs", int), ("--eval_episodes", int)))      # the evaluation cadence (crl_ddpg_evaluate, critic 1)
        te = take((("--target_entropy", float),))                                               # None (= -act_dim) unless given: no type to parse it by
        cfg = config_parser.argparse_struct(dataclasses.replace(crl.SACConfig(), target_entropy=0.0), argv)
        cfg.target_entropy = te.get("target_entropy")
        crl.sac(cfg, "pendulum", to_terminal=True, to_tensorboard=False, **kw).close()
    else:
        kw = take((("--eval_every", int), ("--eval_envs", int), ("--eval_episodes", int)))      # the evaluation cadence (crl_dqn_evaluate)
        # prioritized replay (crl_dqn_per_create): --per switches it on, the --per_* options are PEROptions' fields and imply it
        po = take((("--per_alpha", float), ("--per_beta_start", float), ("--per_beta_end", float), ("--per_beta_duration", float), ("--per_eps", float)))
        per = None
        if "--per" in argv or po:
            argv = [a for a in argv if a != "--per"]
            per = crl.PEROptions(**{name[4:]: v for name, v in po.items()})
        # the TD target (crl_dqn_create_with): --double_q and --n_step N are DQNTargetOptions' fields; both combine with --per
        to = take((("--n_step", int),))
        target = None
        if "--double_q" in argv or to:
            target = crl.DQNTargetOptions(n_step=to.get("n_step", 1), double_q="--double_q" in argv)
            argv = [a for a in argv if a != "--double_q"]
        # the categorical critic (crl_dqn_c51_create): --c51 switches it on, --n_atoms / --v_min / --v_max are C51Options' fields and imply it
        co = take((("--n_atoms", int), ("--v_min", float), ("--v_max", float)))
        dist = None
        if "--c51" in argv or co:
            argv = [a for a in argv if a != "--c51"]
            dist = crl.C51Options(**co)
        # the dueling heads (crl_dqn_dueling_create): --dueling combines with --per, --double_q / --n_step and --c51
        dueling = "--dueling" in argv
        argv = [a for a in argv if a != "--dueling"]
        # noisy linear layers (crl_dqn_noisy_create): --noisy switches them on, --sigma0 is NoisyOptions' field and implies it; combines with all of
        # the above. NoisyNets explore by their noise, so epsilon_start / epsilon_end default to 0 here unless they are given.
        no = take((("--sigma0", float),))
        noisy = None
        base = crl.DQNConfig()
        if "--noisy" in argv or no:
            argv = [a for a in argv if a != "--noisy"]
            noisy = crl.NoisyOptions(**no)
            base = dataclasses.replace(base, epsilon_start=0.0, epsilon_end=0.0)
        crl.dqn(config_parser.argparse_struct(base, argv), per, target, dist, dueling, noisy, to_terminal=True, to_tensorboard=False, **kw).close()


if __name__ == "__main__":
    main()
