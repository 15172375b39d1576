# CleanRLHip.jl — the Julia shell a CleanRL.jl maintainer drops next to src/algorithms/ppo.jl.
#
# It keeps the reference's surface (PPOConfig, ppo, get_action, logprob_actions, gae and the two @info records of
# src/algorithms/ppo.jl:157,247) and forwards every numeric step to libcleanrl_hip.so through `ccall`.
# NOT EXECUTED IN THIS REPO'S CI: the build image has no Julia (SURVEY.md F4). The same C entry points are exercised
# through the ctypes mirror (cleanrl.jl_amd/_lib.py) by tests/; the struct layout below is the one
# tests/test_host_cpu.py::test_config_struct_matches_header_and_reference_defaults pins (104 bytes).
module CleanRLHip

export PPOConfig, ppo, get_action, logprob_actions, gae, a2c, dqn, PEROptions, DQNTargetOptions, C51Options, NoisyOptions, c51_probs, per_status, q_values, ddpg, ddpg_external, ddpg_evaluate, td3, td3_external, sac, sac_external, sac_status, get_q_both, dqn_evaluate, a2c_evaluate, a2c_forward, a2c_read_grads, get_q, actor_mean, reference_ddpg_params, reference_params, init_params!, comm_unique_id, comm_init!, comm_peer_export!, comm_peer_attach!, env_step!, act_device!, record_device!, update!, stream, ppo_external,
       comm_destroy!, set_option!, get_option, evaluate, diagnose

const libcrl = get(ENV, "CLEANRL_HIP_LIB", joinpath(@__DIR__, "..", "cleanrl.jl_amd", "libcleanrl_hip.so"))

# ppo.jl:1-19 — unchanged
Base.@kwdef struct PPOConfig
  total_timesteps::Int = 500_000
  num_steps::Int = 32
  num_envs::Int = 4
  num_minibatches::Int = 4
  update_epochs::Int = 4
  lr::Float32 = 2.5f-4
  gamma::Float32 = 0.99
  gae_lambda::Float32 = 0.95
  clip_coef::Float32 = 0.2
  ent_coeff::Float32 = 0.01
  v_coef::Float32 = 0.5
  normalize_advantages::Bool = true
  clip_value_loss::Bool = true
  anneal_lr::Bool = true
end

# crl_ppo_config (include/cleanrl_hip.h) — isbits, C layout
struct CrlConfig
  total_timesteps::Int64
  num_steps::Int32; num_envs::Int32; num_minibatches::Int32; update_epochs::Int32
  lr::Float32; gamma::Float32; gae_lambda::Float32; clip_coef::Float32; ent_coeff::Float32; v_coef::Float32
  normalize_advantages::Int32; clip_value_loss::Int32; anneal_lr::Int32
  obs_dim::Int32; n_act::Int32; hidden::Int32; gae_mode::Int32; env_kind::Int32; stale_obs::Int32
  env_id_offset::Int32; shuffle_mode::Int32
  seed::UInt64
end

struct CrlStats            # crl_ppo_stats
  loss::Float64; pg_loss::Float64; v_loss::Float64; entropy_loss::Float64
  adv_mean::Float64; adv_std::Float64; u_value::Float64; n_unclipped_wins::Float64
end
struct CrlEpisodeStats     # crl_episode_stats
  episodes::Float64; return_sum::Float64; length_sum::Float64; return_max::Float64
end
struct CrlEpisodeRecord    # crl_episode_record: one per finished episode (ppo.jl:147-162)
  episode_return::Float32; episode_length::Int32; env::Int32; step::Int32
end
struct CrlIterationReport  # crl_ppo_iteration_report: whose records crl_ppo_iterate_async / crl_ppo_drain handed back
  iteration::Int64; episodes::CrlEpisodeStats; n_episodes::Int64; n_ring::Int32; pad::Int32
end
struct CrlEvalConfig       # crl_eval_config: what crl_ppo_evaluate runs (mode 0 = greedy, 1 = sampled)
  num_envs::Int32; episodes_per_env::Int32; mode::Int32; trace_steps::Int32; seed::UInt64
end
struct CrlEvalReport       # crl_eval_report: Float64 summary of the per-episode arrays (population standard deviation)
  episodes::Int64; env_steps::Int64; return_mean::Float64; return_std::Float64; return_min::Float64; return_max::Float64; length_mean::Float64
end
struct CrlDiag             # crl_ppo_diag: raw Float64 sums of crl_ppo_diagnose and the fields derived from them (entropy: per sample = n_act x entropy_loss)
  n::Int64; n_clipped::Int64
  sum_logratio::Float64; sum_kl::Float64; sum_entropy::Float64; ratio_min::Float64; ratio_max::Float64
  sum_ret::Float64; sum_ret2::Float64; sum_res_old::Float64; sum_res_old2::Float64; sum_res_new::Float64; sum_res_new2::Float64
  old_approx_kl::Float64; approx_kl::Float64; clipfrac::Float64; entropy::Float64; explained_variance::Float64; explained_variance_new::Float64
end

check(rc::Int32) = rc == 0 || error(unsafe_string(ccall((:crl_last_error, libcrl), Cstring, ())))

mutable struct Agent
  h::Ptr{Cvoid}
  config::PPOConfig
  obs_dim::Int; n_act::Int; hidden::Int; device::Int
  # The reference derives the shapes from the env and the network builder (ppo.jl:85-87: single_state_space / single_action_space;
  # networks.jl:36-38: make_actor_critic(action_space, obs_space, hidden_sizes = [64, 64])); here they are keywords with the same
  # defaults — obs_dim = length(single_state_space), n_act = length(single_action_space), hidden = hidden_sizes[1] (both hidden layers
  # are equal, as in the reference). 4 / 2 / 64 runs the fused kernels; any other shape (obs ≤ 64, act ≤ 16, hidden 64 / 128 / 256 —
  # e.g. the LunarLander-shaped 8 / 4 / 256 of BASELINE config 3) runs the layer-wise path and needs env_kind 1 (synthetic) or 2 (external).
  # gae_mode 0 = the reference's loop (ppo.jl:66), 1 = bootstrap from next_value; stale_obs = the reference's Q7 behaviour.
  # shuffle_mode 2 = CRL_SHUFFLE_BLOCKED_FY: an exact uniform shuffle like Random.shuffle (ppo.jl:194); same default as the
  # ctypes mirror (cleanrl.jl_amd/ppo.py). 0 = serial Fisher–Yates, 1 = keyed bijection (pseudo-random, faster).
  function Agent(config::PPOConfig; obs_dim::Integer=4, n_act::Integer=2, hidden::Integer=64, env_kind::Integer=(obs_dim == 4 && n_act == 2 ? 0 : 1),
                 gae_mode::Integer=0, stale_obs::Bool=true, device::Integer=0, seed=0x5EED, env_id_offset::Integer=0, shuffle_mode::Integer=2)
    c = CrlConfig(config.total_timesteps, config.num_steps, config.num_envs, config.num_minibatches, config.update_epochs,
                  config.lr, config.gamma, config.gae_lambda, config.clip_coef, config.ent_coeff, config.v_coef,
                  config.normalize_advantages, config.clip_value_loss, config.anneal_lr,
                  obs_dim, n_act, hidden, gae_mode, env_kind, stale_obs, env_id_offset, shuffle_mode, seed)
    out = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:crl_ppo_create, libcrl), Int32, (Ref{CrlConfig}, Int32, Ref{Ptr{Cvoid}}), c, device, out))
    a = new(out[], config, obs_dim, n_act, hidden, device)
    finalizer(x -> ccall((:crl_ppo_destroy, libcrl), Int32, (Ptr{Cvoid},), x.h), a)
  end
end
# number of Float32 parameters of Flux.params(actor, critic) for the handle's shapes (networks.jl:36-49)
function param_count(a::Agent)
  n = Ref{Int64}(0)
  check(ccall((:crl_ppo_param_count, libcrl), Int32, (Ptr{Cvoid}, Ref{Int64}), a.h, n))
  Int(n[])
end

# Flux.params(actor, critic) → one flat Float32 vector in the same order (ppo.jl:196); W is (out,in) column-major
# exactly as Flux stores it, so `vcat(vec.(Flux.params(actor, critic))...)` is the argument.
set_params!(a::Agent, flat::Vector{Float32}) =
  GC.@preserve flat check(ccall((:crl_ppo_write, libcrl), Int32, (Ptr{Cvoid}, Int32, Ptr{Cvoid}, Csize_t), a.h, 9, pointer(flat), sizeof(flat)))

# ppo.jl:87 — `actor, critic = Networks.make_actor_critic(single_act_space, single_obs_space) .|> Flux.f32` — when the caller has no Flux
# networks to upload: the library's own host-side restatement of networks.jl:36-49 (orthogonal weights, gains √2 / 0.01 / 1.0, zero biases;
# crl_ppo_init_params). A fresh handle holds zeros and every computing entry point refuses to run on them ("parameters not set").
init_params!(a::Agent, seed::Integer=0) = check(ccall((:crl_ppo_init_params, libcrl), Int32, (Ptr{Cvoid}, UInt64), a.h, UInt64(seed)))

# The reference's own builder, flattened the way the boundary wants it: `Networks` is the reference's module (src/utils/networks.jl), `Flux` the
# Flux it loaded. make_actor_critic only takes `length` of its two spaces (networks.jl:37-38), so Base.OneTo stands in for them.
function reference_params(Networks, Flux, n_act::Integer, obs_dim::Integer, hidden::Integer)
  actor, critic = Networks.make_actor_critic(Base.OneTo(n_act), Base.OneTo(obs_dim), Int[hidden, hidden]) .|> Flux.f32     # ppo.jl:87
  Vector{Float32}(vcat(vec.(Flux.params(actor, critic))...))                                                             # ppo.jl:196 order
end
# Default network builder of ppo / a2c: inside the reference package (this file included next to src/algorithms/ppo.jl, where `Networks` and
# `Flux` are names of the enclosing module, src/CleanRL.jl:12,23) the reference's own make_actor_critic; standalone `nothing`, and the entry
# points then take the library's initialiser — never zeros.
function _default_init()
  pm = parentmodule(@__MODULE__)
  (isdefined(pm, :Networks) && isdefined(pm, :Flux)) || return nothing
  (n_act, obs_dim, hidden) -> reference_params(getfield(pm, :Networks), getfield(pm, :Flux), n_act, obs_dim, hidden)
end

# ppo.jl:21-32 — `actor` is the Agent holding the weights on the GPU; u are the rand() draws of StatsBase.sample
function get_action(obs::AbstractVecOrMat{Float32}, actor::Agent; u::Vector{Float64}=rand(size(obs, ndims(obs))))
  n = size(obs, ndims(obs)); o = Array(obs)
  action = Vector{Int32}(undef, n); logprob = Vector{Float32}(undef, n)
  GC.@preserve o u action logprob check(ccall((:crl_policy_act, libcrl), Int32,
    (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float64}, Int32, Ptr{Int32}, Ptr{Float32}, Ptr{Float32}),
    actor.h, o, u, n, action, logprob, C_NULL))
  Int.(action) .+ 1, logprob                      # 1-based like Base.OneTo(2) (ppo.jl:26)
end

# ppo.jl:34-45
function logprob_actions(obs::AbstractVecOrMat{Float32}, actor::Agent, actions::AbstractVector{Int32})
  n = size(obs, ndims(obs)); o = Array(obs); a0 = Int32.(actions .- 1)
  logprob = Vector{Float32}(undef, n); entropy = Matrix{Float32}(undef, actor.n_act, n)   # (n_act, batch): -p .* logp (ppo.jl:42)
  GC.@preserve o a0 logprob entropy check(ccall((:crl_logprob_actions, libcrl), Int32,
    (Ptr{Cvoid}, Ptr{Float32}, Ptr{Int32}, Int32, Ptr{Float32}, Ptr{Float32}), actor.h, o, a0, n, logprob, entropy))
  logprob, entropy
end

# ppo.jl:48-73 — one env; values [0,k], rewards [1,k], terminals [0,k]. The last slot is 0 (upstream: uninitialised).
# `device` names the GPU the stateless scan runs on (an Agent's own is agent.device).
function gae(values::AbstractVector{Float32}, rewards::AbstractVector{Float32}, terminals::AbstractVector{Bool},
             γ::Float32, λ::Float32; mode::Integer=0, device::Integer=0, seg::Integer=0, tile::Integer=0, nt_loads::Integer=2)
  k = length(rewards)
  v = Vector{Float32}(values[1:k]); r = Vector{Float32}(rewards); t = UInt8.(terminals[1:k])   # BitArray → bytes
  nv = Float32[values[k+1]]; nd = UInt8[terminals[k+1]]
  adv = Vector{Float32}(undef, k)
  GC.@preserve v r t nv nd adv check(ccall((:crl_gae_opt, libcrl), Int32,
    (Int32, Ptr{Float32}, Ptr{Float32}, Ptr{UInt8}, Ptr{Float32}, Ptr{UInt8}, Int32, Int32, Float32, Float32, Int32,
     Ptr{Float32}, Ptr{Float32}, Int32, Int32, Int32), device, v, r, t, nv, nd, 1, k, γ, λ, mode, adv, C_NULL, seg, tile, nt_loads))
  adv
end

# Data parallelism over num_envs, one Julia process per GPU (the reference is single-process): rank 0 draws the 128-byte RCCL
# id, the launcher (MPI.jl, Distributed, a file) hands it to every rank, each rank attaches its shard handle.
function comm_unique_id()
  id = Vector{UInt8}(undef, 128)
  GC.@preserve id check(ccall((:crl_comm_unique_id, libcrl), Int32, (Ptr{UInt8},), id))
  id
end
comm_init!(a::Agent, id::Vector{UInt8}, world_size::Integer, rank::Integer) =
  GC.@preserve id check(ccall((:crl_comm_init, libcrl), Int32, (Ptr{Cvoid}, Ptr{UInt8}, Int32, Int32), a.h, id, world_size, rank))

# The same exchange without RCCL: a one-shot all-reduce over peer-mapped mailboxes (csrc/peer.hip). Every rank exports its
# mailbox (64-byte hipIpcMemHandle_t), the launcher all-gathers the handles, every rank attaches all of them in rank order.
function comm_peer_export!(a::Agent, world_size::Integer, rank::Integer)
  hnd = Vector{UInt8}(undef, 64)
  GC.@preserve hnd check(ccall((:crl_comm_peer_export, libcrl), Int32, (Ptr{Cvoid}, Int32, Int32, Ptr{UInt8}), a.h, world_size, rank, hnd))
  hnd
end
comm_peer_attach!(a::Agent, handles::Vector{UInt8}) =
  GC.@preserve handles check(ccall((:crl_comm_peer_attach, libcrl), Int32, (Ptr{Cvoid}, Ptr{UInt8}), a.h, handles))

# Detaches whatever exchange is attached (a launcher falling back from a partially failed RCCL start to the peer all-reduce)
comm_destroy!(a::Agent) = check(ccall((:crl_comm_destroy, libcrl), Int32, (Ptr{Cvoid},), a.h))

# Per-handle options (include/cleanrl_hip.h lists them): kernel-flavour / numerics switches, integer-valued, by name, e.g.
# set_option!(agent, "gemm", 1) selects the bf16x3 flavour, set_option!(agent, "guard_window", 1) a read-back per iteration.
set_option!(a::Agent, key::AbstractString, value::Integer) =
  check(ccall((:crl_ppo_set_option, libcrl), Int32, (Ptr{Cvoid}, Cstring, Int64), a.h, key, value))
function get_option(a::Agent, key::AbstractString)
  v = Ref{Int64}(0)
  check(ccall((:crl_ppo_get_option, libcrl), Int32, (Ptr{Cvoid}, Cstring, Ref{Int64}), a.h, key, v))
  v[]
end

# ppo.jl:75 — same signature; the loop body (ppo.jl:117-253) runs on the GPU, one ccall per update.
# episode_records > 0 turns on the device ring (crl_episode_ring_enable): every finished episode leaves {return, length, env,
# step} and `ppo` emits ONE "Episode Statistics" record per episode in the reference's order (ppo.jl:147-165: step by step,
# done envs ascending; global_step as of that step, ppo.jl:124). With 0 it emits one aggregate record per update (65536 envs
# finish ~10^5 episodes per rollout). Multi-GPU: pass comm = (id, world_size, rank) and a config whose num_envs is the shard.
# Shapes other than the reference's CartPole 4 / 2 / 64 are keywords forwarded to Agent (obs_dim, n_act, hidden, env_kind, gae_mode,
# stale_obs): ppo(cfg; obs_dim = 8, n_act = 4, hidden = 256) is BASELINE config 3 on the synthetic env.
# ppo.jl:77 installs the global logger before anything else (`Logger.make_logger("ppo-2-test"; to_terminal=false)`, logger.jl:7-29): `make_logger`
# is that function — by default the `Logger` module of the package this file is included into (src/CleanRL.jl includes utils/logger.jl before
# the algorithms), `nothing` when there is none (standalone use: the caller's own global logger receives the @info records).
_default_make_logger() = isdefined(parentmodule(@__MODULE__), :Logger) ? getfield(parentmodule(@__MODULE__), :Logger).make_logger : nothing
# ppo.jl:87 — the networks: `params` (a caller's own `vcat(vec.(Flux.params(actor, critic))...)`) wins; otherwise `init(n_act, obs_dim, hidden)` builds them —
# by default the reference's Networks.make_actor_critic(...) .|> Flux.f32 when this file lives inside the reference package (_default_init), and
# the library's restatement of it (init_params!, seeded by init_seed) when it does not. There is no path that leaves the handle's zeros in place:
# under data parallelism every rank must end up with the SAME parameters, so pass `params` or a seeded init there (init_params! with one
# init_seed is identical on all ranks; the reference builder draws from each process's own RNG).
# ppo.jl:82 — the env is one keyword: ppo(config; env = :acrobot). obs_dim / n_act follow from it like ppo.jl:85-86 reads them off the env's spaces;
# env_kind numbers are include/cleanrl_hip.h's CRL_ENV_*. `env = nothing` keeps the explicit shape keywords (env_kind = ... keeps working).
const ENVS = Dict(:cartpole => (env_kind=0, obs_dim=4, n_act=2), :mountaincar => (env_kind=3, obs_dim=2, n_act=3), :acrobot => (env_kind=4, obs_dim=6, n_act=3))
function env_shape(env::Union{Nothing,Symbol,AbstractString}; shape...)
  env === nothing && return (; shape...)
  key = Symbol(lowercase(String(env)))
  haskey(ENVS, key) || throw(ArgumentError("unknown env $(repr(env)): one of $(sort(collect(keys(ENVS))))"))
  want = ENVS[key]
  for (k, v) in pairs(want)
    haskey(shape, k) && shape[k] != v && throw(ArgumentError("env = $(repr(env)) has $k = $v, got $k = $(shape[k])"))
  end
  return merge((; shape...), want)
end
# env(actions) + reward / is_terminated / state + reset!(env) of the terminated (ppo.jl:130-165 without the policy) on the agent's on-device envs:
# 0-based actions, `gstep` keys the reset stream like step gstep of the training loop. Returns (next_obs (obs_dim, num_envs), reward, done).
function env_step!(a::Agent, action::Vector{Int32}, gstep::Integer=0)
  nt = length(action)
  obs = Matrix{Float32}(undef, a.obs_dim, nt); reward = Vector{Float32}(undef, nt); done = Vector{UInt8}(undef, nt)
  GC.@preserve action obs reward done check(ccall((:crl_env_step, libcrl), Int32, (Ptr{Cvoid}, Ptr{Int32}, UInt64, Ptr{Float32}, Ptr{Float32}, Ptr{UInt8}),
                                                  a.h, action, UInt64(gstep), obs, reward, done))
  return obs, reward, done .!= 0
end
# How good is the current policy? crl_ppo_evaluate: the agent's actor, frozen, plays episodes_per_env whole episodes on each of num_envs fresh on-device
# envs of its kind, in one launch; training state is not touched (no reference counterpart: ppo.jl only logs the returns of its sampled rollouts).
# greedy = largest logit (lowest index on a tie), else get_action's sampler (ppo.jl:21-32). returns / lengths are (num_envs, episodes_per_env) —
# the C arrays are env-fastest —, trace (num_envs, trace_steps) holds the 0-based actions of the first trace_steps steps, -1 once an env was done.
const EVAL_SEED = UInt64(0xE7A1)
function evaluate(a::Agent; num_envs::Integer=256, episodes_per_env::Integer=1, greedy::Bool=true, seed::Integer=EVAL_SEED, trace_steps::Integer=0)
  num_envs >= 1 || throw(ArgumentError("evaluate: num_envs must be >= 1, got $num_envs"))
  episodes_per_env >= 1 || throw(ArgumentError("evaluate: episodes_per_env must be >= 1, got $episodes_per_env"))
  trace_steps >= 0 || throw(ArgumentError("evaluate: trace_steps must be >= 0, got $trace_steps"))
  cfg = Ref(CrlEvalConfig(num_envs, episodes_per_env, greedy ? 0 : 1, trace_steps, UInt64(seed)))
  report = Ref{CrlEvalReport}()
  returns = Matrix{Float32}(undef, num_envs, episodes_per_env); lengths = Matrix{Int32}(undef, num_envs, episodes_per_env)
  trace = Matrix{Int32}(undef, num_envs, trace_steps)
  GC.@preserve returns lengths trace check(ccall((:crl_ppo_evaluate, libcrl), Int32,
                                                 (Ptr{Cvoid}, Ref{CrlEvalConfig}, Ref{CrlEvalReport}, Ptr{Float32}, Ptr{Int32}, Ptr{Int32}),
                                                 a.h, cfg, report, returns, lengths, trace_steps > 0 ? pointer(trace) : Ptr{Int32}(C_NULL)))
  return (; report = report[], returns, lengths, trace)
end
# Is the update healthy? crl_ppo_diagnose: one read-only launch over the rollout buffer the agent currently holds, with its current parameters (after an
# update: the last rollout against the post-update policy; no reference counterpart). Returns the CrlDiag struct: approx_kl, old_approx_kl, clipfrac,
# entropy, explained_variance, explained_variance_new, the ratio's range and the raw sums. per_sample = true also returns new_logprob / new_value (num_envs, num_steps).
function diagnose(a::Agent; per_sample::Bool=false)
  out = Ref{CrlDiag}()
  nt, k = Int(a.config.num_envs), Int(a.config.num_steps)
  lp = Matrix{Float32}(undef, per_sample ? nt : 0, per_sample ? k : 0); v = similar(lp)
  GC.@preserve lp v check(ccall((:crl_ppo_diagnose, libcrl), Int32, (Ptr{Cvoid}, Ref{CrlDiag}, Ptr{Float32}, Ptr{Float32}),
                                a.h, out, per_sample ? pointer(lp) : Ptr{Float32}(C_NULL), per_sample ? pointer(v) : Ptr{Float32}(C_NULL)))
  return per_sample ? (; report = out[], new_logprob = lp, new_value = v) : out[]
end
function ppo(config::PPOConfig=PPOConfig(); device::Integer=0, params::Union{Nothing,Vector{Float32}}=nothing, init=_default_init(), init_seed::Integer=0,
             episode_records::Integer=4096, comm::Union{Nothing,Tuple{Vector{UInt8},Int,Int}}=nothing, run_name::AbstractString="ppo-2-test",
             make_logger=_default_make_logger(), env::Union{Nothing,Symbol,AbstractString}=nothing,
             eval_every::Integer=0, eval_envs::Integer=256, eval_episodes::Integer=1, shape...)
  shape = env_shape(env; shape...)                                         # ppo.jl:82,85-86
  eval_every >= 0 || throw(ArgumentError("ppo: eval_every must be >= 0, got $eval_every"))
  if eval_every > 0                                                        # checked here, not at the first evaluation in the middle of training
    eval_envs >= 1 || throw(ArgumentError("ppo: eval_envs must be >= 1, got $eval_envs"))
    eval_episodes >= 1 || throw(ArgumentError("ppo: eval_episodes must be >= 1, got $eval_episodes"))
  end
  make_logger === nothing || make_logger(run_name; to_terminal=false)      # ppo.jl:77
  world, rank = comm === nothing ? (1, 0) : (comm[2], comm[3])
  agent = Agent(config; device, env_id_offset=rank * config.num_envs, shape...)
  if params === nothing && init !== nothing && world == 1
    params = init(agent.n_act, agent.obs_dim, agent.hidden)                # ppo.jl:87 with the reference's own builder
  end
  if params === nothing
    init_params!(agent, init_seed)                                         # ppo.jl:87 through crl_ppo_init_params (same on every rank)
  else
    length(params) == param_count(agent) || error("params has $(length(params)) entries, the networks have $(param_count(agent))")
    set_params!(agent, params)
  end
  comm === nothing || comm_init!(agent, comm[1], world, rank)
  episode_records > 0 && check(ccall((:crl_episode_ring_enable, libcrl), Int32, (Ptr{Cvoid}, Int32), agent.h, episode_records))
  check(ccall((:crl_env_reset, libcrl), Int32, (Ptr{Cvoid},), agent.h))
  batch_size = config.num_steps * config.num_envs * world          # ppo.jl:89 over the whole job
  num_updates = config.total_timesteps ÷ batch_size                # ppo.jl:91
  nstats = config.update_epochs * config.num_minibatches
  stats = Vector{CrlStats}(undef, nstats)
  recs = Vector{CrlEpisodeRecord}(undef, max(episode_records, 1)); rep = Ref{CrlIterationReport}()
  last_log_step = 0; start_time = time()
  # the records of one update, in the reference's order: its episodes (ppo.jl:147-165), then its minibatches (ppo.jl:246-248)
  function emit(r::CrlIterationReport)
    base = r.iteration * batch_size
    global_step = base + batch_size
    if episode_records > 0
      for e in sort!(recs[1:r.n_ring]; by = x -> (x.step, x.env))          # the reference's order: step by step, done envs ascending
        gs = base + (e.step + 1) * config.num_envs * world                # ppo.jl:124 global_step += num_envs per step
        steps_per_sec = trunc(gs / (time() - start_time))
        log_step_inc = last_log_step == 0 ? 0 : gs - last_log_step
        @info "Episode Statistics" episode_return = e.episode_return episode_length = e.episode_length global_step = gs steps_per_sec log_step_increment = log_step_inc
        last_log_step = gs
      end
    elseif r.episodes.episodes > 0
      steps_per_sec = trunc(global_step / (time() - start_time))
      episode_return = r.episodes.return_sum / r.episodes.episodes; episode_length = r.episodes.length_sum / r.episodes.episodes
      log_step_inc = last_log_step == 0 ? 0 : global_step - last_log_step
      @info "Episode Statistics" episode_return episode_length global_step steps_per_sec log_step_increment = log_step_inc
      last_log_step = global_step
    end
    for s in stats
      log_step_inc = last_log_step == 0 ? 0 : global_step - last_log_step
      @info "Training Statistics" loss = s.loss pg_loss = s.pg_loss v_loss = s.v_loss entropy_loss = s.entropy_loss log_step_increment = log_step_inc
      last_log_step = global_step
    end
  end
  # Pipelined read-back (crl_ppo_iterate_async): update k's records are handed over after update k + 1 has been enqueued, so the GPU never waits while Julia
  # logs; the record stream is the reference's, one update late, and crl_ppo_drain hands over the last one.
  for update in 1:num_updates
    GC.@preserve stats recs check(ccall((:crl_ppo_iterate_async, libcrl), Int32, (Ptr{Cvoid}, Ref{CrlIterationReport}, Ptr{CrlStats}, Ptr{CrlEpisodeRecord}, Int32),
                                        agent.h, rep, stats, recs, episode_records))
    rep[].iteration >= 0 && emit(rep[])
    evaluating = eval_every > 0 && update % eval_every == 0
    if evaluating || update == num_updates
      # the update's own records, which would otherwise arrive one call late: after the last update, and in front of an evaluation, whose record
      # follows them (the next crl_ppo_iterate_async then has nothing to hand over)
      GC.@preserve stats recs check(ccall((:crl_ppo_drain, libcrl), Int32, (Ptr{Cvoid}, Ref{CrlIterationReport}, Ptr{CrlStats}, Ptr{CrlEpisodeRecord}, Int32),
                                          agent.h, rep, stats, recs, episode_records))
      rep[].iteration >= 0 && emit(rep[])
    end
    if evaluating
      # "Evaluation Statistics": a greedy held-out score of the parameters this update left (the call runs behind the update on the stream)
      ev = evaluate(agent; num_envs=eval_envs, episodes_per_env=eval_episodes).report
      @info "Evaluation Statistics" eval_return_mean = ev.return_mean eval_return_std = ev.return_std eval_length_mean = ev.length_mean global_step = update * batch_size
    end
  end
  agent
end

# ------------------------------------------------------------------------------------------------------
# Device-resident external envs (include/cleanrl_hip.h, "Device-resident external envs"): the env lives on the agent's GPU — AMDGPU.jl arrays, the caller's
# own kernels — and hands over DEVICE pointers (`pointer(roc_array)`); nothing is staged and no call below makes the host wait, except update! on the
# 4 / 2 / 64 path (once per update). peer_stream: the env's hipStream_t when it is not the agent's (`C_NULL`: the caller orders its work itself).
# ------------------------------------------------------------------------------------------------------
# the agent's hipStream_t: run the env on it (AMDGPU.jl: HIPStream(stream(agent))), or pass the env's own stream as peer_stream
function stream(a::Agent)
  s = Ref{Ptr{Cvoid}}(C_NULL)
  check(ccall((:crl_ppo_stream, libcrl), Int32, (Ptr{Cvoid}, Ref{Ptr{Cvoid}}), a.h, s))
  return s[]
end
# ppo.jl:127-128 + the policy's share of Buffer.add! (:133-140) for slot `step` (0-based), one launch; the 0-based actions land in action_d
act_device!(a::Agent, step::Integer, obs_d::Ptr{Float32}, done_d::Ptr{UInt8}, action_d::Ptr{Int32}; peer_stream::Ptr{Cvoid}=C_NULL) =
  check(ccall((:crl_rollout_act_device, libcrl), Int32, (Ptr{Cvoid}, Int32, Ptr{Float32}, Ptr{UInt8}, Ptr{Int32}, Ptr{Cvoid}),
              a.h, step, obs_d, done_d, action_d, peer_stream))
# ppo.jl:132,137,143-165: reward into slot `step`, next_obs / next_done, the episode bookkeeping
record_device!(a::Agent, step::Integer, reward_d::Ptr{Float32}, next_obs_d::Ptr{Float32}, next_done_d::Ptr{UInt8}; peer_stream::Ptr{Cvoid}=C_NULL) =
  check(ccall((:crl_rollout_record_device, libcrl), Int32, (Ptr{Cvoid}, Int32, Ptr{Float32}, Ptr{Float32}, Ptr{UInt8}, Ptr{Cvoid}),
              a.h, step, reward_d, next_obs_d, next_done_d, peer_stream))
# ppo.jl:168-253 on the resident buffer; returns the update_epochs * num_minibatches loss records
function update!(a::Agent)
  stats = Vector{CrlStats}(undef, a.config.update_epochs * a.config.num_minibatches)
  GC.@preserve stats check(ccall((:crl_ppo_update, libcrl), Int32, (Ptr{Cvoid}, Ptr{CrlStats}), a.h, stats))
  return stats
end
# The ppo.jl:117-253 loop with the env outside the library. `env` is anything with env.num_envs, env.obs_dim, env.n_act, env.action (a Ptr{Int32} the actions
# are written to), reset!(env) -> (obs_d, done_d) and step!(env) -> (reward_d, next_obs_d, next_done_d), all device pointers into arrays the env keeps alive;
# env.stream (a hipStream_t, optional) is passed as peer_stream. `reset!` / `step!` are the caller's functions, given as keywords.
function ppo_external(config::PPOConfig, env; reset!, step!, device::Integer=0, params::Union{Nothing,Vector{Float32}}=nothing, init_seed::Integer=0,
                      run_name::AbstractString="ppo-external", make_logger=_default_make_logger(), shape...)
  make_logger === nothing || make_logger(run_name; to_terminal=false)
  agent = Agent(config; device, obs_dim=env.obs_dim, n_act=env.n_act, env_kind=2, shape...)
  params === nothing ? init_params!(agent, init_seed) : set_params!(agent, params)
  peer = hasproperty(env, :stream) ? Ptr{Cvoid}(env.stream) : Ptr{Cvoid}(C_NULL)
  batch_size = config.num_steps * config.num_envs
  num_updates = config.total_timesteps ÷ batch_size
  last_log_step = 0; start_time = time()
  obs_d, done_d = reset!(env)                                              # ppo.jl:112-115
  for update in 1:num_updates
    for step in 0:config.num_steps - 1                                     # ppo.jl:123-166
      act_device!(agent, step, obs_d, done_d, env.action; peer_stream=peer)
      reward_d, obs_d, done_d = step!(env)
      record_device!(agent, step, reward_d, obs_d, done_d; peer_stream=peer)
    end
    ep = Ref{CrlEpisodeStats}()
    check(ccall((:crl_episode_stats_read, libcrl), Int32, (Ptr{Cvoid}, Ref{CrlEpisodeStats}), agent.h, ep))
    stats = update!(agent)                                                 # ppo.jl:168-253
    global_step = update * batch_size
    if ep[].episodes > 0
      steps_per_sec = trunc(global_step / (time() - start_time))
      episode_return = ep[].return_sum / ep[].episodes; episode_length = ep[].length_sum / ep[].episodes
      log_step_inc = last_log_step == 0 ? 0 : global_step - last_log_step
      @info "Episode Statistics" episode_return episode_length global_step steps_per_sec log_step_increment = log_step_inc
      last_log_step = global_step
    end
    for s in stats
      log_step_inc = last_log_step == 0 ? 0 : global_step - last_log_step
      @info "Training Statistics" loss = s.loss pg_loss = s.pg_loss v_loss = s.v_loss entropy_loss = s.entropy_loss log_step_increment = log_step_inc
      last_log_step = global_step
    end
  end
  return agent
end

# ------------------------------------------------------------------------------------------------------
# a2c.jl — same names: A2CConfig keeps the reference's fields (a2c.jl:1-10); the loop body runs on the GPU
# ------------------------------------------------------------------------------------------------------
struct CrlA2CConfig       # include/cleanrl_hip.h crl_a2c_config
  lr::Float64; total_timesteps::Int64; min_replay_size::Int32; max_steps::Int32; gamma::Float64; seed::UInt64
end
struct CrlA2CTrainStats; actor_loss::Float64; critic_loss::Float64; n::Int32; trained::Int32; end
struct CrlA2CEpisode; episode_return::Float64; episode_length::Int64; global_step::Int64; end

struct CrlValueEvalReport # crl_value_eval_report: what crl_dqn_evaluate / crl_a2c_evaluate report (v_bias_mean = mean(v0 - disc_return))
  episodes::Int64; env_steps::Int64; return_mean::Float64; return_std::Float64; return_min::Float64; return_max::Float64
  length_mean::Float64; disc_return_mean::Float64; v0_mean::Float64; v_bias_mean::Float64
end

mutable struct A2CAgent
  h::Ptr{Cvoid}
end

# crl_dqn_evaluate / crl_a2c_evaluate (they share their signature): episodes_per_env whole episodes on each of num_envs fresh on-device CartPoles
# in one read-only launch. returns / lengths / disc_returns / v0 are (num_envs, episodes_per_env) — the C arrays are env-fastest —, trace_action
# (num_envs, trace_steps) holds the actions of each env's first trace_steps steps, -1 once the env has played its quota.
function _value_evaluate(sym::Symbol, who::String, h::Ptr{Cvoid}, num_envs, episodes_per_env, mode, seed, trace_steps)
  1 <= num_envs <= 65536 || throw(ArgumentError("$who: num_envs must be in 1..65536, got $num_envs"))
  1 <= episodes_per_env <= 1024 || throw(ArgumentError("$who: episodes_per_env must be in 1..1024, got $episodes_per_env"))
  trace_steps >= 0 || throw(ArgumentError("$who: trace_steps must be >= 0, got $trace_steps"))
  cfg = Ref(CrlEvalConfig(num_envs, episodes_per_env, mode, trace_steps, UInt64(seed)))
  report = Ref{CrlValueEvalReport}()
  returns = Matrix{Float64}(undef, num_envs, episodes_per_env); disc_returns = similar(returns); v0 = similar(returns)
  lengths = Matrix{Int32}(undef, num_envs, episodes_per_env); trace_action = Matrix{Int32}(undef, num_envs, trace_steps)
  tp = trace_steps > 0 ? pointer(trace_action) : Ptr{Int32}(C_NULL)
  GC.@preserve returns lengths disc_returns v0 trace_action check(sym === :dqn ?
    ccall((:crl_dqn_evaluate, libcrl), Int32, (Ptr{Cvoid}, Ref{CrlEvalConfig}, Ref{CrlValueEvalReport}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}),
          h, cfg, report, returns, lengths, disc_returns, v0, tp) :
    ccall((:crl_a2c_evaluate, libcrl), Int32, (Ptr{Cvoid}, Ref{CrlEvalConfig}, Ref{CrlValueEvalReport}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}),
          h, cfg, report, returns, lengths, disc_returns, v0, tp))
  return (report[], returns, lengths, disc_returns, v0, trace_action)
end

# the actor's logits (net = 0: (4, n) → (2, n)) or the critic's values (net = 1: (4, n) → (n,)) for caller-supplied observations: crl_a2c_forward
function a2c_forward(agent::A2CAgent, net::Integer, obs::AbstractMatrix{Float64})
  o = Array(obs); n = size(o, 2); out = net == 1 ? Vector{Float64}(undef, n) : Matrix{Float64}(undef, 2, n)
  GC.@preserve o out check(ccall((:crl_a2c_forward, libcrl), Int32, (Ptr{Cvoid}, Int32, Ptr{Float64}, Int32, Ptr{Float64}), agent.h, net, o, n, out))
  out
end

# the last update's Float32 gradients before ClipNorm, in the parameters' flat layout (an error before the first update): crl_a2c_read_grads
a2c_read_grads(agent::A2CAgent) = (g = Vector{Float32}(undef, 9155); GC.@preserve g check(ccall((:crl_a2c_read_grads, libcrl), Int32, (Ptr{Cvoid}, Ptr{Float32}, Csize_t), agent.h, g, length(g))); g)

# How good is the current actor, and does the critic over-estimate? crl_a2c_evaluate: the actor, frozen, greedy (the larger logit) or sampled from
# the softmax as the training loop does; v0 = critic(s0), report.v_bias_mean = mean(v0 - discounted return). Training state is not touched.
function a2c_evaluate(agent::A2CAgent; num_envs::Integer=256, episodes_per_env::Integer=1, greedy::Bool=true, seed::Integer=EVAL_SEED, trace_steps::Integer=0)
  report, returns, lengths, disc_returns, v0, trace_action =
    _value_evaluate(:a2c, "a2c_evaluate", agent.h, num_envs, episodes_per_env, greedy ? 0 : 1, seed, trace_steps)
  return (; report, returns, lengths, disc_returns, v0, trace_action)
end

# a2c.jl:13-24 — same signature
function discounted_future_rewards(rewards::Vector{Float64}, terminals::Vector{Bool}, final_value::Float64, γ::Float64; device=0)
  out = similar(rewards); t = UInt8.(terminals)
  GC.@preserve rewards t out check(ccall((:crl_a2c_discounted_future_rewards, libcrl), Int32,
    (Int32, Ptr{Float64}, Ptr{UInt8}, Int32, Float64, Float64, Ptr{Float64}), device, rewards, t, length(rewards), final_value, γ, out))
  out
end

# a2c.jl:29 — same signature; `config` is the reference's A2CConfig. a2c.jl:30 installs the logger (terminal + TensorBoard: make_logger's own
# defaults), a2c.jl:37 builds the networks: `params` wins, else `init` (the reference's Networks.make_actor_critic inside the package — a2c.jl:37
# does not pipe through Flux.f32, Flux.orthogonal is Float32 already), else the library's initialiser. Never the handle's zeros.
# eval_every = N > 0: an "Evaluation Statistics" record (eval_return_mean, eval_return_std, eval_v_bias, global_step) after the records of every env
# step that is a multiple of N — the library calls are cut there (chunking changes no bit of the run). Returns the agent (for a2c_evaluate).
function a2c(config; device=0, seed=UInt64(0x5EED), params::Union{Nothing,Vector{Float32}}=nothing, init=_default_init(), init_seed::Integer=0,
             make_logger=_default_make_logger(), eval_every::Integer=0, eval_envs::Integer=256, eval_episodes::Integer=1)
  eval_every >= 0 || throw(ArgumentError("a2c: eval_every must be >= 0, got $eval_every"))
  make_logger === nothing || make_logger("a2c|$(config.run_name)")         # a2c.jl:30
  cfg = CrlA2CConfig(config.lr, config.total_timesteps, config.min_replay_size, 500, config.gamma, seed)
  h = Ref{Ptr{Cvoid}}(C_NULL)
  check(ccall((:crl_a2c_create, libcrl), Int32, (Ref{CrlA2CConfig}, Int32, Ref{Ptr{Cvoid}}), cfg, device, h))
  agent = A2CAgent(h[])
  finalizer(x -> ccall((:crl_a2c_destroy, libcrl), Int32, (Ptr{Cvoid},), x.h), agent)
  params === nothing && init !== nothing && (params = init(2, 4, 64))      # a2c.jl:37 make_actor_critic(env): CartPole 4 / 2, hidden [64, 64]
  if params === nothing
    check(ccall((:crl_a2c_init_params, libcrl), Int32, (Ptr{Cvoid}, UInt64), h[], UInt64(init_seed)))
  else
    GC.@preserve params check(ccall((:crl_a2c_write_params, libcrl), Int32, (Ptr{Cvoid}, Ptr{Float32}, Csize_t), h[], params, length(params)))
  end
  stats = Ref{CrlA2CTrainStats}(); eps = Vector{CrlA2CEpisode}(undef, 4096); n_eps = Ref{Int32}(0); taken = Ref{Int64}(0)
  start_time = time(); global_step = 0
  while global_step < config.total_timesteps
    GC.@preserve eps check(ccall((:crl_a2c_run_until_update, libcrl), Int32,
      (Ptr{Cvoid}, Int64, Ref{CrlA2CTrainStats}, Ptr{CrlA2CEpisode}, Int32, Ref{Int32}, Ref{Int64}),
      h[], eval_every > 0 ? Int64(eval_every - global_step % eval_every) : typemax(Int64), stats, eps, length(eps), n_eps, taken))
    taken[] == 0 && break
    global_step += taken[]
    # the episode whose end triggered the update is the call's LAST record, and the reference logs the update first (a2c.jl:100, then :106)
    for (i, e) in enumerate(@view eps[1:n_eps[]])
      i == n_eps[] && stats[].trained == 1 && @info "Training Statistics" actor_loss = stats[].actor_loss critic_loss = stats[].critic_loss
      steps_per_sec = trunc(e.global_step / (time() - start_time))
      @info "Episode Statistics" episode_return = e.episode_return episode_length = e.episode_length global_step = e.global_step steps_per_sec
    end
    n_eps[] == 0 && stats[].trained == 1 && @info "Training Statistics" actor_loss = stats[].actor_loss critic_loss = stats[].critic_loss
    if eval_every > 0 && global_step % eval_every == 0
      ev = a2c_evaluate(agent; num_envs=eval_envs, episodes_per_env=eval_episodes).report
      @info "Evaluation Statistics" eval_return_mean = ev.return_mean eval_return_std = ev.return_std eval_v_bias = ev.v_bias_mean global_step
    end
  end
  agent
end

# ------------------------------------------------------------------------------------------------------
# dqn.jl — same names: DQNConfig keeps the reference's fields (dqn.jl:1-19); the loop body runs on the GPU
# ------------------------------------------------------------------------------------------------------
struct CrlDQNConfig       # include/cleanrl_hip.h crl_dqn_config
  log_frequency::Int64; total_timesteps::Int64; buffer_size::Int64; min_buff_size::Int64
  lr::Float64
  train_freq::Int64; target_net_freq::Int64; batch_size::Int64
  gamma::Float64; epsilon_start::Float64; epsilon_end::Float64; epsilon_duration::Float64
  max_steps::Int32; pad::Int32
  seed::UInt64
end
struct CrlDQNEpisode; episode_return::Float64; episode_length::Int64; global_step::Int64; epsilon::Float64; end   # dqn.jl:88
struct CrlDQNLossRecord; global_step::Int64; loss::Float64; end                                                    # dqn.jl:116

mutable struct DQNAgent
  h::Ptr{Cvoid}
end

# Prioritized experience replay (Schaul et al. 2016, proportional; include/cleanrl_hip.h crl_dqn_per_options) — not in dqn.jl, so not a DQNConfig
# field: `dqn(config; per = PEROptions())`. beta_duration = nothing means config.total_timesteps. Like the rest of this file, not executed here.
Base.@kwdef struct PEROptions
  alpha::Float64 = 0.6
  beta_start::Float64 = 0.4
  beta_end::Float64 = 1.0
  beta_duration::Union{Nothing,Float64} = nothing
  eps::Float64 = 1e-6
end
struct CrlDQNPEROptions; alpha::Float64; beta_start::Float64; beta_end::Float64; beta_duration::Float64; eps::Float64; end   # crl_dqn_per_options
struct CrlDQNPERStatus; beta::Float64; total::Float64; max_leaf::Float32; tree_leaves::Int32; end                            # crl_dqn_per_status
# beta(g) as the header pins it: the "Training Statistics" record of a PER run carries it
function _per_beta(p::CrlDQNPEROptions, g)
  slope = (p.beta_end - p.beta_start) / p.beta_duration
  v = slope * Float64(g) + p.beta_start
  slope < 0 ? (v < p.beta_end ? p.beta_end : v) : (v > p.beta_end ? p.beta_end : v)
end
# crl_dqn_per_status_read: (beta, total, max_leaf, tree_leaves) of a PER agent; an error on a uniform one
function per_status(agent::DQNAgent)
  st = Ref(CrlDQNPERStatus(0, 0, 0, 0))
  check(ccall((:crl_dqn_per_status_read, libcrl), Int32, (Ptr{Cvoid}, Ref{CrlDQNPERStatus}), agent.h, st))
  st[]
end

# How the TD target is formed (include/cleanrl_hip.h crl_dqn_target_options) — not in dqn.jl, so not a DQNConfig field: `dqn(config; target =
# DQNTargetOptions(n_step = 3, double_q = true))`, with either replay. n_step in 1..16 (uncorrected n-step returns), double_q: the bootstrap action is
# q_net's, its value target_net's. The defaults are dqn.jl's 1-step max. Like the rest of this file, not executed here.
Base.@kwdef struct DQNTargetOptions
  n_step::Int = 1
  double_q::Bool = false
end
struct CrlDQNTargetOptions; n_step::Int32; double_q::Int32; end                                                              # crl_dqn_target_options

# The categorical critic of Bellemare et al. 2017 (include/cleanrl_hip.h crl_dqn_c51_options) — not in dqn.jl, so not a DQNConfig field: `dqn(config;
# dist = C51Options())`, with either replay and any target options. n_atoms in 2..64 atoms evenly spaced on [v_min, v_max]; the head becomes
# Dense(84, 2·n_atoms) and the parameter vector 10764 + 85·2·n_atoms long (crl_dqn_param_count). q_values then returns the expected values, and
# "Training Statistics".loss is the cross-entropy. Like the rest of this file, not executed here.
Base.@kwdef struct C51Options
  n_atoms::Int = 51
  v_min::Float64 = 0.0
  v_max::Float64 = 100.0
end
struct CrlDQNC51Options; n_atoms::Int32; pad::Int32; v_min::Float64; v_max::Float64; end                                     # crl_dqn_c51_options

# Noisy linear layers (NoisyNets, Fortunato et al. 2018; include/cleanrl_hip.h crl_dqn_noisy_options) — not in dqn.jl, so not a DQNConfig field:
# `dqn(config; noisy = NoisyOptions())`, with every other option. Every dense layer learns mu and sigma (the parameter vector is twice the twin's: mu,
# then sigma; crl_dqn_param_count) and acts on mu + sigma·eps with factorised Gaussian eps, redrawn after every update; evaluation and q_values run with
# the noise off. ε-greedy is honoured as configured: the NoisyNet setting is epsilon_start = epsilon_end = 0. Like the rest of this file, not executed here.
Base.@kwdef struct NoisyOptions
  sigma0::Float64 = 0.5
end
struct CrlDQNNoisyOptions; sigma0::Float64; end                                                                              # crl_dqn_noisy_options

# crl_dqn_c51_probs: softmax of q_net(obs) per action, (4, n) → (n_atoms, 2, n); an error on an agent with the scalar critic
function c51_probs(agent::DQNAgent, obs::AbstractMatrix{Float64}, n_atoms::Integer)
  o = Array(obs); n = size(o, 2); p = Array{Float64}(undef, n_atoms, 2, n)
  GC.@preserve o p check(ccall((:crl_dqn_c51_probs, libcrl), Int32, (Ptr{Cvoid}, Ptr{Float64}, Int32, Ptr{Float64}), agent.h, o, n, p))
  p
end

# q_net(obs) (dqn.jl:64) for observations (4, n) Float64 → (2, n) Float64; the expected values on a C51 agent
function q_values(agent::DQNAgent, obs::AbstractMatrix{Float64})
  o = Array(obs); n = size(o, 2); q = Matrix{Float64}(undef, 2, n)
  GC.@preserve o q check(ccall((:crl_dqn_q_values, libcrl), Int32, (Ptr{Cvoid}, Ptr{Float64}, Int32, Ptr{Float64}), agent.h, o, n, q))
  q
end

# How good is the greedy policy, and does q_net over-estimate? crl_dqn_evaluate: q_net (not the target), frozen and WITHOUT the ε-greedy exploration
# (dqn.jl:61-68 never lets ε below 0.05, so the reference's "Episode Statistics" score an exploring policy); q0 = max_a Q(s0, a),
# report.v_bias_mean = mean(q0 - discounted return). Training state is not touched.
function dqn_evaluate(agent::DQNAgent; num_envs::Integer=256, episodes_per_env::Integer=1, seed::Integer=EVAL_SEED, trace_steps::Integer=0)
  report, returns, lengths, disc_returns, q0, trace_action = _value_evaluate(:dqn, "dqn_evaluate", agent.h, num_envs, episodes_per_env, 0, seed, trace_steps)
  return (; report, returns, lengths, disc_returns, q0, trace_action)
end

# dqn.jl:34 — same signature; `config` is the reference's DQNConfig (note its field `log_frequencey`, sic), `params` =
# vcat(vec.(Flux.params(q_net))...) of make_nn(env) (dqn.jl:22-26: 4 → 120 → 84 → 2, 10,934 parameters)
# dqn.jl:35 installs the logger, dqn.jl:39 builds q_net: `params` wins, else `init()` (inside the reference package its own make_nn(CartPoleEnv()),
# dqn.jl:22-26), else the library's initialiser (crl_dqn_init_params: the same glorot-uniform layers). Never the handle's zeros.
function _default_dqn_init()
  pm = parentmodule(@__MODULE__)
  (isdefined(pm, :make_nn) && isdefined(pm, :CartPoleEnv) && isdefined(pm, :Flux)) || return nothing
  () -> Vector{Float32}(vcat(vec.(getfield(pm, :Flux).params(getfield(pm, :make_nn)(getfield(pm, :CartPoleEnv)())))...))
end
function dqn(config; device=0, seed=UInt64(0x5EED), params::Union{Nothing,Vector{Float32}}=nothing, init=_default_dqn_init(), init_seed::Integer=0,
             chunk::Integer=10_000, make_logger=_default_make_logger(), eval_every::Integer=0, eval_envs::Integer=256, eval_episodes::Integer=1,
             per::Union{Nothing,PEROptions}=nothing, target::Union{Nothing,DQNTargetOptions}=nothing, dist::Union{Nothing,C51Options}=nothing,
             dueling::Bool=false, noisy::Union{Nothing,NoisyOptions}=nothing)
  eval_every >= 0 || throw(ArgumentError("dqn: eval_every must be >= 0, got $eval_every"))
  make_logger === nothing || make_logger("dqn|$(config.run_name)")         # dqn.jl:35
  cfg = CrlDQNConfig(config.log_frequencey, config.total_timesteps, config.buffer_size, config.min_buff_size, config.lr,
                     config.train_freq, config.target_net_freq, config.batch_size, config.gamma, config.epsilon_start,
                     config.epsilon_end, config.epsilon_duration, 200, 0, seed)
  h = Ref{Ptr{Cvoid}}(C_NULL)
  popt = per === nothing ? nothing :
         CrlDQNPEROptions(per.alpha, per.beta_start, per.beta_end, something(per.beta_duration, Float64(config.total_timesteps)), per.eps)
  if noisy !== nothing      # noisy linear layers (crl_dqn_noisy_create) on top of any of the kinds below. Like the rest of this file, never executed.
    0.0 <= noisy.sigma0 <= 10.0 || throw(ArgumentError("dqn: noisy.sigma0 must be in 0..10, got $(noisy.sigma0)"))
    nopt = Ref(CrlDQNNoisyOptions(noisy.sigma0))
    copt = dist === nothing ? C_NULL : Ref(CrlDQNC51Options(dist.n_atoms, 0, dist.v_min, dist.v_max))
    pref = popt === nothing ? C_NULL : Ref(popt)
    tref = target === nothing ? C_NULL : Ref(CrlDQNTargetOptions(target.n_step, target.double_q ? 1 : 0))
    GC.@preserve nopt copt pref tref check(ccall((:crl_dqn_noisy_create, libcrl), Int32,
      (Ref{CrlDQNConfig}, Ptr{Cvoid}, Int32, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ref{Ptr{Cvoid}}),
      cfg, Base.unsafe_convert(Ptr{Cvoid}, nopt), dueling ? 1 : 0, copt === C_NULL ? C_NULL : Base.unsafe_convert(Ptr{Cvoid}, copt),
      pref === C_NULL ? C_NULL : Base.unsafe_convert(Ptr{Cvoid}, pref), tref === C_NULL ? C_NULL : Base.unsafe_convert(Ptr{Cvoid}, tref), device, h))
  elseif dueling            # the dueling heads (Wang et al. 2016; crl_dqn_dueling_create), with either head (NULL = scalar), either replay and any target
                            # options: ten arrays, 20928 + 255·R parameters (crl_dqn_param_count). Like the rest of this file, never executed.
    copt = dist === nothing ? C_NULL : Ref(CrlDQNC51Options(dist.n_atoms, 0, dist.v_min, dist.v_max))
    pref = popt === nothing ? C_NULL : Ref(popt)
    tref = target === nothing ? C_NULL : Ref(CrlDQNTargetOptions(target.n_step, target.double_q ? 1 : 0))
    GC.@preserve copt pref tref check(ccall((:crl_dqn_dueling_create, libcrl), Int32, (Ref{CrlDQNConfig}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ref{Ptr{Cvoid}}),
      cfg, copt === C_NULL ? C_NULL : Base.unsafe_convert(Ptr{Cvoid}, copt), pref === C_NULL ? C_NULL : Base.unsafe_convert(Ptr{Cvoid}, pref),
      tref === C_NULL ? C_NULL : Base.unsafe_convert(Ptr{Cvoid}, tref), device, h))
  elseif dist !== nothing   # the categorical critic, with either replay and any target options (NULL = uniform, NULL = {1, 0})
    2 <= dist.n_atoms <= 64 || throw(ArgumentError("dqn: dist.n_atoms must be in 2..64, got $(dist.n_atoms)"))
    (isfinite(dist.v_min) && isfinite(dist.v_max) && dist.v_min < dist.v_max) || throw(ArgumentError("dqn: dist needs finite v_min < v_max"))
    target === nothing || 1 <= target.n_step <= 16 || throw(ArgumentError("dqn: target.n_step must be in 1..16, got $(target.n_step)"))
    copt = Ref(CrlDQNC51Options(dist.n_atoms, 0, dist.v_min, dist.v_max))
    pref = popt === nothing ? C_NULL : Ref(popt)
    tref = target === nothing ? C_NULL : Ref(CrlDQNTargetOptions(target.n_step, target.double_q ? 1 : 0))
    GC.@preserve copt pref tref check(ccall((:crl_dqn_c51_create, libcrl), Int32, (Ref{CrlDQNConfig}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ref{Ptr{Cvoid}}),
      cfg, Base.unsafe_convert(Ptr{Cvoid}, copt), pref === C_NULL ? C_NULL : Base.unsafe_convert(Ptr{Cvoid}, pref),
      tref === C_NULL ? C_NULL : Base.unsafe_convert(Ptr{Cvoid}, tref), device, h))
  elseif target !== nothing     # n-step / double-Q targets, uniform or prioritized replay (a NULL per is uniform); the library validates the options
    1 <= target.n_step <= 16 || throw(ArgumentError("dqn: target.n_step must be in 1..16, got $(target.n_step)"))
    topt = CrlDQNTargetOptions(target.n_step, target.double_q ? 1 : 0)
    if popt === nothing
      check(ccall((:crl_dqn_create_with, libcrl), Int32, (Ref{CrlDQNConfig}, Ptr{Cvoid}, Ref{CrlDQNTargetOptions}, Int32, Ref{Ptr{Cvoid}}),
                  cfg, C_NULL, topt, device, h))
    else
      check(ccall((:crl_dqn_create_with, libcrl), Int32, (Ref{CrlDQNConfig}, Ref{CrlDQNPEROptions}, Ref{CrlDQNTargetOptions}, Int32, Ref{Ptr{Cvoid}}),
                  cfg, popt, topt, device, h))
    end
  elseif popt === nothing
    check(ccall((:crl_dqn_create, libcrl), Int32, (Ref{CrlDQNConfig}, Int32, Ref{Ptr{Cvoid}}), cfg, device, h))
  else       # prioritized replay: the same handle type and the same calls from here on; the library validates the options
    check(ccall((:crl_dqn_per_create, libcrl), Int32, (Ref{CrlDQNConfig}, Ref{CrlDQNPEROptions}, Int32, Ref{Ptr{Cvoid}}), cfg, popt, device, h))
  end
  agent = DQNAgent(h[])
  finalizer(x -> ccall((:crl_dqn_destroy, libcrl), Int32, (Ptr{Cvoid},), x.h), agent)
  params === nothing && init !== nothing && dist === nothing && !dueling && noisy === nothing && (params = init())   # dqn.jl:39 make_nn(env); its head is the scalar one, so a C51
                                                                                    # agent without `params` takes the library's initialiser
  if params === nothing
    check(ccall((:crl_dqn_init_params, libcrl), Int32, (Ptr{Cvoid}, UInt64), agent.h, UInt64(init_seed)))
  else
    GC.@preserve params check(ccall((:crl_dqn_write_params, libcrl), Int32, (Ptr{Cvoid}, Ptr{Float32}, Csize_t), agent.h, params, length(params)))
  end
  eps = Vector{CrlDQNEpisode}(undef, 8192); losses = Vector{CrlDQNLossRecord}(undef, 4096)
  n_eps = Ref{Int32}(0); n_losses = Ref{Int32}(0); taken = Ref{Int64}(0)
  start_time = time(); global_step = 0
  while global_step < config.total_timesteps
    GC.@preserve eps losses check(ccall((:crl_dqn_run, libcrl), Int32,
      (Ptr{Cvoid}, Int64, Ptr{CrlDQNEpisode}, Int32, Ref{Int32}, Ptr{CrlDQNLossRecord}, Int32, Ref{Int32}, Ref{Int64}),
      agent.h, eval_every > 0 ? min(chunk, eval_every - global_step % eval_every) : chunk, eps, length(eps), n_eps, losses, length(losses), n_losses, taken))
    taken[] == 0 && break
    global_step += taken[]
    for e in @view eps[1:n_eps[]]
      steps_per_sec = trunc(e.global_step / (time() - start_time))
      @info "Episode Statistics" episode_return = e.episode_return episode_length = e.episode_length global_step = e.global_step steps_per_sec ϵ = e.epsilon
    end
    for l in @view losses[1:n_losses[]]
      if popt === nothing
        @info "Training Statistics" loss = l.loss global_step = l.global_step
      else
        @info "Training Statistics" loss = l.loss beta = _per_beta(popt, l.global_step) global_step = l.global_step
      end
    end
    if eval_every > 0 && global_step % eval_every == 0           # "Evaluation Statistics" after the records of that step; the calls are cut there
      ev = dqn_evaluate(agent; num_envs=eval_envs, episodes_per_env=eval_episodes).report
      @info "Evaluation Statistics" eval_return_mean = ev.return_mean eval_return_std = ev.return_std eval_q_bias = ev.v_bias_mean global_step
    end
  end
  agent
end

# ------------------------------------------------------------------------------------------------------
# ddpg.jl — same names: DDPGConfig keeps the reference's fields (ddpg.jl:1-15); the loop body runs on the GPU, the env is the library's
# Pendulum (`ddpg`) or any Julia env the caller steps (`ddpg_external`: the reference's own is GymEnv("HalfCheetah-v3"), ddpg.jl:50)
# ------------------------------------------------------------------------------------------------------
struct CrlDDPGConfig      # include/cleanrl_hip.h crl_ddpg_config
  total_timesteps::Int64; buffer_size::Int64; min_buff_size::Int64; batch_size::Int64; warmup_steps::Int64; log_frequency::Int64
  lr::Float64; tau::Float64; gamma::Float64; exploration_noise::Float64
  obs_dim::Int32; act_dim::Int32; env_kind::Int32; max_steps::Int32
  act_low::Float64; act_high::Float64
  noise_in_update::Int32; pad::Int32
  seed::UInt64
end
struct CrlDDPGEpisode; episode_return::Float64; episode_length::Int64; global_step::Int64; end                  # ddpg.jl:97
struct CrlDDPGLossRecord; global_step::Int64; actor_loss::Float64; critic_loss::Float64; end                    # ddpg.jl:132
struct CrlSACAlphaRecord; global_step::Int64; alpha::Float64; alpha_loss::Float64; entropy::Float64; end   # crl_sac_alpha_record: beside each loss record of a SAC handle; here, above _log_training's ccall that names it
struct CrlDDPGStatus
  theta::Float64; theta_dot::Float64
  env_t::Int64; global_step::Int64; rb_size::Int64; rb_ptr::Int64; n_updates::Int64
  actor_loss::Float64; critic_loss::Float64
end
struct CrlDDPGEvalConfig  # crl_ddpg_eval_config: what crl_ddpg_evaluate runs
  num_envs::Int32; episodes_per_env::Int32; trace_steps::Int32; pad::Int32; seed::UInt64
end
struct CrlDDPGEvalReport  # crl_ddpg_eval_report: Float64 summary of the per-episode arrays (population standard deviation; q_bias_mean = mean(q0 - disc_return))
  episodes::Int64; env_steps::Int64
  return_mean::Float64; return_std::Float64; return_min::Float64; return_max::Float64; disc_return_mean::Float64; q0_mean::Float64; q_bias_mean::Float64
end
const DDPG_ENV_PENDULUM = Int32(0)
const DDPG_ENV_EXTERNAL = Int32(1)

mutable struct DDPGAgent
  h::Ptr{Cvoid}
  obs_dim::Int
  act_dim::Int
end

# The package's own builder: make_ddpg_nn(env, exploration_noise) (ddpg.jl:19-37) flattened in Flux.params order — the noise closure at the end
# of the actor Chain has no parameters. It needs the caller's env (ddpg.jl:20-21 read its spaces), so it is handed over as
#   init = () -> reference_ddpg_params(CleanRL.make_ddpg_nn, CleanRL.Flux, env, config.exploration_noise)
# and the default is the library's restatement of the same glorot layers (crl_ddpg_init_params).
function reference_ddpg_params(make_ddpg_nn, Flux, env, exploration_noise::Float64)
  actor, critic = make_ddpg_nn(env, exploration_noise)
  (Vector{Float32}(vcat(vec.(Flux.params(actor))...)), Vector{Float32}(vcat(vec.(Flux.params(critic))...)))
end
_default_ddpg_init() = nothing

# ddpg.jl:52-54: `params` = (vcat(vec.(Flux.params(actor))...), vcat(vec.(Flux.params(critic))...)) wins, else `init()` (e.g. the package's
# make_ddpg_nn flattened), else the library's initialiser (crl_ddpg_init_params). Never the handle's zeros.
function _ddpg_start!(config, obs_dim, act_dim, env_kind, act_low, act_high, max_steps, noise_in_update, device, seed, params, init, init_seed)
  cfg = CrlDDPGConfig(config.total_timesteps, config.buffer_size, config.min_buff_size, config.batch_size, config.warmup_steps,
                      config.log_frequencey, config.lr, config.tau, config.gamma, config.exploration_noise, obs_dim, act_dim, env_kind,
                      max_steps, act_low, act_high, noise_in_update ? 1 : 0, 0, seed)
  h = Ref{Ptr{Cvoid}}(C_NULL)
  check(ccall((:crl_ddpg_create, libcrl), Int32, (Ref{CrlDDPGConfig}, Int32, Ref{Ptr{Cvoid}}), cfg, device, h))
  agent = DDPGAgent(h[], obs_dim, act_dim)
  finalizer(x -> ccall((:crl_ddpg_destroy, libcrl), Int32, (Ptr{Cvoid},), x.h), agent)
  params === nothing && init !== nothing && (params = init())             # ddpg.jl:52 make_ddpg_nn(env, exploration_noise)
  if params === nothing
    check(ccall((:crl_ddpg_init_params, libcrl), Int32, (Ptr{Cvoid}, UInt64), agent.h, UInt64(init_seed)))
  else
    actor, critic = params
    GC.@preserve actor critic check(ccall((:crl_ddpg_write_params, libcrl), Int32, (Ptr{Cvoid}, Ptr{Float32}, Csize_t, Ptr{Float32}, Csize_t),
                                          agent.h, actor, length(actor), critic, length(critic)))
  end
  agent
end

# the noise-free actor output 2·tanh_fast(·) for observations (obs_dim, n) → (act_dim, n)
function actor_mean(agent::DDPGAgent, obs::AbstractMatrix{Float64})
  o = Array(obs); n = size(o, 2); out = Matrix{Float64}(undef, agent.act_dim, n)
  GC.@preserve o out check(ccall((:crl_ddpg_actor, libcrl), Int32, (Ptr{Cvoid}, Ptr{Float64}, Int32, Ptr{Float64}), agent.h, o, n, out))
  out
end
# get_q(critic, obs, act) (ddpg.jl:45)
function get_q(agent::DDPGAgent, obs::AbstractMatrix{Float64}, act::AbstractMatrix{Float64})
  o = Array(obs); a = Array(act); n = size(o, 2); q = Vector{Float64}(undef, n)
  GC.@preserve o a q check(ccall((:crl_ddpg_q_values, libcrl), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int32, Ptr{Float64}), agent.h, o, a, n, q))
  q
end

# How good is the current actor, and does the critic over-estimate? crl_ddpg_evaluate: the agent's actor, frozen and WITHOUT the exploration noise
# (ddpg.jl:28 puts it inside the actor, so the reference's "Episode Statistics" score the noisy behaviour policy), plays episodes_per_env whole
# episodes on each of num_envs fresh on-device Pendulums in one launch; training state is not touched. returns / disc_returns / q0 are
# (num_envs, episodes_per_env) — the C arrays are env-fastest —, q0 = Q(s0, actor(s0)), report.q_bias_mean = mean(q0 - discounted return);
# trace_action (num_envs, trace_steps) holds the actions of each env's first trace_steps steps. An agent of ddpg_external has its env in the
# caller's process: the library refuses it here — step that env and take the actions from actor_mean.
function ddpg_evaluate(agent::DDPGAgent; num_envs::Integer=256, episodes_per_env::Integer=1, seed::Integer=EVAL_SEED, trace_steps::Integer=0)
  1 <= num_envs <= 65536 || throw(ArgumentError("ddpg_evaluate: num_envs must be in 1..65536, got $num_envs"))
  1 <= episodes_per_env <= 1024 || throw(ArgumentError("ddpg_evaluate: episodes_per_env must be in 1..1024, got $episodes_per_env"))
  trace_steps >= 0 || throw(ArgumentError("ddpg_evaluate: trace_steps must be >= 0, got $trace_steps"))
  cfg = Ref(CrlDDPGEvalConfig(num_envs, episodes_per_env, trace_steps, 0, UInt64(seed)))
  report = Ref{CrlDDPGEvalReport}()
  returns = Matrix{Float64}(undef, num_envs, episodes_per_env); disc_returns = similar(returns); q0 = similar(returns)
  trace_action = Matrix{Float64}(undef, num_envs, trace_steps)
  GC.@preserve returns disc_returns q0 trace_action check(ccall((:crl_ddpg_evaluate, libcrl), Int32,
    (Ptr{Cvoid}, Ref{CrlDDPGEvalConfig}, Ref{CrlDDPGEvalReport}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
    agent.h, cfg, report, returns, disc_returns, q0, trace_steps > 0 ? pointer(trace_action) : Ptr{Float64}(C_NULL)))
  return (; report = report[], returns, disc_returns, q0, trace_action)
end

# ddpg.jl:47 on the library's Pendulum (obs 3, act 1, torque ±2, 200-step episodes). eval_every = N > 0: an "Evaluation Statistics" record
# (eval_return_mean, eval_return_std, eval_q_bias, global_step) after the records of every step that is a multiple of N — the calls are cut there
function ddpg(config; device=0, seed=UInt64(0x5EED), params=nothing, init=_default_ddpg_init(), init_seed::Integer=0, chunk::Integer=4096,
              noise_in_update::Bool=true, make_logger=_default_make_logger(), eval_every::Integer=0, eval_envs::Integer=256, eval_episodes::Integer=1)
  eval_every >= 0 || throw(ArgumentError("ddpg: eval_every must be >= 0, got $eval_every"))
  make_logger === nothing || make_logger("ddpg|$(config.run_name)")        # ddpg.jl:48
  agent = _ddpg_start!(config, 3, 1, DDPG_ENV_PENDULUM, -2.0, 2.0, 200, noise_in_update, device, seed, params, init, init_seed)
  _ddpg_run!(agent, config, chunk, eval_every, eval_envs, eval_episodes)
end
# the "Training Statistics" records of the loss records a crl_ddpg_run / crl_ddpg_read_losses call just returned; sac: with the alpha records beside them
function _log_training(agent, losses, n, sac::Bool)
  if !sac
    for l in @view losses[1:n]
      @info "Training Statistics" actor_loss = l.actor_loss critic_loss = l.critic_loss
    end
    return
  end
  recs = Vector{CrlSACAlphaRecord}(undef, max(n, 1)); n_recs = Ref{Int32}(0)
  GC.@preserve recs check(ccall((:crl_sac_alpha_records, libcrl), Int32, (Ptr{Cvoid}, Ptr{CrlSACAlphaRecord}, Int32, Ref{Int32}), agent.h, recs, n, n_recs))
  n_recs[] == n || error("crl_sac_alpha_records: $(n_recs[]) records for $n loss records")
  for (l, r) in zip(@view(losses[1:n]), @view(recs[1:n]))
    @info "Training Statistics" actor_loss = l.actor_loss critic_loss = l.critic_loss alpha = r.alpha alpha_loss = r.alpha_loss entropy = r.entropy
  end
end

# the loop of ddpg() on a started agent (td3() and sac() run it too): one crl_ddpg_run per chunk, the records of ddpg.jl:97 / :132 after each
function _ddpg_run!(agent::DDPGAgent, config, chunk, eval_every, eval_envs, eval_episodes; sac::Bool=false)
  eps = Vector{CrlDDPGEpisode}(undef, 8192); losses = Vector{CrlDDPGLossRecord}(undef, 4096)
  n_eps = Ref{Int32}(0); n_losses = Ref{Int32}(0); taken = Ref{Int64}(0)
  start_time = time(); global_step = 0
  while global_step < config.total_timesteps
    budget = eval_every > 0 ? min(chunk, eval_every - global_step % eval_every) : chunk
    GC.@preserve eps losses check(ccall((:crl_ddpg_run, libcrl), Int32,
      (Ptr{Cvoid}, Int64, Ptr{CrlDDPGEpisode}, Int32, Ref{Int32}, Ptr{CrlDDPGLossRecord}, Int32, Ref{Int32}, Ref{Int64}),
      agent.h, budget, eps, length(eps), n_eps, losses, length(losses), n_losses, taken))
    taken[] == 0 && break
    global_step += taken[]
    for e in @view eps[1:n_eps[]]
      steps_per_sec = trunc(e.global_step / (time() - start_time))
      @info "Episode Statistics" episode_return = e.episode_return episode_length = e.episode_length steps_per_sec global_step = e.global_step
    end
    _log_training(agent, losses, n_losses[], sac)
    if eval_every > 0 && global_step % eval_every == 0
      ev = ddpg_evaluate(agent; num_envs=eval_envs, episodes_per_env=eval_episodes).report
      @info "Evaluation Statistics" eval_return_mean = ev.return_mean eval_return_std = ev.return_std eval_q_bias = ev.q_bias_mean global_step
    end
  end
  agent
end

# ddpg.jl:47 with the env in the caller's process. `env` is driven through three closures-or-methods the caller supplies:
#   reset_env!(env) -> obs::Vector{Float64},  step_env!(env, action::Vector{Float64}) -> (reward, next_obs::Vector{Float64}, terminal::Bool)
# (for a ReinforcementLearning.jl env: env -> (reset!(env); state(env)) and (env, a) -> (env(a); (reward(env), state(env), is_terminated(env)))).
function ddpg_external(config, env; obs_dim::Integer, act_dim::Integer, act_low::Real, act_high::Real, reset_env!, step_env!, device=0,
                       seed=UInt64(0x5EED), params=nothing, init=_default_ddpg_init(), init_seed::Integer=0, noise_in_update::Bool=true,
                       make_logger=_default_make_logger())
  make_logger === nothing || make_logger("ddpg|$(config.run_name)")        # ddpg.jl:48
  agent = _ddpg_start!(config, obs_dim, act_dim, DDPG_ENV_EXTERNAL, Float64(act_low), Float64(act_high), 200, noise_in_update, device, seed, params,
                       init, init_seed)
  _ddpg_run_external!(agent, config, env, act_dim, reset_env!, step_env!)
end
# the loop of ddpg_external() on a started agent (td3_external() and sac_external() run it too)
function _ddpg_run_external!(agent::DDPGAgent, config, env, act_dim, reset_env!, step_env!; sac::Bool=false)
  action = Vector{Float64}(undef, act_dim); losses = Vector{CrlDDPGLossRecord}(undef, 4096); n_losses = Ref{Int32}(0)
  episode_return = 0.0; episode_length = 0
  start_time = time()
  obs = Vector{Float64}(reset_env!(env))                                   # ddpg.jl:74
  for global_step in 1:config.total_timesteps
    GC.@preserve obs action check(ccall((:crl_ddpg_act, libcrl), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), agent.h, obs, action))   # :79
    reward, next_obs, terminal = step_env!(env, copy(action))              # :80
    next_obs = Vector{Float64}(next_obs)
    GC.@preserve obs action next_obs check(ccall((:crl_ddpg_observe, libcrl), Int32,
      (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Float64, Ptr{Float64}, Int32), agent.h, obs, action, Float64(reward), next_obs, terminal ? 1 : 0))   # :83-90, 105-129
    episode_return += reward; episode_length += 1                          # :93-94
    obs = next_obs
    if terminal                                                            # :95-101
      steps_per_sec = trunc(global_step / (time() - start_time))
      @info "Episode Statistics" episode_return episode_length steps_per_sec global_step
      episode_length, episode_return = 0, 0.0
      obs = Vector{Float64}(reset_env!(env))
    end
    if global_step % config.log_frequencey == 0                            # :131-133
      GC.@preserve losses check(ccall((:crl_ddpg_read_losses, libcrl), Int32, (Ptr{Cvoid}, Ptr{CrlDDPGLossRecord}, Int32, Ref{Int32}),
                                      agent.h, losses, length(losses), n_losses))
      _log_training(agent, losses, n_losses[], sac)
    end
  end
  agent
end

# ------------------------------------------------------------------------------------------------------
# TD3 (Fujimoto et al. 2018) on the same handle — the reference has no TD3. `config` carries DDPGConfig's fields plus policy_delay, policy_noise
# and noise_clip (defaults of the paper: 2, 0.2, 0.5); the agent is a DDPGAgent: actor_mean, get_q (critic 1) and ddpg_evaluate (q0 = critic 1) serve it.
# ------------------------------------------------------------------------------------------------------
struct CrlTD3Options      # include/cleanrl_hip.h crl_td3_options
  policy_delay::Int32; pad::Int32; policy_noise::Float64; noise_clip::Float64
end

# `params` = (actor, critic1, critic2) flat in Flux.params order wins, else the library's initialiser (crl_td3_init_params: make_ddpg_nn's glorot
# layers, critic 2 from a second draw). Never the handle's zeros.
function _td3_start!(config, obs_dim, act_dim, env_kind, act_low, act_high, max_steps, device, seed, params, init_seed)
  cfg = CrlDDPGConfig(config.total_timesteps, config.buffer_size, config.min_buff_size, config.batch_size, config.warmup_steps,
                      config.log_frequencey, config.lr, config.tau, config.gamma, config.exploration_noise, obs_dim, act_dim, env_kind,
                      max_steps, act_low, act_high, 0, 0, seed)
  opt = CrlTD3Options(config.policy_delay, 0, config.policy_noise, config.noise_clip)
  h = Ref{Ptr{Cvoid}}(C_NULL)
  check(ccall((:crl_td3_create, libcrl), Int32, (Ref{CrlDDPGConfig}, Ref{CrlTD3Options}, Int32, Ref{Ptr{Cvoid}}), cfg, opt, device, h))
  agent = DDPGAgent(h[], obs_dim, act_dim)
  finalizer(x -> ccall((:crl_ddpg_destroy, libcrl), Int32, (Ptr{Cvoid},), x.h), agent)
  if params === nothing
    check(ccall((:crl_td3_init_params, libcrl), Int32, (Ptr{Cvoid}, UInt64), agent.h, UInt64(init_seed)))
  else
    actor, critic1, critic2 = params
    GC.@preserve actor critic1 critic2 check(ccall((:crl_td3_write_params, libcrl), Int32,
      (Ptr{Cvoid}, Ptr{Float32}, Csize_t, Ptr{Float32}, Csize_t, Ptr{Float32}, Csize_t),
      agent.h, actor, length(actor), critic1, length(critic1), critic2, length(critic2)))
  end
  agent
end

# (Q_1, Q_2) of a td3 agent for (obs_dim, n), (act_dim, n)
function get_q_both(agent::DDPGAgent, obs::AbstractMatrix{Float64}, act::AbstractMatrix{Float64})
  o = Array(obs); a = Array(act); n = size(o, 2); q1 = Vector{Float64}(undef, n); q2 = Vector{Float64}(undef, n)
  GC.@preserve o a q1 q2 check(ccall((:crl_td3_q_values, libcrl), Int32, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int32, Ptr{Float64}, Ptr{Float64}),
                                     agent.h, o, a, n, q1, q2))
  (q1, q2)
end

# ddpg()'s loop and records with TD3's update, on the library's Pendulum
function td3(config; device=0, seed=UInt64(0x5EED), params=nothing, init_seed::Integer=0, chunk::Integer=4096, make_logger=_default_make_logger(),
             eval_every::Integer=0, eval_envs::Integer=256, eval_episodes::Integer=1)
  eval_every >= 0 || throw(ArgumentError("td3: eval_every must be >= 0, got $eval_every"))
  make_logger === nothing || make_logger("td3|$(config.run_name)")
  agent = _td3_start!(config, 3, 1, DDPG_ENV_PENDULUM, -2.0, 2.0, 200, device, seed, params, init_seed)
  _ddpg_run!(agent, config, chunk, eval_every, eval_envs, eval_episodes)
end

# ddpg_external()'s loop with TD3's update: the env lives in the caller's process (reset_env! / step_env! as there)
function td3_external(config, env; obs_dim::Integer, act_dim::Integer, act_low::Real, act_high::Real, reset_env!, step_env!, device=0,
                      seed=UInt64(0x5EED), params=nothing, init_seed::Integer=0, make_logger=_default_make_logger())
  make_logger === nothing || make_logger("td3|$(config.run_name)")
  agent = _td3_start!(config, obs_dim, act_dim, DDPG_ENV_EXTERNAL, Float64(act_low), Float64(act_high), 200, device, seed, params, init_seed)
  _ddpg_run_external!(agent, config, env, act_dim, reset_env!, step_env!)
end

# ------------------------------------------------------------------------------------------------------
# SAC (Haarnoja et al. 2018) on the same handle — the reference lists it as a to-do. `config` carries DDPGConfig's fields (exploration_noise is not
# read) plus autotune::Bool, alpha and target_entropy (`nothing`: -act_dim); the agent is a DDPGAgent: actor_mean (the deterministic action
# scale·tanh(μ) + bias), get_q (critic 1) and ddpg_evaluate (q0 = critic 1) serve it. "Training Statistics" carry alpha, alpha_loss and entropy.
# ------------------------------------------------------------------------------------------------------
struct CrlSACOptions      # include/cleanrl_hip.h crl_sac_options
  autotune::Int32; pad::Int32; alpha::Float64; target_entropy::Float64
end
struct CrlSACStatus       # crl_sac_status
  alpha::Float64; alpha_loss::Float64; entropy::Float64; log_alpha::Float32; pad::Int32
end

# `params` = (actor, critic1, critic2) flat in Flux.params order (the actor's head has 2·act_dim rows) wins, else crl_sac_init_params
function _sac_start!(config, obs_dim, act_dim, env_kind, act_low, act_high, max_steps, device, seed, params, init_seed)
  cfg = CrlDDPGConfig(config.total_timesteps, config.buffer_size, config.min_buff_size, config.batch_size, config.warmup_steps,
                      config.log_frequencey, config.lr, config.tau, config.gamma, config.exploration_noise, obs_dim, act_dim, env_kind,
                      max_steps, act_low, act_high, 0, 0, seed)
  target_entropy = config.target_entropy === nothing ? -Float64(act_dim) : Float64(config.target_entropy)
  opt = CrlSACOptions(config.autotune ? 1 : 0, 0, config.alpha, target_entropy)
  h = Ref{Ptr{Cvoid}}(C_NULL)
  check(ccall((:crl_sac_create, libcrl), Int32, (Ref{CrlDDPGConfig}, Ref{CrlSACOptions}, Int32, Ref{Ptr{Cvoid}}), cfg, opt, device, h))
  agent = DDPGAgent(h[], obs_dim, act_dim)
  finalizer(x -> ccall((:crl_ddpg_destroy, libcrl), Int32, (Ptr{Cvoid},), x.h), agent)
  if params === nothing
    check(ccall((:crl_sac_init_params, libcrl), Int32, (Ptr{Cvoid}, UInt64), agent.h, UInt64(init_seed)))
  else
    actor, critic1, critic2 = params
    GC.@preserve actor critic1 critic2 check(ccall((:crl_sac_write_params, libcrl), Int32,
      (Ptr{Cvoid}, Ptr{Float32}, Csize_t, Ptr{Float32}, Csize_t, Ptr{Float32}, Csize_t),
      agent.h, actor, length(actor), critic1, length(critic1), critic2, length(critic2)))
  end
  agent
end

# (alpha, alpha_loss, entropy) of the last update and log_alpha as it stands
function sac_status(agent::DDPGAgent)
  st = Ref(CrlSACStatus(0.0, 0.0, 0.0, 0.0f0, 0))
  check(ccall((:crl_sac_status_read, libcrl), Int32, (Ptr{Cvoid}, Ref{CrlSACStatus}), agent.h, st))
  (alpha = st[].alpha, alpha_loss = st[].alpha_loss, entropy = st[].entropy, log_alpha = st[].log_alpha)
end

# ddpg()'s loop and records with SAC's update, on the library's Pendulum
function sac(config; device=0, seed=UInt64(0x5EED), params=nothing, init_seed::Integer=0, chunk::Integer=4096, make_logger=_default_make_logger(),
             eval_every::Integer=0, eval_envs::Integer=256, eval_episodes::Integer=1)
  eval_every >= 0 || throw(ArgumentError("sac: eval_every must be >= 0, got $eval_every"))
  make_logger === nothing || make_logger("sac|$(config.run_name)")
  agent = _sac_start!(config, 3, 1, DDPG_ENV_PENDULUM, -2.0, 2.0, 200, device, seed, params, init_seed)
  _ddpg_run!(agent, config, chunk, eval_every, eval_envs, eval_episodes; sac=true)
end

# ddpg_external()'s loop with SAC's update: the env lives in the caller's process (reset_env! / step_env! as there)
function sac_external(config, env; obs_dim::Integer, act_dim::Integer, act_low::Real, act_high::Real, reset_env!, step_env!, device=0,
                      seed=UInt64(0x5EED), params=nothing, init_seed::Integer=0, make_logger=_default_make_logger())
  make_logger === nothing || make_logger("sac|$(config.run_name)")
  agent = _sac_start!(config, obs_dim, act_dim, DDPG_ENV_EXTERNAL, Float64(act_low), Float64(act_high), 200, device, seed, params, init_seed)
  _ddpg_run_external!(agent, config, env, act_dim, reset_env!, step_env!; sac=true)
end

end # module
