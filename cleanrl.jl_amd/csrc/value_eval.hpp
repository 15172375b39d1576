// value_eval.hpp — what crl_dqn_evaluate (dqn.hip) and crl_a2c_evaluate (a2c.hip) share: the kernel arguments, the argument checks, the device
// scratch layout and the Float64 report on the host (include/cleanrl_hip.h, crl_value_eval_report). The two step loops themselves differ only in the
// network, so they live beside their networks; the tail of a finished env (its trace rows) is stated here once for both.
#pragma once
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "common.hpp"
#include "ppo_ctx.hpp"

namespace crl {

constexpr uint32_t S_VEVAL_RESET = 0x20, S_VEVAL_DRAW = 0x21;   // Philox streams "evaluation reset" / "evaluation draw" (loops: 0, 1, 2, 4; DDPG: 0x10–0x16)

struct ValueEvalArgs {
  int32_t n, episodes, trace_steps, mode; uint64_t seed;
  double *ret, *disc_ret, *v0;        // [episodes][n] each
  int32_t *len, *trace;               // [episodes][n], [trace_steps][n]
};

// rows of the trace an env no longer reaches once its quota is played: −1, written by the whole wave
__device__ __forceinline__ void value_eval_trace_tail(const ValueEvalArgs& ev, int env, int64_t row, int lane) {
  for (int64_t r = row + lane; r < ev.trace_steps; r += 64) ev.trace[(size_t)r * ev.n + env] = -1;
}

struct ValueEvalScratch { void* p = nullptr; size_t bytes = 0; };

// argument checks of crl_*_evaluate after the handle guard; `who` names the call in every message
inline int value_eval_check(const char* who, const crl_eval_config* cfg, const crl_value_eval_report* report, bool params_set, const char* how_to_set,
                            int max_steps, bool has_sampler, const int32_t* trace_action) {
  const std::string w(who);
  if (!cfg || !report) { set_error(w + ": null cfg or report"); return 1; }
  if (!params_set) { set_error(w + ": parameters not set — " + how_to_set); return 1; }
  const int64_t n = cfg->num_envs, E = cfg->episodes_per_env, T = cfg->trace_steps, steps = E * ((int64_t)max_steps + 1);
  if (n < 1 || n > 65536) { set_error(w + ": num_envs must be in 1..65536, got " + std::to_string(n)); return 1; }
  if (E < 1 || E > 1024) { set_error(w + ": episodes_per_env must be in 1..1024, got " + std::to_string(E)); return 1; }
  if (n * E > (1 << 20)) { set_error(w + ": num_envs * episodes_per_env must be <= 1048576, got " + std::to_string(n * E)); return 1; }
  if (cfg->mode != CRL_EVAL_GREEDY && cfg->mode != CRL_EVAL_SAMPLE) {
    set_error(w + ": mode must be CRL_EVAL_GREEDY (0) or CRL_EVAL_SAMPLE (1), got " + std::to_string(cfg->mode)); return 1;
  }
  if (cfg->mode == CRL_EVAL_SAMPLE && !has_sampler) {
    set_error(w + ": mode CRL_EVAL_SAMPLE — DQN has no sampling policy (its ε-greedy exploration is not a policy to score); use CRL_EVAL_GREEDY"); return 1;
  }
  if (T < 0 || T > steps) {
    set_error(w + ": trace_steps must be in 0..episodes_per_env * (max_steps + 1) = " + std::to_string(steps) + ", got " + std::to_string(T)); return 1;
  }
  if ((T > 0) != (trace_action != nullptr)) { set_error(w + ": trace_action must be given exactly when trace_steps > 0"); return 1; }
  if (T * n > (1 << 24)) { set_error(w + ": trace_steps * num_envs must be <= 16777216, got " + std::to_string(T * n)); return 1; }
  return 0;
}

// device scratch, grown on demand and kept on the handle: three double arrays, then the lengths, then the trace
inline int value_eval_scratch(ValueEvalScratch& s, const crl_eval_config* cfg, ValueEvalArgs& ev) {
  const size_t ne = (size_t)cfg->num_envs * (size_t)cfg->episodes_per_env, nt = (size_t)cfg->trace_steps * (size_t)cfg->num_envs;
  const size_t need = 3 * ne * 8 + (ne + nt) * 4;
  if (s.bytes < need) {
    if (s.p) CRL_HIP_CHECK(hipFree(s.p));
    s.p = nullptr; s.bytes = 0;
    CRL_HIP_CHECK(hipMalloc(&s.p, need));
    s.bytes = need;
  }
  ev.n = cfg->num_envs; ev.episodes = cfg->episodes_per_env; ev.trace_steps = cfg->trace_steps; ev.mode = cfg->mode; ev.seed = cfg->seed;
  ev.ret = static_cast<double*>(s.p); ev.disc_ret = ev.ret + ne; ev.v0 = ev.disc_ret + ne;
  ev.len = reinterpret_cast<int32_t*>(ev.v0 + ne); ev.trace = ev.len + ne;
  return 0;
}

// after the launch: the arrays back to the host (synchronises), the report in Float64 with sums in array order, the caller's copies
inline int value_eval_finish(hipStream_t st, const ValueEvalArgs& ev, crl_value_eval_report* report, double* returns, int32_t* lengths,
                             double* disc_returns, double* v0, int32_t* trace_action) {
#pragma clang fp contract(off)
  const size_t ne = (size_t)ev.n * (size_t)ev.episodes, nt = (size_t)ev.trace_steps * (size_t)ev.n;
  std::vector<double> host(3 * ne);
  std::vector<int32_t> len(ne);
  CRL_HIP_CHECK(hipMemcpyAsync(host.data(), ev.ret, 3 * ne * 8, hipMemcpyDeviceToHost, st));
  CRL_HIP_CHECK(hipMemcpyAsync(len.data(), ev.len, ne * 4, hipMemcpyDeviceToHost, st));
  if (nt > 0) CRL_HIP_CHECK(hipMemcpyAsync(trace_action, ev.trace, nt * 4, hipMemcpyDeviceToHost, st));
  CRL_HIP_CHECK(hipStreamSynchronize(st));   // host buffers are only borrowed for the call
  const double *ret = host.data(), *disc = ret + ne, *v = disc + ne;
  double rsum = 0.0, dsum = 0.0, vsum = 0.0, bsum = 0.0, lsum = 0.0, rmin = ret[0], rmax = ret[0];
  int64_t steps = 0;
  for (size_t i = 0; i < ne; ++i) {
    rsum += ret[i]; dsum += disc[i]; vsum += v[i]; bsum += v[i] - disc[i]; lsum += (double)len[i]; steps += len[i];
    rmin = ret[i] < rmin ? ret[i] : rmin; rmax = ret[i] > rmax ? ret[i] : rmax;
  }
  const double mean = rsum / (double)ne;
  double var = 0.0;
  for (size_t i = 0; i < ne; ++i) { const double d = ret[i] - mean; var += d * d; }
  report->episodes = (int64_t)ne; report->env_steps = steps;
  report->return_mean = mean; report->return_std = std::sqrt(var / (double)ne); report->return_min = rmin; report->return_max = rmax;
  report->length_mean = lsum / (double)ne; report->disc_return_mean = dsum / (double)ne;
  report->v0_mean = vsum / (double)ne; report->v_bias_mean = bsum / (double)ne;
  if (returns) memcpy(returns, ret, ne * 8);
  if (lengths) memcpy(lengths, len.data(), ne * 4);
  if (disc_returns) memcpy(disc_returns, disc, ne * 8);
  if (v0) memcpy(v0, v, ne * 8);
  return 0;
}

}  // namespace crl
