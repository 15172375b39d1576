// init.cpp — host-side network initialisers: what `Networks.make_actor_critic` (networks.jl:36-49, called at ppo.jl:87 and a2c.jl:37) and
// `make_nn` (dqn.jl:22-26) leave in the Flux layers, as ONE flat float vector in Flux.params order. Run once per handle, on the host:
// 9,155 / 137,477 / 10,934 numbers — nothing for a kernel to win. They exist so that NO entry point of the boundary can train the all-zero
// network a fresh handle holds: a caller either uploads the reference's own `Flux.params` (crl_ppo_write(CRL_F_PARAMS)) or asks for this
// reference-shaped start; anything that computes with unset parameters is an error (api.cpp: params_set).
//
// [3P-memory, Flux 0.13.4] `Flux.orthogonal(rng, rows, cols; gain)`: rows < cols → the transpose of orthogonal(cols, rows);
// otherwise mat = randn(Float32, rows, cols); Q, R = qr(mat); Q · sign.(Diagonal(R)) · gain. `Dense(in => out; init)` has a zero bias.
// `Flux.glorot_uniform(out, in)` = (rand(Float32, out, in) .- 0.5) .* 2·sqrt(6 / (in + out)) — the default init of the DQN layers.
// The random STREAM is this library's own (splitmix64 + Box–Muller): Flux draws from Julia's task-local Xoshiro, which nobody outside
// Julia reproduces; the DISTRIBUTION (Haar-orthogonal columns times the gain, zero biases) is the reference's.
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/cleanrl_hip.h"

namespace crl {
void set_error(const std::string& msg);

namespace {
struct Rng {
  uint64_t s;
  uint64_t next() {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  double uniform() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }   // [0, 1)
  double normal() {
    double u1 = uniform(), u2 = uniform();
    if (u1 < 1e-300) u1 = 1e-300;
    return std::sqrt(-2.0 * std::log(u1)) * std::cos(6.283185307179586 * u2);
  }
};

// W (rows, cols) column-major = gain · (Haar-orthogonal): Gaussian (n, m) with n = max, m = min, columns orthonormalised by modified
// Gram–Schmidt run twice (the second pass removes what rounding left) — the Q of the QR factorisation whose R has a positive diagonal,
// i.e. Householder's Q · sign(diag R) — transposed when rows < cols.
void orthogonal(Rng& rng, int rows, int cols, double gain, float* out) {
  const int n = rows > cols ? rows : cols, m = rows > cols ? cols : rows;
  std::vector<double> a((size_t)n * m);
  for (double& x : a) x = rng.normal();
  for (int j = 0; j < m; ++j) {
    double* cj = &a[(size_t)j * n];
    for (int pass = 0; pass < 2; ++pass)
      for (int i = 0; i < j; ++i) {
        const double* ci = &a[(size_t)i * n];
        double d = 0.0;
        for (int r = 0; r < n; ++r) d += ci[r] * cj[r];
        for (int r = 0; r < n; ++r) cj[r] -= d * ci[r];
      }
    double nn = 0.0;
    for (int r = 0; r < n; ++r) nn += cj[r] * cj[r];
    nn = std::sqrt(nn);
    for (int r = 0; r < n; ++r) cj[r] /= nn;
  }
  for (int c = 0; c < cols; ++c)
    for (int r = 0; r < rows; ++r)
      out[(size_t)c * rows + r] = (float)(gain * (rows >= cols ? a[(size_t)c * n + r] : a[(size_t)r * n + c]));
}

void glorot_uniform(Rng& rng, int out_dim, int in_dim, float* out) {
  const double s = 2.0 * std::sqrt(6.0 / (double)(in_dim + out_dim));
  for (size_t i = 0; i < (size_t)out_dim * in_dim; ++i) out[i] = (float)((rng.uniform() - 0.5) * s);
}
}  // namespace
}  // namespace crl

using crl::set_error;

extern "C" {

int32_t crl_make_actor_critic(int32_t obs_dim, int32_t n_act, int32_t hidden, uint64_t seed, float* out, size_t n) {
  if (obs_dim < 1 || n_act < 1 || hidden < 1 || !out) { set_error("crl_make_actor_critic: bad arguments"); return 1; }
  const size_t h = (size_t)hidden, d = (size_t)obs_dim, A = (size_t)n_act;
  const size_t want = 2 * (h * d + h + h * h + h) + A * h + A + h + 1;
  if (n != want) { set_error("crl_make_actor_critic: expected " + std::to_string(want) + " floats, got " + std::to_string(n)); return 1; }
  crl::Rng rng{seed ^ 0xC1EA9B1ull};
  const double g = std::sqrt(2.0);
  float* p = out;
  for (size_t i = 0; i < n; ++i) out[i] = 0.0f;                                  // biases: zeros (Dense's default)
  // actor: mlp([in, h, h]) gain √2 (networks.jl:6-13,45), final layer gain 0.01 (networks.jl:40,42)
  crl::orthogonal(rng, hidden, obs_dim, g, p); p += h * d + h;
  crl::orthogonal(rng, hidden, hidden, g, p); p += h * h + h;
  crl::orthogonal(rng, n_act, hidden, 0.01, p); p += A * h + A;
  // critic: same trunk shape, final layer gain 1.0 (networks.jl:41,43,46)
  crl::orthogonal(rng, hidden, obs_dim, g, p); p += h * d + h;
  crl::orthogonal(rng, hidden, hidden, g, p); p += h * h + h;
  crl::orthogonal(rng, 1, hidden, 1.0, p);
  return 0;
}

int32_t crl_dqn_make_nn(uint64_t seed, float* out, size_t n) {
  if (!out || n != (size_t)CRL_DQN_PARAM_COUNT) { set_error("crl_dqn_make_nn: expected 10934 floats"); return 1; }
  crl::Rng rng{seed ^ 0xD09ull};
  for (size_t i = 0; i < n; ++i) out[i] = 0.0f;
  float* p = out;
  crl::glorot_uniform(rng, 120, 4, p); p += 120 * 4 + 120;     // dqn.jl:25 Dense(4, 120, relu)
  crl::glorot_uniform(rng, 84, 120, p); p += 84 * 120 + 84;    //           Dense(120, 84, relu)
  crl::glorot_uniform(rng, 2, 84, p);                          //           Dense(84, 2)
  return 0;
}

// the C51 net: crl_dqn_make_nn's trunk (the same draws for the same seed), then the head Dense(84, 2N)
int32_t crl_dqn_c51_make_nn(uint64_t seed, int32_t n_atoms, float* out, size_t n) {
  if (n_atoms < 2 || n_atoms > 64) { set_error("crl_dqn_c51_make_nn: n_atoms must be in 2..64"); return 1; }
  const size_t need = 10764 + 85 * 2 * (size_t)n_atoms;
  if (!out || n != need) { set_error("crl_dqn_c51_make_nn: expected " + std::to_string(need) + " floats"); return 1; }
  crl::Rng rng{seed ^ 0xD09ull};
  for (size_t i = 0; i < n; ++i) out[i] = 0.0f;
  float* p = out;
  crl::glorot_uniform(rng, 120, 4, p); p += 120 * 4 + 120;
  crl::glorot_uniform(rng, 84, 120, p); p += 84 * 120 + 84;
  crl::glorot_uniform(rng, 2 * n_atoms, 84, p);
  return 0;
}

// the dueling net: crl_dqn_make_nn's W1 and W2 draws go to W1 and W2v, then the arrays draw in layout order: W3v(R, 84), W2a(84, 120), W3a(2R, 84)
int32_t crl_dqn_dueling_make_nn(uint64_t seed, int32_t n_atoms, float* out, size_t n) {
  if (n_atoms != 0 && (n_atoms < 2 || n_atoms > 64)) { set_error("crl_dqn_dueling_make_nn: n_atoms must be 0 (scalar) or in 2..64"); return 1; }
  const int R = n_atoms == 0 ? 1 : n_atoms;
  const size_t need = 20928 + 255 * (size_t)R;
  if (!out || n != need) { set_error("crl_dqn_dueling_make_nn: expected " + std::to_string(need) + " floats"); return 1; }
  crl::Rng rng{seed ^ 0xD09ull};
  for (size_t i = 0; i < n; ++i) out[i] = 0.0f;
  float* p = out;
  crl::glorot_uniform(rng, 120, 4, p); p += 120 * 4 + 120;
  crl::glorot_uniform(rng, 84, 120, p); p += 84 * 120 + 84;
  crl::glorot_uniform(rng, R, 84, p); p += R * 84 + R;
  crl::glorot_uniform(rng, 84, 120, p); p += 84 * 120 + 84;
  crl::glorot_uniform(rng, 2 * R, 84, p);
  return 0;
}

// a noisy net (Fortunato et al. 2018, factorised rule): per layer (in, out), in the twin's array order, lim = 1/sqrt(in); mu of the weights, then of the
// biases, = (float)((u − 0.5)·(2·lim)), u one draw each in storage order; sigma = (float)(sigma0·lim) everywhere. out = mu (P) then sigma (P).
int32_t crl_dqn_noisy_make_nn(uint64_t seed, double sigma0, int32_t dueling, int32_t n_atoms, float* out, size_t n) {
  if (!(sigma0 >= 0.0 && sigma0 <= 10.0)) { set_error("crl_dqn_noisy_make_nn: sigma0 must be in 0..10"); return 1; }
  if (dueling != 0 && dueling != 1) { set_error("crl_dqn_noisy_make_nn: dueling must be 0 or 1"); return 1; }
  if (n_atoms != 0 && (n_atoms < 2 || n_atoms > 64)) { set_error("crl_dqn_noisy_make_nn: n_atoms must be 0 (scalar) or in 2..64"); return 1; }
  const int R = n_atoms == 0 ? 1 : n_atoms, rows3 = n_atoms == 0 ? 2 : 2 * n_atoms;
  const int plain[3][2] = {{4, 120}, {120, 84}, {84, rows3}}, duel[5][2] = {{4, 120}, {120, 84}, {84, R}, {120, 84}, {84, 2 * R}};
  const int (*layers)[2] = dueling ? duel : plain;
  const int nl = dueling ? 5 : 3;
  size_t P = 0;
  for (int l = 0; l < nl; ++l) P += (size_t)layers[l][1] * (size_t)(layers[l][0] + 1);
  if (!out || n != 2 * P) { set_error("crl_dqn_noisy_make_nn: expected " + std::to_string(2 * P) + " floats"); return 1; }
  crl::Rng rng{seed ^ 0x2015ull};
  float* p = out;
  for (int l = 0; l < nl; ++l) {
    const size_t cnt = (size_t)layers[l][1] * (size_t)(layers[l][0] + 1);
    const double lim = 1.0 / std::sqrt((double)layers[l][0]);
    const float sigma = (float)(sigma0 * lim);
    for (size_t i = 0; i < cnt; ++i) { p[i] = (float)((rng.uniform() - 0.5) * (2.0 * lim)); p[P + i] = sigma; }
    p += cnt;
  }
  return 0;
}

int32_t crl_ddpg_make_nn(int32_t obs_dim, int32_t act_dim, uint64_t seed, float* actor, size_t actor_n, float* critic, size_t critic_n) {
  int64_t na = 0, nc = 0;
  if (crl_ddpg_param_count(obs_dim, act_dim, &na, &nc)) return 1;
  if (!actor || !critic || actor_n != (size_t)na || critic_n != (size_t)nc) {
    set_error("crl_ddpg_make_nn: expected " + std::to_string(na) + " actor and " + std::to_string(nc) + " critic floats"); return 1;
  }
  crl::Rng rng{seed ^ 0xDD96ull};
  for (size_t i = 0; i < actor_n; ++i) actor[i] = 0.0f;
  for (size_t i = 0; i < critic_n; ++i) critic[i] = 0.0f;
  const int D = obs_dim, A = act_dim;
  float* p = actor;
  crl::glorot_uniform(rng, 64, D, p); p += 64 * D + 64;        // ddpg.jl:24 Dense(ob_size, 64, tanh_fast)
  crl::glorot_uniform(rng, 64, 64, p); p += 64 * 64 + 64;      //         25 Dense(64, 64, tanh_fast)
  crl::glorot_uniform(rng, A, 64, p);                          //         26 Dense(64, ac_size, tanh_fast)
  p = critic;
  crl::glorot_uniform(rng, 64, D + A, p); p += 64 * (D + A) + 64;   // :31 Dense(ob_size + ac_size, 64, relu)
  crl::glorot_uniform(rng, 64, 64, p); p += 64 * 64 + 64;           // :32 Dense(64, 64, relu)
  crl::glorot_uniform(rng, 1, 64, p);                               // :33 Dense(64, 1)
  return 0;
}

// SAC's networks: the critics are the two TD3 draws for `seed`; the actor (head of 2·act_dim rows) has a generator of its own
int32_t crl_sac_make_nn(int32_t obs_dim, int32_t act_dim, uint64_t seed, float* actor, size_t actor_n, float* critic1, size_t critic1_n, float* critic2,
                        size_t critic2_n) {
  int64_t na = 0, nc = 0, nda = 0;
  if (crl_sac_param_count(obs_dim, act_dim, &na, &nc) || crl_ddpg_param_count(obs_dim, act_dim, &nda, nullptr)) return 1;
  if (!actor || !critic1 || !critic2 || actor_n != (size_t)na || critic1_n != (size_t)nc || critic2_n != (size_t)nc) {
    set_error("crl_sac_make_nn: expected " + std::to_string(na) + " actor floats and " + std::to_string(nc) + " floats for each critic"); return 1;
  }
  std::vector<float> dropped((size_t)nda);                         // the DDPG-shaped actors of the two draws
  if (crl_ddpg_make_nn(obs_dim, act_dim, seed, dropped.data(), dropped.size(), critic1, critic1_n)) return 1;
  if (crl_ddpg_make_nn(obs_dim, act_dim, seed + 1, dropped.data(), dropped.size(), critic2, critic2_n)) return 1;
  crl::Rng rng{seed ^ 0x5ACull};
  for (size_t i = 0; i < actor_n; ++i) actor[i] = 0.0f;
  float* p = actor;
  crl::glorot_uniform(rng, 64, obs_dim, p); p += 64 * obs_dim + 64;
  crl::glorot_uniform(rng, 64, 64, p); p += 64 * 64 + 64;
  crl::glorot_uniform(rng, 2 * act_dim, 64, p);
  return 0;
}

}  // extern "C"
