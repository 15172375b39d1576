// norm.hip — crl_norm: running observation / reward normalisation for device-resident envs (include/cleanrl_hip.h, "Running normalisation"). An object
// of its own between any device env and any agent: no handle, rollout kernel or record layout knows about it. All state is Float64.
//
// The work of one step is a per-dimension reduction over N envs followed by an elementwise pass that needs the reduced values — at most 4 MB, so the
// cost is launches and barriers, not bytes. Two dependent launches, no grid-wide wait inside a kernel, one block of 256 threads per tile of T = 256 envs
// (the tile's T·D floats are contiguous in the (obs_dim, num_envs) layout):
//   norm_moments_kernel  tile -> LDS with 16-byte loads | pass A: Float64 sums per dimension, tile mean | pass B: M2 ABOUT THE TILE MEAN (never
//                        E[x²] − mean²) | the block's envs' acc = acc·gamma + reward and its moments as dimension D | one partial row
//                        (n_b, mean_b[D+1], M2_b[D+1]) per block. Thread t < S = D·⌊256/D⌋ walks the flat tile t, t + S, …: its dimension t mod D
//                        is fixed and consecutive lanes read consecutive LDS words. The per-thread values of a dimension are added by a radix-4
//                        tree over LDS in a fixed order (norm_tree4).
//   norm_apply_kernel    EVERY block merges the partial rows in block order onto the statistics of state buffer p (thread d dimension d, thread D
//                        the return statistic: the same bits in every block), keeps mean and 1/sqrt(var + eps) in LDS, writes obs_out / reward_out of
//                        its tile and keeps the raw episode books of its envs. Block 0 writes the merged statistics to buffer p ^ 1 — in place they
//                        would race with the other blocks' reads — and the host flips p after the launch. Finished episodes are added per block
//                        (fixed tree) to the block's own aggregate row; crl_norm_episode_stats_read folds the rows in block order. No Float64 atomics.
//   norm_fused_kernel    N <= T: moments, merge and apply of the one tile in ONE launch, observations read from memory once.
// With update = 0 only norm_apply_kernel runs, without the merge. Every sum has a fixed order: results are bit-identical from call to call.
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/cleanrl_hip.h"
#include "stage.hpp"

namespace crl {

constexpr int NORM_T = 256;          // envs per tile = threads per block
constexpr int NORM_DMAX = 64;
enum : int { NORM_UPD_OBS = 1, NORM_UPD_RET = 2, NORM_RESET = 4, NORM_OBS = 8, NORM_REW = 16, NORM_VEC = 32, NORM_ACC_DONE = 64 };

struct NormArgs {
  const float* obs_in; const float* reward_in; const uint8_t* done;   // (D, N), [N], [N]
  float* obs_out; float* reward_out;
  const double* st_in; double* st_out;     // count_o, mean[D], var[D], count_r, mean_r, var_r: buffers p and p ^ 1
  double* acc; double* ep_ret; int32_t* ep_len;   // [N] each
  double* part;                            // [blocks][2(D+1)+1]: n_b | mean_b[D+1] | M2_b[D+1], entry D = the return accumulator
  double* agg;                             // [blocks][4]: episodes, return_sum, length_sum, return_max of the block's envs since the last clear
  int N, D, flags;
  double gamma, eps, clip_obs, clip_rew;
};
__host__ __device__ inline int norm_row(int D) { return 2 * (D + 1) + 1; }

struct NormLds {
  double red[4][NORM_T];                   // reduction scratch: [0] dimensions, [1] return accumulator; all four for the episode aggregate
  double tmean[NORM_DMAX + 1], mean[NORM_DMAX + 1], rstd[NORM_DMAX + 1];
  double row[2 * (NORM_DMAX + 1) + 1];     // the fused kernel's one partial row
};

// red[g·D + d], g < G: the G per-thread values of dimension d; reda[t], t < 256. Afterwards red[d] and reda[0] hold the sums, added in a fixed radix-4
// tree: at width h thread g < h takes g, g + h, g + 2h, g + 3h, left to right. Entry g is read by thread g alone, so one barrier per level is enough.
__device__ __forceinline__ void norm_tree4(double* red, int D, int G, int g, int d, bool act, double* reda, bool with_a, int t) {
#pragma clang fp contract(off)
  const int top = with_a ? NORM_T : G;
  for (int h = NORM_T / 4; h >= 1; h >>= 2) {
    if (h >= top) continue;                // uniform: nothing to fold at this width
    __syncthreads();
    const int lim = G < 4 * h ? G : 4 * h;
    if (act && g < h) {
      double v = red[g * D + d];
      for (int k = 1; k < 4; ++k) if (g + k * h < lim) v += red[(g + k * h) * D + d];
      red[g * D + d] = v;
    }
    if (with_a && t < h) reda[t] = ((reda[t] + reda[t + h]) + reda[t + 2 * h]) + reda[t + 3 * h];
  }
  __syncthreads();
}

// cnt floats of one tile, memory -> LDS; nothing at or past src + cnt is read
__device__ __forceinline__ void norm_tile_load(float* tile, const float* src, int cnt, bool vec, int t) {
  if (vec) {
    const int n4 = cnt >> 2;
    for (int i = t; i < n4; i += NORM_T) reinterpret_cast<float4*>(tile)[i] = reinterpret_cast<const float4*>(src)[i];
    for (int i = 4 * n4 + t; i < cnt; i += NORM_T) tile[i] = src[i];
  } else {
    for (int i = t; i < cnt; i += NORM_T) tile[i] = src[i];
  }
}

// The moments of one tile (ne envs from e0, in LDS) into `row`; with NORM_UPD_RET also acc <- acc·gamma + reward of the tile's envs and its moments.
__device__ __forceinline__ void norm_tile_moments(const NormArgs& a, NormLds& l, const float* tile, int e0, int ne, double* row, int t) {
#pragma clang fp contract(off)
  const int D = a.D, G = NORM_T / D, S = G * D, cnt = ne * D;
  const bool obs = a.flags & NORM_UPD_OBS, ret = a.flags & NORM_UPD_RET, act = obs && t < S;
  const int g = t / D, d = t - g * D;
  const double n_b = (double)ne;
  double av = 0.0;
  if (ret && t < ne) { av = a.acc[e0 + t] * a.gamma; av = av + (double)a.reward_in[e0 + t]; a.acc[e0 + t] = av; }
  // pass A: sums
  if (act) { double s = 0.0; for (int i = t; i < cnt; i += S) s += (double)tile[i]; l.red[0][t] = s; }
  if (ret) l.red[1][t] = t < ne ? av : 0.0;
  norm_tree4(l.red[0], D, G, g, d, act, l.red[1], ret, t);
  if (obs && t < D) l.tmean[t] = l.red[0][t] / n_b;
  if (ret && t == 0) l.tmean[D] = l.red[1][0] / n_b;
  __syncthreads();
  // pass B: squares about the tile mean
  if (act) { const double m = l.tmean[d]; double q = 0.0; for (int i = t; i < cnt; i += S) { const double x = (double)tile[i] - m; q += x * x; } l.red[0][t] = q; }
  if (ret) { const double x = av - l.tmean[D]; l.red[1][t] = t < ne ? x * x : 0.0; }
  norm_tree4(l.red[0], D, G, g, d, act, l.red[1], ret, t);
  if (t == 0) row[0] = (double)ne;
  if (obs && t < D) { row[1 + t] = l.tmean[t]; row[1 + (D + 1) + t] = l.red[0][t]; }
  if (ret && t == 0) { row[1 + D] = l.tmean[D]; row[1 + (D + 1) + D] = l.red[1][0]; }
}

// gymnasium's update_from_moments of `nb` partial rows, in row order, onto the statistics of st_in: thread d <= D owns one statistic. mean and
// 1/sqrt(var + eps) go to LDS; `store` (block 0) also writes the whole merged state to st_out.
__device__ __forceinline__ void norm_merge(const NormArgs& a, NormLds& l, const double* rows, int nb, bool store, int t) {
#pragma clang fp contract(off)
  const int D = a.D, RS = norm_row(D);
  if (t <= D) {
    const bool isret = t == D;
    const int ic = isret ? 2 * D + 1 : 0, im = isret ? 2 * D + 2 : 1 + t, iv = isret ? 2 * D + 3 : 1 + D + t;
    double cnt = a.st_in[ic], mean = a.st_in[im], var = a.st_in[iv];
    if (a.flags & (isret ? NORM_UPD_RET : NORM_UPD_OBS)) {
      // 1 / tot hangs on the counts alone: the divisions of successive rows overlap, and the chain through mean and var is multiplications and additions
#pragma unroll 4
      for (int b = 0; b < nb; ++b) {
        const double* r = rows + (size_t)b * RS;
        const double n_b = r[0], tot = cnt + n_b, inv = 1.0 / tot, w = n_b * inv, delta = r[1 + t] - mean;
        mean = mean + delta * w;
        var = (var * cnt + r[1 + (D + 1) + t] + delta * delta * (cnt * w)) * inv;
        cnt = tot;
      }
    }
    l.mean[t] = mean; l.rstd[t] = 1.0 / sqrt(var + a.eps);
    if (store) {
      a.st_out[im] = mean; a.st_out[iv] = var;
      if (t == 0 || isret) a.st_out[ic] = cnt;
    }
  }
  __syncthreads();
}

__device__ __forceinline__ float norm_scale(float x, double mean, double rstd, double clip) {
#pragma clang fp contract(off)
  double y = ((double)x - mean) * rstd;
  y = y < -clip ? -clip : (y > clip ? clip : y);
  return (float)y;
}

// obs_out of one tile from src (memory or the LDS tile): flat index i has dimension i mod D, carried along instead of divided out.
__device__ __forceinline__ void norm_apply_obs(const NormArgs& a, const NormLds& l, const float* src, float* dst, int cnt, int t) {
  const int D = a.D;
  const bool norm = a.flags & NORM_OBS;
  const double clip = a.clip_obs;
  if (a.flags & NORM_VEC) {
    const int n4 = cnt >> 2, step = (4 * NORM_T) % D;
    int d = (4 * t) % D;
    for (int i = t; i < n4; i += NORM_T) {
      float4 x = reinterpret_cast<const float4*>(src)[i];
      if (norm) {
        int dd = d;
        x.x = norm_scale(x.x, l.mean[dd], l.rstd[dd], clip); dd = dd + 1 == D ? 0 : dd + 1;
        x.y = norm_scale(x.y, l.mean[dd], l.rstd[dd], clip); dd = dd + 1 == D ? 0 : dd + 1;
        x.z = norm_scale(x.z, l.mean[dd], l.rstd[dd], clip); dd = dd + 1 == D ? 0 : dd + 1;
        x.w = norm_scale(x.w, l.mean[dd], l.rstd[dd], clip);
      }
      reinterpret_cast<float4*>(dst)[i] = x;
      d += step; if (d >= D) d -= D;
    }
    for (int i = 4 * n4 + t; i < cnt; i += NORM_T) { const int dd = i % D; dst[i] = norm ? norm_scale(src[i], l.mean[dd], l.rstd[dd], clip) : src[i]; }
  } else {
    const int step = NORM_T % D;
    int d = t % D;
    for (int i = t; i < cnt; i += NORM_T) {
      dst[i] = norm ? norm_scale(src[i], l.mean[d], l.rstd[d], clip) : src[i];
      d += step; if (d >= D) d -= D;
    }
  }
}

// reward_out and the raw episode books of the tile's envs (steps 3 and 4), or the zeroing of a reset.
__device__ __forceinline__ void norm_apply_env(const NormArgs& a, NormLds& l, int e0, int ne, int t) {
#pragma clang fp contract(off)
  const int e = e0 + t;
  const bool live = t < ne;
  if (a.flags & NORM_RESET) {
    if (live) { a.acc[e] = 0.0; a.ep_ret[e] = 0.0; a.ep_len[e] = 0; }
    return;
  }
  double s_n = 0.0, s_ret = 0.0, s_len = 0.0, s_max = -INFINITY;
  if (live) {
    const float r = a.reward_in[e];
    const double rd = (double)r;
    const bool dn = a.done[e] != 0;
    if (a.flags & NORM_REW) {
      if (!(a.flags & NORM_ACC_DONE)) { double av = a.acc[e] * a.gamma; av = av + rd; if (!dn) a.acc[e] = av; }
      if (dn) a.acc[e] = 0.0;
      double y = rd * l.rstd[a.D];
      y = y < -a.clip_rew ? -a.clip_rew : (y > a.clip_rew ? a.clip_rew : y);
      a.reward_out[e] = (float)y;
    } else {
      a.reward_out[e] = r;
    }
    double er = a.ep_ret[e] + rd;
    int el = a.ep_len[e] + 1;
    if (dn) { s_n = 1.0; s_ret = er; s_len = (double)el; s_max = er; er = 0.0; el = 0; }
    a.ep_ret[e] = er; a.ep_len[e] = el;
  }
  if (__syncthreads_count(s_n != 0.0) == 0) return;        // uniform: no episode ended in this tile
  l.red[0][t] = s_n; l.red[1][t] = s_ret; l.red[2][t] = s_len; l.red[3][t] = s_max;
  for (int h = NORM_T / 4; h >= 1; h >>= 2) {
    __syncthreads();
    if (t < h) {
      for (int j = 0; j < 3; ++j) l.red[j][t] = ((l.red[j][t] + l.red[j][t + h]) + l.red[j][t + 2 * h]) + l.red[j][t + 3 * h];
      l.red[3][t] = fmax(fmax(l.red[3][t], l.red[3][t + h]), fmax(l.red[3][t + 2 * h], l.red[3][t + 3 * h]));
    }
  }
  if (t == 0) {                                            // the row belongs to this block alone
    double* r = a.agg + 4 * (size_t)blockIdx.x;
    r[3] = r[0] == 0.0 ? l.red[3][0] : fmax(r[3], l.red[3][0]);
    r[0] += l.red[0][0]; r[1] += l.red[1][0]; r[2] += l.red[2][0];
  }
}

__global__ void __launch_bounds__(NORM_T) norm_moments_kernel(NormArgs a) {
  extern __shared__ __attribute__((aligned(16))) float norm_tile[];
  __shared__ NormLds l;
  const int t = threadIdx.x, e0 = blockIdx.x * NORM_T, ne = a.N - e0 < NORM_T ? a.N - e0 : NORM_T;
  if (a.flags & NORM_UPD_OBS) norm_tile_load(norm_tile, a.obs_in + (size_t)e0 * a.D, ne * a.D, a.flags & NORM_VEC, t);
  __syncthreads();
  norm_tile_moments(a, l, norm_tile, e0, ne, a.part + (size_t)blockIdx.x * norm_row(a.D), t);
}

__global__ void __launch_bounds__(NORM_T) norm_apply_kernel(NormArgs a) {
  __shared__ NormLds l;
  const int t = threadIdx.x, e0 = blockIdx.x * NORM_T, ne = a.N - e0 < NORM_T ? a.N - e0 : NORM_T;
  const bool upd = a.flags & (NORM_UPD_OBS | NORM_UPD_RET);
  norm_merge(a, l, a.part, (int)gridDim.x, upd && blockIdx.x == 0, t);
  norm_apply_obs(a, l, a.obs_in + (size_t)e0 * a.D, a.obs_out + (size_t)e0 * a.D, ne * a.D, t);
  norm_apply_env(a, l, e0, ne, t);
}

__global__ void __launch_bounds__(NORM_T) norm_fused_kernel(NormArgs a) {   // N <= NORM_T, one block, an update
  extern __shared__ __attribute__((aligned(16))) float norm_tile[];
  __shared__ NormLds l;
  const int t = threadIdx.x, ne = a.N;
  norm_tile_load(norm_tile, a.obs_in, ne * a.D, a.flags & NORM_VEC, t);
  __syncthreads();
  norm_tile_moments(a, l, norm_tile, 0, ne, l.row, t);
  __syncthreads();
  norm_merge(a, l, l.row, 1, true, t);
  norm_apply_obs(a, l, norm_tile, a.obs_out, ne * a.D, t);
  norm_apply_env(a, l, 0, ne, t);
}

}  // namespace crl

using namespace crl;

struct crl_norm {
  int device = 0;
  crl_norm_options opt{};
  int blocks = 0, p = 0;                   // p: which state buffer is current
  double* state[2] = {nullptr, nullptr};   // 2D + 4 doubles each
  double* acc = nullptr; double* ep_ret = nullptr; int32_t* ep_len = nullptr;
  double* part = nullptr; double* agg = nullptr;
  hipStream_t stream = nullptr;            // the stream of the last _device call: what read / write / episode_stats_read synchronise
};

static size_t norm_state_len(const crl_norm* n) { return 2 * (size_t)n->opt.obs_dim + 4; }

static int norm_check(const crl_norm_options* o) {
  const std::string w = "crl_norm_create: ";
  if (o->num_envs < 1 || o->num_envs > (1 << 20)) { set_error(w + "num_envs must be in 1..1048576, got " + std::to_string(o->num_envs)); return 1; }
  if (o->obs_dim < 1 || o->obs_dim > NORM_DMAX) { set_error(w + "obs_dim must be in 1..64, got " + std::to_string(o->obs_dim)); return 1; }
  if (!(o->gamma >= 0.0 && o->gamma <= 1.0)) { set_error(w + "gamma must be in [0, 1]"); return 1; }
  if (!(o->epsilon > 0.0) || std::isinf(o->epsilon)) { set_error(w + "epsilon must be positive and finite"); return 1; }
  if (!(o->clip_obs > 0.0)) { set_error(w + "clip_obs must be positive"); return 1; }
  if (!(o->clip_reward > 0.0)) { set_error(w + "clip_reward must be positive"); return 1; }
  return 0;
}

static int norm_create(crl_norm* n) {
  const size_t N = (size_t)n->opt.num_envs, L = norm_state_len(n), D = (size_t)n->opt.obs_dim;
  n->blocks = (int)((N + NORM_T - 1) / NORM_T);
  if (dalloc(&n->state[0], L) || dalloc(&n->state[1], L) || dalloc(&n->acc, N) || dalloc(&n->ep_ret, N) || dalloc(&n->ep_len, N) ||
      dalloc(&n->part, (size_t)n->blocks * norm_row((int)D)) || dalloc(&n->agg, (size_t)n->blocks * 4)) return 1;
  std::vector<double> s(L, 0.0);
  s[0] = 1e-4; s[2 * D + 1] = 1e-4; s[2 * D + 3] = 1.0;
  for (size_t d = 0; d < D; ++d) s[1 + D + d] = 1.0;
  CRL_HIP_CHECK(hipMemcpy(n->state[0], s.data(), L * sizeof(double), hipMemcpyHostToDevice));
  // the tile of the widest observation is 64 KB of dynamic LDS next to the static block
  const int tile = NORM_T * NORM_DMAX * (int)sizeof(float);
  CRL_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(norm_moments_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, tile));
  CRL_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(norm_fused_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, tile));
  CRL_HIP_CHECK(hipDeviceSynchronize());
  return 0;
}

// reset (reward_in = done = reward_out = nullptr) or step: only enqueues on `stream`
static int norm_launch(crl_norm* n, const float* obs_in, const float* reward_in, const uint8_t* done, float* obs_out, float* reward_out, bool reset,
                       int update, hipStream_t stream) {
  const crl_norm_options& o = n->opt;
  NormArgs a;
  a.obs_in = obs_in; a.reward_in = reward_in; a.done = done; a.obs_out = obs_out; a.reward_out = reward_out;
  a.st_in = n->state[n->p]; a.st_out = n->state[n->p ^ 1];
  a.acc = n->acc; a.ep_ret = n->ep_ret; a.ep_len = n->ep_len; a.part = n->part; a.agg = n->agg;
  a.N = o.num_envs; a.D = o.obs_dim;
  a.gamma = o.gamma; a.eps = o.epsilon; a.clip_obs = o.clip_obs; a.clip_rew = o.clip_reward;
  int f = (reset ? NORM_RESET : 0) | (o.norm_obs ? NORM_OBS : 0) | (o.norm_reward ? NORM_REW : 0);
  if (update && o.norm_obs) f |= NORM_UPD_OBS;
  if (update && o.norm_reward && !reset) f |= NORM_UPD_RET | NORM_ACC_DONE;
  if (((reinterpret_cast<uintptr_t>(obs_in) | reinterpret_cast<uintptr_t>(obs_out)) & 15) == 0) f |= NORM_VEC;
  a.flags = f;
  n->stream = stream;
  const bool upd = f & (NORM_UPD_OBS | NORM_UPD_RET);
  const size_t tile = (f & NORM_UPD_OBS) ? (size_t)NORM_T * o.obs_dim * sizeof(float) : 0;
  if (upd && n->blocks == 1) {
    hipLaunchKernelGGL(norm_fused_kernel, dim3(1), dim3(NORM_T), (size_t)NORM_T * o.obs_dim * sizeof(float), stream, a);
  } else {
    if (upd) hipLaunchKernelGGL(norm_moments_kernel, dim3(n->blocks), dim3(NORM_T), tile, stream, a);
    hipLaunchKernelGGL(norm_apply_kernel, dim3(n->blocks), dim3(NORM_T), 0, stream, a);
  }
  CRL_HIP_CHECK(hipGetLastError());
  if (upd) n->p ^= 1;
  return 0;
}

extern "C" {

int32_t crl_norm_create(const crl_norm_options* opt, int32_t device, crl_norm** out) {
  if (!opt || !out) { set_error("crl_norm_create: null argument"); return 1; }
  if (norm_check(opt)) return 1;
  CRL_HIP_CHECK(hipSetDevice(device));
  crl_norm* n = new crl_norm();
  n->device = device; n->opt = *opt;
  if (norm_create(n)) { crl_norm_destroy(n); return 1; }
  *out = n;
  return 0;
}

int32_t crl_norm_destroy(crl_norm* n) {
  if (!n) return 0;
  (void)hipSetDevice(n->device);
  if (n->stream) (void)hipStreamSynchronize(n->stream);
  void* bufs[] = {n->state[0], n->state[1], n->acc, n->ep_ret, n->ep_len, n->part, n->agg};
  for (void* b : bufs) if (b) (void)hipFree(b);
  delete n;
  return 0;
}

int32_t crl_norm_reset_device(crl_norm* n, const float* obs_in_d, float* obs_out_d, int32_t update, void* stream) {
  CRL_HANDLE_GUARD(n, "crl_norm");
  if (!obs_in_d || !obs_out_d) { set_error(std::string("crl_norm_reset_device: ") + (!obs_in_d ? "obs_in_d" : "obs_out_d") + " is NULL"); return 1; }
  return norm_launch(n, obs_in_d, nullptr, nullptr, obs_out_d, nullptr, true, update, static_cast<hipStream_t>(stream));
}

int32_t crl_norm_step_device(crl_norm* n, const float* obs_in_d, const float* reward_in_d, const uint8_t* done_d, float* obs_out_d, float* reward_out_d,
                             int32_t update, void* stream) {
  CRL_HANDLE_GUARD(n, "crl_norm");
  const void* ptr[] = {obs_in_d, reward_in_d, done_d, obs_out_d, reward_out_d};
  const char* name[] = {"obs_in_d", "reward_in_d", "done_d", "obs_out_d", "reward_out_d"};
  for (int i = 0; i < 5; ++i) if (!ptr[i]) { set_error(std::string("crl_norm_step_device: ") + name[i] + " is NULL"); return 1; }
  return norm_launch(n, obs_in_d, reward_in_d, done_d, obs_out_d, reward_out_d, false, update, static_cast<hipStream_t>(stream));
}

int32_t crl_norm_read(crl_norm* n, double* out, size_t count) {
  CRL_HANDLE_GUARD(n, "crl_norm");
  if (!out || count != norm_state_len(n)) { set_error("crl_norm_read: out must hold 2·obs_dim + 4 doubles"); return 1; }
  CRL_HIP_CHECK(hipStreamSynchronize(n->stream));
  CRL_HIP_CHECK(hipMemcpy(out, n->state[n->p], count * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

int32_t crl_norm_write(crl_norm* n, const double* in, size_t count) {
  CRL_HANDLE_GUARD(n, "crl_norm");
  if (!in || count != norm_state_len(n)) { set_error("crl_norm_write: in must hold 2·obs_dim + 4 doubles"); return 1; }
  CRL_HIP_CHECK(hipStreamSynchronize(n->stream));
  CRL_HIP_CHECK(hipMemcpy(n->state[n->p], in, count * sizeof(double), hipMemcpyHostToDevice));
  return 0;
}

int32_t crl_norm_episode_stats_read(crl_norm* n, crl_episode_stats* out, int32_t clear) {
  CRL_HANDLE_GUARD(n, "crl_norm");
  if (!out) { set_error("crl_norm_episode_stats_read: null argument"); return 1; }
  std::vector<double> rows((size_t)n->blocks * 4);
  CRL_HIP_CHECK(hipStreamSynchronize(n->stream));
  CRL_HIP_CHECK(hipMemcpy(rows.data(), n->agg, rows.size() * sizeof(double), hipMemcpyDeviceToHost));
  crl_episode_stats s{0.0, 0.0, 0.0, 0.0};
  for (int b = 0; b < n->blocks; ++b) {                   // block order
    const double* r = &rows[4 * (size_t)b];
    if (r[0] == 0.0) continue;
    s.return_max = s.episodes == 0.0 ? r[3] : std::fmax(s.return_max, r[3]);
    s.episodes += r[0]; s.return_sum += r[1]; s.length_sum += r[2];
  }
  *out = s;
  if (clear) {
    CRL_HIP_CHECK(hipMemsetAsync(n->agg, 0, rows.size() * sizeof(double), n->stream));
    CRL_HIP_CHECK(hipStreamSynchronize(n->stream));
  }
  return 0;
}

}  // extern "C"
