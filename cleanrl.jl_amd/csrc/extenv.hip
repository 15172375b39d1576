// extenv.hip — device-resident external envs: the two per-step launches of crl_rollout_act_device / crl_rollout_record_device. The caller's simulator
// lives on the same GPU and hands over device pointers; nothing is staged and the host never waits inside the rollout loop.
//
// ext_act_kernel<H>: ppo.jl:127-128 plus the state / action / logprob / terminal / value fields of Buffer.add! (:133-140) for ONE step of all envs. The block
// of diag_kernel (diag.hip): H / 32 waves, wave w keeps rows 32w … 32w + 31 of W2 as bf16x3 A fragments in registers (the last three k-steps in LDS at 256),
// persistent over 32-env tiles; ROLES ARE BLOCKS — even blocks hold the actor, odd blocks the critic, block 2j / 2j + 1 both walk tiles j, j + nrb, … . One kernel
// family for the 4 / 2 / 64 shape and every layer-wise shape (obs_dim <= 64, n_act <= 16, hidden 64 / 128 / 256); no option and no route of the handle is read.
//   per tile  the 32 x obs_dim observations (contiguous in obs_d) to LDS — the ACTOR block also copies them to slot `step` of the buffer, it has them in
//             flight anyway | barrier | layer 1 on the vector pipe from LDS: tanh_fast, bf16x3 split, B-fragment order | barrier | layer 2 on
//             v_mfma_f32_32x32x16_bf16 (f32 accumulation), tanh_fast | barrier | the wave's head partials to LDS | barrier | lanes 0-31 of wave 0, one env each:
//             actor  softmax_rt (policy_rt.hpp), u = u53(philox_env(seed, env_id_offset + e, iteration * num_steps + step, 0)) — the draw every on-device
//                    rollout kernel takes for that env and step —, sample_rt, the logprob of the drawn action; action to the buffer and to action_d, logprob
//             critic the value; terminal <- done_d
//   stores    plain vector stores to the (·, num_envs, num_steps) layout, env fastest; a partial last tile reads and writes nothing past num_envs.
//
// ext_record_kernel: ppo.jl:132,137,143-165 for one step, one thread per env: reward to the slot, CRL_F_CUR_OBS / CRL_F_NEXT_DONE <- next_obs_d / next_done_d
// (what the fixed-mode bootstrap reads), ep_length += 1, ep_return += reward (Float32, step order); where next_done: the four ep_stats doubles (wave sums, one
// atomic set per wave like the rollout kernels), a record {return, length, env_id_offset + e, step} to the episode ring through the same atomic counter, and
// zeroed accumulators. return_max keeps the order-preserving key of the signed env kinds (api.cpp maps it back).
#include "common.hpp"
#include "mlp_x3.hpp"
#include "policy_rt.hpp"
#include "ppo_ctx.hpp"

namespace crl {

constexpr int EXT_OBS_MAX = 64;

struct ExtActArgs {
  const float* params; int64_t Pa;   // actor | critic, each W1(H,D) b1(H) W2(H,H) b2(H) W3(n_out,H) b3(n_out), (out,in) column-major
  const float* obs_in; const uint8_t* done_in; int32_t* action_out;   // the caller's: (D, N), [N], [N]
  float* obs; int32_t* action; float* logprob; float* value; uint8_t* terminal;   // slot `step` of the resident buffer: (D, N), [N] each
  int D, A, N;
  int w1_lds;                        // 1 = W1 fits LDS next to everything else, 0 = layer 1 reads it from the parameters (hidden 256 with a wide observation)
  uint64_t seed, gstep; uint32_t gid0;
};

__host__ __device__ constexpr int ext_ks_lds(int H) { return H == 256 ? 3 : 0; }
// LDS (floats): h1 pieces | W2 fragments of the k-steps that are not in registers | b1 | b2 (C-fragment order) | b3 | W3 (C-fragment order) [n_out][H] |
// observations [32][D | 1] | W1 [D][H] as the parameters hold it (when it fits)
__host__ __device__ constexpr int ext_lds_fixed(int H) { return 3 * H * 16 + ext_ks_lds(H) * 3 * (H / 32) * 64 * 4 + H + H + AMAX; }
__host__ __device__ constexpr int ext_xs(int D) { return D | 1; }   // odd row stride: the 32 envs of a column sit in 32 banks
static inline size_t ext_lds_bytes(int H, int D, int A, bool w1_lds) {
  return sizeof(float) * (size_t)(ext_lds_fixed(H) + ((A * H + 3) & ~3) + ((32 * ext_xs(D) + 3) & ~3) + (w1_lds ? H * D : 0));
}

typedef float f32x4w __attribute__((ext_vector_type(4), aligned(4)));   // the critic's W1 starts where the actor's parameters end: 4-byte aligned only
// eight consecutive hidden rows of one env: column k of W1 (two 16-byte reads, from LDS or from the parameters as they lie in HBM) times x[k], k in order
template <typename V>
__device__ __forceinline__ void ext_layer1(const float* wcol, int ldw, const float* x, int D, float (&hv)[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) hv[j] = 0.0f;
#pragma unroll 2
  for (int k = 0; k < D; ++k) {
    const V w0 = reinterpret_cast<const V*>(wcol + (size_t)ldw * k)[0], w1 = reinterpret_cast<const V*>(wcol + (size_t)ldw * k)[1];
    const float xv = x[k];
#pragma unroll
    for (int j = 0; j < 4; ++j) { hv[j] = __builtin_fmaf(w0[j], xv, hv[j]); hv[4 + j] = __builtin_fmaf(w1[j], xv, hv[4 + j]); }
  }
}

template <int H>
__global__ void __launch_bounds__(2 * H) ext_act_kernel(ExtActArgs a) {
  constexpr int NW = H / 32, KS = H / 16, NT = 2 * H, KL = ext_ks_lds(H), KR = KS - KL;
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int D = a.D, XS = ext_xs(D), N = a.N;
  const int role = blockIdx.x & 1, rb = blockIdx.x >> 1, nrb = gridDim.x >> 1;   // 0 = actor, 1 = critic
  const int A = role ? 1 : a.A;
  bf16x8* h1p = reinterpret_cast<bf16x8*>(sm);                  // [piece][ks][lane]: B fragments of h1, k = 16 ks + 8 (lane >> 5) + j
  bf16x8* wl = h1p + 3 * KS * 64;                               // [KL][piece][wave][lane]: A fragments of the last KL k-steps of W2
  float* b1l = sm + 3 * H * 16 + KL * 3 * NW * 64 * 4;
  float* b2c = b1l + H;                                         // [wave][hf][16]: b2[32 wave + rowmap(r, hf)]
  float* b3l = b2c + H;
  float* zp = sm;                                               // [wave][AMAX][32 envs]: head partials, in the first third of the h1 region once layer 2 has read it
  float* w3c = b3l + AMAX;                                      // [A][wave][hf][16]
  float* xt = w3c + ((a.A * H + 3) & ~3);                       // [32 envs][XS]
  float* w1l = xt + ((32 * XS + 3) & ~3);                       // [D][H], column k at 16-byte aligned H k
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, hf = lane >> 5, i = lane & 31;
  const float* W1 = a.params + (role ? a.Pa : 0); const float* b1 = W1 + H * D; const float* W2 = b1 + H; const float* b2 = W2 + H * H;
  const float* W3 = b2 + H; const float* b3 = W3 + A * H;

  if (a.w1_lds) for (int idx = tid; idx < H * D; idx += NT) w1l[idx] = W1[idx];
  for (int idx = tid; idx < H; idx += NT) {
    b1l[idx] = b1[idx];
    b2c[idx] = b2[32 * (idx >> 5) + rowmap(idx & 15, (idx >> 4) & 1)];
  }
  for (int idx = tid; idx < A * H; idx += NT) {
    const int aa = idx / H, q = idx % H;
    w3c[idx] = W3[aa + A * (32 * (q >> 5) + rowmap(q & 15, (q >> 4) & 1))];
  }
  if (tid < AMAX) b3l[tid] = tid < A ? b3[tid] : 0.0f;
  P3 wr[KR];                                                     // this wave's 32 rows of W2: A fragments, row = 32 w + i
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = W2[(32 * w + i) + H * (16 * ks + 8 * hf + j)];
    if (ks < KR) wr[ks] = split3(v);
    else { const P3 p = split3(v); bf16x8* q = wl + ((ks - KR) * 3 * NW + w) * 64 + lane; q[0] = p.hi; q[NW * 64] = p.mid; q[2 * NW * 64] = p.lo; }
    if (ks & 1) __builtin_amdgcn_sched_barrier(0);               // raw rows of two k-steps in flight: the split pieces fill the file
  }
  __syncthreads();

  for (int tile = rb; tile * 32 < N; tile += nrb) {
    const int e0 = tile * 32, ne = N - e0 < 32 ? N - e0 : 32;
    const bool mine = w == 0 && lane < ne;
    for (int idx = tid; idx < 32 * D; idx += NT) {               // obs (D, N): the tile's 32 D floats are contiguous; nothing at or past env N is touched
      const int m = idx / D, k = idx - m * D;
      float x = 0.0f;
      if (m < ne) {
        x = a.obs_in[(size_t)e0 * D + idx];
        if (role == 0) a.obs[(size_t)e0 * D + idx] = x;          // Buffer.add!'s state field: written once, by the actor's block
      }
      xt[m * XS + k] = x;
    }
    __syncthreads();
    {                                                            // layer 1: env m, hidden rows 8 oct … 8 oct + 7
      const int m = tid & 31, g8 = tid >> 5;
#pragma unroll 1
      for (int half = 0; half < 2; ++half) {
        const int oct = g8 + half * (H / 16);
        float hv[8];
        if (a.w1_lds) ext_layer1<f32x4>(w1l + 8 * oct, H, xt + m * XS, D, hv);
        else ext_layer1<f32x4w>(W1 + 8 * oct, H, xt + m * XS, D, hv);
#pragma unroll
        for (int j = 0; j < 8; ++j) hv[j] = tanh_fast(hv[j] + b1l[8 * oct + j]);
        const P3 p = split3(hv);
        const int slot = (oct >> 1) * 64 + (oct & 1) * 32 + m;
        h1p[slot] = p.hi; h1p[KS * 64 + slot] = p.mid; h1p[2 * KS * 64 + slot] = p.lo;
      }
    }
    __syncthreads();
    {                                                            // layer 2 + the wave's head partials
      f32x16 acc = load16(b2c + (2 * w + hf) * 16);
      const bf16x8* hb = h1p + lane;
      asm volatile("" : "+v"(hb));                               // one base per tile, constant offsets behind it
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        P3 b;
        b.hi = hb[ks * 64]; b.mid = hb[(KS + ks) * 64]; b.lo = hb[(2 * KS + ks) * 64];
        if (ks < KR) acc = mfma_x3(wr[ks], b, acc);
        else {
          const bf16x8* q = wl + ((ks - KR) * 3 * NW + w) * 64 + lane;
          P3 aw; aw.hi = q[0]; aw.mid = q[NW * 64]; aw.lo = q[2 * NW * 64];
          acc = mfma_x3(aw, b, acc);
        }
        if (ks & 1) __builtin_amdgcn_sched_barrier(0);           // at most two k-steps of B fragments in flight
      }
      __syncthreads();                                           // every wave has read its h1 fragments: the region now takes the head partials
      float h2[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) h2[r] = tanh_fast(acc[r]);
      for (int aa = 0; aa < A; ++aa) {
        const f32x4* wv = reinterpret_cast<const f32x4*>(w3c + aa * H + (2 * w + hf) * 16);
        float p = 0.0f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const f32x4 v = wv[q];
#pragma unroll
          for (int c = 0; c < 4; ++c) p = __builtin_fmaf(v[c], h2[4 * q + c], p);
        }
        p = add32(p);
        if (hf == 0) zp[(w * AMAX + aa) * 32 + i] = p;
      }
    }
    __syncthreads();
    if (mine) {                                                  // one lane per env; the next tile's first barrier stands between these reads of zp and layer 1's writes of h1
      const int e = e0 + lane;
      float z[AMAX];
      const float* zl = zp + lane;
      asm volatile("" : "+v"(zl));
#pragma unroll
      for (int aa = 0; aa < AMAX; ++aa) {
        float v = 0.0f;
        if (aa < A) {
          v = b3l[aa];
          for (int ww = 0; ww < NW; ++ww) v += zl[(ww * AMAX + aa) * 32];
        }
        z[aa] = v;
      }
      if (role == 0) {                                           // ppo.jl:21-32 get_action
        float p[AMAX], lp[AMAX];
#pragma unroll
        for (int aa = 0; aa < AMAX; ++aa) { p[aa] = 0.0f; lp[aa] = 0.0f; }
        softmax_rt(z, A, p, lp);
        const double u = u53(philox_env(a.seed, a.gid0 + (uint32_t)e, a.gstep, 0));
        const int act = sample_rt(p, A, u);
        float lpa = lp[0];
#pragma unroll
        for (int aa = 1; aa < AMAX; ++aa) lpa = (act == aa) ? lp[aa] : lpa;
        a.action[e] = act; a.action_out[e] = act; a.logprob[e] = lpa;
      } else {
        a.value[e] = z[0];
        a.terminal[e] = a.done_in[e];
      }
    }
  }
}

// order-preserving u64 key of a double (as wide.hip's signed env kinds keep their return_max): 0 is below every key, so a zeroed accumulator means "no episode"
__device__ __forceinline__ unsigned long long ext_max_key(double x) {
  unsigned long long b; __builtin_memcpy(&b, &x, 8);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

struct ExtRecArgs {
  const float* reward_in; const float* next_obs_in; const uint8_t* next_done_in;
  float* reward;                                   // slot `step`
  float* cur_obs; uint8_t* next_done; float* ep_return; int32_t* ep_length; double* ep_stats;
  crl_episode_record* ring; uint32_t* ring_count; int ring_cap;
  int D, N, step; uint32_t gid0;
};

__global__ void __launch_bounds__(256) ext_record_kernel(ExtRecArgs a) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  const bool live = e < a.N;
  double st_n = 0.0, st_ret = 0.0, st_len = 0.0, st_max = -__builtin_inf();
  if (live) {
    const float rew = a.reward_in[e];
    a.reward[e] = rew;                                            // ppo.jl:132,137
    for (int k = 0; k < a.D; ++k) a.cur_obs[(size_t)e * a.D + k] = a.next_obs_in[(size_t)e * a.D + k];   // ppo.jl:143
    const uint8_t nd = a.next_done_in[e];
    a.next_done[e] = nd;                                          // ppo.jl:144
    int ep_len = a.ep_length[e] + 1;                              // ppo.jl:125
    float ep_ret = a.ep_return[e] + rew;                          // ppo.jl:145
    if (nd) {                                                     // ppo.jl:147-165
      st_n = 1.0; st_ret = (double)ep_ret; st_len = (double)ep_len; st_max = (double)ep_ret;
      if (a.ring_cap > 0) {
        const uint32_t slot = atomicAdd(a.ring_count, 1u);
        if (slot < (uint32_t)a.ring_cap) a.ring[slot] = crl_episode_record{ep_ret, ep_len, (int32_t)(a.gid0 + (uint32_t)e), a.step};
      }
      ep_ret = 0.0f; ep_len = 0;
    }
    a.ep_return[e] = ep_ret; a.ep_length[e] = ep_len;
  }
  // one atomic set per wave (lanes past num_envs bring the neutral elements)
  st_n = wave_sum(st_n); st_ret = wave_sum(st_ret); st_len = wave_sum(st_len);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) st_max = fmax(st_max, __shfl_xor(st_max, o, 64));
  if ((threadIdx.x & 63) == 0 && st_n > 0.0) {
    atomicAdd(&a.ep_stats[0], st_n); atomicAdd(&a.ep_stats[1], st_ret); atomicAdd(&a.ep_stats[2], st_len);
    atomicMax(reinterpret_cast<unsigned long long*>(&a.ep_stats[3]), ext_max_key(st_max));
  }
}

// The launch of crl_rollout_act_device on the handle's stream. Grid like launch_diag: what the device holds at once (the occupancy query), at most four blocks
// per CU, half of them per role, never more role-block pairs than tiles.
int launch_ext_act(crl_ppo* h, int step, const float* obs_d, const uint8_t* done_d, int32_t* action_d) {
  const int H = h->cfg.hidden, D = h->dc.D, A = h->dc.A, N = h->dc.nt;
  if (D < 1 || D > EXT_OBS_MAX || A < 1 || A > AMAX || (H != 64 && H != 128 && H != 256)) {
    set_error("crl_rollout_act_device: no kernel for this shape (obs_dim <= 64, n_act <= 16, hidden 64 / 128 / 256)");
    return 1;
  }
  const bool w1_lds = ext_lds_bytes(H, D, A, true) <= 160 * 1024;
  const size_t lds = ext_lds_bytes(H, D, A, w1_lds);
  if (lds > 160 * 1024) { set_error("crl_rollout_act_device: this shape needs more LDS than a CU has"); return 1; }
  if (h->diag_cus == 0) {
    hipDeviceProp_t prop;
    CRL_HIP_CHECK(hipGetDeviceProperties(&prop, h->device));
    h->diag_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  }
  if (h->ext_per_cu == 0) {
    int per_cu = 0;
    if (H == 64) CRL_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, ext_act_kernel<64>, 2 * H, lds));
    else if (H == 128) CRL_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, ext_act_kernel<128>, 2 * H, lds));
    else CRL_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, ext_act_kernel<256>, 2 * H, lds));
    h->ext_per_cu = per_cu > 4 ? 4 : per_cu < 1 ? 1 : per_cu;    // the shape is fixed for the life of the handle: asked once, not per step
  }
  const int ntiles = (N + 31) / 32;
  int nrb = h->ext_per_cu * h->diag_cus / 2;
  nrb = nrb > ntiles ? ntiles : nrb;
  nrb = nrb < 1 ? 1 : nrb;
  const size_t off = (size_t)N * (size_t)step;
  ExtActArgs a;
  a.params = h->params; a.Pa = h->Pa;
  a.obs_in = obs_d; a.done_in = done_d; a.action_out = action_d;
  a.obs = h->obs + off * (size_t)D; a.action = h->action + off; a.logprob = h->logprob + off; a.value = h->value + off; a.terminal = h->terminal + off;
  a.D = D; a.A = A; a.N = N; a.w1_lds = w1_lds ? 1 : 0;
  a.seed = h->dc.seed; a.gstep = (uint64_t)h->iteration * (uint64_t)h->dc.k + (uint64_t)step; a.gid0 = h->dc.env_id_offset;
  const dim3 grid(2 * nrb), block(2 * H);
  if (H == 64) hipLaunchKernelGGL(ext_act_kernel<64>, grid, block, lds, h->stream, a);
  else if (H == 128) hipLaunchKernelGGL(ext_act_kernel<128>, grid, block, lds, h->stream, a);
  else hipLaunchKernelGGL(ext_act_kernel<256>, grid, block, lds, h->stream, a);
  CRL_HIP_CHECK(hipGetLastError());
  return 0;
}

int launch_ext_record(crl_ppo* h, int step, const float* reward_d, const float* next_obs_d, const uint8_t* next_done_d) {
  ExtRecArgs a;
  a.reward_in = reward_d; a.next_obs_in = next_obs_d; a.next_done_in = next_done_d;
  a.reward = h->reward + (size_t)h->dc.nt * (size_t)step;
  a.cur_obs = h->cur_obs; a.next_done = h->next_done; a.ep_return = h->ep_return; a.ep_length = h->ep_length; a.ep_stats = h->ep_stats;
  a.ring = h->ep_ring; a.ring_count = h->ep_ring_count; a.ring_cap = h->ep_ring_cap;
  a.D = h->dc.D; a.N = h->dc.nt; a.step = step; a.gid0 = h->dc.env_id_offset;
  hipLaunchKernelGGL(ext_record_kernel, dim3((h->dc.nt + 255) / 256), dim3(256), 0, h->stream, a);
  CRL_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace crl
