// diag.hip — crl_ppo_diagnose: is the update healthy? One read-only, forward-only launch over the RESIDENT rollout buffer (the plain arrays obs / action /
// logprob / value / ret, never the packed records) with the handle's CURRENT parameters: per sample b the new log-probability of the stored action, the
// policy entropy and the new critic value; per block Float64 partial sums of everything approx-KL, clip fraction, entropy and explained variance are made
// of. No reference counterpart (ppo.jl logs its four losses only). One kernel family for the fused 4 / 2 / 64 shape and every layer-wise shape
// (obs_dim <= 64, n_act <= 16, hidden 64 / 128 / 256); no option and no route of the handle is read.
//
// diag_kernel<H>: the eval_rollout_kernel block (H / 32 waves, wave w keeps rows 32w … 32w + 31 of W2 as bf16x3 A fragments in registers, the last three
// k-steps in LDS at 256) made persistent over 32-sample tiles of the flat batch. ROLES ARE BLOCKS: even blocks hold the actor, odd blocks the critic, and
// block 2j / 2j + 1 both walk tiles j, j + nrb, j + 2 nrb, … — every tile gets its actor forward and its critic forward, W2 of one network stays where it is
// for the life of the block, and neither role needs anything of the other: the actor's sums are Σr, Σkl, Σclipped, ΣH, min / max ratio, the critic's
// Σret, Σret², Σ(ret − value), Σ(ret − value)², Σ(ret − v_new), Σ(ret − v_new)². (The price is that a tile's observations are fetched twice.)
//   LDS       the head partials live where the h1 pieces were (one more barrier per tile buys 16 KB at 256, which is what lets obs 64 / act 16 / hidden 256 fit)
//   per tile  the 32 x obs_dim observations, contiguous in the buffer, to LDS (rows padded by four floats: obs_dim up to 64 does not fit a thread's
//             registers next to W2, so layer 1 streams x and W1 from LDS in chunks of four) | barrier | layer 1 on the vector pipe: tanh_fast, bf16x3 split,
//             B-fragment order | barrier | layer 2 on the matrix pipe (f32 accumulation), tanh_fast | barrier | the wave's head partials | barrier | lanes 0-31 of
//             wave 0: one sample each — log-softmax at the stored action, entropy, or the value — then Float64 from the Float32 log-ratio on.
//   exit      wave 0 adds its lanes' sums (butterfly, fixed order) and writes ONE record of six doubles; the host adds the records in block order, so two
//             calls on the same state give the same bits. Nothing B-sized is written unless the caller asked for the per-sample outputs.
#include <vector>

#include "common.hpp"
#include "mlp_x3.hpp"
#include "policy_rt.hpp"
#include "ppo_ctx.hpp"

namespace crl {

constexpr int DIAG_REC = 8;        // doubles per block record (six used)
constexpr int DIAG_OBS_MAX = 64;

struct DiagArgs {
  const float* params; int64_t Pa;   // actor | critic, each W1(H,D) b1(H) W2(H,H) b2(H) W3(n_out,H) b3(n_out), (out,in) column-major
  const float* obs; const int32_t* action; const float* logprob; const float* value; const float* ret;
  int D, A, B;
  int w1_lds;                        // 1 = W1 fits LDS next to everything else, 0 = layer 1 reads it from the parameters (hidden 256 with a wide observation)
  float clip;
  double* part;                      // [gridDim.x][DIAG_REC]
  float* new_logprob; float* new_value;   // [B] each, may be null
};

__host__ __device__ constexpr int diag_ks_lds(int H) { return H == 256 ? 3 : 0; }
// LDS (floats): h1 pieces | W2 fragments of the k-steps that are not in registers | the running sums [6][32 lanes] (Float64) | b1 | b2 (C-fragment order) | b3 |
// W3 (C-fragment order) [n_out][H] | observations [32][D | 1] | W1 [D][H] as the parameters hold it (when it fits)
__host__ __device__ constexpr int diag_lds_fixed(int H) { return 3 * H * 16 + diag_ks_lds(H) * 3 * (H / 32) * 64 * 4 + 6 * 32 * 2 + H + H + AMAX; }
__host__ __device__ constexpr int diag_xs(int D) { return D | 1; }   // odd row stride: the 32 samples of a column sit in 32 banks
static inline size_t diag_lds_bytes(int H, int D, int A, bool w1_lds) {
  return sizeof(float) * (size_t)(diag_lds_fixed(H) + ((A * H + 3) & ~3) + ((32 * diag_xs(D) + 3) & ~3) + (w1_lds ? H * D : 0));
}

__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) { const double u = __shfl_xor(v, o, 64); v = u < v ? u : v; }
  return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) { const double u = __shfl_xor(v, o, 64); v = u > v ? u : v; }
  return v;
}

// eight consecutive hidden rows of one sample: column k of W1 (out, in column-major: rows r … r + 7 are two 16-byte reads, from LDS or from the
// parameters as they lie in HBM) times x[k], k in order
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));   // the critic's W1 starts where the actor's parameters end: 4-byte aligned only
template <typename V>
__device__ __forceinline__ void diag_layer1(const float* wcol, int ldw, const float* x, int D, float (&hv)[8]) {
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
__global__ void __launch_bounds__(2 * H) diag_kernel(DiagArgs a) {
  constexpr int NW = H / 32, KS = H / 16, NT = 2 * H, KL = diag_ks_lds(H), KR = KS - KL;
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int D = a.D, XS = diag_xs(D), B = a.B;
  const int role = blockIdx.x & 1, rb = blockIdx.x >> 1, nrb = gridDim.x >> 1;   // 0 = actor, 1 = critic
  const int A = role ? 1 : a.A;
  bf16x8* h1p = reinterpret_cast<bf16x8*>(sm);                  // [piece][ks][lane]: B fragments of h1, k = 16 ks + 8 (lane >> 5) + j
  bf16x8* wl = h1p + 3 * KS * 64;                               // [KL][piece][wave][lane]: A fragments of the last KL k-steps of W2
  double* acc64 = reinterpret_cast<double*>(sm + 3 * H * 16 + KL * 3 * NW * 64 * 4);   // [6][32]: lane's sums, in LDS so that they cost W2 no registers
  float* b1l = sm + 3 * H * 16 + KL * 3 * NW * 64 * 4 + 6 * 32 * 2;
  float* b2c = b1l + H;                                         // [wave][hf][16]: b2[32 wave + rowmap(r, hf)]
  float* b3l = b2c + H;
  float* zp = sm;                                               // [wave][AMAX][32 samples]: head partials, in the first third of the h1 region once layer 2 has read it
  float* w3c = b3l + AMAX;                                      // [A][wave][hf][16]
  float* xt = w3c + ((a.A * H + 3) & ~3);                       // [32 samples][XS]
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

  // lane's sums (lanes 0-31 of wave 0, nobody else touches them). actor: Σr, Σkl, Σclipped, ΣH, min ratio, max ratio; critic: Σret, Σret², Σ(ret − value),
  // Σ(ret − value)², Σ(ret − v_new), Σ(ret − v_new)²
  if (tid < 32) {
    acc64[tid] = 0.0; acc64[32 + tid] = 0.0; acc64[64 + tid] = 0.0; acc64[96 + tid] = 0.0;
    acc64[128 + tid] = role ? 0.0 : __builtin_inf(); acc64[160 + tid] = role ? 0.0 : -__builtin_inf();
  }
  const double clip = (double)a.clip;

  for (int tile = rb; tile * 32 < B; tile += nrb) {
    const int b0 = tile * 32, nb = B - b0 < 32 ? B - b0 : 32;
    // what the last phase needs of the buffer, asked for in front of the forward: actor = action, old logprob; critic = ret, old value
    const bool mine = w == 0 && lane < nb;
    int act = 0; float f0 = 0.0f, f1 = 0.0f;
    if (mine) {
      if (role == 0) { act = a.action[b0 + lane]; f0 = a.logprob[b0 + lane]; }
      else { f0 = a.ret[b0 + lane]; f1 = a.value[b0 + lane]; }
    }
    for (int idx = tid; idx < 32 * D; idx += NT) {               // obs (D, B): the tile's 32 D floats are contiguous
      const int m = idx / D, k = idx - m * D;
      xt[m * XS + k] = m < nb ? a.obs[(size_t)b0 * D + idx] : 0.0f;
    }
    __syncthreads();
    {                                                            // layer 1: sample m, hidden rows 8 oct … 8 oct + 7
      const int m = tid & 31, g8 = tid >> 5;
#pragma unroll 1
      for (int half = 0; half < 2; ++half) {
        const int oct = g8 + half * (H / 16);
        float hv[8];
        if (a.w1_lds) diag_layer1<f32x4>(w1l + 8 * oct, H, xt + m * XS, D, hv);
        else diag_layer1<f32x4u>(W1 + 8 * oct, H, xt + m * XS, D, hv);
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
    if (mine) {                                                  // one lane per sample; the next tile's first barrier stands between these reads of zp and layer 1's writes of h1
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
      if (role == 0) {
        // softmax_rt's operations in its order (policy_rt.hpp), an action at a time: p = exp(z - m) / Σ, lp = (z - m) - log Σ
        float mx = z[0];
#pragma unroll
        for (int aa = 1; aa < AMAX; ++aa) if (aa < A) mx = fmaxf(mx, z[aa]);
        float se = 0.0f;
#pragma unroll
        for (int aa = 0; aa < AMAX; ++aa) if (aa < A) se += expf(z[aa] - mx);
        const float lse = logf(se);
        float lp_new = (z[0] - mx) - lse;                        // an action outside 0 … n_act - 1 (a buffer nobody filled) selects nothing out of bounds
        double ent = 0.0;
#pragma unroll
        for (int aa = 0; aa < AMAX; ++aa)
          if (aa < A) {
            const float zc = z[aa] - mx, pa = expf(zc) / se, lpa = zc - lse;
            lp_new = aa == act ? lpa : lp_new;
            ent += (double)(-(pa * lpa));                        // the Float32 elements of ppo.jl:41, added in index order
          }
        const float logratio = lp_new - f0;                      // Float32 (ppo.jl:224); Float64 from here on
        const double r = (double)logratio, ratio = exp(r), rm1 = ratio - 1.0;
        double* s = acc64 + lane;
        s[0] += r; s[32] += rm1 - r; s[64] += fabs(rm1) > clip ? 1.0 : 0.0; s[96] += ent;
        s[128] = ratio < s[128] ? ratio : s[128]; s[160] = ratio > s[160] ? ratio : s[160];
        if (a.new_logprob) a.new_logprob[b0 + lane] = lp_new;
      } else {
        const float v_new = z[0];
        const double R = (double)f0, eo = R - (double)f1, en = R - (double)v_new;
        double* s = acc64 + lane;
        s[0] += R; s[32] += R * R; s[64] += eo; s[96] += eo * eo; s[128] += en; s[160] += en * en;
        if (a.new_value) a.new_value[b0 + lane] = v_new;
      }
    }
  }
  if (w == 0) {                                                  // lanes 32-63 bring the neutral element
    const bool lo = lane < 32;
    const double* s = acc64 + (lane & 31);
    const double s0 = wave_sum(lo ? s[0] : 0.0), s1 = wave_sum(lo ? s[32] : 0.0), s2 = wave_sum(lo ? s[64] : 0.0), s3 = wave_sum(lo ? s[96] : 0.0);
    const double m4 = wave_min(lo ? s[128] : __builtin_inf()), m5 = wave_max(lo ? s[160] : -__builtin_inf());
    const double t4 = wave_sum(lo ? s[128] : 0.0), t5 = wave_sum(lo ? s[160] : 0.0);
    if (lane == 0) {
      double* o = a.part + (size_t)blockIdx.x * DIAG_REC;
      o[0] = s0; o[1] = s1; o[2] = s2; o[3] = s3; o[4] = role ? t4 : m4; o[5] = role ? t5 : m5; o[6] = 0.0; o[7] = 0.0;
    }
  }
}

// The derived fields from the raw sums, exactly as include/cleanrl_hip.h states them (no contraction: a host that adds shards' sums and applies the
// same formulas in Float64 gets the same bits).
static void diag_finish(crl_ppo_diag* d) {
#pragma clang fp contract(off)
  const double n = (double)d->n;
  d->old_approx_kl = -d->sum_logratio / n;
  d->approx_kl = d->sum_kl / n;
  d->clipfrac = (double)d->n_clipped / n;
  d->entropy = d->sum_entropy / n;
  const double m_ret = d->sum_ret / n, var_ret = d->sum_ret2 / n - m_ret * m_ret;
  const double m_old = d->sum_res_old / n, var_old = d->sum_res_old2 / n - m_old * m_old;
  const double m_new = d->sum_res_new / n, var_new = d->sum_res_new2 / n - m_new * m_new;
  const double nan = __builtin_nan("");
  d->explained_variance = var_ret > 0.0 ? 1.0 - var_old / var_ret : nan;
  d->explained_variance_new = var_ret > 0.0 ? 1.0 - var_new / var_ret : nan;
}

// The launch of crl_ppo_diagnose: scratch on first use (block records | the two optional per-sample arrays), one kernel, records and per-sample outputs
// back to the host, the records added in block order.
int launch_diag(crl_ppo* h, crl_ppo_diag* out, float* new_logprob, float* new_value) {
  const int H = h->cfg.hidden, D = h->dc.D, A = h->dc.A, B = h->dc.B;
  if (D < 1 || D > DIAG_OBS_MAX || A < 1 || A > AMAX || (H != 64 && H != 128 && H != 256)) {
    set_error("crl_ppo_diagnose: no diagnostics kernel for this shape (obs_dim <= 64, n_act <= 16, hidden 64 / 128 / 256)");
    return 1;
  }
  const bool w1_lds = diag_lds_bytes(H, D, A, true) <= 160 * 1024;
  const size_t lds = diag_lds_bytes(H, D, A, w1_lds);
  if (lds > 160 * 1024) { set_error("crl_ppo_diagnose: this shape needs more LDS than a CU has"); return 1; }
  if (h->diag_cus == 0) {
    hipDeviceProp_t prop;
    CRL_HIP_CHECK(hipGetDeviceProperties(&prop, h->device));
    h->diag_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  }
  // persistent grid: what the device holds at once (registers and LDS decide), at most four blocks per CU, half of them per role, never more than tiles
  int per_cu = 0;
  if (H == 64) CRL_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, diag_kernel<64>, 2 * H, lds));
  else if (H == 128) CRL_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, diag_kernel<128>, 2 * H, lds));
  else CRL_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, diag_kernel<256>, 2 * H, lds));
  per_cu = per_cu > 4 ? 4 : per_cu < 1 ? 1 : per_cu;
  const int ntiles = (B + 31) / 32;
  int nrb = per_cu * h->diag_cus / 2;
  nrb = nrb > ntiles ? ntiles : nrb;
  nrb = nrb < 1 ? 1 : nrb;
  const int nblk = 2 * nrb;
  const bool per_sample = new_logprob || new_value;
  const size_t o_lp = ((size_t)nblk * DIAG_REC * 8 + 255) & ~(size_t)255, o_v = o_lp + (per_sample ? (size_t)B * 4 : 0), total = o_v + (per_sample ? (size_t)B * 4 : 0);
  if (h->diag_ws_bytes < total) {
    CRL_HIP_CHECK(hipStreamSynchronize(h->stream));
    if (h->diag_ws) CRL_HIP_CHECK(hipFree(h->diag_ws));
    h->diag_ws = nullptr; h->diag_ws_bytes = 0;
    CRL_HIP_CHECK(hipMalloc(&h->diag_ws, total));
    h->diag_ws_bytes = total;
  }
  if (!h->diag_ev[0]) { CRL_HIP_CHECK(hipEventCreate(&h->diag_ev[0])); CRL_HIP_CHECK(hipEventCreate(&h->diag_ev[1])); }
  char* ws = static_cast<char*>(h->diag_ws);
  DiagArgs a;
  a.params = h->params; a.Pa = h->Pa;
  a.obs = h->obs; a.action = h->action; a.logprob = h->logprob; a.value = h->value; a.ret = h->ret;
  a.D = D; a.w1_lds = w1_lds ? 1 : 0; a.A = A; a.B = B; a.clip = h->dc.clip;
  a.part = reinterpret_cast<double*>(ws);
  a.new_logprob = new_logprob ? reinterpret_cast<float*>(ws + o_lp) : nullptr;
  a.new_value = new_value ? reinterpret_cast<float*>(ws + o_v) : nullptr;
  const dim3 grid(nblk), block(2 * H);
  CRL_HIP_CHECK(hipEventRecord(h->diag_ev[0], h->stream));
  if (H == 64) hipLaunchKernelGGL(diag_kernel<64>, grid, block, lds, h->stream, a);
  else if (H == 128) hipLaunchKernelGGL(diag_kernel<128>, grid, block, lds, h->stream, a);
  else hipLaunchKernelGGL(diag_kernel<256>, grid, block, lds, h->stream, a);
  CRL_HIP_CHECK(hipGetLastError());
  CRL_HIP_CHECK(hipEventRecord(h->diag_ev[1], h->stream));
  std::vector<double> part((size_t)nblk * DIAG_REC);
  CRL_HIP_CHECK(hipMemcpyAsync(part.data(), ws, part.size() * 8, hipMemcpyDeviceToHost, h->stream));
  if (new_logprob) CRL_HIP_CHECK(hipMemcpyAsync(new_logprob, ws + o_lp, (size_t)B * 4, hipMemcpyDeviceToHost, h->stream));
  if (new_value) CRL_HIP_CHECK(hipMemcpyAsync(new_value, ws + o_v, (size_t)B * 4, hipMemcpyDeviceToHost, h->stream));
  CRL_HIP_CHECK(hipStreamSynchronize(h->stream));   // host buffers are only borrowed for the call
  float ms = 0.0f;
  CRL_HIP_CHECK(hipEventElapsedTime(&ms, h->diag_ev[0], h->diag_ev[1]));
  h->diag_last_ns = (int64_t)((double)ms * 1e6);

  crl_ppo_diag d = {};
  d.n = B;
  double nclip = 0.0;
  d.ratio_min = part[4]; d.ratio_max = part[5];
  for (int blk = 0; blk < nblk; ++blk) {             // block order: the same bits on every call
    const double* p = &part[(size_t)blk * DIAG_REC];
    if ((blk & 1) == 0) {
      d.sum_logratio += p[0]; d.sum_kl += p[1]; nclip += p[2]; d.sum_entropy += p[3];
      d.ratio_min = p[4] < d.ratio_min ? p[4] : d.ratio_min; d.ratio_max = p[5] > d.ratio_max ? p[5] : d.ratio_max;
    } else {
      d.sum_ret += p[0]; d.sum_ret2 += p[1]; d.sum_res_old += p[2]; d.sum_res_old2 += p[3]; d.sum_res_new += p[4]; d.sum_res_new2 += p[5];
    }
  }
  d.n_clipped = (int64_t)nclip;
  diag_finish(&d);
  *out = d;
  return 0;
}

}  // namespace crl
