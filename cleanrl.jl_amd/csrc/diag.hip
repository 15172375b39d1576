// diag.hip — crl_ppo_diagnose: is the update healthy? One read-only, forward-only launch over the RESIDENT rollout buffer (the plain arrays obs / action /
// logprob / value / ret, never the packed records) with the handle's CURRENT parameters: per sample b the new log-probability of the stored action, the
// policy entropy and the new critic value; per block Float64 partial sums of everything approx-KL, clip fraction, entropy and explained variance are made
// of. No reference counterpart (ppo.jl logs its four losses only). One kernel family for the fused 4 / 2 / 64 shape and every layer-wise shape
// (obs_dim <= 64, n_act <= 16, hidden 64 / 128 / 256); no option and no route of the handle is read.
//
// diag_kernel<H>: the register-stationary bf16x3 forward block and the role-pair frame of fwd_rs_x3.hpp (even blocks hold the actor, odd blocks the critic, both
// persistent over 32-sample tiles of the flat batch; the price is that a tile's observations are fetched twice). W2 of one network stays where it is for the
// life of the block, and neither role needs anything of the other: the actor's sums are Σr, Σkl, Σclipped, ΣH, min / max ratio, the critic's
// Σret, Σret², Σ(ret − value), Σ(ret − value)², Σ(ret − v_new), Σ(ret − v_new)².
//   per tile  what the last phase needs of the buffer and the 32 x obs_dim observations, contiguous in the buffer, to LDS | barrier | layer 1 | barrier |
//             layer 2 | barrier | the wave's head partials | barrier | lanes 0-31 of wave 0: one sample each — log-softmax at the stored action, entropy, or
//             the value — then Float64 from the Float32 log-ratio on.
//   exit      wave 0 adds its lanes' sums (butterfly, fixed order) and writes ONE record of six doubles; the host adds the records in block order, so two
//             calls on the same state give the same bits. Nothing B-sized is written unless the caller asked for the per-sample outputs.
#include <vector>

#include "fwd_rs_x3.hpp"

namespace crl {

constexpr int DIAG_REC = 8;        // doubles per block record (six used)
constexpr int DIAG_OWN = 6 * 32 * 2;   // the kernel's own LDS floats: the running sums [6][32 lanes] (Float64)

struct DiagArgs {
  const float* params; int64_t Pa;   // actor | critic, each W1(H,D) b1(H) W2(H,H) b2(H) W3(n_out,H) b3(n_out), (out,in) column-major
  const float* obs; const int32_t* action; const float* logprob; const float* value; const float* ret;
  int D, A, B;
  int w1_lds;                        // 1 = W1 fits LDS next to everything else, 0 = layer 1 reads it from the parameters (hidden 256 with a wide observation)
  float clip;
  double* part;                      // [gridDim.x][DIAG_REC]
  float* new_logprob; float* new_value;   // [B] each, may be null
};

template <int H>
__global__ void __launch_bounds__(2 * H) diag_kernel(DiagArgs a) {
  constexpr int NT = RsGeom<H>::NT, KR = RsGeom<H>::KR;
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int D = a.D, XS = rs_xs(D), B = a.B;
  const int role = blockIdx.x & 1, rb = blockIdx.x >> 1, nrb = gridDim.x >> 1;   // 0 = actor, 1 = critic
  const int A = role ? 1 : a.A;
  const RsRoleLds l = rs_role_lds<H>(sm, DIAG_OWN, D, a.A);
  double* acc64 = reinterpret_cast<double*>(l.own);             // [6][32]: lane's sums, in LDS so that they cost W2 no registers
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const RsNet net = rs_net<H>(a.params + (role ? a.Pa : 0), D, A);

  if (a.w1_lds) for (int idx = tid; idx < H * D; idx += NT) l.w1l[idx] = net.W1[idx];
  rs_stage_head<H>(net, A, l.b1l, l.b2c, l.w3c, l.b3l, tid);
  P3 wr[KR];
  rs_stage_w2<H>(net.W2, wr, l.wl, w, lane);
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
      l.xt[m * XS + k] = m < nb ? a.obs[(size_t)b0 * D + idx] : 0.0f;
    }
    __syncthreads();
    rs_layer1_stream<H>(l, net.W1, a.w1_lds, D, tid);
    __syncthreads();
    const f32x16 acc = rs_layer2<H>(wr, l.wl, l.h1p, l.b2c, w, lane);
    __syncthreads();                                             // every wave has read its h1 fragments: the region now takes the head partials
    rs_head_partials<H>(acc, l.w3c, A, l.zp, w, lane);
    __syncthreads();
    if (mine) {                                                  // one lane per sample; the next tile's first barrier stands between these reads of zp and layer 1's writes of h1
      float z[AMAX];
      rs_logits<H>(l.zp, l.b3l, A, lane, z);
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
  bool w1_lds; size_t lds;
  if (rs_role_shape(h, DIAG_OWN, "crl_ppo_diagnose: no diagnostics kernel for this shape (obs_dim <= 64, n_act <= 16, hidden 64 / 128 / 256)",
                    "crl_ppo_diagnose: this shape needs more LDS than a CU has", &w1_lds, &lds)) return 1;
  int per_cu = 0;
  if (rs_dispatch_h(H, [&](auto hc) { return rs_role_per_cu(diag_kernel<decltype(hc)::value>, H, lds, &per_cu); })) return 1;
  const int nblk = 2 * rs_role_pairs(h, per_cu, B);
  const bool per_sample = new_logprob || new_value;
  const size_t o_lp = ((size_t)nblk * DIAG_REC * 8 + 255) & ~(size_t)255, o_v = o_lp + (per_sample ? (size_t)B * 4 : 0), total = o_v + (per_sample ? (size_t)B * 4 : 0);
  if (ensure_scratch(h, &h->diag_ws, &h->diag_ws_bytes, total)) return 1;
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
  rs_dispatch_h(H, [&](auto hc) { hipLaunchKernelGGL(diag_kernel<decltype(hc)::value>, grid, block, lds, h->stream, a); return 0; });
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
