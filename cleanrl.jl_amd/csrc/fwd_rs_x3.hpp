// fwd_rs_x3.hpp — the register-stationary bf16x3 forward block of one 2 x H network (actor or critic) for a 32-row tile, read straight from the flat
// Flux-ordered parameters: no pack, no option and no route of the handle is involved. Three kernels are built from it: eval_rollout_kernel (eval.hip),
// diag_kernel (diag.hip) and ext_act_kernel (extenv.hip).
//
// A block has H / 32 waves. W2 as bf16x3 A fragments is REGISTER-STATIONARY for every width: wave w keeps rows 32w … 32w + 31 over all H columns, 12
// registers per 16-wide k-step (48 / 96 registers at H = 64 / 128). At 256 the 384 KB of pieces fit neither LDS nor, at 192 registers a lane, the file
// next to everything else: 13 of the 16 k-steps live in registers (156), the last three in LDS (72 KB, written once, read as three 16-byte fragments per
// k-step like the activations).
//   layer 1   on the vector pipe: a thread forms two octets of hidden rows of one row of the tile, then tanh_fast, the bf16x3 split and three 16-byte LDS
//             stores in B-fragment order (rs_l1_epilogue). The dot product is the caller's: eval holds x in registers against padded W1 rows, the
//             role-pair kernels stream columns of W1 (rs_layer1_stream).
//   layer 2   on the matrix pipe (rs_layer2: 6 v_mfma_f32_32x32x16_bf16 per k-step, f32 accumulation), then tanh_fast and the wave's head partials to LDS
//             (rs_head_partials); one lane per row adds them in wave order on top of b3 (rs_logits).
// The pieces stay separate because the kernels place their barriers differently between them: where the head partials alias the h1 pieces (the role-pair
// kernels) a barrier stands between rs_layer2 and rs_head_partials. The H = 256 instantiations sit at the top of the register file; they reach scratch 0
// only through the sched barriers, the opaque bases and the AMAX-strided partials below, so those are part of the block.
//
// The second half of the file is what diag_kernel and ext_act_kernel share beyond the block: ROLES ARE BLOCKS — even blocks hold the actor, odd blocks the
// critic, block 2j / 2j + 1 both walk tiles j, j + nrb, j + 2 nrb, … — with one LDS layout, the column-streaming layer 1 and the host-side shape check,
// LDS size and grid rule.
#pragma once
#include <type_traits>

#include "common.hpp"
#include "mlp_x3.hpp"
#include "policy_rt.hpp"
#include "ppo_ctx.hpp"

namespace crl {

__host__ __device__ constexpr int rs_ks_lds(int H) { return H == 256 ? 3 : 0; }   // k-steps of W2 whose A fragments sit in LDS, not in registers
template <int H>
struct RsGeom { static constexpr int NW = H / 32, KS = H / 16, NT = 2 * H, KL = rs_ks_lds(H), KR = KS - KL; };   // waves, k-steps, threads, k-steps in LDS / in registers
// LDS prefix of every kernel (floats): h1 pieces [piece][ks][lane] (B fragments, k = 16 ks + 8 (lane >> 5) + j) | A fragments of the last KL k-steps of W2 [KL][piece][wave][lane]
__host__ __device__ constexpr int rs_lds_prefix(int H) { return 3 * H * 16 + rs_ks_lds(H) * 3 * (H / 32) * 64 * 4; }

// one network in the flat parameters: W1(H,D) b1(H) W2(H,H) b2(H) W3(n_out,H) b3(n_out), (out,in) column-major
struct RsNet { const float *W1, *b1, *W2, *b2, *W3, *b3; };
template <int H>
__device__ __forceinline__ RsNet rs_net(const float* p, int D, int A) {
  RsNet n;
  n.W1 = p; n.b1 = n.W1 + H * D; n.W2 = n.b1 + H; n.b2 = n.W2 + H * H; n.W3 = n.b2 + H; n.b3 = n.W3 + A * H;
  return n;
}

// b1 as it lies, b2 [wave][hf][16] and W3 [A][wave][hf][16] in C-fragment order (row 32 wave + rowmap(r, hf)), b3 padded to AMAX
template <int H>
__device__ __forceinline__ void rs_stage_head(const RsNet& n, int A, float* b1l, float* b2c, float* w3c, float* b3l, int tid) {
  constexpr int NT = RsGeom<H>::NT;
  for (int idx = tid; idx < H; idx += NT) {
    b1l[idx] = n.b1[idx];
    b2c[idx] = n.b2[32 * (idx >> 5) + rowmap(idx & 15, (idx >> 4) & 1)];
  }
  for (int idx = tid; idx < A * H; idx += NT) {
    const int aa = idx / H, q = idx % H;
    w3c[idx] = n.W3[aa + A * (32 * (q >> 5) + rowmap(q & 15, (q >> 4) & 1))];
  }
  if (tid < AMAX) b3l[tid] = tid < A ? n.b3[tid] : 0.0f;
}

// this wave's 32 rows of W2 as A fragments (row = 32 w + i): the first KR k-steps to wr, the rest to wl
template <int H>
__device__ __forceinline__ void rs_stage_w2(const float* W2, P3 (&wr)[RsGeom<H>::KR], bf16x8* wl, int w, int lane) {
  constexpr int NW = RsGeom<H>::NW, KS = RsGeom<H>::KS, KR = RsGeom<H>::KR;
  const int hf = lane >> 5, i = lane & 31;
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = W2[(32 * w + i) + H * (16 * ks + 8 * hf + j)];
    if (ks < KR) wr[ks] = split3(v);
    else { const P3 p = split3(v); bf16x8* q = wl + ((ks - KR) * 3 * NW + w) * 64 + lane; q[0] = p.hi; q[NW * 64] = p.mid; q[2 * NW * 64] = p.lo; }
    if (ks & 1) __builtin_amdgcn_sched_barrier(0);               // raw rows of two k-steps in flight: the split pieces fill the file
  }
}

// layer-1 epilogue: the pre-activation sums of hidden rows 8 oct … 8 oct + 7 of tile row m -> h1 pieces in B-fragment order
template <int H>
__device__ __forceinline__ void rs_l1_epilogue(float (&hv)[8], const float* b1l, int oct, int m, bf16x8* h1p) {
  constexpr int KS = RsGeom<H>::KS;
#pragma unroll
  for (int j = 0; j < 8; ++j) hv[j] = tanh_fast(hv[j] + b1l[8 * oct + j]);
  const P3 p = split3(hv);
  const int slot = (oct >> 1) * 64 + (oct & 1) * 32 + m;
  h1p[slot] = p.hi; h1p[KS * 64 + slot] = p.mid; h1p[2 * KS * 64 + slot] = p.lo;
}

// layer 2 of the wave's 32 hidden rows for the tile: b2 + W2 h1 in C-fragment order, before the activation
template <int H>
__device__ __forceinline__ f32x16 rs_layer2(const P3 (&wr)[RsGeom<H>::KR], const bf16x8* wl, const bf16x8* h1p, const float* b2c, int w, int lane) {
  constexpr int NW = RsGeom<H>::NW, KS = RsGeom<H>::KS, KR = RsGeom<H>::KR;
  f32x16 acc = load16(b2c + (2 * w + (lane >> 5)) * 16);
  const bf16x8* hb = h1p + lane;
  asm volatile("" : "+v"(hb));                                   // one base per call, constant offsets behind it (see zl below)
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
    if (ks & 1) __builtin_amdgcn_sched_barrier(0);               // at most two k-steps of B fragments in flight
  }
  return acc;
}

// tanh_fast and the wave's share of every head row: zp [wave][AMAX][32 rows]. The partials are laid out for AMAX outputs whatever A is: every address
// is then the block's base plus a constant.
template <int H>
__device__ __forceinline__ void rs_head_partials(const f32x16& acc, const float* w3c, int A, float* zp, int w, int lane) {
  const int hf = lane >> 5, i = lane & 31;
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

// the A head outputs of tile row `lane` (lanes 0-31): b3 plus the partials in wave order, zero beyond A
template <int H>
__device__ __forceinline__ void rs_logits(const float* zp, const float* b3l, int A, int lane, float (&z)[AMAX]) {
  constexpr int NW = RsGeom<H>::NW;
  const float* zl = zp + lane;
  asm volatile("" : "+v"(zl));                                   // formed per call: 128 hoisted addresses would cost W2 its registers
#pragma unroll
  for (int aa = 0; aa < AMAX; ++aa) {
    float v = 0.0f;
    if (aa < A) {
      v = b3l[aa];
      for (int ww = 0; ww < NW; ++ww) v += zl[(ww * AMAX + aa) * 32];
    }
    z[aa] = v;
  }
}

// ------------------------------------------------------------------------------------------------------
// Role-pair kernels (diag_kernel, ext_act_kernel): obs_dim <= 64, n_act <= 16, hidden 64 / 128 / 256.
// LDS (floats): the prefix | `own` floats of the kernel's own | b1 | b2 (C-fragment order) | b3 | W3 (C-fragment order) [n_out][H] | tile rows [32][D | 1] |
// W1 [D][H] as the parameters hold it (when it fits). The head partials live where the h1 pieces were (one more barrier per tile buys 16 KB at 256, which
// is what lets obs 64 / act 16 / hidden 256 fit).
// ------------------------------------------------------------------------------------------------------
constexpr int RS_OBS_MAX = 64;
__host__ __device__ constexpr int rs_xs(int D) { return D | 1; }   // odd row stride: the 32 rows of a column sit in 32 banks
static inline size_t rs_role_lds_bytes(int H, int D, int A, bool w1_lds, int own) {
  return sizeof(float) * (size_t)(rs_lds_prefix(H) + own + H + H + AMAX + ((A * H + 3) & ~3) + ((32 * rs_xs(D) + 3) & ~3) + (w1_lds ? H * D : 0));
}
struct RsRoleLds { bf16x8 *h1p, *wl; float *own, *b1l, *b2c, *b3l, *zp, *w3c, *xt, *w1l; };
template <int H>
__device__ __forceinline__ RsRoleLds rs_role_lds(float* sm, int own, int D, int A_actor) {   // both roles lay W3 out for the actor's n_act
  RsRoleLds l;
  l.h1p = reinterpret_cast<bf16x8*>(sm);
  l.wl = l.h1p + 3 * RsGeom<H>::KS * 64;
  l.own = sm + rs_lds_prefix(H);
  l.b1l = l.own + own;
  l.b2c = l.b1l + H;                                             // [wave][hf][16]: b2[32 wave + rowmap(r, hf)]
  l.b3l = l.b2c + H;
  l.zp = sm;                                                     // [wave][AMAX][32 rows]: in the first third of the h1 region once layer 2 has read it
  l.w3c = l.b3l + AMAX;                                          // [A][wave][hf][16]
  l.xt = l.w3c + ((A_actor * H + 3) & ~3);                       // [32 rows][XS]
  l.w1l = l.xt + ((32 * rs_xs(D) + 3) & ~3);                     // [D][H], column k at 16-byte aligned H k
  return l;
}

// eight consecutive hidden rows of one tile row: column k of W1 (out, in column-major: rows r … r + 7 are two 16-byte reads, from LDS or from the
// parameters as they lie in HBM) times x[k], k in order
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));   // the critic's W1 starts where the actor's parameters end: 4-byte aligned only
template <typename V>
__device__ __forceinline__ void rs_layer1_cols(const float* wcol, int ldw, const float* x, int D, float (&hv)[8]) {
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
// layer 1 of the tile in l.xt: thread tid takes tile row m = tid & 31 and hidden rows 8 oct … 8 oct + 7 for two octets (obs_dim up to 64 does not fit a
// thread's registers next to W2, so x and W1 are streamed); W1 from LDS when it was staged there, else from the parameters
template <int H>
__device__ __forceinline__ void rs_layer1_stream(const RsRoleLds& l, const float* W1, int w1_lds, int D, int tid) {
  const int m = tid & 31, g8 = tid >> 5, XS = rs_xs(D);
#pragma unroll 1
  for (int half = 0; half < 2; ++half) {
    const int oct = g8 + half * (H / 16);
    float hv[8];
    if (w1_lds) rs_layer1_cols<f32x4>(l.w1l + 8 * oct, H, l.xt + m * XS, D, hv);
    else rs_layer1_cols<f32x4u>(W1 + 8 * oct, H, l.xt + m * XS, D, hv);
    rs_l1_epilogue<H>(hv, l.b1l, oct, m, l.h1p);
  }
}

// f(std::integral_constant<int, H>) for the three widths the block exists for (the caller has checked H)
template <typename F>
static inline int rs_dispatch_h(int H, F&& f) {
  if (H == 64) return f(std::integral_constant<int, 64>{});
  if (H == 128) return f(std::integral_constant<int, 128>{});
  return f(std::integral_constant<int, 256>{});
}

// Host side of a role-pair launch. The shape check and the LDS size with the "W1 in LDS if it fits" decision; the caller brings its messages.
static inline int rs_role_shape(const crl_ppo* h, int own, const char* err_shape, const char* err_lds, bool* w1_lds, size_t* lds) {
  const int H = h->cfg.hidden, D = h->dc.D, A = h->dc.A;
  if (D < 1 || D > RS_OBS_MAX || A < 1 || A > AMAX || (H != 64 && H != 128 && H != 256)) { set_error(err_shape); return 1; }
  *w1_lds = rs_role_lds_bytes(H, D, A, true, own) <= 160 * 1024;
  *lds = rs_role_lds_bytes(H, D, A, *w1_lds, own);
  if (*lds > 160 * 1024) { set_error(err_lds); return 1; }
  return 0;
}
// Persistent grid of role-block pairs: what the device holds at once (registers and LDS decide: the occupancy query), at most four blocks per CU …
template <typename K>
static inline int rs_role_per_cu(K kernel, int H, size_t lds, int* per_cu) {
  int n = 0;
  CRL_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel, 2 * H, lds));
  *per_cu = n > 4 ? 4 : n < 1 ? 1 : n;
  return 0;
}
// … half of them per role, never more pairs than 32-row tiles
static inline int rs_role_pairs(const crl_ppo* h, int per_cu, int rows) {
  const int ntiles = (rows + 31) / 32;
  int nrb = per_cu * h->cus / 2;
  nrb = nrb > ntiles ? ntiles : nrb;
  return nrb < 1 ? 1 : nrb;
}

}  // namespace crl
