// wide_wgrad.hpp — weight gradient of a hidden layer of the layer-wise path: dW[n, k] = Σ_m dY[n, m]·X[k, m], db[n] = Σ_m dY[n, m] over one sample
// chunk (ppo.jl:202 pullback of Dense(H, H)); the per-chunk partials are summed in fixed order afterwards (wide_reduce_kernel). Included by wide.hip
// behind wide_fused.hpp (lds_dma16*, lds_addr_of, load_obs8, the stamp macros; X3ROW, split3x4, split2x4, pow2_scale come from wide.hip itself).
//   wide_wgrad_kernel<1|2>        f32 MFMA: hidden 64 / 128, or wide_gemm = 0
//   wide_wgrad_x3_kernel<4>       bf16x3 (wide_gemm = 1)
//   wide_wgrad_x2_kernel<4>       fp16x2 on the stored h1 (BWD_LAYERS, WGRAD_H1); <4, true>: h1 regenerated, 256 x 128 tiles (WGRAD_GEN_128)
//   wide_wgrad_gen_kernel<8|16>   fp16x2, h1 regenerated, the whole 256 x 256 tile per block (WGRAD_GEN_256)
//   wide_wgrad_split_kernel<8|16> the same from the backward's split δ2 planes (WGRAD_SPLIT, the default at C3)
// What the kernels share is stated once, as pieces: block_max, wgrad_chunk_scale, quad_row / stage_d2_slab, RegenW1 + regen_h1_product +
// regen_h1_store, load_frag, acc_quad / wgrad_store_partial, wgrad_bias_fold. What differs for recorded reasons stays in the kernels: the fetch
// schedules (and the masking that goes with them), every wait and barrier, the stamp points. These kernels sit at the edge of the register file
// (DESIGN.md §3b): the pieces take vectors by value, and a kernel whose registers or static instruction mix moved with a piece keeps its own
// statement of it — profiles/wgrad_refactor_cost.txt lists which (wide_wgrad_gen_kernel: h1 store and partial write-out; wide_wgrad_x2_kernel: staging).
#pragma once

namespace crl {

struct WgradArgs {
  const float* dY; const float* X; int H; int M; int chunk; float* pW; float* pB;
  // x2 kernel: the head cotangent (bz, ld bld, bA live rows) and wmax bound |δ2| per sample — the block's scale comes from them
  const float* bz; int bld; int bA; const float* wmax;
  // GEN flavour (wide_wgrad_x2_kernel<4, true>): X is not read — h1 is regenerated from the observations (as in wide_wgrad_gen_kernel)
  const float* obs = nullptr; const int32_t* perm = nullptr; int D = 0; const float* W1f = nullptr; const float* w1sc = nullptr;
};

// ------------------------------------------------------------------------------------------------------
// The pieces
// ------------------------------------------------------------------------------------------------------
// maximum over the block's NW waves: wave butterfly, one LDS slot per wave, two barriers (red is free again behind the second)
template <int NW>
__device__ __forceinline__ float block_max(float v, float* red, int lane, int wave) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = __builtin_fmaxf(v, __shfl_xor(v, o, 64));
  if (lane == 0) red[wave] = v;
  __syncthreads();
  v = red[0];
  for (int w8 = 1; w8 < NW; ++w8) v = __builtin_fmaxf(v, red[w8]);
  __syncthreads();
  return v;
}

// The reduction runs over samples, so dY = δ2 needs ONE power-of-two scale for everything a block accumulates — and a block owns one sample chunk
// whose partial is unscaled before it is written, so the scale is the block's own: G = 2^(14 − ⌈log2 max_m bound_m⌉) over the chunk's samples,
// bound_m = Σ_a |δ3[a, m]|·wmax[a] (≥ every |δ2[·, m]|; a few KB of reads, no pass over δ2).
template <int NT>
__device__ __forceinline__ void wgrad_chunk_scale(const float* bz, int bld, int bA, const float* wmax, int c0, int c1, float* red, int lane, int wave, float& G, float& Ginv) {
  const int tid = threadIdx.x;
  float bmax = 0.0f;
  for (int m = c0 + tid; m < c1; m += NT) {
    float bound = 0.0f;
    for (int q2 = 0; q2 < bA; ++q2) bound = __builtin_fmaf(__builtin_fabsf(bz[(size_t)bld * m + q2]), wmax[q2], bound);
    bmax = __builtin_fmaxf(bmax, bound);
  }
  pow2_scale(block_max<NT / 64>(bmax, red, lane, wave), G, Ginv);
}

// The staging loads of the sample-reduced products are 4×4 blocks per thread (4 consecutive rows × 4 consecutive samples: four 16-B loads), which
// a thread transposes in its own registers: row e's four samples sit in component e of the four loads
__device__ __forceinline__ f32x4 quad_row(const f32x4 (&r)[4], int e) {
  f32x4 v;
  v[0] = r[0][e]; v[1] = r[1][e]; v[2] = r[2][e]; v[3] = r[3][e];
  return v;
}
// a δ2 slab under the block's scale G → fp16x2 pieces, [piece][rows][X3ROW] with [unit][sample] rows: one ds_write_b64 per row and piece
__device__ __forceinline__ void stage_d2_slab(const f32x4 (&yr)[4], float G, _Float16* Yp, int rows, int rrow, int sg) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    uint2 hh, ll;
    split2x4(quad_row(yr, e), G, hh, ll);
    *reinterpret_cast<uint2*>(Yp + (0 * rows + rrow + e) * X3ROW + 4 * sg) = hh;
    *reinterpret_cast<uint2*>(Yp + (1 * rows + rrow + e) * X3ROW + 4 * sg) = ll;
  }
}

// h1 REGENERATED on the CU: a wave produces one 32-unit tile of the h1 slab per 32 samples with ONE fp16x2 product on the matrix pipe —
// mfma(x-fragment, W1ᵀ-fragment): rows = samples, columns = units, i.e. lane = unit, registers = 4 consecutive samples per quad, exactly the
// [unit][sample] image the K = samples product wants — then tanh, split, 8-byte LDS stores.
// The wave's tile: its W1ᵀ B-fragment (= the A-fragment of W1 the forward's producers use), bias and the fragments' inverse scale stay in registers
struct RegenW1 { P2 w1b; float b1u, w1un; };
__device__ __forceinline__ void regen_w1_load(RegenW1& r, const float* W1f, const float* w1sc, int tile, int lane) {
  const f16x8* wf = reinterpret_cast<const f16x8*>(W1f) + (tile * 2) * 64 + lane;
  r.w1b.hi = wf[0]; r.w1b.lo = wf[64];
  r.b1u = W1f[4096 + 32 * tile + (lane & 31)]; r.w1un = w1sc[1];
}
// x0, x1: the observation half (k = 8hf …) of sample (lane & 31) of the slab, zero beyond obs_dim. The slab's observations are scaled by ONE power
// of two (the scale must not vary along the rows of the result: they are the registers here); un1 takes it out again together with W1's.
// The limit of that: the slab's largest value lands at [2^14, 2^15) and a pair of pieces resolves 2^-24 absolute, so a sample whose observations are
// 2^k below the largest keeps all 22 bits up to k = 16 and 38 − k beyond. Within 1e-5 of Float64 on dW2 up to k = 16; 3.5e-5 at k = 24, 8e-3 at
// 32, nothing left at 40 (tests/test_gpu_wide_range.py; wide_fuse = 0 and wide_gemm = 1 / 0 have no such limit).
// (Operands and result by value: with the arrays handed over by reference the compiler's register assignment in the kernels changes.)
struct H1Prod { f32x16 c16; float un1; };
__device__ __forceinline__ H1Prod regen_h1_product(const f32x4 x0, const f32x4 x1, const P2 w1b, float w1un) {
  float mx = 0.0f;
#pragma unroll
  for (int c = 0; c < 4; ++c) mx = __builtin_fmaxf(mx, __builtin_fabsf(x0[c]));
#pragma unroll
  for (int c = 0; c < 4; ++c) mx = __builtin_fmaxf(mx, __builtin_fabsf(x1[c]));
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) mx = __builtin_fmaxf(mx, __shfl_xor(mx, o, 64));
  float sx, ix;
  pow2_scale(mx, sx, ix);
  float v[8];
#pragma unroll
  for (int c = 0; c < 4; ++c) { v[c] = x0[c] * sx; v[4 + c] = x1[c] * sx; }
  const P2 xa = split2(v);
  H1Prod r;
#pragma unroll
  for (int r16 = 0; r16 < 16; ++r16) r.c16[r16] = 0.0f;
  r.c16 = mfma_x2(xa, w1b, r.c16);                             // rows = samples (registers), columns = units (lanes)
  r.un1 = ix * w1un;
  return r;
}
// tanh, split, stores into the [piece][rows][X3ROW] image at row `unit`. PER_SAMPLE: times the samples' factors tc[·]·iinv (the split kernel)
template <bool PER_SAMPLE>
__device__ __forceinline__ void regen_h1_store(const f32x16& c16, float un1, float b1u, const float* tc, float iinv, _Float16* Xp, int rows, int unit, int hf) {
#pragma unroll
  for (int g = 0; g < 4; ++g) {                               // registers 4g … 4g + 3 = samples 8g + 4hf + {0..3} of the slab
    f32x4 hv;
#pragma unroll
    for (int e = 0; e < 4; ++e) hv[e] = tanh_exp2_arg(__builtin_fmaf(c16[4 * g + e], un1, b1u), X2_ACT_SCALE);
    if (PER_SAMPLE) hv = hv * (*reinterpret_cast<const f32x4*>(tc + 8 * g + 4 * hf) * iinv);
    uint2 hh, ll;
    split2x4(hv, 1.0f, hh, ll);
    *reinterpret_cast<uint2*>(Xp + (0 * rows + unit) * X3ROW + 8 * g + 4 * hf) = hh;
    *reinterpret_cast<uint2*>(Xp + (1 * rows + unit) * X3ROW + 8 * g + 4 * hf) = ll;
  }
}

// one fp16x2 fragment of the slab product's k-step ks (of the slab's two): the 32-row tile `tile` of a [piece][rows][X3ROW] image
__device__ __forceinline__ P2 load_frag(const _Float16* P, int rows, int tile, int ks, int j, int hf) {
  const int off = (tile * 32 + j) * X3ROW + 16 * ks + 8 * hf;
  P2 f;
  f.hi = *reinterpret_cast<const f16x8*>(P + 0 * rows * X3ROW + off);
  f.lo = *reinterpret_cast<const f16x8*>(P + 1 * rows * X3ROW + off);
  return f;
}

// rows 8g + 4hf … + 3 of the lane's column of an accumulator tile, as they go into the chunk's [k][n] partial; SCALED: times un on the way
template <bool SCALED>
__device__ __forceinline__ f32x4 acc_quad(const f32x16 acc, int g, float un) {
  f32x4 o;
  if (SCALED) { o[0] = acc[4 * g] * un; o[1] = acc[4 * g + 1] * un; o[2] = acc[4 * g + 2] * un; o[3] = acc[4 * g + 3] * un; }
  else { o[0] = acc[4 * g]; o[1] = acc[4 * g + 1]; o[2] = acc[4 * g + 2]; o[3] = acc[4 * g + 3]; }
  return o;
}
// the wave's NX × NY accumulator tiles (first rows n0 of dY, k0 of X) into the chunk's [k][n] partial (SCALED = false never multiplies)
template <int NX, int NY, bool SCALED>
__device__ __forceinline__ void wgrad_store_partial(const f32x16 (&acc)[NX][NY], float un, float* pw, int H, int n0, int k0, int j, int hf) {
#pragma unroll
  for (int x = 0; x < NX; ++x)
#pragma unroll
    for (int y = 0; y < NY; ++y) {
      const int k = k0 + 32 * y + j;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int n = n0 + 32 * x + 8 * g + 4 * hf;
        *reinterpret_cast<f32x4*>(pw + (size_t)H * k + n) = acc_quad<SCALED>(acc[x][y], g, un);
      }
    }
}

// db: fold the 8 sample groups of a row quad (lanes 8·ql + sg) in group order; lanes with sg = 0 own the four rows at pb
__device__ __forceinline__ void wgrad_bias_fold(const f32x4 bacc, float* scr, int tid, int sg, float* pb) {
  *reinterpret_cast<f32x4*>(scr + 4 * tid) = bacc;
  __syncthreads();
  if (sg == 0) {
    f32x4 sacc = bacc;
    for (int q = 1; q < 8; ++q) sacc += *reinterpret_cast<const f32x4*>(scr + 4 * (tid + q));
    *reinterpret_cast<f32x4*>(pb) = sacc;
  }
}

// ------------------------------------------------------------------------------------------------------
// f32 MFMA. Block = one (64·TW)² output tile × one chunk; both operands are (feature, sample) arrays, so a 32-sample slab of
// either is BT contiguous floats per sample and the MFMA operands are read feature-fastest from LDS.
// ------------------------------------------------------------------------------------------------------
template <int TW>
__global__ void __launch_bounds__(256) wide_wgrad_kernel(WgradArgs a) {
  constexpr int BT = 64 * TW;
  __shared__ __attribute__((aligned(16))) float Yl[32 * BT];
  __shared__ __attribute__((aligned(16))) float Xl[32 * BT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 31, hf = lane >> 5;
  const int nb = a.H / BT, tnb = blockIdx.y % nb, tkb = blockIdx.y / nb;
  const int n0 = tnb * BT, kk0 = tkb * BT;
  const int wn = wave & 1, wk = wave >> 1;
  f32x16 acc[TW][TW];
#pragma unroll
  for (int x = 0; x < TW; ++x)
#pragma unroll
    for (int y = 0; y < TW; ++y)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[x][y][r] = 0.0f;
  f32x4 bacc = {0.0f, 0.0f, 0.0f, 0.0f};
  const int c0 = blockIdx.x * a.chunk;
  const int c1 = (c0 + a.chunk) < a.M ? (c0 + a.chunk) : a.M;
  // thread t stages float4 slots t, t+256, … of the [32][BT] slab: slot → (sample p / BT, rows p % BT); BT·8 slots / 256
  // threads = BT/32 per thread, each a fixed (sample offset, row) pair — pointers are set up once
  constexpr int NU = BT / 32;
  int soff[NU], mmu[NU];   // element offset of the slot inside a slab (rows relative to the block's first row)
#pragma unroll
  for (int u = 0; u < NU; ++u) {
    const int p = 4 * (tid + 256 * u), mm = p / BT, n = p - mm * BT;
    mmu[u] = mm;
    soff[u] = a.H * mm + n;
  }
  const float* ybase = a.dY + (size_t)a.H * c0 + n0;
  const float* xbase = a.X + (size_t)a.H * c0 + kk0;
  const bool do_bias = (tkb == 0) && a.pB;
  const f32x4 zero4 = {0.0f, 0.0f, 0.0f, 0.0f};
  f32x4 yr[NU], xr[NU];
  auto fetch = [&](int m) {
    const int mv = c1 - m;   // samples left in the chunk
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      const bool ok = mmu[u] < mv;
      const size_t off = (size_t)a.H * (m - c0);   // wave-uniform
      yr[u] = ok ? *reinterpret_cast<const f32x4*>(ybase + off + soff[u]) : zero4;
      xr[u] = ok ? *reinterpret_cast<const f32x4*>(xbase + off + soff[u]) : zero4;
    }
  };
  if (c0 < c1) fetch(c0);
  for (int m = c0; m < c1; m += 32) {
    if (m != c0) __syncthreads();
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      *reinterpret_cast<f32x4*>(Yl + 4 * (tid + 256 * u)) = yr[u];
      *reinterpret_cast<f32x4*>(Xl + 4 * (tid + 256 * u)) = xr[u];
      if (do_bias) bacc += yr[u];
    }
    __syncthreads();
    if (m + 32 < c1) fetch(m + 32);
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      const int mm = 2 * s + hf;
      float av[TW], bv[TW];
#pragma unroll
      for (int x = 0; x < TW; ++x) av[x] = Yl[mm * BT + (wn * TW + x) * 32 + j];
#pragma unroll
      for (int y = 0; y < TW; ++y) bv[y] = Xl[mm * BT + (wk * TW + y) * 32 + j];
#pragma unroll
      for (int x = 0; x < TW; ++x)
#pragma unroll
        for (int y = 0; y < TW; ++y) acc[x][y] = mfma32(av[x], bv[y], acc[x][y]);
    }
  }
  __syncthreads();
  wgrad_store_partial<TW, TW, false>(acc, 1.0f, a.pW + (size_t)blockIdx.x * a.H * a.H, a.H, n0 + wn * TW * 32, kk0 + wk * TW * 32, j, hf);
  if (tkb == 0 && a.pB) {
    // thread t always staged rows (4t mod BT)..+3: fold the 1024/BT threads that share a row quad, in thread order
    *reinterpret_cast<f32x4*>(Yl + 4 * tid) = bacc;
    __syncthreads();
    if (tid < BT) {
      const int quad = tid >> 2, e = tid & 3;
      float s = 0.0f;
      for (int q = 0; q < 1024 / BT; ++q) s += Yl[4 * (quad + (BT / 4) * q) + e];
      a.pB[(size_t)blockIdx.x * a.H + n0 + tid] = s;
    }
  }
}

// ------------------------------------------------------------------------------------------------------
// The same weight gradient on the bf16 matrix pipe (bf16x3) for 256-wide layers. The reduction runs over SAMPLES, so an
// MFMA operand needs 8 consecutive samples of one row — the strided direction of the (feature, sample) arrays. The
// staging loads are therefore the 4×4 blocks of quad_row: each row's 4 samples are split into bf16 hi/mid/lo and
// written with one ds_write_b64 per piece into row-major [row][sample] LDS images (row stride 80 B: conflict-free
// b128 fragment reads). No f32 copy of the slab ever exists in LDS.
// ------------------------------------------------------------------------------------------------------
template <int WNB>   // output tile = (64·WNB rows of dY) × (128 rows of X); 2·WNB waves, each 2×2 MFMA tiles
__global__ void __launch_bounds__(128 * WNB) wide_wgrad_x3_kernel(WgradArgs a) {
  constexpr int BN = 64 * WNB, BK = 128;
  extern __shared__ __attribute__((aligned(16))) unsigned char smw[];
  __bf16* Yp = reinterpret_cast<__bf16*>(smw);                 // [3][BN][X3ROW]
  __bf16* Xp = Yp + 3 * BN * X3ROW;                            // [3][BK][X3ROW]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 31, hf = lane >> 5;
  const int nbn = a.H / BN;
  const int tnb = blockIdx.y % nbn, tkb = blockIdx.y / nbn;
  const int n0 = tnb * BN, kk0 = tkb * BK;
  const int wn = wave % WNB, wk = wave / WNB;
  f32x16 acc[2][2];
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[x][y][r] = 0.0f;
  const int c0 = blockIdx.x * a.chunk;
  const int c1 = (c0 + a.chunk) < a.M ? (c0 + a.chunk) : a.M;
  // staging role of this thread: rows 32·wave + 4·ql .. +3, samples 4·sg .. +3 of the slab's 32 (X: the first 4 waves).
  // sg on the low lane bits: the 16 lanes one ds_write_b64 group covers are then 8 sample groups (16 consecutive dwords)
  // of two row quads (80 dwords apart = 16 banks) — conflict-free; with the row quad on the low bits the same store
  // was 4-way conflicted (SQ_LDS_BANK_CONFLICT 21 % of the kernel's CU cycles)
  const int sg = lane & 7, ql = lane >> 3;
  const int rrow = 32 * wave + 4 * ql;
  const bool stage_x = wave < BK / 32;
  const float* ybase = a.dY + (size_t)a.H * c0 + n0 + rrow;
  const float* xbase = a.X + (size_t)a.H * c0 + kk0 + rrow;
  const bool do_bias = (tkb == 0) && a.pB;
  const f32x4 zero4 = {0.0f, 0.0f, 0.0f, 0.0f};
  f32x4 yr[4], xr[4], bacc = zero4;
  auto fetch = [&](int m) {
    const size_t off = (size_t)a.H * (m - c0 + 4 * sg);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bool ok = m + 4 * sg + e < c1;
      yr[e] = ok ? *reinterpret_cast<const f32x4*>(ybase + off + (size_t)a.H * e) : zero4;
      xr[e] = (ok && stage_x) ? *reinterpret_cast<const f32x4*>(xbase + off + (size_t)a.H * e) : zero4;
    }
  };
  auto stage3 = [&](const f32x4 (&r)[4], int e, __bf16* P, int rows) {
    uint2 h, mm, l;
    split3x4(quad_row(r, e), h, mm, l);
    *reinterpret_cast<uint2*>(P + (0 * rows + rrow + e) * X3ROW + 4 * sg) = h;
    *reinterpret_cast<uint2*>(P + (1 * rows + rrow + e) * X3ROW + 4 * sg) = mm;
    *reinterpret_cast<uint2*>(P + (2 * rows + rrow + e) * X3ROW + 4 * sg) = l;
  };
  if (c0 < c1) fetch(c0);
  for (int m = c0; m < c1; m += 32) {
    if (m != c0) __syncthreads();
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      stage3(yr, e, Yp, BN);
      if (stage_x) stage3(xr, e, Xp, BK);
    }
    if (do_bias) bacc += (yr[0] + yr[1]) + (yr[2] + yr[3]);
    __syncthreads();
    if (m + 32 < c1) fetch(m + 32);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      P3 af[2], bf[2];
#pragma unroll
      for (int x = 0; x < 2; ++x) {
        const int off = ((wn * 2 + x) * 32 + j) * X3ROW + 16 * ks + 8 * hf;
        af[x].hi = *reinterpret_cast<const bf16x8*>(Yp + 0 * BN * X3ROW + off);
        af[x].mid = *reinterpret_cast<const bf16x8*>(Yp + 1 * BN * X3ROW + off);
        af[x].lo = *reinterpret_cast<const bf16x8*>(Yp + 2 * BN * X3ROW + off);
      }
#pragma unroll
      for (int y = 0; y < 2; ++y) {
        const int off = ((wk * 2 + y) * 32 + j) * X3ROW + 16 * ks + 8 * hf;
        bf[y].hi = *reinterpret_cast<const bf16x8*>(Xp + 0 * BK * X3ROW + off);
        bf[y].mid = *reinterpret_cast<const bf16x8*>(Xp + 1 * BK * X3ROW + off);
        bf[y].lo = *reinterpret_cast<const bf16x8*>(Xp + 2 * BK * X3ROW + off);
      }
#pragma unroll
      for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y) acc[x][y] = mfma_x3(af[x], bf[y], acc[x][y]);
    }
  }
  __syncthreads();
  wgrad_store_partial<2, 2, false>(acc, 1.0f, a.pW + (size_t)blockIdx.x * a.H * a.H, a.H, n0 + wn * 64, kk0 + wk * 64, j, hf);
  if (do_bias) wgrad_bias_fold(bacc, reinterpret_cast<float*>(smw), tid, sg, a.pB + (size_t)blockIdx.x * a.H + n0 + rrow);
}

// ------------------------------------------------------------------------------------------------------
// The same weight gradient as fp16x2 (mlp_x2.hpp): δ2 under the block's scale of wgrad_chunk_scale, X = h1 under the static 2^14.
// ------------------------------------------------------------------------------------------------------
template <int WNB, bool GEN = false>
__global__ void __launch_bounds__(128 * WNB) wide_wgrad_x2_kernel(WgradArgs a) {
  constexpr int BN = 64 * WNB, BK = 128, NT = 128 * WNB;
  extern __shared__ __attribute__((aligned(16))) unsigned char smw[];
  _Float16* Yp = reinterpret_cast<_Float16*>(smw);             // [2][BN][X3ROW]
  _Float16* Xp = Yp + 2 * BN * X3ROW;                          // [2][BK][X3ROW]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 31, hf = lane >> 5;
  const int nbn = a.H / BN;
  const int tnb = blockIdx.y % nbn, tkb = blockIdx.y / nbn;
  const int n0 = tnb * BN, kk0 = tkb * BK;
  const int wn = wave % WNB, wk = wave / WNB;
  const int c0 = blockIdx.x * a.chunk;
  const int c1 = (c0 + a.chunk) < a.M ? (c0 + a.chunk) : a.M;
  float G, Ginv;
  wgrad_chunk_scale<NT>(a.bz, a.bld, a.bA, a.wmax, c0, c1, reinterpret_cast<float*>(smw), lane, wave, G, Ginv);
  f32x16 acc[2][2];
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[x][y][r] = 0.0f;
  const int sg = lane & 7, ql = lane >> 3;                     // (staging roles: as wide_wgrad_x3_kernel)
  const int rrow = 32 * wave + 4 * ql;
  const bool stage_x = wave < BK / 32;
  const float* ybase = a.dY + (size_t)a.H * c0 + n0 + rrow;
  const float* xbase = GEN ? nullptr : a.X + (size_t)a.H * c0 + kk0 + rrow;
  const bool do_bias = (tkb == 0) && a.pB;
  const f32x4 zero4 = {0.0f, 0.0f, 0.0f, 0.0f};
  f32x4 yr[4], xr[4], bacc = zero4;
  // GEN: waves 0-3 regenerate their 32-unit tile of the h1 slab
  RegenW1 w1; w1.b1u = 0.0f; w1.w1un = 0.0f;
  float xo[8];
  int src_nx = 0;
  if (GEN && stage_x) {
    src_nx = (c0 + j < c1) ? (a.perm ? a.perm[c0 + j] : c0 + j) : 0;
    regen_w1_load(w1, a.W1f, a.w1sc, kk0 / 32 + wave, lane);
  }
  auto fetch = [&](int m) {
    const size_t off = (size_t)a.H * (m - c0 + 4 * sg);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bool ok = m + 4 * sg + e < c1;
      yr[e] = ok ? *reinterpret_cast<const f32x4*>(ybase + off + (size_t)a.H * e) : zero4;
      if (!GEN) xr[e] = (ok && stage_x) ? *reinterpret_cast<const f32x4*>(xbase + off + (size_t)a.H * e) : zero4;
    }
    if (GEN && stage_x) {
      // the observation row index of this slab's sample was loaded a slab earlier (a dependent perm → obs chain inside one fetch stalls the
      // wave for a memory round trip before its MFMAs: 497 instead of ≈300 us per launch)
      const bool ok = m + j < c1;
#pragma unroll
      for (int c = 0; c < 8; ++c) xo[c] = 0.0f;
      load_obs8(a.obs, (size_t)src_nx, a.D, 8 * hf, ok, xo);
      const int mn = m + 32 + j;
      src_nx = mn < c1 ? (a.perm ? a.perm[mn] : mn) : 0;
    }
  };
  if (c0 < c1) fetch(c0);
  for (int m = c0; m < c1; m += 32) {
    if (m != c0) __syncthreads();
    if (GEN) stage_d2_slab(yr, G, Yp, BN, rrow, sg);
    else {
      // δ2 and the stored h1 row by row (this flavour's own statement of the staging: the compiler pairs the ds_write_b64 of the two images, and
      // through two calls of stage_d2_slab it paired them differently, profiles/wgrad_refactor_cost.txt)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        uint2 hh, ll;
        split2x4(quad_row(yr, e), G, hh, ll);
        *reinterpret_cast<uint2*>(Yp + (0 * BN + rrow + e) * X3ROW + 4 * sg) = hh;
        *reinterpret_cast<uint2*>(Yp + (1 * BN + rrow + e) * X3ROW + 4 * sg) = ll;
        if (stage_x) {
          split2x4(quad_row(xr, e), X2_ACT_SCALE, hh, ll);
          *reinterpret_cast<uint2*>(Xp + (0 * BK + rrow + e) * X3ROW + 4 * sg) = hh;
          *reinterpret_cast<uint2*>(Xp + (1 * BK + rrow + e) * X3ROW + 4 * sg) = ll;
        }
      }
    }
    if (GEN && stage_x) {
      f32x4 x0, x1;
      x0[0] = xo[0]; x0[1] = xo[1]; x0[2] = xo[2]; x0[3] = xo[3]; x1[0] = xo[4]; x1[1] = xo[5]; x1[2] = xo[6]; x1[3] = xo[7];
      const H1Prod hp = regen_h1_product(x0, x1, w1.w1b, w1.w1un);
      regen_h1_store<false>(hp.c16, hp.un1, w1.b1u, nullptr, 0.0f, Xp, BK, 32 * wave + j, hf);
    }
    if (do_bias) bacc += (yr[0] + yr[1]) + (yr[2] + yr[3]);
    __syncthreads();
    if (m + 32 < c1) fetch(m + 32);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      P2 af[2], bf[2];
#pragma unroll
      for (int x = 0; x < 2; ++x) af[x] = load_frag(Yp, BN, wn * 2 + x, ks, j, hf);
#pragma unroll
      for (int y = 0; y < 2; ++y) bf[y] = load_frag(Xp, BK, wk * 2 + y, ks, j, hf);
#pragma unroll
      for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y) acc[x][y] = mfma_x2(af[x], bf[y], acc[x][y]);
    }
  }
  __syncthreads();
  wgrad_store_partial<2, 2, true>(acc, Ginv * (1.0f / X2_ACT_SCALE), a.pW + (size_t)blockIdx.x * a.H * a.H, a.H, n0 + wn * 64, kk0 + wk * 64, j, hf);
  if (do_bias) wgrad_bias_fold(bacc, reinterpret_cast<float*>(smw), tid, sg, a.pB + (size_t)blockIdx.x * a.H + n0 + rrow);
}

// ======================================================================================================================================
// The fp16x2 weight gradient with a block owning the whole 256 x 256 tile (2 x 4 MFMA tiles per wave, 128 accumulator registers).
// wide_wgrad_x2_kernel reads both [256 x M] operands from HBM (δ2 twice: two 128-column blocks); this one reads δ2 ONCE and never reads h1:
// every wave regenerates one 32-unit tile of the slab (RegenW1). With it the forward pass no longer stores h1 at all: 2.1 GB of HBM traffic
// per optimiser step less (h1 written once, read once per network).
// ======================================================================================================================================
struct WgradGenArgs {
  const float* dY; const float* obs; const int32_t* perm; int D;
  const float* W1f; const float* w1sc;
  const float* bz; int bld; int bA; const float* wmax;
  float* pW; float* pB; int M; int chunk;
};

template <int DP>
__device__ __forceinline__ void wide_wgrad_gen_body(const WgradGenArgs& a) {
  constexpr int H = 256, NT = 512;
  extern __shared__ __attribute__((aligned(16))) unsigned char smw[];
  _Float16* Yp = reinterpret_cast<_Float16*>(smw);             // [2][256][X3ROW]: δ2·G pieces, [unit][sample]
  _Float16* Xp = Yp + 2 * H * X3ROW;                           // [2][256][X3ROW]: 2^14·h1 pieces, [unit][sample]
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), j = lane & 31, hf = lane >> 5;
  const int wn = wave & 3, wk = wave >> 2;
  const int c0 = blockIdx.x * a.chunk;
  const int c1 = (c0 + a.chunk) < a.M ? (c0 + a.chunk) : a.M;
  float G, Ginv;
  wgrad_chunk_scale<NT>(a.bz, a.bld, a.bA, a.wmax, c0, c1, reinterpret_cast<float*>(smw), lane, wave, G, Ginv);
  RegenW1 w1;                                                  // this wave's h1 tile: units 32·wave …
  regen_w1_load(w1, a.W1f, a.w1sc, wave, lane);
  f32x16 acc[2][4];
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 4; ++y)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[x][y][r] = 0.0f;
  const int sg = lane & 7, ql = lane >> 3;
  const int rrow = 32 * wave + 4 * ql;
  const f32x4 zero4 = {0.0f, 0.0f, 0.0f, 0.0f};
  f32x4 yr[4], bacc = zero4;
  float xo[8];                                                 // observation half (k = 8hf …) of sample m + (lane & 31)
  int src_nx = (c0 + j < c1) ? (a.perm ? a.perm[c0 + j] : c0 + j) : 0;
  // The next slab's loads. NO lane-dependent branch may surround a load here: behind an `if (row < c1) load` the compiler loses count of the loads in
  // flight and falls back to s_waitcnt vmcnt(0) — round 4's fetch had one before its observation loads and one behind its index load, i.e. every slab
  // waited out the HBM round trip of the δ2 loads it had just issued: 2.1 of a slab's 5.0 µs (in-kernel stamps, profiles/r05_c3_wgrad_stamps.txt). So
  // every lane loads from a clamped, valid address and what lies beyond the chunk / beyond obs_dim is zeroed where it is USED (a slab later). Order: the
  // observation rows first — their address is the index the PREVIOUS fetch loaded last, complete long ago —, then δ2, then the next index.
  const int k0x = (8 * hf < a.D && 8 * hf < DP) ? 8 * hf : 0;
  const bool ragged = ((c1 - c0) & 31) != 0;                   // (uniform) the chunk's last slab is partial
  auto fetch_y = [&](int m) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      int mm = m + 4 * sg + e; mm = mm < c1 ? mm : c1 - 1;
      yr[e] = *reinterpret_cast<const f32x4*>(a.dY + (size_t)H * mm + rrow);
    }
  };
  auto fetch_x = [&](int m) {
    if ((a.D & 3) == 0) {
      const f32x4* p = reinterpret_cast<const f32x4*>(a.obs + (size_t)src_nx * (size_t)a.D + k0x);
      const f32x4 q0 = p[0], q1 = p[k0x + 4 < a.D ? 1 : 0];
      xo[0] = q0[0]; xo[1] = q0[1]; xo[2] = q0[2]; xo[3] = q0[3]; xo[4] = q1[0]; xo[5] = q1[1]; xo[6] = q1[2]; xo[7] = q1[3];
    } else {
#pragma unroll
      for (int c = 0; c < 8; ++c) { const int cc = k0x + c < a.D ? k0x + c : a.D - 1; xo[c] = a.obs[(size_t)src_nx * (size_t)a.D + cc]; }
    }
    int mn = m + 32 + j; mn = mn < c1 ? mn : c1 - 1;
    src_nx = a.perm ? a.perm[mn] : mn;
  };
  // The two waves of a SIMD (wave w and w + 4: wk = 0 / 1) request the next slab's δ2 at DIFFERENT points of the slab. Issuing 32 KB of loads takes a CU
  // 0.9 µs (the "loads issued" interval of the timeline: the wave sits in the issue stage until the memory pipeline has taken its requests), and with all
  // eight waves doing that behind barrier 2 the matrix pipe waited for it. Now waves 4-7 ask for their δ2 rows as soon as they have staged the current ones
  // (their stall runs beside their partner's h1 arithmetic, which gets the issue port to itself meanwhile) and go straight to the MFMAs behind barrier 2,
  // while waves 0-3 issue their loads there as before — beside their partner's MFMAs.
  const bool early_y = wk == 1;
  if (c0 < c1) { fetch_x(c0); fetch_y(c0); }
  for (int m = c0; m < c1; m += 32) {
    const bool gst = m == c0 + 32 * 40;          // (diagnostic builds stamp the chunk's 41st slab)
    if (gst) CRL_GSTAMP(0);
    if (m != c0) __syncthreads();
    if (gst) CRL_GSTAMP(1);
    if (ragged) {                                              // rows beyond the chunk were loaded from its last row: they count as zero
#pragma unroll
      for (int e = 0; e < 4; ++e) if (m + 4 * sg + e >= c1) yr[e] = zero4;
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) if (8 * hf + c >= a.D || 8 * hf >= DP) xo[c] = 0.0f;   // beyond obs_dim (a sample beyond the chunk has δ2 = 0: its h1 does not matter)
    stage_d2_slab(yr, G, Yp, H, rrow, sg);
    bacc += (yr[0] + yr[1]) + (yr[2] + yr[3]);
    if (early_y && m + 32 < c1) fetch_y(m + 32);
    if (gst) CRL_GSTAMP(2);
    {
      f32x4 x0, x1;
      x0[0] = xo[0]; x0[1] = xo[1]; x0[2] = xo[2]; x0[3] = xo[3]; x1[0] = xo[4]; x1[1] = xo[5]; x1[2] = xo[6]; x1[3] = xo[7];
      const H1Prod hp = regen_h1_product(x0, x1, w1.w1b, w1.w1un);
      const f32x16 c16 = hp.c16; const float un1 = hp.un1;
      // (this kernel's own statement of regen_h1_store: through the function the compiler's register assignment here changes, profiles/wgrad_refactor_cost.txt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {                             // registers 4g … 4g + 3 = samples 8g + 4hf + {0..3} of the slab
        f32x4 hv;
#pragma unroll
        for (int e = 0; e < 4; ++e) hv[e] = tanh_exp2_arg(__builtin_fmaf(c16[4 * g + e], un1, w1.b1u), X2_ACT_SCALE);
        uint2 hh, ll;
        split2x4(hv, 1.0f, hh, ll);
        *reinterpret_cast<uint2*>(Xp + (0 * H + 32 * wave + j) * X3ROW + 8 * g + 4 * hf) = hh;
        *reinterpret_cast<uint2*>(Xp + (1 * H + 32 * wave + j) * X3ROW + 8 * g + 4 * hf) = ll;
      }
    }
    if (gst) CRL_GSTAMP(3);
    __syncthreads();
    if (gst) CRL_GSTAMP(4);
    if (m + 32 < c1) { fetch_x(m + 32); if (!early_y) fetch_y(m + 32); }
    if (gst) CRL_GSTAMP(5);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      P2 af[2], bf[4];
#pragma unroll
      for (int x = 0; x < 2; ++x) af[x] = load_frag(Yp, H, wn * 2 + x, ks, j, hf);
#pragma unroll
      for (int y = 0; y < 4; ++y) bf[y] = load_frag(Xp, H, wk * 4 + y, ks, j, hf);
#pragma unroll
      for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 4; ++y) acc[x][y] = mfma_x2(af[x], bf[y], acc[x][y]);
      if (gst && ks == 0) CRL_GSTAMP(6);
    }
    if (gst) CRL_GSTAMP(7);
  }
  __syncthreads();
  // (this kernel's own statement of wgrad_store_partial, for the same reason)
  const float un = Ginv * (1.0f / X2_ACT_SCALE);
  float* pw = a.pW + (size_t)blockIdx.x * H * H;
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 4; ++y) {
      const int k = (wk * 4 + y) * 32 + j;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int n = (wn * 2 + x) * 32 + 8 * g + 4 * hf;
        *reinterpret_cast<f32x4*>(pw + (size_t)H * k + n) = acc_quad<true>(acc[x][y], g, un);
      }
    }
  if (a.pB) wgrad_bias_fold(bacc, reinterpret_cast<float*>(smw), tid, sg, a.pB + (size_t)blockIdx.x * H + rrow);
}

template <int DP>
__global__ void __launch_bounds__(512) wide_wgrad_gen_kernel(WgradGenArgs a0, WgradGenArgs a1) {
  if (blockIdx.y == 0) wide_wgrad_gen_body<DP>(a0); else wide_wgrad_gen_body<DP>(a1);
}
constexpr int WG_LDS = 2 * 2 * 256 * X3ROW * 2;   // 81,920 bytes

// ======================================================================================================================================
// The same weight gradient from δ2 as the backward kernel's SPLIT output (FusedBwdArgs::D2h): nothing is converted here, and nothing is loaded into
// registers — every global read of the slab loop is an LDS-DMA, so the loop has no compiler-counted load and its only vmcnt wait is the one written
// below. With the operand staging gone, the loop is a ONE-barrier software pipeline: between two barriers every wave multiplies slab m (48 MFMAs from
// the landed planes and the h1 pieces made during the previous slab) and makes the h1 pieces of slab m + 32 into the other buffer — the matrix work and
// the vector work of a slab no longer alternate in lock-step phases with a barrier and the block's wave skew between them (in-kernel stamps of the
// two-barrier form of this kernel: 1.2 µs of h1 arithmetic with the matrix pipe idle, 1.8 µs of products with the vector pipe idle, 0.9 µs of
// barriers and skew per slab).
// A slab's 32 sample rows of the hi and the lo plane (2 x 16 KB) are requested one slab ahead, between the slab's two jobs (the buffer is free from the
// barrier on; the request costs a wave 0.2 µs of issue); the A operand (rows = units, k = samples) is read from that [sample][unit] image with ds_read_b64_tr_b16 —
// the transposing read — so the image is what the DMA can write: lane-linear rows, 16-byte chunks XORed with the row's low two bits so that the four
// rows of a transposed block sit in four different bank groups (chunk c of row r lies at 512·r + 16·(c ^ ((r & 3) << 2)); the DMA's lanes fetch the
// permuted chunk, the reads undo it). Wave 0 also gathers the observation rows (per-lane addresses) and the inverse scales of the slab after next and
// the permutation indices of the slab after that.
// The planes carry δ2·s1 with a PER-SAMPLE power of two, and the sum runs over samples: the factor 1/s1 goes onto the other operand — the regenerated
// h1 tile is multiplied by t = (1/s1) / max over the chunk of (1/s1), a power of two ≤ 1 (samples with small cotangents lose low bits of h1 exactly as
// they lost low bits of δ2 under the one scale per chunk of wide_wgrad_gen_kernel) — and the chunk's maximum is taken out of the accumulators at the end.
// db2 = Σ δ2 is summed from the A fragments themselves ((hi + lo)·t, exact in f32) by the four waves that hold distinct fragments.
// ======================================================================================================================================
struct WgradSplitArgs {
  const _Float16* Yh; const float* ys;
  const float* obs; const int32_t* perm; int D;
  const float* W1f; const float* w1sc;
  float* pW; float* pB; int M; int chunk;
};
constexpr int WS_YBUF = 2 * 32 * 512;                          // 32,768: one slab, 32 hi rows then 32 lo rows of 512 B
constexpr int WS_XBUF = 2 * 256 * X3ROW * 2;                   // 40,960: [2 pieces][256][X3ROW] f16, the h1 pieces of one slab
constexpr int WS_OFF_X = 2 * WS_YBUF;                          // 65,536
constexpr int WS_OFF_O = WS_OFF_X + 2 * WS_XBUF;               // 147,456: a slab's observation rows as gathered, [2 buffers][2,048 B]
constexpr int WS_OFF_T = WS_OFF_O + 2 * 2048;                  // 151,552: 1/s1 of a slab's samples, [3][64] f32 (32 used)
constexpr int WS_OFF_I = WS_OFF_T + 3 * 256;                   // 152,320: permutation indices of a slab, [2][64] i32 (32 used)
constexpr int WS_LDS = WS_OFF_I + 2 * 256;                     // 152,832
static_assert(WS_LDS <= 160 * 1024, "split weight gradient: LDS budget");
typedef __fp16 h16x4 __attribute__((__vector_size__(4 * sizeof(__fp16))));
typedef __attribute__((address_space(3))) h16x4 lds_h16x4;

template <int DP>
__device__ __forceinline__ void wide_wgrad_split_body(const WgradSplitArgs& a) {
  constexpr int H = 256, NT = 512;
  extern __shared__ __attribute__((aligned(16))) unsigned char smw[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), j = lane & 31, hf = lane >> 5;
  const int wn = wave & 3, wk = wave >> 2;
  const int c0 = blockIdx.x * a.chunk;
  const int c1 = (c0 + a.chunk) < a.M ? (c0 + a.chunk) : a.M;     // (the launcher guarantees whole 32-sample slabs)
  // the chunk's largest 1/s1 (every entry is a power of two: the reciprocal below is exact)
  float imax, iinv;
  {
    float mx = 0.0f;
    for (int m = c0 + tid; m < c1; m += NT) mx = __builtin_fmaxf(mx, a.ys[m]);
    mx = block_max<NT / 64>(mx, reinterpret_cast<float*>(smw), lane, wave);
    imax = mx > 0.0f ? mx : 1.0f;
    iinv = __uint_as_float((254u - ((__float_as_uint(imax) >> 23) & 0xFFu)) << 23);
  }
  RegenW1 w1;
  regen_w1_load(w1, a.W1f, a.w1sc, wave, lane);
  f32x16 acc[2][4];
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 4; ++y)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[x][y][r] = 0.0f;
  float bsum[2] = {0.0f, 0.0f};
  const int k0x = (8 * hf < a.D && 8 * hf < DP) ? 8 * hf : 0;
  const bool obs16 = (a.D & 3) == 0;
  const unsigned ybase = lds_addr_of(smw);
  // wave 0's side requests (clamped addresses: a lane past the chunk fetches the chunk's last sample, nobody uses it)
  auto gather_obs = [&](int idx, int buf) {      // rows of a slab's samples: lane (j, hf) fetches elements 8hf … of sample j
    const unsigned dst = ybase + WS_OFF_O + buf * 2048;
    if (obs16) {
      const float* p = a.obs + (size_t)idx * (size_t)a.D + k0x;
      lds_dma16_v(p, dst);
      lds_dma16_v(p + (k0x + 4 < a.D ? 4 : 0), dst + 1024);
    } else {
#pragma unroll
      for (int c = 0; c < 8; ++c) { const int cc = k0x + c < a.D ? k0x + c : a.D - 1; lds_dma4_v(a.obs + (size_t)idx * (size_t)a.D + cc, dst + 256 * c); }
    }
  };
  auto fetch_scales = [&](int m, int buf) { int mm = m + lane; mm = mm < c1 ? mm : c1 - 1; lds_dma4_v(a.ys + mm, ybase + WS_OFF_T + buf * 256); };
  auto fetch_index = [&](int m, int buf) { int mm = m + lane; mm = mm < c1 ? mm : c1 - 1; lds_dma4_v(a.perm + mm, ybase + WS_OFF_I + buf * 256); };
  // DMA of one slab's planes: piece p (0..31) = rows 2(p & 15), +1 of plane p >> 4; this wave takes pieces wave, wave + 8, +16, +24 (p & 1 = wave & 1 for all four)
  const unsigned dvoff = (unsigned)(hf * 512 + 16 * (j ^ (((2 * (wave & 1) + hf) & 3) << 2)));
  const _Float16* ylo = a.Yh + (size_t)256 * a.M;
  auto dma_slab = [&](int m, int buf) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int p = wave + 8 * i;
      const _Float16* plane = (i < 2) ? a.Yh : ylo;
      lds_dma16(plane + (size_t)256 * (m + 2 * (p & 15)), dvoff, ybase + buf * WS_YBUF + (p >> 4) * 16384 + (p & 15) * 1024);
    }
  };
  // transposed-read addresses (bytes from the buffer's base): 16-lane group gq, q = row of the 4-row block, pp = 4-column piece
  const int gq = lane >> 4, q4 = (lane & 15) >> 2, pp = lane & 3;
  const int abase = 512 * q4 + 8 * (pp & 1) + 16 * (2 * (gq & 1) + (pp >> 1)) + 4096 * (gq >> 1);
  int aoff[2];
#pragma unroll
  for (int x = 0; x < 2; ++x) aoff[x] = abase + 64 * ((wn * 2 + x) ^ q4);
  auto tr8 = [&](const unsigned char* base, int off) -> f16x8 {   // samples r0 … r0 + 7 of the lane's unit: two 4-row blocks
    const h16x4 u = __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_h16x4*)(base + off));
    const h16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_h16x4*)(base + off + 2048));
    f16x8 r;
    r[0] = (_Float16)u[0]; r[1] = (_Float16)u[1]; r[2] = (_Float16)u[2]; r[3] = (_Float16)u[3];
    r[4] = (_Float16)v[0]; r[5] = (_Float16)v[1]; r[6] = (_Float16)v[2]; r[7] = (_Float16)v[3];
    return r;
  };
  // h1 pieces of one slab, in two halves so that the products of the slab in flight can be issued between them:
  //   pre: the gathered observation rows → regen_h1_product;
  //   post: regen_h1_store with the samples' t into the [unit][sample] image
  auto h1_pre = [&](int obuf, float& un1) -> f32x16 {
    float xo[8];
    const float* xs = reinterpret_cast<const float*>(smw + WS_OFF_O + obuf * 2048);
    if (obs16) {
      const f32x4 q0 = *reinterpret_cast<const f32x4*>(xs + 4 * lane), q1 = *reinterpret_cast<const f32x4*>(xs + 256 + 4 * lane);
      xo[0] = q0[0]; xo[1] = q0[1]; xo[2] = q0[2]; xo[3] = q0[3]; xo[4] = q1[0]; xo[5] = q1[1]; xo[6] = q1[2]; xo[7] = q1[3];
    } else {
#pragma unroll
      for (int c = 0; c < 8; ++c) xo[c] = xs[64 * c + lane];
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) if (8 * hf + c >= a.D || 8 * hf >= DP) xo[c] = 0.0f;
    f32x4 x0, x1;
    x0[0] = xo[0]; x0[1] = xo[1]; x0[2] = xo[2]; x0[3] = xo[3]; x1[0] = xo[4]; x1[1] = xo[5]; x1[2] = xo[6]; x1[3] = xo[7];
    const H1Prod hp = regen_h1_product(x0, x1, w1.w1b, w1.w1un);
    un1 = hp.un1;
    return hp.c16;
  };
  auto h1_post = [&](const f32x16& c16, float un1, int tbuf, int xbuf) {
    regen_h1_store<true>(c16, un1, w1.b1u, reinterpret_cast<const float*>(smw + WS_OFF_T) + 64 * tbuf, iinv,
                         reinterpret_cast<_Float16*>(smw + WS_OFF_X + xbuf * WS_XBUF), H, 32 * wave + j, hf);
  };
  // the loop below must not contain a compiler-counted wait: the values loaded above are made "used" here, so their s_waitcnt is emitted before the loop
  // (the compiler does not count the LDS-DMA pieces, so a vmcnt(n) of its own inside the loop would wait for all but n of THEM)
  asm volatile("" :: "v"(w1.w1b.hi), "v"(w1.w1b.lo), "v"(w1.b1u), "v"(w1.w1un));
  if (c0 < c1) {
    dma_slab(c0, 0);
    if (wave == 0) {
      int m0 = c0 + j; m0 = m0 < c1 ? m0 : c1 - 1;
      int m1 = c0 + 32 + j; m1 = m1 < c1 ? m1 : c1 - 1;
      gather_obs(a.perm ? a.perm[m0] : m0, 0);
      gather_obs(a.perm ? a.perm[m1] : m1, 1);
      fetch_scales(c0, 0); fetch_scales(c0 + 32, 1);
      if (a.perm) fetch_index(c0 + 64, 0);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    float un1;
    const f32x16 c16 = h1_pre(0, un1);
    h1_post(c16, un1, 0, 0);
  }
  // The two waves of a SIMD (w and w + 4) take a slab's two jobs in OPPOSITE order: a wave issues in order, so its own matrix and vector work never overlap,
  // but its partner's can — while waves 0-3 make their h1 tiles (vector pipe) waves 4-7 run their 48 MFMAs, then they swap. Two copies of the loop, one per
  // order (as an if / else inside one loop body the compiler spilled 400 bytes per lane); both execute the same barriers.
  auto slab_loop = [&](auto h1_first_tag) {
  constexpr bool H1_FIRST = decltype(h1_first_tag)::value;
  int cur = 0, i3 = 0;                                          // parity of the slab, slab index mod 3
  for (int m = c0; m < c1; m += 32, cur ^= 1, i3 = i3 == 2 ? 0 : i3 + 1) {
    const bool more = m + 32 < c1, more2 = m + 64 < c1;
    const bool gst = m == c0 + 32 * 40;          // (diagnostic builds stamp the chunk's 41st slab)
    if (gst) CRL_GSTAMP(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");            // this slab's planes (requested a slab ago) and the side requests of the last slab have landed
    __syncthreads();                                            // … for every wave; the h1 pieces of this slab are complete; the previous slab's products have read their buffers
    if (gst) CRL_GSTAMP(1);
    if (more) dma_slab(m + 32, cur ^ 1);
    if (more2 && wave == 0) {                                   // observation rows and scales of slab m + 64, indices of slab m + 96
      int idx = m + 64 + j;
      if (a.perm) idx = reinterpret_cast<const int*>(smw + WS_OFF_I)[64 * cur + j];
      gather_obs(idx, cur);
      fetch_scales(m + 64, i3 == 0 ? 2 : i3 - 1);
      if (a.perm && m + 96 < c1) fetch_index(m + 96, cur ^ 1);
    }
    if (gst) CRL_GSTAMP(2);
    const float* tc = reinterpret_cast<const float*>(smw + WS_OFF_T) + 64 * i3;
    const unsigned char* yb = smw + cur * WS_YBUF;
    const _Float16* Xp = reinterpret_cast<const _Float16*>(smw + WS_OFF_X + cur * WS_XBUF);
    auto products = [&]() {
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        P2 af[2], bf[4];
#pragma unroll
        for (int x = 0; x < 2; ++x) {
          af[x].hi = tr8(yb, aoff[x] + 8192 * ks);
          af[x].lo = tr8(yb + 16384, aoff[x] + 8192 * ks);
        }
#pragma unroll
        for (int y = 0; y < 4; ++y) bf[y] = load_frag(Xp, H, wk * 4 + y, ks, j, hf);
#pragma unroll
        for (int x = 0; x < 2; ++x)
#pragma unroll
          for (int y = 0; y < 4; ++y) acc[x][y] = mfma_x2(af[x], bf[y], acc[x][y]);
        if (wk == 0) {                                          // db2: the fragment's 8 samples of unit 32(2wn + x) + j, scaled back per sample
          const f32x4 t0 = *reinterpret_cast<const f32x4*>(tc + 16 * ks + 8 * hf) * iinv, t1 = *reinterpret_cast<const f32x4*>(tc + 16 * ks + 8 * hf + 4) * iinv;
#pragma unroll
          for (int x = 0; x < 2; ++x) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              bsum[x] = __builtin_fmaf((float)af[x].hi[e], t0[e], bsum[x]); bsum[x] = __builtin_fmaf((float)af[x].lo[e], t0[e], bsum[x]);
              bsum[x] = __builtin_fmaf((float)af[x].hi[4 + e], t1[e], bsum[x]); bsum[x] = __builtin_fmaf((float)af[x].lo[4 + e], t1[e], bsum[x]);
            }
          }
        }
      }
    };
    auto make_h1 = [&]() {
      if (more) {
        float un1;
        const f32x16 c16 = h1_pre(cur ^ 1, un1);
        h1_post(c16, un1, i3 == 2 ? 0 : i3 + 1, cur ^ 1);
      }
    };
    if constexpr (H1_FIRST) { make_h1(); if (gst) CRL_GSTAMP(3); products(); }
    else { products(); if (gst) CRL_GSTAMP(3); make_h1(); }
    if (gst) CRL_GSTAMP(7);
  }
  };
  if (wk == 0) slab_loop(std::true_type{}); else slab_loop(std::false_type{});
  __syncthreads();
  wgrad_store_partial<2, 4, true>(acc, imax * (1.0f / X2_ACT_SCALE), a.pW + (size_t)blockIdx.x * H * H, H, wn * 64, wk * 128, j, hf);
  if (a.pB && wk == 0) {
#pragma unroll
    for (int x = 0; x < 2; ++x) {
      const float v = bsum[x] + xor32(bsum[x]);
      if (hf == 0) a.pB[(size_t)blockIdx.x * H + (wn * 2 + x) * 32 + j] = v * imax;
    }
  }
}

template <int DP>
__global__ void __launch_bounds__(512) wide_wgrad_split_kernel(WgradSplitArgs a0, WgradSplitArgs a1) {
  if (blockIdx.y == 0) wide_wgrad_split_body<DP>(a0); else wide_wgrad_split_body<DP>(a1);
}

}  // namespace crl
