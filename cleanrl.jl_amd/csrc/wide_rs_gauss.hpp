// wide_rs_gauss.hpp — the one-launch rollout of a Gaussian handle at 2x256 (included by wide.hip behind wide_rs.hpp; route RS_ACTOR).
//
// wide_rs_rollout_gauss_kernel is wide_rs_rollout_kernel with another tail. The block owns 64 envs for all num_steps steps, the actor's fp16x2 W2
// pieces stay in the eight waves' registers, and phases P, M, E with barriers B1-B3 are that kernel's (rg_roll_load / rg_roll_pme / rg_roll_store
// below restate them: stating them once for both kernels changed wide_rs_rollout_kernel's register allocation, and the softmax kernel's code is
// not to move for this one). What differs is S. The softmax tail is one lane per env doing a <= 8-way softmax and one Philox draw; the Gaussian tail per env is,
// for EVERY action component, a Float64 Box–Muller (log, sqrt, cos), a tanhf, an expf and the logπ term — as gauss_step_act walks them, act_dim
// dependent chains on one lane, behind B3, with seven waves idle. Two facts take that apart:
//   * ξ_i depends on (seed, env id, gstep, i) and on nothing the forward pass computes. Wave 4 + i (lane = env) draws ξ_i of step s + 1 while wave 0
//     runs the env step of step s, into an LDS table [parity][component][env]; step 0's is drawn in the prologue, beside the weight loads. The
//     Float64 chain is then never between B3 and B4 of the step that needs it. Waves 4 … 7, not 1 … 4: the waves that own components (below) stay
//     free of it, and the draw is cut in two — the integer Philox block before barrier B3b, the Float64 chain behind it — so neither half
//     stands between the component waves and wave 0.
//   * the components are independent until logπ is summed. Behind B3 wave i < act_dim (lane = env) folds the eight row-group partials and b3 of rows
//     i (μ_i) and act_dim + i (s_i) — waves 0 … 7, then the bias: wide_rs_rollout_kernel's order —, forms log_std, σ, a_i and the logπ term, stores
//     a_i to the float action plane and leaves (a_i, term_i) in an LDS exchange area [slot 8][env]. One more barrier (B3b), then wave 0 adds the terms
//     in index order from 0.0f (the order gauss_step_act pins), steps the env and keeps the books (rg_step_env).
// PAR = false is the other split: no B3b, wave 0 walks the components itself (through the same exchange area) — one barrier less per step, act_dim
// serial chains more. Which one a given act_dim takes is CRL_RG_PAR_FROM, set from the measurement in DESIGN.md.
// Every expression is ppo_gauss.hpp's, so given the same head outputs the action, logπ and ξ of an (env, step) are the per-step route's bit for bit;
// the forward flavour (fp16x2 pieces, tanh_fast) is what differs between the routes, as it does for the softmax head.
#pragma once

namespace crl {

constexpr int RG_ADMAX = 4;                                    // act_dim on this route: the head's 2·act_dim rows fit the [8] partials
constexpr int RG_XI_WAVE0 = 4;                                 // wave RG_XI_WAVE0 + i draws ξ_i
constexpr int RG_OFF_XI = RR_LDS;                              // ξ [parity 2][component 4][env 64] f32
constexpr int RG_OFF_EX = RG_OFF_XI + 2 * RG_ADMAX * RR_MB * 4;   // exchange [slot 8][env 64] f32: a_0 … a_3, logπ terms 0 … 3
constexpr int RG_LDS = RG_OFF_EX + 2 * RG_ADMAX * RR_MB * 4;   // 120,864 bytes
static_assert(RG_LDS <= 160 * 1024 && RG_OFF_XI % 16 == 0, "the Gaussian rollout block's LDS");
#ifndef CRL_RG_PAR_FROM
#define CRL_RG_PAR_FROM 1                                      // smallest act_dim whose components run on waves of their own (5 = never)
#endif

// rs_step_env (wide_rs.hpp) for the Gaussian head — the env's running state in LDS, a step loads nothing from global memory. ex: the exchange area at
// this env (lane = env): a_i at ex[i·64], the logπ terms behind them. The terms are added in index order from 0.0f, as gauss_step_act adds them.
__device__ __forceinline__ void rg_step_env(const WStepArgs& a, int ad, const float* ex, int e, int step, float* obs_l, float* st_l,
                                            double& st_n, double& st_ret, double& st_len, double& st_max) {
  const DevCfg& c = a.c;
  const int D = c.D;
  const uint32_t gid = c.env_id_offset + (uint32_t)e;
  const uint64_t gstep = a.iteration * (uint64_t)c.k + (uint64_t)step;
  const size_t b = (size_t)e + (size_t)c.nt * step;
  const f32x4 s0 = *reinterpret_cast<const f32x4*>(st_l), s1 = *reinterpret_cast<const f32x4*>(st_l + 4);
  f32x4 x[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) x[q] = *reinterpret_cast<const f32x4*>(obs_l + 4 * q);
  const int nd = __float_as_int(s0[0]);
  int ep_len = __float_as_int(s0[2]) + 1;                            // ppo.jl:125
  float actf[RG_ADMAX], lpa = 0.0f;
#pragma unroll
  for (int i = 0; i < RG_ADMAX; ++i) {
    actf[i] = 0.0f;
    if (i < ad) { actf[i] = ex[i * RR_MB]; lpa += ex[(RG_ADMAX + i) * RR_MB]; }
  }
  float* ob = a.obs + b * (size_t)D;
  if ((D & 3) == 0) {                                                // ppo.jl:133-140 Buffer.add!
#pragma unroll
    for (int q = 0; q < 4; ++q) if (4 * q < D) *reinterpret_cast<f32x4*>(ob + 4 * q) = x[q];
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int i = 0; i < 4; ++i) if (4 * q + i < D) ob[4 * q + i] = x[q][i];
  }
  a.logprob[b] = lpa; a.terminal[b] = (uint8_t)nd;
  bool done; float rew;
  f32x4 es = s1; int t_env = __float_as_int(s0[3]);
  if (env_continuous(c.env_kind)) {
    float s[4] = {s1[0], s1[1], s1[2], s1[3]}, so[ENV_OBS_MAX];
    env_transition_c(c.env_kind, c.stale_obs, s, t_env, actf, c.seed, gid, gstep, so, rew, done);
#pragma unroll
    for (int i = 0; i < 4; ++i) { x[0][i] = so[i]; x[1][i] = so[4 + i]; es[i] = s[i]; }
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (4 * q < D) {
        float o4[4];
        synth_obs4(c.seed, gid, gstep, q, o4);
#pragma unroll
        for (int i = 0; i < 4; ++i) x[q][i] = 4 * q + i < D ? o4[i] : 0.0f;
      }
    synth_reward_done(c.seed, gid, gstep, rew, done);
  }
  a.reward[b] = rew;
  float ep_ret = s0[1] + rew;                                        // ppo.jl:145
  if (done) {                                                        // ppo.jl:147-165
    st_n += 1.0; st_ret += (double)ep_ret; st_len += (double)ep_len;
    st_max = step_stat_max_s(head_signed_returns<HeadGauss>(c.env_kind), st_n, st_max, (double)ep_ret);
    episode_ring_push(a.ring, a.ring_count, a.ring_cap, ep_ret, ep_len, gid, step);
    ep_ret = 0.0f; ep_len = 0;
  }
  f32x4 n0; n0[0] = __int_as_float(done ? 1 : 0); n0[1] = ep_ret; n0[2] = __int_as_float(ep_len); n0[3] = __int_as_float(t_env);   // ppo.jl:144
  *reinterpret_cast<f32x4*>(st_l) = n0; *reinterpret_cast<f32x4*>(st_l + 4) = es;
#pragma unroll
  for (int q = 0; q < 4; ++q) *reinterpret_cast<f32x4*>(obs_l + 4 * q) = x[q];
}

// The block's pieces that do not know what the head rows mean, as wide_rs_rollout_kernel has them inline.
// rg_roll_load: the actor's tables, the block's 64 observations and its envs' running state, global -> LDS (the caller's barrier follows)
template <int NA>
__device__ __forceinline__ void rg_roll_load(const RsRollArgs& r, unsigned char* smx, int tid, int m0) {
  const RollPCNet& nn = r.n;
  float* b1tab = reinterpret_cast<float*>(smx + RR_OFF_B1);
  float* w3tab = reinterpret_cast<float*>(smx + RR_OFF_W3);
  float* b2tab = reinterpret_cast<float*>(smx + RR_OFF_B2);
  float* obsl = reinterpret_cast<float*>(smx + RR_OFF_OBS);
  float* stl = reinterpret_cast<float*>(smx + RR_OFF_ST);
  float* b3l = reinterpret_cast<float*>(smx + RR_OFF_B3);
  const int D = r.D, Dst = r.s.c.D;
  if (tid < 256) { b1tab[tid] = nn.W1f[4096 + tid]; b2tab[tid] = nn.b2[tid]; }
  for (int i = tid; i < NA * 256; i += 512) w3tab[i] = i < nn.A * 256 ? nn.W3t[i] : 0.0f;
  for (int i = tid; i < 1024; i += 512) reinterpret_cast<f32x4*>(smx + RR_OFF_W1)[i] = reinterpret_cast<const f32x4*>(nn.W1f)[i];
  for (int i = tid; i < RR_MB * 16; i += 512) { const int e = i >> 4, c = i & 15; obsl[i] = c < D ? r.s.cur_obs[(size_t)(m0 + e) * D + c] : 0.0f; }
  if (tid < 8) b3l[tid] = tid < nn.A ? nn.b3[tid] : 0.0f;
  if (tid < RR_MB) {                                                    // the envs' running state: global -> LDS for the launch
    const int e = m0 + tid;
    float* q = stl + tid * 8;
    q[0] = __int_as_float((int)r.s.next_done[e]); q[1] = r.s.ep_return[e]; q[2] = __int_as_float(r.s.ep_length[e]); q[3] = __int_as_float(r.s.env_t[e]);
    for (int i = 0; i < 4; ++i) q[4 + i] = i < Dst ? r.s.env_state[(size_t)Dst * e + i] : 0.0f;
  }
}

// rg_roll_pme: phases P, M and E of one step, through barrier B3 — behind it all head partials [wave][env][8] of the step are in LDS
template <int DP, int NA>
__device__ __forceinline__ void rg_roll_pme(unsigned char* smx, const RsWeights& W, int D, float w1un, float cs, int wave, int j, int hf) {
  float* b1tab = reinterpret_cast<float*>(smx + RR_OFF_B1);
  float* w3tab = reinterpret_cast<float*>(smx + RR_OFF_W3);
  float* b2tab = reinterpret_cast<float*>(smx + RR_OFF_B2);
  float* hpall = reinterpret_cast<float*>(smx + RR_OFF_HP);
  float* obsl = reinterpret_cast<float*>(smx + RR_OFF_OBS);
  _Float16* Xl = reinterpret_cast<_Float16*>(smx);
  // layer 1 of one 32-env half: observation fragment from LDS, product, activation, split, h1 tile
  auto p_begin = [&](int ct, P2& xb, float& xinv) {
    float xr[8];
    const float* xo = obsl + (32 * ct + j) * 16 + 8 * hf;
    const f32x4 q0 = *reinterpret_cast<const f32x4*>(xo), q1 = *reinterpret_cast<const f32x4*>(xo + 4);
    xr[0] = q0[0]; xr[1] = q0[1]; xr[2] = q0[2]; xr[3] = q0[3]; xr[4] = q1[0]; xr[5] = q1[1]; xr[6] = q1[2]; xr[7] = q1[3];
    rs_xfrag<DP>(xr, D, hf, xb, xinv, w1un);
  };
  {
    const f16x8* w1l = reinterpret_cast<const f16x8*>(smx + RR_OFF_W1) + (wave * 2) * 64 + 32 * hf + j;
    // P(0): this wave's 32 units of h1 for envs 0-31
    P2 xb; float xinv;
    p_begin(0, xb, xinv);
    f32x16 c1 = rs_layer1(w1l, xb);
    rs_produce<true, RR_MB>(c1, xinv, b1tab, Xl, wave, j, hf);
    p_begin(1, xb, xinv);
    c1 = rs_layer1(w1l, xb);                                            // the second half's layer-1 product: ahead of the 48 MFMAs it would queue behind
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                                       // B1: h1 of envs 0-31 is complete
    f32x16 a0, c0;
    // M(0) beside P(1): the matrix pipe multiplies the first half while the vector pipe makes the second half's h1. Four groups of four k-steps, each
    // followed by the activation of four elements; the scheduler may reorder inside a group, not across (one bias quad in flight ahead)
    {
#pragma unroll
      for (int q = 0; q < 16; ++q) { a0[q] = 0.0f; c0[q] = 0.0f; }
      const _Float16* x0 = Xl + j * RS_ROW + 8 * hf;
      const float* b1l = b1tab + 32 * wave + 4 * hf;
      f32x4 bv = *reinterpret_cast<const f32x4*>(b1l);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4 bn = *reinterpret_cast<const f32x4*>(b1l + 8 * (g < 3 ? g + 1 : 3));
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
          const int ks = 4 * g + kk;
          const f16x8 bh = *reinterpret_cast<const f16x8*>(x0 + 16 * ks), bl = *reinterpret_cast<const f16x8*>(x0 + RR_MB * RS_ROW + 16 * ks);
          a0 = mfma_f16(W.wl[ks], bh, a0);
          c0 = mfma_f16(W.wh[ks], bh, c0);
          a0 = mfma_f16(W.wh[ks], bl, a0);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) c1[4 * g + e] = tanh_fast(__builtin_fmaf(c1[4 * g + e], xinv, bv[e]) * INV_TWO_LOG2E) * X2_ACT_SCALE;   // P(1), in place
        uint2 hh, ll;
        f32x4 hv; hv[0] = c1[4 * g]; hv[1] = c1[4 * g + 1]; hv[2] = c1[4 * g + 2]; hv[3] = c1[4 * g + 3];
        split2x4(hv, 1.0f, hh, ll);
        _Float16* xo = Xl + (32 + j) * RS_ROW + 32 * wave + 4 * hf + 8 * g;
        *reinterpret_cast<uint2*>(xo) = hh;
        *reinterpret_cast<uint2*>(xo + RR_MB * RS_ROW) = ll;
        bv = bn;
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int q = 0; q < 16; ++q) a0[q] += c0[q];
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                                       // B2: h1 of envs 32-63 is complete
    // M(1) beside E(0)
    f32x16 a1, c1b;
    {
#pragma unroll
      for (int q = 0; q < 16; ++q) { a1[q] = 0.0f; c1b[q] = 0.0f; }
      const _Float16* x1 = Xl + (32 + j) * RS_ROW + 8 * hf;
      const float* b2l = b2tab + 32 * wave + 4 * hf;
      f32x4 bv = *reinterpret_cast<const f32x4*>(b2l);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4 bn = *reinterpret_cast<const f32x4*>(b2l + 8 * (g < 3 ? g + 1 : 3));
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
          const int ks = 4 * g + kk;
          const f16x8 bh = *reinterpret_cast<const f16x8*>(x1 + 16 * ks), bl = *reinterpret_cast<const f16x8*>(x1 + RR_MB * RS_ROW + 16 * ks);
          a1 = mfma_f16(W.wl[ks], bh, a1);
          c1b = mfma_f16(W.wh[ks], bh, c1b);
          a1 = mfma_f16(W.wh[ks], bl, a1);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) a0[4 * g + e] = tanh_fast(__builtin_fmaf(a0[4 * g + e], cs, bv[e]));                                  // E(0), in place
        bv = bn;
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    float* hp = hpall + wave * (RR_MB * 8);
    rs_heads<NA>(a0, w3tab, hp, wave, j, hf);
#pragma unroll
    for (int q = 0; q < 16; ++q) a1[q] += c1b[q];
    rs_epilogue<true, NA>(a1, cs, b2tab, w3tab, hp + 32 * 8, nullptr, wave, j, hf);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                                       // B3: all head partials are in LDS
  }
}

// rg_roll_store: the envs' state back to global memory for the next launch (one-launch or per-step). stateful: the env keeps (at most four) state
// words of its own; else — the synthetic env — its state is its observation
__device__ __forceinline__ void rg_roll_store(const RsRollArgs& r, const unsigned char* smx, int tid, int m0, bool stateful) {
  const float* obsl = reinterpret_cast<const float*>(smx + RR_OFF_OBS);
  const float* stl = reinterpret_cast<const float*>(smx + RR_OFF_ST);
  const int Dst = r.s.c.D;
  if (tid < RR_MB) {
    const int e = m0 + tid;
    const float* q = stl + tid * 8;
    r.s.next_done[e] = (uint8_t)__float_as_int(q[0]); r.s.ep_return[e] = q[1]; r.s.ep_length[e] = __float_as_int(q[2]); r.s.env_t[e] = __float_as_int(q[3]);
    for (int i = 0; i < Dst; ++i) {
      const float o = obsl[tid * 16 + (i < 16 ? i : 0)];
      r.s.cur_obs[(size_t)Dst * e + i] = o;
      r.s.env_state[(size_t)Dst * e + i] = stateful ? (i < 4 ? q[4 + i] : 0.0f) : o;
    }
  }
}

template <int DP, int NA, bool PAR>
__global__ void __launch_bounds__(512) wide_rs_rollout_gauss_kernel(RsRollArgs r, HeadGauss hd) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smx[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int j = lane & 31, hf = lane >> 5;
  const int m0 = blockIdx.x * RR_MB;
  const RollPCNet& nn = r.n;
  const DevCfg& c = r.s.c;
  const float* hpall = reinterpret_cast<const float*>(smx + RR_OFF_HP);
  float* obsl = reinterpret_cast<float*>(smx + RR_OFF_OBS);
  float* stl = reinterpret_cast<float*>(smx + RR_OFF_ST);
  const float* b3l = reinterpret_cast<const float*>(smx + RR_OFF_B3);
  float* xitab = reinterpret_cast<float*>(smx + RG_OFF_XI);
  float* ex = reinterpret_cast<float*>(smx + RG_OFF_EX);
  const int ad = hd.g.ad, nsteps = c.k;
  const uint32_t gid = c.env_id_offset + (uint32_t)(m0 + lane);
  const uint64_t g0 = r.s.iteration * (uint64_t)c.k;
  const int xc = wave - RG_XI_WAVE0;                                    // the component this wave draws noise for
  const bool xi_wave = xc >= 0 && xc < ad;
  rg_roll_load<NA>(r, smx, tid, m0);
  if (xi_wave) xitab[xc * RR_MB + lane] = gauss_xi(c.seed, gid, g0, xc);   // step 0's ξ (parity 0)
  RsWeights W;
  rs_load_weights(nn.Wx2, wave, lane, W);
  const float w1un = nn.w1sc[1];
  const float cs = nn.wsc[1] * (1.0f / X2_ACT_SCALE);
  double st_n = 0.0, st_ret = 0.0, st_len = 0.0, st_max = 0.0;
  __syncthreads();
#pragma unroll 1
  for (int step = 0; step < nsteps; ++step) {
    asm volatile("" : "+v"(j), "+v"(hf));                               // per-lane addresses are formed per step, not kept across the loop
    rg_roll_pme<DP, NA>(smx, W, r.D, w1un, cs, wave, j, hf);            // P, M, E, barriers B1-B3
    const int par = step & 1;
    // component i of this lane's env: μ_i and s_i from the eight row groups' partials in fixed order, then the bias; a_i out, (a_i, logπ term) to LDS
    auto component = [&](int i) {
      float mu = 0.0f, s = 0.0f;
#pragma unroll
      for (int w8 = 0; w8 < 8; ++w8) { const float* hq = hpall + w8 * (RR_MB * 8) + lane * 8; mu += hq[i]; s += hq[ad + i]; }
      mu += b3l[i]; s += b3l[ad + i];
      float th;
      const float ls = gauss_log_std(hd.g, s, th), xi = xitab[(par * RG_ADMAX + i) * RR_MB + lane];
      const float a = gauss_action(mu, expf(ls), xi);
      hd.action_f[((size_t)(m0 + lane) + (size_t)c.nt * step) * (size_t)ad + i] = a;
      ex[i * RR_MB + lane] = a; ex[(RG_ADMAX + i) * RR_MB + lane] = gauss_lp_term(xi, ls);
    };
    const bool draw = xi_wave && step + 1 < nsteps;                     // ξ of step + 1 into the other parity: its last readers left before B4 of step - 1
    u32x4 blk{};
    if constexpr (PAR) {
      if (wave < ad) component(wave);
      if (draw) blk = gauss_xi_block(c.seed, gid, g0 + (uint64_t)(step + 1), xc);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();                                     // B3b: every component's action and logπ term are in LDS
    }
    if (wave == 0) {
      if constexpr (!PAR) {                                             // (one wave's LDS accesses stay in order: no barrier before it reads them back)
#pragma unroll
        for (int i = 0; i < RG_ADMAX; ++i) if (i < ad) component(i);
      }
      rg_step_env(r.s, ad, ex + lane, m0 + lane, step, obsl + lane * 16, stl + lane * 8, st_n, st_ret, st_len, st_max);
    } else if (draw) {
      if constexpr (!PAR) blk = gauss_xi_block(c.seed, gid, g0 + (uint64_t)(step + 1), xc);
      xitab[((par ^ 1) * RG_ADMAX + xc) * RR_MB + lane] = gauss_xi_of(blk);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                                       // B4: the next observations and the next step's ξ are in LDS
  }
  if (wave == 0) episode_stats_flush(r.s.ep_stats, st_n, st_ret, st_len, st_max, head_signed_returns<HeadGauss>(c.env_kind));
  rg_roll_store(r, smx, tid, m0, env_continuous(c.env_kind));
}

}  // namespace crl
