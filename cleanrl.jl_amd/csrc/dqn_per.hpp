// dqn_per.hpp — proportional prioritized replay (Schaul et al. 2016) for dqn.hip: a sum tree in heap order, stratified draws with replacement,
// importance weights normalised by the batch maximum, the priority write-back. The expressions are pinned in include/cleanrl_hip.h (crl_dqn_per_*
// block); tests/dqn_per_ref.py restates them in numpy. Everything here is Float64 with contraction off; leaves are Float32 values stored widened.
//
// tree[1 .. 2C) with C = the smallest power of two >= buffer_size; leaf of ring slot s = tree[C + s]; every inner node is tree[2i] + tree[2i+1], one
// add, left operand first — the tree is a pure function of its leaves, so any repair order gives the same bits.
//
// per_repair, per_draw, per_weights, per_block_max and per_batch_tail are called by EVERY thread of ONE block (at most 1024 threads): the sampling
// launches, dqn_td_kernel<·, true> and the categorical handles' Adam launch in dqn.hip and the probe kernel run the same functions.
#pragma once
#include "common.hpp"

namespace crl {

constexpr uint32_t PER_SAMPLE_STREAM = 0xDAu;
constexpr double PER_LEAF_MIN = 0x1.0p-100, PER_LEAF_MAX = 0x1.0p100;

// How many levels of the tree per_draw stages in LDS (level 0 = the root; L levels = nodes 1 .. 2^L − 1, 2^L doubles with the unused node 0). The
// bottom levels are walked in global memory (L2). 0 = no staging. Measured 0, 8, 10, 12 on the GPU: DESIGN.md §3g; 12 levels = 32 KB, half the
// 64 KB static limit.
#ifndef CRL_DQN_PER_LDS_LEVELS
#define CRL_DQN_PER_LDS_LEVELS 12
#endif
constexpr int PER_LDS_LEVELS = CRL_DQN_PER_LDS_LEVELS;
static_assert(PER_LDS_LEVELS >= 0 && PER_LDS_LEVELS <= 12, "up to 12 levels (32 KB) of the tree in LDS");

struct PerCtl {
  double beta;            // beta(g) of the last update
  int64_t synced_step;    // the global step up to which the ring's new slots have their leaves
  float max_leaf;         // the largest leaf any update has written; 1.0f before the first
  int32_t pad;
};

struct PerDev {
  double* tree;           // [2·C]
  PerCtl* ctl;
  double *w, *abs_td;     // [k] importance weights and |δ| of the last update
  int32_t C, on;
  double alpha, beta_start, beta_end, beta_duration, eps;
};

__host__ __device__ __forceinline__ int per_tree_leaves(int64_t n) {
  int c = 1;
  while (c < n) c <<= 1;
  return c;
}

// beta(g) = slope·g + beta_start, clipped at beta_end from whichever side the slope approaches
__device__ __forceinline__ double per_beta(double beta_start, double beta_end, double duration, double g) {
#pragma clang fp contract(off)
  const double slope = (beta_end - beta_start) / duration;
  const double v = slope * g + beta_start;
  if (slope < 0.0) return v < beta_end ? beta_end : v;
  return v > beta_end ? beta_end : v;
}

// leaf = (float)clamp(pow(|δ| + eps, alpha), 2^-100, 2^100): Float32, so that the last bits of the Float64 pow do not reach the sampler
__device__ __forceinline__ float per_leaf(double abs_td, double eps, double alpha) {
#pragma clang fp contract(off)
  double p = pow(abs_td + eps, alpha);
  p = p >= PER_LEAF_MIN ? (p > PER_LEAF_MAX ? PER_LEAF_MAX : p) : PER_LEAF_MIN;   // a NaN (a diverged net) becomes 2^-100: the tree stays finite
  return (float)p;
}

// The ancestors of m touched leaves (slot_of(i), 0 <= i < m, duplicates allowed), level by level with a block barrier per level; every touched parent
// is recomputed from its two children, duplicates write the same value. A level with no more parents than touched leaves is recomputed whole. The
// caller's leaf writes need no barrier of their own: the first level starts with one.
template <typename SlotOf>
__device__ __forceinline__ void per_repair(double* tree, int C, int m, SlotOf slot_of) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x, nth = blockDim.x;
  for (int P = C >> 1, sh = 1; P >= 1; P >>= 1, ++sh) {    // P parents at this level: nodes P .. 2P − 1
    __syncthreads();
    if (m >= P) {
      for (int p = P + tid; p < 2 * P; p += nth) tree[p] = tree[2 * p] + tree[2 * p + 1];
    } else {
      for (int i = tid; i < m; i += nth) {
        const int p = (C + slot_of(i)) >> sh;
        tree[p] = tree[2 * p] + tree[2 * p + 1];
      }
    }
  }
  __syncthreads();
}

// k stratified draws with replacement at update step g: seg = tree[1] / k, target_j = ((double)j + u_j)·seg with u_j = u53(philox(counter j, g, stream
// 0xDA, seed)); descend from the root: left if target < tree[2i] or tree[2i+1] == 0.0, else target −= tree[2i] and right. The zero test keeps every
// visited node positive (the root is; going left means target < l, so l > 0, or r == 0, so l = the node; going right means r != 0), so neither a slot
// >= n nor an empty leaf is ever returned, whatever rounding does to target. The top PER_LDS_LEVELS levels are read from LDS, the rest from global.
__device__ __forceinline__ void per_draw(const double* tree, int C, int k, uint64_t seed, uint64_t g, int32_t* idx) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x, nth = blockDim.x;
  __shared__ double top[PER_LDS_LEVELS > 0 ? (1 << PER_LDS_LEVELS) : 1];
  const int S = PER_LDS_LEVELS == 0 ? 0 : (2 * C < (1 << PER_LDS_LEVELS) ? 2 * C : (1 << PER_LDS_LEVELS));   // nodes below S come from LDS
  for (int i = tid; i < S; i += nth) top[i] = tree[i];
  __syncthreads();
  const double seg = tree[1] / (double)k;
  for (int j = tid; j < k; j += nth) {
    const double u = u53(philox((uint32_t)j, (uint32_t)g, (uint32_t)(g >> 32), PER_SAMPLE_STREAM, (uint32_t)seed, (uint32_t)(seed >> 32)));
    double target = ((double)j + u) * seg;
    int i = 1;
    while (i < C) {
      const int c = 2 * i;                                  // the two children are one aligned 16-byte pair
      const double l = c < S ? top[c] : tree[c], r = c < S ? top[c + 1] : tree[c + 1];
      if (target < l || r == 0.0) i = c;
      else { target -= l; i = c + 1; }
    }
    idx[j] = i - C;
  }
  __syncthreads();
}

// w_j = pow(n·leaf[idx_j] / tree[1], −beta), then w_j /= max_j w_j (the batch maximum: there is no min tree). The maximum is exact in any order.
__device__ __forceinline__ void per_weights(const double* tree, int C, int n, int k, double beta, const int32_t* idx,
                                            double* w) {
#pragma clang fp contract(off)
  __shared__ double wmax[16];
  __shared__ double top_w;
  const int tid = threadIdx.x, nth = blockDim.x;
  const double total = tree[1];
  double mine = 0.0;
  for (int j = tid; j < k; j += nth) {
    const double v = pow((double)n * tree[C + idx[j]] / total, -beta);
    w[j] = v;
    mine = v > mine ? v : mine;
  }
  mine = wave_max(mine);
  if ((tid & 63) == 0) wmax[tid >> 6] = mine;
  __syncthreads();
  if (tid == 0) {
    double t = 0.0;
    for (int i = 0; i < (nth + 63) / 64; ++i) t = wmax[i] > t ? wmax[i] : t;
    top_w = t;
  }
  __syncthreads();
  const double t = top_w;
  for (int j = tid; j < k; j += nth) w[j] = w[j] / t;
  __syncthreads();
}

// The priority write-back of an update, in three steps. Per sample (ONE thread, slot s = idx_b, ad = |δ_b| or the categorical loss_b): abs_td_b, the
// new leaf of s (duplicates write identical values: the same slot has the same δ), and the thread's running maximum `mine` of the leaves it wrote.
__device__ __forceinline__ void per_td_writeback(const PerDev& p, int b, int s, double ad, float& mine) {
#pragma clang fp contract(off)
  const float leaf = per_leaf(ad, p.eps, p.alpha);
  p.abs_td[b] = ad;
  p.tree[p.C + s] = (double)leaf;
  mine = leaf > mine ? leaf : mine;
}
// Every thread's `mine` → one maximum per wave in lmax[tid / 64] (the caller's __shared__ float[16]: a block has at most 16 waves). The caller's
// block barrier follows; a maximum is exact in any order.
__device__ __forceinline__ void per_block_max(float mine, float* lmax) {
#pragma clang fp contract(off)
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) { const float u = __shfl_xor(mine, o, 64); mine = u > mine ? u : mine; }
  if ((threadIdx.x & 63) == 0) lmax[threadIdx.x >> 6] = mine;
}
// Behind that barrier: max_leaf raised to the batch's largest new leaf, then the ancestors of the k written leaves repaired
__device__ __forceinline__ void per_batch_tail(const PerDev& p, const int32_t* idx, int k, const float* lmax) {
#pragma clang fp contract(off)
  if (threadIdx.x == 0) {
    float top = p.ctl->max_leaf;
    for (int i = 0; i < (int)(blockDim.x + 63) / 64; ++i) top = lmax[i] > top ? lmax[i] : top;
    p.ctl->max_leaf = top;
  }
  per_repair(p.tree, p.C, k, [=](int i) { return (int)idx[i]; });
}

}  // namespace crl
