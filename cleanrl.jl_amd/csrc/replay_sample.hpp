// replay_sample.hpp — Buffer.sample(rb, k) (replay_buffer.jl:40-45: StatsBase.sample(1:size, k, replace=false)) stated once for dqn.hip and
// ddpg.hip (oracle: dqn_sample_indices). Candidates are Philox draws in counter order (counter = candidate number, stream 0xD9, keyed by the
// seed and the global step), mapped to [0, n) by the high half of o.x·n; a candidate already taken is skipped. The whole block draws a round
// of blockDim.x candidates in parallel; thread 0 resolves them in counter order against a bitmap of CAP bits in LDS (CAP / 8 bytes).
#pragma once
#include "common.hpp"

namespace crl {

constexpr uint32_t REPLAY_SAMPLE_STREAM = 0xD9u;

// one block of at most 1024 threads, every thread calls it; needs k <= n <= CAP; idx[0..k) receives the slots in draw order
template <int CAP>
__device__ __forceinline__ void replay_sample(uint64_t seed, uint64_t gstep, int n, int k, int32_t* __restrict__ idx) {
  __shared__ uint32_t bitmap[CAP / 32];
  __shared__ int cand[1024];
  __shared__ int got, cbase;
  const int tid = threadIdx.x, nth = blockDim.x;
  for (int w = tid; w < (n + 31) / 32; w += nth) bitmap[w] = 0u;
  if (tid == 0) { got = 0; cbase = 0; }
  __syncthreads();
  while (got < k) {
    {
      const uint32_t cc = (uint32_t)(cbase + tid);
      const u32x4 o = philox(cc, (uint32_t)gstep, (uint32_t)(gstep >> 32), REPLAY_SAMPLE_STREAM, (uint32_t)seed, (uint32_t)(seed >> 32));
      cand[tid] = (int)(((uint64_t)o.x * (uint64_t)n) >> 32);
    }
    __syncthreads();
    if (tid == 0) {
      int g = got;
      for (int i = 0; i < nth && g < k; ++i) {
        const int j = cand[i];
        if (!((bitmap[j >> 5] >> (j & 31)) & 1u)) { bitmap[j >> 5] |= 1u << (j & 31); idx[g++] = j; }
      }
      got = g; cbase += nth;
    }
    __syncthreads();
  }
}

}  // namespace crl
