// policy_rt.hpp — get_action's per-sample pieces for a runtime n_act ≤ AMAX (ppo.jl:21-32): shared by the layer-wise path's act / logprob /
// loss / step kernels (wide.hip) and the evaluation kernel (eval.hip). Same operation order as softmax_logsoftmax<A> and sample_weights<A>
// in common.hpp.
#pragma once
#include "common.hpp"

namespace crl {

constexpr int AMAX = 16;

__device__ __forceinline__ void softmax_rt(const float (&z)[AMAX], int A, float (&p)[AMAX], float (&lp)[AMAX]) {
  float m = z[0];
#pragma unroll
  for (int a = 1; a < AMAX; ++a) if (a < A) m = fmaxf(m, z[a]);
  float s = 0.0f;
#pragma unroll
  for (int a = 0; a < AMAX; ++a) if (a < A) { p[a] = expf(z[a] - m); s += p[a]; }
#pragma unroll
  for (int a = 0; a < AMAX; ++a) if (a < A) p[a] = p[a] / s;
  float ls = 0.0f;
#pragma unroll
  for (int a = 0; a < AMAX; ++a) if (a < A) { lp[a] = z[a] - m; ls += expf(lp[a]); }
  const float l = logf(ls);
#pragma unroll
  for (int a = 0; a < AMAX; ++a) if (a < A) lp[a] = lp[a] - l;
}
__device__ __forceinline__ int sample_rt(const float (&p)[AMAX], int A, double u) {
  float sw = 0.0f;
#pragma unroll
  for (int a = 0; a < AMAX; ++a) if (a < A) sw += p[a];
  const double t = u * (double)sw;
  int i = 0;
  float cw = p[0];
#pragma unroll
  for (int a = 1; a < AMAX; ++a) {
    const bool go = (a < A) && ((double)cw < t) && (i == a - 1);
    i = go ? a : i;
    cw = go ? cw + p[a] : cw;
  }
  return i;
}

}  // namespace crl
