// tanh64.hpp — NNlib's tanh_fast on Float64 (oracle: a2c_tanh_fast), stated once for a2c.hip and ddpg.hip: the Float32-weight Dense layers of
// a2c.jl / ddpg.jl see Float64 observations, so their activations are Float64. Contraction is off: the polynomial rounds like the CPU oracle's.
#pragma once
#include <hip/hip_runtime.h>

namespace crl {

__device__ __forceinline__ double tanh_fast64(double x) {
#pragma clang fp contract(off)
  const double exp2x = exp(x + x);
  const double y = (exp2x - 1.0) / (exp2x + 1.0);
  const double x2 = x * x;
  double p = -0.008697141630499953;
  p = p * x2 + 0.02186660872609521;
  p = p * x2 + -0.05396823125794372;
  p = p * x2 + 0.13333333325511604;
  p = p * x2 + -0.33333333333324583;
  p = p * x2 + 1.0;
  const double ypoly = x * p;
  if (x2 > 900.0) return (double)((x > 0.0) - (x < 0.0));
  return x2 < 0.017 ? ypoly : y;
}

}  // namespace crl
