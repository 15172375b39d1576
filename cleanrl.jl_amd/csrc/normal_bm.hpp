// normal_bm.hpp — the library's one Float64 standard normal on the device, stated once: Box–Muller from the two u53 halves of ONE Philox block,
// sqrt(−2·log(1 − u_xy))·cos(2π·u_zw). ddpg.hip's ddpg_normal (behaviour, target, actor and smoothing noise; SAC's ε through sac.hpp) and
// dqn_noisy.hpp's ξ draw both call it, so the expression and its operation order exist in one place.
#pragma once
#include "common.hpp"

namespace crl {

__device__ __forceinline__ double box_muller(const u32x4& o) {
#pragma clang fp contract(off)
  const double u1 = u53(o);
  const double u2 = (double)((((uint64_t)o.z << 32) | o.w) >> 11) * 0x1.0p-53;
  return sqrt(-2.0 * log(1.0 - u1)) * cos(6.283185307179586 * u2);
}

}  // namespace crl
