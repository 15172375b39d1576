// env64.hpp — the reference's single CartPoleEnv{Float64} of a2c.jl / dqn.jl (oracle: a2c_sin, a2c_cos, a2c_cartpole_step): one statement for a2c.hip and dqn.hip.
// Contraction is off in the step and the reset so that they round like the CPU oracle's; the polynomials are explicit fma chains.
#pragma once
#include "common.hpp"

namespace crl {

__device__ __forceinline__ double sin64(double x) {
  const double c[10] = {-1.0 / 6, 1.0 / 120, -1.0 / 5040, 1.0 / 362880, -1.0 / 39916800, 1.0 / 6227020800.0,
                        -1.0 / 1307674368000.0, 1.0 / 355687428096000.0, -1.0 / 121645100408832000.0,
                        1.0 / 51090942171709440000.0};
  const double x2 = x * x;
  double p = c[9];
#pragma unroll
  for (int i = 8; i >= 0; --i) p = __builtin_fma(p, x2, c[i]);
  return __builtin_fma(x * x2, p, x);
}
__device__ __forceinline__ double cos64(double x) {
  const double c[10] = {-0.5, 1.0 / 24, -1.0 / 720, 1.0 / 40320, -1.0 / 3628800, 1.0 / 479001600.0,
                        -1.0 / 87178291200.0, 1.0 / 20922789888000.0, -1.0 / 6402373705728000.0,
                        1.0 / 2432902008176640000.0};
  const double x2 = x * x;
  double p = c[9];
#pragma unroll
  for (int i = 8; i >= 0; --i) p = __builtin_fma(p, x2, c[i]);
  return __builtin_fma(x2, p, 1.0);
}
__device__ __forceinline__ bool cartpole_step64(double* s, int& t, int action, int max_steps) {
#pragma clang fp contract(off)
  const double gravity = 9.8, masspole = 0.1, totalmass = 1.1, halflength = 0.5, pml = 0.05;
  const double forcemag = 10.0, dt = 0.02, ththr = 12.0 * 2.0 * 3.141592653589793 / 360.0, xthr = 2.4;
  t += 1;
  const double force = action == 1 ? forcemag : -forcemag;
  const double xdot = s[1], theta = s[2], thetadot = s[3];
  const double costheta = cos64(theta), sintheta = sin64(theta);
  const double tmp = (force + pml * thetadot * thetadot * sintheta) / totalmass;
  const double thetaacc = (gravity * sintheta - costheta * tmp) / (halflength * (4.0 / 3.0 - masspole * costheta * costheta / totalmass));
  const double xacc = tmp - pml * thetaacc * costheta / totalmass;
  s[0] += dt * xdot;
  s[1] += dt * xacc;
  s[2] += dt * thetadot;
  s[3] += dt * thetaacc;
  return (fabs(s[0]) > xthr) || (fabs(s[2]) > ththr) || (t > max_steps);
}
__device__ __forceinline__ void env_reset64(double* s, uint64_t seed, uint64_t gstep, uint32_t stream) {
#pragma clang fp contract(off)
#pragma unroll
  for (int i = 0; i < 4; ++i) s[i] = 0.1 * u53(philox_env(seed, (uint32_t)i, gstep, stream)) - 0.05;
}

}  // namespace crl
