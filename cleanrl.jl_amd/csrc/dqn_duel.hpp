// dqn_duel.hpp — the dueling decomposition of Wang et al. 2016 for dqn.hip: a value stream and an advantage stream behind the shared first layer,
// combined where the head's output is written, out_{a,i} = V_i + (A_{a,i} − (A_{0,i} + A_{1,i})·0.5). R = 1 on a scalar handle (out = Q(a)), R = n_atoms
// on a categorical one (out = the logits c51_softmax takes). The expressions are pinned in include/cleanrl_hip.h ("Dueling heads" block);
// tests/duel_ref.py restates them in numpy. Everything here is Float64 with contraction off; every dot product runs in input order, bias last.
//
// Ten arrays, flat: W1 b1 W2v b2v W3v b3v W2a b2a W3a b3a. The first four sit at the plain net's offsets (W1 b1 W2 b2), so dqn_fwd1_kernel runs
// unchanged on such a handle. The hidden buffers hold 168 units per sample: the value stream at 0..83, the advantage stream at 84..167.
#pragma once
#include "common.hpp"

namespace crl {

constexpr int DUEL_H1 = 120, DUEL_H2 = 84, DUEL_U2 = 2 * DUEL_H2, DUEL_D = 4;
constexpr int DUEL_MAX_R = 64;
constexpr int DUEL_ARRAYS = 10;

struct DuelDev {
  int32_t on, R, P, pad;               // P = 20928 + 255·R parameters
};

// the ten arrays' offsets for a head of R rows per stream output
struct DuelOff {
  int W1, b1, W2v, b2v, W3v, b3v, W2a, b2a, W3a, b3a, P;
};
__host__ __device__ __forceinline__ DuelOff duel_off(int R) {
  DuelOff o;
  o.W1 = 0; o.b1 = DUEL_H1 * DUEL_D; o.W2v = o.b1 + DUEL_H1; o.b2v = o.W2v + DUEL_H2 * DUEL_H1; o.W3v = o.b2v + DUEL_H2; o.b3v = o.W3v + R * DUEL_H2;
  o.W2a = o.b3v + R; o.b2a = o.W2a + DUEL_H2 * DUEL_H1; o.W3a = o.b2a + DUEL_H2; o.b3a = o.W3a + 2 * R * DUEL_H2; o.P = o.b3a + 2 * R;
  return o;
}
constexpr int duel_param_count(int R) { return 20928 + 255 * R; }
static_assert(duel_param_count(1) == 21183 && duel_param_count(51) == 33933, "20 928 + 255·R");

// which of the ten arrays parameter p belongs to (Adam keeps one β-power pair per array)
__device__ __forceinline__ int duel_array_of(const DuelOff& o, int p) {
  return p < o.b1 ? 0 : p < o.W2v ? 1 : p < o.b2v ? 2 : p < o.W3v ? 3 : p < o.b3v ? 4 : p < o.W2a ? 5 : p < o.b2a ? 6 : p < o.W3a ? 7 : p < o.b3a ? 8 : 9;
}

// mean = (A0 + A1)·0.5; out_a = V + (A_a − mean). Halving is exact, so a scalar dueling handle still runs no transcendental.
__device__ __forceinline__ void duel_combine(double V, double A0, double A1, double& out0, double& out1) {
#pragma clang fp contract(off)
  const double mean = (A0 + A1) * 0.5;
  out0 = V + (A0 - mean);
  out1 = V + (A1 - mean);
}

// the cotangent of advantage row (aa, i) given g_i on out_{act,i}: dA_{act,i} = g·0.5, dA_{1−act,i} = −(g·0.5)
__device__ __forceinline__ double duel_dadv(double g, int act, int aa) {
#pragma clang fp contract(off)
  const double half = g * 0.5;
  return aa == act ? half : -half;
}

// one unit of the two-stream hidden layer: u < 84 is value unit u, else advantage unit u − 84; W any float image of the net (global or LDS)
template <typename WP>
__device__ __forceinline__ double duel_hidden2(const WP W, const DuelOff& o, int u, const double* __restrict__ h1) {
#pragma clang fp contract(off)
  const int s = u >= DUEL_H2, j = u - DUEL_H2 * s, w = s ? o.W2a : o.W2v, b = s ? o.b2a : o.b2v;
  double acc = 0.0;
#pragma unroll 8
  for (int kk = 0; kk < DUEL_H1; ++kk) acc += (double)W[w + j + DUEL_H2 * kk] * h1[kk];
  acc += (double)W[b + j];
  return acc > 0.0 ? acc : 0.0;
}

// one row of the stacked heads before they are combined: r < R is V_r (from h2[0..83]), else advantage row r − R = a·R + i (from h2[84..167])
template <typename WP>
__device__ __forceinline__ double duel_head_row(const WP W, const DuelOff& o, int R, int r, const double* __restrict__ h2) {
#pragma clang fp contract(off)
  const bool adv = r >= R;
  const int row = adv ? r - R : r, rows = adv ? 2 * R : R, w = adv ? o.W3a : o.W3v, b = adv ? o.b3a : o.b3v;
  const double* h = h2 + (adv ? DUEL_H2 : 0);
  double acc = 0.0;
#pragma unroll 4
  for (int kk = 0; kk < DUEL_H2; ++kk) acc += (double)W[w + row + rows * kk] * h[kk];
  return acc + (double)W[b + row];
}

}  // namespace crl
