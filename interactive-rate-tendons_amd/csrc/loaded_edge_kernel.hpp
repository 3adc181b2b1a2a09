// loaded_edge_kernel.hpp -- the per-sample helpers of the loaded edge check (loaded_edges_host.inc): checkMotion with every FK sample
// taken from the loaded FK (fk_loaded_kernel.hpp), as the reference does after AbstractValidityChecker::set_fk_func has swapped the
// checker's FK for TendonRobot::general_shape.
//
//   loaded_sample_loads   the (F_e, L_e) and (f_e, l_e) rows of every sample of a level from the call's one load set: copied (frame
//                         BASE: fixed before the state's rotation, as tr_fk_loaded_batch takes them) or turned by Rz(-theta) of the
//                         sample's own rotation (frame WORLD: fixed behind rotate_z, e.g. gravity on a robot that turns about z)
//   loaded_sample_guess   warm start: the start strains of a midpoint are the accepted base strains of its interval's sample at t_a
//   loaded_sample_tally   samples whose shooting did not converge, and the integrations of all samples, summed per run
//
// IEEE fp64 without contraction throughout, and no library sine or cosine: edge_sincos is a fixed sequence of IEEE operations
// (two-term reduction by pi/2, Taylor polynomials in Horner form), so that a host restatement of it gives the same bits and the
// rotated rows -- with them the shapes and the bisection -- can be reproduced outside the library.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "edge_kernel.hpp"

namespace trk {

struct EdgeLoadsK { double wrench[6], dist[6]; int32_t world, pad_; };

// sin and cos of x, |x| of a few turns at most, to ~1e-16: k = rint(x 2/pi), r = (x - k hi) - k lo with hi the leading 33 bits of
// pi/2 (k hi is exact), sin r and cos r by their Taylor polynomials to r^17 and r^18 (|r| <= pi/4: the next terms are below 1e-18)
__device__ __host__ inline void edge_sincos(double x, double &s, double &c) {
#pragma clang fp contract(off)
  const double k = rint(x * 0.63661977236758138);                       // 2 / pi
  const double r = (x - k * 1.57079632673412561417e+00) - k * 6.07710050650619224932e-11;
  const double z = r * r;
  double ps = 1.0 / 355687428096000.0;                                  // 1 / 17!
  ps = -1.0 / 1307674368000.0 + z * ps;                                 // 15!
  ps = 1.0 / 6227020800.0 + z * ps;                                     // 13!
  ps = -1.0 / 39916800.0 + z * ps;                                      // 11!
  ps = 1.0 / 362880.0 + z * ps;                                         // 9!
  ps = -1.0 / 5040.0 + z * ps;                                          // 7!
  ps = 1.0 / 120.0 + z * ps;                                            // 5!
  ps = -1.0 / 6.0 + z * ps;                                             // 3!
  const double sr = r + r * (z * ps);
  double pc = -1.0 / 6402373705728000.0;                                // 18!
  pc = 1.0 / 20922789888000.0 + z * pc;                                 // 16!
  pc = -1.0 / 87178291200.0 + z * pc;                                   // 14!
  pc = 1.0 / 479001600.0 + z * pc;                                      // 12!
  pc = -1.0 / 3628800.0 + z * pc;                                       // 10!
  pc = 1.0 / 40320.0 + z * pc;                                          // 8!
  pc = -1.0 / 720.0 + z * pc;                                           // 6!
  pc = 1.0 / 24.0 + z * pc;                                             // 4!
  pc = -0.5 + z * pc;                                                   // 2!
  const double cr = 1.0 + z * pc;
  const int q = (int)((long long)k & 3);                                // quadrant (two's complement: also for negative k)
  s = q == 0 ? sr : (q == 1 ? cr : (q == 2 ? -sr : -cr));
  c = q == 0 ? cr : (q == 1 ? -sr : (q == 2 ? -cr : sr));
}

// rows [m][6] of the tip wrench and of the distributed load for the m states of a level; theta_col < 0: the rows are the call's
__global__ __launch_bounds__(256) void loaded_sample_loads(const double *__restrict__ states, int64_t m, int S, int theta_col, EdgeLoadsK k,
                                                           double *__restrict__ wrench, double *__restrict__ dist) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  if (!k.world || theta_col < 0) {
    for (int q = 0; q < 6; q++) { wrench[i * 6 + q] = k.wrench[q]; dist[i * 6 + q] = k.dist[q]; }
    return;
  }
  double s, c;
  edge_sincos(states[i * S + theta_col], s, c);
  // Rz(-theta) (x, y, z) = (c x + s y, c y - s x, z)
  for (int h = 0; h < 2; h++) {
    const double *w = k.wrench + 3 * h, *d = k.dist + 3 * h;
    wrench[i * 6 + 3 * h + 0] = c * w[0] + s * w[1];
    wrench[i * 6 + 3 * h + 1] = c * w[1] - s * w[0];
    wrench[i * 6 + 3 * h + 2] = w[2];
    dist[i * 6 + 3 * h + 0] = c * d[0] + s * d[1];
    dist[i * 6 + 3 * h + 1] = c * d[1] - s * d[0];
    dist[i * 6 + 3 * h + 2] = d[2];
  }
}

// guess[q] = vu_pool[open[q].sa]: only intervals whose sample at t_a is valid are opened (edge_filter), so it has converged
__global__ __launch_bounds__(256) void loaded_sample_guess(const EdgeIv *__restrict__ open, int64_t m, int64_t cap, const double *__restrict__ vu_pool,
                                                           double *__restrict__ guess) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= m * 6) return;
  const int64_t q = t / 6, j = t - q * 6;
  const int64_t sa = open[q].sa;
  guess[t] = (sa >= 0 && sa < cap) ? vu_pool[sa * 6 + j] : 0.0;
}

// tally[0] += samples of the m that did not converge, tally[1] += their integrations
__global__ __launch_bounds__(256) void loaded_sample_tally(const uint8_t *__restrict__ conv, const int32_t *__restrict__ calls, int64_t m,
                                                           unsigned long long *__restrict__ tally) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = i < m;
  const unsigned long long bad = __ballot(live && conv[i] == 0);
  long long n = live ? (long long)calls[i] : 0;
  for (int o = 32; o > 0; o >>= 1) n += __shfl_down(n, o);
  if ((threadIdx.x & 63) == 0) {
    if (bad) atomicAdd(&tally[0], (unsigned long long)__popcll(bad));
    if (n) atomicAdd(&tally[1], (unsigned long long)n);
  }
}

}  // namespace trk
