// edge_sincos.hpp -- sine and cosine as a fixed sequence of IEEE fp64 operations, shared by the kernels that turn load rows by a
// state's rotation (loaded_edge_kernel.hpp: loaded_sample_loads; fk_loaded_lin_kernel.hpp: the lanes of the loaded IK whose rotation
// is perturbed; loaded_ik_kernel.hpp: the trial states' rows).  No library call, no contraction: a host restatement of the sequence
// (engine.py: edge_sincos) gives the same bits.
#pragma once
#include <hip/hip_runtime.h>

namespace trk {

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

// the 6 numbers (force, moment) of a load row turned by Rz(-theta): Rz(-theta) (x, y, z) = (c x + s y, c y - s x, z)
__device__ __host__ inline void edge_turn_row(const double *w, double s, double c, double *o) {
#pragma clang fp contract(off)
  for (int h = 0; h < 2; h++) {
    o[3 * h + 0] = c * w[3 * h + 0] + s * w[3 * h + 1];
    o[3 * h + 1] = c * w[3 * h + 1] - s * w[3 * h + 0];
    o[3 * h + 2] = w[3 * h + 2];
  }
}

}  // namespace trk
