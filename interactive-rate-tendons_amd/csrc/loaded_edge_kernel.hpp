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
#include "edge_sincos.hpp"

namespace trk {

struct EdgeLoadsK { double wrench[6], dist[6]; int32_t world, pad_; };

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
