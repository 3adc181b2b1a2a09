// tipq_loaded_kernel.hpp -- the device side of the tip-goal queries on LOADED shapes (tr_roadmap_ik_batch_loaded /
// tr_roadmap_solve_tips_loaded / tr_roadmap_set_tips_loaded; roadmap_tips_host.inc).  The IK batch and the pair check turn the
// call's load set per state themselves (loaded_ik_kernel.hpp, loaded_edge_kernel.hpp); what is left to this file:
//   tipql_load_rows   the (F_e, L_e) and (f_e, l_e) rows of m states from the call's one load set: copied (frame BASE) or turned by
//                     Rz(-theta) of the state's own rotation (frame WORLD) with edge_sincos / edge_turn_row -- loaded_sample_loads'
//                     rows and Engine.sample_loads' bit for bit
//   tipql_live_rows   the compaction of the live pairs for rule 5L / 5'L: the last valid state g of every pair that exists goes,
//                     in pair order, into a dense array with its load rows beside it (one cold shooting solve each, never one of
//                     a dead pair)
//   tipql_scatter     the solves' tips, converged flags and base strains back to their pairs
//   tipql_select      rules 4L / 5L and 4'L / 5'L, one lane per request: tipq_select_pairs with the equilibrium mask on REACHED,
//                     the converged mask on the CLOSEST candidates and the strains of the chosen state gathered.  P = 1 with
//                     src = the neighbour table is the one-edge rule (tipq_select's walk)
// IEEE fp64 without contraction, no library sine or cosine: a host restatement gives the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "stateq_kernel.hpp"
#include "edge_sincos.hpp"

namespace trk {

struct TipqLoadsK { double wrench[6], dist[6]; int32_t world, pad_; };

// the two rows of one state; theta_col < 0: the robot does not turn
__device__ __forceinline__ void tipql_rows_of(const double *__restrict__ state, int theta_col, const TipqLoadsK &k, double *__restrict__ w,
                                              double *__restrict__ d) {
#pragma clang fp contract(off)
  if (!k.world || theta_col < 0) {
    for (int q = 0; q < 6; q++) { w[q] = k.wrench[q]; d[q] = k.dist[q]; }
    return;
  }
  double s, c;
  edge_sincos(state[theta_col], s, c);
  edge_turn_row(k.wrench, s, c, w);
  edge_turn_row(k.dist, s, c, d);
}

__global__ __launch_bounds__(256) void tipql_load_rows(const double *__restrict__ states, int64_t m, int S, int theta_col, TipqLoadsK k,
                                                       double *__restrict__ wrench, double *__restrict__ dist) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  tipql_rows_of(states + i * S, theta_col, k, wrench + i * 6, dist + i * 6);
}

// live[i] = the pair whose state g[live[i]] becomes row i of gl; its load rows beside it
__global__ __launch_bounds__(256) void tipql_live_rows(const double *__restrict__ g, const int32_t *__restrict__ live, int64_t ml, int S,
                                                       int theta_col, TipqLoadsK k, double *__restrict__ gl, double *__restrict__ wrench,
                                                       double *__restrict__ dist) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= ml) return;
  const int64_t p = live[i];
  for (int d = 0; d < S; d++) gl[i * S + d] = g[p * S + d];
  tipql_rows_of(g + p * S, theta_col, k, wrench + i * 6, dist + i * 6);
}

// row i of the dense results -> pair live[i] (gconv was cleared: a dead pair has converged = 0)
__global__ __launch_bounds__(256) void tipql_scatter(const int32_t *__restrict__ live, int64_t ml, const double *__restrict__ tipc,
                                                     const uint8_t *__restrict__ convc, const double *__restrict__ vuc,
                                                     double *__restrict__ gtip, uint8_t *__restrict__ gconv, double *__restrict__ gvu) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= ml) return;
  const int64_t p = live[i];
  for (int d = 0; d < 3; d++) gtip[p * 3 + d] = tipc[i * 3 + d];
  for (int d = 0; d < 6; d++) gvu[p * 6 + d] = vuc[i * 6 + d];
  gconv[p] = convc[i];
}

// Rules 4L - 5L (P = 1, src = nbr) and 4'L - 5'L, one lane per request over its k slots of P pairs each.  Per slot: x / xtip / err /
// eq / xvu = the loaded IK's result; per pair: src, ok / t = checkMotion(states[src], x, last_valid) on loaded samples, g / gtip /
// gconv / gvu = the interpolated state and its cold loaded solve.
//   REACHED: the first pair in (slot, source) order with err < tolerance, eq and ok -> (x, xtip, err, t = 1, xvu)
//   CLOSEST: otherwise, among the pairs whose g converged, the one whose gtip is nearest the request, the first winning a tie
//            -> (g, gtip, |gtip - request|, t, gvu)
//   NO_NEIGHBOR: the row is empty, or no pair's g has an equilibrium -> NaN outputs, vertices -1
__global__ __launch_bounds__(256) void tipql_select(const int32_t *__restrict__ nbr, const double *__restrict__ req, int64_t n, int k, int P, int S,
                                                    double tolerance, const int32_t *__restrict__ src, const double *__restrict__ x,
                                                    const double *__restrict__ xtip, const double *__restrict__ err,
                                                    const uint8_t *__restrict__ eq, const double *__restrict__ xvu,
                                                    const uint8_t *__restrict__ ok, const double *__restrict__ t,
                                                    const double *__restrict__ g, const double *__restrict__ gtip,
                                                    const uint8_t *__restrict__ gconv, const double *__restrict__ gvu,
                                                    double *__restrict__ controls, double *__restrict__ tip_out, double *__restrict__ err_out,
                                                    int32_t *__restrict__ nbr_out, int32_t *__restrict__ ik_out, int32_t *__restrict__ outcome,
                                                    double *__restrict__ t_out, double *__restrict__ vu_out, uint8_t *__restrict__ flags) {
#pragma clang fp contract(off)
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= n) return;
  const double rx = req[q * 3], ry = req[q * 3 + 1], rz = req[q * 3 + 2];
  int64_t best = -1, hit = -1;
  int best_slot = -1, hit_slot = -1;
  double best_e = 1.0 / 0.0;
  bool plain_hit = false;
  for (int i = 0; i < k; i++) {
    const int64_t slot = q * k + i;
    const int32_t nv = nbr[slot];
    if (nv < 0) break;                                                  // (rows are filled from the front)
    const bool within = err[slot] < tolerance && eq[slot] != 0;
    for (int j = 0; j < P; j++) {
      const int64_t p = slot * P + j;
      const int32_t v = src[p];
      if (v < 0) continue;
      const bool reaches = within && ok[p];
      if (reaches && v == nv) plain_hit = true;
      if (hit >= 0) continue;                                           // (the answer is known; the rest of the walk is for `plain_hit`)
      if (reaches) { hit = p; hit_slot = i; continue; }
      if (!gconv[p]) continue;                                          // a state without an equilibrium is never a goal
      const double dx = gtip[p * 3] - rx, dy = gtip[p * 3 + 1] - ry, dz = gtip[p * 3 + 2] - rz;
      const double e = sqrt((dx * dx + dy * dy) + dz * dz);
      if (best < 0 || e < best_e) { best = p; best_slot = i; best_e = e; }
    }
  }
  const bool reached = hit >= 0;
  const int64_t p = reached ? hit : best;
  if (p < 0) {
    const double nan_ = __longlong_as_double(0x7ff8000000000000LL);
    for (int d = 0; d < S; d++) controls[q * S + d] = nan_;
    for (int d = 0; d < 3; d++) tip_out[q * 3 + d] = nan_;
    for (int d = 0; d < 6; d++) vu_out[q * 6 + d] = nan_;
    err_out[q] = nan_; t_out[q] = nan_; nbr_out[q] = -1; ik_out[q] = -1;
    outcome[q] = TRK_TIPQ_NO_NEIGHBOR;
    flags[q] = 0;
    return;
  }
  const int64_t slot = q * k + (reached ? hit_slot : best_slot);
  outcome[q] = reached ? TRK_TIPQ_REACHED : TRK_TIPQ_CLOSEST;
  for (int d = 0; d < S; d++) controls[q * S + d] = reached ? x[slot * S + d] : g[p * S + d];
  for (int d = 0; d < 3; d++) tip_out[q * 3 + d] = reached ? xtip[slot * 3 + d] : gtip[p * 3 + d];
  for (int d = 0; d < 6; d++) vu_out[q * 6 + d] = reached ? xvu[slot * 6 + d] : gvu[p * 6 + d];
  err_out[q] = reached ? err[slot] : best_e;
  t_out[q] = reached ? 1.0 : t[p];
  nbr_out[q] = src[p];
  ik_out[q] = nbr[slot];
  flags[q] = (uint8_t)((reached ? TRK_TIPQ_FLAG_REACHED : 0) | (src[p] != nbr[slot] ? TRK_TIPQ_FLAG_MOVED : 0) |
                       (reached && !plain_hit ? TRK_TIPQ_FLAG_GAINED : 0));
}

}  // namespace trk
