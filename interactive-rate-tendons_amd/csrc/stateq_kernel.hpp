// stateq_kernel.hpp -- nearest roadmap vertices of arbitrary states (tr_roadmap_nearest_states) and the device side of the accurate
// connection rule of the tip queries (tr_roadmap_ik_batch_connect / tr_roadmap_solve_tips_connect; host glue in roadmap_tips_host.inc):
//   state_knn          exact k nearest valid roadmap vertices per query STATE, order (distance, vertex index), over a
//                      structure-of-arrays copy of the states ([S][V]); tip_knn's shape, knn_wave_query's metric
//   tipq_pair_rows     the (source vertex, IK answer) pairs of rule 3': per candidate slot its state-space neighbours C_i and, last, the
//                      vertex IK started from when C_i does not hold it
//   tipq_select_pairs  rules 4' - 5' over the pairs of a request, one lane per request; the one-edge rule's verdict in the same pass
// The lists of a query live across the lanes exactly as tip_knn's do (TipList) and tip_knn_merge merges the slices.  Everything is
// fp64 without contraction, in the arithmetic of knn_kernel.hpp: a numpy restatement gives the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tipq_kernel.hpp"

namespace trk {

// queries per wave and tiles in flight by state size: the queries sit in scalar registers (Q SS doubles), the tiles in vector
// registers (G SS doubles per lane); the larger states take fewer of both so that nothing spills
__host__ __device__ constexpr int stateq_q(int ss) { return ss <= 6 ? 4 : 2; }
__host__ __device__ constexpr int stateq_g(int ss) { return ss <= 4 ? 4 : 2; }

// CompoundStateSpace::distance (Problem.cpp:112-152) as knn_wave_query forms it: x the query, c the candidate
template <int NT, bool ROT, bool RET>
__device__ __forceinline__ double stateq_distance(const double *x, const double *c, double w_rot, double w_ret) {
#pragma clang fp contract(off)
  double s2 = 0.0;
#pragma unroll
  for (int d = 0; d < NT; d++) { const double t = x[d] - c[d]; s2 += t * t; }
  double dist = sqrt(s2);
  if constexpr (ROT) {                                      // SO2StateSpace::distance
    double a_ = fabs(x[NT] - c[NT]);
    a_ = (a_ > 3.14159265358979323846) ? 2.0 * 3.14159265358979323846 - a_ : a_;
    dist += w_rot * a_;
  }
  if constexpr (RET) {
    constexpr int R = NT + (ROT ? 1 : 0);
    const double t = x[R] - c[R];
    dist += w_ret * sqrt(t * t);
  }
  return dist;
}

// A wave serves Q queries; its 64 lanes each take one vertex of a tile (G tiles in flight), so a tile is read once for all Q.
// blockIdx.y = slice of the vertex array.  Output rows [query][slice][k] (-1 / +inf where fewer than k vertices qualify or the
// entry lies beyond max_dist: the lists are ordered, so those are a suffix).  soa: coordinate d of vertex v at soa[d V + v].
template <int NT, bool ROT, bool RET, int Q, int G>
__global__ __launch_bounds__(256) void state_knn(const double *__restrict__ soa, const uint8_t *__restrict__ vstat, int64_t V,
                                                 const double *__restrict__ qry, int64_t n, int k, double w_rot, double w_ret,
                                                 double max_dist, int32_t *__restrict__ out_idx, double *__restrict__ out_d) {
#pragma clang fp contract(off)
  constexpr int SS = NT + (ROT ? 1 : 0) + (RET ? 1 : 0);
  const int lane = threadIdx.x & 63;
  const int64_t q0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * Q;
  if (q0 >= n) return;                                                  // wave-uniform
  const int slices = (int)gridDim.y, slice = (int)blockIdx.y;
  // slices start at multiples of 64 vertices
  const int64_t tiles = (V + 63) / 64;
  const int64_t a = (tiles * slice / slices) * 64;
  int64_t b = (tiles * (slice + 1) / slices) * 64;
  b = b < V ? b : V;
  double x[Q][SS];
  TipList l[Q];
#pragma unroll
  for (int q = 0; q < Q; q++) {
    const int64_t qi = q0 + q < n ? q0 + q : n - 1;                     // (a query beyond n repeats the last one; it is not written)
#pragma unroll
    for (int d = 0; d < SS; d++) x[q][d] = qry[qi * SS + d];
    tip_list_init(l[q], lane, k);
  }
  for (int64_t jt = a; jt < b; jt += 64 * G) {
    double c[G][SS];
    bool live[G];
#pragma unroll
    for (int g = 0; g < G; g++) {
      const int64_t j = jt + 64 * g + lane;
      const bool have = j < b;
      const int64_t jl = have ? j : b - 1;
#pragma unroll
      for (int d = 0; d < SS; d++) c[g][d] = soa[(int64_t)d * V + jl];
      live[g] = have && vstat[jl] == 1;
    }
#pragma unroll
    for (int g = 0; g < G; g++) {
      if (jt + 64 * g >= b) break;                                      // wave-uniform
      const int32_t cj = (int32_t)(jt + 64 * g + lane);
#pragma unroll
      for (int q = 0; q < Q; q++) {
        const double dist = stateq_distance<NT, ROT, RET>(x[q], c[g], w_rot, w_ret);
        unsigned long long mk = __ballot(live[g] && dist <= l[q].worst);
        while (mk) {
          const int src = __builtin_ctzll(mk);
          mk &= mk - 1;
          const double cd = tipq_lane_value(dist, src);
          const int32_t ci = __builtin_amdgcn_readlane(cj, src);
          if (tip_list_takes(l[q], cd, ci)) tip_list_insert(l[q], lane, k, cd, ci);      // against the CURRENT threshold
        }
      }
    }
  }
  if (lane < k) {
#pragma unroll
    for (int q = 0; q < Q; q++) {
      if (q0 + q >= n) break;
      const int64_t o = ((q0 + q) * slices + slice) * k + lane;
      const bool keep = l[q].i >= 0 && !(l[q].d > max_dist);
      out_idx[o] = keep ? l[q].i : -1;
      if (out_d) out_d[o] = keep ? l[q].d : 1.0 / 0.0;
    }
  }
}

// Rule 3', one lane per pair: slot i (a candidate of a request: neighbour N_i, IK answer x_i) has P = kc + 1 pairs; pair j < kc
// starts at C_i[j], pair kc at N_i unless C_i holds N_i already (:3238-3241).  src = the source vertex, -1 where the pair does not
// exist (an empty slot, a padded C entry, N_i repeated); a / b = the rows tipq_interp and the edge check read (a dead pair: x_i twice).
__global__ __launch_bounds__(256) void tipq_pair_rows(const double *__restrict__ states, int S, const int32_t *__restrict__ nbr,
                                                      const int32_t *__restrict__ cidx, const double *__restrict__ x, int64_t m, int kc,
                                                      int32_t *__restrict__ src, double *__restrict__ a, double *__restrict__ b) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int P = kc + 1;
  if (p >= m * P) return;
  const int64_t i = p / P;
  const int j = (int)(p - i * P);
  const int32_t nv = nbr[i];
  int32_t v = -1;
  if (nv >= 0) {
    if (j < kc) {
      v = cidx[i * kc + j];
    } else {
      v = nv;
      for (int e = 0; e < kc; e++) if (cidx[i * kc + e] == nv) v = -1;
    }
  }
  src[p] = v;
  for (int d = 0; d < S; d++) {
    const double xd = x[i * S + d];
    a[p * S + d] = v >= 0 ? states[(int64_t)v * S + d] : xd;
    b[p * S + d] = xd;
  }
}

#define TRK_TIPQ_FLAG_REACHED 1       // the request is REACHED
#define TRK_TIPQ_FLAG_MOVED 2         // its connection vertex is not the vertex IK started from
#define TRK_TIPQ_FLAG_GAINED 4        // REACHED, and no pair (i, N_i) alone reaches it: the one-edge rule would have said CLOSEST

// Rules 4' - 5', one lane per request over its k slots of P pairs each.  Per slot: x / xtip / err = the IK result; per pair:
// src, ok / t = checkMotion(states[src], x, last_valid), g / gtip = the interpolated state and its FK tip.
//   REACHED: the first pair in (slot, source) order with err < tolerance and ok -> (x, xtip, err, t = 1)
//   CLOSEST: otherwise the pair whose gtip is nearest the request, the first winning a tie -> (g, gtip, |gtip - request|, t)
//   NO_NEIGHBOR: the row is empty -> NaN outputs, vertices -1
__global__ __launch_bounds__(256) void tipq_select_pairs(const int32_t *__restrict__ nbr, const double *__restrict__ req, int64_t n, int k, int P,
                                                         int S, double tolerance, const int32_t *__restrict__ src, const double *__restrict__ x,
                                                         const double *__restrict__ xtip, const double *__restrict__ err,
                                                         const uint8_t *__restrict__ ok, const double *__restrict__ t,
                                                         const double *__restrict__ g, const double *__restrict__ gtip,
                                                         double *__restrict__ controls, double *__restrict__ tip_out,
                                                         double *__restrict__ err_out, int32_t *__restrict__ nbr_out,
                                                         int32_t *__restrict__ ik_out, int32_t *__restrict__ outcome,
                                                         double *__restrict__ t_out, uint8_t *__restrict__ flags) {
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
    const bool within = err[slot] < tolerance;
    for (int j = 0; j < P; j++) {
      const int64_t p = slot * P + j;
      const int32_t v = src[p];
      if (v < 0) continue;
      const bool reaches = within && ok[p];
      if (reaches && v == nv) plain_hit = true;
      if (hit >= 0) continue;                                           // (the answer is known; the rest of the walk is for `plain_hit`)
      if (reaches) { hit = p; hit_slot = i; continue; }
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
    err_out[q] = nan_; t_out[q] = nan_; nbr_out[q] = -1; ik_out[q] = -1;
    outcome[q] = TRK_TIPQ_NO_NEIGHBOR;
    flags[q] = 0;
    return;
  }
  const int64_t slot = q * k + (reached ? hit_slot : best_slot);
  outcome[q] = reached ? TRK_TIPQ_REACHED : TRK_TIPQ_CLOSEST;
  for (int d = 0; d < S; d++) controls[q * S + d] = reached ? x[slot * S + d] : g[p * S + d];
  for (int d = 0; d < 3; d++) tip_out[q * 3 + d] = reached ? xtip[slot * 3 + d] : gtip[p * 3 + d];
  err_out[q] = reached ? err[slot] : best_e;
  t_out[q] = reached ? 1.0 : t[p];
  nbr_out[q] = src[p];
  ik_out[q] = nbr[slot];
  flags[q] = (uint8_t)((reached ? TRK_TIPQ_FLAG_REACHED : 0) | (src[p] != nbr[slot] ? TRK_TIPQ_FLAG_MOVED : 0) |
                       (reached && !plain_hit ? TRK_TIPQ_FLAG_GAINED : 0));
}

}  // namespace trk
