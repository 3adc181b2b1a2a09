// tipq_kernel.hpp -- the device side of the batched tip-goal queries (tr_roadmap_nearest_tips / tr_roadmap_ik_batch /
// tr_roadmap_solve_tips; host glue in roadmap_tips_host.inc):
//   tip_knn        exact k nearest roadmap tips per request over the valid vertices that have a tip, order (d2, vertex index)
//   tip_knn_merge  the ordered lists of the slices of one request into one (few requests: the tip array is cut into slices so that
//                  more than a handful of waves stream it)
//   tipq_gather    IK start rows and repeated goals from the neighbour table, straight from the device copy of the states
//   tipq_interp    interpolate(states[N_i], x_i, t_i) for every candidate (the state checkMotion's last_valid names)
//   tipq_select    the accept / step-back rule of roadmapIk (motion-planning/VoxelCachedLazyPRM.cpp:3214-3287, :3445-3521), one
//                  lane per request over its k candidates
// Everything is fp64 without contraction: numpy restates d2, the interpolation and the error bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace trk {

#define TRK_TIPQ_MAX_K 64
#define TRK_TIPQ_REACHED 0
#define TRK_TIPQ_CLOSEST 1
#define TRK_TIPQ_NO_NEIGHBOR 2

__device__ __forceinline__ double tipq_lane_value(double v, int src) {      // src wave-uniform
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), src), __builtin_amdgcn_readlane(__double2loint(v), src));
}

// The k best of one request live one per lane, ORDERED by (d2, index): lane e < k holds the e-th entry (+inf / -1 while empty),
// lanes >= k an inert (-inf, 0).  An accepted candidate shifts the entries that sort after it one lane up and the last one falls
// out (knn_kernel.hpp: knn_wave_query keeps its lists the same way); the threshold is whatever lane k - 1 then holds.
struct TipList {
  double d;        // per lane
  int32_t i;       // per lane
  double worst;    // wave-uniform: lane k - 1's entry
  int32_t worst_i;
};

__device__ __forceinline__ void tip_list_init(TipList &l, int lane, int k) {
  l.d = lane < k ? 1.0 / 0.0 : -1.0 / 0.0;
  l.i = lane < k ? -1 : 0;
  l.worst = 1.0 / 0.0;
  l.worst_i = -1;
}

// (cd, ci) wave-uniform; the caller has checked that it sorts before the list's last entry
__device__ __forceinline__ void tip_list_insert(TipList &l, int lane, int k, double cd, int32_t ci) {
  const bool after = lane < k && (l.i < 0 || cd < l.d || (cd == l.d && ci < l.i));      // my entry sorts after the new one
  const int prev_after = __shfl_up((int)after, 1, 64);
  const double pd = __shfl_up(l.d, 1, 64);
  const int32_t pi = __shfl_up(l.i, 1, 64);
  if (after) {
    const bool from_prev = lane > 0 && prev_after != 0;
    l.d = from_prev ? pd : cd;
    l.i = from_prev ? pi : ci;
  }
  l.worst = tipq_lane_value(l.d, k - 1);
  l.worst_i = __builtin_amdgcn_readlane(l.i, k - 1);
}

__device__ __forceinline__ bool tip_list_takes(const TipList &l, double cd, int32_t ci) {
  return cd < l.worst || (cd == l.worst && (l.worst_i < 0 || ci < l.worst_i));
}

// A wave serves Q requests; its 64 lanes each take one tip of a tile (G tiles in flight), so a tile is read once for all Q.
// blockIdx.y = slice of the tip array.  Output rows [request][slice][k]: with one slice that is the final table (-1 / +inf where
// fewer than k vertices qualify).  vstat: the roadmap's validity bytes (1 = valid); present: one bit per vertex that has a tip.
template <int Q, int G>
__global__ __launch_bounds__(256) void tip_knn(const double *__restrict__ tips, const uint8_t *__restrict__ vstat,
                                               const uint64_t *__restrict__ present, int64_t V, const double *__restrict__ req, int64_t n,
                                               int k, int32_t *__restrict__ out_idx, double *__restrict__ out_d2) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int64_t q0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * Q;
  if (q0 >= n) return;                                                  // wave-uniform
  const int slices = (int)gridDim.y, slice = (int)blockIdx.y;
  // slices start at multiples of 64 tips
  const int64_t tiles = (V + 63) / 64;
  const int64_t a = (tiles * slice / slices) * 64;
  int64_t b = (tiles * (slice + 1) / slices) * 64;
  b = b < V ? b : V;
  double rx[Q], ry[Q], rz[Q];
  TipList l[Q];
#pragma unroll
  for (int q = 0; q < Q; q++) {
    const int64_t qi = q0 + q < n ? q0 + q : n - 1;                     // (a request beyond n repeats the last one; it is not written)
    rx[q] = req[qi * 3]; ry[q] = req[qi * 3 + 1]; rz[q] = req[qi * 3 + 2];
    tip_list_init(l[q], lane, k);
  }
  for (int64_t jt = a; jt < b; jt += 64 * G) {
    double tx[G], ty[G], tz[G];
    bool live[G];
#pragma unroll
    for (int g = 0; g < G; g++) {
      const int64_t j = jt + 64 * g + lane;
      const bool have = j < b;
      const int64_t jl = have ? j : b - 1;
      tx[g] = tips[jl * 3]; ty[g] = tips[jl * 3 + 1]; tz[g] = tips[jl * 3 + 2];
      live[g] = have && vstat[jl] == 1 && ((present[jl >> 6] >> (jl & 63)) & 1);
    }
#pragma unroll
    for (int g = 0; g < G; g++) {
      if (jt + 64 * g >= b) break;                                      // wave-uniform
      const int32_t cj = (int32_t)(jt + 64 * g + lane);
#pragma unroll
      for (int q = 0; q < Q; q++) {
        const double dx = tx[g] - rx[q], dy = ty[g] - ry[q], dz = tz[g] - rz[q];
        const double d2 = (dx * dx + dy * dy) + dz * dz;
        unsigned long long mk = __ballot(live[g] && d2 <= l[q].worst);
        while (mk) {
          const int src = __builtin_ctzll(mk);
          mk &= mk - 1;
          const double cd = tipq_lane_value(d2, src);
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
      out_idx[o] = l[q].i;
      if (out_d2) out_d2[o] = l[q].d;
    }
  }
}

// One wave per request: the slices' lists [request][slice][k] are candidates like any other (the order (d2, index) is total, so
// the k best of the union of the slices' k best are the k best of all).
__global__ __launch_bounds__(256) void tip_knn_merge(const int32_t *__restrict__ part_idx, const double *__restrict__ part_d2, int64_t n,
                                                     int slices, int k, int32_t *__restrict__ out_idx, double *__restrict__ out_d2) {
  const int lane = threadIdx.x & 63;
  const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= n) return;                                                   // wave-uniform
  TipList l;
  tip_list_init(l, lane, k);
  const int64_t m = (int64_t)slices * k;
  for (int64_t jt = 0; jt < m; jt += 64) {
    const int64_t j = jt + lane;
    const bool have = j < m;
    const int32_t cj = have ? part_idx[q * m + j] : -1;
    const double d2 = have ? part_d2[q * m + j] : 1.0 / 0.0;
    unsigned long long mk = __ballot(cj >= 0 && d2 <= l.worst);
    while (mk) {
      const int src = __builtin_ctzll(mk);
      mk &= mk - 1;
      const double cd = tipq_lane_value(d2, src);
      const int32_t ci = __builtin_amdgcn_readlane(cj, src);
      if (tip_list_takes(l, cd, ci)) tip_list_insert(l, lane, k, cd, ci);
    }
  }
  if (lane < k) {
    out_idx[q * k + lane] = l.i;
    if (out_d2) out_d2[q * k + lane] = l.d;
  }
}

// One lane per (request, candidate) slot: the IK start row states[N] and the request as its goal.  An empty slot (-1: fewer than
// k vertices qualify) repeats the row's first neighbour (vertex 0 when the row has none) so that the IK batch stays dense; the
// selection never looks at it.
__global__ __launch_bounds__(256) void tipq_gather(const double *__restrict__ states, int S, const int32_t *__restrict__ nbr,
                                                   const double *__restrict__ req, int64_t n, int k, double *__restrict__ starts,
                                                   double *__restrict__ goals) {
  const int64_t slot = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= n * k) return;
  const int64_t q = slot / k;
  int32_t v = nbr[slot];
  if (v < 0) v = nbr[q * k];
  if (v < 0) v = 0;
  for (int d = 0; d < S; d++) starts[slot * S + d] = states[(int64_t)v * S + d];
  for (int d = 0; d < 3; d++) goals[slot * 3 + d] = req[q * 3 + d];
}

// CompoundStateSpace::interpolate as Problem.cpp:101-163 wires the space: linear, the shortest arc on the SO2 rotation
// (rot_index < 0: no rotation coordinate).  One lane per slot.
__global__ __launch_bounds__(256) void tipq_interp(const double *__restrict__ a, const double *__restrict__ b, const double *__restrict__ t,
                                                   int64_t m, int S, int rot_index, double *__restrict__ out) {
#pragma clang fp contract(off)
  const int64_t slot = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= m) return;
  const double tt = t[slot];
  for (int d = 0; d < S; d++) {
    const double x = a[slot * S + d], y = b[slot * S + d];
    double v = x + (y - x) * tt;
    if (d == rot_index) {
      const double kPi = 3.14159265358979323846;
      double diff = y - x;
      if (fabs(diff) > kPi) {
        diff = diff > 0.0 ? 2.0 * kPi - diff : -2.0 * kPi - diff;
        v = x - diff * tt;
        if (v > kPi) v -= 2.0 * kPi; else if (v < -kPi) v += 2.0 * kPi;
      }
    }
    out[slot * S + d] = v;
  }
}

// Rules 4 - 5, one lane per request.  Per slot: x / xtip / err = the IK result, ok / t = checkMotion(states[N], x, last_valid),
// g / gtip = the interpolated state and its FK tip.
//   REACHED: the first slot in neighbour order with err < tolerance and ok -> (x, xtip, err, t = 1)
//   CLOSEST: otherwise the slot whose gtip is nearest the request, the first winning a tie -> (g, gtip, |gtip - request|, t)
//   NO_NEIGHBOR: the row is empty -> NaN outputs, vertex -1
__global__ __launch_bounds__(256) void tipq_select(const int32_t *__restrict__ nbr, const double *__restrict__ req, int64_t n, int k, int S,
                                                   double tolerance, const double *__restrict__ x, const double *__restrict__ xtip,
                                                   const double *__restrict__ err, const uint8_t *__restrict__ ok, const double *__restrict__ t,
                                                   const double *__restrict__ g, const double *__restrict__ gtip, double *__restrict__ controls,
                                                   double *__restrict__ tip_out, double *__restrict__ err_out, int32_t *__restrict__ nbr_out,
                                                   int32_t *__restrict__ outcome, double *__restrict__ t_out) {
#pragma clang fp contract(off)
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= n) return;
  const double rx = req[q * 3], ry = req[q * 3 + 1], rz = req[q * 3 + 2];
  int best = -1, what = TRK_TIPQ_NO_NEIGHBOR;
  double best_e = 1.0 / 0.0;
  for (int i = 0; i < k; i++) {
    const int64_t slot = q * k + i;
    if (nbr[slot] < 0) break;                                           // (rows are filled from the front)
    if (err[slot] < tolerance && ok[slot]) { best = i; what = TRK_TIPQ_REACHED; break; }
    const double dx = gtip[slot * 3] - rx, dy = gtip[slot * 3 + 1] - ry, dz = gtip[slot * 3 + 2] - rz;
    const double e = sqrt((dx * dx + dy * dy) + dz * dz);
    if (best < 0 || e < best_e) { best = i; best_e = e; what = TRK_TIPQ_CLOSEST; }
  }
  outcome[q] = what;
  if (best < 0) {
    const double nan_ = __longlong_as_double(0x7ff8000000000000LL);
    for (int d = 0; d < S; d++) controls[q * S + d] = nan_;
    for (int d = 0; d < 3; d++) tip_out[q * 3 + d] = nan_;
    err_out[q] = nan_; t_out[q] = nan_; nbr_out[q] = -1;
    return;
  }
  const int64_t slot = q * k + best;
  const bool reached = what == TRK_TIPQ_REACHED;
  const double *cs = reached ? x : g, *ct = reached ? xtip : gtip;
  for (int d = 0; d < S; d++) controls[q * S + d] = cs[slot * S + d];
  for (int d = 0; d < 3; d++) tip_out[q * 3 + d] = ct[slot * 3 + d];
  err_out[q] = reached ? err[slot] : best_e;
  t_out[q] = reached ? 1.0 : t[slot];
  nbr_out[q] = nbr[slot];
}

}  // namespace trk
