// edge_plan.hpp -- the sizing arithmetic of the batched edge check (edge_*_host.inc): how many pool slots a call asks for, how the
// workspace pool grows, how a call is split into lanes and whether the lanes fit, how the one-lane path cuts its chunks.  Plain
// integer and double arithmetic, no HIP: tests/cpp/edge_plan_test.cpp drives it with g++ alone.  Every factor and threshold here
// came out of a tuning round (CHANGELOG.md, profiles/r02 .. r05); the host code holds none of its own.
#pragma once
#include <algorithm>
#include <cstdint>

namespace edge_plan {

constexpr int kMaxLanes = 4;          // lanes of an edge bisection: streams, counters, fallback lists, ordering buffers (tr_ctx::lane)

inline int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

// samples per edge a pool is sized for: 12, or what two lanes need at the rate the context's last indexed call saw (a rotating
// robot: ~10 own samples per edge)
inline double pool_rate(double rate_seen) { return std::max(12.0, 2.6 * rate_seen); }

// ---- pool slots of one call through the verdict-only kernels (the pool is EdgeDev's per-sample arrays alone) ----
// pairwise form
inline int64_t pairwise_slots(int64_t n_edges, int64_t slots_max) {
  return round_up(std::min<int64_t>(slots_max, std::max<int64_t>(12 * n_edges, 1 << 14)), 64);
}
// indexed form: two lanes' worth at the rate last seen, and at least twice the vertex block (a sparse roadmap -- few edges per
// vertex -- must not leave the indexed form for want of slots)
inline int64_t indexed_slots(double rate_seen, int64_t n_edges, int64_t n_states, int64_t slots_max) {
  const double per_edge = pool_rate(rate_seen);
  const int64_t want = std::min<int64_t>(slots_max, std::max<int64_t>(std::max<int64_t>((int64_t)(per_edge * (double)(n_edges + n_states / 8)),
                                                                                         2 * round_up(n_states, 64) + 4096), 1 << 14));
  return round_up(std::max<int64_t>(want, 256), 64);
}
// what tr_reserve_edges sets aside for an indexed call of n_edges to come: 5 % over, the vertices not yet known
inline int64_t reserve_slots(double rate_seen, int64_t n_edges, int64_t slots_max) {
  const double per_edge = pool_rate(rate_seen);
  return round_up(std::min<int64_t>(slots_max, std::max<int64_t>((int64_t)(per_edge * 1.05 * (double)n_edges), 1 << 14)), 64);
}

// ---- the workspace as the pool (stored points): 0 when `ld` columns do, else the size to grow to ----
// by at least an eighth: a roadmap a few hundred edges larger than the last one must not reallocate the pool (and the scratch
// arrays sized after it) call after call -- tens of milliseconds each time
inline int64_t pool_growth(double rate_seen, int64_t n_edges, int64_t ld, int64_t pool_max) {
  const int64_t want = std::min<int64_t>(pool_max, std::max<int64_t>((int64_t)(pool_rate(rate_seen) * (double)n_edges), 1 << 14));
  if (ld >= want) return 0;
  return std::min<int64_t>(pool_max, std::max(want, ld + ld / 8));
}

// ---- lanes ----
struct LaneQuery {
  int64_t n_edges, cap, Vp;           // the call: edges, pool slots, slots of the vertex block (a multiple of 64)
  int64_t ws_ld, fb_cap;              // workspace columns, columns of one lane's fallback pass
  int edge_lanes; bool lanes_fixed;   // TENDON_HIP_EDGE_LANES: the upper bound, and whether it was given
  double rate_seen;                   // own samples per edge of the context's last indexed call (0: none yet)
  double lane_guess; bool guess_forced;   // TENDON_HIP_EDGE_LANE_GUESS
  bool slots_only, rotation;          // verdict-only schedule; the robot rotates
};
struct LanePlan {
  int NL;                             // lanes, if the call is split
  int64_t R;                          // pool slots of one lane: lane l owns [Vp + l R, Vp + (l + 1) R)
  int64_t eb[kMaxLanes + 1];          // lane l takes edges [eb[l], eb[l + 1]): whole mask words per lane
  int64_t Emax;                       // the longest lane
  int64_t lvl_share;                  // a lane's part of the per-level arrays (a level has at most R samples)
  double per_edge;                    // own samples per edge assumed
  bool fits;                          // split the call: every lane fits its share as one chunk
};

// four lanes from 2^19 edges, three from 2^16, else two (profiles/r03/edge_lanes_1to4_v1.txt: 588 k edges 34.5 / 32.0 / 30.8 / 30.2 ms on
// one .. four lanes, 148 k edges 16.0 / 14.3 / 14.1 / 14.5); TENDON_HIP_EDGE_LANES is the upper bound, and the count when given
inline int lane_count(int edge_lanes, bool lanes_fixed, int64_t n_edges) {
  return std::max(1, std::min(std::min(edge_lanes, kMaxLanes), lanes_fixed ? kMaxLanes : (n_edges >= (1 << 19) ? 4 : (n_edges >= (1 << 16) ? 3 : 2))));
}

inline LanePlan plan_lanes(const LaneQuery &q) {
  LanePlan p{};
  const int NL = p.NL = lane_count(q.edge_lanes, q.lanes_fixed, q.n_edges);
  p.R = ((q.cap - q.Vp) / NL) & ~(int64_t)63;
  for (int l = 0; l < NL; l++) p.eb[l] = (q.n_edges * l / NL) & ~(int64_t)63;
  p.eb[NL] = q.n_edges;
  for (int l = 0; l < NL; l++) p.Emax = std::max(p.Emax, p.eb[l + 1] - p.eb[l]);
  p.lvl_share = (q.cap / NL) & ~(int64_t)63;
  // own samples per edge: what this context's last indexed call needed with 30 % to spare (a dense roadmap's short edges take ~2,
  // config 3's ~4, a rotating robot's ~10), or the guess on a first call.  (Round 2 took the larger of the two, which kept config 4's
  // 3.5 M short edges -- 2.3 samples each -- from ever fitting their lanes.)  An explicit TENDON_HIP_EDGE_LANE_GUESS always wins (tests).
  p.per_edge = (q.rate_seen > 0.0 && !q.guess_forced) ? std::max(1.5, 1.3 * q.rate_seen) : q.lane_guess;
  // (a rotating robot's first call is not split: its edges need two to three times the samples of a tension-only robot's, and a
  // lane that overflows costs the whole attempt)
  p.fits = NL >= 2 && q.slots_only && (q.rate_seen > 0.0 || !q.rotation) && q.n_edges >= 8192 &&
           q.cap >= 2 * NL * q.fb_cap && q.ws_ld >= NL * q.fb_cap && (int64_t)(p.per_edge * (double)p.Emax) <= p.R &&
           q.n_edges <= q.cap / 2;
  return p;
}

// ---- chunks of the one-lane path ----
// `avail` pool samples for a chunk's own samples at `rate` samples per edge, 13 % to spare
inline int64_t chunk_length(int64_t avail, double rate) { return std::max<int64_t>(1, (int64_t)(0.87 * (double)avail / rate)); }
// the end of the chunk that starts at e0.  A remainder smaller than a quarter chunk is not left over as a launch-latency-bound
// straggler: the rest is split in two halves instead.
inline int64_t chunk_end(int64_t e0, int64_t n_edges, int64_t avail, double rate) {
  const int64_t per = chunk_length(avail, rate);
  int64_t e1 = std::min(n_edges, e0 + per);
  if (e1 < n_edges && n_edges - e1 < per / 4) e1 = e0 + (n_edges - e0 + 1) / 2;
  return e1;
}
// the next chunk's rate: what the last one needed (its mean FK count per edge, minus `ends` samples that do not live in the
// chunk's part of the pool) with 15 % to spare
inline double chunk_rate(double mean_nfk, int ends) { return std::max(2.0, 1.15 * (mean_nfk - ends)); }

}  // namespace edge_plan
