// The sizing arithmetic of the batched edge check (csrc/edge_plan.hpp) on its own: no device, no library.
//   (a) lane bounds are whole mask words, ascending, and cover [0, n_edges);
//   (b) the lane count steps at 2^16 and 2^19 edges, a call is split from 8 192 edges on, a fixed TENDON_HIP_EDGE_LANES is obeyed;
//   (c) a rotating robot's first call is not split;
//   (d) the shapes of test_two_lane_bisection_equals_one_lane with a 40 000-slot pool;
//   (e) chunks tile [0, n) in order and leave no remainder under a quarter chunk;
//   (f) known answers at 10 500 / 148 000 / 588 000 edges, worked by hand from the expressions (arithmetic in the comments).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "edge_plan.hpp"

namespace {

using namespace edge_plan;

int failures = 0;
#define CHECK(c)                                                            \
  do {                                                                      \
    if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } \
  } while (0)

constexpr int64_t kSlotsMax = (int64_t)1 << 24, kFbCap = (int64_t)1 << 17;     // tr_ctx's defaults

// an indexed call as ValidateIndexed::size_pool + plan_lanes form it: verdict-only schedule, pool sized by indexed_slots
LaneQuery query(int64_t n_edges, int64_t n_states, double rate_seen, int64_t fb_cap, int64_t ws_ld, int64_t slots_max = kSlotsMax) {
  LaneQuery q{};
  q.n_edges = n_edges; q.cap = indexed_slots(rate_seen, n_edges, n_states, slots_max); q.Vp = round_up(n_states, 64);
  q.ws_ld = ws_ld; q.fb_cap = fb_cap;
  q.edge_lanes = kMaxLanes; q.lanes_fixed = false;
  q.rate_seen = rate_seen; q.lane_guess = 6.0; q.guess_forced = false;
  q.slots_only = true; q.rotation = false;
  return q;
}

void lane_bounds() {
  for (int64_t n : {(int64_t)1, (int64_t)63, (int64_t)64, (int64_t)65, (int64_t)8192, (int64_t)10500, (int64_t)65536, (int64_t)148000, (int64_t)524288,
                    (int64_t)588000, (int64_t)3500001})
    for (int lanes = 1; lanes <= kMaxLanes; lanes++) {
      LaneQuery q = query(n, n / 6 + 1, 4.0, 64, 1 << 14);
      q.edge_lanes = lanes; q.lanes_fixed = true;
      const LanePlan p = plan_lanes(q);
      CHECK(p.NL == lanes);
      CHECK(p.eb[0] == 0 && p.eb[p.NL] == n);
      int64_t longest = 0;
      for (int l = 0; l < p.NL; l++) {
        CHECK(p.eb[l] % 64 == 0);
        CHECK(p.eb[l] <= p.eb[l + 1]);
        longest = std::max(longest, p.eb[l + 1] - p.eb[l]);
      }
      CHECK(p.Emax == longest);
      CHECK(p.R % 64 == 0 && p.lvl_share % 64 == 0);
      CHECK(q.Vp + p.NL * p.R <= q.cap);                    // the lanes' shares lie inside the pool, behind the vertices
      CHECK(p.NL * p.lvl_share <= q.cap);
    }
}

void lane_count_steps() {
  CHECK(lane_count(kMaxLanes, false, 8192) == 2 && lane_count(kMaxLanes, false, (1 << 16) - 1) == 2);
  CHECK(lane_count(kMaxLanes, false, 1 << 16) == 3 && lane_count(kMaxLanes, false, (1 << 19) - 1) == 3);
  CHECK(lane_count(kMaxLanes, false, 1 << 19) == 4 && lane_count(kMaxLanes, false, (int64_t)1 << 40) == 4);
  // TENDON_HIP_EDGE_LANES given: exactly that many, whatever the edge count
  for (int lanes = 1; lanes <= kMaxLanes; lanes++)
    for (int64_t n : {(int64_t)9000, (int64_t)1 << 16, (int64_t)1 << 19}) CHECK(lane_count(lanes, true, n) == lanes);
  CHECK(lane_count(0, true, 9000) == 1 && lane_count(9, true, 9000) == kMaxLanes);
  // a call is split from 8 192 edges on (a small fallback workspace, so that nothing else stands in the way)
  CHECK(!plan_lanes(query(8191, 1500, 0.0, 64, 1 << 14)).fits);
  CHECK(plan_lanes(query(8192, 1500, 0.0, 64, 1 << 14)).fits);
  LaneQuery one = query(10500, 1500, 0.0, 64, 1 << 14);
  one.edge_lanes = 1; one.lanes_fixed = true;
  CHECK(!plan_lanes(one).fits);
  LaneQuery stored = query(10500, 1500, 0.0, 64, 1 << 14);
  stored.slots_only = false;                                // stored points: never split
  CHECK(!plan_lanes(stored).fits);
}

void rotating_first_call() {
  LaneQuery q = query(10500, 1500, 0.0, 64, 1 << 14);
  q.rotation = true;
  CHECK(!plan_lanes(q).fits);                               // no rate seen yet: not split
  LaneQuery later = query(10500, 1500, 10.0, 64, 1 << 14);
  later.rotation = true;
  CHECK(plan_lanes(later).fits);                            // 26 x 10 687 -> cap = 277 888; 1.3 x 10 x 5 252 = 68 276 <= R = 276 352 / 2 = 138 176
}

// test_two_lane_bisection_equals_one_lane: 1 500 vertices, 10 500 edges, TENDON_HIP_FB_CAP=64, TENDON_HIP_EDGE_POOL=40000,
// TENDON_HIP_EDGE_LANE_GUESS=1, two and four lanes.
//   cap = min(40 000, 12 x 10 687) = 40 000; Vp = 1 536; two lanes: R = (38 464 / 2) & ~63 = 19 200, Emax = 5 252;
//   four lanes: R = (38 464 / 4) & ~63 = 9 600, Emax = 10 500 - 7 872 = 2 628.
// At the default guess of 6 samples per edge the halves do not fit their shares (31 512 > 19 200, 15 768 > 9 600): the call stays on
// one lane.  The forced guess of 1 is what lets the plan say "fits" (5 252 <= 19 200) for edges that take ~4 samples each, so that
// the lanes start, overflow their shares, and the call starts over on one lane -- the path that test is about.
void small_pool_of_the_two_lane_test() {
  for (int lanes : {2, 4}) {
    LaneQuery q = query(10500, 1500, 0.0, 64, 1 << 14, 40000);
    q.edge_lanes = lanes; q.lanes_fixed = true;
    CHECK(q.cap == 40000);
    const LanePlan honest = plan_lanes(q);
    CHECK(honest.R == (lanes == 2 ? 19200 : 9600) && honest.Emax == (lanes == 2 ? 5252 : 2628));
    CHECK(!honest.fits);
    q.lane_guess = 1.0; q.guess_forced = true;
    const LanePlan forced = plan_lanes(q);
    CHECK(forced.fits);
    CHECK(4 * forced.Emax > forced.R);                      // ... and ~4 own samples per edge then overflow the share
    q.rate_seen = 4.0;                                      // the forced guess also wins over a rate seen
    CHECK(plan_lanes(q).per_edge == 1.0);
  }
}

// for_edge_chunks' loop with FK counts of `nfk_each` per edge
void chunks_tile(int64_t n, int64_t avail, double guess, int ends, int nfk_each) {
  double rate = guess;
  int64_t e0 = 0, chunks = 0;
  while (e0 < n) {
    const int64_t e1 = chunk_end(e0, n, avail, rate), per = chunk_length(avail, rate);
    CHECK(e1 > e0 && e1 <= n && e1 - e0 <= std::max(per, (n - e0 + 1) / 2));
    if (e1 < n) CHECK(n - e1 >= per / 4);                   // no straggler under a quarter chunk is left over
    rate = chunk_rate((double)nfk_each, ends);
    CHECK(rate >= 2.0);
    e0 = e1;
    chunks++;
  }
  CHECK(e0 == n && chunks >= 1);
}

void chunks() {
  for (int64_t n : {(int64_t)1, (int64_t)2, (int64_t)700, (int64_t)10500, (int64_t)30000, (int64_t)148000, (int64_t)588001})
    for (int64_t avail : {(int64_t)1, (int64_t)960, (int64_t)4096, (int64_t)100032, (int64_t)1 << 22})
      for (int nfk_each : {2, 3, 8, 40}) {
        chunks_tile(n, avail, 9.0, 0, nfk_each);
        chunks_tile(n, avail, 6.0, 2, nfk_each);
      }
  // by hand: avail = 100 032, 6 samples per edge: per = floor(0.87 x 100 032 / 6) = floor(87 027.84 / 6) = floor(14 504.64) = 14 504
  CHECK(chunk_length(100032, 6.0) == 14504);
  CHECK(chunk_end(0, 30000, 100032, 6.0) == 14504);
  // from 14 504: 29 008 would leave 992 < 14 504 / 4 = 3 626 edges: the rest, 15 496, in halves: 14 504 + (15 496 + 1) / 2 = 22 252
  CHECK(chunk_end(14504, 30000, 100032, 6.0) == 22252);
  CHECK(chunk_end(22252, 30000, 100032, 6.0) == 30000);
  // the whole of config 3's smallest lane-sized roadmap is one chunk: avail = 128 256 - 1 536, per = floor(110 246.4 / 6) = 18 374 >= 10 500
  CHECK(chunk_length(126720, 6.0) == 18374 && chunk_end(0, 10500, 126720, 6.0) == 10500);
  // rate: 8 FK calls per edge, two of them the ends: 1.15 x 6 = 6.9; never under 2
  CHECK(std::fabs(chunk_rate(8.0, 2) - 6.9) < 1e-12 && chunk_rate(3.0, 2) == 2.0 && chunk_rate(2.0, 2) == 2.0);
}

void known_answers() {
  // ---- 10 500 edges on 1 500 vertices, a first call (no rate seen), TENDON_HIP_FB_CAP=64, two lanes (the new GPU test's shape) ----
  //   per_edge = max(12, 0) = 12; 12 x (10 500 + 1 500 / 8 = 10 687) = 128 244; vertex floor 2 x 1 536 + 4 096 = 7 168;
  //   cap = round_up(128 244, 64) = 2 004 x 64 = 128 256; Vp = 1 536
  //   R = ((128 256 - 1 536) / 2) & ~63 = 63 360 (= 990 x 64); eb = {0, 5 250 & ~63 = 5 248, 10 500}; Emax = 5 252
  //   lvl_share = (128 256 / 2) & ~63 = 64 128; per_edge (lanes) = the guess, 6: 6 x 5 252 = 31 512 <= 63 360: fits
  {
    LaneQuery q = query(10500, 1500, 0.0, 64, 1 << 14);
    q.edge_lanes = 2; q.lanes_fixed = true;
    CHECK(q.cap == 128256 && q.Vp == 1536);
    const LanePlan p = plan_lanes(q);
    CHECK(p.NL == 2 && p.R == 63360 && p.eb[0] == 0 && p.eb[1] == 5248 && p.eb[2] == 10500 && p.Emax == 5252 && p.lvl_share == 64128);
    CHECK(p.per_edge == 6.0 && p.fits);
    // with the default fallback workspace (2^17 columns a lane) this pool is too small for lanes: 128 256 < 2 x 2 x 131 072
    q.fb_cap = kFbCap; q.ws_ld = 4 * kFbCap;
    CHECK(!plan_lanes(q).fits);
    // pairwise form: max(12 x 10 500, 2^14) = 126 000 -> 1 969 x 64 = 126 016
    CHECK(pairwise_slots(10500, kSlotsMax) == 126016 && pairwise_slots(100, kSlotsMax) == 16384 && pairwise_slots(10500, 1024) == 1024);
    // tr_reserve_edges, 10 501 edges: 12 x 1.05 x 10 501 = 132 312.6 -> 132 312 -> 2 068 x 64 = 132 352
    CHECK(reserve_slots(0.0, 10501, kSlotsMax) == 132352);
    // the workspace as the pool: want = 126 000; from 16 384 columns straight to it, from 120 000 by an eighth (135 000), enough at 126 000
    CHECK(pool_growth(0.0, 10500, 16384, 1 << 22) == 126000 && pool_growth(0.0, 10500, 120000, 1 << 22) == 135000);
    CHECK(pool_growth(0.0, 10500, 126000, 1 << 22) == 0 && pool_growth(0.0, 10500, 120000, 130000) == 130000);
  }
  // ---- 148 000 edges on 25 000 vertices, 4 samples per edge seen, default fallback workspace (ws_ld = 4 x 2^17) ----
  //   per_edge = max(12, 10.4) = 12; 12 x (148 000 + 3 125) = 1 813 500 -> cap = 28 336 x 64 = 1 813 504; Vp = 391 x 64 = 25 024
  //   NL = 3 (2^16 <= 148 000 < 2^19); R = (1 788 480 / 3) & ~63 = 596 160 (= 9 315 x 64)
  //   eb = {0, 49 333 & ~63 = 49 280, 98 666 & ~63 = 98 624, 148 000}: lanes of 49 280, 49 344, 49 376 edges: Emax = 49 376
  //   lvl_share = 604 501 & ~63 = 604 480; per_edge (lanes) = max(1.5, 1.3 x 4) = 5.2: floor(5.2 x 49 376 = 256 755.2) <= R
  //   cap >= 2 x 3 x 131 072 = 786 432, ws_ld = 524 288 >= 3 x 131 072: fits
  {
    const LaneQuery q = query(148000, 25000, 4.0, kFbCap, 4 * kFbCap);
    CHECK(q.cap == 1813504 && q.Vp == 25024);
    const LanePlan p = plan_lanes(q);
    CHECK(p.NL == 3 && p.R == 596160 && p.eb[1] == 49280 && p.eb[2] == 98624 && p.eb[3] == 148000 && p.Emax == 49376 && p.lvl_share == 604480);
    CHECK(std::fabs(p.per_edge - 5.2) < 1e-12 && p.fits);
  }
  // ---- 588 000 edges on 100 000 vertices, 2.3 samples per edge seen ----
  //   per_edge = max(12, 5.98) = 12; 12 x (588 000 + 12 500) = 7 206 000 -> cap = 112 594 x 64 = 7 206 016; Vp = 1 563 x 64 = 100 032
  //   NL = 4; R = (7 105 984 / 4 = 1 776 496) & ~63 = 27 757 x 64 = 1 776 448
  //   eb = {0, 147 000 & ~63 = 146 944, 294 000 & ~63 = 293 952, 441 000 & ~63 = 440 960, 588 000}: the last lane is the longest, 147 040
  //   lvl_share = 1 801 504 & ~63 = 1 801 472; per_edge (lanes) = max(1.5, 2.99) = 2.99: floor(439 649.6) <= R
  //   cap >= 2 x 4 x 131 072, ws_ld = 524 288 >= 4 x 131 072 (with nothing to spare): fits; one column fewer and it does not
  {
    LaneQuery q = query(588000, 100000, 2.3, kFbCap, 4 * kFbCap);
    CHECK(q.cap == 7206016 && q.Vp == 100032);
    const LanePlan p = plan_lanes(q);
    CHECK(p.NL == 4 && p.R == 1776448 && p.eb[1] == 146944 && p.eb[2] == 293952 && p.eb[3] == 440960 && p.eb[4] == 588000 && p.Emax == 147040);
    CHECK(p.lvl_share == 1801472 && std::fabs(p.per_edge - 2.99) < 1e-12 && p.fits);
    q.ws_ld -= 1;
    CHECK(!plan_lanes(q).fits);
    // a rotating robot's rate, 10 samples per edge: the pool is sized at 26 per edge, 26 x 600 500 = 15 613 000 -> 243 954 x 64 = 15 613 056
    CHECK(indexed_slots(10.0, 588000, 100000, kSlotsMax) == 15613056);
    // ... and bounded by the largest pool: 2^24 slots from 1.4 M such edges on
    CHECK(indexed_slots(10.0, 1400000, 100000, kSlotsMax) == kSlotsMax);
    // a sparse roadmap: the vertex block's floor, 2 x 100 032 + 4 096 = 204 160 > 12 x (1 000 + 12 500)
    CHECK(indexed_slots(0.0, 1000, 100000, kSlotsMax) == 204160);
  }
}

}  // namespace

int main() {
  lane_bounds();
  lane_count_steps();
  rotating_first_call();
  small_pool_of_the_two_lane_test();
  chunks();
  known_answers();
  if (failures) { std::printf("%d checks failed\n", failures); return 1; }
  std::printf("edge plan ok\n");
  return 0;
}
