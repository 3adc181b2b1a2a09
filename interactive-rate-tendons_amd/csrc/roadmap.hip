// roadmap.hip -- tr_roadmap_*: the interactive query loop of motion_planning::VoxelCachedLazyPRM on a cached
// roadmap (BASELINE config 5): solveWithRoadmap / constructSolution
// (motion-planning/VoxelCachedLazyPRM.cpp:1977-2096, :2689-2771), astarSearch (:2950-2976),
// computeVertexValidity / computeEdgeValidity on cached voxel sets (:2607-2631), clearValidity (:1656-1663).
//
// The reference answers one (start, goal) pair at a time: A* over the Boost graph, then every interior vertex of the
// candidate path is tested (cached voxel set AND obstacle octree), ALL invalid ones are removed, else the path's edges are
// tested from the goal side and the FIRST invalid one is removed; repeat until a path survives or start and goal fall
// into different components.  Each test is a tiny octree intersection -- latency-bound on the CPU and far too small for a
// GPU launch of its own.  Here a whole batch of queries advances in rounds:
//   round = [A* for every unresolved query on the graph minus what is known invalid: large rounds on the device, one wave per
//            query (search_kernel.hpp: roadmap_astar), shared with the host threads; small rounds on the host threads alone]
//           -> the union of the still-unknown vertices and edges on all candidate paths -> ONE K4 launch on that subset
//              (cached_subset_vs_grid; the caches live in HBM as one CSR) -> validity recorded, invalid items leave the graph
//   queries whose candidate path turned out all valid are done; the others search again next round.
//   Two shortcuts that change no answer (round 4): queries whose end points lie in different components of what is left of the
//   graph are answered from component labels computed on the device (component_labels; the reference's solutionComponent test),
//   and when queries are still open while ONE launch over every cached set is cheaper than another round of searches, everything
//   is tested and the next round is the last (the loop turns eager; TENDON_HIP_LAZY_ONLY=1 forbids it).
// tr_roadmap_revalidate is the eager form: one K4 pass over every cached set (well under a millisecond for 10^5..10^6
// items), after which every query resolves in its first round.
// Returned paths are the reference's: a path is accepted only when all its items are valid, and it is the shortest path
// of the graph minus the invalid items discovered so far -- which, all of its own items being valid, is also the
// shortest path of the graph minus ALL invalid items, whatever subset has been discovered (equal costs; equal vertex
// sequences unless two paths tie exactly).  What differs is bookkeeping only: every unknown edge of a vertex-clean path
// is tested in the round (the reference stops at the first invalid one), so the set of DISCOVERED invalid edges is a superset.
// A search is latency-bound pointer chasing: one search is ~8x faster on a host core than on a wave, but the device runs three
// thousand of them at once -- hence the shared schedule.  The heuristic is the reference's state-space distance, sharpened by landmark
// lower bounds (tr_roadmap_prepare): distances from a few extremal vertices over the FULL graph; |d(l, v) - d(l, goal)| never
// exceeds the distance from v to the goal, and stays a lower bound when invalid items leave the graph (distances only
// grow).  The path A* returns is still the shortest one -- an admissible heuristic only changes how few vertices are expanded.
// Queries between arbitrary STATES (tr_roadmap_attach_states / _solve_seeded / _solve_states; roadmap_attach_host.inc) run the same rounds
// with astar_seeded as the search -- on the host threads at every batch size: those calls never launch roadmap_astar.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/tendon_hip.h"
#include "roadmap_kernel.hpp"
#include "tipq_kernel.hpp"
#include "stateq_kernel.hpp"
#include "tipq_loaded_kernel.hpp"
#include "attach_kernel.hpp"
#include "handback_feed.hpp"

namespace {

// The environment switches of this unit (the table in include/tendon_hip.h, "read per call"): parsed and clamped HERE and nowhere else.
// Every tr_roadmap_* entry point that needs them reads them once and hands them down -- tests and benchmarks flip them between two
// calls of one process, so none is kept from call to call.
struct RoadmapSwitches {
  int search_mode = 1;                 // TENDON_HIP_SEARCH: 0 = the host threads, 1 = the device for rounds of at least kSearchMinQueries queries, 2 = the device always (tests)
  int components_mode = 1;             // TENDON_HIP_COMPONENTS: 0: never; 1: when they have paid before on this roadmap (a search walked kComponentTrigger vertices and
                                       // found no path) or the kernel hands searches back (unset); 2: every round of kComponentMinQueries or more
  bool lazy_only = false;              // TENDON_HIP_LAZY_ONLY
  bool host_share_set = false;         // TENDON_HIP_SEARCH_HOST_SHARE (per cent): the share of a round's searches (the ones expected to be longest) that the
  double host_share = 0.01;            // host threads take while the kernel runs
  bool budget_set = false;             // TENDON_HIP_SEARCH_BUDGET: the kernel's pop budget per search (0: none)
  int64_t budget = 6500;
  int kbest = trk::SR_K;               // TENDON_HIP_SEARCH_K: vertices a step of the kernel takes off a search's open list (1: the host's order of expansions exactly)
  int64_t sweep_cap = -1;              // TENDON_HIP_SEARCH_SWEEP (< 0: not set)
  int64_t slots = 0;                   // TENDON_HIP_SEARCH_SLOTS (0: not set; as given -- search_setup bounds it by what the device holds)
  int lc0 = 12;                        // TENDON_HIP_SEARCH_LC0
  bool pool_set = false;               // TENDON_HIP_SEARCH_POOL=a,b,c
  long long pool[3] = {0, 0, 0};
  bool landmarks_host = false, landmarks_check = false;   // TENDON_HIP_LANDMARKS=host | check
  bool stats = false;                  // TENDON_HIP_SEARCH_STATS
  bool hist = false;                   // TENDON_HIP_SEARCH_HIST; with a path (a value that starts with '/'): one line per search appended to that file
  const char *hist_path = nullptr;
  bool timing = false;                 // TENDON_HIP_ROADMAP_TIMING
};

RoadmapSwitches read_switches() {
  RoadmapSwitches s;
  if (const char *e = std::getenv("TENDON_HIP_SEARCH")) {
    if (std::strcmp(e, "host") == 0 || std::strcmp(e, "0") == 0) s.search_mode = 0;
    else if (std::strcmp(e, "device") == 0 || std::strcmp(e, "force") == 0) s.search_mode = 2;
  }
  if (const char *e = std::getenv("TENDON_HIP_COMPONENTS")) s.components_mode = (std::strcmp(e, "0") == 0 || std::strcmp(e, "off") == 0) ? 0 : 2;
  s.lazy_only = std::getenv("TENDON_HIP_LAZY_ONLY") != nullptr;
  if (const char *e = std::getenv("TENDON_HIP_SEARCH_HOST_SHARE")) { s.host_share_set = true; s.host_share = std::min(100.0, std::max(0.0, std::atof(e))) / 100.0; }
  if (const char *e = std::getenv("TENDON_HIP_SEARCH_BUDGET")) { s.budget_set = true; const long long b = std::atoll(e); s.budget = b > 0 ? (int64_t)b : 0; }
  if (const char *e = std::getenv("TENDON_HIP_SEARCH_K")) s.kbest = std::max(1, std::min(std::atoi(e), (int)trk::SR_K));
  if (const char *e = std::getenv("TENDON_HIP_SEARCH_SWEEP")) s.sweep_cap = std::max<long long>(0, std::atoll(e));
  if (const char *e = std::getenv("TENDON_HIP_SEARCH_SLOTS")) s.slots = std::max<long long>(1, std::atoll(e));
  if (const char *e = std::getenv("TENDON_HIP_SEARCH_LC0")) s.lc0 = std::max(8, std::min(14, std::atoi(e)));
  if (const char *e = std::getenv("TENDON_HIP_SEARCH_POOL")) s.pool_set = std::sscanf(e, "%lld,%lld,%lld", &s.pool[0], &s.pool[1], &s.pool[2]) >= 1;
  if (const char *e = std::getenv("TENDON_HIP_LANDMARKS")) { s.landmarks_host = std::strcmp(e, "host") == 0; s.landmarks_check = std::strcmp(e, "check") == 0; }
  s.stats = std::getenv("TENDON_HIP_SEARCH_STATS") != nullptr;
  if (const char *e = std::getenv("TENDON_HIP_SEARCH_HIST")) { s.hist = true; if (e[0] == '/') s.hist_path = e; }
  s.timing = std::getenv("TENDON_HIP_ROADMAP_TIMING") != nullptr;
  return s;
}

}  // namespace

#include "roadmap_infra_host.inc"

struct tr_roadmap {
  std::mutex mu;
  std::atomic<bool> busy{false};       // a call holds `mu` (RmLock): the out-of-memory trim leaves this roadmap alone
  tr_ctx *ctx = nullptr;
  std::string err;
  int S = 0, NT = 0;
  bool rot = false, ret = false;
  double w_rot = 0, w_ret = 0;
  int64_t V = 0, E = 0;
  std::vector<double> states;
  RawArray<int32_t> eu, ev;
  RawArray<double> w;
  std::vector<int64_t> adj_off;        // CSR adjacency, both directions
  RawArray<Arc> adj;
  // landmark lower bounds (tr_roadmap_prepare): lm_d[v * lm_n + l] = graph distance landmark l -> v over all edges, as float; SR_LM_FAR
  // (not +inf) where v is not connected to l: what the branch-free bounds of the host A* and of the kernel's rows read
  // (+inf = not connected); lm_n = 0: none, -1: not built yet (built with the default count by the first solve)
  int lm_n = -1;
  std::vector<float> lm_d;
  std::vector<int32_t> lm_v;
  bool lm_mismatch = false;            // TENDON_HIP_LANDMARKS=check: the device's table differed from the host's
  std::vector<uint8_t> vstat, estat;   // V_*
  std::vector<uint8_t> vpresent, epresent;
  // cached voxel sets in HBM: one CSR, items [0, V) = vertices, [V, V + E) = edges
  bool has_caches = false;
  uint32_t *d_ids = nullptr; uint64_t *d_masks = nullptr; int64_t *d_off = nullptr;
  int32_t *d_list = nullptr; uint8_t *d_hit = nullptr; uint64_t *d_bits = nullptr;
  uint64_t *h_bits = nullptr;          // pinned image of d_bits (tr_roadmap_revalidate)
  std::vector<uint64_t> absent;        // per word of the combined item index: bit set = the item has no cache (invalid for good)
  int64_t list_cap = 0;
  int64_t nnz = 0;
  // results of the last tr_roadmap_solve
  std::vector<int64_t> path_off;
  std::vector<int32_t> path_v;
  std::vector<std::vector<int32_t>> paths_buf, paths_e_buf;   // per query of the last solve: vertices goal ... start, their edges (capacity kept)
  // statistics of the last solve
  int64_t st_rounds = 0, st_items_checked = 0, st_astar_runs = 0, st_expanded = 0;
  std::vector<Scratch> scratch;
  // the graph searches on the device (search_kernel.hpp): everything below lives in HBM for the life of the roadmap
  struct DevSearch {
    int state = 0;                       // 0: not set up yet, 1: ready, -1: not available for this roadmap (reason in `why`)
    std::string why;
    int64_t slots = 0, nq_cap = 0;
    int64_t max_slots = 0;               // what the device holds at once (or TENDON_HIP_SEARCH_SLOTS); `slots` follows the rounds' sizes up to it
    int32_t lc0 = 12;                    // log2 of the records of a slot's own table
    int32_t pool_n[trk::SR_CLASSES] = {0, 0, 0, 0}, pool_word[trk::SR_CLASSES] = {0, 0, 0, 0};
    size_t ctl_bytes = 0, table_bytes = 0;
    uint32_t pbuf_cap = 0;
    uint64_t gens_issued = 0;
    bool lm_current = false;
    char *arena = nullptr;               // adjacency rows | states | landmark table | validity bytes | control words + pool bitmaps
    char *tables = nullptr;              // the slots' tables, then the pool's, class by class
    char *pool[trk::SR_CLASSES] = {nullptr, nullptr, nullptr, nullptr};
    char *qarena = nullptr;              // per-round arrays (queries, results, packed paths)
    trk::SArc *d_rows = nullptr; char *d_vrows = nullptr;        // adjacency rows; per vertex: state | landmark distances
    int32_t row_bytes = 0;
    uint8_t *d_vstat = nullptr, *d_estat = nullptr, *d_deg = nullptr;
    uint32_t *d_ctl = nullptr;
    int32_t *d_qs = nullptr, *d_qg = nullptr, *d_poff = nullptr, *d_plen = nullptr, *d_pbuf = nullptr;
    uint8_t *d_found = nullptr;
    uint32_t *h_handback = nullptr, *d_handback = nullptr;   // pinned: the kernel marks a search here the moment it hands it back
    int64_t handback_cap = 0;
    double kernel_ms = 0, host_after_ms = 0;                   // of the last shared round: the kernel's span, the host threads' work after it
    hipEvent_t ev[2] = {nullptr, nullptr};                     // around every roadmap_astar launch (tr_roadmap_profile)
    bool ev_pending = false;
    double st_kernel_ms = 0; int64_t st_launches = 0;          // of the last tr_roadmap_solve
    int64_t st_queries = 0, st_fallbacks = 0, st_host_share = 0, st_moves = 0, st_expanded = 0, st_grows = 0, st_max_records = 0;   // of the last tr_roadmap_solve
    int64_t in_flight = 0;               // queries of the launch that has not been collected yet
    bool budget_from_env = false;
    double share = -1.0;                 // the host threads' share of a shared round (< 0: not chosen yet); follows the two sides' times
    int64_t budget = 0;                  // expansions per search before the kernel hands it back (0: not chosen yet); doubles when
                                         // more than a twentieth of a round came back -- a larger roadmap has longer searches
    // sweep_search: a single-source sweep over the valid arcs for the few searches that expand a large part of the graph
    std::mutex sweep_mu;
    hipStream_t sweep_stream = nullptr;
    char *sweep_arena = nullptr;         // distances (ordered bit patterns) | validity bytes of this round | flags
    unsigned long long *sweep_h_dist = nullptr;   // pinned: the distances come back here
    int64_t sweep_round = -1;            // the round whose validity bytes the arena holds
    int64_t st_sweeps = 0;               // searches answered this way in the last tr_roadmap_solve
    std::vector<int32_t> h_qs, h_qg;     // host images of what the pending copies read
    std::vector<char> h_vrows;
  } ds;
  // connected components of the roadmap minus what is known invalid (component_labels): the edge list and the labels in HBM
  struct DevComp {
    int state = 0;                       // 0: not set up yet, 1: ready, -1: not available
    char *arena = nullptr;
    int32_t *d_eu = nullptr, *d_ev = nullptr, *d_parent = nullptr, *d_label = nullptr;
    uint8_t *d_vstat = nullptr, *d_estat = nullptr;
    bool status_current = false;         // d_vstat / d_estat hold this round's validity bytes (the search kernel reads them too)
    bool wanted = false;                 // a search on this roadmap has walked a component in vain: label every large round from now on
    std::vector<int32_t> label;          // per vertex: the smallest vertex of its component
    int64_t st_cut = 0;                  // searches of the last solve answered by the labels alone
  } dc;
  // tip-goal queries (tr_roadmap_set_tips .. tr_roadmap_solve_tips; roadmap_tips_host.inc): the tips, a copy of the states and the
  // validity bytes in HBM for the life of the roadmap, and one grow-only arena for the arrays of a call
  struct DevTips {
    bool set = false;
    bool own_tips = false;               // the tips are tr_fk_tips_dev's of the states (unloaded): the loaded tip queries refuse them
    double *d_tips = nullptr, *d_states = nullptr;
    double *d_soa = nullptr;             // the states coordinate by coordinate ([S][V]): what state_knn streams
    uint8_t *d_vstat = nullptr;          // the image of `vstat` the kernel filters by; sent again only when `vstat` differs from `vstat_sent`
    uint64_t *d_present = nullptr;       // bit v: vertex v has a tip
    std::vector<uint8_t> vstat_sent;
    std::vector<uint64_t> present;
    char *arena = nullptr;
    size_t arena_bytes = 0;
    double phase_ms[5] = {0, 0, 0, 0, 0};   // of the last call: nearest, IK, edges, select, solve
    int64_t st_ik_rounds = 0;
    int64_t connect_stats[4] = {0, 0, 0, 0};   // of the last *_connect call (tr_roadmap_tip_connect_stats)
    // the attach phase (roadmap_attach_host.inc): the roadmap's rows with room for ext_cap query rows behind them, what the index pairs refer to
    double *d_ext = nullptr;
    int64_t ext_cap = 0;
    double state_phase_ms[4] = {0, 0, 0, 0};   // of the last tr_roadmap_solve_states: nearest + validity, edges, seeded search, results
  } dt;
};

namespace {

// Every entry point that works on a roadmap holds its mutex through this; `busy` lets the trim path (which may run on the very
// thread that holds the mutex: an allocation inside a call ran out of memory) tell without touching the mutex.
struct RmLock {
  tr_roadmap *r;
  explicit RmLock(tr_roadmap *r_) : r(r_) { r->mu.lock(); r->busy.store(true, std::memory_order_release); }
  ~RmLock() { r->busy.store(false, std::memory_order_release); r->mu.unlock(); }
  RmLock(const RmLock &) = delete;
  RmLock &operator=(const RmLock &) = delete;
};
// the live roadmaps (tr_roadmap_create .. tr_roadmap_destroy), for release_idle_search_tables
std::mutex g_roadmaps_mu;
std::vector<tr_roadmap *> g_roadmaps;

int rfail(tr_roadmap *r, int code, const std::string &m) { if (r) r->err = m; return code; }

#define RM_HIP(r, expr)                                                                      \
  do {                                                                                       \
    hipError_t e_ = (expr);                                                                  \
    if (e_ != hipSuccess) return rfail(r, TR_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)


// the cached voxel sets in HBM go (tr_roadmap_set_caches attaches new ones; tr_roadmap_destroy)
void free_dev(tr_roadmap *r) {
  void *p[] = {r->d_ids, r->d_masks, r->d_off, r->d_list, r->d_hit, r->d_bits};
  for (void *q : p) if (q) dev_cache().release(q);
  r->d_ids = nullptr; r->d_masks = nullptr; r->d_off = nullptr; r->d_list = nullptr; r->d_hit = nullptr; r->d_bits = nullptr;
  if (r->h_bits) { (void)hipHostFree(r->h_bits); r->h_bits = nullptr; }
  r->list_cap = 0; r->has_caches = false;
}

}  // namespace

#include "roadmap_astar_host.inc"
#include "roadmap_components_host.inc"
#include "roadmap_search_host.inc"
#include "roadmap_solve_host.inc"
#include "roadmap_tips_host.inc"
#include "roadmap_attach_host.inc"

extern "C" {

const char *tr_roadmap_last_error(const tr_roadmap *r) { return r ? r->err.c_str() : "null roadmap"; }

int tr_roadmap_create(tr_ctx *ctx, const double *states, int64_t n_vertices, const int32_t *edges, const double *weights,
                      int64_t n_edges, tr_roadmap **out) {
  if (!ctx || !out || n_vertices < 0 || n_edges < 0 || (n_vertices > 0 && !states) || (n_edges > 0 && !edges)) return TR_ERR_INVALID_ARG;
  *out = nullptr;
  if (n_vertices > std::numeric_limits<int32_t>::max() / 2 || n_edges > std::numeric_limits<int32_t>::max() / 2) return TR_ERR_INVALID_ARG;
  tr_roadmap *r = new tr_roadmap();
  r->ctx = ctx;
  r->S = tr_state_size(ctx);
  r->V = n_vertices; r->E = n_edges;
  tr_space_weights(ctx, &r->w_rot, &r->w_ret);
  {
    int rot = 0, ret = 0, nt = 0;
    tr_state_layout(ctx, &nt, &rot, &ret);
    r->NT = nt; r->rot = rot != 0; r->ret = ret != 0;
  }
  const RoadmapSwitches sw = read_switches();
  Laps laps(sw, "tr_roadmap_create");
  r->states.assign(states, states + (size_t)n_vertices * r->S);
  r->eu.resize_uninit((size_t)n_edges); r->ev.resize_uninit((size_t)n_edges); r->w.resize_uninit((size_t)n_edges);
  // One team of T threads, three phases with a barrier between them (a team per phase cost ~1 ms each in thread starts):
  //   1. the edge arrays by edge ranges (end points, weights);  2. degrees by edge ranges (atomic increments), then thread 0 turns
  //   them into offsets and sizes the arc array;  3. the arcs by VERTEX ranges: every thread scans all edges in order and takes the
  //   arcs that leave its vertices, so a vertex's arcs keep the edge order whatever T is (atomic cursors + a per-vertex sort were
  //   slower: 5.6 against 3.0 ms, scattered first touches of the 19 MB).
  const int T = n_edges >= (1 << 16) ? std::min(host_threads(0), 16) : 1;
  std::atomic<int> bad{TR_OK};
  r->adj_off.assign((size_t)n_vertices + 1, 0);
  struct Barrier {
    const int n; std::atomic<int> arrived{0}, phase{0};
    explicit Barrier(int n_) : n(n_) {}
    void wait() {
      const int ph = phase.load(std::memory_order_acquire);
      if (arrived.fetch_add(1, std::memory_order_acq_rel) + 1 == n) { arrived.store(0, std::memory_order_relaxed); phase.store(ph + 1, std::memory_order_release); }
      else while (phase.load(std::memory_order_acquire) == ph) std::this_thread::yield();
    }
  } barrier(T);
  on_threads(T, [&](int t) {
    const int64_t lo = n_edges * t / T, hi = n_edges * (t + 1) / T;
    for (int64_t e = lo; e < hi; e++) {
      const int32_t a = edges[2 * e], b = edges[2 * e + 1];
      if (a < 0 || a >= n_vertices || b < 0 || b >= n_vertices) { bad = TR_ERR_OUT_OF_RANGE; break; }
      r->eu[(size_t)e] = a; r->ev[(size_t)e] = b;
      // edge cost = opt_->motionCost = si->distance(a, b) unless the file supplies one (weightProperty_, :2598-2603)
      r->w[(size_t)e] = weights ? weights[e] : state_distance(r, &r->states[(size_t)a * r->S], &r->states[(size_t)b * r->S]);
      if (!(r->w[(size_t)e] >= 0)) { int want = TR_OK; bad.compare_exchange_strong(want, TR_ERR_INVALID_ARG); break; }
    }
    barrier.wait();
    if (bad != TR_OK) return;                                   // (every thread sees the same value after the barrier)
    for (int64_t e = lo; e < hi; e++) {
      __atomic_fetch_add(&r->adj_off[(size_t)r->eu[(size_t)e] + 1], (int64_t)1, __ATOMIC_RELAXED);
      __atomic_fetch_add(&r->adj_off[(size_t)r->ev[(size_t)e] + 1], (int64_t)1, __ATOMIC_RELAXED);
    }
    barrier.wait();
    if (t == 0) {
      for (int64_t v = 0; v < n_vertices; v++) r->adj_off[(size_t)v + 1] += r->adj_off[(size_t)v];
      r->adj.resize_uninit((size_t)r->adj_off[(size_t)n_vertices]);
    }
    barrier.wait();
    const int32_t vlo = (int32_t)(n_vertices * t / T), vhi = (int32_t)(n_vertices * (t + 1) / T);
    if (vlo == vhi) return;
    std::vector<int64_t> fill(r->adj_off.begin() + vlo, r->adj_off.begin() + vhi);
    for (int64_t e = 0; e < n_edges; e++) {
      const int32_t a = r->eu[(size_t)e], b = r->ev[(size_t)e];
      if (a >= vlo && a < vhi) r->adj[(size_t)fill[(size_t)(a - vlo)]++] = Arc{b, (int32_t)e, r->w[(size_t)e]};
      if (b >= vlo && b < vhi) r->adj[(size_t)fill[(size_t)(b - vlo)]++] = Arc{a, (int32_t)e, r->w[(size_t)e]};
    }
  });
  if (bad != TR_OK) { const int rc = bad; delete r; return rc; }
  laps.lap("edges + degrees + adjacency");
  r->vstat.assign((size_t)n_vertices, V_UNKNOWN); r->estat.assign((size_t)n_edges, V_UNKNOWN);
  r->vpresent.assign((size_t)n_vertices, 1); r->epresent.assign((size_t)n_edges, 1);
  { std::lock_guard<std::mutex> g(g_roadmaps_mu); g_roadmaps.push_back(r); }
  *out = r;
  return TR_OK;
}

void tr_roadmap_destroy(tr_roadmap *r) {
  if (!r) return;
  { std::lock_guard<std::mutex> g(g_roadmaps_mu); g_roadmaps.erase(std::remove(g_roadmaps.begin(), g_roadmaps.end(), r), g_roadmaps.end()); }
  (void)hipSetDevice(tr_device(r->ctx));
  free_dev(r);
  free_search(r);
  free_comp(r);
  free_tips(r);
  delete r;
}

}  // extern "C"
namespace {
int set_caches_impl(tr_roadmap *r, const int64_t *v_offsets, const uint32_t *v_ids, const uint64_t *v_masks,
                    const uint64_t *v_present_bits, const int64_t *e_offsets, const uint32_t *e_ids,
                    const uint64_t *e_masks, const uint64_t *e_present_bits, hipMemcpyKind kind) {
  if (!r) return TR_ERR_INVALID_ARG;
  RmLock lock_(r);
  if (!v_offsets || !e_offsets) return rfail(r, TR_ERR_INVALID_ARG, "null offsets");
  const int64_t nv = v_offsets[r->V], ne = e_offsets[r->E];
  if (nv < 0 || ne < 0 || (nv > 0 && (!v_ids || !v_masks)) || (ne > 0 && (!e_ids || !e_masks))) return rfail(r, TR_ERR_INVALID_ARG, "bad CSR arrays");
  for (int64_t i = 0; i < r->V; i++) if (v_offsets[i] > v_offsets[i + 1]) return rfail(r, TR_ERR_INVALID_ARG, "offsets must be non-decreasing");
  for (int64_t i = 0; i < r->E; i++) if (e_offsets[i] > e_offsets[i + 1]) return rfail(r, TR_ERR_INVALID_ARG, "offsets must be non-decreasing");
  RM_HIP(r, hipSetDevice(tr_device(r->ctx)));
  free_dev(r);
  const int64_t items = r->V + r->E;
  r->nnz = nv + ne;
  std::vector<int64_t> off((size_t)items + 1);
  for (int64_t i = 0; i <= r->V; i++) off[(size_t)i] = v_offsets[i];
  for (int64_t i = 0; i <= r->E; i++) off[(size_t)(r->V + i)] = nv + e_offsets[i];
  const int dev = tr_device(r->ctx);
  RM_HIP(r, dev_cache().alloc(dev, (void **)&r->d_ids, std::max<size_t>(1, (size_t)r->nnz) * sizeof(uint32_t)));
  RM_HIP(r, dev_cache().alloc(dev, (void **)&r->d_masks, std::max<size_t>(1, (size_t)r->nnz) * sizeof(uint64_t)));
  RM_HIP(r, dev_cache().alloc(dev, (void **)&r->d_off, off.size() * sizeof(int64_t)));
  RM_HIP(r, dev_cache().alloc(dev, (void **)&r->d_bits, ((size_t)items / 64 + 1) * sizeof(uint64_t)));
  if (nv) {
    RM_HIP(r, hipMemcpy(r->d_ids, v_ids, (size_t)nv * sizeof(uint32_t), kind));
    RM_HIP(r, hipMemcpy(r->d_masks, v_masks, (size_t)nv * sizeof(uint64_t), kind));
  }
  if (ne) {
    RM_HIP(r, hipMemcpy(r->d_ids + nv, e_ids, (size_t)ne * sizeof(uint32_t), kind));
    RM_HIP(r, hipMemcpy(r->d_masks + nv, e_masks, (size_t)ne * sizeof(uint64_t), kind));
  }
  RM_HIP(r, hipMemcpy(r->d_off, off.data(), off.size() * sizeof(int64_t), hipMemcpyHostToDevice));
  for (int64_t i = 0; i < r->V; i++) r->vpresent[(size_t)i] = v_present_bits ? (uint8_t)((v_present_bits[i >> 6] >> (i & 63)) & 1) : 1;
  for (int64_t i = 0; i < r->E; i++) r->epresent[(size_t)i] = e_present_bits ? (uint8_t)((e_present_bits[i >> 6] >> (i & 63)) & 1) : 1;
  // what tr_roadmap_revalidate needs on the host: a pinned image of the hit words and, per word, the items without a cache
  RM_HIP(r, hipHostMalloc((void **)&r->h_bits, ((size_t)items / 64 + 1) * sizeof(uint64_t), hipHostMallocDefault));
  r->absent.assign((size_t)items / 64 + 1, 0);
  for (int64_t i = 0; i < r->V; i++) if (!r->vpresent[(size_t)i]) r->absent[(size_t)i >> 6] |= (uint64_t)1 << (i & 63);
  for (int64_t i = 0; i < r->E; i++) if (!r->epresent[(size_t)i]) { const int64_t q = r->V + i; r->absent[(size_t)q >> 6] |= (uint64_t)1 << (q & 63); }
  r->has_caches = true;
  return TR_OK;
}
}  // namespace
extern "C" {

int tr_roadmap_set_caches(tr_roadmap *r, const int64_t *v_offsets, const uint32_t *v_ids, const uint64_t *v_masks,
                          const uint64_t *v_present_bits, const int64_t *e_offsets, const uint32_t *e_ids,
                          const uint64_t *e_masks, const uint64_t *e_present_bits) {
  return set_caches_impl(r, v_offsets, v_ids, v_masks, v_present_bits, e_offsets, e_ids, e_masks, e_present_bits, hipMemcpyHostToDevice);
}

int tr_roadmap_set_caches_dev(tr_roadmap *r, const int64_t *v_offsets, const uint32_t *d_v_ids, const uint64_t *d_v_masks,
                              const uint64_t *v_present_bits, const int64_t *e_offsets, const uint32_t *d_e_ids,
                              const uint64_t *d_e_masks, const uint64_t *e_present_bits) {
  return set_caches_impl(r, v_offsets, d_v_ids, d_v_masks, v_present_bits, e_offsets, d_e_ids, d_e_masks, e_present_bits, hipMemcpyDeviceToDevice);
}

int tr_roadmap_prepare(tr_roadmap *r, int32_t n_landmarks, int32_t n_threads) {
  if (!r) return TR_ERR_INVALID_ARG;
  RmLock lock_(r);
  if (n_landmarks < 0 || n_landmarks > 64) return rfail(r, TR_ERR_INVALID_ARG, "landmark count must be in [0, 64]");
  build_landmarks(r, n_landmarks, host_threads(n_threads), read_switches());
  if (r->lm_mismatch) return rfail(r, TR_ERR_RUNTIME, "landmark distances: the device's table differs from the host's (TENDON_HIP_LANDMARKS=check)");
  return TR_OK;
}

int tr_roadmap_clear_validity(tr_roadmap *r) {
  if (!r) return TR_ERR_INVALID_ARG;
  RmLock lock_(r);
  std::fill(r->vstat.begin(), r->vstat.end(), (uint8_t)V_UNKNOWN);
  std::fill(r->estat.begin(), r->estat.end(), (uint8_t)V_UNKNOWN);
  return TR_OK;
}

}  // extern "C"
extern "C" {

int tr_roadmap_revalidate(tr_roadmap *r, int64_t *n_invalid_vertices, int64_t *n_invalid_edges) {
  if (!r) return TR_ERR_INVALID_ARG;
  RmLock lock_(r);
  return revalidate_locked(r, n_invalid_vertices, n_invalid_edges);
}

int tr_roadmap_get_validity(tr_roadmap *r, uint8_t *vertex_status, uint8_t *edge_status) {
  if (!r) return TR_ERR_INVALID_ARG;
  RmLock lock_(r);
  if (vertex_status) std::memcpy(vertex_status, r->vstat.data(), r->vstat.size());
  if (edge_status) std::memcpy(edge_status, r->estat.data(), r->estat.size());
  return TR_OK;
}

int tr_roadmap_set_validity(tr_roadmap *r, const uint8_t *vertex_status, const uint8_t *edge_status) {
  if (!r) return TR_ERR_INVALID_ARG;
  RmLock lock_(r);
  for (int64_t i = 0; vertex_status && i < r->V; i++) if (vertex_status[i] > V_INVALID) return rfail(r, TR_ERR_INVALID_ARG, "vertex status must be 0, 1 or 2");
  for (int64_t i = 0; edge_status && i < r->E; i++) if (edge_status[i] > V_INVALID) return rfail(r, TR_ERR_INVALID_ARG, "edge status must be 0, 1 or 2");
  if (vertex_status) std::memcpy(r->vstat.data(), vertex_status, r->vstat.size());
  if (edge_status) std::memcpy(r->estat.data(), edge_status, r->estat.size());
  return TR_OK;
}

int tr_roadmap_solve(tr_roadmap *r, const int32_t *starts, const int32_t *goals, int64_t n_queries, int32_t n_threads,
                     int32_t *status, double *cost, int64_t *path_offsets, tr_roadmap_stats *stats) {
  if (!r) return TR_ERR_INVALID_ARG;
  RmLock lock_(r);
  return solve_locked(r, starts, goals, n_queries, n_threads, status, cost, path_offsets, stats);
}

int tr_roadmap_search_stats(tr_roadmap *r, int64_t out[8]) {
  if (!r || !out) return TR_ERR_INVALID_ARG;
  RmLock lock_(r);
  out[0] = r->ds.st_queries; out[1] = r->ds.st_fallbacks; out[2] = r->ds.st_host_share; out[3] = r->ds.st_moves;
  out[4] = r->ds.st_expanded; out[5] = r->st_expanded - r->ds.st_expanded;
  out[6] = r->dc.st_cut; out[7] = r->ds.st_grows;
  return TR_OK;
}

int tr_roadmap_profile(tr_roadmap *r, double out[4]) {
  if (!r || !out) return TR_ERR_INVALID_ARG;
  RmLock lock_(r);
  const double deg = r->V > 0 ? (double)r->adj.size() / (double)r->V : 0.0;
  const int L = r->lm_n > 0 ? r->lm_n : 0;
  out[0] = r->ds.st_kernel_ms; out[1] = (double)r->ds.st_launches; out[2] = (double)r->ds.st_expanded;
  // per expansion: the vertex's record and row header, per arc the arc, two validity bytes, the arc count, the neighbour's record read
  // and written, its state and landmark rows
  out[3] = 48.0 + deg * (16.0 + 2.0 + 1.0 + 32.0 + 8.0 * r->S + 4.0 * L + 32.0);
  return TR_OK;
}

int tr_roadmap_release_search_state(tr_roadmap *r, int64_t *bytes_released) {
  if (!r) return TR_ERR_INVALID_ARG;
  RmLock lock_(r);
  RM_HIP(r, hipSetDevice(tr_device(r->ctx)));
  const size_t b = release_search_tables(r);
  dev_cache().trim();                                       // (not parked for the next owner: back to the device)
  if (bytes_released) *bytes_released = (int64_t)b;
  return TR_OK;
}

int tr_roadmap_search_sweeps(tr_roadmap *r, int64_t *n) {
  if (!r || !n) return TR_ERR_INVALID_ARG;
  RmLock lock_(r);
  *n = r->ds.st_sweeps;
  return TR_OK;
}

int tr_roadmap_reserve_search_state(tr_roadmap *r, int64_t n_queries) {
  if (!r || n_queries < 0) return TR_ERR_INVALID_ARG;
  RmLock lock_(r);
  RM_HIP(r, hipSetDevice(tr_device(r->ctx)));
  if (n_queries == 0) return TR_OK;
  const RoadmapSwitches sw = read_switches();
  if (!search_setup(r, sw) || !search_tables(r, n_queries, sw)) return rfail(r, TR_ERR_UNSUPPORTED, "device searches not available for this roadmap: " + r->ds.why);
  RM_HIP(r, hipStreamSynchronize(nullptr));
  return TR_OK;
}

int tr_roadmap_search_state_bytes(tr_roadmap *r, int64_t *bytes) {
  if (!r || !bytes) return TR_ERR_INVALID_ARG;
  RmLock lock_(r);
  const auto &d = r->ds;
  *bytes = (int64_t)((d.tables ? d.table_bytes : 0) + (d.qarena ? (size_t)d.nq_cap * 17 + (size_t)d.pbuf_cap * 4 : 0));
  return TR_OK;
}

int tr_roadmap_fetch_paths(tr_roadmap *r, int32_t *path_vertices, int64_t capacity) {
  if (!r) return TR_ERR_INVALID_ARG;
  RmLock lock_(r);
  const int64_t n = (int64_t)r->path_v.size();
  if (capacity < n) return rfail(r, TR_ERR_INVALID_ARG, "capacity smaller than the stored paths");
  if (n > 0) {
    if (!path_vertices) return rfail(r, TR_ERR_INVALID_ARG, "null output");
    std::memcpy(path_vertices, r->path_v.data(), (size_t)n * sizeof(int32_t));
  }
  return TR_OK;
}

}  // extern "C"

// An allocation somewhere in the library ran out of memory (tr_dev_cache_trim): the search tables of every roadmap that is not inside
// a call right now go back to the device; their next large round allocates them again.
void release_idle_search_tables() {
  std::lock_guard<std::mutex> g(g_roadmaps_mu);
  for (tr_roadmap *r : g_roadmaps) {
    if (r->busy.load(std::memory_order_acquire)) continue;  // (possibly by this very thread: the mutex is not asked)
    if (!r->mu.try_lock()) continue;
    (void)release_search_tables(r);
    r->mu.unlock();
  }
}
