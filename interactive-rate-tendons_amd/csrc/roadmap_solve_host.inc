// roadmap_solve_host.inc -- part of roadmap.hip: tr_roadmap_solve as a sequence of steps.
namespace {

// validity of the listed combined items (vertex v -> v, edge e -> V + e) against the current obstacle grid: one K4 launch
int check_items(tr_roadmap *r, const std::vector<int32_t> &list, std::vector<uint8_t> &hit) {
  hit.assign(list.size(), 0);
  if (list.empty()) return TR_OK;
  if (!r->has_caches) return rfail(r, TR_ERR_INVALID_ARG, "no voxel caches attached (tr_roadmap_set_caches)");
  const int64_t n = (int64_t)list.size();
  if (n > r->list_cap) {
    if (r->d_list) dev_cache().release(r->d_list);
    if (r->d_hit) dev_cache().release(r->d_hit);
    r->d_list = nullptr; r->d_hit = nullptr;
    r->list_cap = std::max<int64_t>(n + n / 2, 1 << 14);
    RM_HIP(r, dev_cache().alloc(tr_device(r->ctx), (void **)&r->d_list, (size_t)r->list_cap * sizeof(int32_t)));
    RM_HIP(r, dev_cache().alloc(tr_device(r->ctx), (void **)&r->d_hit, (size_t)r->list_cap));
  }
  RM_HIP(r, hipMemcpy(r->d_list, list.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice));
  const int rc = tr_check_cached_subset_dev(r->ctx, r->d_ids, r->d_masks, r->d_off, r->V + r->E, r->d_list, n, r->d_hit, nullptr);
  if (rc) return rfail(r, rc, tr_last_error(r->ctx));
  RM_HIP(r, hipMemcpy(hit.data(), r->d_hit, (size_t)n, hipMemcpyDeviceToHost));     // synchronises with the launch
  return TR_OK;
}

// (the caller holds r->mu)
int revalidate_locked(tr_roadmap *r, int64_t *n_invalid_vertices, int64_t *n_invalid_edges) {
  if (!r->has_caches) return rfail(r, TR_ERR_INVALID_ARG, "no voxel caches attached (tr_roadmap_set_caches)");
  RM_HIP(r, hipSetDevice(tr_device(r->ctx)));
  const int64_t items = r->V + r->E;
  int64_t nv = 0, ne = 0;
  if (items > 0) {
    const int rc = tr_check_cached_dev(r->ctx, r->d_ids, r->d_masks, r->d_off, items, r->d_bits, nullptr);
    if (rc) return rfail(r, rc, tr_last_error(r->ctx));
    // one kernel, one copy of the hit words into pinned memory, and a pass over WORDS, not items: a word's 64 items are marked
    // valid at once, then its set bits -- hits and missing caches, a few per cent of the items -- invalid one by one
    // (the per-item pass of round 3 was 0.4 of the call's 0.58 ms at 6.8 x 10^5 items, the kernel 0.115)
    const size_t nw = (size_t)(items + 63) / 64;
    RM_HIP(r, hipMemcpyAsync(r->h_bits, r->d_bits, nw * sizeof(uint64_t), hipMemcpyDeviceToHost, nullptr));
    RM_HIP(r, hipStreamSynchronize(nullptr));
    uint8_t *vs = r->vstat.data(), *es = r->estat.data();
    const int64_t V = r->V;
    for (size_t w = 0; w < nw; w++) {
      const int64_t q0 = (int64_t)w * 64, q1 = std::min<int64_t>(q0 + 64, items);
      uint64_t bad = r->h_bits[w] | r->absent[w];
      if (q1 - q0 < 64) bad &= ((uint64_t)1 << (q1 - q0)) - 1;
      if (q1 <= V || q0 >= V) {                             // the word's items are all vertices or all edges: valid, except the set bits
        uint8_t *st = q1 <= V ? vs + q0 : es + (q0 - V);
        std::memset(st, V_VALID, (size_t)(q1 - q0));
        (q1 <= V ? nv : ne) += __builtin_popcountll(bad);
        for (; bad; bad &= bad - 1) st[__builtin_ctzll(bad)] = V_INVALID;
        continue;
      }
      for (int64_t q = q0; q < q1; q++) {                   // (the one word that holds the last vertices and the first edges)
        const bool b = (bad >> (q - q0)) & 1;
        if (q < V) { vs[q] = b ? V_INVALID : V_VALID; nv += b; }
        else { es[q - V] = b ? V_INVALID : V_VALID; ne += b; }
      }
    }
  }
  if (n_invalid_vertices) *n_invalid_vertices = nv;
  if (n_invalid_edges) *n_invalid_edges = ne;
  return TR_OK;
}

// ---- what TENDON_HIP_SEARCH_STATS / TENDON_HIP_SEARCH_HIST print (stderr; people read these lines: the text is fixed) ----
// a shared round: times in ms from the round's start (`..._at`) or spans
void report_shared_round(int64_t round, double launched_at, double kernel_done_at, size_t n_dev, size_t n_share, double share_done_at, int64_t handed_back,
                         int64_t cut, double all_done_at, double collect, size_t n_after, double after, int64_t next_budget, double next_share) {
  std::fprintf(stderr, "[tendon_hip] round %lld: order + launch %.2f ms; kernel done at %.2f ms (%zu searches); host threads: own share %zu done at %.2f ms, %lld handed back meanwhile (%lld answered by labels), all done at %.2f ms; collect %.2f ms, %zu afterwards %.2f ms; next budget %lld, share %.4f\n",
               (long long)round, launched_at, kernel_done_at, n_dev, n_share, share_done_at, (long long)handed_back, (long long)cut, all_done_at, collect,
               n_after, after, (long long)next_budget, next_share);
}

// ---- tr_roadmap_solve: the state of one call, and the call as a sequence of steps (run) ----
struct Solve {
  tr_roadmap *const r;
  const int32_t *const starts, *const goals;
  const int64_t n_queries;
  int32_t *const status;
  double *const cost;
  const RoadmapSwitches &sw;
  const int T;
  SeededQueries *const seeded;                          // tr_roadmap_solve_seeded: the queries are seed lists (starts / goals null), every search astar_seeded's
  // (the queries' path vectors live with the roadmap: ten thousand small vectors cost 1 - 2 ms to allocate and to free per call otherwise)
  std::vector<std::vector<int32_t>> &paths, &paths_e;   // per query: vertices goal ... start, the edges between them
  std::vector<int64_t> active;                          // the queries still open; a "position" below is an index into it
  std::vector<uint8_t> found;                           // per position: this round's search came back with a candidate path
  std::vector<int32_t> list;                            // combined items to test (vertex v -> v, edge e -> V + e), and the verdicts
  std::vector<uint8_t> hit;
  std::vector<uint8_t> vmark, emark;                    // the item is on `list` already
  bool went_eager = false;                              // every cached set has been tested in this call: the next round is the last
  // of the round
  Clock::time_point t_round;
  bool labels_now = false;                              // r->dc.label holds the labels of this round's graph
  std::vector<size_t> todo, host_list, dev_list, redo;  // positions: that need a search; the host threads' share and the kernel's; left over by the kernel
  std::atomic<int64_t> expanded{0};
  std::atomic<bool> walked_in_vain{false};
  int64_t cap_sweep = 0;
  std::vector<int64_t> hist;                            // (TENDON_HIP_SEARCH_HIST) per position: expansions of its host search, and Scratch::trace_f
  std::vector<double> hist_f;

  Solve(tr_roadmap *r_, const int32_t *starts_, const int32_t *goals_, int64_t n, int32_t *status_, double *cost_, const RoadmapSwitches &sw_, int T_,
        SeededQueries *seeded_ = nullptr)
      : r(r_), starts(starts_), goals(goals_), n_queries(n), status(status_), cost(cost_), sw(sw_), T(T_), seeded(seeded_), paths(r_->paths_buf), paths_e(r_->paths_e_buf),
        vmark((size_t)r_->V, 0), emark((size_t)r_->E, 0) {
    if ((int64_t)paths.size() < n_queries) { paths.resize((size_t)n_queries); paths_e.resize((size_t)n_queries); }
    for (int64_t q = 0; q < n_queries; q++) { paths[(size_t)q].clear(); paths_e[(size_t)q].clear(); }
  }

  int run(Laps &laps, int64_t *path_offsets, tr_roadmap_stats *stats) {
    int rc;
    if ((rc = end_points()) || (rc = start_eager_if_large())) return rc;
    laps.lap("end points + set-up");
    while (!active.empty()) {
      begin_round();
      const bool on_device = !seeded && launch_on_device();     // (seeded searches: the host threads at every batch size)
      begin_host_searches();
      if (!on_device) host_round(todo);
      else if ((rc = shared_round())) return rc;
      if (walked_in_vain.load()) r->dc.wanted = true;
      if (sw.hist) report_hist();
      laps.lap("searches");
      r->st_astar_runs += (int64_t)todo.size();
      r->st_expanded += expanded.load();
      if ((rc = check_candidates())) return rc;
      std::vector<int64_t> still = settle();
      if ((rc = turn_eager_if_many_open((int64_t)still.size()))) return rc;
      active.swap(still);
      laps.lap("items + verdicts");
    }
    paths_out(path_offsets);
    laps.lap("paths out");
    if (stats) *stats = tr_roadmap_stats{r->st_rounds, r->st_items_checked, r->st_astar_runs, r->st_expanded};
    if (sw.stats) report_searches();
    return TR_OK;
  }

  // One K4 launch on `list`; the items become known: a missing cache (the voxelisation found the shape invalid when the cache was
  // built) is invalid for good
  int test_listed() {
    if (list.empty()) return TR_OK;
    if (const int rc = check_items(r, list, hit)) return rc;
    for (size_t k = 0; k < list.size(); k++) {
      const int64_t it = list[k], e = it - r->V;
      if (it < r->V) { r->vstat[(size_t)it] = (hit[k] || !r->vpresent[(size_t)it]) ? V_INVALID : V_VALID; vmark[(size_t)it] = 0; }
      else { r->estat[(size_t)e] = (hit[k] || !r->epresent[(size_t)e]) ? V_INVALID : V_VALID; emark[(size_t)e] = 0; }
    }
    r->st_items_checked += (int64_t)list.size();
    return TR_OK;
  }

  // a query with an end point known invalid ends with that status
  bool invalid_end_point(int64_t q) {
    if (r->vstat[(size_t)starts[q]] == V_INVALID) { status[q] = TR_QUERY_INVALID_START; return true; }
    if (r->vstat[(size_t)goals[q]] == V_INVALID) { status[q] = TR_QUERY_INVALID_GOAL; return true; }
    return false;
  }

  // the query end points first (solvePrep :2978-3010 only admits valid start / goal states)
  // tr_roadmap_solve_seeded: the seed vertices of unknown validity are tested first, as the end points are; a seed whose vertex is
  // invalid is no seed (astar_seeded skips it -- also one that a later eager test finds invalid)
  int seed_vertices() {
    for (int side = 0; side < 2; side++) {
      const int64_t n_seeds = (side ? seeded->dst_off : seeded->src_off)[n_queries];
      const int32_t *sv = side ? seeded->dst_v : seeded->src_v;
      for (int64_t i = 0; i < n_seeds; i++)
        if (r->vstat[(size_t)sv[i]] == V_UNKNOWN && !vmark[(size_t)sv[i]]) { vmark[(size_t)sv[i]] = 1; list.push_back(sv[i]); }
    }
    if (const int rc = test_listed()) return rc;
    for (int64_t q = 0; q < n_queries; q++) {
      status[q] = TR_QUERY_SOLVED;
      cost[q] = std::numeric_limits<double>::infinity();
      seeded->src_pick[q] = seeded->dst_pick[q] = -1;
      active.push_back(q);
    }
    return TR_OK;
  }

  int end_points() {
    if (seeded) return seed_vertices();
    for (int64_t q = 0; q < n_queries; q++) {
      for (int32_t v : {starts[q], goals[q]})
        if (r->vstat[(size_t)v] == V_UNKNOWN && !vmark[(size_t)v]) { vmark[(size_t)v] = 1; list.push_back(v); }
    }
    if (const int rc = test_listed()) return rc;
    for (int64_t q = 0; q < n_queries; q++) {
      status[q] = TR_QUERY_SOLVED;
      if (cost) cost[q] = std::numeric_limits<double>::infinity();
      if (invalid_end_point(q)) continue;
      if (starts[q] == goals[q]) { paths[(size_t)q] = {starts[q]}; if (cost) cost[q] = 0.0; }   // constructSolution :2696-2701
      else active.push_back(q);
    }
    return TR_OK;
  }

  // The loop turns eager: ONE launch tests every cached set (0.25 ms at 6.8 x 10^5 sets), what was unknown is booked as checked, and
  // the searches that follow run on known validity.  Three rules call this (below); each reads counts, never a clock, so rounds,
  // items_checked and the validity a call leaves behind are the same run after run (tests/test_gpu_search.py), and
  // TENDON_HIP_LAZY_ONLY=1 forbids all three (the reference's loop item by item).  Answers are those of the lazy loop (validity is a
  // function of the environment); what changes is which items end up known.
  int test_everything(bool only_if_unknown = false) {
    int64_t unknown = 0;
    for (uint8_t x : r->vstat) unknown += x == V_UNKNOWN;
    for (uint8_t x : r->estat) unknown += x == V_UNKNOWN;
    if (only_if_unknown && unknown == 0) return TR_OK;
    if (const int rc = revalidate_locked(r, nullptr, nullptr)) return rc;
    r->st_items_checked += unknown;
    went_eager = true;
    return TR_OK;
  }

  // Rule 1: a batch so large that its candidate paths would hold a quarter of the cached sets anyway (at ~64 items a path) does not
  // start lazily: the searches run on known validity -- one round instead of two or more.
  int start_eager_if_large() {
    if (!r->has_caches || (int64_t)active.size() * 256 < r->V + r->E || sw.lazy_only) return TR_OK;
    if (const int rc = test_everything(true)) return rc;
    if (!went_eager || seeded) return TR_OK;
    // (end points found invalid by that test: their queries end here, as they would have before the first search)
    std::vector<int64_t> keep;
    for (int64_t q : active) if (!invalid_end_point(q)) keep.push_back(q);
    active.swap(keep);
    return TR_OK;
  }

  // Rule 3.  The lazy loop exists to save validity tests; here a test of EVERY cached set is one K4 launch, while every further round
  // costs at least its longest search (milliseconds on a core) -- and in a cluttered environment the open queries find new candidate
  // paths through untested items round after round, hundreds of rounds in the worst case.  So when enough queries are still open for
  // another round to cost more than that launch (one open query per 2^17 sets, four at least), everything is tested.
  int turn_eager_if_many_open(int64_t n_open) {
    const int64_t eager_from = std::max<int64_t>(4, (r->V + r->E) >> 17);
    if (went_eager || !r->has_caches || n_open < eager_from || sw.lazy_only) return TR_OK;
    return test_everything();
  }

  bool ensure_labels() {
    if (labels_now) return true;
    const auto t_cc = Clock::now();
    if (sw.components_mode == 0 || !component_labels(r, sw)) return false;
    labels_now = true;
    if (sw.stats) std::fprintf(stderr, "[tendon_hip] round %lld: component labels %.3f ms\n", (long long)r->st_rounds, ms_between(t_cc, Clock::now()));
    return true;
  }

  // The label filter: a query whose end points carry different labels (r->dc.label) has no path; it is answered without a search.
  bool cut_by_labels(size_t k) {
    const int64_t q = active[k];
    if (r->dc.label[(size_t)starts[q]] == r->dc.label[(size_t)goals[q]]) return false;
    found[k] = 0;
    r->dc.st_cut++;
    return true;
  }
  // ... over a list of positions: those cut leave it; returns how many did
  int64_t cut_by_labels(std::vector<size_t> &positions) {
    const size_t n = positions.size();
    positions.erase(std::remove_if(positions.begin(), positions.end(), [this](size_t k) { return cut_by_labels(k); }), positions.end());
    return (int64_t)(n - positions.size());
  }

  // A round: every open query needs a search, except those the labels answer: queries whose end points lie in different components
  // of what is left of the graph have no path (rounds of kComponentMinQueries or more; TENDON_HIP_COMPONENTS=0 searches them as
  // before, to the same answer)
  void begin_round() {
    r->st_rounds++;
    found.assign(active.size(), 0);
    expanded.store(0);
    walked_in_vain.store(false);
    r->dc.status_current = false;
    labels_now = false;
    host_list.clear(); dev_list.clear(); redo.clear();
    todo.resize(active.size());
    for (size_t k = 0; k < active.size(); k++) todo[k] = k;
    const int cmode = sw.components_mode;
    if (!seeded && (int64_t)active.size() >= kComponentMinQueries && (cmode == 2 || (cmode == 1 && r->dc.wanted)) && ensure_labels()) cut_by_labels(todo);
    t_round = Clock::now();
  }

  // ... on the device when the round is large enough to fill it (search_kernel.hpp).  The searches are ordered by the state-space
  // distance between their end points, longest first: the host threads take the head of that order (a core expands a vertex in
  // a fraction of the time a wave does, so the searches expected to be longest are theirs) while the kernel works through the
  // rest, longest first; what the kernel hands back (over its pop budget, or a list full) the host threads search afterwards.
  // false: the round is the host threads' alone.
  bool launch_on_device() {
    const int smode = sw.search_mode;
    if (todo.empty() || !(smode == 2 || (smode == 1 && (int64_t)todo.size() >= kSearchMinQueries))) return false;
    std::vector<std::pair<double, size_t>> key(todo.size());
    for (size_t j = 0; j < todo.size(); j++) {
      const size_t k = todo[j];
      const int64_t q = active[k];
      key[j] = {state_distance(r, &r->states[(size_t)starts[q] * r->S], &r->states[(size_t)goals[q] * r->S]), k};
    }
    std::sort(key.begin(), key.end(), [](const std::pair<double, size_t> &x, const std::pair<double, size_t> &y) { return x.first > y.first || (x.first == y.first && x.second < y.second); });
    if (r->ds.share < 0 || sw.host_share_set) r->ds.share = sw.host_share;
    const size_t n_h = smode == 2 ? 0 : (size_t)((double)todo.size() * r->ds.share);
    for (size_t i = 0; i < key.size(); i++) (i < n_h ? host_list : dev_list).push_back(key[i].second);
    // (a roadmap's first shared round: 6 500 expansions, or a sixteenth of its vertices if that is more -- searches grow with the
    // graph; afterwards the budget doubles whenever more than one search in fifty came back: adapt_schedule.  A budget the LAST call
    // took from the environment is chosen anew)
    if (r->ds.budget == 0 || sw.budget_set || r->ds.budget_from_env) r->ds.budget = sw.budget_set ? sw.budget : std::max<int64_t>(sw.budget, r->V / 16);
    r->ds.budget_from_env = sw.budget_set;
    // (TENDON_HIP_SEARCH=device: no budget unless TENDON_HIP_SEARCH_BUDGET asks for one)
    if (!device_search_launch(r, starts, goals, active, dev_list, smode == 2 && !sw.budget_set ? 0 : r->ds.budget, sw)) {
      host_list.clear(); dev_list.clear();
      return false;
    }
    r->ds.st_host_share += (int64_t)host_list.size();
    return true;
  }

  // (after the launch: the first one sets the device searches up, and sweep_cap asks whether they are)
  void begin_host_searches() {
    cap_sweep = seeded ? 0 : sweep_cap(r, sw);
    if (sw.hist) { hist.assign(active.size(), 0); hist_f.assign(active.size() * 4, 0.0); }
  }

  // one query on a host thread: A*, and past sweep_cap expansions the parallel sweep on the device (which failing, A* to the end)
  void search_on_host(Scratch &sc, size_t k, int64_t &ex) {
    const int64_t q = active[k], ex0 = ex;
    if (seeded) {
      found[k] = astar_seeded(r, sc, *seeded, q, paths[(size_t)q], paths_e[(size_t)q], ex) ? 1 : 0;
      if (sw.hist) hist[k] = ex - ex0;
      return;
    }
    bool abandoned = false;
    bool f = astar(r, sc, starts[q], goals[q], paths[(size_t)q], paths_e[(size_t)q], ex, cap_sweep, &abandoned);
    if (abandoned) {
      const int m = sweep_search(r, starts[q], goals[q], paths[(size_t)q], paths_e[(size_t)q]);
      f = m >= 0 ? m == 1 : astar(r, sc, starts[q], goals[q], paths[(size_t)q], paths_e[(size_t)q], ex);
    }
    found[k] = f ? 1 : 0;
    if (!f && ex - ex0 >= kComponentTrigger) walked_in_vain.store(true, std::memory_order_relaxed);
    if (sw.hist) { hist[k] = ex - ex0; for (int i = 0; i < 4; i++) hist_f[k * 4 + (size_t)i] = sc.trace_f[i]; }
  }

  // the host threads over a list of positions
  void host_round(const std::vector<size_t> &positions) {
    const int64_t n_host = (int64_t)positions.size();
    if (n_host == 0) return;
    std::atomic<int64_t> next{0};
    on_threads((int)std::min<int64_t>(T, n_host), [&](int t) {
      int64_t ex = 0;
      for (int64_t j; (j = next.fetch_add(1)) < n_host;) search_on_host(r->scratch[(size_t)t], positions[(size_t)j], ex);
      expanded += ex;
    });
  }

  // one host thread of a shared round
  template <class Feed> void serve(Feed &feed, int t, int dev_id) {
    (void)hipSetDevice(dev_id);
    int64_t ex = 0;
    feed.run([&](size_t k) { search_on_host(r->scratch[(size_t)t], k, ex); });
    expanded += ex;
  }

  // The round the kernel and the host threads share (handback_feed.hpp).  Unreachable goals among the searches the kernel hands back
  // are weeded out by component labels computed here on the host (the device's stream is busy), once, when the first one comes back.
  // A stream that reports an error ends the call: the host threads finish what they were fed, then TR_ERR_HIP.
  int shared_round() {
    const int dev_id = tr_device(r->ctx);
    const uint32_t *flags = (r->ds.handback_cap >= (int64_t)dev_list.size()) ? r->ds.h_handback : nullptr;
    const int64_t n_dev = (int64_t)dev_list.size(), n_share = (int64_t)host_list.size(), cut0 = r->dc.st_cut;
    bool labels_host = labels_now;                              // (poller only)
    hipError_t stream_error = hipSuccess;                       // (poller only)
    handback::Feed feed(
        flags, dev_list, host_list, active.size(),
        [&stream_error] {
          const hipError_t e = hipStreamQuery(nullptr);
          if (e == hipSuccess) return handback::Stream::done;
          if (e == hipErrorNotReady) return handback::Stream::running;
          stream_error = e;
          return handback::Stream::failed;
        },
        [&](size_t k) {
          if (!labels_host && sw.components_mode != 0) { host_component_labels(r); labels_host = true; }
          return !(labels_host && cut_by_labels(k));
        });
    on_threads(std::max(1, T), [&](int t) { serve(feed, t, dev_id); });
    const int64_t n_cut_host = r->dc.st_cut - cut0;
    if (n_cut_host) r->dc.wanted = true;
    if (feed.failed) {
      r->ds.in_flight = 0;
      return rfail(r, TR_ERR_HIP, std::string("hipStreamQuery(nullptr): ") + hipGetErrorString(stream_error));
    }
    const auto t1 = Clock::now();
    int64_t ex = 0;
    device_search_collect(r, active, dev_list, found, paths, paths_e, redo, ex, T, sw, &feed.handled);
    expanded += ex;
    const auto t_kernel_done = feed.stream_done ? feed.stream_done_at : Clock::now();     // (no flags to poll: collect waited for it)
    const auto t2 = Clock::now();
    // what is left (a path that did not fit its buffer; everything, without the pinned words): as before, after the kernel
    if (!redo.empty() && !labels_now && !labels_host && ensure_labels()) labels_host = true;
    if (!redo.empty() && (labels_now || labels_host) && cut_by_labels(redo) > 0) r->dc.wanted = true;
    host_round(redo);
    const auto t3 = Clock::now();
    const double t_kernel = ms_between(t_round, t_kernel_done), t_after = std::max(0.0, ms_between(t_kernel_done, t3)),
                 t_share = n_share ? ms_between(feed.started_at, feed.own_done_at) : 0.0;
    // (only the searches that came back OVER THE BUDGET count: one that found no table left for its records says nothing about the budget --
    // at 6 x 10^5 vertices those alone are 2 % of a round, and doubling on them let single searches run 600 ms on their wave)
    adapt_schedule(flags ? feed.over_budget : feed.handed_back + (int64_t)redo.size(), n_dev, n_share, t_kernel, t_after, t_share);
    if (sw.stats)
      report_shared_round(r->st_rounds, ms_between(t_round, feed.started_at), t_kernel, dev_list.size(), host_list.size(), ms_between(t_round, feed.own_done_at),
                          feed.handed_back, n_cut_host, ms_between(t_round, t1), ms_between(t1, t2), redo.size(), ms_between(t2, t3), r->ds.budget, r->ds.share);
    return TR_OK;
  }

  // The budget doubles when more than one search in fifty came back.  The host's share follows the clock (answers do not depend on
  // it): halved when the host's own share outlasted the kernel, raised when it was done in a fraction of the kernel's span and
  // nothing was left to do after it.
  void adapt_schedule(int64_t came_back, int64_t n_dev, int64_t n_share, double t_kernel, double t_after, double t_share) {
    auto &d = r->ds;
    d.kernel_ms = t_kernel; d.host_after_ms = t_after;
    if (sw.search_mode == 2) return;
    if (!d.budget_from_env && d.budget > 0 && came_back * 50 > n_dev && d.budget < 16 * r->V) d.budget *= 2;
    if (!sw.host_share_set && n_share > 0) {
      if (t_share > t_kernel) d.share = std::max(0.0025, d.share * 0.5);
      else if (t_share < 0.4 * t_kernel && t_after < 0.1 * t_kernel) d.share = std::min(0.08, d.share * 1.5);
    }
  }

  int range_threads() const { return active.size() >= 2048 ? std::min(T, 16) : 1; }     // (large rounds: by ranges of queries on the host threads)

  // unknown items on the candidate paths: all interior vertices, and the edges of paths without an unknown vertex
  // are only worth testing once the vertices are clean -- but testing them in the same launch costs nothing, saves
  // a round, and removing more invalid items never changes an accepted path (see the header comment of roadmap.hip)
  int check_candidates() {
    list.clear();
    // (Rule 2: a large round from unknown validity: when the candidate paths hold a quarter as many items as there are cached sets, listing
    // the unknown ones, sending the list and fetching the verdicts costs several times the one launch that tests EVERY cached set)
    if (!went_eager && r->has_caches && !sw.lazy_only) {
      int64_t on_paths = 0;
      for (size_t k = 0; k < active.size(); k++)
        if (found[k]) on_paths += (int64_t)(paths[(size_t)active[k]].size() + paths_e[(size_t)active[k]].size());
      if (on_paths * 4 >= r->V + r->E) return test_everything();
    }
    gather_unknown_items();
    return test_listed();
  }

  // (an item goes to the list of the thread that marks it first -- the set is the same whoever that is, and the order of the list decides nothing)
  void gather_unknown_items() {
    const int Tb = range_threads();
    std::vector<std::vector<int32_t>> part((size_t)Tb);
    on_threads(Tb, [&](int t) {
      std::vector<int32_t> &mine = part[(size_t)t];
      const size_t k0 = active.size() * (size_t)t / (size_t)Tb, k1 = active.size() * (size_t)(t + 1) / (size_t)Tb;
      for (size_t k = k0; k < k1; k++) {
        if (!found[k]) continue;
        const int64_t q = active[k];
        const auto &pv = paths[(size_t)q];
        const auto &pe = paths_e[(size_t)q];
        for (size_t i = 1; i + 1 < pv.size(); i++) {
          const int32_t v = pv[i];
          if (r->vstat[(size_t)v] == V_UNKNOWN && !__atomic_exchange_n(&vmark[(size_t)v], (uint8_t)1, __ATOMIC_RELAXED)) mine.push_back(v);
        }
        for (int32_t e : pe)
          if (r->estat[(size_t)e] == V_UNKNOWN && !__atomic_exchange_n(&emark[(size_t)e], (uint8_t)1, __ATOMIC_RELAXED)) mine.push_back((int32_t)(r->V + e));
      }
    });
    for (const auto &p : part) list.insert(list.end(), p.begin(), p.end());
  }

  // queries whose candidate path turned out all valid are done (their cost is booked); no candidate: no path; the others stay open
  std::vector<int64_t> settle() {
    const int Tb = range_threads();
    std::vector<std::vector<int64_t>> part((size_t)Tb);
    on_threads(Tb, [&](int t) {
      const size_t k0 = active.size() * (size_t)t / (size_t)Tb, k1 = active.size() * (size_t)(t + 1) / (size_t)Tb;
      for (size_t k = k0; k < k1; k++) {
        const int64_t q = active[k];
        if (!found[k]) { status[q] = TR_QUERY_NO_PATH; paths[(size_t)q].clear(); continue; }   // different components (:2026-2036)
        bool ok = true;
        for (size_t i = 1; i + 1 < paths[(size_t)q].size() && ok; i++) ok = r->vstat[(size_t)paths[(size_t)q][i]] == V_VALID;
        for (size_t i = 0; i < paths_e[(size_t)q].size() && ok; i++) ok = r->estat[(size_t)paths_e[(size_t)q][i]] == V_VALID;
        if (ok) {
          if (seeded) cost[q] = seeded_cost(q);
          else if (cost) { double c = 0; for (size_t i = paths_e[(size_t)q].size(); i-- > 0;) c += r->w[(size_t)paths_e[(size_t)q][i]]; cost[q] = c; }
        } else part[(size_t)t].push_back(q);
      }
    });
    std::vector<int64_t> still;
    for (const auto &p : part) still.insert(still.end(), p.begin(), p.end());    // (ranges in order: the queries keep their order)
    return still;
  }

  // ((c_i + w_1) + w_2 ...) + d_j from the source along the accepted path: A*'s own g, then the target seed; the direct cost without a path
  double seeded_cost(int64_t q) const {
    const int32_t i = seeded->src_pick[q], j = seeded->dst_pick[q];
    if (i < 0) return seeded->direct[q];
    double c = seeded->src_c[seeded->src_off[q] + i];
    for (size_t e = paths_e[(size_t)q].size(); e-- > 0;) c += r->w[(size_t)paths_e[(size_t)q][e]];
    return c + seeded->dst_c[seeded->dst_off[q] + j];
  }

  void paths_out(int64_t *path_offsets) {
    for (int64_t q = 0; q < n_queries; q++) {
      const auto &pv = paths[(size_t)q];
      if (status[q] == TR_QUERY_SOLVED) r->path_v.insert(r->path_v.end(), pv.rbegin(), pv.rend());     // start ... goal
      r->path_off[(size_t)q + 1] = (int64_t)r->path_v.size();
      path_offsets[q + 1] = r->path_off[(size_t)q + 1];
    }
  }

  // (reports)
  void report_hist() const;
  void report_searches() const {
    std::fprintf(stderr, "[tendon_hip] searches: mode %d, device state %d%s%s, %lld slots, %lld searches finished on the device, %lld handed back to the host, %lld on the host meanwhile, %lld answered by a sweep\n",
                 sw.search_mode, r->ds.state, r->ds.why.empty() ? "" : " -- ", r->ds.why.c_str(), (long long)r->ds.slots, (long long)r->ds.st_queries,
                 (long long)r->ds.st_fallbacks, (long long)r->ds.st_host_share, (long long)r->ds.st_sweeps);
  }
};

void report_expansions(const char *name, std::vector<int64_t> &v) {
  if (v.empty()) { std::fprintf(stderr, "  %s: none\n", name); return; }
  std::sort(v.begin(), v.end());
  int64_t sum = 0; for (int64_t x : v) sum += x;
  std::fprintf(stderr, "  %s: %zu searches, %lld expansions; median %lld, 90%% %lld, 99%% %lld, max %lld\n", name, v.size(), (long long)sum,
               (long long)v[v.size() / 2], (long long)v[v.size() * 9 / 10], (long long)v[v.size() * 99 / 100], (long long)v.back());
}

void Solve::report_hist() const {
  std::vector<int64_t> f, nf;
  for (size_t k = 0; k < active.size(); k++) (found[k] ? f : nf).push_back(hist[k]);
  std::fprintf(stderr, "[tendon_hip] round %lld:\n", (long long)r->st_rounds);
  report_expansions("found", f); report_expansions("not found", nf);
  // (the file's columns describe a search between two vertices: a seeded query has seed lists, no `starts` / `goals` -- the summary above is its report)
  if (!sw.hist_path || seeded) return;
  FILE *fh = std::fopen(sw.hist_path, "a");                   // (a path: one line per search -- expansions against what could predict them)
  if (!fh) return;
  const int L = r->lm_n > 0 ? r->lm_n : 0;
  for (size_t k = 0; k < active.size(); k++) {
    const int64_t q = active[k];
    const int32_t s_ = starts[q], g_ = goals[q];
    double lb = 0.0, sum_s = 1e300;
    for (int l = 0; l < L; l++) {
      const double a_ = r->lm_d[(size_t)s_ * L + l], b_ = r->lm_d[(size_t)g_ * L + l];
      lb = std::max(lb, std::fabs(a_ - b_)); sum_s = std::min(sum_s, a_ + b_);
    }
    std::fprintf(fh, "%lld %lld %d %lld %.6g %.6g %.6g %d %d %.6g %.6g %.6g %.6g\n", (long long)r->st_rounds, (long long)q, (int)found[k], (long long)hist[k],
                 state_distance(r, &r->states[(size_t)s_ * r->S], &r->states[(size_t)g_ * r->S]), lb, sum_s,
                 (int)(r->adj_off[(size_t)s_ + 1] - r->adj_off[(size_t)s_]), (int)(r->adj_off[(size_t)g_ + 1] - r->adj_off[(size_t)g_]),
                 hist_f[k * 4], hist_f[k * 4 + 1], hist_f[k * 4 + 2], hist_f[k * 4 + 3]);
  }
  std::fclose(fh);
}

// what the last call left behind goes, before the first check that can fail
void reset_last_solve(tr_roadmap *r, int64_t n_queries) {
  r->path_off.assign((size_t)n_queries + 1, 0); r->path_v.clear();
  r->st_rounds = r->st_items_checked = r->st_astar_runs = r->st_expanded = 0;
  r->ds.st_queries = r->ds.st_fallbacks = r->ds.st_host_share = r->ds.st_moves = r->ds.st_expanded = r->ds.st_grows = r->ds.st_max_records = 0;
  r->ds.st_kernel_ms = 0; r->ds.st_launches = 0;
  r->ds.st_sweeps = 0; r->ds.sweep_round = -1;
  r->dc.st_cut = 0;
}

// tr_roadmap_solve behind the lock (tr_roadmap_solve_tips runs the same call on the connection vertices its IK step chose)
int solve_locked(tr_roadmap *r, const int32_t *starts, const int32_t *goals, int64_t n_queries, int32_t n_threads,
                 int32_t *status, double *cost, int64_t *path_offsets, tr_roadmap_stats *stats) {
  if (n_queries < 0 || (n_queries > 0 && (!starts || !goals || !status || !path_offsets))) return rfail(r, TR_ERR_INVALID_ARG, "bad argument");
  reset_last_solve(r, n_queries);
  if (path_offsets) path_offsets[0] = 0;
  if (n_queries == 0) { if (stats) *stats = tr_roadmap_stats{0, 0, 0, 0}; return TR_OK; }
  for (int64_t q = 0; q < n_queries; q++)
    if (starts[q] < 0 || starts[q] >= r->V || goals[q] < 0 || goals[q] >= r->V) return rfail(r, TR_ERR_OUT_OF_RANGE, "query vertex outside the roadmap");
  RM_HIP(r, hipSetDevice(tr_device(r->ctx)));
  const RoadmapSwitches sw = read_switches();
  Laps laps(sw, "tr_roadmap_solve");
  const int T = host_threads(n_threads);
  if ((int)r->scratch.size() < T) r->scratch.resize((size_t)T);
  for (Scratch &sc : r->scratch) sc.trace = sw.hist_path != nullptr;
  if (r->lm_n < 0 && n_queries >= 64) build_landmarks(r, 16, T, sw);         // a handful of queries does not repay 16 graph sweeps
  Solve solve(r, starts, goals, n_queries, status, cost, sw, T);
  return solve.run(laps, path_offsets, stats);
}

}  // namespace
