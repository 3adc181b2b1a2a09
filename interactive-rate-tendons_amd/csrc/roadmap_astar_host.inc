// roadmap_astar_host.inc -- part of roadmap.hip: the graph search on a host thread and the landmark tables of its heuristic.
namespace {

// CompoundStateSpace::distance with the subspace weights of motion-planning/Problem.cpp:112-152
inline double state_distance(const tr_roadmap *r, const double *a, const double *b) {
  double s = 0;
  for (int i = 0; i < r->NT; i++) { const double d = a[i] - b[i]; s += d * d; }
  double dist = std::sqrt(s);
  int k = r->NT;
  if (r->rot) {
    double d = std::fabs(a[k] - b[k]);
    d = (d > M_PI) ? 2.0 * M_PI - d : d;
    dist += r->w_rot * d;
    k++;
  }
  if (r->ret) { const double d = a[k] - b[k]; dist += r->w_ret * std::sqrt(d * d); }
  return dist;
}

// relative slack that keeps the float-stored landmark distances on the safe side of the true ones (rounding to float is
// 2^-24 relative per distance; the fp64 path sums behind them differ from A*'s own sums by ~1e-16 per hop)
constexpr double kLmSlack = 1.0 / (1 << 21);

// The heuristic of one search towards one goal vertex: the state-space distance (costHeuristic :2773-2775 -> motionCostHeuristic),
// and with landmark tables the larger of that and the landmark bounds; +inf where a landmark shows v and the goal in different components.
struct GoalHeuristic {
  const tr_roadmap *const r;
  const double *const sg;
  const int L;
  const float *const lg;
  GoalHeuristic(const tr_roadmap *r_, int32_t goal)
      : r(r_), sg(&r_->states[(size_t)goal * r_->S]), L(r_->lm_n > 0 ? r_->lm_n : 0), lg(L ? &r_->lm_d[(size_t)goal * L] : nullptr) {}
  double operator()(int32_t v) const {
    const double inf = std::numeric_limits<double>::infinity();
    double h = state_distance(r, &r->states[(size_t)v * r->S], sg);
    if (L) {
      // (SR_LM_FAR where a vertex is not connected to the landmark: two far entries bound nothing -- their term is hugely negative --, one
      // makes the term huge: different components; no comparison with infinity, no branch: the loop vectorises, and every term is the
      // kernel's (search_kernel.hpp: heuristic), float operation for float operation)
      const float *lv = &r->lm_d[(size_t)v * L];
      const float slack = (float)kLmSlack;
      float b8[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};   // (eight running maxima side by side: element-wise work the compiler turns into vector code)
      int l = 0;
      for (; l + 8 <= L; l += 8)
        for (int j = 0; j < 8; j++) {
          const float a = lv[l + j], b = lg[l + j];
          const float hi = a > b ? a : b, lo = a > b ? b : a;
          const float t = (hi - lo) - slack * hi;                // float subtraction of nearby values: error <= 2^-24 hi, inside the slack
          b8[j] = t > b8[j] ? t : b8[j];
        }
      float best = 0.0f;
      for (; l < L; l++) {
        const float a = lv[l], b = lg[l];
        const float hi = a > b ? a : b, lo = a > b ? b : a;
        const float t = (hi - lo) - slack * hi;
        best = t > best ? t : best;
      }
      for (int j = 0; j < 8; j++) best = b8[j] > best ? b8[j] : best;
      if (best >= 0.5f * trk::SR_LM_FAR) return inf;
      if ((double)best > h) h = (double)best;
    }
    return h;
  }
};

// astarSearch (:2950-2976): A* with the state-space distance to the goal as heuristic (costHeuristic :2773-2775 ->
// motionCostHeuristic), edge weights as given; stops when the goal is taken off the open list (AStarGoalVisitor).
// Vertices / edges known invalid are not part of the graph (the reference has removed them).  Returns false when the
// goal cannot be reached.  path: goal ... start (vertex ids), path_e: the edges between them.
// With landmark tables the heuristic is the larger of that distance and the landmark bounds: admissible, so the goal
// leaves the open list with the same (optimal) cost and, ties apart, the same parents; a vertex whose cost improves after
// it was expanded is opened again (with the consistent state-space distance alone that never happens).
// `cap` > 0: the search gives up after that many expansions (*abandoned = true, false returned): tr_roadmap_solve then answers it with a
// parallel sweep on the device (sweep_search below) -- a search that expands a large part of the graph is a poor fit for one core.
bool astar(const tr_roadmap *r, Scratch &sc, int32_t start, int32_t goal, std::vector<int32_t> &path, std::vector<int32_t> &path_e,
           int64_t &expanded, int64_t cap = 0, bool *abandoned = nullptr) {
  if (sc.node.size() != (size_t)r->V) { sc.node.assign((size_t)r->V, Node{0.0, 0.0, -1, -1, 0u, 0u}); sc.gen = 0; }
  if (++sc.gen == 0) { for (Node &nd : sc.node) nd.stamp = 0u; sc.gen = 1; }
  Node *node = sc.node.data();
  const uint32_t gen = sc.gen;
  auto &heap = sc.heap;
  heap.clear();
  const GoalHeuristic heuristic(r, goal);
  const int L = heuristic.L;
  const double inf = std::numeric_limits<double>::infinity();
  auto cmp = [](const std::pair<double, int32_t> &a, const std::pair<double, int32_t> &b) { return a.first > b.first; };
  node[start] = Node{0.0, heuristic(start), start, -1, gen, 0u};
  if (node[start].h == inf) return false;
  const bool trace = sc.trace;
  const int64_t expanded0 = expanded;
  if (trace) { sc.trace_f[0] = node[start].h; sc.trace_f[1] = sc.trace_f[2] = sc.trace_f[3] = 0.0; }
  heap.emplace_back(node[start].h, start);
  bool found = false;
  constexpr bool node_is_new_hint = true;       // (the state / landmark rows are only read for a vertex met for the first time; most are)
  while (!heap.empty()) {
    std::pop_heap(heap.begin(), heap.end(), cmp);
    const int32_t u = heap.back().second;
    heap.pop_back();
    if (!heap.empty()) {                        // the likely next vertex: its record and its arcs on their way while this one is expanded
      const int32_t nx = heap.front().second;   // (the top's two children as well: measured, no gain)
      __builtin_prefetch(&node[nx]);
      __builtin_prefetch(r->adj.data() + r->adj_off[nx]);
    }
    if (node[u].closed) continue;               // a stale entry of a vertex already expanded with a better cost
    node[u].closed = 1u;
    expanded++;
    if (trace) {
      const int64_t n_ = expanded - expanded0;
      if (n_ == 2000) sc.trace_f[1] = node[u].g + node[u].h;
      else if (n_ == 3000) sc.trace_f[2] = node[u].g + node[u].h;
      else if (n_ == 4000) sc.trace_f[3] = node[u].g + node[u].h;
    }
    if (cap > 0 && expanded - expanded0 > cap) { if (abandoned) *abandoned = true; return false; }
    if (u == goal) { found = true; break; }
    const double gu = node[u].g;
    const Arc *arc = r->adj.data() + r->adj_off[u], *end = r->adj.data() + r->adj_off[u + 1];
    // (every neighbour is four lines somewhere in a few hundred megabytes -- its record, its validity byte, its state, its landmark
    // row: asked for together before the first is used, the misses overlap instead of queueing behind one another)
    for (const Arc *a = arc; a != end; ++a) {
      const int32_t v = a->v;
      __builtin_prefetch(&node[v], 1);
      __builtin_prefetch(&r->vstat[v]);
      __builtin_prefetch(&r->estat[a->e]);
      if (node_is_new_hint) {
        __builtin_prefetch(&r->states[(size_t)v * r->S]);
        if (L) __builtin_prefetch(&r->lm_d[(size_t)v * L]);
      }
    }
    for (; arc != end; ++arc) {
      const int32_t e = arc->e, v = arc->v;
      if (r->estat[e] == V_INVALID || r->vstat[v] == V_INVALID) continue;
      const double gv = gu + arc->w;
      Node &nv = node[v];
      if (nv.stamp != gen) { nv.stamp = gen; nv.h = heuristic(v); }     // h(v) is fixed for the query: computed when v is first reached
      else if (!(gv < nv.g)) continue;
      nv.g = gv;
      if (nv.h == inf) { nv.closed = 1u; continue; }
      nv.parent = u; nv.parent_edge = e; nv.closed = 0u;
      heap.emplace_back(gv + nv.h, v);
      std::push_heap(heap.begin(), heap.end(), cmp);
    }
  }
  if (!found) return false;
  path.clear(); path_e.clear();
  for (int32_t v = goal;; v = node[v].parent) {
    path.push_back(v);
    if (v == start) break;
    path_e.push_back(node[v].parent_edge);
  }
  return true;
}

// The queries of tr_roadmap_solve_seeded: per query CSR lists of source seeds (u_i, c_i) and target seeds (v_j, d_j), an optional direct
// cost (+inf or no array: none), and the picks that come back (indices into the query's lists; -1: the direct connection, or no answer)
struct SeededQueries {
  const int64_t *src_off; const int32_t *src_v; const double *src_c;
  const int64_t *dst_off; const int32_t *dst_v; const double *dst_c;
  const double *direct;
  int32_t *src_pick, *dst_pick;
};

// astar from several weighted sources to several weighted targets: the sources enter the open list with g = c_i, a virtual goal record
// is relaxed with g(v_j) + d_j whenever a target vertex is expanded, and the search ends when the virtual goal leaves the open list --
// with min over i, j of c_i + dist(u_i, v_j) + d_j, summed left to right from the source as every g is.  The heuristic towards the
// virtual goal is min_j (h(v, v_j) + d_j) with GoalHeuristic's h (landmark terms included): admissible as each term is; vertices are
// opened again when their cost improves, as in astar.  Seeds whose vertex is known invalid are not seeds.  The direct connection wins
// when direct <= that minimum; the search stops as soon as nothing on the open list can beat it.  Returns false when there is no
// answer at all; a direct answer leaves path / path_e empty and the picks -1.  path: v_j ... u_i, path_e: the edges between them.
bool astar_seeded(const tr_roadmap *r, Scratch &sc, const SeededQueries &s, int64_t q, std::vector<int32_t> &path, std::vector<int32_t> &path_e,
                  int64_t &expanded) {
  if (sc.node.size() != (size_t)r->V) { sc.node.assign((size_t)r->V, Node{0.0, 0.0, -1, -1, 0u, 0u}); sc.gen = 0; }
  if (++sc.gen == 0) { for (Node &nd : sc.node) nd.stamp = 0u; sc.gen = 1; }
  Node *node = sc.node.data();
  const uint32_t gen = sc.gen;
  auto &heap = sc.heap;
  heap.clear();
  path.clear(); path_e.clear();
  s.src_pick[q] = s.dst_pick[q] = -1;
  const double inf = std::numeric_limits<double>::infinity();
  const double direct = s.direct ? s.direct[q] : inf;
  // the targets that count: per vertex its cheapest seed (the first of equal ones), ordered by vertex for the look-up at expansion
  // (the list lives with the thread: no allocation per query; a GoalHeuristic is four words of pointers into the roadmap, made where it is used)
  using Target = SeedTarget;
  auto &tg = sc.targets;
  tg.clear();
  for (int64_t j = s.dst_off[q]; j < s.dst_off[q + 1]; j++)
    if (r->vstat[(size_t)s.dst_v[j]] != V_INVALID) tg.push_back(Target{s.dst_v[j], s.dst_c[j], (int32_t)(j - s.dst_off[q])});
  std::sort(tg.begin(), tg.end(), [](const Target &a, const Target &b) { return a.v < b.v || (a.v == b.v && (a.d < b.d || (a.d == b.d && a.j < b.j))); });
  tg.erase(std::unique(tg.begin(), tg.end(), [](const Target &a, const Target &b) { return a.v == b.v; }), tg.end());
  auto heuristic = [&](int32_t v) {
    double h = inf;
    for (const Target &t : tg) { const double x = GoalHeuristic(r, t.v)(v) + t.d; h = x < h ? x : h; }
    return h;
  };
  auto cmp = [](const std::pair<double, int32_t> &a, const std::pair<double, int32_t> &b) { return a.first > b.first; };
  // the sources: parent = the vertex itself, parent_edge = -(seed index) - 2 (so the pick is read off the path's first record)
  for (int64_t i = s.src_off[q]; !tg.empty() && i < s.src_off[q + 1]; i++) {
    const int32_t u = s.src_v[i];
    if (r->vstat[(size_t)u] == V_INVALID) continue;
    Node &nu = node[u];
    if (nu.stamp != gen) { nu.stamp = gen; nu.h = heuristic(u); }
    else if (!(s.src_c[i] < nu.g)) continue;
    nu.g = s.src_c[i];
    nu.parent = u; nu.parent_edge = -(int32_t)(i - s.src_off[q]) - 2; nu.closed = 0u;
    if (nu.h == inf) { nu.closed = 1u; continue; }
    heap.emplace_back(nu.g + nu.h, u);
    std::push_heap(heap.begin(), heap.end(), cmp);
  }
  constexpr int32_t kGoal = -1;                  // the virtual goal on the open list
  double best = inf;                             // its g
  int32_t best_v = -1, best_j = -1;
  bool found = false;
  while (!heap.empty()) {
    std::pop_heap(heap.begin(), heap.end(), cmp);
    const double f = heap.back().first;
    const int32_t u = heap.back().second;
    heap.pop_back();
    if (f >= direct) break;                      // whatever is still open costs at least the direct connection
    if (u == kGoal) { if (f == best) { found = true; break; } continue; }
    if (node[u].closed) continue;
    node[u].closed = 1u;
    expanded++;
    const double gu = node[u].g;
    const auto t = std::lower_bound(tg.begin(), tg.end(), u, [](const Target &a, int32_t v) { return a.v < v; });
    if (t != tg.end() && t->v == u && gu + t->d < best) {
      best = gu + t->d; best_v = u; best_j = t->j;
      heap.emplace_back(best, kGoal);
      std::push_heap(heap.begin(), heap.end(), cmp);
    }
    for (const Arc *arc = r->adj.data() + r->adj_off[u], *end = r->adj.data() + r->adj_off[u + 1]; arc != end; ++arc) {
      const int32_t e = arc->e, v = arc->v;
      if (r->estat[e] == V_INVALID || r->vstat[v] == V_INVALID) continue;
      const double gv = gu + arc->w;
      Node &nv = node[v];
      if (nv.stamp != gen) { nv.stamp = gen; nv.h = heuristic(v); }
      else if (!(gv < nv.g)) continue;
      nv.g = gv;
      if (nv.h == inf) { nv.closed = 1u; continue; }
      nv.parent = u; nv.parent_edge = e; nv.closed = 0u;
      heap.emplace_back(gv + nv.h, v);
      std::push_heap(heap.begin(), heap.end(), cmp);
    }
  }
  if (!found) return direct < inf;
  // (the records behind best_v are those its g was summed over: a vertex on that chain whose cost improved later would have been
  // expanded again before the goal, and best with it)
  for (int32_t v = best_v;; v = node[v].parent) {
    path.push_back(v);
    if (node[v].parent_edge < -1) { s.src_pick[q] = -node[v].parent_edge - 2; break; }
    path_e.push_back(node[v].parent_edge);
  }
  s.dst_pick[q] = best_j;
  return true;
}

// One Dijkstra per landmark over ALL edges on the host threads: lm_d[v * L + l] = (float) graph distance landmark l -> v.
void landmark_distances_host(tr_roadmap *r, int T) {
  const int64_t V = r->V;
  const int L = (int)r->lm_v.size();
  std::atomic<int> next{0};
  auto worker = [&]() {
    std::vector<double> dist((size_t)V);
    std::vector<std::pair<double, int32_t>> heap;
    auto cmp = [](const std::pair<double, int32_t> &a, const std::pair<double, int32_t> &b) { return a.first > b.first; };
    for (;;) {
      const int l = next.fetch_add(1);
      if (l >= L) break;
      std::fill(dist.begin(), dist.end(), std::numeric_limits<double>::infinity());
      heap.clear();
      dist[(size_t)r->lm_v[(size_t)l]] = 0.0;
      heap.emplace_back(0.0, r->lm_v[(size_t)l]);
      while (!heap.empty()) {
        std::pop_heap(heap.begin(), heap.end(), cmp);
        const double du = heap.back().first;
        const int32_t u = heap.back().second;
        heap.pop_back();
        if (du > dist[(size_t)u]) continue;
        for (int64_t k = r->adj_off[u]; k < r->adj_off[u + 1]; k++) {
          const Arc &a = r->adj[(size_t)k];
          const double dv = du + a.w;
          if (dv < dist[(size_t)a.v]) { dist[(size_t)a.v] = dv; heap.emplace_back(dv, a.v); std::push_heap(heap.begin(), heap.end(), cmp); }
        }
      }
      for (int64_t v = 0; v < V; v++) r->lm_d[(size_t)v * L + l] = (float)dist[(size_t)v];
    }
  };
  on_threads(std::max(1, std::min(T, L)), [&](int) { worker(); });
}

bool landmark_distances_device(tr_roadmap *r) {
  const int64_t V = r->V;
  const int L = (int)r->lm_v.size();
  if (hipSetDevice(tr_device(r->ctx)) != hipSuccess) return false;
  constexpr int BATCH = 8;                                     // sweeps between two looks at the flags
  // one allocation: offsets | arcs | distances (as ordered bit patterns) | float table | landmark vertices | flags
  const size_t b_off = up((size_t)(V + 1) * sizeof(int64_t)), b_adj = up(std::max<size_t>(1, r->adj.size()) * sizeof(Arc)),
               b_dist = up((size_t)V * L * sizeof(unsigned long long)), b_out = up((size_t)V * L * sizeof(float)),
               b_lm = up((size_t)L * sizeof(int32_t)), b_flags = up(BATCH * sizeof(uint32_t));
  char *arena = nullptr;
  if (dev_cache().alloc(tr_device(r->ctx), (void **)&arena, b_off + b_adj + b_dist + b_out + b_lm + b_flags) != hipSuccess) return false;
  int64_t *d_off = (int64_t *)arena;
  Arc *d_adj = (Arc *)(arena + b_off);
  unsigned long long *d_dist = (unsigned long long *)(arena + b_off + b_adj);
  float *d_out = (float *)(arena + b_off + b_adj + b_dist);
  int32_t *d_lm = (int32_t *)(arena + b_off + b_adj + b_dist + b_out);
  uint32_t *d_changed = (uint32_t *)(arena + b_off + b_adj + b_dist + b_out + b_lm);
  const unsigned grid = (unsigned)((V * L + 255) / 256);
  bool ok = hipMemcpyAsync(d_lm, r->lm_v.data(), (size_t)L * sizeof(int32_t), hipMemcpyHostToDevice, nullptr) == hipSuccess;
  if (ok) {
    hipLaunchKernelGGL(landmark_init, dim3(grid), dim3(256), 0, nullptr, d_dist, V * L, d_lm, L);
    ok = hipGetLastError() == hipSuccess;
  }
  ok = ok && hipMemcpyAsync(d_off, r->adj_off.data(), (size_t)(V + 1) * sizeof(int64_t), hipMemcpyHostToDevice, nullptr) == hipSuccess &&
       hipMemcpyAsync(d_adj, r->adj.data(), r->adj.size() * sizeof(Arc), hipMemcpyHostToDevice, nullptr) == hipSuccess;
  bool converged = false;
  for (int64_t sweeps = 0; ok && !converged && sweeps < 4 * V + BATCH; sweeps += BATCH) {     // (V - 1 sweeps always suffice)
    uint32_t flags[BATCH];
    ok = hipMemsetAsync(d_changed, 0, BATCH * sizeof(uint32_t), nullptr) == hipSuccess;
    for (int b = 0; ok && b < BATCH; b++) {
      hipLaunchKernelGGL(landmark_relax, dim3(grid), dim3(256), 0, nullptr, d_off, d_adj, V, L, d_dist, d_changed + b);
      ok = hipGetLastError() == hipSuccess;
    }
    ok = ok && hipMemcpy(flags, d_changed, sizeof(flags), hipMemcpyDeviceToHost) == hipSuccess;
    for (int b = 0; ok && b < BATCH; b++) if (!flags[b]) converged = true;            // a sweep without a change: the fixed point
  }
  if (ok && converged) {
    hipLaunchKernelGGL(landmark_to_float, dim3(grid), dim3(256), 0, nullptr, d_dist, V * L, d_out);
    ok = hipGetLastError() == hipSuccess &&
         hipMemcpy(r->lm_d.data(), d_out, (size_t)V * L * sizeof(float), hipMemcpyDeviceToHost) == hipSuccess;
  }
  dev_cache().release(arena);
  return ok && converged;
}

// comp[v] = the smallest vertex of v's component, by union-find over the edge list on one host thread (sequential reads; the parent array
// stays in cache -- a graph traversal would take one cache miss per vertex into the 16-byte arcs; a few ms at 6 x 10^5 edges).
// valid_only: components of the roadmap minus the items known invalid.
void host_components(const tr_roadmap *r, bool valid_only, std::vector<int32_t> &comp) {
  comp.resize((size_t)r->V);
  for (int64_t v = 0; v < r->V; v++) comp[(size_t)v] = (int32_t)v;
  auto root = [&comp](int32_t x) {
    while (comp[(size_t)x] != x) { comp[(size_t)x] = comp[(size_t)comp[(size_t)x]]; x = comp[(size_t)x]; }     // path halving
    return x;
  };
  for (int64_t e = 0; e < r->E; e++) {
    const int32_t u = r->eu[(size_t)e], v = r->ev[(size_t)e];
    if (valid_only && (r->estat[(size_t)e] == V_INVALID || r->vstat[(size_t)u] == V_INVALID || r->vstat[(size_t)v] == V_INVALID)) continue;
    const int32_t a = root(u), b = root(v);
    if (a != b) comp[(size_t)std::max(a, b)] = std::min(a, b);          // the smaller index becomes the root
  }
  for (int64_t v = 0; v < r->V; v++) comp[(size_t)v] = root((int32_t)v);
}

// Landmark tables: n extremal vertices of the largest component (the corners of the sampled state box first, then fixed
// pseudo-random directions), one Dijkstra each over ALL edges -- validity plays no part, see the header comment.
void build_landmarks(tr_roadmap *r, int n, int T, const RoadmapSwitches &sw) {
  r->lm_d.clear(); r->lm_v.clear(); r->lm_n = 0; r->lm_mismatch = false;
  r->ds.lm_current = false;
  const int64_t V = r->V;
  const int S = r->S;
  if (n <= 0 || V < 2 || r->E == 0) return;
  Laps laps(sw, "build_landmarks");
  // largest connected component (ties: the smallest root)
  std::vector<int32_t> comp;
  host_components(r, false, comp);
  int32_t big = -1;
  int64_t big_n = 0;
  {
    std::vector<int32_t> cnt((size_t)V, 0);
    for (int64_t v = 0; v < V; v++) cnt[(size_t)comp[(size_t)v]]++;
    for (int64_t v = 0; v < V; v++) if (cnt[(size_t)v] > big_n) { big_n = cnt[(size_t)v]; big = (int32_t)v; }
  }
  if (big_n < 2) return;
  laps.lap("components");
  std::vector<double> lo((size_t)S, std::numeric_limits<double>::infinity()), hi((size_t)S, -std::numeric_limits<double>::infinity());
  for (int64_t v = 0; v < V; v++)
    for (int i = 0; i < S; i++) { const double x = r->states[(size_t)v * S + i]; lo[(size_t)i] = std::min(lo[(size_t)i], x); hi[(size_t)i] = std::max(hi[(size_t)i], x); }
  // the directions, in their fixed order; the vertex furthest along each of the first n on the host threads, any further one
  // (needed only when two directions pick the same vertex) when its turn comes
  std::vector<double> dirs((size_t)4 * n * S);
  {
    uint64_t lcg = 0x9E3779B97F4A7C15ull;
    for (int l = 0; l < 4 * n; l++)
      for (int i = 0; i < S; i++) {
        double c;
        if (S <= 16 && l < (1 << S)) c = ((l >> i) & 1) ? 1.0 : -1.0;
        else { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; c = (double)(int64_t)(lcg >> 11) / (double)(1ll << 52) - 1.0; }
        const double ext = hi[(size_t)i] - lo[(size_t)i];
        dirs[(size_t)l * S + i] = ext > 0 ? c / ext : 0.0;
      }
  }
  auto furthest = [&](int l) {
    const double *dir = &dirs[(size_t)l * S];
    int32_t arg = -1;
    double best = -std::numeric_limits<double>::infinity();
    for (int64_t v = 0; v < V; v++) {
      if (comp[(size_t)v] != big) continue;
      double d = 0;
      for (int i = 0; i < S; i++) d += dir[i] * r->states[(size_t)v * S + i];
      if (d > best) { best = d; arg = (int32_t)v; }
    }
    return arg;
  };
  std::vector<int32_t> first((size_t)n, -1);
  {
    const int Tn = std::max(1, std::min(T, n));
    on_threads(Tn, [&](int t) { for (int l = t; l < n; l += Tn) first[(size_t)l] = furthest(l); });
  }
  for (int l = 0; l < 4 * n && (int)r->lm_v.size() < n; l++) {
    const int32_t arg = l < n ? first[(size_t)l] : furthest(l);
    if (arg >= 0 && std::find(r->lm_v.begin(), r->lm_v.end(), arg) == r->lm_v.end()) r->lm_v.push_back(arg);
  }
  const int L = (int)r->lm_v.size();
  if (L == 0) return;
  laps.lap("extremal vertices");
  r->lm_d.assign((size_t)V * L, std::numeric_limits<float>::infinity());
  // the distances: on the device (landmark_distances_device), or L Dijkstras on the host threads (TENDON_HIP_LANDMARKS=host, or when
  // the device path fails); TENDON_HIP_LANDMARKS=check builds both and keeps the host's if they differ in any bit
  const bool host_only = sw.landmarks_host, check = sw.landmarks_check;
  bool done = false;
  if (!host_only) done = landmark_distances_device(r);
  laps.lap("distances");
  if (!done || check) {
    std::vector<float> dev;
    if (done) dev = r->lm_d;
    landmark_distances_host(r, T);
    if (done && check && std::memcmp(dev.data(), r->lm_d.data(), dev.size() * sizeof(float)) != 0) r->lm_mismatch = true;
  }
  for (float &x_ : r->lm_d) if (!(x_ < trk::SR_LM_FAR)) x_ = trk::SR_LM_FAR;
  r->lm_n = L;
}

}  // namespace
