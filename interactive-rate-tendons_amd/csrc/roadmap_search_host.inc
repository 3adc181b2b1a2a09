// roadmap_search_host.inc -- part of roadmap.hip: the graph searches on the device (search_kernel.hpp): set-up, tables, launch, collect, and the sweep.
namespace {

// The searches' tables and per-round arrays -- all of the search state that does not depend on the roadmap -- go back to the buffer
// cache; the adjacency rows stay, and the next large round allocates tables again (search_tables).  Caller holds r->mu.
size_t release_search_tables(tr_roadmap *r) {
  auto &d = r->ds;
  if (d.in_flight) return 0;
  size_t b = 0;
  if (d.tables) {
    dev_cache().release(d.tables);
    b += d.table_bytes;
    d.tables = nullptr; d.table_bytes = 0; d.slots = 0; d.gens_issued = 0;
    for (int c = 0; c < trk::SR_CLASSES; c++) { d.pool[c] = nullptr; d.pool_n[c] = 0; }
  }
  if (d.qarena) {
    dev_cache().release(d.qarena);
    b += (size_t)d.nq_cap * 17 + (size_t)d.pbuf_cap * 4;
    d.qarena = nullptr; d.nq_cap = 0; d.pbuf_cap = 0;
  }
  return b;
}

void free_search(tr_roadmap *r) {
  auto &d = r->ds;
  if (d.arena) dev_cache().release(d.arena);
  if (d.tables) dev_cache().release(d.tables);
  if (d.qarena) dev_cache().release(d.qarena);
  if (d.h_handback) (void)hipHostFree(d.h_handback);
  if (d.sweep_arena) dev_cache().release(d.sweep_arena);
  if (d.sweep_h_dist) (void)hipHostFree(d.sweep_h_dist);
  if (d.sweep_stream) (void)hipStreamDestroy(d.sweep_stream);
  for (hipEvent_t e : d.ev) if (e) (void)hipEventDestroy(e);
  d.~DevSearch();
  new (&d) tr_roadmap::DevSearch();
}

// ---- the graph searches on the device (search_kernel.hpp) ----
static_assert(sizeof(trk::SArc) == sizeof(Arc) && sizeof(trk::SRec) == 32, "the device's arcs are the host's; two records to a 64-byte line");

constexpr int64_t kSearchMinQueries = 512;                       // rounds of fewer queries stay on the host threads (unless TENDON_HIP_SEARCH=device)
constexpr int64_t kComponentMinQueries = 64;                     // rounds smaller than this are searched without component labels
constexpr int64_t kComponentTrigger = 2000;                      // expansions of a search that ends without a path, from which on labels pay

// The kernel for the roadmap's state size (the heuristic keeps SX coordinates in registers)
using SearchKernel = void (*)(trk::SearchArgs);
SearchKernel search_kernel_for(int S) { return S <= 4 ? trk::roadmap_astar<4> : S <= 8 ? trk::roadmap_astar<8> : trk::roadmap_astar<trk::SR_MAXS>; }

// The resident part: adjacency rows, states, landmark table, validity bytes -- what depends on the roadmap -- and the searches' own state,
// which does not: per wave slot a table of 2^lc0 records with its far list (44 B per record: 176 KiB at lc0 = 12), and a pool of larger
// tables (x 4 per class) that long searches move into.  The slot count is what the chip holds of this kernel (LDS: 9.8 KiB per wave).
//   TENDON_HIP_SEARCH_SLOTS=n     searches in flight (default: what the device holds)
//   TENDON_HIP_SEARCH_LC0=8..14   log2 of a slot's own table (default 12; tests: a small value makes every search grow)
//   TENDON_HIP_SEARCH_POOL=a,b,c  tables of the three larger classes (default slots, slots / 4, slots / 64 -- 5.3 GB with the slots' own at
//                                 3 072 slots: a 6 x 10^5-vertex roadmap's searches touch 10^4 - 10^5 vertices each; 0,0,0: every search that outgrows
//                                 its table is handed back to the host threads)
// pool tables per class for `slots` searches in flight (class 0: the slots' own)
void search_pool_counts(int64_t slots, int64_t pn[trk::SR_CLASSES], const RoadmapSwitches &sw) {
  pn[0] = 0; pn[1] = std::max<int64_t>(64, slots); pn[2] = std::max<int64_t>(16, slots / 4); pn[3] = std::max<int64_t>(8, slots / 64);
  if (sw.pool_set)
    for (int c = 1; c < trk::SR_CLASSES; c++) pn[c] = std::min<int64_t>(std::max<int64_t>(pn[c], (int64_t)1 << 16), std::max(0ll, sw.pool[c - 1]));
}
bool search_setup(tr_roadmap *r, const RoadmapSwitches &sw) {
  auto &d = r->ds;
  if (d.state != 0) return d.state > 0;
  d.state = -1;
  Laps laps(sw, "search_setup");
  const int64_t V = r->V;
  if (r->S > trk::SR_MAXS) { d.why = "state size above the kernel's"; return false; }
  if (V < 2 || r->adj.size() == 0) { d.why = "no graph"; return false; }
  if (V >= ((int64_t)1 << trk::SR_VBITS)) { d.why = "more vertices than an open-list word names"; return false; }
  // two arcs between the same pair of vertices would make two lanes relax the same record in one step: such roadmaps stay on the host
  {
    std::vector<int32_t> nb;
    for (int64_t v = 0; v < V; v++) {
      const int64_t a0 = r->adj_off[(size_t)v], a1 = r->adj_off[(size_t)v + 1];
      if (a1 - a0 < 2) continue;
      nb.clear();
      for (int64_t k = a0; k < a1; k++) nb.push_back(r->adj[(size_t)k].v);
      std::sort(nb.begin(), nb.end());
      if (std::adjacent_find(nb.begin(), nb.end()) != nb.end()) { d.why = "parallel edges"; return false; }
    }
  }
  laps.lap("parallel-edge check");
  // adjacency at a fixed stride: row v holds v's arcs (at most SR_D; unused slots marked); a vertex with more keeps SR_D - 1 in a
  // row whose last slot names its next row (rows V, V + 1, ... in vertex order)
  constexpr int D = trk::SR_D;
  int64_t n_rows = V;
  for (int64_t v = 0; v < V; v++) {
    int64_t deg = r->adj_off[(size_t)v + 1] - r->adj_off[(size_t)v];
    while (deg > D) { deg -= D - 1; n_rows++; }
  }
  if (n_rows > std::numeric_limits<int32_t>::max() / D) { d.why = "roadmap too large for the row index"; return false; }
  RawArray<trk::SArc> rows;
  rows.resize_uninit((size_t)n_rows * D);
  std::vector<uint8_t> lanes((size_t)V);                          // lanes a vertex's first row needs (an open-list word carries it)
  {
    int64_t next_row = V;
    for (int64_t v = 0; v < V; v++) {
      const Arc *arc = r->adj.data() + r->adj_off[(size_t)v];
      int64_t deg = r->adj_off[(size_t)v + 1] - r->adj_off[(size_t)v], row = v;
      lanes[(size_t)v] = (uint8_t)std::max<int64_t>(1, std::min<int64_t>(deg, D));
      for (;;) {
        trk::SArc *out = rows.data() + (size_t)row * D;
        const int take = deg > D ? D - 1 : (int)deg;
        for (int j = 0; j < take; j++) out[j] = trk::SArc{arc[j].v, arc[j].e, arc[j].w};        // (the neighbours' lane counts: second pass below)
        for (int j = take; j < D; j++) out[j] = trk::SArc{trk::SR_ARC_NONE, -1, 0.0};
        arc += take; deg -= take;
        if (deg == 0) break;
        out[D - 1] = trk::SArc{trk::SR_ARC_MORE, (int32_t)next_row, 0.0};
        row = next_row++;
      }
    }
  }
  for (size_t t = 0; t < (size_t)n_rows * D; t++) {                 // an arc's vertex word carries the lanes its neighbour's own row needs
    trk::SArc &x = rows[t];
    if (x.v >= 0) x.v |= (int32_t)lanes[(size_t)x.v] << trk::SR_VBITS;
  }
  laps.lap("adjacency rows");
  const int dev = tr_device(r->ctx);
  if (hipSetDevice(dev) != hipSuccess) { d.why = "hipSetDevice"; return false; }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, dev) != hipSuccess) { d.why = "hipGetDeviceProperties"; return false; }
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, search_kernel_for(r->S), 64, trk::search_lds_bytes()) != hipSuccess || per_cu < 1) {
    d.why = "occupancy query"; return false;
  }
  int64_t slots = (int64_t)per_cu * prop.multiProcessorCount;
  if (sw.slots > 0) slots = std::min<int64_t>(slots, sw.slots);
  d.max_slots = slots;
  d.lc0 = sw.lc0;
  {
    // control words: the counters, then the pool's claim bitmaps at their largest (search_tables lays them out per table set)
    int64_t pn[trk::SR_CLASSES];
    search_pool_counts(slots, pn, sw);
    int64_t word = trk::SR_CTL_WORDS;
    for (int c = 0; c < trk::SR_CLASSES; c++) word += (pn[c] + 31) / 32;
    d.ctl_bytes = ((size_t)word * 4 + 255) & ~(size_t)255;
  }
  const int Lmax = trk::SR_MAXL;
  const size_t b_rows = up((size_t)n_rows * D * sizeof(trk::SArc)), b_vr = up((size_t)V * trk::search_row_bytes(r->S, Lmax)),
               b_vs = up((size_t)V), b_es = up((size_t)std::max<int64_t>(r->E, 1));
  if (dev_cache().alloc(dev, (void **)&d.arena, b_rows + b_vr + 2 * b_vs + b_es + d.ctl_bytes) != hipSuccess) {
    d.why = "out of device memory"; return false;
  }
  char *p = d.arena;
  d.d_rows = (trk::SArc *)p; p += b_rows;
  d.d_vrows = p; p += b_vr;
  d.d_vstat = (uint8_t *)p; p += b_vs;
  d.d_estat = (uint8_t *)p; p += b_es;
  d.d_deg = (uint8_t *)p; p += b_vs;
  d.d_ctl = (uint32_t *)p;
  laps.lap("device properties + arena");
  const bool ok = hipMemcpyAsync(d.d_rows, rows.data(), (size_t)n_rows * D * sizeof(trk::SArc), hipMemcpyHostToDevice, nullptr) == hipSuccess &&
                  hipMemcpyAsync(d.d_deg, lanes.data(), (size_t)V, hipMemcpyHostToDevice, nullptr) == hipSuccess &&
                  hipStreamSynchronize(nullptr) == hipSuccess;
  laps.lap("graph uploaded");
  if (!ok) { free_search(r); r->ds.state = -1; r->ds.why = "out of device memory"; return false; }
  if (sw.stats)
    std::fprintf(stderr, "[tendon_hip] search graph: %lld rows of %d arcs (%lld continued), %.1f MiB\n", (long long)n_rows, D, (long long)(n_rows - V),
                 (double)(b_rows + b_vr + 2 * b_vs + b_es) / 1048576.0);
  d.lm_current = false;
  d.state = 1;
  return true;
}

// The tables of the searches in flight, sized by the round: `want` queries need min(want, max_slots) slots (in steps of 256, and at
// least twice what a smaller round left, so a caller whose rounds grow re-allocates a handful of times) and a pool in proportion.
// A 512-query round on a fresh roadmap holds ~0.9 GB, a 10 000-query round the device's full 3 072 slots (~5.3 GB); the state stays
// with the roadmap until tr_roadmap_release_search_state, the out-of-memory trim (release_idle_search_tables) or tr_roadmap_destroy.
bool search_tables(tr_roadmap *r, int64_t want, const RoadmapSwitches &sw) {
  auto &d = r->ds;
  int64_t slots = std::min<int64_t>(d.max_slots, std::max<int64_t>(256, (want + 255) & ~(int64_t)255));
  if (d.tables && d.slots >= slots) return true;
  if (d.tables) slots = std::max(slots, std::min<int64_t>(d.max_slots, 2 * d.slots));
  Laps laps(sw, "search_tables");
  const int dev = tr_device(r->ctx);
  if (d.tables) { dev_cache().release(d.tables); d.tables = nullptr; d.slots = 0; }
  int64_t pn[trk::SR_CLASSES];
  search_pool_counts(slots, pn, sw);
  // within a third of what is free: the pool shrinks first, then the slots
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { d.why = "hipMemGetInfo"; return false; }
  auto tables_bytes = [&](int64_t s_) {
    size_t b = (size_t)s_ * trk::search_chunk_bytes(d.lc0);
    for (int c = 1; c < trk::SR_CLASSES; c++) b += (size_t)pn[c] * trk::search_chunk_bytes(d.lc0 + 2 * c);
    return b;
  };
  for (int c = trk::SR_CLASSES - 1; c >= 1; c--)
    while (pn[c] > 0 && tables_bytes(slots) > free_b / 3) pn[c] /= 2;
  while (slots > 64 && tables_bytes(slots) > free_b / 3) slots /= 2;
  if (tables_bytes(slots) > free_b / 3) { d.why = "out of device memory"; return false; }
  int64_t word = trk::SR_CTL_WORDS;
  for (int c = 0; c < trk::SR_CLASSES; c++) { d.pool_n[c] = (int32_t)pn[c]; d.pool_word[c] = (int32_t)word; word += (pn[c] + 31) / 32; }
  if ((size_t)word * 4 > d.ctl_bytes) { d.why = "pool larger than the control words"; return false; }
  d.table_bytes = tables_bytes(slots);
  if (dev_cache().alloc(dev, (void **)&d.tables, d.table_bytes) != hipSuccess) { d.tables = nullptr; d.table_bytes = 0; d.why = "out of device memory"; return false; }
  char *q = d.tables + (size_t)slots * trk::search_chunk_bytes(d.lc0);
  for (int c = 1; c < trk::SR_CLASSES; c++) { d.pool[c] = q; q += (size_t)pn[c] * trk::search_chunk_bytes(d.lc0 + 2 * c); }
  laps.lap("tables allocated");
  // (generation 0 is nobody's: cleared once, never again until the generation counter would wrap)
  if (hipMemsetAsync(d.tables, 0, d.table_bytes, nullptr) != hipSuccess) {
    dev_cache().release(d.tables); d.tables = nullptr; d.table_bytes = 0; d.why = "hipMemsetAsync"; return false;
  }
  d.gens_issued = 0;
  d.slots = slots;
  laps.lap("tables cleared");
  if (sw.stats)
    std::fprintf(stderr, "[tendon_hip] search state: %lld slots x %zu KiB + pool %d / %d / %d tables = %.1f MiB (whatever the roadmap's size)\n",
                 (long long)slots, trk::search_chunk_bytes(d.lc0) >> 10, d.pool_n[1], d.pool_n[2], d.pool_n[3], (double)d.table_bytes / 1048576.0);
  return true;
}

// 1: path found (path: goal ... start, path_e: the edges between them, as astar leaves them), 0: no path, -1: not available (the caller
// searches on).  Serialised per roadmap (one arena); runs on a stream of its own beside the searches' kernel.
int sweep_search(tr_roadmap *r, int32_t start, int32_t goal, std::vector<int32_t> &path, std::vector<int32_t> &path_e) {
  auto &d = r->ds;
  std::lock_guard<std::mutex> lk(d.sweep_mu);
  if (d.state != 1 || !d.d_rows) return -1;
  const int64_t V = r->V, E = r->E;
  if (hipSetDevice(tr_device(r->ctx)) != hipSuccess) return -1;
  constexpr int BATCH = 8;
  const size_t b_dist = up((size_t)V * 8), b_vs = up((size_t)V), b_es = up((size_t)std::max<int64_t>(E, 1));
  if (!d.sweep_stream && hipStreamCreateWithFlags(&d.sweep_stream, hipStreamNonBlocking) != hipSuccess) { d.sweep_stream = nullptr; return -1; }
  if (!d.sweep_arena && dev_cache().alloc(tr_device(r->ctx), (void **)&d.sweep_arena, b_dist + b_vs + b_es + 256) != hipSuccess) { d.sweep_arena = nullptr; return -1; }
  if (!d.sweep_h_dist && hipHostMalloc((void **)&d.sweep_h_dist, (size_t)V * 8, hipHostMallocDefault) != hipSuccess) { d.sweep_h_dist = nullptr; return -1; }
  unsigned long long *d_dist = (unsigned long long *)d.sweep_arena;
  uint8_t *d_vs = (uint8_t *)(d.sweep_arena + b_dist), *d_es = d_vs + b_vs;
  uint32_t *d_changed = (uint32_t *)(d.sweep_arena + b_dist + b_vs + b_es);
  hipStream_t st = d.sweep_stream;
  bool ok = true;
  if (d.sweep_round != r->st_rounds) {                          // the round's validity bytes (they do not change inside a round)
    ok = hipMemcpyAsync(d_vs, r->vstat.data(), (size_t)V, hipMemcpyHostToDevice, st) == hipSuccess &&
         (E == 0 || hipMemcpyAsync(d_es, r->estat.data(), (size_t)E, hipMemcpyHostToDevice, st) == hipSuccess);
    if (ok) d.sweep_round = r->st_rounds;
  }
  const unsigned grid = (unsigned)((V + 255) / 256);
  if (ok) { hipLaunchKernelGGL(sweep_init, dim3(grid), dim3(256), 0, st, d_dist, V, start); ok = hipGetLastError() == hipSuccess; }
  bool converged = false;
  for (int64_t sweeps = 0; ok && !converged && sweeps < V + BATCH; sweeps += BATCH) {
    uint32_t flags[BATCH];
    ok = hipMemsetAsync(d_changed, 0, BATCH * sizeof(uint32_t), st) == hipSuccess;
    for (int b = 0; ok && b < BATCH; b++) {
      hipLaunchKernelGGL(sweep_relax, dim3(grid), dim3(256), 0, st, (const trk::SArc *)d.d_rows, (int)trk::SR_D, (const uint8_t *)d_vs, (const uint8_t *)d_es, V, goal,
                         d_dist, d_changed + b);
      ok = hipGetLastError() == hipSuccess;
    }
    ok = ok && hipMemcpyAsync(flags, d_changed, sizeof(flags), hipMemcpyDeviceToHost, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess;
    for (int b = 0; ok && b < BATCH; b++) if (!flags[b]) converged = true;
  }
  ok = ok && converged && hipMemcpyAsync(d.sweep_h_dist, d_dist, (size_t)V * 8, hipMemcpyDeviceToHost, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess;
  if (!ok) { d.sweep_round = -1; return -1; }
  const unsigned long long *dist = d.sweep_h_dist;
  const unsigned long long inf_b = 0x7FF0000000000000ull;
  if (dist[goal] >= inf_b) return 0;
  path.clear(); path_e.clear();
  int32_t v = goal;
  for (int64_t guard = 0; guard <= V; guard++) {
    path.push_back(v);
    if (v == start) { d.st_sweeps++; return 1; }
    const double dv = __builtin_bit_cast(double, dist[v]);
    const Arc *arc = r->adj.data() + r->adj_off[(size_t)v], *end = r->adj.data() + r->adj_off[(size_t)v + 1];
    const Arc *pick = nullptr;
    for (; arc != end; ++arc) {
      if (r->estat[(size_t)arc->e] == V_INVALID || r->vstat[(size_t)arc->v] == V_INVALID) continue;
      const unsigned long long bu = dist[arc->v];
      if (bu >= inf_b) continue;
      if (__builtin_bit_cast(double, bu) + arc->w == dv && bu < dist[v]) { pick = arc; break; }
    }
    if (!pick) break;                                           // (cannot happen at a fixed point; the caller searches on)
    path_e.push_back(pick->e);
    v = pick->v;
  }
  path.clear(); path_e.clear();
  return -1;
}

// expansions after which a host search is given to sweep_search (0: never): a sixth of the graph, 50 000 at least (well above the kernel's
// budget: what comes back over that is still a core's work); TENDON_HIP_SEARCH_SWEEP=n
// overrides (tests: a small n sends most searches that way), =0 switches it off
int64_t sweep_cap(const tr_roadmap *r, const RoadmapSwitches &sw) {
  if (sw.sweep_cap >= 0) return sw.sweep_cap;
  return r->ds.state == 1 ? std::max<int64_t>(50000, r->V / 6) : 0;
}

// One round's searches in two halves, so that the host threads can search their share while the kernel runs.
// device_search_launch: the queries active[klist[.]], in that order (the caller puts the ones it expects to be long first), are sent
// to the kernel; nothing is waited for.  `budget` caps the pops of one search (0: no cap): a search that reaches it is handed back.
// Returns false when the device cannot take the round (the caller then searches everything on the host).
// device_search_collect: waits for the kernel and leaves found[k] / paths / paths_e as the host search would; the queries the
// kernel gave up on (SR_FALLBACK) are listed in `redo`.
bool device_search_launch(tr_roadmap *r, const int32_t *starts, const int32_t *goals, const std::vector<int64_t> &active,
                          const std::vector<size_t> &klist, int64_t budget, const RoadmapSwitches &sw) {
  if (!search_setup(r, sw)) return false;
  auto &d = r->ds;
  const int dev = tr_device(r->ctx);
  const int64_t nq = (int64_t)klist.size(), V = r->V;
  if (nq == 0) return false;
  if (!search_tables(r, nq, sw)) return false;
  const int L = r->lm_n > 0 ? r->lm_n : 0;
  if (L > trk::SR_MAXL) return false;
  if (nq > d.nq_cap) {
    if (d.qarena) dev_cache().release(d.qarena);
    d.qarena = nullptr;
    d.nq_cap = std::max<int64_t>(nq, 1024);
    d.pbuf_cap = (uint32_t)std::min<int64_t>((int64_t)d.nq_cap * 256, (int64_t)1 << 28);
    const size_t bq = up((size_t)d.nq_cap * 4);
    if (dev_cache().alloc(dev, (void **)&d.qarena, 4 * bq + up((size_t)d.nq_cap) + (size_t)d.pbuf_cap * 4) != hipSuccess) { d.nq_cap = 0; return false; }
    char *p = d.qarena;
    d.d_qs = (int32_t *)p; p += bq;
    d.d_qg = (int32_t *)p; p += bq;
    d.d_poff = (int32_t *)p; p += bq;
    d.d_plen = (int32_t *)p; p += bq;
    d.d_found = (uint8_t *)p; p += up((size_t)d.nq_cap);
    d.d_pbuf = (int32_t *)p;
  }
  if (nq > d.handback_cap) {
    if (d.h_handback) (void)hipHostFree(d.h_handback);
    d.h_handback = nullptr; d.d_handback = nullptr; d.handback_cap = 0;
    const int64_t cap = std::max<int64_t>(nq, 4096);
    if (hipHostMalloc((void **)&d.h_handback, (size_t)cap * sizeof(uint32_t), hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess &&
        hipHostGetDevicePointer((void **)&d.d_handback, d.h_handback, 0) == hipSuccess) d.handback_cap = cap;
    else { if (d.h_handback) (void)hipHostFree(d.h_handback); d.h_handback = nullptr; d.d_handback = nullptr; }
  }
  if (d.h_handback) std::memset(d.h_handback, 0, (size_t)nq * sizeof(uint32_t));
  if (d.gens_issued + (uint64_t)nq >= ((uint64_t)1 << 31) - 2) {     // (a generation may not come round again while its records could be met)
    if (hipMemsetAsync(d.tables, 0, d.table_bytes, nullptr) != hipSuccess) return false;
    d.gens_issued = 0;
  }
  const uint32_t gen_base = (uint32_t)d.gens_issued;
  d.gens_issued += (uint64_t)nq;
  std::vector<int32_t> &qs = d.h_qs, &qg = d.h_qg;                  // (members: the copies below may still be reading them when this returns)
  qs.resize((size_t)nq); qg.resize((size_t)nq);
  for (int64_t j = 0; j < nq; j++) { qs[(size_t)j] = starts[active[klist[(size_t)j]]]; qg[(size_t)j] = goals[active[klist[(size_t)j]]]; }
  bool ok = true;
  if (!d.lm_current) {
    // the vertices' rows: state | landmark distances (padded to a multiple of four floats with zeros, which bound nothing)
    d.row_bytes = trk::search_row_bytes(r->S, L);
    const int lm_off = trk::search_lm_offset(r->S);
    std::vector<char> &rows = d.h_vrows;                          // (a member: the copy below may still be reading it when this returns)
    rows.assign((size_t)V * d.row_bytes, 0);
    for (int64_t v = 0; v < V; v++) {
      char *row = rows.data() + (size_t)v * d.row_bytes;
      std::memcpy(row, &r->states[(size_t)v * r->S], (size_t)r->S * 8);
      if (L) {
        float *lm = (float *)(row + lm_off);
        for (int l = 0; l < L; l++) { const float x = r->lm_d[(size_t)v * L + l]; lm[l] = x < trk::SR_LM_FAR ? x : trk::SR_LM_FAR; }   // (+inf: see the kernel's heuristic)
      }
    }
    ok = hipMemcpyAsync(d.d_vrows, rows.data(), rows.size(), hipMemcpyHostToDevice, nullptr) == hipSuccess;
    if (!ok) return false;
    d.lm_current = true;
  }
  const bool shared_status = r->dc.status_current;               // this round's validity bytes are in HBM already (component_labels)
  ok = ok && (shared_status || (hipMemcpyAsync(d.d_vstat, r->vstat.data(), (size_t)V, hipMemcpyHostToDevice, nullptr) == hipSuccess &&
       (r->E == 0 || hipMemcpyAsync(d.d_estat, r->estat.data(), (size_t)r->E, hipMemcpyHostToDevice, nullptr) == hipSuccess))) &&
       hipMemcpyAsync(d.d_qs, qs.data(), (size_t)nq * 4, hipMemcpyHostToDevice, nullptr) == hipSuccess &&
       hipMemcpyAsync(d.d_qg, qg.data(), (size_t)nq * 4, hipMemcpyHostToDevice, nullptr) == hipSuccess &&
       hipMemsetAsync(d.d_ctl, 0, d.ctl_bytes, nullptr) == hipSuccess &&
       hipMemsetAsync(d.d_ctl + 40, 0xff, 8, nullptr) == hipSuccess;       // (a -DTRK_SEARCH_CLOCKS build keeps the first wave's start there)
  if (!ok) return false;
  trk::SearchArgs a{};
  a.rows = d.d_rows; a.states = (const double *)d.d_vrows; a.lm = L ? (const float *)(d.d_vrows + trk::search_lm_offset(r->S)) : nullptr;
  a.row_bytes = d.row_bytes;
  a.S = r->S; a.NT = r->NT; a.rot = r->rot; a.ret = r->ret; a.L = L;
  a.w_rot = r->w_rot; a.w_ret = r->w_ret; a.lm_slack = kLmSlack;
  a.vstat = shared_status ? r->dc.d_vstat : d.d_vstat; a.estat = shared_status ? r->dc.d_estat : d.d_estat; a.deg = d.d_deg; a.V = V; a.E = r->E;
  a.qs = d.d_qs; a.qg = d.d_qg; a.nq = nq;
  a.next = d.d_ctl; a.pbuf_used = d.d_ctl + 1; a.expanded = (unsigned long long *)(d.d_ctl + 2);
  a.base = d.tables; a.lc0 = d.lc0; a.gen_base = gen_base;
  for (int c = 0; c < trk::SR_CLASSES; c++) { a.pool[c] = d.pool[c]; a.pool_n[c] = d.pool_n[c]; a.pool_word[c] = d.pool_word[c]; }
  a.found = d.d_found; a.poff = d.d_poff; a.plen = d.d_plen; a.pbuf = d.d_pbuf; a.pbuf_cap = d.pbuf_cap;
  a.handback = d.handback_cap >= nq ? d.d_handback : nullptr;
  a.max_pops = budget > 0 ? budget : 16 * V + 1024;             // (uncapped: every vertex reopened a few times, far beyond what a search does)
  a.kbest = sw.kbest;
  const unsigned grid = (unsigned)std::min<int64_t>(d.slots, nq);
  if (!d.ev[0] && (hipEventCreate(&d.ev[0]) != hipSuccess || hipEventCreate(&d.ev[1]) != hipSuccess)) { d.ev[0] = d.ev[1] = nullptr; }
  if (d.ev[0]) (void)hipEventRecord(d.ev[0], nullptr);
  hipLaunchKernelGGL(search_kernel_for(r->S), dim3(grid), dim3(64), trk::search_lds_bytes(), nullptr, a);
  if (hipGetLastError() != hipSuccess) return false;
  if (d.ev[0]) { (void)hipEventRecord(d.ev[1], nullptr); d.ev_pending = true; }
  d.in_flight = nq;
  return true;
}

// TENDON_HIP_SEARCH_STATS: what the kernel's own clocks say of a launch (the words are non-zero only in a -DTRK_SEARCH_CLOCKS build)
void report_search_clocks(const uint32_t ctl[136]) {
  unsigned long long c[7];
  std::memcpy(c, &ctl[16], sizeof(c));
  const double tot = (double)(c[0] + c[1] + c[2] + c[3] + c[4]);
  unsigned long long sp[2];
  std::memcpy(sp, &ctl[32], sizeof(sp));
  if (tot > 0) std::fprintf(stderr, "[tendon_hip] search steps: %llu steps, %llu passes, %.2f us per step\n", sp[0], sp[1], sp[0] ? tot * 1e-2 / (double)sp[0] : 0.0);
  if (tot > 0) {
    unsigned long long rx[3];
    std::memcpy(rx, &ctl[124], sizeof(rx));
    std::fprintf(stderr, "[tendon_hip] inside arcs + rows + relax: loads + heuristic + lookup %.1f%%, conflicts %.1f%%, claims + writes %.1f%% (of all)\n",
                 100.0 * rx[0] / tot, 100.0 * rx[1] / tot, 100.0 * rx[2] / tot);
    std::fprintf(stderr, "[tendon_hip] searches ended per 2 ms (count/expansions):");
    for (int b = 0; b < 40; b++) if (ctl[44 + b]) std::fprintf(stderr, " %d:%u/%u", 2 * b, ctl[44 + b], ctl[84 + b]);
    std::fprintf(stderr, "\n");
  }
  if (tot > 0)
    std::fprintf(stderr, "[tendon_hip] search clocks: %.1f wave-ms in all (longest search %.2f ms): refill %.1f%%, pop %.1f%%, record + offsets %.1f%%, arcs + rows + relax %.1f%%, append %.1f%%\n",
                 tot * 1e-5, (double)c[6] * 1e-5, 100.0 * c[0] / tot, 100.0 * c[1] / tot, 100.0 * c[2] / tot, 100.0 * c[3] / tot, 100.0 * c[4] / tot);
}

void device_search_collect(tr_roadmap *r, const std::vector<int64_t> &active, const std::vector<size_t> &klist,
                           std::vector<uint8_t> &found, std::vector<std::vector<int32_t>> &paths,
                           std::vector<std::vector<int32_t>> &paths_e, std::vector<size_t> &redo, int64_t &expanded, int T,
                           const RoadmapSwitches &sw, const std::vector<uint8_t> *handled = nullptr) {
  auto &d = r->ds;
  const int64_t nq = d.in_flight;
  d.in_flight = 0;
  // (any failure: the whole list goes back to the host threads)
  // (`handled`: positions the host threads have searched already -- handed back while the kernel ran: their answers stand)
  auto give_back = [&]() { redo.clear(); for (size_t k : klist) if (!handled || !(*handled)[k]) { redo.push_back(k); found[k] = 0; } };
  redo.clear();
  if (nq != (int64_t)klist.size()) { give_back(); return; }
  bool ok = true;
  std::vector<uint8_t> res((size_t)nq);
  std::vector<int32_t> poff((size_t)nq), plen((size_t)nq);
  uint32_t ctl[136] = {0};
  ok = hipMemcpy(ctl, d.d_ctl, sizeof(ctl), hipMemcpyDeviceToHost) == hipSuccess &&
       hipMemcpy(res.data(), d.d_found, (size_t)nq, hipMemcpyDeviceToHost) == hipSuccess &&
       hipMemcpy(poff.data(), d.d_poff, (size_t)nq * 4, hipMemcpyDeviceToHost) == hipSuccess &&
       hipMemcpy(plen.data(), d.d_plen, (size_t)nq * 4, hipMemcpyDeviceToHost) == hipSuccess;
  if (!ok) { give_back(); return; }
  if (d.ev_pending) {
    float ms_ = 0.0f;
    if (hipEventElapsedTime(&ms_, d.ev[0], d.ev[1]) == hipSuccess) { d.st_kernel_ms += (double)ms_; d.st_launches++; }
    d.ev_pending = false;
  }
  if (sw.stats) report_search_clocks(ctl);
  const uint32_t used = std::min(ctl[1], d.pbuf_cap);
  std::vector<int32_t> pbuf((size_t)used);
  if (used && hipMemcpy(pbuf.data(), d.d_pbuf, (size_t)used * 4, hipMemcpyDeviceToHost) != hipSuccess) { give_back(); return; }
  unsigned long long ex = 0;
  std::memcpy(&ex, &ctl[2], sizeof(ex));
  expanded += (int64_t)ex;
  d.st_expanded += (int64_t)ex;
  const int Tb = nq >= 2048 ? std::max(1, std::min(T, 16)) : 1;            // (ten thousand small vectors: by ranges on the host threads)
  std::vector<std::vector<size_t>> part((size_t)Tb);
  std::vector<int64_t> nfb((size_t)Tb, 0);
  on_threads(Tb, [&](int t) {
    const int64_t j0 = nq * t / Tb, j1 = nq * (t + 1) / Tb;
    for (int64_t j = j0; j < j1; j++) {
      const size_t k = klist[(size_t)j];
      const int64_t q = active[k];
      if (res[(size_t)j] == trk::SR_FALLBACK) nfb[(size_t)t]++;
      if (handled && (*handled)[k]) continue;
      found[k] = 0;
      if (res[(size_t)j] == trk::SR_FALLBACK) { part[(size_t)t].push_back(k); continue; }
      if (res[(size_t)j] != trk::SR_FOUND) continue;
      const int32_t n = plen[(size_t)j], o = poff[(size_t)j];
      if (n < 1 || o < 0 || (uint64_t)o + (uint64_t)(2 * n - 1) > used) { part[(size_t)t].push_back(k); continue; }
      paths[(size_t)q].assign(pbuf.begin() + o, pbuf.begin() + o + n);
      paths_e[(size_t)q].assign(pbuf.begin() + o + n, pbuf.begin() + o + 2 * n - 1);
      found[k] = 1;
    }
  });
  for (const auto &p : part) redo.insert(redo.end(), p.begin(), p.end());
  int64_t n_fb = 0;
  for (int64_t x : nfb) n_fb += x;
  n_fb = std::max<int64_t>(n_fb, (int64_t)redo.size());          // (a path that did not fit its buffer comes back too)
  d.st_queries += nq - n_fb; d.st_fallbacks += n_fb; d.st_moves += (int64_t)ctl[4];
  d.st_grows += (int64_t)ctl[5]; d.st_max_records = std::max<int64_t>(d.st_max_records, (int64_t)ctl[6]);
}

}  // namespace
