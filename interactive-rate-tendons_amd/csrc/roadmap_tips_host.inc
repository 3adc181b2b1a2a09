// roadmap_tips_host.inc -- part of roadmap.hip: batched tip-goal queries.  The reference's interactive loop
// (apps/roadmap_chained_plan.cpp:535-679) asks per waypoint roadmapIk(goal_tip, tol, k, opts)
// (motion-planning/VoxelCachedLazyPRM.cpp:3095-3577) and then solveWithRoadmap; here a batch of requests goes through
//   tip_knn (the k nearest tips among the valid vertices) -> tipq_gather -> ONE tr_ik_batch_dev of Q k problems ->
//   checkMotion(states[N], x, last_valid) on all of them -> tipq_interp + tr_fk_tips_dev -> tipq_select -> tr_roadmap_solve
// with the roadmap's tips, states and validity bytes resident in HBM: nothing V-sized moves per call (the validity bytes are
// sent again only after they changed on the host).  A result joins the roadmap through exactly one edge, to the neighbour IK
// started from (:3242-3244, :3276-3287); the graph itself is not edited.  The accurate rule (RMAP_IK_ACCURATE: the *_connect entry
// points) tries an edge from every state-space neighbour of the IK answer as well (:3237-3244): state_knn on the IK answers ->
// tipq_pair_rows -> ONE last-valid edge check of all the pairs -> tipq_interp + tr_fk_tips_dev on the pairs -> tipq_select_pairs.
// On LOADED shapes (the *_loaded entry points; with general_shape installed roadmapIk takes every shape from voxelStateChecker_->fk,
// :3052, :3187) the same body runs with a TipLoaded evaluator at the three places that differ: ONE tr_ik_loaded_batch_dev ->
// ONE tr_validate_edges_loaded with last_valid_t -> tipql_live_rows + tr_fk_loaded_tips_dev + tipql_scatter -> tipql_select
// (tipq_loaded_kernel.hpp), every solve cold.
namespace {

void free_tips(tr_roadmap *r) {
  auto &d = r->dt;
  void *p[] = {d.d_tips, d.d_states, d.d_soa, d.d_vstat, d.d_present, d.arena, d.d_ext};
  for (void *q : p) if (q) dev_cache().release(q);
  d = tr_roadmap::DevTips{};
}

// Vertex validity the nearest-tips filter needs: while a vertex is still unknown, every vertex's cached set is tested against the
// current grid in one K4 launch (the vertex part of tr_roadmap_revalidate: same kernel, same rule -- a hit or a missing cache is
// invalid) and the unknown ones become known; known ones keep what they have.  Then the device image follows `vstat`.
int tips_validity(tr_roadmap *r) {
  auto &d = r->dt;
  const int64_t V = r->V;
  bool unknown = false;
  for (int64_t v = 0; v < V && !unknown; v++) unknown = r->vstat[(size_t)v] == V_UNKNOWN;
  if (unknown) {
    if (!r->has_caches) return rfail(r, TR_ERR_INVALID_ARG, "vertices of unknown validity and no voxel caches attached (tr_roadmap_set_caches)");
    const int rc = tr_check_cached_dev(r->ctx, r->d_ids, r->d_masks, r->d_off, V, r->d_bits, nullptr);
    if (rc) return rfail(r, rc, tr_last_error(r->ctx));
    const size_t nw = (size_t)(V + 63) / 64;
    RM_HIP(r, hipMemcpyAsync(r->h_bits, r->d_bits, nw * sizeof(uint64_t), hipMemcpyDeviceToHost, nullptr));
    RM_HIP(r, hipStreamSynchronize(nullptr));
    for (int64_t v = 0; v < V; v++) {
      if (r->vstat[(size_t)v] != V_UNKNOWN) continue;
      const bool bad = ((r->h_bits[(size_t)v >> 6] | r->absent[(size_t)v >> 6]) >> (v & 63)) & 1;
      r->vstat[(size_t)v] = bad ? V_INVALID : V_VALID;
    }
  }
  if (d.vstat_sent != r->vstat) {
    RM_HIP(r, hipMemcpy(d.d_vstat, r->vstat.data(), (size_t)V, hipMemcpyHostToDevice));
    d.vstat_sent = r->vstat;
  }
  return TR_OK;
}

// the arena of one call, carved in order
struct TipArena {
  char *base = nullptr;
  size_t used = 0;
  template <class T> T *take(size_t n) { T *p = (T *)(base ? base + used : nullptr); used += up(std::max<size_t>(n, 1) * sizeof(T)); return p; }
};

struct TipBuffers {
  double *req, *d2, *part_d2, *starts, *goals, *x, *xtip, *err, *t, *g, *gtip, *o_controls, *o_tip, *o_err, *o_t;
  int32_t *nbr, *part_idx, *o_nbr, *o_outcome;
  uint8_t *ok;
  // the accurate rule (kc > 0): the source table C (m x kc) and its slices, and per pair (m (kc + 1) of them) the source vertex and
  // the two end rows; t / ok / g / gtip are per pair then
  int32_t *cidx, *c_part_idx, *src, *o_ik;
  double *c_part_d, *pa, *pb;
  uint8_t *o_flags;
  void carve(TipArena &a, int64_t n, int k, int S, int slices, bool full, int kc = 0, int c_slices = 1) {
    const size_t m = (size_t)n * (size_t)k, mp = m * (size_t)(kc > 0 ? kc + 1 : 1);
    req = a.take<double>((size_t)n * 3); nbr = a.take<int32_t>(m); d2 = a.take<double>(m);
    part_idx = a.take<int32_t>(slices > 1 ? m * (size_t)slices : 1); part_d2 = a.take<double>(slices > 1 ? m * (size_t)slices : 1);
    if (!full) return;
    starts = a.take<double>(m * S); goals = a.take<double>(m * 3); x = a.take<double>(m * S); xtip = a.take<double>(m * 3);
    err = a.take<double>(m); t = a.take<double>(mp); ok = a.take<uint8_t>(mp); g = a.take<double>(mp * S); gtip = a.take<double>(mp * 3);
    o_controls = a.take<double>((size_t)n * S); o_tip = a.take<double>((size_t)n * 3); o_err = a.take<double>((size_t)n);
    o_t = a.take<double>((size_t)n); o_nbr = a.take<int32_t>((size_t)n); o_outcome = a.take<int32_t>((size_t)n);
    if (kc <= 0) return;
    const size_t mc = m * (size_t)kc;
    cidx = a.take<int32_t>(mc);
    c_part_idx = a.take<int32_t>(c_slices > 1 ? mc * (size_t)c_slices : 1); c_part_d = a.take<double>(c_slices > 1 ? mc * (size_t)c_slices : 1);
    src = a.take<int32_t>(mp); pa = a.take<double>(mp * S); pb = a.take<double>(mp * S);
    o_ik = a.take<int32_t>((size_t)n); o_flags = a.take<uint8_t>((size_t)n);
  }
};

// what the loaded calls (tr_roadmap_ik_batch_loaded ...) keep beside TipBuffers: per slot the IK's equilibrium flag, strains and
// integrations; per pair the g solve's converged flag and strains; the dense arrays of the live pairs (rows, never planes); outputs
struct LoadedTipBuffers {
  uint8_t *eq, *gconv, *convc, *o_flags;
  int32_t *fkc, *live, *o_ik;
  double *xvu, *gvu, *gl, *gw, *gd, *tipc, *vuc, *o_vu;
  void carve(TipArena &a, int64_t n, int k, int S, int kc) {
    const size_t m = (size_t)n * (size_t)k, mp = m * (size_t)(kc > 0 ? kc + 1 : 1);
    eq = a.take<uint8_t>(m); fkc = a.take<int32_t>(m); xvu = a.take<double>(m * 6);
    gconv = a.take<uint8_t>(mp); gvu = a.take<double>(mp * 6); live = a.take<int32_t>(mp);
    gl = a.take<double>(mp * S); gw = a.take<double>(mp * 6); gd = a.take<double>(mp * 6);
    tipc = a.take<double>(mp * 3); convc = a.take<uint8_t>(mp); vuc = a.take<double>(mp * 6);
    o_vu = a.take<double>((size_t)n * 6); o_ik = a.take<int32_t>((size_t)n); o_flags = a.take<uint8_t>((size_t)n);
  }
};

// The evaluator of the three places where the loaded rules differ (the IK batch, the pair check, the tips of g): null = the unloaded
// rules with their launches, order and bits.  One load set per call; every solve is cold.
struct TipLoaded {
  const tr_shoot_params *shoot;
  tr_edge_loads loads;                  // warm_start = 0
  trk::TipqLoadsK k;                    // the same set as the kernels take it
  double *vu0;                          // optional outputs
  int64_t *counts;
};

constexpr int kTipQ = 4, kTipG = 4;     // requests per wave, tiles in flight (tip_knn)

// Slices of the tip array: a batch that fills the device with request groups streams it whole; a handful of requests cuts it so
// that ~1024 waves share the work (one wave alone would take V / 256 dependent rounds of loads).
int knn_slices(int64_t n, int64_t V, int Q, int G) {
  const int64_t groups = (n + Q - 1) / Q, tiles = (V + 63) / 64;
  const int64_t by_work = std::max<int64_t>(1, tiles / (2 * G));
  return (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(64, by_work), 1024 / groups));
}

int tip_slices(int64_t n, int64_t V) { return knn_slices(n, V, kTipQ, kTipG); }
// ... and of the vertex array for state_knn, whose Q and G follow the state size
int state_slices(const tr_roadmap *r, int64_t n) { return knn_slices(n, r->V, trk::stateq_q(r->S), trk::stateq_g(r->S)); }

// the call's arena holds at least `bytes`
int tip_arena(tr_roadmap *r, size_t bytes) {
  auto &d = r->dt;
  if (bytes > d.arena_bytes) {
    if (d.arena) dev_cache().release(d.arena);
    d.arena = nullptr; d.arena_bytes = 0;
    const size_t want = bytes + bytes / 2;
    RM_HIP(r, dev_cache().alloc(tr_device(r->ctx), (void **)&d.arena, want));
    d.arena_bytes = want;
  }
  return TR_OK;
}

int tip_buffers(tr_roadmap *r, int64_t n, int k, bool full, TipBuffers &b, int &slices, int kc = 0, int *c_slices = nullptr,
                LoadedTipBuffers *lb = nullptr) {
  slices = tip_slices(n, r->V);
  const int cs = kc > 0 ? state_slices(r, n * k) : 1;
  if (c_slices) *c_slices = cs;
  TipArena size;
  TipBuffers dummy;
  dummy.carve(size, n, k, r->S, slices, full, kc, cs);
  if (lb) { LoadedTipBuffers dl; dl.carve(size, n, k, r->S, kc); }
  if (const int rc = tip_arena(r, size.used)) return rc;
  TipArena a;
  a.base = r->dt.arena;
  b.carve(a, n, k, r->S, slices, full, kc, cs);
  if (lb) lb->carve(a, n, k, r->S, kc);
  return TR_OK;
}

// the arrays of tr_roadmap_nearest_states, from the same arena
struct StateBuffers {
  double *qry, *dist, *part_d;
  int32_t *idx, *part_idx;
  void carve(TipArena &a, int64_t n, int k, int S, int slices) {
    const size_t m = (size_t)n * (size_t)k;
    qry = a.take<double>((size_t)n * S); idx = a.take<int32_t>(m); dist = a.take<double>(m);
    part_idx = a.take<int32_t>(slices > 1 ? m * (size_t)slices : 1); part_d = a.take<double>(slices > 1 ? m * (size_t)slices : 1);
  }
};

int state_buffers(tr_roadmap *r, int64_t n, int k, StateBuffers &b, int &slices) {
  slices = state_slices(r, n);
  TipArena size;
  StateBuffers dummy;
  dummy.carve(size, n, k, r->S, slices);
  if (const int rc = tip_arena(r, size.used)) return rc;
  TipArena a;
  a.base = r->dt.arena;
  b.carve(a, n, k, r->S, slices);
  return TR_OK;
}

// tip_knn (+ tip_knn_merge) on the null stream: d_req n x 3 -> d_nbr n x k, d_d2 n x k (may be null)
int launch_nearest(tr_roadmap *r, const double *d_req, int64_t n, int k, int slices, const TipBuffers &b, int32_t *d_nbr, double *d_d2) {
  auto &d = r->dt;
  const int64_t groups = (n + kTipQ - 1) / kTipQ;
  const dim3 grid((unsigned)((groups + 3) / 4), (unsigned)slices);
  if (slices == 1) {
    hipLaunchKernelGGL((trk::tip_knn<kTipQ, kTipG>), grid, dim3(256), 0, nullptr, (const double *)d.d_tips, (const uint8_t *)d.d_vstat,
                       (const uint64_t *)d.d_present, r->V, d_req, n, k, d_nbr, d_d2);
    RM_HIP(r, hipGetLastError());
    return TR_OK;
  }
  hipLaunchKernelGGL((trk::tip_knn<kTipQ, kTipG>), grid, dim3(256), 0, nullptr, (const double *)d.d_tips, (const uint8_t *)d.d_vstat,
                     (const uint64_t *)d.d_present, r->V, d_req, n, k, b.part_idx, b.part_d2);
  RM_HIP(r, hipGetLastError());
  hipLaunchKernelGGL(trk::tip_knn_merge, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, nullptr, (const int32_t *)b.part_idx,
                     (const double *)b.part_d2, n, slices, k, d_nbr, d_d2);
  RM_HIP(r, hipGetLastError());
  return TR_OK;
}

// state_knn (+ tip_knn_merge) on the null stream: d_qry n x S -> d_idx n x k, d_dist n x k (may be null); part_*: the slices' lists
int launch_nearest_states(tr_roadmap *r, const double *d_qry, int64_t n, int k, double max_distance, int slices, int32_t *part_idx,
                          double *part_d, int32_t *d_idx, double *d_dist) {
  auto &d = r->dt;
  const int Q = trk::stateq_q(r->S);
  const int64_t groups = (n + Q - 1) / Q;
  const dim3 grid((unsigned)((groups + 3) / 4), (unsigned)slices);
  int32_t *oi = slices > 1 ? part_idx : d_idx;
  double *od = slices > 1 ? part_d : d_dist;
  const int variant = (r->rot ? 1 : 0) | (r->ret ? 2 : 0);
#define TRK_SKNN(NT, R, T) do { constexpr int SS_ = NT + (R ? 1 : 0) + (T ? 1 : 0); \
    hipLaunchKernelGGL((trk::state_knn<NT, R, T, trk::stateq_q(SS_), trk::stateq_g(SS_)>), grid, dim3(256), 0, nullptr, (const double *)d.d_soa, \
                       (const uint8_t *)d.d_vstat, r->V, d_qry, n, k, r->w_rot, r->w_ret, max_distance, oi, od); } while (0)
#define TRK_SCASE(NT) case NT: if (variant == 0) TRK_SKNN(NT, false, false); else if (variant == 1) TRK_SKNN(NT, true, false); \
                               else if (variant == 2) TRK_SKNN(NT, false, true); else TRK_SKNN(NT, true, true); break;
  switch (r->NT) {
    TRK_SCASE(1) TRK_SCASE(2) TRK_SCASE(3) TRK_SCASE(4) TRK_SCASE(5) TRK_SCASE(6) TRK_SCASE(7) TRK_SCASE(8)
    default: return rfail(r, TR_ERR_UNSUPPORTED, "nearest states: 1 .. 8 tendons");
  }
#undef TRK_SCASE
#undef TRK_SKNN
  RM_HIP(r, hipGetLastError());
  if (slices > 1) {
    hipLaunchKernelGGL(trk::tip_knn_merge, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, nullptr, (const int32_t *)part_idx, (const double *)part_d, n,
                       slices, k, d_idx, d_dist);
    RM_HIP(r, hipGetLastError());
  }
  return TR_OK;
}

int tips_ready(tr_roadmap *r, int64_t n, int32_t k) {
  if (!r->dt.set) return rfail(r, TR_ERR_INVALID_ARG, "the roadmap has no tips (tr_roadmap_set_tips)");
  if (n < 0 || k < 1 || k > TRK_TIPQ_MAX_K) return rfail(r, TR_ERR_INVALID_ARG, "bad argument (k: 1 .. 64)");
  if (n * (int64_t)k > ((int64_t)1 << 28)) return rfail(r, TR_ERR_INVALID_ARG, "too many candidates in one call (n k <= 2^28)");
  RM_HIP(r, hipSetDevice(tr_device(r->ctx)));
  return TR_OK;
}

static_assert(TRK_TIPQ_REACHED == TR_TIPQ_REACHED && TRK_TIPQ_CLOSEST == TR_TIPQ_CLOSEST && TRK_TIPQ_NO_NEIGHBOR == TR_TIPQ_NO_NEIGHBOR, "outcome codes");

// tr_fk_tips_dev on the null stream, a K1 launch per 2^18 states (a state's tip does not depend on the launch it is in)
int fk_tips_chunked(tr_roadmap *r, const double *d_states, int64_t n, double *d_tips) {
  const int64_t chunk = (int64_t)1 << 18;
  for (int64_t off = 0; off < n; off += chunk) {
    const int rc = tr_fk_tips_dev(r->ctx, d_states + off * r->S, std::min(chunk, n - off), d_tips + off * 3, nullptr, nullptr);
    if (rc) return rfail(r, rc, tr_last_error(r->ctx));
  }
  return TR_OK;
}

unsigned tipq_grid(int64_t n) { return (unsigned)((n + 255) / 256); }

// Rules 1 - 5 behind the lock, for both connection rules; every output may be null.  connect null or k_connect 0: every candidate
// slot has ONE source, the vertex IK started from (rules 3 - 5; ik_vertex = neighbor_vertex); otherwise the k_connect state-space
// neighbours of its IK answer and that vertex (rules 3' - 5').  count_stats: this is a *_connect call, dt.connect_stats follows it.
// L: the loaded rules' evaluator (2L - 5'L), null for the unloaded ones.
int tip_query_locked(tr_roadmap *r, const tr_space_params *sp, const tr_tip_query_params *params, const tr_tip_connect_params *connect,
                     bool count_stats, const double *requests, int64_t n, double *controls, double *tips, double *error,
                     int32_t *neighbor_vertex, int32_t *ik_vertex, int32_t *outcome, double *last_valid_t, const TipLoaded *L = nullptr) {
  const tr_tip_query_params def{5, 1e-4, tr_ik_params{100, 0.1, 1e-9, 1e-4, 1e-4, 1e-6}};      // roadmapIk's defaults and what it hands to IK
  const tr_tip_query_params &p = params ? *params : def;
  const tr_space_params spd{0.02, 0.01, 0.0001};                                                // Problem.h:59-62
  const tr_space_params &space = sp ? *sp : spd;
  int rc;
  if ((rc = tips_ready(r, n, p.k))) return rc;
  auto &d = r->dt;
  for (double &x : d.phase_ms) x = 0;
  d.st_ik_rounds = 0;
  if (count_stats) for (int64_t &x : d.connect_stats) x = 0;
  const int kc = connect ? connect->k_connect : 0;
  if (kc < 0 || kc > TRK_TIPQ_MAX_K) return rfail(r, TR_ERR_INVALID_ARG, "bad argument (k_connect: 0 .. 64)");
  if (kc > 0 && !(connect->max_distance >= 0)) return rfail(r, TR_ERR_INVALID_ARG, "max_distance must be >= 0 (INFINITY: no bound)");
  const int P = kc > 0 ? kc + 1 : 1;                                    // sources per candidate slot
  if (n * (int64_t)p.k * P > ((int64_t)1 << 28)) return rfail(r, TR_ERR_INVALID_ARG, "too many pairs in one call (n k (k_connect + 1) <= 2^28)");
  if (n == 0) return TR_OK;
  if (!requests) return rfail(r, TR_ERR_INVALID_ARG, "null requests");
  if (!(p.tolerance >= 0)) return rfail(r, TR_ERR_INVALID_ARG, "tolerance must be >= 0");
  const int k = p.k, S = r->S;
  const int64_t m = n * k, mp = m * P;
  auto t0 = Clock::now();
  auto lap = [&](int phase) { const auto t1 = Clock::now(); d.phase_ms[phase] += ms_between(t0, t1); t0 = t1; };
  // 1. neighbours
  if ((rc = tips_validity(r))) return rc;
  TipBuffers b;
  LoadedTipBuffers lb{};
  int slices = 1, c_slices = 1;
  if ((rc = tip_buffers(r, n, k, true, b, slices, kc, &c_slices, L ? &lb : nullptr))) return rc;
  int64_t n_integrations = 0, n_no_equilibrium = 0, n_g_unconverged = 0;
  RM_HIP(r, hipMemcpyAsync(b.req, requests, (size_t)n * 3 * sizeof(double), hipMemcpyHostToDevice, nullptr));
  if ((rc = launch_nearest(r, b.req, n, k, slices, b, b.nbr, nullptr))) return rc;
  // 2. IK from every neighbour, one batch
  hipLaunchKernelGGL(trk::tipq_gather, dim3(tipq_grid(m)), dim3(256), 0, nullptr, (const double *)d.d_states, S, (const int32_t *)b.nbr,
                     (const double *)b.req, n, k, b.starts, b.goals);
  RM_HIP(r, hipGetLastError());
  std::vector<int32_t> nbr((size_t)m);
  RM_HIP(r, hipMemcpy(nbr.data(), b.nbr, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost));     // (synchronises: the nearest phase ends here)
  lap(0);
  if (L) {
    int64_t rounds[2] = {0, 0};
    if ((rc = tr_ik_loaded_batch_dev(r->ctx, &p.ik, L->shoot, &L->loads, b.starts, m, b.goals, 3, nullptr, nullptr, nullptr, b.x, b.xtip, b.err,
                                     nullptr, lb.fkc, lb.xvu, lb.eq, rounds, nullptr))) return rfail(r, rc, tr_last_error(r->ctx));
    d.st_ik_rounds = rounds[0];
    std::vector<uint8_t> eq((size_t)m);
    std::vector<int32_t> fkc((size_t)m);
    RM_HIP(r, hipMemcpy(eq.data(), lb.eq, (size_t)m, hipMemcpyDeviceToHost));
    RM_HIP(r, hipMemcpy(fkc.data(), lb.fkc, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (int64_t s = 0; s < m; s++)
      if (nbr[(size_t)s] >= 0) { n_no_equilibrium += eq[(size_t)s] == 0; n_integrations += fkc[(size_t)s]; }
  } else if ((rc = tr_ik_batch_dev(r->ctx, &p.ik, b.starts, m, b.goals, 3, nullptr, nullptr, b.x, b.xtip, b.err, nullptr, nullptr, &d.st_ik_rounds, nullptr)))
    return rfail(r, rc, tr_last_error(r->ctx));
  // 3. partial edges: checkMotion(states[N], x, last_valid) on the slots that hold a neighbour (host-array form: Q k S doubles each way)
  std::vector<double> x((size_t)m * S);
  RM_HIP(r, hipMemcpy(x.data(), b.x, x.size() * sizeof(double), hipMemcpyDeviceToHost));
  lap(1);
  // the sources of every slot (pair p = slot P + j): the slot's neighbour alone, or (rule 3') the state-space neighbours of x_i first
  const int32_t *src = nbr.data();
  const double *d_a = b.starts, *d_b = b.x;
  std::vector<int32_t> pair_src;
  if (kc > 0) {
    if ((rc = launch_nearest_states(r, b.x, m, kc, connect->max_distance, c_slices, b.c_part_idx, b.c_part_d, b.cidx, nullptr))) return rc;
    hipLaunchKernelGGL(trk::tipq_pair_rows, dim3(tipq_grid(mp)), dim3(256), 0, nullptr, (const double *)d.d_states, S, (const int32_t *)b.nbr,
                       (const int32_t *)b.cidx, (const double *)b.x, m, kc, b.src, b.pa, b.pb);
    RM_HIP(r, hipGetLastError());
    pair_src.resize((size_t)mp);
    RM_HIP(r, hipMemcpy(pair_src.data(), b.src, (size_t)mp * sizeof(int32_t), hipMemcpyDeviceToHost));
    src = pair_src.data(); d_a = b.pa; d_b = b.pb;
    lap(0);                                                              // (the source search counts as `nearest`)
  }
  std::vector<int64_t> live;
  live.reserve((size_t)mp);
  for (int64_t s = 0; s < mp; s++) if (src[(size_t)s] >= 0) live.push_back(s);
  const int64_t ml = (int64_t)live.size();
  std::vector<uint8_t> ok((size_t)mp, 0);
  std::vector<double> t((size_t)mp, 0.0);
  if (ml > 0) {
    std::vector<double> ea((size_t)ml * S), eb((size_t)ml * S), et((size_t)ml);
    std::vector<uint64_t> bits((size_t)(ml + 63) / 64, 0);
    for (int64_t i = 0; i < ml; i++) {
      std::memcpy(&ea[(size_t)i * S], &r->states[(size_t)src[(size_t)live[(size_t)i]] * S], (size_t)S * sizeof(double));
      std::memcpy(&eb[(size_t)i * S], &x[(size_t)(live[(size_t)i] / P) * S], (size_t)S * sizeof(double));
    }
    if (L) {
      int64_t ni = 0;
      if ((rc = tr_validate_edges_loaded(r->ctx, &space, L->shoot, &L->loads, ea.data(), eb.data(), ml, bits.data(), et.data(), nullptr, nullptr,
                                         nullptr, &ni))) return rfail(r, rc, tr_last_error(r->ctx));
      n_integrations += ni;
    } else if ((rc = tr_validate_edges_last_valid(r->ctx, &space, ea.data(), eb.data(), ml, bits.data(), et.data(), nullptr)))
      return rfail(r, rc, tr_last_error(r->ctx));
    for (int64_t i = 0; i < ml; i++) {
      ok[(size_t)live[(size_t)i]] = (uint8_t)((bits[(size_t)i >> 6] >> (i & 63)) & 1);
      t[(size_t)live[(size_t)i]] = et[(size_t)i];
    }
  }
  RM_HIP(r, hipMemcpyAsync(b.ok, ok.data(), (size_t)mp, hipMemcpyHostToDevice, nullptr));
  RM_HIP(r, hipMemcpyAsync(b.t, t.data(), (size_t)mp * sizeof(double), hipMemcpyHostToDevice, nullptr));
  lap(2);
  // 4 - 5. the last valid state of every pair, its tip, and the choice
  hipLaunchKernelGGL(trk::tipq_interp, dim3(tipq_grid(mp)), dim3(256), 0, nullptr, d_a, d_b, (const double *)b.t, mp, S, r->rot ? r->NT : -1, b.g);
  RM_HIP(r, hipGetLastError());
  if (L) {
    // 5L: one cold loaded solve per live pair, dense; a dead pair has converged = 0
    RM_HIP(r, hipMemsetAsync(lb.gconv, 0, (size_t)mp, nullptr));
    if (ml > 0) {
      std::vector<int32_t> live32((size_t)ml);
      for (int64_t i = 0; i < ml; i++) live32[(size_t)i] = (int32_t)live[(size_t)i];
      RM_HIP(r, hipMemcpy(lb.live, live32.data(), (size_t)ml * sizeof(int32_t), hipMemcpyHostToDevice));
      hipLaunchKernelGGL(trk::tipql_live_rows, dim3(tipq_grid(ml)), dim3(256), 0, nullptr, (const double *)b.g, (const int32_t *)lb.live, ml, S,
                         r->rot ? r->NT : -1, L->k, lb.gl, lb.gw, lb.gd);
      RM_HIP(r, hipGetLastError());
      int64_t rounds[2] = {0, 0};
      if ((rc = tr_fk_loaded_tips_dev(r->ctx, L->shoot, lb.gl, ml, lb.gw, 6, lb.gd, 6, nullptr, lb.tipc, lb.convc, lb.vuc, rounds, nullptr)))
        return rfail(r, rc, tr_last_error(r->ctx));
      n_integrations += rounds[1];
      hipLaunchKernelGGL(trk::tipql_scatter, dim3(tipq_grid(ml)), dim3(256), 0, nullptr, (const int32_t *)lb.live, ml, (const double *)lb.tipc,
                         (const uint8_t *)lb.convc, (const double *)lb.vuc, b.gtip, lb.gconv, lb.gvu);
      RM_HIP(r, hipGetLastError());
      std::vector<uint8_t> conv((size_t)ml);
      RM_HIP(r, hipMemcpy(conv.data(), lb.convc, (size_t)ml, hipMemcpyDeviceToHost));
      for (const uint8_t c : conv) n_g_unconverged += c == 0;
    }
    hipLaunchKernelGGL(trk::tipql_select, dim3(tipq_grid(n)), dim3(256), 0, nullptr, (const int32_t *)b.nbr, (const double *)b.req, n, k, P, S,
                       p.tolerance, (const int32_t *)(kc > 0 ? b.src : b.nbr), (const double *)b.x, (const double *)b.xtip, (const double *)b.err,
                       (const uint8_t *)lb.eq, (const double *)lb.xvu, (const uint8_t *)b.ok, (const double *)b.t, (const double *)b.g,
                       (const double *)b.gtip, (const uint8_t *)lb.gconv, (const double *)lb.gvu, b.o_controls, b.o_tip, b.o_err, b.o_nbr, lb.o_ik,
                       b.o_outcome, b.o_t, lb.o_vu, lb.o_flags);
  } else if ((rc = fk_tips_chunked(r, b.g, mp, b.gtip))) return rc;
  else if (kc > 0)
    hipLaunchKernelGGL(trk::tipq_select_pairs, dim3(tipq_grid(n)), dim3(256), 0, nullptr, (const int32_t *)b.nbr, (const double *)b.req, n, k, P, S,
                       p.tolerance, (const int32_t *)b.src, (const double *)b.x, (const double *)b.xtip, (const double *)b.err, (const uint8_t *)b.ok,
                       (const double *)b.t, (const double *)b.g, (const double *)b.gtip, b.o_controls, b.o_tip, b.o_err, b.o_nbr, b.o_ik,
                       b.o_outcome, b.o_t, b.o_flags);
  else
    hipLaunchKernelGGL(trk::tipq_select, dim3(tipq_grid(n)), dim3(256), 0, nullptr, (const int32_t *)b.nbr, (const double *)b.req, n, k, S, p.tolerance,
                       (const double *)b.x, (const double *)b.xtip, (const double *)b.err, (const uint8_t *)b.ok, (const double *)b.t, (const double *)b.g,
                       (const double *)b.gtip, b.o_controls, b.o_tip, b.o_err, b.o_nbr, b.o_outcome, b.o_t);
  RM_HIP(r, hipGetLastError());
  if (controls) RM_HIP(r, hipMemcpyAsync(controls, b.o_controls, (size_t)n * S * sizeof(double), hipMemcpyDeviceToHost, nullptr));
  if (tips) RM_HIP(r, hipMemcpyAsync(tips, b.o_tip, (size_t)n * 3 * sizeof(double), hipMemcpyDeviceToHost, nullptr));
  if (error) RM_HIP(r, hipMemcpyAsync(error, b.o_err, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, nullptr));
  if (neighbor_vertex) RM_HIP(r, hipMemcpyAsync(neighbor_vertex, b.o_nbr, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, nullptr));
  if (ik_vertex) RM_HIP(r, hipMemcpyAsync(ik_vertex, L ? lb.o_ik : (kc > 0 ? b.o_ik : b.o_nbr), (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, nullptr));
  if (L && L->vu0) RM_HIP(r, hipMemcpyAsync(L->vu0, lb.o_vu, (size_t)n * 6 * sizeof(double), hipMemcpyDeviceToHost, nullptr));
  if (outcome) RM_HIP(r, hipMemcpyAsync(outcome, b.o_outcome, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, nullptr));
  if (last_valid_t) RM_HIP(r, hipMemcpyAsync(last_valid_t, b.o_t, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, nullptr));
  RM_HIP(r, hipStreamSynchronize(nullptr));
  if (count_stats) {
    // [0] pairs checked, [1] REACHED, [2] connection vertex != IK vertex, [3] REACHED where the one-edge rule is not
    d.connect_stats[0] = ml;
    if (kc > 0 || L) {
      std::vector<uint8_t> fl((size_t)n);
      RM_HIP(r, hipMemcpy(fl.data(), L ? lb.o_flags : b.o_flags, (size_t)n, hipMemcpyDeviceToHost));
      for (const uint8_t f : fl) {
        d.connect_stats[1] += (f & TRK_TIPQ_FLAG_REACHED) != 0; d.connect_stats[2] += (f & TRK_TIPQ_FLAG_MOVED) != 0;
        d.connect_stats[3] += (f & TRK_TIPQ_FLAG_GAINED) != 0;
      }
    } else {
      std::vector<int32_t> oc((size_t)n);
      RM_HIP(r, hipMemcpy(oc.data(), b.o_outcome, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
      for (const int32_t o : oc) d.connect_stats[1] += o == TR_TIPQ_REACHED;
    }
  }
  if (L && L->counts) { L->counts[0] = ml; L->counts[1] = n_no_equilibrium; L->counts[2] = n_g_unconverged; L->counts[3] = n_integrations; }
  lap(3);
  return TR_OK;
}

int solve_tips_locked(tr_roadmap *r, const tr_space_params *sp, const tr_tip_query_params *params, const tr_tip_connect_params *connect,
                      bool count_stats, const int32_t *starts, const double *requests, int64_t n, int32_t n_threads, double *controls,
                      double *tips, double *error, int32_t *neighbor_vertex, int32_t *ik_vertex, int32_t *outcome, double *last_valid_t,
                      int32_t *status, double *cost, int64_t *path_offsets, tr_roadmap_stats *stats, const TipLoaded *L = nullptr);

// What the loaded entry points check before rules 1 - 5, in this order: the frame, the robot and the solver's parameters (shoot_check's
// and shoot_params' wording, through an empty tr_fk_loaded_tips_dev), an empty call, the roadmap's tips.  `empty`: nothing to do.
int tip_loaded_begin(tr_roadmap *r, const tr_shoot_params *shoot, const tr_edge_loads *loads, int64_t n, double *vu0, int64_t *counts,
                     TipLoaded &L, bool &empty) {
  empty = false;
  L = TipLoaded{};
  L.shoot = shoot; L.vu0 = vu0; L.counts = counts;
  if (counts) for (int i = 0; i < 4; i++) counts[i] = 0;
  if (loads) {
    if (loads->frame != TR_LOAD_FRAME_BASE && loads->frame != TR_LOAD_FRAME_WORLD)
      return rfail(r, TR_ERR_INVALID_ARG, "bad argument (frame: TR_LOAD_FRAME_BASE or TR_LOAD_FRAME_WORLD)");
    L.loads = *loads;
  }
  L.loads.warm_start = 0;
  for (int q = 0; q < 6; q++) { L.k.wrench[q] = L.loads.wrench[q]; L.k.dist[q] = L.loads.dist[q]; }
  L.k.world = L.loads.frame == TR_LOAD_FRAME_WORLD;
  if (const int rc = tr_fk_loaded_tips_dev(r->ctx, shoot, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr))
    return rfail(r, rc, tr_last_error(r->ctx));
  // tr_fk_loaded_tips* takes a robot with retraction; the queries do not: their IK needs the tip's derivative along s_start
  if (r->ret)
    return rfail(r, TR_ERR_UNSUPPORTED, "loaded tip queries (tr_roadmap_ik_batch_loaded, tr_roadmap_solve_tips_loaded, tr_roadmap_set_tips_loaded): "
                                        "loaded FK (general_shape) is not built for robots with retraction in this call "
                                        "(tr_fk_loaded_batch*, tr_fk_loaded_tips* and the validity of loaded shapes are)");
  if (n == 0) { empty = true; return TR_OK; }
  if (r->dt.set && r->dt.own_tips)
    return rfail(r, TR_ERR_INVALID_ARG, "the roadmap's tips are those of UNLOADED shapes (tr_roadmap_set_tips computed them with tr_fk_tips_dev): "
                                        "pass loaded tips to tr_roadmap_set_tips or call tr_roadmap_set_tips_loaded");
  return TR_OK;
}

// tr_roadmap_set_tips behind the lock
int set_tips_locked(tr_roadmap *r, const double *tips, const uint64_t *present_bits) {
  RM_HIP(r, hipSetDevice(tr_device(r->ctx)));
  free_tips(r);
  auto &d = r->dt;
  const int64_t V = r->V;
  const int dev = tr_device(r->ctx);
  const size_t nw = (size_t)V / 64 + 1;
  RM_HIP(r, dev_cache().alloc(dev, (void **)&d.d_tips, std::max<size_t>(1, (size_t)V * 3) * sizeof(double)));
  RM_HIP(r, dev_cache().alloc(dev, (void **)&d.d_states, std::max<size_t>(1, (size_t)V * r->S) * sizeof(double)));
  RM_HIP(r, dev_cache().alloc(dev, (void **)&d.d_soa, std::max<size_t>(1, (size_t)V * r->S) * sizeof(double)));
  RM_HIP(r, dev_cache().alloc(dev, (void **)&d.d_vstat, std::max<size_t>(1, (size_t)V)));
  RM_HIP(r, dev_cache().alloc(dev, (void **)&d.d_present, nw * sizeof(uint64_t)));
  d.present.assign(nw, 0);
  for (int64_t v = 0; v < V; v++)
    if (!present_bits || ((present_bits[v >> 6] >> (v & 63)) & 1)) d.present[(size_t)v >> 6] |= (uint64_t)1 << (v & 63);
  if (V > 0) {
    RM_HIP(r, hipMemcpy(d.d_states, r->states.data(), (size_t)V * r->S * sizeof(double), hipMemcpyHostToDevice));
    // ... and coordinate by coordinate ([S][V]): state_knn's tiles read 64 consecutive doubles per coordinate
    std::vector<double> soa((size_t)V * r->S);
    for (int64_t v = 0; v < V; v++)
      for (int c = 0; c < r->S; c++) soa[(size_t)c * V + v] = r->states[(size_t)v * r->S + c];
    RM_HIP(r, hipMemcpy(d.d_soa, soa.data(), soa.size() * sizeof(double), hipMemcpyHostToDevice));
    if (tips) {
      RM_HIP(r, hipMemcpy(d.d_tips, tips, (size_t)V * 3 * sizeof(double), hipMemcpyHostToDevice));
    } else {
      // fk_shape(state).p.back() of every vertex, once (voxelizeVertex stores it: vertexTipPositionProperty_, :2803-2837)
      if (const int rc = fk_tips_chunked(r, d.d_states, V, d.d_tips)) return rc;
      RM_HIP(r, hipStreamSynchronize(nullptr));
    }
  }
  RM_HIP(r, hipMemcpy(d.d_present, d.present.data(), nw * sizeof(uint64_t), hipMemcpyHostToDevice));
  d.vstat_sent.clear();                                     // (differs from `vstat` unless the roadmap is empty: the first call sends it)
  d.set = true;
  d.own_tips = tips == nullptr;
  return TR_OK;
}

// a device array of the call, handed back when the call ends
struct TipScratch {
  void *p = nullptr;
  ~TipScratch() { if (p) dev_cache().release(p); }
};

}  // namespace

extern "C" {

int tr_roadmap_set_tips(tr_roadmap *r, const double *tips, const uint64_t *present_bits) {
  if (!r) return TR_ERR_INVALID_ARG;
  RmLock lock_(r);
  return set_tips_locked(r, tips, present_bits);
}

int tr_roadmap_set_tips_loaded(tr_roadmap *r, const tr_shoot_params *shoot, const tr_edge_loads *loads, const uint64_t *present_bits) {
  if (!r) return TR_ERR_INVALID_ARG;
  RmLock lock_(r);
  TipLoaded L;
  bool empty;
  int rc;
  if ((rc = tip_loaded_begin(r, shoot, loads, 0, nullptr, nullptr, L, empty))) return rc;
  const int64_t V = r->V;
  const int S = r->S;
  std::vector<double> tips((size_t)std::max<int64_t>(V, 1) * 3, 0.0);
  std::vector<uint64_t> present((size_t)V / 64 + 1, 0);
  for (int64_t v = 0; v < V; v++)
    if (!present_bits || ((present_bits[v >> 6] >> (v & 63)) & 1)) present[(size_t)v >> 6] |= (uint64_t)1 << (v & 63);
  if (V > 0) {
    RM_HIP(r, hipSetDevice(tr_device(r->ctx)));
    const int dev = tr_device(r->ctx);
    TipScratch st, w, dd, tp, cv;
    RM_HIP(r, dev_cache().alloc(dev, &st.p, (size_t)V * S * sizeof(double)));
    RM_HIP(r, dev_cache().alloc(dev, &w.p, (size_t)V * 6 * sizeof(double)));
    RM_HIP(r, dev_cache().alloc(dev, &dd.p, (size_t)V * 6 * sizeof(double)));
    RM_HIP(r, dev_cache().alloc(dev, &tp.p, (size_t)V * 3 * sizeof(double)));
    RM_HIP(r, dev_cache().alloc(dev, &cv.p, (size_t)V));
    RM_HIP(r, hipMemcpy(st.p, r->states.data(), (size_t)V * S * sizeof(double), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(trk::tipql_load_rows, dim3(tipq_grid(V)), dim3(256), 0, nullptr, (const double *)st.p, V, S, r->rot ? r->NT : -1, L.k,
                       (double *)w.p, (double *)dd.p);
    RM_HIP(r, hipGetLastError());
    if ((rc = tr_fk_loaded_tips_dev(r->ctx, shoot, (const double *)st.p, V, (const double *)w.p, 6, (const double *)dd.p, 6, nullptr, (double *)tp.p,
                                    (uint8_t *)cv.p, nullptr, nullptr, nullptr))) return rfail(r, rc, tr_last_error(r->ctx));
    std::vector<uint8_t> conv((size_t)V);
    RM_HIP(r, hipMemcpy(tips.data(), tp.p, (size_t)V * 3 * sizeof(double), hipMemcpyDeviceToHost));
    RM_HIP(r, hipMemcpy(conv.data(), cv.p, (size_t)V, hipMemcpyDeviceToHost));
    for (int64_t v = 0; v < V; v++)
      if (!conv[(size_t)v]) present[(size_t)v >> 6] &= ~((uint64_t)1 << (v & 63));      // no equilibrium: no tip
  }
  return set_tips_locked(r, tips.data(), present.data());
}

int tr_roadmap_ik_batch_loaded(tr_roadmap *r, const tr_space_params *sp, const tr_tip_query_params *params, const tr_tip_connect_params *connect,
                               const tr_shoot_params *shoot, const tr_edge_loads *loads, const double *requests, int64_t n, double *controls,
                               double *tips, double *error, int32_t *neighbor_vertex, int32_t *ik_vertex, int32_t *outcome,
                               double *last_valid_t, double *vu0, int64_t *counts) {
  if (!r) return TR_ERR_INVALID_ARG;
  RmLock lock_(r);
  TipLoaded L;
  bool empty;
  if (const int rc = tip_loaded_begin(r, shoot, loads, n, vu0, counts, L, empty)) return rc;
  if (empty) return TR_OK;
  return tip_query_locked(r, sp, params, connect, true, requests, n, controls, tips, error, neighbor_vertex, ik_vertex, outcome, last_valid_t, &L);
}

int tr_roadmap_solve_tips_loaded(tr_roadmap *r, const tr_space_params *sp, const tr_tip_query_params *params, const tr_tip_connect_params *connect,
                                 const tr_shoot_params *shoot, const tr_edge_loads *loads, const int32_t *starts, const double *requests, int64_t n,
                                 int32_t n_threads, double *controls, double *tips, double *error, int32_t *neighbor_vertex, int32_t *ik_vertex,
                                 int32_t *outcome, double *last_valid_t, double *vu0, int64_t *counts, int32_t *status, double *cost,
                                 int64_t *path_offsets, tr_roadmap_stats *stats) {
  if (!r) return TR_ERR_INVALID_ARG;
  RmLock lock_(r);
  TipLoaded L;
  bool empty;
  if (const int rc = tip_loaded_begin(r, shoot, loads, n, vu0, counts, L, empty)) return rc;
  if (empty) {
    reset_last_solve(r, 0);
    if (path_offsets) path_offsets[0] = 0;
    if (stats) *stats = tr_roadmap_stats{0, 0, 0, 0};
    return TR_OK;
  }
  return solve_tips_locked(r, sp, params, connect, true, starts, requests, n, n_threads, controls, tips, error, neighbor_vertex, ik_vertex, outcome,
                           last_valid_t, status, cost, path_offsets, stats, &L);
}

int tr_roadmap_nearest_tips_dev(tr_roadmap *r, const double *d_requests, int64_t n, int32_t k, int32_t *d_vertices, double *d_dist2) {
  if (!r) return TR_ERR_INVALID_ARG;
  RmLock lock_(r);
  int rc;
  if ((rc = tips_ready(r, n, k))) return rc;
  if (n == 0) return TR_OK;
  if (!d_requests || !d_vertices) return rfail(r, TR_ERR_INVALID_ARG, "null device pointer");
  RM_HIP(r, hipDeviceSynchronize());                        // (the requests may have been written on any stream)
  if ((rc = tips_validity(r))) return rc;
  TipBuffers b;
  int slices = 1;
  if ((rc = tip_buffers(r, n, k, false, b, slices))) return rc;
  if ((rc = launch_nearest(r, d_requests, n, k, slices, b, d_vertices, d_dist2))) return rc;
  RM_HIP(r, hipStreamSynchronize(nullptr));
  return TR_OK;
}

int tr_roadmap_nearest_tips(tr_roadmap *r, const double *requests, int64_t n, int32_t k, int32_t *vertices, double *dist2) {
  if (!r) return TR_ERR_INVALID_ARG;
  RmLock lock_(r);
  int rc;
  if ((rc = tips_ready(r, n, k))) return rc;
  if (n == 0) return TR_OK;
  if (!requests || !vertices) return rfail(r, TR_ERR_INVALID_ARG, "null argument");
  if ((rc = tips_validity(r))) return rc;
  TipBuffers b;
  int slices = 1;
  if ((rc = tip_buffers(r, n, k, false, b, slices))) return rc;
  RM_HIP(r, hipMemcpyAsync(b.req, requests, (size_t)n * 3 * sizeof(double), hipMemcpyHostToDevice, nullptr));
  if ((rc = launch_nearest(r, b.req, n, k, slices, b, b.nbr, b.d2))) return rc;
  RM_HIP(r, hipMemcpyAsync(vertices, b.nbr, (size_t)n * k * sizeof(int32_t), hipMemcpyDeviceToHost, nullptr));
  if (dist2) RM_HIP(r, hipMemcpyAsync(dist2, b.d2, (size_t)n * k * sizeof(double), hipMemcpyDeviceToHost, nullptr));
  RM_HIP(r, hipStreamSynchronize(nullptr));
  return TR_OK;
}

int tr_roadmap_nearest_states_dev(tr_roadmap *r, const double *d_queries, int64_t n, int32_t k, double max_distance, int32_t *d_vertices,
                                  double *d_dist) {
  if (!r) return TR_ERR_INVALID_ARG;
  RmLock lock_(r);
  int rc;
  if ((rc = tips_ready(r, n, k))) return rc;
  if (!(max_distance >= 0)) return rfail(r, TR_ERR_INVALID_ARG, "max_distance must be >= 0 (INFINITY: no bound)");
  if (n == 0) return TR_OK;
  if (!d_queries || !d_vertices) return rfail(r, TR_ERR_INVALID_ARG, "null device pointer");
  RM_HIP(r, hipDeviceSynchronize());                        // (the queries may have been written on any stream)
  if ((rc = tips_validity(r))) return rc;
  StateBuffers b;
  int slices = 1;
  if ((rc = state_buffers(r, n, k, b, slices))) return rc;
  // (the slices' lists carry their distances whether or not the caller wants them: the merge orders by them)
  if ((rc = launch_nearest_states(r, d_queries, n, k, max_distance, slices, b.part_idx, b.part_d, d_vertices, d_dist))) return rc;
  RM_HIP(r, hipStreamSynchronize(nullptr));
  return TR_OK;
}

int tr_roadmap_nearest_states(tr_roadmap *r, const double *queries, int64_t n, int32_t k, double max_distance, int32_t *vertices, double *dist) {
  if (!r) return TR_ERR_INVALID_ARG;
  RmLock lock_(r);
  int rc;
  if ((rc = tips_ready(r, n, k))) return rc;
  if (!(max_distance >= 0)) return rfail(r, TR_ERR_INVALID_ARG, "max_distance must be >= 0 (INFINITY: no bound)");
  if (n == 0) return TR_OK;
  if (!queries || !vertices) return rfail(r, TR_ERR_INVALID_ARG, "null argument");
  if ((rc = tips_validity(r))) return rc;
  StateBuffers b;
  int slices = 1;
  if ((rc = state_buffers(r, n, k, b, slices))) return rc;
  RM_HIP(r, hipMemcpyAsync(b.qry, queries, (size_t)n * r->S * sizeof(double), hipMemcpyHostToDevice, nullptr));
  if ((rc = launch_nearest_states(r, b.qry, n, k, max_distance, slices, b.part_idx, b.part_d, b.idx, b.dist))) return rc;
  RM_HIP(r, hipMemcpyAsync(vertices, b.idx, (size_t)n * k * sizeof(int32_t), hipMemcpyDeviceToHost, nullptr));
  if (dist) RM_HIP(r, hipMemcpyAsync(dist, b.dist, (size_t)n * k * sizeof(double), hipMemcpyDeviceToHost, nullptr));
  RM_HIP(r, hipStreamSynchronize(nullptr));
  return TR_OK;
}

int tr_roadmap_ik_batch(tr_roadmap *r, const tr_space_params *sp, const tr_tip_query_params *params, const double *requests, int64_t n,
                        double *controls, double *tips, double *error, int32_t *neighbor_vertex, int32_t *outcome, double *last_valid_t) {
  if (!r) return TR_ERR_INVALID_ARG;
  RmLock lock_(r);
  return tip_query_locked(r, sp, params, nullptr, false, requests, n, controls, tips, error, neighbor_vertex, nullptr, outcome, last_valid_t);
}

int tr_roadmap_ik_batch_connect(tr_roadmap *r, const tr_space_params *sp, const tr_tip_query_params *params, const tr_tip_connect_params *connect,
                                const double *requests, int64_t n, double *controls, double *tips, double *error, int32_t *neighbor_vertex,
                                int32_t *ik_vertex, int32_t *outcome, double *last_valid_t) {
  if (!r) return TR_ERR_INVALID_ARG;
  RmLock lock_(r);
  return tip_query_locked(r, sp, params, connect, true, requests, n, controls, tips, error, neighbor_vertex, ik_vertex, outcome, last_valid_t);
}

int tr_roadmap_tip_connect_stats(tr_roadmap *r, int64_t out[4]) {
  if (!r || !out) return TR_ERR_INVALID_ARG;
  RmLock lock_(r);
  for (int i = 0; i < 4; i++) out[i] = r->dt.connect_stats[i];
  return TR_OK;
}

int tr_roadmap_solve_tips(tr_roadmap *r, const tr_space_params *sp, const tr_tip_query_params *params, const int32_t *starts,
                          const double *requests, int64_t n, int32_t n_threads, double *controls, double *tips, double *error,
                          int32_t *neighbor_vertex, int32_t *outcome, double *last_valid_t, int32_t *status, double *cost,
                          int64_t *path_offsets, tr_roadmap_stats *stats) {
  if (!r) return TR_ERR_INVALID_ARG;
  RmLock lock_(r);
  return solve_tips_locked(r, sp, params, nullptr, false, starts, requests, n, n_threads, controls, tips, error, neighbor_vertex, nullptr, outcome,
                           last_valid_t, status, cost, path_offsets, stats);
}

int tr_roadmap_solve_tips_connect(tr_roadmap *r, const tr_space_params *sp, const tr_tip_query_params *params, const tr_tip_connect_params *connect,
                                  const int32_t *starts, const double *requests, int64_t n, int32_t n_threads, double *controls, double *tips,
                                  double *error, int32_t *neighbor_vertex, int32_t *ik_vertex, int32_t *outcome, double *last_valid_t,
                                  int32_t *status, double *cost, int64_t *path_offsets, tr_roadmap_stats *stats) {
  if (!r) return TR_ERR_INVALID_ARG;
  RmLock lock_(r);
  return solve_tips_locked(r, sp, params, connect, true, starts, requests, n, n_threads, controls, tips, error, neighbor_vertex, ik_vertex, outcome,
                           last_valid_t, status, cost, path_offsets, stats);
}

}  // extern "C"

namespace {

// Rules 1 - 6 behind the lock, for both connection rules
int solve_tips_locked(tr_roadmap *r, const tr_space_params *sp, const tr_tip_query_params *params, const tr_tip_connect_params *connect,
                      bool count_stats, const int32_t *starts, const double *requests, int64_t n, int32_t n_threads, double *controls,
                      double *tips, double *error, int32_t *neighbor_vertex, int32_t *ik_vertex, int32_t *outcome, double *last_valid_t,
                      int32_t *status, double *cost, int64_t *path_offsets, tr_roadmap_stats *stats, const TipLoaded *L) {
  if (n < 0 || (n > 0 && (!starts || !requests || !status || !path_offsets))) return rfail(r, TR_ERR_INVALID_ARG, "bad argument");
  reset_last_solve(r, n);
  if (path_offsets) path_offsets[0] = 0;
  if (stats) *stats = tr_roadmap_stats{0, 0, 0, 0};
  for (int64_t q = 0; q < n; q++)
    if (starts[q] < 0 || starts[q] >= r->V) return rfail(r, TR_ERR_OUT_OF_RANGE, "query vertex outside the roadmap");
  // rules 1 - 5 (the solve below needs the connection vertices and the goal states whether or not the caller asked for them)
  std::vector<double> own_controls;
  std::vector<int32_t> own_nbr, own_outcome;
  if (!controls) { own_controls.resize((size_t)n * r->S); controls = own_controls.data(); }
  if (!neighbor_vertex) { own_nbr.resize((size_t)n); neighbor_vertex = own_nbr.data(); }
  if (!outcome) { own_outcome.resize((size_t)n); outcome = own_outcome.data(); }
  int rc;
  if ((rc = tip_query_locked(r, sp, params, connect, count_stats, requests, n, controls, tips, error, neighbor_vertex, ik_vertex, outcome, last_valid_t, L)))
    return rc;
  if (n == 0) return TR_OK;
  // rule 6: the roadmap query to the connection vertex; a request without a neighbour has no goal
  const auto t0 = Clock::now();
  std::vector<int64_t> live;
  std::vector<int32_t> s2, g2;
  for (int64_t q = 0; q < n; q++)
    if (outcome[q] != TR_TIPQ_NO_NEIGHBOR) { live.push_back(q); s2.push_back(starts[q]); g2.push_back(neighbor_vertex[q]); }
  const int64_t nl = (int64_t)live.size();
  std::vector<int32_t> st2((size_t)nl);
  std::vector<double> c2((size_t)nl);
  std::vector<int64_t> off2((size_t)nl + 1, 0);
  if ((rc = solve_locked(r, s2.data(), g2.data(), nl, n_threads, st2.data(), c2.data(), off2.data(), stats))) return rc;
  // (the stored paths are the live requests' in order: only the offsets change)
  r->path_off.assign((size_t)n + 1, 0);
  for (int64_t q = 0; q < n; q++) { status[q] = TR_QUERY_INVALID_GOAL; if (cost) cost[q] = std::numeric_limits<double>::infinity(); }
  int64_t j = 0;
  for (int64_t q = 0; q < n; q++) {
    int64_t len = 0;
    if (j < nl && live[(size_t)j] == q) {
      len = off2[(size_t)j + 1] - off2[(size_t)j];
      status[q] = st2[(size_t)j];
      // the one edge that joins the goal state to the roadmap: its cost is the state-space distance (connectVertices :2857-2861)
      if (cost && st2[(size_t)j] == TR_QUERY_SOLVED)
        cost[q] = c2[(size_t)j] + state_distance(r, &r->states[(size_t)neighbor_vertex[q] * r->S], &controls[(size_t)q * r->S]);
      j++;
    }
    r->path_off[(size_t)q + 1] = r->path_off[(size_t)q] + len;
    path_offsets[q + 1] = r->path_off[(size_t)q + 1];
  }
  r->dt.phase_ms[4] = ms_between(t0, Clock::now());
  return TR_OK;
}

}  // namespace

extern "C" {

int tr_roadmap_tip_query_profile(tr_roadmap *r, double out[6]) {
  if (!r || !out) return TR_ERR_INVALID_ARG;
  RmLock lock_(r);
  for (int i = 0; i < 5; i++) out[i] = r->dt.phase_ms[i];
  out[5] = (double)r->dt.st_ik_rounds;
  return TR_OK;
}

}  // extern "C"
