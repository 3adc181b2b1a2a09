// roadmap_attach_host.inc -- part of roadmap.hip: queries between ARBITRARY states.  solvePrep (motion-planning/VoxelCachedLazyPRM.cpp:2978-3020)
// turns the problem's start and goal states into milestones with addMilestone(state, connect = true) (:1854-1885) and A* runs over the
// augmented graph; here nothing is inserted:
//   attach (tr_roadmap_attach_states): a batch of states -> tr_validate_batch_dev -> state_knn -> attach_mark .. attach_fill (the live
//     slots as index pairs over [roadmap rows | query rows], resident in HBM) -> ONE tr_validate_edges_indexed_dev -> attach_scatter;
//     between the states going up and the result arrays coming down the pairs never cross the bus, only their number (the edge call's
//     own results -- verdict words, FK counts when asked for -- bounce through the host inside it: validate_edges_indexed_to_dev)
//   seeded search (tr_roadmap_solve_seeded): Solve's lazy rounds with astar_seeded in place of astar -- on the host threads at every
//     batch size; roadmap_astar is never launched by these calls (tr_roadmap_search_stats out[0] stays 0)
//   tr_roadmap_solve_states: starts attached OUT, goals IN and the direct edges in one attach pass, then the seeded search.
namespace {

struct AttachBuffers {
  uint64_t *valid_bits, *pair_bits;
  int32_t *idx, *part_idx, *pair_all, *pairs, *slot_pos, *pair_nfk, *nfk;
  double *dist, *part_d, *ddist;
  uint8_t *valid, *live, *ok;
  uint32_t *block_count, *block_off;
  void carve(TipArena &a, int64_t rows, int k, int slices, int64_t n_direct) {
    const size_t m = (size_t)rows * (size_t)k, mt = m + (size_t)n_direct, nb = (mt + trk::ATTACH_BLOCK - 1) / trk::ATTACH_BLOCK;
    valid_bits = a.take<uint64_t>((size_t)rows / 64 + 1); valid = a.take<uint8_t>((size_t)rows);
    idx = a.take<int32_t>(m); dist = a.take<double>(m);
    part_idx = a.take<int32_t>(slices > 1 ? m * (size_t)slices : 1); part_d = a.take<double>(slices > 1 ? m * (size_t)slices : 1);
    live = a.take<uint8_t>(mt); pair_all = a.take<int32_t>(2 * mt); pairs = a.take<int32_t>(2 * mt); slot_pos = a.take<int32_t>(mt);
    block_count = a.take<uint32_t>(nb); block_off = a.take<uint32_t>(nb + 1);
    pair_bits = a.take<uint64_t>(mt / 64 + 1); pair_nfk = a.take<int32_t>(mt);
    ok = a.take<uint8_t>(mt); nfk = a.take<int32_t>(mt); ddist = a.take<double>((size_t)n_direct);
  }
};

// the array the index pairs refer to: the roadmap's rows (copied once, resident from then on) with room for `rows` query rows behind them
int attach_rows(tr_roadmap *r, int64_t rows) {
  auto &d = r->dt;
  if (d.d_ext && d.ext_cap >= rows) return TR_OK;
  if (d.d_ext) dev_cache().release(d.d_ext);
  d.d_ext = nullptr; d.ext_cap = 0;
  const int64_t cap = std::max<int64_t>(rows + rows / 2, 1024);
  RM_HIP(r, dev_cache().alloc(tr_device(r->ctx), (void **)&d.d_ext, (size_t)(r->V + cap) * r->S * sizeof(double)));
  d.ext_cap = cap;
  if (r->V > 0) RM_HIP(r, hipMemcpyAsync(d.d_ext, d.d_states, (size_t)r->V * r->S * sizeof(double), hipMemcpyDeviceToDevice, nullptr));
  return TR_OK;
}

const tr_space_params kAttachSpace{0.02, 0.01, 0.0001};                 // Problem.h:59-62

int attach_params(tr_roadmap *r, const tr_attach_params *params, int64_t rows, int &k, double &max_distance) {
  k = params ? params->k : 10;                                           // connect_k's defaults
  max_distance = params ? params->max_distance : std::numeric_limits<double>::infinity();
  if (const int rc = tips_ready(r, rows, k)) return rc;
  if (!(max_distance >= 0)) return rfail(r, TR_ERR_INVALID_ARG, "max_distance must be >= 0 (INFINITY: no bound)");
  return TR_OK;
}

// Rules A1 - A4 for `rows` query states (host or device rows), the first n_out of them attached OUT, the others IN; with `direct`
// (rows = 2 n: n starts, then n goals) the direct edges of tr_roadmap_solve_states ride in the same edge call, n slots behind the
// rows x k attach slots.  The results stay in the call's arena (b).  phase_ms (optional): [0] += validity + nearest + pairs, [1] += edges.
int attach_pass(tr_roadmap *r, const tr_space_params &space, int k, double max_distance, const double *qry, bool qry_on_device, int64_t rows,
                int64_t n_out, bool direct, bool want_nfk, AttachBuffers &b, int64_t *n_pairs, int64_t *n_domain_errors, double *phase_ms) {
  auto t0 = Clock::now();
  auto lap = [&](int phase) { const auto t1 = Clock::now(); if (phase_ms) phase_ms[phase] += ms_between(t0, t1); t0 = t1; };
  int rc;
  const int S = r->S;
  const int64_t V = r->V, m = rows * k, n_direct = direct ? rows / 2 : 0, mt = m + n_direct;
  if ((rc = tips_validity(r)) || (rc = attach_rows(r, rows))) return rc;
  const int slices = state_slices(r, rows);
  {
    TipArena size;
    AttachBuffers dummy;
    dummy.carve(size, rows, k, slices, n_direct);
    if ((rc = tip_arena(r, size.used))) return rc;
    TipArena a;
    a.base = r->dt.arena;
    b.carve(a, rows, k, slices, n_direct);
  }
  double *d_q = r->dt.d_ext + (size_t)V * S;
  RM_HIP(r, hipMemcpyAsync(d_q, qry, (size_t)rows * S * sizeof(double), qry_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, nullptr));
  // A1, A2
  if ((rc = tr_validate_batch_dev(r->ctx, d_q, rows, b.valid_bits, nullptr, nullptr, nullptr))) return rfail(r, rc, tr_last_error(r->ctx));
  if ((rc = launch_nearest_states(r, d_q, rows, k, max_distance, slices, b.part_idx, b.part_d, b.idx, b.dist))) return rc;
  // the live slots as index pairs, in slot order
  hipLaunchKernelGGL(trk::attach_mark, dim3(tipq_grid(m)), dim3(256), 0, nullptr, (const uint64_t *)b.valid_bits, rows, n_out, k, V, b.idx, b.dist,
                     b.valid, b.live, b.pair_all);
  RM_HIP(r, hipGetLastError());
  if (direct) {
    hipLaunchKernelGGL(trk::attach_mark_direct, dim3(tipq_grid(n_direct)), dim3(256), 0, nullptr, (const uint64_t *)b.valid_bits, n_direct, k, V, S,
                       r->NT, r->rot ? 1 : 0, r->ret ? 1 : 0, r->w_rot, r->w_ret, max_distance, (const double *)d_q, (const double *)b.dist,
                       b.live + m, b.pair_all + 2 * m, b.ddist);
    RM_HIP(r, hipGetLastError());
  }
  const int64_t nb = (mt + trk::ATTACH_BLOCK - 1) / trk::ATTACH_BLOCK;
  hipLaunchKernelGGL(trk::attach_count, dim3((unsigned)nb), dim3(trk::ATTACH_BLOCK), 0, nullptr, (const uint8_t *)b.live, mt, b.block_count);
  RM_HIP(r, hipGetLastError());
  hipLaunchKernelGGL(trk::attach_scan, dim3(1), dim3(trk::ATTACH_BLOCK), 0, nullptr, (const uint32_t *)b.block_count, nb, b.block_off);
  RM_HIP(r, hipGetLastError());
  hipLaunchKernelGGL(trk::attach_fill, dim3((unsigned)nb), dim3(trk::ATTACH_BLOCK), 0, nullptr, (const uint8_t *)b.live, mt,
                     (const uint32_t *)b.block_off, (const int32_t *)b.pair_all, b.pairs, b.slot_pos);
  RM_HIP(r, hipGetLastError());
  uint32_t total = 0;
  RM_HIP(r, hipMemcpy(&total, b.block_off + nb, sizeof(total), hipMemcpyDeviceToHost));      // (synchronises: of the pairs only the count comes down)
  lap(0);
  // A3: one edge check over [roadmap rows | query rows]
  int64_t nd = 0;
  if (total > 0 &&
      (rc = tr_validate_edges_indexed_dev(r->ctx, &space, r->dt.d_ext, V + rows, b.pairs, (int64_t)total, b.pair_bits, want_nfk ? b.pair_nfk : nullptr, &nd)))
    return rfail(r, rc, tr_last_error(r->ctx));
  hipLaunchKernelGGL(trk::attach_scatter, dim3(tipq_grid(mt)), dim3(256), 0, nullptr, (const int32_t *)b.slot_pos, mt, (const uint64_t *)b.pair_bits,
                     (const int32_t *)b.pair_nfk, b.ok, want_nfk ? b.nfk : nullptr);
  RM_HIP(r, hipGetLastError());
  if (n_pairs) *n_pairs = (int64_t)total;
  if (n_domain_errors) *n_domain_errors = nd;
  RM_HIP(r, hipStreamSynchronize(nullptr));
  lap(1);
  return TR_OK;
}

int attach_states_locked(tr_roadmap *r, const tr_space_params *sp, const tr_attach_params *params, int32_t direction, const double *states, int64_t n,
                         bool on_device, uint8_t *valid, int32_t *vertices, double *cost, uint8_t *edge_ok, int32_t *n_fk, int64_t *n_domain_errors) {
  if (n_domain_errors) *n_domain_errors = 0;
  int k, rc;
  double max_distance;
  if ((rc = attach_params(r, params, n, k, max_distance))) return rc;
  if (direction != TR_ATTACH_OUT && direction != TR_ATTACH_IN) return rfail(r, TR_ERR_INVALID_ARG, "bad argument (direction: TR_ATTACH_OUT or TR_ATTACH_IN)");
  if (n == 0) return TR_OK;
  if (!states || !valid || !vertices || !cost || !edge_ok) return rfail(r, TR_ERR_INVALID_ARG, on_device ? "null device pointer" : "null argument");
  if (on_device) RM_HIP(r, hipDeviceSynchronize());                    // (the states may have been written on any stream)
  AttachBuffers b;
  if ((rc = attach_pass(r, sp ? *sp : kAttachSpace, k, max_distance, states, on_device, n, direction == TR_ATTACH_OUT ? n : 0, false, n_fk != nullptr,
                        b, nullptr, n_domain_errors, nullptr))) return rc;
  const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  const size_t m = (size_t)n * (size_t)k;
  RM_HIP(r, hipMemcpyAsync(valid, b.valid, (size_t)n, kind, nullptr));
  RM_HIP(r, hipMemcpyAsync(vertices, b.idx, m * sizeof(int32_t), kind, nullptr));
  RM_HIP(r, hipMemcpyAsync(cost, b.dist, m * sizeof(double), kind, nullptr));
  RM_HIP(r, hipMemcpyAsync(edge_ok, b.ok, m, kind, nullptr));
  if (n_fk) RM_HIP(r, hipMemcpyAsync(n_fk, b.nfk, m * sizeof(int32_t), kind, nullptr));
  RM_HIP(r, hipStreamSynchronize(nullptr));
  return TR_OK;
}

// tr_roadmap_solve_seeded behind the lock.  s.src_pick / s.dst_pick must be arrays of n_queries.
int solve_seeded_locked(tr_roadmap *r, SeededQueries &s, int64_t n_queries, int32_t n_threads, int32_t *status, double *cost,
                        int64_t *path_offsets, tr_roadmap_stats *stats) {
  if (n_queries < 0 || (n_queries > 0 && (!s.src_off || !s.dst_off || !status || !path_offsets || !s.src_pick || !s.dst_pick)))
    return rfail(r, TR_ERR_INVALID_ARG, "bad argument");
  reset_last_solve(r, n_queries);
  if (path_offsets) path_offsets[0] = 0;
  if (n_queries == 0) { if (stats) *stats = tr_roadmap_stats{0, 0, 0, 0}; return TR_OK; }
  for (int side = 0; side < 2; side++) {
    const int64_t *off = side ? s.dst_off : s.src_off;
    const int32_t *v = side ? s.dst_v : s.src_v;
    const double *c = side ? s.dst_c : s.src_c;
    if (off[0] != 0) return rfail(r, TR_ERR_INVALID_ARG, "seed offsets must start at 0");
    for (int64_t q = 0; q < n_queries; q++) if (off[q] > off[q + 1]) return rfail(r, TR_ERR_INVALID_ARG, "seed offsets must be non-decreasing");
    if (off[n_queries] > 0 && (!v || !c)) return rfail(r, TR_ERR_INVALID_ARG, "null seed arrays");
    for (int64_t i = 0; i < off[n_queries]; i++) {
      if (v[i] < 0 || v[i] >= r->V) return rfail(r, TR_ERR_OUT_OF_RANGE, "seed vertex outside the roadmap");
      if (!(c[i] >= 0) || !std::isfinite(c[i])) return rfail(r, TR_ERR_INVALID_ARG, "seed costs must be finite and >= 0");
    }
  }
  for (int64_t q = 0; s.direct && q < n_queries; q++)
    if (!(s.direct[q] >= 0)) return rfail(r, TR_ERR_INVALID_ARG, "direct costs must be >= 0 (INFINITY: none)");
  RM_HIP(r, hipSetDevice(tr_device(r->ctx)));
  const RoadmapSwitches sw = read_switches();
  Laps laps(sw, "tr_roadmap_solve_seeded");
  const int T = host_threads(n_threads);
  if ((int)r->scratch.size() < T) r->scratch.resize((size_t)T);
  for (Scratch &sc : r->scratch) sc.trace = false;
  if (r->lm_n < 0 && n_queries >= 64) build_landmarks(r, 16, T, sw);
  std::vector<double> own_cost;
  if (!cost) { own_cost.resize((size_t)n_queries); cost = own_cost.data(); }
  Solve solve(r, nullptr, nullptr, n_queries, status, cost, sw, T, &s);
  return solve.run(laps, path_offsets, stats);
}

int solve_states_locked(tr_roadmap *r, const tr_space_params *sp, const tr_attach_params *params, const double *starts, const double *goals, int64_t n,
                        int32_t n_threads, int32_t *status, double *cost, int32_t *start_vertex, int32_t *goal_vertex, uint8_t *direct,
                        int32_t *src_pick, int32_t *dst_pick, int64_t *path_offsets, tr_roadmap_stats *stats) {
  auto &ph = r->dt.state_phase_ms;
  for (double &x : ph) x = 0;
  int k, rc;
  double max_distance;
  if ((rc = attach_params(r, params, 2 * n, k, max_distance))) return rc;
  if (n > 0 && (!starts || !goals || !status || !path_offsets)) return rfail(r, TR_ERR_INVALID_ARG, "bad argument");
  reset_last_solve(r, n);
  if (path_offsets) path_offsets[0] = 0;
  if (stats) *stats = tr_roadmap_stats{0, 0, 0, 0};
  if (n == 0) return TR_OK;
  const int S = r->S;
  const size_t m = (size_t)n * (size_t)k;
  // one attach pass: the starts OUT, the goals IN, the direct edges where the rule applies
  std::vector<double> rows((size_t)2 * n * S);
  std::memcpy(rows.data(), starts, (size_t)n * S * sizeof(double));
  std::memcpy(rows.data() + (size_t)n * S, goals, (size_t)n * S * sizeof(double));
  AttachBuffers b;
  if ((rc = attach_pass(r, sp ? *sp : kAttachSpace, k, max_distance, rows.data(), false, 2 * n, n, true, false, b, nullptr, nullptr, ph))) return rc;
  auto t0 = Clock::now();
  std::vector<uint8_t> valid((size_t)2 * n), ok(2 * m + (size_t)n);
  std::vector<int32_t> idx(2 * m);
  std::vector<double> dist(2 * m), ddist((size_t)n);
  RM_HIP(r, hipMemcpy(valid.data(), b.valid, valid.size(), hipMemcpyDeviceToHost));
  RM_HIP(r, hipMemcpy(ok.data(), b.ok, ok.size(), hipMemcpyDeviceToHost));
  RM_HIP(r, hipMemcpy(idx.data(), b.idx, idx.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  RM_HIP(r, hipMemcpy(dist.data(), b.dist, dist.size() * sizeof(double), hipMemcpyDeviceToHost));
  RM_HIP(r, hipMemcpy(ddist.data(), b.ddist, ddist.size() * sizeof(double), hipMemcpyDeviceToHost));
  // the seeds: the slots whose edge is valid, at their attach distance; slot[] maps a seed back to its slot
  std::vector<int64_t> off[2];
  std::vector<int32_t> sv[2], slot[2];
  std::vector<double> sc[2], dc((size_t)n);
  for (int side = 0; side < 2; side++) {
    off[side].assign((size_t)n + 1, 0);
    for (int64_t q = 0; q < n; q++) {
      const size_t row = ((size_t)side * n + (size_t)q) * k;
      for (int j = 0; j < k; j++)
        if (ok[row + j]) { sv[side].push_back(idx[row + j]); sc[side].push_back(dist[row + j]); slot[side].push_back(j); }
      off[side][(size_t)q + 1] = (int64_t)sv[side].size();
    }
  }
  for (int64_t q = 0; q < n; q++) dc[(size_t)q] = ok[2 * m + (size_t)q] ? ddist[(size_t)q] : std::numeric_limits<double>::infinity();
  std::vector<int32_t> sp_((size_t)n), dp_((size_t)n);
  std::vector<double> own_cost;
  if (!cost) { own_cost.resize((size_t)n); cost = own_cost.data(); }
  SeededQueries s{off[0].data(), sv[0].data(), sc[0].data(), off[1].data(), sv[1].data(), sc[1].data(), dc.data(), sp_.data(), dp_.data()};
  auto lap = [&](int phase) { const auto t1 = Clock::now(); ph[phase] += ms_between(t0, t1); t0 = t1; };
  lap(3);
  if ((rc = solve_seeded_locked(r, s, n, n_threads, status, cost, path_offsets, stats))) return rc;
  lap(2);
  // solvePrep only admits valid start / goal states (:2995-3010)
  for (int64_t q = 0; q < n; q++) {
    const bool bad_s = !valid[(size_t)q], bad_g = !valid[(size_t)n + (size_t)q];
    if (bad_s || bad_g) { status[q] = bad_s ? TR_QUERY_INVALID_START : TR_QUERY_INVALID_GOAL; cost[q] = std::numeric_limits<double>::infinity(); }
    const bool solved = status[q] == TR_QUERY_SOLVED;
    const int32_t a = solved ? sp_[(size_t)q] : -1, g = solved ? dp_[(size_t)q] : -1;
    if (start_vertex) start_vertex[q] = a >= 0 ? sv[0][(size_t)off[0][(size_t)q] + a] : -1;
    if (goal_vertex) goal_vertex[q] = g >= 0 ? sv[1][(size_t)off[1][(size_t)q] + g] : -1;
    if (src_pick) src_pick[q] = a >= 0 ? slot[0][(size_t)off[0][(size_t)q] + a] : -1;
    if (dst_pick) dst_pick[q] = g >= 0 ? slot[1][(size_t)off[1][(size_t)q] + g] : -1;
    if (direct) direct[q] = solved && a < 0;
  }
  lap(3);
  return TR_OK;
}

}  // namespace

extern "C" {

int tr_roadmap_attach_states(tr_roadmap *r, const tr_space_params *sp, const tr_attach_params *params, int32_t direction, const double *states,
                             int64_t n, uint8_t *valid, int32_t *vertices, double *cost, uint8_t *edge_ok, int32_t *n_fk, int64_t *n_domain_errors) {
  if (!r) return TR_ERR_INVALID_ARG;
  RmLock lock_(r);
  return attach_states_locked(r, sp, params, direction, states, n, false, valid, vertices, cost, edge_ok, n_fk, n_domain_errors);
}

int tr_roadmap_attach_states_dev(tr_roadmap *r, const tr_space_params *sp, const tr_attach_params *params, int32_t direction, const double *d_states,
                                 int64_t n, uint8_t *d_valid, int32_t *d_vertices, double *d_cost, uint8_t *d_edge_ok, int32_t *d_n_fk,
                                 int64_t *n_domain_errors) {
  if (!r) return TR_ERR_INVALID_ARG;
  RmLock lock_(r);
  return attach_states_locked(r, sp, params, direction, d_states, n, true, d_valid, d_vertices, d_cost, d_edge_ok, d_n_fk, n_domain_errors);
}

int tr_roadmap_solve_seeded(tr_roadmap *r, int64_t n_queries, const int64_t *src_offsets, const int32_t *src_vertices, const double *src_costs,
                            const int64_t *dst_offsets, const int32_t *dst_vertices, const double *dst_costs, const double *direct_cost,
                            int32_t n_threads, int32_t *status, double *cost, int32_t *src_pick, int32_t *dst_pick, int64_t *path_offsets,
                            tr_roadmap_stats *stats) {
  if (!r) return TR_ERR_INVALID_ARG;
  RmLock lock_(r);
  std::vector<int32_t> own_s, own_d;
  if (!src_pick && n_queries > 0) { own_s.resize((size_t)n_queries); src_pick = own_s.data(); }
  if (!dst_pick && n_queries > 0) { own_d.resize((size_t)n_queries); dst_pick = own_d.data(); }
  SeededQueries s{src_offsets, src_vertices, src_costs, dst_offsets, dst_vertices, dst_costs, direct_cost, src_pick, dst_pick};
  return solve_seeded_locked(r, s, n_queries, n_threads, status, cost, path_offsets, stats);
}

int tr_roadmap_solve_states(tr_roadmap *r, const tr_space_params *sp, const tr_attach_params *params, const double *starts, const double *goals,
                            int64_t n, int32_t n_threads, int32_t *status, double *cost, int32_t *start_vertex, int32_t *goal_vertex,
                            uint8_t *direct, int32_t *src_pick, int32_t *dst_pick, int64_t *path_offsets, tr_roadmap_stats *stats) {
  if (!r) return TR_ERR_INVALID_ARG;
  RmLock lock_(r);
  return solve_states_locked(r, sp, params, starts, goals, n, n_threads, status, cost, start_vertex, goal_vertex, direct, src_pick, dst_pick,
                             path_offsets, stats);
}

int tr_roadmap_state_query_profile(tr_roadmap *r, double out[4]) {
  if (!r || !out) return TR_ERR_INVALID_ARG;
  RmLock lock_(r);
  for (int i = 0; i < 4; i++) out[i] = r->dt.state_phase_ms[i];
  return TR_OK;
}

}  // extern "C"
