// loaded_roadmap_host.inc -- the roadmap build on loaded shapes: createRoadmap's vertex phase (tr_sample_valid_vertices_loaded*),
// voxelizeVertex (tr_voxelize_batch_loaded) and the indexed voxelize / connect forms (tr_voxelize_edges_loaded_indexed,
// tr_connect_edges_loaded_indexed) with every shape taken from the loaded FK.  In the reference set_fk_func(general_shape ...) changes
// all of these loops at once, because they go through voxelStateChecker_->fk (motion-planning/VoxelCachedLazyPRM.cpp:1415-1439,
// 2803-2837, 2879-2902).
//
// Every vertex is solved cold, and a cold solve does not depend on the rest of its call: a vertex has the same strains, points and tip
// in the vertex phase, in tr_voxelize_batch_loaded, as an end state of the indexed edge calls and in tr_fk_loaded_batch.  Nothing is
// handed over between the phases.
//
// The evaluator is LoadedEdges (loaded_edges_host.inc): loads -> shooting -> K2 on the stored planes; the edge forms run the EdgeRun
// with it and `vox` set.  Null stream, one lane: the shooting workspace is one per context.
// Included at the end of tendon_hip.hip (needs loaded_edges_host.inc and sample_host.inc).
namespace {

// what the calls without a state space check after their own arguments, in loaded_edges_begin's order: the load set, the robot, the
// solver's parameters, an empty call, the grid
int loaded_states_begin(tr_ctx *c, const tr_shoot_params *shoot, const tr_edge_loads *loads, int64_t n, LoadedEdges &le, bool &empty) {
  empty = false;
  int rc;
  le.c = c;
  if ((rc = parse_loads(c, loads, le.loads))) return rc;
  le.warm = false;                             // every vertex is solved cold
  if ((rc = shoot_check(c, n, 0, 0)) || (rc = refuse_retraction(c, "loaded roadmap builds (tr_sample_valid_vertices_loaded*, tr_voxelize_batch_loaded)"))) return rc;
  if ((rc = shoot_params(c, shoot, le.prm))) return rc;
  if (n == 0) { empty = true; return TR_OK; }
  if (!c->has_grid) return fail(c, TR_ERR_INVALID_ARG, "no obstacle grid set (tr_set_grid)");
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipDeviceSynchronize());          // the workspaces are shared with *_dev calls that may still run on other streams
  return TR_OK;
}

// the tips of workspace columns [0, m) into d_tips [m][3]
int loaded_tips(tr_ctx *c, int64_t m, double *d_tips) {
  const Workspace &w = c->ws;
  ProfScope ps(c, 3, nullptr);
  hipLaunchKernelGGL(trk::loaded_tip_rows, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, nullptr, (const double *)w.px, (const double *)w.py,
                     (const double *)w.pz, w.ld, (int)c->K.n_points - 1, m, d_tips);
  HIP_TRY(c, hipGetLastError());
  return TR_OK;
}

// The rejection loop on loaded shapes.  Outputs are device arrays (the context's own when the caller passes no d_states_out).
int sample_valid_loaded_impl(tr_ctx *c, const tr_shoot_params *shoot, const tr_edge_loads *loads, uint64_t seed, uint64_t first, const double *lo,
                             const double *hi, int64_t n_want, int64_t max_candidates, double *d_states_out, double *d_tips_out,
                             int64_t *d_index_out, double *d_vu_out, int64_t *n_accepted, int64_t *n_tried, int64_t *n_unconverged,
                             int64_t *n_integrations) {
  if (n_accepted) *n_accepted = 0;
  if (n_tried) *n_tried = 0;
  if (n_unconverged) *n_unconverged = 0;
  if (n_integrations) *n_integrations = 0;
  if (n_want < 0) return fail(c, TR_ERR_INVALID_ARG, "negative vertex count");
  LoadedEdges le{};
  bool empty;
  int rc;
  if ((rc = loaded_states_begin(c, shoot, loads, n_want, le, empty)) || empty) return rc;
  trk::SampleBox box;
  if ((rc = sample_box(c, lo, hi, box))) return rc;
  if (max_candidates <= 0) max_candidates = 64 * n_want + ((int64_t)1 << 20);
  tr_ctx::Sampler &sm = c->samp;
  tr_ctx::LoadedEdgeDev &ld = c->ledge;
  const bool own = d_states_out == nullptr;
  if (ld.out_cap < n_want) {
    ld.out.release();
    ld.out_cap = 0;
    if ((rc = ld.out.alloc(c, &ld.out_vu, (size_t)n_want * 6)) || (rc = ld.out.alloc(c, &ld.out_index, (size_t)n_want))) return rc;
    ld.out_cap = n_want;
  }
  if (!ld.vtally && (rc = ld.once.alloc(c, &ld.vtally, 2))) return rc;
  // a batch lives in the point workspace: what is still missing over the acceptance rate seen so far, 3 % + 512 on top, whole waves
  const int64_t kMaxBatch = c->loaded_vertex_batch > 0 ? c->loaded_vertex_batch : (int64_t)1 << 16;
  double rate = ld.rate_seen > 0.0 ? ld.rate_seen : 1.0;
  int64_t have = 0, tried = 0, pos = 0;
  const int S = c->K.state_size;
  const int sample_test = c->checker == TR_CHECKER_SPHERES ? 2 : 1;
  const dim3 th(256);
  auto blocks = [](int64_t n) { return dim3((unsigned)((n + 255) / 256)); };
  bool first_batch = true;
  ld.n_vertices = 0;                           // rows of vu_pool are the batches' from here on
  while (have < n_want && pos < max_candidates) {
    const int64_t need = n_want - have;
    int64_t m = (int64_t)std::ceil((double)need / std::max(rate, 1e-3) * 1.03) + 512;
    m = std::min<int64_t>({round_up(m, 64), kMaxBatch, max_candidates - pos});
    if ((rc = ensure_workspace(c, std::min<int64_t>(c->max_chunk, round_up(m, 64))))) return rc;
    const int64_t cap = c->ws.ld;
    m = std::min(m, cap);
    if ((rc = ensure_sample_scratch(c, round_up(m, 64), std::max<int64_t>(sm.out_cap, own ? n_want : 1)))) return rc;
    if ((rc = le.reserve(cap)) || (rc = ensure_edge_dev(c, cap))) return rc;
    double *so = own ? sm.out_states : d_states_out;
    double *to = own ? sm.out_tips : d_tips_out;
    int64_t *io = own ? sm.out_index : (d_index_out ? d_index_out : ld.out_index);
    double *vo = own ? ld.out_vu : d_vu_out;
    if (first_batch) {
      HIP_TRY(c, hipMemsetAsync(sm.d_ctr, 0, sizeof(trk::SampleCounters), nullptr));
      HIP_TRY(c, hipMemsetAsync(ld.vtally, 0, 2 * sizeof(unsigned long long), nullptr));
      if ((rc = le.clear_tally())) return rc;
      first_batch = false;
    }
    const uint64_t index_base = first + (uint64_t)pos;
    {
      ProfScope ps(c, 3, nullptr);
      trk::launch_candidate_states(seed, index_base, m, box, sm.states, nullptr);
      HIP_TRY(c, hipGetLastError());
    }
    if ((rc = le.samples(sm.states, 0, m, nullptr, sample_test))) return rc;
    if ((rc = loaded_tips(c, m, sm.tips))) return rc;
    {
      ProfScope ps(c, 3, nullptr);
      trk::launch_compact_rows(c->edge.bits, m, index_base, sm.states, S, sm.tips, n_want, so, to, io, sm.d_ctr, sm.wprefix, nullptr);
      if (vo) hipLaunchKernelGGL(trk::loaded_gather_strains, blocks(need * 6), th, 0, nullptr, (const int64_t *)io, (const unsigned long long *)&sm.d_ctr->have, have,
                                 need, index_base, m, (const double *)ld.vu_pool, vo);
      hipLaunchKernelGGL(trk::loaded_vertex_tally, blocks(m), th, 0, nullptr, (const uint8_t *)c->ws.conv, (const int32_t *)ld.calls, m, index_base,
                         (const unsigned long long *)&sm.d_ctr->tried, ld.vtally);
      HIP_TRY(c, hipGetLastError());
    }
    HIP_TRY(c, hipMemcpyAsync(sm.h_ctr, sm.d_ctr, sizeof(trk::SampleCounters), hipMemcpyDeviceToHost, nullptr));
    HIP_TRY(c, hipStreamSynchronize(nullptr));
    have = (int64_t)sm.h_ctr->have;
    tried = (int64_t)(sm.h_ctr->tried - first);
    pos += m;
    const double seen = have < n_want ? (double)pos : (double)tried;
    if (seen > 0) rate = std::max((double)have / seen, 1e-3);
  }
  if (have > 0) ld.rate_seen = rate;
  unsigned long long h[2] = {0, 0};
  HIP_TRY(c, hipMemcpy(h, ld.vtally, sizeof(h), hipMemcpyDeviceToHost));
  le.note();
  if (n_accepted) *n_accepted = have;
  if (n_tried) *n_tried = tried;
  if (n_unconverged) *n_unconverged = (int64_t)h[0];
  if (n_integrations) *n_integrations = (int64_t)h[1];
  return TR_OK;
}

// tr_voxelize_edges_indexed (collide = false) or tr_connect_edges_indexed (true) on loaded samples
int voxelize_edges_loaded_indexed_impl(tr_ctx *c, const tr_space_params *sp, const tr_shoot_params *shoot, const tr_edge_loads *loads,
                                       const double *states, int64_t n_states, const int32_t *edges, int64_t n_edges, int64_t *offsets,
                                       uint64_t *fully_valid_bits, int32_t *n_fk, int64_t *n_unconverged, int64_t *n_integrations, bool collide) {
  if (!c) return TR_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lock_(c->mu);
  int64_t nd = 0, nu = 0, ni = 0;
  if (n_unconverged) *n_unconverged = 0;
  if (n_integrations) *n_integrations = 0;
  if (n_edges < 0 || n_states < 0 || (n_edges > 0 && (!sp || !states || !edges || !offsets || !fully_valid_bits)))
    return fail(c, TR_ERR_INVALID_ARG, "bad argument");
  c->vstore.n = 0;
  if (offsets) offsets[0] = 0;
  LoadedEdges le{};
  bool empty;
  int rc;
  if ((rc = loaded_edges_begin(c, sp, shoot, loads, n_edges, le, empty, /*voxel_form=*/true)) || empty) return rc;
  if ((rc = check_edge_indices(c, edges, n_edges, n_states))) return rc;
  if ((rc = ensure_edge_pool(c, n_edges + n_states / 8))) return rc;
  const int S = c->K.state_size;
  const int64_t cap = c->ws.ld, Vp = round_up(n_states, 64);
  if ((rc = le.reserve(cap)) || (rc = ensure_edge_dev(c, cap)) || (rc = ensure_vox_scratch(c, cap))) return rc;
  std::vector<uint8_t> ok((size_t)n_edges, 1);
  std::vector<int32_t> nfk((size_t)n_edges, 0);
  EdgeVoxOut vox;
  vox.count.assign((size_t)n_edges, 0);
  vox.collide = collide;
  le.vox = &vox;
  c->ledge.n_vertices = 0;
  if (Vp > cap / 2) {
    // more vertices than half the sample pool: gather on the host; every edge then solves its own two ends (cold, so the same shapes)
    std::vector<double> a((size_t)n_edges * S), b((size_t)n_edges * S);
    for (int64_t k = 0; k < n_edges; k++) {
      std::memcpy(&a[(size_t)k * S], states + (size_t)edges[2 * k] * S, S * sizeof(double));
      std::memcpy(&b[(size_t)k * S], states + (size_t)edges[2 * k + 1] * S, S * sizeof(double));
    }
    if ((rc = for_edge_chunks(n_edges, cap, 9.0, 0, nfk, [&](int64_t e0, int64_t e1) {
          return le.range(sp, a.data(), b.data(), e0, e1, ok, nfk, &nd, nullptr, nullptr, &nu, &ni); }))) return rc;
  } else {
    EdgeDev &d = c->edge;
    Workspace &w = c->ws;
    EdgeIndexed ix{};
    if ((rc = upload_indexed_inputs(c, states, n_states, edges, n_edges, false, &ix))) return rc;
    HIP_TRY(c, hipMemsetAsync(d.sample_edge, 0xff, (size_t)cap * sizeof(int32_t), nullptr));
    // every vertex once, cold: pool slots [0, n_states), then its block list
    if ((rc = le.clear_tally()) || (rc = le.samples(ix.d_states, 0, n_states, nullptr, collide ? 1 : 0)) || (rc = le.add_tally(&nu, &ni))) return rc;
    {
      ProfScope ps(c, 3, nullptr);
      hipLaunchKernelGGL(trk::backbone_voxelize, dim3((unsigned)((n_states + 63) / 64)), dim3(64), 0, nullptr, w.px, w.py, w.pz, (const int32_t *)nullptr,
                         d.bits, n_states, cap, (int)c->K.n_points, c->G, vox_max_blocks(c), c->d_vids, c->d_vmasks, c->d_vcounts);
      HIP_TRY(c, hipGetLastError());
    }
    c->ledge.n_vertices = n_states;            // (the edges' samples live behind the vertex block: its rows of vu_pool stay)
    if ((rc = for_edge_chunks(n_edges, cap - Vp, 6.0, 2, nfk, [&](int64_t e0, int64_t e1) {
          return le.range(sp, nullptr, nullptr, e0, e1, ok, nfk, &nd, nullptr, &ix, &nu, &ni); }))) return rc;
  }
  pack_edge_results(ok, nfk, fully_valid_bits, n_fk, &vox.count, offsets);
  le.note();
  if (n_unconverged) *n_unconverged = nu;
  if (n_integrations) *n_integrations = ni;
  return TR_OK;
}

// tr_fk_loaded_tips*'s body: n device states under per-state (or one, ld = 0) load rows, solved by shoot_chunk_solve into the point
// workspace a chunk at a time -- planes exist for one chunk only -- and loaded_tip_rows on each chunk.  Null stream; ends synchronised.
int loaded_tips_run(tr_ctx *c, const trk::ShootParams &prm, const double *d_states, int64_t n, const double *d_wrench, int64_t wrench_ld,
                    const double *d_dist, int64_t dist_ld, const double *d_guess, double *d_tips, uint8_t *d_conv, double *d_vu0,
                    int64_t *rounds_out) {
  LoadedEdges le{};
  le.c = c;
  le.prm = prm;
  int rc;
  const int64_t chunk = std::min<int64_t>(shoot_chunk_size(c), std::min<int64_t>(c->max_chunk, (int64_t)1 << 16));
  if ((rc = ensure_workspace(c, std::min(n, chunk)))) return rc;
  const int64_t cap = c->ws.ld;
  if ((rc = le.reserve(cap)) || (rc = le.clear_tally())) return rc;
  const int S = c->K.state_size;
  int64_t rounds = 0, nu = 0, ni = 0;
  for (int64_t off = 0; off < n; off += chunk) {
    const int64_t m = std::min(chunk, n - off);
    uint8_t *conv = d_conv ? d_conv + off : c->ws.conv;
    // (one chunk of the shooting's: m <= shoot_chunk_size; a robot with retraction: the chunk in the order of its backbone lengths)
    if ((rc = shoot_run(c, prm, d_states + off * S, m, cap, d_wrench ? d_wrench + off * wrench_ld : nullptr, wrench_ld,
                        rows_at(d_dist, off, dist_ld), dist_ld, rows_at(d_guess, off, 6), ws_fk_out(c, 0), conv, rows_at(d_vu0, off, 6),
                        nullptr, nullptr, nullptr, c->ledge.calls, nullptr, rounds))) return rc;
    {
      ProfScope ps(c, 3, nullptr);
      hipLaunchKernelGGL(trk::loaded_sample_tally, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, nullptr, (const uint8_t *)conv,
                         (const int32_t *)c->ledge.calls, m, c->ledge.tally);
      HIP_TRY(c, hipGetLastError());
    }
    if (d_tips && (rc = loaded_tips(c, m, d_tips + off * 3))) return rc;
  }
  if ((rc = le.add_tally(&nu, &ni))) return rc;                          // (synchronises the null stream)
  if (rounds_out) { rounds_out[0] = rounds; rounds_out[1] = ni; }
  return TR_OK;
}

}  // namespace

extern "C" {

int tr_fk_loaded_tips_dev(tr_ctx *c, const tr_shoot_params *shoot, const double *d_states, int64_t n, const double *d_wrench, int64_t wrench_ld,
                          const double *d_dist, int64_t dist_ld, const double *d_guess, double *d_tips, uint8_t *d_converged, double *d_vu0,
                          int64_t *rounds_out, void *stream) {
  if (!c) return TR_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lock_(c->mu);
  if (rounds_out) rounds_out[0] = rounds_out[1] = 0;
  int rc;
  if ((rc = shoot_check(c, n, wrench_ld, dist_ld))) return rc;
  trk::ShootParams prm;
  if ((rc = shoot_params(c, shoot, prm))) return rc;
  if (n == 0) return TR_OK;
  if (!d_states) return fail(c, TR_ERR_INVALID_ARG, "null device pointer");
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipDeviceSynchronize());          // the run is the null stream's; the workspaces are shared with *_dev calls on other streams
  if ((rc = loaded_tips_run(c, prm, d_states, n, d_wrench, wrench_ld, d_dist, dist_ld, d_guess, d_tips, d_converged, d_vu0, rounds_out))) return rc;
  return note_dev_work(c, (hipStream_t)stream);
}

int tr_fk_loaded_tips(tr_ctx *c, const tr_shoot_params *shoot, const double *states, int64_t n, const double *wrench, int64_t wrench_ld,
                      const double *dist, int64_t dist_ld, const double *guess, double *tips, uint8_t *converged, double *vu0,
                      int64_t *rounds_out) {
  if (!c) return TR_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lock_(c->mu);
  if (rounds_out) rounds_out[0] = rounds_out[1] = 0;
  int rc;
  if ((rc = shoot_check(c, n, wrench_ld, dist_ld))) return rc;
  trk::ShootParams prm;
  if ((rc = shoot_params(c, shoot, prm))) return rc;
  if (n == 0) return TR_OK;
  if (!states) return fail(c, TR_ERR_INVALID_ARG, "bad argument");
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipDeviceSynchronize());
  const int S = c->K.state_size;
  const int64_t chunk = shoot_io_chunk(c);       // the staging of tr_fk_loaded_batch: states, load rows, guess, strains, flags
  if ((rc = shoot_reserve_io(c, n, false)) || (rc = ensure_staging(c, std::min(n, chunk)))) return rc;
  tr_ctx::ShootDev &k = c->shoot;
  int64_t rounds[2] = {0, 0};
  for (int64_t off = 0; off < n; off += chunk) {
    const int64_t m = std::min(chunk, n - off);
    int64_t r2[2] = {0, 0};
    if ((rc = upload_rows(c, k.io_states, states, S, off, m, S))) return rc;
    if (wrench && (rc = upload_rows(c, k.io_w, wrench, wrench_ld, off, m, 6))) return rc;
    if (dist && (rc = upload_rows(c, k.io_d, dist, dist_ld, off, m, 6))) return rc;
    if (guess && (rc = upload_rows(c, k.io_g, guess, 6, off, m, 6))) return rc;
    if ((rc = loaded_tips_run(c, prm, k.io_states, m, wrench ? k.io_w : nullptr, wrench_ld ? 6 : 0, dist ? k.io_d : nullptr, dist_ld ? 6 : 0,
                              guess ? k.io_g : nullptr, c->ws.tips, k.io_conv, k.io_vu, r2))) return rc;
    rounds[0] += r2[0]; rounds[1] += r2[1];
    if (tips) HIP_TRY(c, hipMemcpy(tips + 3 * off, c->ws.tips, (size_t)m * 3 * sizeof(double), hipMemcpyDeviceToHost));
    if ((rc = download_rows(c, converged, k.io_conv, off, m)) || (rc = download_rows(c, vu0, k.io_vu, off, m, 6))) return rc;
  }
  if (rounds_out) { rounds_out[0] = rounds[0]; rounds_out[1] = rounds[1]; }
  return TR_OK;
}

int tr_sample_valid_vertices_loaded_dev(tr_ctx *c, const tr_shoot_params *shoot, const tr_edge_loads *loads, uint64_t seed, uint64_t first_candidate,
                                        const double *lo, const double *hi, int64_t n_want, int64_t max_candidates, double *d_states, double *d_tips,
                                        int64_t *d_index, double *d_vu0, int64_t *n_accepted, int64_t *n_tried, int64_t *n_unconverged,
                                        int64_t *n_integrations, void *stream) {
  if (!c) return TR_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lock_(c->mu);
  if ((n_want > 0 && !d_states) || (!lo != !hi)) return fail(c, TR_ERR_INVALID_ARG, "bad argument");
  // the run is the null stream's and ends synchronised: the caller's stream only has to be drained before it (loaded_states_begin)
  const int rc = sample_valid_loaded_impl(c, shoot, loads, seed, first_candidate, lo, hi, n_want, max_candidates, d_states, d_tips, d_index, d_vu0,
                                          n_accepted, n_tried, n_unconverged, n_integrations);
  if (rc || n_want == 0) return rc;
  return note_dev_work(c, (hipStream_t)stream);
}

int tr_sample_valid_vertices_loaded(tr_ctx *c, const tr_shoot_params *shoot, const tr_edge_loads *loads, uint64_t seed, uint64_t first_candidate,
                                    const double *lo, const double *hi, int64_t n_want, int64_t max_candidates, double *states, double *tips,
                                    int64_t *index, double *vu0, int64_t *n_accepted, int64_t *n_tried, int64_t *n_unconverged,
                                    int64_t *n_integrations) {
  if (!c) return TR_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lock_(c->mu);
  if ((n_want > 0 && !states) || (!lo != !hi)) return fail(c, TR_ERR_INVALID_ARG, "bad argument");
  int64_t have = 0;
  int rc;
  if ((rc = sample_valid_loaded_impl(c, shoot, loads, seed, first_candidate, lo, hi, n_want, max_candidates, nullptr, nullptr, nullptr, nullptr, &have,
                                     n_tried, n_unconverged, n_integrations))) return rc;
  if (n_accepted) *n_accepted = have;
  if (have > 0) {
    const size_t S = (size_t)c->K.state_size;
    HIP_TRY(c, hipMemcpy(states, c->samp.out_states, (size_t)have * S * sizeof(double), hipMemcpyDeviceToHost));
    if (tips) HIP_TRY(c, hipMemcpy(tips, c->samp.out_tips, (size_t)have * 3 * sizeof(double), hipMemcpyDeviceToHost));
    if (index) HIP_TRY(c, hipMemcpy(index, c->samp.out_index, (size_t)have * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (vu0) HIP_TRY(c, hipMemcpy(vu0, c->ledge.out_vu, (size_t)have * 6 * sizeof(double), hipMemcpyDeviceToHost));
  }
  return TR_OK;
}

int tr_voxelize_batch_loaded(tr_ctx *c, const tr_shoot_params *shoot, const tr_edge_loads *loads, const double *states, int64_t n, int64_t *offsets,
                             uint64_t *shape_valid_bits, double *tips, int64_t *n_unconverged, int64_t *n_integrations) {
  if (!c) return TR_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lock_(c->mu);
  int64_t nu = 0, ni = 0;
  if (n_unconverged) *n_unconverged = 0;
  if (n_integrations) *n_integrations = 0;
  if (n < 0 || (n > 0 && (!states || !offsets || !shape_valid_bits))) return fail(c, TR_ERR_INVALID_ARG, "bad argument");
  c->vstore.n = 0;
  if (offsets) offsets[0] = 0;
  LoadedEdges le{};
  bool empty;
  int rc;
  if ((rc = loaded_states_begin(c, shoot, loads, n, le, empty)) || empty) return rc;
  const int64_t chunk = std::min<int64_t>(c->max_chunk, c->loaded_vertex_batch > 0 ? c->loaded_vertex_batch : (int64_t)1 << 16);
  if ((rc = ensure_workspace(c, std::min(n, chunk)))) return rc;
  const int64_t cap = c->ws.ld;
  if ((rc = ensure_staging(c, std::min(n, chunk))) || (rc = le.reserve(cap)) || (rc = ensure_edge_dev(c, cap)) || (rc = le.clear_tally())) return rc;
  Workspace &w = c->ws;
  EdgeDev &d = c->edge;
  const int S = c->K.state_size;
  c->ledge.n_vertices = 0;
  std::vector<int32_t> counts; std::vector<int64_t> offs;
  for (int64_t off = 0; off < n; off += chunk) {
    const int64_t m = std::min(chunk, n - off);
    if ((rc = upload_staged(c, w.states, states + off * S, (size_t)m * S * sizeof(double), nullptr))) return rc;
    if ((rc = le.samples(w.states, 0, m, nullptr, 0))) return rc;             // is_valid_shape only
    if (tips && (rc = loaded_tips(c, m, w.tips))) return rc;
    const int64_t base = c->vstore.n;
    if ((rc = voxelize_samples(c, m, cap, nullptr, d.bits, counts, offs))) return rc;
    HIP_TRY(c, hipMemcpy(shape_valid_bits + off / 64, d.bits, (size_t)((m + 63) / 64) * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (tips) HIP_TRY(c, hipMemcpy(tips + 3 * off, w.tips, (size_t)m * 3 * sizeof(double), hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < m; i++) offsets[off + i + 1] = base + offs[(size_t)i + 1];
  }
  if ((rc = le.add_tally(&nu, &ni))) return rc;
  le.note();
  if (n_unconverged) *n_unconverged = nu;
  if (n_integrations) *n_integrations = ni;
  return TR_OK;
}

int tr_voxelize_edges_loaded_indexed(tr_ctx *c, const tr_space_params *sp, const tr_shoot_params *shoot, const tr_edge_loads *loads,
                                     const double *states, int64_t n_states, const int32_t *edges, int64_t n_edges, int64_t *offsets,
                                     uint64_t *fully_valid_bits, int32_t *n_fk, int64_t *n_unconverged, int64_t *n_integrations) {
  return voxelize_edges_loaded_indexed_impl(c, sp, shoot, loads, states, n_states, edges, n_edges, offsets, fully_valid_bits, n_fk, n_unconverged,
                                            n_integrations, false);
}

int tr_connect_edges_loaded_indexed(tr_ctx *c, const tr_space_params *sp, const tr_shoot_params *shoot, const tr_edge_loads *loads,
                                    const double *states, int64_t n_states, const int32_t *edges, int64_t n_edges, int64_t *offsets,
                                    uint64_t *valid_bits, int32_t *n_fk, int64_t *n_unconverged, int64_t *n_integrations) {
  return voxelize_edges_loaded_indexed_impl(c, sp, shoot, loads, states, n_states, edges, n_edges, offsets, valid_bits, n_fk, n_unconverged,
                                            n_integrations, true);
}

}  // extern "C"
