// loaded_edges_host.inc -- checkMotion on loaded shapes (tr_validate_edges_loaded, tr_validate_edges_loaded_indexed): the level-
// synchronous bisection of edge_run_host.inc with every FK sample taken from the loaded FK, as the reference's motion validator
// does once AbstractValidityChecker::set_fk_func has put TendonRobot::general_shape in the checker's place of fk(state)
// (motion-planning/VoxelBackboneMotionValidator.cpp:25, apps/profile_chained_plan.cpp:407-451).
//
// EdgeRun::run_samples is the one place that evaluates samples; a LoadedEdges object is its evaluator.  Per level:
//   loaded_sample_loads  -> the level's wrench / distributed-load rows (frame BASE: the call's; WORLD: turned by Rz(-theta))
//   loaded_sample_guess  -> with warm start, the start strains of a midpoint = the accepted base strains of its interval's sample
//                           at t_a, from vu_pool (level 0 and the indexed form's vertices start cold)
//   shoot_run            -> over the level in chunks of shoot_chunk_size: points and L_i into the pool's workspace columns, the
//                           shooting's converged flag into the column K2 reads, the accepted strains into vu_pool
//   launch_sweep         -> K2 on the stored planes with the sample test the run chose (+ the sphere test under that checker)
// A sample whose shooting does not converge is an invalid sample (is_valid_shape rejects res.converged == false), never an error.
// The run lives in the point workspace (slots_only = false), compares stored points (sig = nullptr), and stays on one lane and the
// null stream: the shooting workspace is one per context.
// Included at the end of tendon_hip.hip (needs edge_run_host.inc, edge_pairs_host.inc and loaded_host.inc).
namespace {

struct LoadedEdges {
  tr_ctx *c; trk::ShootParams prm; trk::EdgeLoadsK loads; bool warm;
  int64_t rounds = 0;                  // Levenberg-Marquardt rounds of all solves (one host synchronisation each)
  int64_t n_samples = 0, n_levels = 0, n_chunks = 0;     // evaluated (retried chunks included), evaluator calls, chunk attempts
  EdgeVoxOut *vox = nullptr;           // the voxelize / connect forms (loaded_roadmap_host.inc): the run's vox branch on the workspace planes

  // what tr_edges_loaded_last reports
  void note() {
    int64_t *q = c->ledge.last;
    q[0] = n_samples; q[1] = n_levels; q[2] = rounds; q[3] = n_chunks;
  }

  int reserve(int64_t cap) {
    tr_ctx::LoadedEdgeDev &le = c->ledge;
    int rc;
    if (!le.tally && (rc = le.once.alloc(c, &le.tally, 2))) return rc;
    if (le.cap < cap) {
      HIP_TRY(c, hipDeviceSynchronize());
      DevOwner &o = le.pool;
      o.release();
      le.cap = 0;
      if ((rc = o.alloc(c, &le.vu_pool, (size_t)cap * 6)) || (rc = o.alloc(c, &le.w, (size_t)cap * 6)) ||
          (rc = o.alloc(c, &le.d, (size_t)cap * 6)) || (rc = o.alloc(c, &le.g, (size_t)cap * 6)) ||
          (rc = o.alloc(c, &le.calls, (size_t)cap))) return rc;
      le.cap = cap;
    }
    return shoot_reserve(c, cap);
  }

  int clear_tally() {
    HIP_TRY(c, hipMemsetAsync(c->ledge.tally, 0, 2 * sizeof(unsigned long long), nullptr));
    return TR_OK;
  }
  int add_tally(int64_t *n_unconverged, int64_t *n_integrations) {      // synchronises the null stream
    unsigned long long h[2] = {0, 0};
    HIP_TRY(c, hipMemcpy(h, c->ledge.tally, sizeof(h), hipMemcpyDeviceToHost));
    *n_unconverged += (int64_t)h[0]; *n_integrations += (int64_t)h[1];
    return TR_OK;
  }

  // the m states -> pool samples [s0, s0 + m): loaded FK into the workspace columns, K2 verdicts into bits.  `open`: the level's
  // intervals (null: cold start)
  int samples(const double *d_states, int64_t s0, int64_t m, const trk::EdgeIv *open, int sample_test) {
    if (m <= 0) return TR_OK;
    n_samples += m; n_levels++;
    tr_ctx::LoadedEdgeDev &le = c->ledge;
    EdgeDev &d = c->edge;
    const int S = c->K.state_size;
    const int64_t cap = c->ws.ld;
    if (s0 + m > cap || m > le.cap || (s0 & 63)) return fail(c, TR_ERR_RUNTIME, "loaded edges: samples beyond the point workspace");
    const dim3 th(256);
    auto blocks = [](int64_t n) { return dim3((unsigned)((n + 255) / 256)); };
    int rc;
    {
      ProfScope ps(c, 3, nullptr);
      hipLaunchKernelGGL(trk::loaded_sample_loads, blocks(m), th, 0, nullptr, d_states, m, S, c->K.enable_rotation ? c->K.n_tendons : -1, loads, le.w, le.d);
      const bool guess = warm && open != nullptr;
      if (guess) hipLaunchKernelGGL(trk::loaded_sample_guess, blocks(m * 6), th, 0, nullptr, open, m, cap, (const double *)le.vu_pool, le.g);
      HIP_TRY(c, hipGetLastError());
    }
    const bool guess = warm && open != nullptr;
    // (in chunks of shoot_chunk_size; a robot with retraction: the level's samples in the order of their backbone lengths, shoot_run)
    if ((rc = shoot_run(c, prm, d_states, m, cap, le.w, 6, le.d, 6, guess ? le.g : nullptr, ws_fk_out(c, s0), c->ws.conv + s0,
                        le.vu_pool + s0 * 6, nullptr, nullptr, nullptr, le.calls, nullptr, rounds))) return rc;
    {
      ProfScope ps(c, 3, nullptr);
      hipLaunchKernelGGL(trk::loaded_sample_tally, blocks(m), th, 0, nullptr, (const uint8_t *)(c->ws.conv + s0), (const int32_t *)le.calls, m, le.tally);
      HIP_TRY(c, hipGetLastError());
    }
    if (sample_test == 2 && (rc = ensure_sphere_near(c, nullptr))) return rc;
    const trk::SweepIn in = ws_sweep_in(c, s0);
    if ((rc = launch_sweep(c, in, m, cap, sample_test == 1 ? 1 : 0, d.bits + s0 / 64, nullptr, nullptr))) return rc;
    if (sample_test == 2) {
      ProfScope ps(c, 3, nullptr);
      hipLaunchKernelGGL(trk::spheres_vs_grid, dim3((unsigned)((m + 63) / 64)), dim3(64), 0, nullptr, in.px, in.py, in.pz, in.n_points, m, cap,
                         (int)c->K.n_points, c->K.radius, c->G, c->d_grid, c->d_sph_near, d.bits + s0 / 64, (uint8_t *)nullptr);
      HIP_TRY(c, hipGetLastError());
    }
    return TR_OK;
  }

  // One chunk of edges on the whole workspace and the null stream; its tally joins the call's only when the chunk went through
  int chunk(const tr_space_params *sp, const double *A, const double *B, int64_t e0, int64_t e1, std::vector<uint8_t> &ok,
            std::vector<int32_t> &nfk, int64_t *nd, double *last_valid, const EdgeIndexed *ix, int64_t *n_unconverged, int64_t *n_integrations) {
    int rc;
    n_chunks++;
    if ((rc = ensure_edge_dev(c, c->ws.ld)) || (rc = ensure_edge_lanes(c)) || (rc = clear_tally())) return rc;
    EdgeRun r{c, sp, A, B, e0, e1, &ok, &nfk, nd, vox, last_valid, ix};
    r.L = EdgeLane{nullptr, 0, ix ? ix->pool_base : 0, c->ws.ld, 0, 0, c->lane[0].counters, c->lane[0].hc};
    r.eval = [this](EdgeRun &run, int64_t s0, int64_t m) {
      return samples(run.lvl_states, s0, m, s0 == 0 ? nullptr : run.open, run.sample_test);      // (s0 == 0: the end states of pairwise edges)
    };
    int stt = r.start();
    while (stt == EDGE_MORE) {
      HIP_TRY(c, hipStreamSynchronize(nullptr));
      stt = r.resume();
    }
    if (stt == TR_OK) stt = add_tally(n_unconverged, n_integrations);
    return stt;
  }

  // ... retried with fewer edges when the pool overflows, like edges_range
  int range(const tr_space_params *sp, const double *A, const double *B, int64_t e0, int64_t e1, std::vector<uint8_t> &ok,
            std::vector<int32_t> &nfk, int64_t *n_domain, double *last_valid, const EdgeIndexed *ix, int64_t *n_unconverged, int64_t *n_integrations) {
    for (int64_t e = e0; e < e1; e++) { ok[(size_t)e] = 1; nfk[(size_t)e] = 0; }
    int64_t nd = 0;
    const int64_t vox_mark = c->vstore.n;
    int rc = chunk(sp, A, B, e0, e1, ok, nfk, &nd, last_valid, ix, n_unconverged, n_integrations);
    if (rc == EDGE_OVERFLOW) {
      if (vox) c->vstore.n = vox_mark;
      if (e1 - e0 <= 1) return fail(c, TR_ERR_RUNTIME, "an edge needs more FK samples than the workspace holds");
      const int64_t mid = e0 + (e1 - e0) / 2;
      if ((rc = range(sp, A, B, e0, mid, ok, nfk, n_domain, last_valid, ix, n_unconverged, n_integrations))) return rc;
      return range(sp, A, B, mid, e1, ok, nfk, n_domain, last_valid, ix, n_unconverged, n_integrations);
    }
    if (rc == TR_OK && n_domain) *n_domain += nd;
    return rc;
  }
};

// what both entry points check after their own arguments, in this order: the load set, the robot, an empty call, the grid and the
// space's resolutions (edge_call_begin).  A robot with retraction: the verdict calls take it on a context opened with
// TR_LOADED_RETRACTION_EDGES -- the run's evaluator writes through ws_fk_out / ws_sweep_in (point counts and per-sample home lengths)
// and the interval test reads the stored point counts (EdgeRun::filter_np = ws.np), the path of the unloaded voxelize forms of such a
// robot; `voxel_form` (the voxelize / connect forms) keeps refusing at every level, under its own name at that one.
int loaded_edges_begin(tr_ctx *c, const tr_space_params *sp, const tr_shoot_params *shoot, const tr_edge_loads *loads, int64_t n_edges,
                       LoadedEdges &le, bool &empty, bool voxel_form = false) {
  empty = false;
  int rc;
  le.c = c;
  if ((rc = parse_loads(c, loads, le.loads))) return rc;
  le.warm = loads && loads->warm_start != 0;
  if ((rc = shoot_check(c, n_edges, 0, 0))) return rc;
  if (c->loaded_retraction != TR_LOADED_RETRACTION_EDGES)
    rc = refuse_retraction(c, "loaded edges (tr_validate_edges_loaded*, tr_*_edges_loaded_indexed)");
  else if (voxel_form)
    rc = refuse_retraction(c, "loaded voxel forms of the edges (tr_voxelize_edges_loaded_indexed, tr_connect_edges_loaded_indexed)");
  if (rc) return rc;
  if ((rc = shoot_params(c, shoot, le.prm))) return rc;
  if (n_edges == 0) { empty = true; return TR_OK; }
  if ((rc = edge_call_begin(c, sp))) return rc;
  c->edge_slots_now = 0;                       // the pool is the point workspace
  return TR_OK;
}

int validate_edges_loaded_impl(tr_ctx *c, const tr_space_params *sp, const tr_shoot_params *shoot, const tr_edge_loads *loads, const double *a,
                               const double *b, int64_t n_edges, uint64_t *valid_bits, double *last_valid_t, int32_t *n_fk,
                               int64_t *n_domain_errors, int64_t *n_unconverged, int64_t *n_integrations) {
  int64_t nd = 0, nu = 0, ni = 0;
  if (n_domain_errors) *n_domain_errors = 0;
  if (n_unconverged) *n_unconverged = 0;
  if (n_integrations) *n_integrations = 0;
  if (n_edges < 0 || (n_edges > 0 && (!sp || !a || !b || !valid_bits))) return fail(c, TR_ERR_INVALID_ARG, "bad argument");
  LoadedEdges le{};
  bool empty;
  int rc;
  if ((rc = loaded_edges_begin(c, sp, shoot, loads, n_edges, le, empty)) || empty) return rc;
  if ((rc = ensure_edge_pool(c, n_edges)) || (rc = le.reserve(c->ws.ld))) return rc;
  c->ledge.n_vertices = 0;                     // pool slots [0, ...) are the edges' own from here on
  std::vector<uint8_t> ok((size_t)n_edges, 1);
  std::vector<int32_t> nfk((size_t)n_edges, 0);
  if ((rc = for_edge_chunks(n_edges, c->ws.ld, 9.0, 0, nfk, [&](int64_t e0, int64_t e1) {
        return le.range(sp, a, b, e0, e1, ok, nfk, &nd, last_valid_t, nullptr, &nu, &ni); }))) return rc;
  pack_edge_results(ok, nfk, valid_bits, n_fk);
  le.note();
  if (n_domain_errors) *n_domain_errors = nd;
  if (n_unconverged) *n_unconverged = nu;
  if (n_integrations) *n_integrations = ni;
  return TR_OK;
}

}  // namespace

extern "C" int tr_validate_edges_loaded(tr_ctx *c, const tr_space_params *sp, const tr_shoot_params *shoot, const tr_edge_loads *loads,
                                        const double *a, const double *b, int64_t n_edges, uint64_t *valid_bits, double *last_valid_t,
                                        int32_t *n_fk, int64_t *n_domain_errors, int64_t *n_unconverged, int64_t *n_integrations) {
  if (!c) return TR_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lock_(c->mu);
  return validate_edges_loaded_impl(c, sp, shoot, loads, a, b, n_edges, valid_bits, last_valid_t, n_fk, n_domain_errors, n_unconverged, n_integrations);
}

// The roadmap form: every vertex is solved and swept once into pool slots [0, n_states) (cold start), its strains stay in vu_pool
// for the warm starts of its edges' first midpoints, then the edges run behind the vertices with index pairs.  n_fk counts as
// tr_validate_edges_indexed does: the two ends plus the edge's own samples.
extern "C" int tr_validate_edges_loaded_indexed(tr_ctx *c, const tr_space_params *sp, const tr_shoot_params *shoot, const tr_edge_loads *loads,
                                                const double *states, int64_t n_states, const int32_t *edges, int64_t n_edges,
                                                uint64_t *valid_bits, int32_t *n_fk, int64_t *n_domain_errors, int64_t *n_unconverged,
                                                int64_t *n_integrations) {
  if (!c) return TR_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lock_(c->mu);
  int64_t nd = 0, nu = 0, ni = 0;
  if (n_domain_errors) *n_domain_errors = 0;
  if (n_unconverged) *n_unconverged = 0;
  if (n_integrations) *n_integrations = 0;
  if (n_edges < 0 || n_states < 0 || (n_edges > 0 && (!sp || !states || !edges || !valid_bits))) return fail(c, TR_ERR_INVALID_ARG, "bad argument");
  LoadedEdges le{};
  bool empty;
  int rc;
  if ((rc = loaded_edges_begin(c, sp, shoot, loads, n_edges, le, empty)) || empty) return rc;
  if ((rc = check_edge_indices(c, edges, n_edges, n_states))) return rc;
  if ((rc = ensure_edge_pool(c, n_edges + n_states / 8))) return rc;
  const int S = c->K.state_size;
  const int64_t cap = c->ws.ld, Vp = round_up(n_states, 64);
  if (Vp > cap / 2) {
    // more vertices than half the sample pool: gather on the host and take the pairwise form
    std::vector<double> a((size_t)n_edges * S), b((size_t)n_edges * S);
    for (int64_t k = 0; k < n_edges; k++) {
      std::memcpy(&a[(size_t)k * S], states + (size_t)edges[2 * k] * S, S * sizeof(double));
      std::memcpy(&b[(size_t)k * S], states + (size_t)edges[2 * k + 1] * S, S * sizeof(double));
    }
    c->ledge.n_vertices = 0;
    return validate_edges_loaded_impl(c, sp, shoot, loads, a.data(), b.data(), n_edges, valid_bits, nullptr, n_fk, n_domain_errors, n_unconverged, n_integrations);
  }
  if ((rc = le.reserve(cap)) || (rc = ensure_edge_dev(c, cap))) return rc;
  EdgeDev &d = c->edge;
  EdgeIndexed ix{};
  if ((rc = upload_indexed_inputs(c, states, n_states, edges, n_edges, false, &ix))) return rc;
  HIP_TRY(c, hipMemsetAsync(d.sample_edge, 0xff, (size_t)cap * sizeof(int32_t), nullptr));
  c->ledge.n_vertices = 0;
  if ((rc = le.clear_tally()) || (rc = le.samples(ix.d_states, 0, n_states, nullptr, 1)) || (rc = le.add_tally(&nu, &ni))) return rc;
  c->ledge.n_vertices = n_states;              // (the edges' samples live behind the vertex block: its rows of vu_pool stay)
  std::vector<uint8_t> ok((size_t)n_edges, 1);
  std::vector<int32_t> nfk((size_t)n_edges, 0);
  if ((rc = for_edge_chunks(n_edges, cap - Vp, 6.0, 2, nfk, [&](int64_t e0, int64_t e1) {
        return le.range(sp, nullptr, nullptr, e0, e1, ok, nfk, &nd, nullptr, &ix, &nu, &ni); }))) return rc;
  pack_edge_results(ok, nfk, valid_bits, n_fk);
  le.note();
  if (n_domain_errors) *n_domain_errors = nd;
  if (n_unconverged) *n_unconverged = nu;
  if (n_integrations) *n_integrations = ni;
  return TR_OK;
}

// How the context's last loaded edge call ran: stats = samples evaluated (those of chunks retried after a pool overflow included),
// levels (evaluator calls: one loads / guess / shooting / K2 sequence each), Levenberg-Marquardt rounds (one host synchronisation
// each), chunk attempts.  Tuning and benchmarks only.
extern "C" int tr_edges_loaded_last(const tr_ctx *c, int64_t stats[4]) {
  if (!c || !stats) return TR_ERR_INVALID_ARG;
  for (int q = 0; q < 4; q++) stats[q] = c->ledge.last[q];
  return TR_OK;
}

// The accepted base strains (v0, u0) of the vertices of the context's last tr_validate_edges_loaded_indexed call, n_states x 6: what
// tr_fk_loaded_batch returns as vu0_out for the same states and per-state loads, and what the warm start of the edges' first
// midpoints began from.  TR_ERR_INVALID_ARG when no indexed call's vertices are resident (none yet, a pairwise call since, or the
// call fell back to the pairwise form) or n_states is not that call's.
extern "C" int tr_edges_loaded_vertex_strains(tr_ctx *c, int64_t n_states, double *vu0_out) {
  if (!c) return TR_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lock_(c->mu);
  if (n_states <= 0 || !vu0_out || n_states != c->ledge.n_vertices) return fail(c, TR_ERR_INVALID_ARG, "no vertex strains of that size are resident");
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipMemcpy(vu0_out, c->ledge.vu_pool, (size_t)n_states * 6 * sizeof(double), hipMemcpyDeviceToHost));
  return TR_OK;
}
