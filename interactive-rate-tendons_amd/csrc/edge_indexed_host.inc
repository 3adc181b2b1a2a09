// edge_indexed_host.inc -- the roadmap form of the edge check, tr_validate_edges_indexed*: the end states of the edges are rows of
// one vertex array, and every vertex is evaluated once for all of its edges (a k-nearest roadmap has ~2k edge ends per vertex).
// One call is a ValidateIndexed: a short run() over named steps that chooses among the edge queue, the lanes and one lane
// (machinery: edge_run_host.inc; sizes: edge_plan.hpp).  tr_reserve_edges warms the same path up.
namespace {

struct ValidateIndexed {
  tr_ctx *const c; const tr_space_params *const sp;
  const double *states; const int64_t n_states;
  const int32_t *edges; const int64_t n_edges;
  uint64_t *const valid_bits; int32_t *const n_fk; int64_t *const n_domain_errors;
  const bool dev_inputs;                  // `states` and `edges` are device arrays (tr_validate_edges_indexed_dev); the results go to host arrays either way
  const uint32_t *const d_vertex_sig;     // the vertices are known to be valid and these are their signature rows (tr_validate_candidates_sig_dev): no vertex pass
  // derived
  bool finished = false;                  // a step has delivered the call's results: run() returns
  bool slots_only = false;                // through the verdict-only kernels: the pool is EdgeDev's per-sample arrays alone
  int64_t cap = 0, Vp = 0;                // pool slots; slots of the vertex block
  EdgeIndexed ix{};
  edge_plan::LanePlan plan{};
  std::vector<uint8_t> ok;                // (filled only on the one-lane path: the lanes deliver packed words and the counts directly)
  std::vector<int32_t> nfk;
  int64_t nd = 0;
  EdgeLaps lap;

  ~ValidateIndexed() { c->edge_slots_now = 0; }

  int run() {
    int rc;
    if ((rc = begin()) || finished) return rc;
    if ((rc = size_pool()) || (rc = pairwise_when_vertices_outgrow_pool()) || finished) return rc;
    if ((rc = upload_inputs()) || (rc = range_check_on_device()) || (rc = vertex_pass())) return rc;
    if ((rc = try_queue()) || finished) return rc;
    plan_lanes();
    if (plan.fits && ((rc = reserve_lanes()) || (rc = run_lanes()) || finished)) return rc;
    return one_lane();
  }

  int begin() {
    if (n_domain_errors) *n_domain_errors = 0;
    if (n_edges < 0 || n_states < 0 || (n_edges > 0 && (!sp || !states || !edges || !valid_bits)))
      return fail(c, TR_ERR_INVALID_ARG, "bad argument");
    for (auto &v : c->edge_queue_last) v = 0;
    if (n_edges == 0) { finished = true; return TR_OK; }
    lap("");
    int rc;
    if (!dev_inputs && (rc = check_edge_indices(c, edges, n_edges, n_states))) return rc;
    if ((rc = edge_call_begin(c, sp))) return rc;
    lap("argument checks");
    return TR_OK;
  }

  // Through the verdict-only kernels (the default) no sample's backbone is stored: the pool is the per-sample arrays of EdgeDev
  // alone and is sized on its own -- two lanes' worth at the sample rate this context last saw, up to 2^24 slots -- while the FK
  // workspace only has to hold the fallback passes' columns.  Otherwise the pool is the workspace.
  int size_pool() {
    int rc;
    slots_only = c->fuse == 2 && edge_signatures(c, false);
    c->edge_slots_now = 0;
    if (slots_only) {
      c->edge_slots_now = edge_plan::indexed_slots(c->edge_rate_seen, n_edges, n_states, c->edge_slots_max);
      // the fallback passes' columns -- and, for the edge queue, 64 columns per persistent wave (sized here, before anything is
      // allocated after the workspace's size)
      const int64_t qcols = (c->edge_queue && !c->K.enable_retraction) ? (int64_t)edge_queue_waves(c) * 64 : 0;
      if ((rc = ensure_workspace(c, std::min<int64_t>(c->max_chunk, std::max<int64_t>(std::max<int64_t>(4 * c->fb_cap, 1 << 14), qcols))))) return rc;
    } else if ((rc = ensure_edge_pool(c, n_edges + n_states / 8))) return rc;
    cap = slots_only ? c->edge_slots_now : c->ws.ld;
    Vp = round_up(n_states, 64);
    if (d_vertex_sig && (!slots_only || c->K.enable_retraction || c->checker == TR_CHECKER_SPHERES))
      return fail(c, TR_ERR_UNSUPPORTED, "vertex signatures: backbone checker, no retraction, verdict-only schedule (tr_signature_words > 0)");
    return TR_OK;
  }

  // more vertices than half the sample pool (more than 2^23 vertices, or a pool bounded below that): gather the end states on the
  // host and take the pairwise path -- device inputs are brought over first (rare, and correct rather than fast)
  int pairwise_when_vertices_outgrow_pool() {
    if (Vp <= cap / 2) return TR_OK;
    const int S = c->K.state_size;
    std::vector<double> hs;
    std::vector<int32_t> he;
    if (dev_inputs) {
      hs.resize((size_t)n_states * S); he.resize((size_t)n_edges * 2);
      HIP_TRY(c, hipMemcpy(hs.data(), states, hs.size() * sizeof(double), hipMemcpyDeviceToHost));
      HIP_TRY(c, hipMemcpy(he.data(), edges, he.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
      if (const int rc = check_edge_indices(c, he.data(), n_edges, n_states)) return rc;
      states = hs.data(); edges = he.data();
    }
    std::vector<double> a((size_t)n_edges * S), b((size_t)n_edges * S);
    for (int64_t k = 0; k < n_edges; k++) {
      std::memcpy(&a[(size_t)k * S], states + (size_t)edges[2 * k] * S, S * sizeof(double));
      std::memcpy(&b[(size_t)k * S], states + (size_t)edges[2 * k + 1] * S, S * sizeof(double));
    }
    c->edge_slots_now = 0;
    finished = true;
    return validate_edges_impl(c, sp, a.data(), b.data(), n_edges, valid_bits, n_fk, n_domain_errors, nullptr);
  }

  int upload_inputs() {
    if (const int rc = ensure_edge_dev(c, std::max(cap, c->ws.ld))) return rc;
    return upload_indexed_inputs(c, states, n_states, edges, n_edges, dev_inputs, &ix);
  }

  // the range test of the index pairs, on the device (the host form does it before anything is uploaded)
  int range_check_on_device() {
    if (!dev_inputs) return TR_OK;
    uint32_t *const flag = c->lane[0].counters;
    if (hipMemsetAsync(flag, 0, sizeof(uint32_t), nullptr) != hipSuccess) return fail(c, TR_ERR_HIP, "hipMemset failed");
    hipLaunchKernelGGL(trk::index_range_check, dim3((unsigned)((2 * n_edges + 255) / 256)), dim3(256), 0, nullptr, ix.d_idx, 2 * n_edges,
                       (int32_t)std::min<int64_t>(n_states, 0x7fffffff), flag);
    uint32_t bad = 0;
    if (hipGetLastError() != hipSuccess || hipMemcpy(&bad, flag, sizeof(bad), hipMemcpyDeviceToHost) != hipSuccess) return fail(c, TR_ERR_HIP, "index check failed");
    if (bad) return fail(c, TR_ERR_OUT_OF_RANGE, "edge refers to a state outside the array");
    return TR_OK;
  }

  // every vertex once: pool slots [0, n_states)
  int vertex_pass() {
    EdgeDev &d = c->edge;
    if (hipMemsetAsync(d.sample_edge, 0xff, (size_t)cap * sizeof(int32_t), nullptr) != hipSuccess) return fail(c, TR_ERR_HIP, "hipMemset failed");
    if (d_vertex_sig) {
      // the caller's rows are the vertices' signatures, and every vertex is valid: what the pass would have left in slots [0, n_states)
      if (hipMemcpyAsync(d.sig, d_vertex_sig, (size_t)n_states * d.sig_stride * sizeof(uint32_t), hipMemcpyDeviceToDevice, nullptr) != hipSuccess ||
          hipMemsetAsync(d.bits, 0xff, (size_t)(Vp / 64) * sizeof(uint64_t), nullptr) != hipSuccess) return fail(c, TR_ERR_HIP, "vertex signatures: copy failed");
    } else {
      const bool sig = edge_signatures(c, false);
      if (const int rc = launch_fk_sweep(c, ix.d_states, n_states, cap, ws_fk_out(c, 0), ws_sweep_in(c, 0), 1, d.bits, nullptr, nullptr, sig ? d.sig : nullptr,
                                         d.sig_stride, /*points_unused=*/sig, (sig && c->K.enable_retraction) ? d.sig_np : nullptr)) return rc;
    }
    lap("uploads + vertex launch");
    lap("host vectors");
    return TR_OK;
  }

  // The edge queue: one persistent launch, a barrier per edge instead of one per level (edge_queue_kernel.hpp).  Where it does
  // not apply -- retraction robots (their samples run through the two-kernel retraction path), another schedule, a pool or an
  // edge level beyond what the queue takes -- the level-synchronous lanes take the call.  By default it serves the
  // device-resident forms (measured in one call each, profiles/r04: 3 % faster than the lanes at config 3's size, 3 - 20 % on the
  // shards of config 4) and the lanes serve the host-array form, whose results they deliver to host memory lane by lane while the
  // other lanes still integrate (the lanes 5 % faster there); TENDON_HIP_EDGE_QUEUE=1 sends both through the queue, =0 neither.
  int try_queue() {
    if (!(c->edge_queue && (dev_inputs || c->edge_queue_forced) && slots_only && !c->K.enable_retraction && n_edges <= cap / 2)) return TR_OK;
    const int waves = edge_queue_waves(c);
    if (waves <= 0 || c->ws.ld < (int64_t)waves * 64) return TR_OK;
    int64_t own = 0, qnd = 0;
    const int rc = edges_queue_run(c, sp, ix, n_edges, cap, valid_bits, n_fk, &qnd, &own, waves);
    lap("edge queue");
    if (rc == EDGE_OVERFLOW) return TR_OK;
    if (rc) return rc;
    c->edge_rate_seen = (double)own / (double)n_edges;
    if (n_domain_errors) *n_domain_errors = qnd;
    finished = true;
    return TR_OK;
  }

  // Lanes: the parts of the edge list bisected side by side on as many streams, each with its share of the pool behind
  // the vertices; one host thread alternates between them (enqueue a level of one lane while the other's runs).  The last,
  // partial round of waves of one lane's FK launch -- and its launches at the latency floor -- are filled by the other
  // lanes' work (profiles/probe_two_streams.py: 3 - 25 % depending on the launch sizes).  Only through the verdict-only kernels (the
  // default schedule) and only when each part fits its share of the pool as one chunk (edge_plan.hpp); a lane that overflows sends
  // the whole call back to the one-lane path.
  void plan_lanes() {
    plan = edge_plan::plan_lanes(edge_plan::LaneQuery{n_edges, cap, Vp, c->ws.ld, c->fb_cap, c->edge_lanes, c->edge_lanes_fixed, c->edge_rate_seen,
                                                      c->edge_lane_guess, c->edge_lane_guess_forced, slots_only, (bool)c->K.enable_rotation});
  }

  int reserve_lanes() {
    if (const int rc = ensure_edge_lanes(c)) return rc;
    HIP_TRY(c, hipDeviceSynchronize());                               // vertices, uploads: done before the lanes' streams start
    lap("vertex pass (wait)");
    return ::reserve_lanes(c, plan.NL, plan.R, c->K.enable_retraction);
  }

  int run_lanes() {
    const int NL = plan.NL;
    std::vector<EdgeRun> run;
    run.reserve((size_t)NL);
    for (int l = 0; l < NL; l++) {
      run.push_back(EdgeRun{c, sp, nullptr, nullptr, plan.eb[l], plan.eb[l + 1], &ok, &nfk, &nd, nullptr, nullptr, &ix});
      EdgeRun &r = run.back();
      r.L = EdgeLane{c->lane[l].stream, l, Vp + l * plan.R, Vp + (l + 1) * plan.R, plan.eb[l], l * plan.lvl_share, c->lane[l].counters, c->lane[l].hc};
      r.direct = true; r.mask_out = valid_bits; r.nfk_out = n_fk;
    }
    int stt[tr_ctx::kMaxLanes];
    for (int l = 0; l < NL; l++) stt[l] = run[(size_t)l].start();
    auto any = [&](auto pred) { for (int l = 0; l < NL; l++) if (pred(stt[l])) return true; return false; };
    while (any([](int v) { return v == EDGE_MORE; })) {
      // whichever lane's stream has drained is resumed first (a fixed order would leave a finished lane waiting behind a busy one)
      bool progressed = false;
      for (int h = 0; h < NL; h++) {
        if (stt[h] != EDGE_MORE) continue;
        const hipError_t he = hipStreamQuery(run[(size_t)h].L.s);
        if (he == hipErrorNotReady) continue;
        stt[h] = he == hipSuccess ? run[(size_t)h].resume() : fail(c, TR_ERR_HIP, std::string("edge lane: ") + hipGetErrorString(he));
        progressed = true;
      }
      if (!progressed) sched_yield();
      if (any([](int v) { return v > 0; })) break;                    // an error on one lane: the others are drained below, not resumed
    }
    {
      const hipError_t he = hipDeviceSynchronize();                   // (also after an error: nothing of this call may still run when it returns)
      if (he != hipSuccess && !any([](int v) { return v > 0; })) stt[0] = fail(c, TR_ERR_HIP, std::string("edge lanes: ") + hipGetErrorString(he));
    }
    lap("lanes (levels + results)");
    for (int l = 0; l < NL; l++) if (stt[l] > 0) return stt[l];
    if (any([](int v) { return v != TR_OK; })) { nd = 0; return TR_OK; }    // a lane's share of the pool overflowed: start over on one lane
    // the mask words and the FK counts are in the caller's arrays; samples per edge for the next call's lanes
    int64_t own = 0;
    for (auto &r : run) own += r.own_samples;
    c->edge_rate_seen = (double)own / (double)n_edges;
    if (n_domain_errors) *n_domain_errors = nd;
    lap("pack results");
    finished = true;
    return TR_OK;
  }

  // chunks of the whole pool behind the vertices on the null stream (typical roadmap edges take 3-6 samples between their ends)
  int one_lane() {
    ok.assign((size_t)n_edges, 1);
    nfk.assign((size_t)n_edges, 0);
    if (const int rc = for_edge_chunks(n_edges, cap - Vp, std::max(6.0, 1.15 * c->edge_rate_seen), 2, nfk, [&](int64_t e0, int64_t e1) {
          return edges_range(c, sp, nullptr, nullptr, e0, e1, ok, nfk, &nd, nullptr, nullptr, &ix); })) return rc;
    double sum = 0;
    for (int64_t e = 0; e < n_edges; e++) sum += nfk[(size_t)e];
    c->edge_rate_seen = std::max(0.0, sum / (double)n_edges - 2.0);
    pack_edge_results(ok, nfk, valid_bits, n_fk);
    if (n_domain_errors) *n_domain_errors = nd;
    lap("pack results");
    return TR_OK;
  }
};

int validate_edges_indexed_impl(tr_ctx *c, const tr_space_params *sp, const double *states, int64_t n_states, const int32_t *edges, int64_t n_edges,
                                uint64_t *valid_bits, int32_t *n_fk, int64_t *n_domain_errors, bool dev_inputs, const uint32_t *d_vertex_sig = nullptr) {
  if (!c) return TR_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lock_(c->mu);
  return ValidateIndexed{c, sp, states, n_states, edges, n_edges, valid_bits, n_fk, n_domain_errors, dev_inputs, d_vertex_sig}.run();
}

// the device-resident forms: the call's host results, then the mask words (and the FK counts, when asked for) up to the caller's arrays
int validate_edges_indexed_to_dev(tr_ctx *c, const tr_space_params *sp, const double *d_states, int64_t n_states, const uint32_t *d_vertex_sig,
                                  const int32_t *d_edges, int64_t n_edges, uint64_t *d_valid_bits, int32_t *d_n_fk, int64_t *n_domain_errors) {
  std::vector<uint64_t> hb((size_t)((n_edges + 63) / 64));
  std::vector<int32_t> hn(d_n_fk ? (size_t)n_edges : 0);
  const int rc = validate_edges_indexed_impl(c, sp, d_states, n_states, d_edges, n_edges, hb.data(), d_n_fk ? hn.data() : nullptr, n_domain_errors, true, d_vertex_sig);
  if (rc || n_edges == 0) return rc;
  HIP_TRY(c, hipMemcpy(d_valid_bits, hb.data(), hb.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
  if (d_n_fk) HIP_TRY(c, hipMemcpy(d_n_fk, hn.data(), hn.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  return TR_OK;
}

}  // namespace

extern "C" int tr_reserve_edges(tr_ctx *c, int64_t n_edges) {
  if (!c) return TR_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lock_(c->mu);
  if (n_edges < 0) return fail(c, TR_ERR_INVALID_ARG, "negative size");
  HIP_TRY(c, hipSetDevice(c->device));
  int rc;
  if ((rc = ensure_edge_pool(c, n_edges))) return rc;
  if ((rc = ensure_edge_lanes(c))) return rc;                        // the lanes' streams and counters
  // ... and the per-sample arrays for the slots the verdict-only indexed form will ask for (tr_validate_edges_indexed)
  const bool slots_only = c->fuse == 2 && edge_signatures(c, false);
  int64_t slots = c->ws.ld;
  if (slots_only) slots = std::max<int64_t>(slots, edge_plan::reserve_slots(c->edge_rate_seen, n_edges, c->edge_slots_max));
  if ((rc = ensure_edge_dev(c, slots))) return rc;
  // what a first indexed call would otherwise allocate on the way: the index pairs and (a k-nearest roadmap has ~6 edges per vertex)
  // the vertex array, the lanes' fallback lists at the largest share of the pool a lane can have
  if ((rc = ensure_indexed_inputs(c, n_edges / 4 + 64, n_edges))) return rc;
  if (slots_only && c->edge_lanes >= 2 && n_edges >= 8192 &&
      (rc = reserve_lanes(c, std::min(c->edge_lanes, tr_ctx::kMaxLanes), round_up(slots / 2, 64), /*order=*/false))) return rc;
  if (c->has_grid && !c->edge_kernels_loaded && slots_only) {
    // the first launch of a kernel loads it (0.1 - 0.5 ms each for the FK kernels): one launch of every kernel of the indexed edge path on
    // nothing -- 64 home states through the vertex pass, the helpers on empty ranges -- so that a roadmap's first call does not pay it
    if ((rc = ensure_workspace(c, std::min<int64_t>(c->max_chunk, std::max<int64_t>(4 * c->fb_cap, 1 << 14))))) return rc;
    EdgeDev &d = c->edge; Workspace &w = c->ws;
    const bool ret = c->K.enable_retraction;
    const int S = c->K.state_size;
    HIP_TRY(c, hipMemsetAsync(d.ix_states, 0, (size_t)64 * S * sizeof(double), nullptr));
    if ((rc = launch_fk_sweep(c, d.ix_states, 64, slots, ws_fk_out(c, 0), ws_sweep_in(c, 0), 1, d.bits, nullptr, nullptr, d.sig, d.sig_stride,
                              /*points_unused=*/true, ret ? d.sig_np : nullptr))) return rc;
    const tr_space_params unit{1.0, 1.0, 1.0};
    const trk::EdgeSpaceK sk = edge_space(c, &unit);
    const trk::EdgeState st = edge_state(c, 0, c->lane[0].counters);
    const dim3 one(1), th(256);
    const int P = c->K.n_points;
    hipLaunchKernelGGL(trk::edge_init_indexed, one, th, 0, nullptr, st, sk, (int64_t)0, (const double *)d.ix_states, (const int32_t *)d.ix_idx, d.A, d.B);
    hipLaunchKernelGGL((trk::edge_filter<true>), one, th, 0, nullptr, st, (const trk::EdgeIv *)nullptr, (const int32_t *)d.ix_idx, (int64_t)0, (int64_t)0,
                       w.px, w.py, w.pz, w.ld, P, (const int32_t *)nullptr, c->G, 0, d.frontier, d.sig, d.sig_stride);
    hipLaunchKernelGGL((trk::edge_filter<false>), one, th, 0, nullptr, st, (const trk::EdgeIv *)d.open, (const int32_t *)nullptr, (int64_t)0, (int64_t)0,
                       w.px, w.py, w.pz, w.ld, P, (const int32_t *)nullptr, c->G, 0, d.frontier, d.sig, d.sig_stride);
    hipLaunchKernelGGL(trk::edge_open, one, th, 0, nullptr, st, sk, (const trk::EdgeIv *)d.frontier, (int64_t)0, (int64_t)0, (int64_t)0, 0, d.open, d.lvl_states);
    hipLaunchKernelGGL(trk::edge_fold, one, th, 0, nullptr, st, (int64_t)0, (int64_t)0, 0);
    hipLaunchKernelGGL(trk::edge_ok_bits, one, th, 0, nullptr, (const uint32_t *)d.edge_ok, (int64_t)0, reinterpret_cast<uint64_t *>(d.nd));
    HIP_TRY(c, hipGetLastError());
    if (c->edge_queue && !ret && d.q_ctl) {
      // ... and the edge queue's: its seed kernel on nothing and the persistent launch over an EMPTY queue (head = tail = done: every
      // wave leaves at once), so that a roadmap's first call finds the code object loaded and the occupancy known
      const int waves = edge_queue_waves(c);
      if (waves > 0 && (rc = ensure_workspace(c, std::max<int64_t>(w.ld, (int64_t)waves * 64))) == TR_OK && w.ld >= (int64_t)waves * 64) {
        HIP_TRY(c, hipMemsetAsync(d.q_ctl, 0, trk::EQ_WORDS * sizeof(uint32_t), nullptr));
        HIP_TRY(c, hipMemsetAsync(st.counters, 0, trk::EC_COUNT * sizeof(uint32_t), nullptr));
        hipLaunchKernelGGL(trk::edge_queue_seed, one, th, 0, nullptr, st, (const trk::EdgeIv *)d.open, (int64_t)0, (int64_t)slots, d.q_remaining, d.q_lvl_base, d.q_lvl_cnt, d.q_ctl);
        if ((rc = fill_queue_args(c, sk, 0))) return rc;
        if ((rc = launch_edge_queue(c, nullptr, d.sig, d.sig_stride, d.q_args, (unsigned)waves))) return rc;
      }
    }
    HIP_TRY(c, hipDeviceSynchronize());
    c->edge_kernels_loaded = true;
  }
  return TR_OK;
}

extern "C" int tr_validate_edges_indexed(tr_ctx *c, const tr_space_params *sp, const double *states, int64_t n_states,
                                         const int32_t *edges, int64_t n_edges, uint64_t *valid_bits, int32_t *n_fk,
                                         int64_t *n_domain_errors) {
  return validate_edges_indexed_impl(c, sp, states, n_states, edges, n_edges, valid_bits, n_fk, n_domain_errors, false);
}

// The same with the vertex states and the index pairs already in HBM (the device-resident roadmap build: sampled vertices ->
// tr_knn_edges_dev -> here): nothing but the mask words (and the FK counts, when asked for) crosses PCIe.  Synchronises.
extern "C" int tr_validate_edges_indexed_dev(tr_ctx *c, const tr_space_params *sp, const double *d_states, int64_t n_states,
                                             const int32_t *d_edges, int64_t n_edges, uint64_t *d_valid_bits, int32_t *d_n_fk,
                                             int64_t *n_domain_errors) {
  if (!c) return TR_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lock_(c->mu);         // (before the first fail(): it writes the context's error text)
  if (n_edges > 0 && !d_valid_bits) return fail(c, TR_ERR_INVALID_ARG, "bad argument");
  return validate_edges_indexed_to_dev(c, sp, d_states, n_states, nullptr, d_edges, n_edges, d_valid_bits, d_n_fk, n_domain_errors);
}

// ... for vertices that have just passed the vertex phase on this context's grid: d_vertex_sig (n_states x tr_signature_words uint32) are
// their signature rows from tr_validate_candidates_sig_dev, compacted like the states; the call then does not integrate the vertices
// again (1.4 ms per 10^5, a term that does not shrink when the edge list is a rank's shard).  Every vertex is taken to be valid.
extern "C" int tr_validate_edges_indexed_sig_dev(tr_ctx *c, const tr_space_params *sp, const double *d_states, int64_t n_states,
                                                 const uint32_t *d_vertex_sig, const int32_t *d_edges, int64_t n_edges,
                                                 uint64_t *d_valid_bits, int32_t *d_n_fk, int64_t *n_domain_errors) {
  if (!c) return TR_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lock_(c->mu);         // (before the first fail(): it writes the context's error text)
  if (n_edges > 0 && (!d_valid_bits || !d_vertex_sig)) return fail(c, TR_ERR_INVALID_ARG, "bad argument");
  return validate_edges_indexed_to_dev(c, sp, d_states, n_states, d_vertex_sig, d_edges, n_edges, d_valid_bits, d_n_fk, n_domain_errors);
}
