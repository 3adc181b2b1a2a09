// edge_pairs_host.inc -- the edge calls on pairs of end states (tr_validate_edges, ..._last_valid, ..._discrete, tr_voxelize_edges)
// and the voxelize forms on index pairs (tr_voxelize_edges_indexed, tr_connect_edges_indexed); machinery: edge_run_host.inc
namespace {

// ---- what the entry points share ----
// after their own argument checks: the grid, the space's resolution, the device -- idle, since the workspace is shared with *_dev
// calls that may still run on other streams
int edge_call_begin(tr_ctx *c, const tr_space_params *sp) {
  if (!c->has_grid) return fail(c, TR_ERR_INVALID_ARG, "no obstacle grid set (tr_set_grid)");
  if (!(sp->min_tension_change > 0) || (c->K.enable_rotation && !(sp->min_rotation_change > 0)) ||
      (c->K.enable_retraction && !(sp->min_retraction_change > 0)))
    return fail(c, TR_ERR_INVALID_ARG, "minimum state changes must be positive");
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipDeviceSynchronize());
  return TR_OK;
}

// the index pairs of a host edge list lie in [0, n_states): one pass, no early exit -- the compiler vectorises the range test
int check_edge_indices(tr_ctx *c, const int32_t *edges, int64_t n_edges, int64_t n_states) {
  const uint32_t lim = (uint32_t)std::min<int64_t>(n_states, 0x7fffffff);
  uint32_t bad = 0;
  for (int64_t k = 0; k < 2 * n_edges; k++) bad |= (uint32_t)((uint32_t)edges[k] >= lim);
  return bad ? fail(c, TR_ERR_OUT_OF_RANGE, "edge refers to a state outside the array") : TR_OK;
}

// the roadmap's vertices and index pairs on the device: grow-only buffers of the context (a hipMalloc / hipFree pair per call is
// milliseconds in a process that holds the sample pool)
int upload_indexed_inputs(tr_ctx *c, const double *states, int64_t n_states, const int32_t *edges, int64_t n_edges, bool dev_inputs, EdgeIndexed *ix) {
  if (const int rc = ensure_indexed_inputs(c, n_states, n_edges)) return rc;
  EdgeDev &d = c->edge;
  const hipMemcpyKind up = dev_inputs ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  if (hipMemcpy(d.ix_states, states, (size_t)n_states * c->K.state_size * sizeof(double), up) != hipSuccess ||
      hipMemcpy(d.ix_idx, edges, (size_t)n_edges * 2 * sizeof(int32_t), up) != hipSuccess) return fail(c, TR_ERR_HIP, "hipMemcpy failed");
  *ix = EdgeIndexed{d.ix_states, d.ix_idx, round_up(n_states, 64)};
  return TR_OK;
}

// per-edge results of the host-side paths into the caller's arrays: mask words, FK counts and, for the voxelize forms, the offsets
// of the edges' block lists
void pack_edge_results(const std::vector<uint8_t> &ok, const std::vector<int32_t> &nfk, uint64_t *bits, int32_t *n_fk,
                       const std::vector<int32_t> *count = nullptr, int64_t *offsets = nullptr) {
  const int64_t n = (int64_t)ok.size();
  for (int64_t w = 0; w < (n + 63) / 64; w++) bits[w] = 0;
  for (int64_t e = 0; e < n; e++) {
    if (ok[(size_t)e]) bits[e >> 6] |= (uint64_t)1 << (e & 63);
    if (count) offsets[e + 1] = offsets[e] + (*count)[(size_t)e];
  }
  if (n_fk) std::memcpy(n_fk, nfk.data(), (size_t)n * sizeof(int32_t));
}

int validate_edges_impl(tr_ctx *c, const tr_space_params *sp, const double *a, const double *b, int64_t n_edges,
                        uint64_t *valid_bits, int32_t *n_fk, int64_t *n_domain_errors, double *last_valid_t) {
  if (!c) return TR_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lock_(c->mu);
  if (n_domain_errors) *n_domain_errors = 0;
  if (n_edges < 0 || (n_edges > 0 && (!sp || !a || !b || !valid_bits))) return fail(c, TR_ERR_INVALID_ARG, "bad argument");
  if (n_edges == 0) return TR_OK;
  int rc;
  if ((rc = edge_call_begin(c, sp))) return rc;
  // Deep bisection levels hold few samples, and a K1 launch costs its full 128-step latency (~0.5 ms) however small the
  // batch, so edges are processed in chunks as large as the sample pool allows.  Through the verdict-only kernels (the
  // default) the pool is EdgeDev's per-sample arrays alone (see tr_validate_edges_indexed), up to 2^24 slots; otherwise it is
  // the FK workspace with its point planes, up to 2^22 samples (17 GB of the 288 GB).
  const bool slots_only = c->fuse == 2 && edge_signatures(c, false);
  c->edge_slots_now = 0;
  if (slots_only) {
    c->edge_slots_now = edge_plan::pairwise_slots(n_edges, c->edge_slots_max);
    if ((rc = ensure_workspace(c, std::min<int64_t>(c->max_chunk, std::max<int64_t>(4 * c->fb_cap, 1 << 14))))) { c->edge_slots_now = 0; return rc; }
  } else if ((rc = ensure_edge_pool(c, n_edges))) return rc;
  const int64_t avail = slots_only ? c->edge_slots_now : c->ws.ld;
  std::vector<uint8_t> ok((size_t)n_edges, 1);
  std::vector<int32_t> nfk((size_t)n_edges, 0);
  int64_t nd = 0;
  // chunks sized for the pool (typical roadmap edges need 5-8 samples incl. their ends); an overflowing chunk is halved
  rc = for_edge_chunks(n_edges, avail, 9.0, 0, nfk, [&](int64_t e0, int64_t e1) {
        return edges_range(c, sp, a, b, e0, e1, ok, nfk, &nd, nullptr, last_valid_t); });
  c->edge_slots_now = 0;
  if (rc) return rc;
  pack_edge_results(ok, nfk, valid_bits, n_fk);
  if (n_domain_errors) *n_domain_errors = nd;
  return TR_OK;
}

int voxelize_edges_pairs_impl(tr_ctx *c, const tr_space_params *sp, const double *a, const double *b, int64_t n_edges,
                              int64_t *offsets, uint64_t *fully_valid_bits, int32_t *n_fk, bool collide) {
  if (!c) return TR_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lock_(c->mu);
  if (n_edges < 0 || (n_edges > 0 && (!sp || !a || !b || !offsets || !fully_valid_bits))) return fail(c, TR_ERR_INVALID_ARG, "bad argument");
  c->vstore.n = 0;
  if (offsets) offsets[0] = 0;
  if (n_edges == 0) return TR_OK;
  int rc;
  if ((rc = edge_call_begin(c, sp)) || (rc = ensure_edge_pool(c, n_edges))) return rc;
  std::vector<uint8_t> ok((size_t)n_edges, 1);
  std::vector<int32_t> nfk((size_t)n_edges, 0);
  EdgeVoxOut vox;
  vox.count.assign((size_t)n_edges, 0);
  vox.collide = collide;
  int64_t nd = 0;
  if ((rc = for_edge_chunks(n_edges, c->ws.ld, 9.0, 0, nfk, [&](int64_t e0, int64_t e1) {
        return edges_range(c, sp, a, b, e0, e1, ok, nfk, &nd, &vox); }))) return rc;
  pack_edge_results(ok, nfk, fully_valid_bits, n_fk, &vox.count, offsets);
  return TR_OK;
}

// Roadmap form of tr_voxelize_edges: every vertex is integrated and voxelised once for all of its edges.
int voxelize_edges_indexed_impl(tr_ctx *c, const tr_space_params *sp, const double *states, int64_t n_states,
                         const int32_t *edges, int64_t n_edges, int64_t *offsets, uint64_t *fully_valid_bits, int32_t *n_fk, bool collide) {
  if (!c) return TR_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lock_(c->mu);
  if (n_edges < 0 || n_states < 0 || (n_edges > 0 && (!sp || !states || !edges || !offsets || !fully_valid_bits)))
    return fail(c, TR_ERR_INVALID_ARG, "bad argument");
  c->vstore.n = 0;
  if (offsets) offsets[0] = 0;
  if (n_edges == 0) return TR_OK;
  int rc;
  if ((rc = check_edge_indices(c, edges, n_edges, n_states)) || (rc = edge_call_begin(c, sp))) return rc;
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
    return voxelize_edges_pairs_impl(c, sp, a.data(), b.data(), n_edges, offsets, fully_valid_bits, n_fk, collide);
  }
  if ((rc = ensure_edge_dev(c, cap))) return rc;
  if ((rc = ensure_vox_scratch(c, cap))) return rc;
  EdgeDev &d = c->edge;
  Workspace &w = c->ws;
  EdgeIndexed ix{};
  if ((rc = upload_indexed_inputs(c, states, n_states, edges, n_edges, false, &ix))) return rc;
  if (hipMemsetAsync(d.sample_edge, 0xff, (size_t)cap * sizeof(int32_t), nullptr) != hipSuccess) return fail(c, TR_ERR_HIP, "hipMemset failed");
  {  // every vertex once, shape validity only (voxelize(): is_valid_shape), then its block list: pool slots [0, n_states)
    const bool ret = c->K.enable_retraction;
    if ((rc = launch_fk_sweep(c, ix.d_states, n_states, cap, ws_fk_out(c, 0), ws_sweep_in(c, 0), collide ? 1 : 0, d.bits, nullptr, nullptr,
                              edge_signatures(c, true) ? d.sig : nullptr, d.sig_stride))) return rc;
    ProfScope ps(c, 3, nullptr);
    hipLaunchKernelGGL(trk::backbone_voxelize, dim3((unsigned)((n_states + 63) / 64)), dim3(64), 0, nullptr, w.px, w.py, w.pz,
                       ret ? w.np : nullptr, d.bits, n_states, cap, (int)c->K.n_points, c->G, vox_max_blocks(c), c->d_vids, c->d_vmasks, c->d_vcounts);
    if (hipGetLastError() != hipSuccess) return fail(c, TR_ERR_HIP, "backbone_voxelize launch failed");
  }
  std::vector<uint8_t> ok((size_t)n_edges, 1);
  std::vector<int32_t> nfk((size_t)n_edges, 0);
  EdgeVoxOut vox;
  vox.count.assign((size_t)n_edges, 0);
  vox.collide = collide;
  int64_t nd = 0;
  if ((rc = for_edge_chunks(n_edges, cap - Vp, std::max(6.0, 1.15 * c->edge_rate_seen), 2, nfk, [&](int64_t e0, int64_t e1) {
        return edges_range(c, sp, nullptr, nullptr, e0, e1, ok, nfk, &nd, &vox, nullptr, &ix); }))) return rc;
  pack_edge_results(ok, nfk, fully_valid_bits, n_fk, &vox.count, offsets);
  return TR_OK;
}
}  // namespace

extern "C" int tr_validate_edges(tr_ctx *c, const tr_space_params *sp, const double *a, const double *b,
                                 int64_t n_edges, uint64_t *valid_bits, int32_t *n_fk, int64_t *n_domain_errors) {
  return validate_edges_impl(c, sp, a, b, n_edges, valid_bits, n_fk, n_domain_errors, nullptr);
}

extern "C" int tr_validate_edges_last_valid(tr_ctx *c, const tr_space_params *sp, const double *a, const double *b,
                                            int64_t n_edges, uint64_t *valid_bits, double *last_valid_t, int32_t *n_fk) {
  if (!c) return TR_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lock_(c->mu);
  if (n_edges > 0 && !last_valid_t) return fail(c, TR_ERR_INVALID_ARG, "null last_valid_t");
  return validate_edges_impl(c, sp, a, b, n_edges, valid_bits, n_fk, nullptr, last_valid_t);
}

// Discrete variant: every edge sampled at a, i / validSegmentCount (i = 1..nd-1), b; one K1 + K2 pass
// per pool-full of samples.  n_fk / last_valid_t follow the sequential loop of
// VoxelBackboneDiscreteMotionValidator::generic_voxelize with full per-sample validity
// (voxelize_until_invalid_impl): it stops after the first invalid sample.
extern "C" int tr_validate_edges_discrete(tr_ctx *c, const tr_space_params *sp, const double *a, const double *b, int64_t n_edges,
                                          uint64_t *valid_bits, double *last_valid_t, int32_t *n_fk) {
  if (!c) return TR_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lock_(c->mu);
  if (n_edges < 0 || (n_edges > 0 && (!sp || !a || !b || !valid_bits))) return fail(c, TR_ERR_INVALID_ARG, "bad argument");
  if (n_edges == 0) return TR_OK;
  int rc;
  if ((rc = edge_call_begin(c, sp)) || (rc = ensure_edge_pool(c, n_edges))) return rc;
  const int64_t cap = c->ws.ld;
  if ((rc = ensure_edge_dev(c, cap))) return rc;
  EdgeDev &d = c->edge;
  const int S = c->K.state_size;
  const trk::EdgeSpaceK sk = edge_space(c, sp);
  const trk::EdgeState st = edge_state(c, 0, c->lane[0].counters);
  auto blocks = [](int64_t n) { return dim3((unsigned)((n + 255) / 256)); };
  const int64_t emax = cap / 2;                       // edges resident at once (>= 2 samples each)
  std::vector<int64_t> offs;
  std::vector<uint32_t> hok;
  for (int64_t k = 0; k < (n_edges + 63) / 64; k++) valid_bits[k] = 0;
  for (int64_t g0 = 0; g0 < n_edges; g0 += emax) {
    const int64_t E = std::min(emax, n_edges - g0);
    HIP_TRY(c, hipMemcpy(d.A, a + g0 * S, (size_t)E * S * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(d.B, b + g0 * S, (size_t)E * S * sizeof(double), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(trk::discrete_count, blocks(E), dim3(256), 0, nullptr, st, sk, E, d.nd, d.cnt);
    HIP_TRY(c, hipGetLastError());
    offs.assign((size_t)E + 1, 0);
    HIP_TRY(c, hipMemcpy(offs.data() + 1, d.cnt, (size_t)E * sizeof(int64_t), hipMemcpyDeviceToHost));
    for (int64_t k = 0; k < E; k++) {
      if (offs[(size_t)k + 1] > cap) return fail(c, TR_ERR_RUNTIME, "an edge needs more FK samples than the workspace holds");
      offs[(size_t)k + 1] += offs[(size_t)k];
    }
    HIP_TRY(c, hipMemcpy(d.cnt, offs.data(), (size_t)(E + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
    {
      std::vector<int32_t> init((size_t)E, 0x7fffffff);
      HIP_TRY(c, hipMemcpy(d.nfk, init.data(), (size_t)E * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    // passes of whole edges, at most `cap` samples each
    for (int64_t e0 = 0; e0 < E;) {
      int64_t e1 = e0 + 1;
      while (e1 < E && offs[(size_t)e1 + 1] - offs[(size_t)e0] <= cap) e1++;
      const int64_t q0 = offs[(size_t)e0], m = offs[(size_t)e1] - q0;
      {
        ProfScope ps(c, 3, nullptr);
        hipLaunchKernelGGL(trk::discrete_samples, blocks(m), dim3(256), 0, nullptr, st, sk, d.nd, d.cnt, E, q0, m, d.lvl_states);
        HIP_TRY(c, hipGetLastError());
      }
      // last_valid_t given = checkMotion(s1, s2, last_valid): the installed state checker decides a sample; without it
      // = checkMotion(s1, s2): is_valid_shape per sample and the union of the BACKBONES against the voxels
      // (nobody reads the samples' points here: with the backbone test they go through the verdict-only kernel)
      if ((rc = launch_fk_sweep(c, d.lvl_states, m, cap, ws_fk_out(c, 0), ws_sweep_in(c, 0), (last_valid_t && c->checker == TR_CHECKER_SPHERES) ? 2 : 1, d.bits, nullptr, nullptr,
                                nullptr, 0, /*points_unused=*/true))) return rc;
      {
        ProfScope ps(c, 3, nullptr);
        hipLaunchKernelGGL(trk::discrete_fold, blocks(m), dim3(256), 0, nullptr, st, d.cnt, q0, m);
        HIP_TRY(c, hipGetLastError());
      }
      e0 = e1;
    }
    hipLaunchKernelGGL(trk::discrete_finish, blocks(E), dim3(256), 0, nullptr, st, d.nd, d.cnt, (int64_t)0, E);
    HIP_TRY(c, hipGetLastError());
    hok.resize((size_t)E);
    HIP_TRY(c, hipMemcpy(hok.data(), d.edge_ok, (size_t)E * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (int64_t k = 0; k < E; k++) if (hok[(size_t)k]) valid_bits[(g0 + k) >> 6] |= (uint64_t)1 << ((g0 + k) & 63);
    if (n_fk) HIP_TRY(c, hipMemcpy(n_fk + g0, d.nfk, (size_t)E * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (last_valid_t) HIP_TRY(c, hipMemcpy(last_valid_t + g0, d.last_t, (size_t)E * sizeof(double), hipMemcpyDeviceToHost));
  }
  return TR_OK;
}

extern "C" int tr_voxelize_edges_indexed(tr_ctx *c, const tr_space_params *sp, const double *states, int64_t n_states,
                                         const int32_t *edges, int64_t n_edges, int64_t *offsets, uint64_t *fully_valid_bits, int32_t *n_fk) {
  return voxelize_edges_indexed_impl(c, sp, states, n_states, edges, n_edges, offsets, fully_valid_bits, n_fk, false);
}

extern "C" int tr_connect_edges_indexed(tr_ctx *c, const tr_space_params *sp, const double *states, int64_t n_states,
                                        const int32_t *edges, int64_t n_edges, int64_t *offsets, uint64_t *valid_bits, int32_t *n_fk) {
  return voxelize_edges_indexed_impl(c, sp, states, n_states, edges, n_edges, offsets, valid_bits, n_fk, true);
}

extern "C" int tr_voxelize_edges(tr_ctx *c, const tr_space_params *sp, const double *a, const double *b, int64_t n_edges,
                                 int64_t *offsets, uint64_t *fully_valid_bits, int32_t *n_fk) {
  return voxelize_edges_pairs_impl(c, sp, a, b, n_edges, offsets, fully_valid_bits, n_fk, false);
}

