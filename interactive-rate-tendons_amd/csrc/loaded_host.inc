// loaded_host.inc -- the loaded forward kinematics behind the C ABI (tr_fk_loaded_batch*): TendonRobot::general_shape for a batch,
// by single shooting on the base strains (fk_loaded_kernel.hpp).  The loop keeps every problem's state on the device, as the IK loop
// does (ik_host.inc): a first launch evaluates every problem's start (one lane each); then per round one expansion (ik_expand at
// S = 6), one launch of 13 lanes per still-active problem and one LM-step launch, and the host reads the 4-byte active count from
// pinned memory.  One last launch over all problems at their final strains writes the outputs.
// Included at the end of tendon_hip.hip (needs tr_ctx and ik_host.inc's helpers).
namespace {

int64_t shoot_chunk_size(const tr_ctx *c) { return c->shoot_chunk > 0 ? c->shoot_chunk : kIkLanes / trk::kShootQ; }
// the host-array form stages its outputs (P point rows, 9 P frame rows per problem): smaller chunks
int64_t shoot_io_chunk(const tr_ctx *c) { return std::min<int64_t>(shoot_chunk_size(c), 8192); }

void shoot_release(tr_ctx *c) {
  tr_ctx::ShootDev &k = c->shoot;
  k.chunk.release(); k.once.release(); k.io.release(); k.io_frames.release(); k.count.release(); k.order.release();
  trk::merge_free(k.ord_ms);
  k = tr_ctx::ShootDev{};
}

// the workspace for chunks of up to `n` problems (grow-only, released with the context)
int shoot_reserve(tr_ctx *c, int64_t n) {
  tr_ctx::ShootDev &k = c->shoot;
  const int64_t probs = round_up(std::max<int64_t>(1, std::min(n, shoot_chunk_size(c))), 64), lanes = round_up(probs * trk::kShootQ, 64);
  int rc;
  if (!k.zero6) {
    if ((rc = k.count.reserve(c, k.once))) return rc;
    const int N = c->K.n_tendons;
    std::vector<double> route((size_t)N * 6);
    routing_at(c, c->K.L, route.data());
    if ((rc = k.once.alloc(c, &k.tip_route, route.size()))) return rc;
    HIP_TRY(c, hipMemcpy(k.tip_route, route.data(), route.size() * sizeof(double), hipMemcpyHostToDevice));
    if ((rc = k.once.alloc(c, &k.zero6, 6))) return rc;
    HIP_TRY(c, hipMemset(k.zero6, 0, 6 * sizeof(double)));
  }
  if (k.probs >= probs) return TR_OK;
  HIP_TRY(c, hipDeviceSynchronize());
  DevOwner &o = k.chunk;
  o.release();
  k.probs = k.lanes = 0;                       // (no buffer is usable until all of them exist again)
  if ((rc = o.alloc_all(c, {&k.xs, &k.res}, (size_t)(lanes * 6)))) return rc;
  // per problem, by shape
  if ((rc = o.alloc_all(c, {&k.p, &k.pn, &k.e}, (size_t)(probs * 6)))) return rc;
  if ((rc = o.alloc(c, &k.J, (size_t)(probs * 36)))) return rc;
  if ((rc = o.alloc_all(c, {&k.err2, &k.mu, &k.nu}, (size_t)probs))) return rc;
  if ((rc = o.alloc_all(c, {&k.iters, &k.calls, &k.list[0], &k.list[1]}, (size_t)probs))) return rc;
  k.probs = probs;
  k.lanes = lanes;
  return TR_OK;
}

// staging of the host-array form for chunks of up to `n` problems
int shoot_reserve_io(tr_ctx *c, int64_t n, bool want_R) {
  tr_ctx::ShootDev &k = c->shoot;
  const int64_t probs = round_up(std::max<int64_t>(1, std::min(n, shoot_io_chunk(c))), 64);
  const size_t P = (size_t)c->K.n_points, N = (size_t)c->K.n_tendons, S = (size_t)c->K.state_size;
  int rc;
  if (k.io_probs < probs) {
    HIP_TRY(c, hipDeviceSynchronize());
    DevOwner &o = k.io;
    o.release();
    k.io_probs = 0;
    if ((rc = o.alloc(c, &k.io_states, (size_t)probs * S))) return rc;
    if ((rc = o.alloc_all(c, {&k.io_w, &k.io_d, &k.io_g, &k.io_vu, &k.io_vuL}, (size_t)probs * 6))) return rc;
    if ((rc = o.alloc_all(c, {&k.io_px, &k.io_py, &k.io_pz}, P * (size_t)probs))) return rc;
    if ((rc = o.alloc(c, &k.io_Li, N * (size_t)probs))) return rc;
    if ((rc = o.alloc_all(c, {&k.io_L, &k.io_e}, (size_t)probs))) return rc;
    if ((rc = o.alloc_all(c, {&k.io_np, &k.io_it, &k.io_fc}, (size_t)probs))) return rc;
    if ((rc = o.alloc(c, &k.io_conv, (size_t)probs))) return rc;
    k.io_probs = probs;
  }
  if (want_R && k.io_R_probs < probs) {
    HIP_TRY(c, hipDeviceSynchronize());
    k.io_frames.release();
    k.io_R_probs = 0;
    if ((rc = k.io_frames.alloc(c, &k.io_R, 9 * P * (size_t)probs))) return rc;
    k.io_R_probs = probs;
  }
  return TR_OK;
}

int shoot_params(tr_ctx *c, const tr_shoot_params *sp, trk::ShootParams &prm) {
  const tr_shoot_params def{100, 0.1, 1e-9, 1e-4, 1e-6};                               // TendonRobot.h:199-203
  const tr_shoot_params &q = sp ? *sp : def;
  if (q.max_iters < 0) return fail(c, TR_ERR_INVALID_ARG, "max_iters must be >= 0");
  prm = trk::ShootParams{};
  prm.max_iters = q.max_iters;
  prm.delta = q.finite_difference_delta;
  prm.mu_init = q.mu_init;
  prm.eps1 = q.stop_threshold_JT_err_inf;
  prm.eps2_sq = q.stop_threshold_Dp * q.stop_threshold_Dp;
  prm.eps3_sq = c->K.residual_threshold * c->K.residual_threshold;
  return TR_OK;
}

// What both forms refuse.  A robot with retraction is refused by EVERY loaded call, in these words, until the caller opens the context
// to it (tr_set_loaded_retraction) -- contexts that never ask behave as they always did; retraction_ok: the call is one whose name
// says retraction (tr_fk_loaded_batch_retraction_dev).
int shoot_check(tr_ctx *c, int64_t n, int64_t wrench_ld, int64_t dist_ld, bool retraction_ok = false) {
  if (n < 0) return fail(c, TR_ERR_INVALID_ARG, "bad argument");
  if (wrench_ld != 0 && wrench_ld < 6) return fail(c, TR_ERR_INVALID_ARG, "bad argument (wrench_ld: 0 or >= 6)");
  if (dist_ld != 0 && dist_ld < 6) return fail(c, TR_ERR_INVALID_ARG, "bad argument (dist_ld: 0 or >= 6)");
  if (c->K.enable_retraction && !c->loaded_retraction && !retraction_ok)
    return fail(c, TR_ERR_UNSUPPORTED, "loaded FK (general_shape) is not built for robots with retraction");
  return TR_OK;
}

// On a context opened by tr_set_loaded_retraction the loaded FK, the loaded tips and the validity of loaded shapes take robots with
// retraction (fk_loaded_retract_kernel.hpp); every loaded call above them still refuses such a robot here, under its own name `call`:
// it needs more than the integrator (the loaded IK, for one, the tip's derivative along s_start through the shooting).
int refuse_retraction(tr_ctx *c, const char *call) {
  if (!c->K.enable_retraction) return TR_OK;
  return fail(c, TR_ERR_UNSUPPORTED, std::string(call) + ": loaded FK (general_shape) is not built for robots with retraction in this call "
                                     "(tr_fk_loaded_batch*, tr_fk_loaded_tips* and the validity of loaded shapes are)");
}

// The one load set of a call (the edge, roadmap, IK and Jacobian calls on loaded shapes) in the form its kernels take: Loads is
// trk::EdgeLoadsK or trk::IklLoads, kernel parameter types with the same three members.  loads == NULL: no load.
template <typename Loads>
int parse_loads(tr_ctx *c, const tr_edge_loads *loads, Loads &dst) {
  dst = Loads{};
  if (!loads) return TR_OK;
  if (loads->frame != TR_LOAD_FRAME_BASE && loads->frame != TR_LOAD_FRAME_WORLD)
    return fail(c, TR_ERR_INVALID_ARG, "bad argument (frame: TR_LOAD_FRAME_BASE or TR_LOAD_FRAME_WORLD)");
  for (int q = 0; q < 6; q++) { dst.wrench[q] = loads->wrench[q]; dst.dist[q] = loads->dist[q]; }
  dst.world = loads->frame == TR_LOAD_FRAME_WORLD;
  return TR_OK;
}

// the installed load profile's table on the device, or null: what every integration of the loaded calls is launched with
const double *profile_weights(const tr_ctx *c) { return c->profile.on ? c->profile.d_table : nullptr; }

// w(x) of a load profile (include/tendon_hip.h: tr_set_load_profile), in the operation order written there
double profile_at(int64_t K, const double *s, const double *w, double x) {
#pragma clang fp contract(off)
  if (!(x > s[0])) return w[0];
  if (!(x < s[K - 1])) return w[K - 1];
  int64_t k = 0;
  while (k + 2 < K && s[k + 1] <= x) k++;
  return w[k] + (w[k + 1] - w[k]) * ((x - s[k]) / (s[k + 1] - s[k]));
}

// `lanes` integrations: lane t is problem list[t / Q] (list null: t / Q) of d_states from strains vu[t].  A robot with retraction:
// every lane on its own grid, rows aligned at the tip (fk_loaded_retract; no load profile can be installed on such a robot).
int shoot_fk(tr_ctx *c, const double *d_states, int64_t lanes, int64_t ld, const trk::FkOut &out, trk::LoadedIn in, hipStream_t s) {
  in.tip_route = c->shoot.tip_route;
  in.weights = profile_weights(c);
  const trk::FkLaunch a = fk_launch_args(c, d_states, lanes, ld, out, out.R != nullptr, s);
  const bool ret = c->K.enable_retraction;
  TRK_FOR_TENDONS(c, if (ret) trk::launch_fk_loaded_retract<N>(a, in); else trk::launch_fk_loaded<N>(a, in));
  HIP_TRY(c, hipGetLastError());
  return TR_OK;
}

// One chunk of m problems to the end.  d_wrench / d_dist / d_guess: the chunk's first row (d_wrench never null here).  `out`: K1's
// outputs with column 0 = the chunk's first problem; the other outputs may be null.
// `perm` (a robot with retraction, shoot_run's order): problem i of the chunk is column perm[i] of the CALL's arrays -- states, load and
// guess rows, and every output are then the call's own, not offset to the chunk; the chunk's workspace stays indexed by i.
int shoot_chunk_solve(tr_ctx *c, const trk::ShootParams &prm, const double *d_states, int64_t m, int64_t ld, const double *d_wrench,
                      int64_t wrench_ld, const double *d_dist, int64_t dist_ld, const double *d_guess, const trk::FkOut &out,
                      uint8_t *d_conv, double *d_vu0, double *d_vuL, double *d_res, int32_t *d_iters, int32_t *d_calls, hipStream_t s,
                      int64_t &rounds, bool final_launch = true, const int32_t *perm = nullptr) {
  tr_ctx::ShootDev &k = c->shoot;
  constexpr int Q = trk::kShootQ;
  const trk::ShootState st{k.p, k.pn, k.e, k.J, k.err2, k.mu, k.nu, k.iters, k.calls};
  trk::LoadedIn base{d_wrench, wrench_ld, d_dist, dist_ld, nullptr, nullptr, 1, nullptr, k.res, k.lanes, nullptr};
  base.perm = perm;
  int rc;
  {
    const trk::FkLaunch a = fk_launch_args(c, d_states, m, ld, kFkOutNone, false, s);
    const bool ret = c->K.enable_retraction;      // (the unloaded solution at the problem's own s_start)
    TRK_FOR_TENDONS(c, if (ret) trk::launch_shoot_start_retract<N>(a, d_guess, k.pn, perm); else trk::launch_shoot_start<N>(a, d_guess, k.pn));
    HIP_TRY(c, hipGetLastError());
  }
  // the start of every problem: one lane each
  int cur = 0;
  int64_t active = 0;
  if ((rc = k.count.zero(cur, s))) return rc;
  {
    trk::LoadedIn in = base;
    in.vu = k.pn;
    if ((rc = shoot_fk(c, d_states, m, ld, kFkOutNone, in, s))) return rc;
  }
  hipLaunchKernelGGL(trk::shoot_begin, dim3(ik_grid(m, 64)), dim3(64), 0, s, prm, st, m, (const double *)k.res, k.lanes, k.list[cur],
                     k.count.d + cur);
  HIP_TRY(c, hipGetLastError());
  if ((rc = k.count.read(cur, s, active))) return rc;
  rounds++;
  while (active > 0) {
    const int nxt = cur ^ 1;
    if ((rc = k.count.zero(nxt, s))) return rc;
    hipLaunchKernelGGL(trk::ik_expand, dim3(ik_grid(active * Q, 256)), dim3(256), 0, s, (const double *)k.pn, (const int32_t *)k.list[cur],
                       active, 6, prm.delta, k.xs);
    HIP_TRY(c, hipGetLastError());
    trk::LoadedIn in = base;
    in.vu = k.xs; in.list = k.list[cur]; in.Q = Q;
    if ((rc = shoot_fk(c, d_states, active * Q, ld, kFkOutNone, in, s))) return rc;
    hipLaunchKernelGGL(trk::shoot_lm_step, dim3(ik_grid(active, 64)), dim3(64), 0, s, prm, st, (const int32_t *)k.list[cur], active,
                       (const double *)k.res, k.lanes, k.list[nxt], k.count.d + nxt);
    HIP_TRY(c, hipGetLastError());
    if ((rc = k.count.read(nxt, s, active))) return rc;
    rounds++;
    cur = nxt;
  }
  // the outputs: every problem once more at its final strains (final_launch false: the caller wants the strains and flags only)
  if (final_launch) {
    trk::LoadedIn in = base;
    in.vu = k.p; in.res = nullptr; in.vu_tip = d_vuL;
    if ((rc = shoot_fk(c, d_states, m, ld, out, in, s))) return rc;
  }
  hipLaunchKernelGGL(trk::shoot_finish, dim3(ik_grid(m, 64)), dim3(64), 0, s, prm, st, m, d_vu0, d_res, d_iters, d_calls, d_conv, perm);
  HIP_TRY(c, hipGetLastError());
  if (c->K.enable_retraction && d_conv) {
    hipLaunchKernelGGL(trk::shoot_negative_start, dim3(ik_grid(m, 64)), dim3(64), 0, s, d_states, (int)c->K.state_size, m, d_conv, perm);
    HIP_TRY(c, hipGetLastError());
  }
  return TR_OK;
}

// tr_fk_loaded_batch*'s body: n device problems in chunks, each to the end.  d_wrench null: no tip wrench; `out`: K1's outputs with
// column 0 = problem 0 (planes of leading dimension ld); every output may be null.  Adds its rounds to `rounds`.
int shoot_run(tr_ctx *c, const trk::ShootParams &prm, const double *d_states, int64_t n, int64_t ld, const double *d_wrench,
              int64_t wrench_ld, const double *d_dist, int64_t dist_ld, const double *d_guess, const trk::FkOut &out, uint8_t *d_conv,
              double *d_vu0, double *d_vuL, double *d_res, int32_t *d_iters, int32_t *d_calls, hipStream_t s, int64_t &rounds) {
  const int S = c->K.state_size;
  int rc;
  if ((rc = shoot_reserve(c, n))) return rc;
  const int64_t chunk = shoot_chunk_size(c);
  tr_ctx::ShootDev &k = c->shoot;
  k.order_last[0] = n; k.order_last[1] = 0;
  if (c->K.enable_retraction && c->loaded_retract_sort_min > 0 && n >= c->loaded_retract_sort_min) {
    // A wave of fk_loaded_retract runs from its longest backbone's base to the tip while its shorter lanes idle: deal the problems to
    // the chunks -- and with them to the waves -- in the order of their s_start.  Every lane reads and writes the caller's column
    // perm[.], so nothing is gathered and nothing comes back out of order.
    if (k.ord_cap < n) {
      HIP_TRY(c, hipDeviceSynchronize());
      k.order.release();
      k.ord_cap = 0;
      const size_t cap = (size_t)round_up(n + n / 4, 64);
      for (int q = 0; q < 2; q++)
        if ((rc = k.order.alloc(c, &k.ord_keys[q], cap)) || (rc = k.order.alloc(c, &k.ord_vals[q], cap))) return rc;
      k.ord_cap = (int64_t)cap;
    }
    const int32_t *perm = nullptr;
    const hipError_t e = trk::retraction_order(k.ord_ms, d_states, n, S, c->K.L, k.ord_keys, k.ord_vals, &perm, s);
    if (e != hipSuccess) return fail(c, TR_ERR_HIP, std::string("retraction order (loaded FK): ") + hipGetErrorString(e));
    for (int64_t off = 0; off < n; off += chunk) {
      const int64_t m = std::min(chunk, n - off);
      if ((rc = shoot_chunk_solve(c, prm, d_states, m, ld, d_wrench ? d_wrench : c->shoot.zero6, d_wrench ? wrench_ld : 0, d_dist, dist_ld,
                                  d_guess, out, d_conv, d_vu0, d_vuL, d_res, d_iters, d_calls, s, rounds, true, perm + off))) return rc;
    }
    k.order_last[1] = n;
    return TR_OK;
  }
  for (int64_t off = 0; off < n; off += chunk) {
    const int64_t m = std::min(chunk, n - off);
    const trk::FkOut o{rows_at(out.px, off), rows_at(out.py, off), rows_at(out.pz, off), rows_at(out.R, off), rows_at(out.L, off),
                       rows_at(out.Li, off), nullptr, nullptr, rows_at(out.n_points, off), rows_at(out.home_Li, off)};
    if ((rc = shoot_chunk_solve(c, prm, d_states + off * S, m, ld, d_wrench ? d_wrench + off * wrench_ld : c->shoot.zero6,
                                d_wrench ? wrench_ld : 0, rows_at(d_dist, off, dist_ld), dist_ld, rows_at(d_guess, off, 6), o,
                                rows_at(d_conv, off), rows_at(d_vu0, off, 6), rows_at(d_vuL, off, 6), rows_at(d_res, off),
                                rows_at(d_iters, off), rows_at(d_calls, off), s, rounds))) return rc;
  }
  return TR_OK;
}

int fk_loaded_dev_impl(tr_ctx *c, const tr_shoot_params *params, const double *d_states, int64_t n, int64_t ld,
                       const double *d_wrench, int64_t wrench_ld, const double *d_dist, int64_t dist_ld, const double *d_guess,
                       double *d_px, double *d_py, double *d_pz, double *d_R, double *d_L, double *d_Li, uint8_t *d_converged,
                       int32_t *d_n_points, double *d_home_Li, double *d_vu0_out, double *d_vuL_out, double *d_residual_out,
                       int32_t *d_iters_out, int32_t *d_fk_calls_out, int64_t *rounds_out, void *stream);

}  // namespace

extern "C" {

int tr_set_load_profile(tr_ctx *c, int64_t n_knots, const double *s, const double *w) {
  if (!c) return TR_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lock_(c->mu);
  if (n_knots < 1 || !s || !w) return fail(c, TR_ERR_INVALID_ARG, "bad argument (load profile: n_knots >= 1 knots and weights)");
  for (int64_t k = 0; k < n_knots; k++) {
    if (!std::isfinite(s[k]) || !std::isfinite(w[k])) return fail(c, TR_ERR_INVALID_ARG, "bad argument (load profile: knots and weights must be finite)");
    if (k > 0 && !(s[k] > s[k - 1])) return fail(c, TR_ERR_INVALID_ARG, "bad argument (load profile: knots must be strictly increasing)");
  }
  // the table is indexed like the shared routing table and has no entries for a lane's own first interval
  if (const int rc = shoot_check(c, 0, 0, 0)) return rc;
  if (const int rc = refuse_retraction(c, "load profiles (tr_set_load_profile)")) return rc;
  const size_t n = 1 + 3 * c->steps.size();
  std::vector<double> table(n);
  table[0] = profile_at(n_knots, s, w, 0.0);
  for (size_t k = 0; k < c->steps.size(); k++) {
    const double tk = c->step_t[k], h = c->steps[k].h;
    table[1 + 3 * k + 0] = profile_at(n_knots, s, w, tk);
    table[1 + 3 * k + 1] = profile_at(n_knots, s, w, tk + h * 0.5);
    table[1 + 3 * k + 2] = profile_at(n_knots, s, w, tk + h);
  }
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipDeviceSynchronize());          // launches that still read the previous table (any stream) finish first
  if (!c->profile.d_table) HIP_TRY(c, hipMalloc((void **)&c->profile.d_table, n * sizeof(double)));
  c->profile.on = false;                       // (a failed upload leaves no profile installed)
  HIP_TRY(c, hipMemcpy(c->profile.d_table, table.data(), n * sizeof(double), hipMemcpyHostToDevice));
  c->profile.table.swap(table);
  c->profile.on = true;
  return TR_OK;
}

// The context's last shooting run (shoot_run: one call of tr_fk_loaded_batch*, one chunk of tr_fk_loaded_tips*, one level of a loaded
// edge call): its problems, and how many of them were solved in backbone-length order (all of them or none).
int tr_loaded_order_last(const tr_ctx *c, int64_t stats[2]) {
  if (!c || !stats) return TR_ERR_INVALID_ARG;
  stats[0] = c->shoot.order_last[0]; stats[1] = c->shoot.order_last[1];
  return TR_OK;
}

int tr_clear_load_profile(tr_ctx *c) {
  if (!c) return TR_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lock_(c->mu);
  c->profile.on = false;                       // (launches already queued hold the table's pointer, and the table stays)
  c->profile.table.clear();
  return TR_OK;
}

int tr_get_load_profile(tr_ctx *c, double *table_out, int64_t capacity, int64_t *n_out) {
  if (!c) return TR_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lock_(c->mu);
  if (!n_out || capacity < 0) return fail(c, TR_ERR_INVALID_ARG, "bad argument");
  const int64_t n = c->profile.on ? (int64_t)c->profile.table.size() : 0;
  *n_out = n;
  if (table_out) for (int64_t k = 0; k < std::min(n, capacity); k++) table_out[k] = c->profile.table[k];
  return TR_OK;
}

int tr_fk_loaded_batch_dev(tr_ctx *c, const tr_shoot_params *params, const double *d_states, int64_t n, int64_t ld,
                           const double *d_wrench, int64_t wrench_ld, const double *d_dist, int64_t dist_ld, const double *d_guess,
                           double *d_px, double *d_py, double *d_pz, double *d_R, double *d_L, double *d_Li, uint8_t *d_converged,
                           int32_t *d_n_points, double *d_vu0_out, double *d_vuL_out, double *d_residual_out, int32_t *d_iters_out,
                           int32_t *d_fk_calls_out, int64_t *rounds_out, void *stream) {
  if (!c) return TR_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lock_(c->mu);
  return fk_loaded_dev_impl(c, params, d_states, n, ld, d_wrench, wrench_ld, d_dist, dist_ld, d_guess, d_px, d_py, d_pz, d_R, d_L, d_Li,
                            d_converged, d_n_points, nullptr, d_vu0_out, d_vuL_out, d_residual_out, d_iters_out, d_fk_calls_out, rounds_out,
                            stream);
}

int tr_fk_loaded_batch_retraction_dev(tr_ctx *c, const tr_shoot_params *params, const double *d_states, int64_t n, int64_t ld,
                                      const double *d_wrench, int64_t wrench_ld, const double *d_dist, int64_t dist_ld,
                                      const double *d_guess, double *d_px, double *d_py, double *d_pz, double *d_R, double *d_L,
                                      double *d_Li, uint8_t *d_converged, int32_t *d_n_points, double *d_home_Li, double *d_vu0_out,
                                      double *d_vuL_out, double *d_residual_out, int32_t *d_iters_out, int32_t *d_fk_calls_out,
                                      int64_t *rounds_out, void *stream) {
  if (!c) return TR_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lock_(c->mu);
  if (rounds_out) *rounds_out = 0;
  if (!c->K.enable_retraction) return fail(c, TR_ERR_INVALID_ARG, "robot has no retraction: use tr_fk_loaded_batch_dev (home lengths: tr_home_lengths)");
  if (n < 0) return fail(c, TR_ERR_INVALID_ARG, "bad argument");
  if (n == 0) return TR_OK;
  if (!d_n_points || !d_home_Li) return fail(c, TR_ERR_INVALID_ARG, "null device pointer");
  return fk_loaded_dev_impl(c, params, d_states, n, ld, d_wrench, wrench_ld, d_dist, dist_ld, d_guess, d_px, d_py, d_pz, d_R, d_L, d_Li,
                            d_converged, d_n_points, d_home_Li, d_vu0_out, d_vuL_out, d_residual_out, d_iters_out, d_fk_calls_out,
                            rounds_out, stream);
}

}  // extern "C"
namespace {
// the device forms' body (d_home_Li: tr_fk_loaded_batch_retraction_dev's, else null); the caller holds the lock
int fk_loaded_dev_impl(tr_ctx *c, const tr_shoot_params *params, const double *d_states, int64_t n, int64_t ld,
                       const double *d_wrench, int64_t wrench_ld, const double *d_dist, int64_t dist_ld, const double *d_guess,
                       double *d_px, double *d_py, double *d_pz, double *d_R, double *d_L, double *d_Li, uint8_t *d_converged,
                       int32_t *d_n_points, double *d_home_Li, double *d_vu0_out, double *d_vuL_out, double *d_residual_out,
                       int32_t *d_iters_out, int32_t *d_fk_calls_out, int64_t *rounds_out, void *stream) {
  if (rounds_out) *rounds_out = 0;
  int rc;
  if ((rc = shoot_check(c, n, wrench_ld, dist_ld, d_home_Li != nullptr))) return rc;
  if (ld < n || (ld & 63)) return fail(c, TR_ERR_INVALID_ARG, "ld must be a multiple of 64 and >= n");
  if (n == 0) return TR_OK;
  if (!d_states) return fail(c, TR_ERR_INVALID_ARG, "null device pointer");
  if ((d_px || d_py || d_pz) && !(d_px && d_py && d_pz)) return fail(c, TR_ERR_INVALID_ARG, "d_px, d_py, d_pz: all or none");
  if (d_R && !d_px) return fail(c, TR_ERR_INVALID_ARG, "d_R needs the point planes");
  HIP_TRY(c, hipSetDevice(c->device));
  const hipStream_t s = (hipStream_t)stream;
  trk::ShootParams prm;
  if ((rc = shoot_params(c, params, prm))) return rc;
  if ((rc = begin_dev_work(c, s))) return rc;
  const trk::FkOut out{d_px, d_py, d_pz, d_R, d_L, d_Li, nullptr, nullptr, d_n_points, d_home_Li};
  int64_t rounds = 0;
  if ((rc = shoot_run(c, prm, d_states, n, ld, d_wrench, wrench_ld, d_dist, dist_ld, d_guess, out, d_converged, d_vu0_out, d_vuL_out,
                      d_residual_out, d_iters_out, d_fk_calls_out, s, rounds))) return rc;
  if (rounds_out) *rounds_out = rounds;
  return note_dev_work(c, s);
}
}  // namespace
extern "C" {

int tr_fk_loaded_batch(tr_ctx *c, const tr_shoot_params *params, const double *states, int64_t n, const double *wrench,
                       int64_t wrench_ld, const double *dist, int64_t dist_ld, const double *guess, double *p, double *R, double *L,
                       double *L_i, uint8_t *converged, int32_t *n_points, double *vu0_out, double *vuL_out, double *residual_out,
                       int32_t *iters_out, int32_t *fk_calls_out, int64_t *rounds_out) {
  if (!c) return TR_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lock_(c->mu);
  if (rounds_out) *rounds_out = 0;
  int rc;
  if ((rc = shoot_check(c, n, wrench_ld, dist_ld))) return rc;
  if (n > 0 && !states) return fail(c, TR_ERR_INVALID_ARG, "bad argument");
  if (n == 0) return TR_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipDeviceSynchronize());          // the workspace is shared with *_dev calls that may still run on other streams
  const int S = c->K.state_size, P = c->K.n_points, N = c->K.n_tendons;
  trk::ShootParams prm;
  if ((rc = shoot_params(c, params, prm))) return rc;
  const int64_t chunk = shoot_io_chunk(c);      // (no more than one chunk of the body's: its loop runs once per staging chunk)
  if ((rc = shoot_reserve_io(c, n, R != nullptr))) return rc;
  tr_ctx::ShootDev &k = c->shoot;
  std::vector<double> hx, hy, hz, hR, hLi;
  std::vector<int32_t> hn;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  int64_t rounds = 0;
  for (int64_t off = 0; off < n; off += chunk) {
    const int64_t m = std::min(chunk, n - off), ld = round_up(m, 64);
    if ((rc = upload_rows(c, k.io_states, states, S, off, m, S))) return rc;
    if (wrench && (rc = upload_rows(c, k.io_w, wrench, wrench_ld, off, m, 6))) return rc;
    if (dist && (rc = upload_rows(c, k.io_d, dist, dist_ld, off, m, 6))) return rc;
    if (guess && (rc = upload_rows(c, k.io_g, guess, 6, off, m, 6))) return rc;
    const trk::FkOut out{p || R ? k.io_px : nullptr, p || R ? k.io_py : nullptr, p || R ? k.io_pz : nullptr, R ? k.io_R : nullptr, k.io_L, k.io_Li,
                         nullptr, nullptr, k.io_np, nullptr};
    if ((rc = shoot_run(c, prm, k.io_states, m, ld, wrench ? k.io_w : nullptr, wrench_ld ? 6 : 0, dist ? k.io_d : nullptr, dist_ld ? 6 : 0,
                        guess ? k.io_g : nullptr, out, k.io_conv, k.io_vu, k.io_vuL, k.io_e, k.io_it, k.io_fc, nullptr, rounds))) return rc;
    HIP_TRY(c, hipDeviceSynchronize());
    // point counts of THIS chunk (a robot with retraction: device rows are aligned at the tip, point j is in row j + (P - n_points);
    // the host arrays start at row 0 and are NaN past n_points, as tr_fk_batch's)
    hn.assign((size_t)m, P);
    if ((p || R) && c->K.enable_retraction) HIP_TRY(c, hipMemcpy(hn.data(), k.io_np, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost));
    // device planes are [P][ld]; only the first m columns are copied (2-D copies, host pitch m)
    if (p) {
      hx.resize((size_t)P * m); hy.resize((size_t)P * m); hz.resize((size_t)P * m);
      HIP_TRY(c, hipMemcpy2D(hx.data(), (size_t)m * 8, k.io_px, (size_t)ld * 8, (size_t)m * 8, (size_t)P, hipMemcpyDeviceToHost));
      HIP_TRY(c, hipMemcpy2D(hy.data(), (size_t)m * 8, k.io_py, (size_t)ld * 8, (size_t)m * 8, (size_t)P, hipMemcpyDeviceToHost));
      HIP_TRY(c, hipMemcpy2D(hz.data(), (size_t)m * 8, k.io_pz, (size_t)ld * 8, (size_t)m * 8, (size_t)P, hipMemcpyDeviceToHost));
      for (int64_t i = 0; i < m; i++) {
        const int np_i = hn[(size_t)i], sh = P - np_i;
        for (int j = 0; j < P; j++) {
          double *o = p + ((size_t)(off + i) * P + j) * 3;
          if (j < np_i) { o[0] = hx[(size_t)(j + sh) * m + i]; o[1] = hy[(size_t)(j + sh) * m + i]; o[2] = hz[(size_t)(j + sh) * m + i]; }
          else o[0] = o[1] = o[2] = nan;
        }
      }
    }
    if (R) {
      hR.resize((size_t)9 * P * m);
      HIP_TRY(c, hipMemcpy2D(hR.data(), (size_t)m * 8, k.io_R, (size_t)ld * 8, (size_t)m * 8, (size_t)9 * P, hipMemcpyDeviceToHost));
      for (int64_t i = 0; i < m; i++) {
        const int np_i = hn[(size_t)i], sh = P - np_i;
        for (int j = 0; j < P; j++)
          for (int q = 0; q < 9; q++) R[((size_t)(off + i) * P + j) * 9 + q] = j < np_i ? hR[((size_t)q * P + j + sh) * m + i] : nan;
      }
    }
    if ((rc = download_rows(c, L, k.io_L, off, m))) return rc;
    if (L_i) {
      hLi.resize((size_t)N * m);
      HIP_TRY(c, hipMemcpy2D(hLi.data(), (size_t)m * 8, k.io_Li, (size_t)ld * 8, (size_t)m * 8, (size_t)N, hipMemcpyDeviceToHost));
      for (int64_t i = 0; i < m; i++) for (int j = 0; j < N; j++) L_i[(size_t)(off + i) * N + j] = hLi[(size_t)j * m + i];
    }
    if ((rc = download_rows(c, converged, k.io_conv, off, m)) || (rc = download_rows(c, n_points, k.io_np, off, m)) ||
        (rc = download_rows(c, vu0_out, k.io_vu, off, m, 6)) || (rc = download_rows(c, vuL_out, k.io_vuL, off, m, 6)) ||
        (rc = download_rows(c, residual_out, k.io_e, off, m)) || (rc = download_rows(c, iters_out, k.io_it, off, m)) ||
        (rc = download_rows(c, fk_calls_out, k.io_fc, off, m))) return rc;
  }
  if (rounds_out) *rounds_out = rounds;
  return TR_OK;
}

}  // extern "C"
