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
  void *p[] = {k.xs, k.res, k.p, k.pn, k.e, k.J, k.err2, k.mu, k.nu, k.iters, k.calls, k.list[0], k.list[1], k.d_count, k.tip_route, k.zero6,
               k.io_states, k.io_w, k.io_d, k.io_g, k.io_px, k.io_py, k.io_pz, k.io_R, k.io_L, k.io_Li, k.io_vu, k.io_vuL, k.io_e, k.io_np, k.io_it,
               k.io_fc, k.io_conv};
  for (void *q : p) if (q) (void)hipFree(q);
  if (k.h_count) (void)hipHostFree(k.h_count);
  k = tr_ctx::ShootDev{};
}

// the workspace for chunks of up to `n` problems (grow-only, released with the context)
int shoot_reserve(tr_ctx *c, int64_t n) {
  tr_ctx::ShootDev &k = c->shoot;
  const int64_t probs = round_up(std::max<int64_t>(1, std::min(n, shoot_chunk_size(c))), 64), lanes = round_up(probs * trk::kShootQ, 64);
  int rc;
  if (!k.d_count) {
    if ((rc = dev_alloc(c, &k.d_count, 2))) return rc;
    HIP_TRY(c, hipHostMalloc((void **)&k.h_count, sizeof(uint32_t), hipHostMallocDefault));
    const int N = c->K.n_tendons;
    std::vector<double> route((size_t)N * 6);
    routing_at(c, c->K.L, route.data());
    if ((rc = dev_alloc(c, &k.tip_route, route.size()))) return rc;
    HIP_TRY(c, hipMemcpy(k.tip_route, route.data(), route.size() * sizeof(double), hipMemcpyHostToDevice));
    if ((rc = dev_alloc(c, &k.zero6, 6))) return rc;
    HIP_TRY(c, hipMemset(k.zero6, 0, 6 * sizeof(double)));
  }
  if (k.probs >= probs) return TR_OK;
  HIP_TRY(c, hipDeviceSynchronize());
  if ((rc = dev_alloc(c, &k.xs, (size_t)(lanes * 6)))) return rc;
  if ((rc = dev_alloc(c, &k.res, (size_t)(lanes * 6)))) return rc;
  if ((rc = dev_alloc(c, &k.p, (size_t)(probs * 6)))) return rc;
  if ((rc = dev_alloc(c, &k.pn, (size_t)(probs * 6)))) return rc;
  if ((rc = dev_alloc(c, &k.e, (size_t)(probs * 6)))) return rc;
  if ((rc = dev_alloc(c, &k.J, (size_t)(probs * 36)))) return rc;
  if ((rc = dev_alloc(c, &k.err2, (size_t)probs))) return rc;
  if ((rc = dev_alloc(c, &k.mu, (size_t)probs))) return rc;
  if ((rc = dev_alloc(c, &k.nu, (size_t)probs))) return rc;
  if ((rc = dev_alloc(c, &k.iters, (size_t)probs))) return rc;
  if ((rc = dev_alloc(c, &k.calls, (size_t)probs))) return rc;
  for (int q = 0; q < 2; q++) if ((rc = dev_alloc(c, &k.list[q], (size_t)probs))) return rc;
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
    if ((rc = dev_alloc(c, &k.io_states, (size_t)probs * S))) return rc;
    if ((rc = dev_alloc(c, &k.io_w, (size_t)probs * 6))) return rc;
    if ((rc = dev_alloc(c, &k.io_d, (size_t)probs * 6))) return rc;
    if ((rc = dev_alloc(c, &k.io_g, (size_t)probs * 6))) return rc;
    if ((rc = dev_alloc(c, &k.io_px, P * (size_t)probs))) return rc;
    if ((rc = dev_alloc(c, &k.io_py, P * (size_t)probs))) return rc;
    if ((rc = dev_alloc(c, &k.io_pz, P * (size_t)probs))) return rc;
    if ((rc = dev_alloc(c, &k.io_L, (size_t)probs))) return rc;
    if ((rc = dev_alloc(c, &k.io_Li, N * (size_t)probs))) return rc;
    if ((rc = dev_alloc(c, &k.io_vu, (size_t)probs * 6))) return rc;
    if ((rc = dev_alloc(c, &k.io_vuL, (size_t)probs * 6))) return rc;
    if ((rc = dev_alloc(c, &k.io_e, (size_t)probs))) return rc;
    if ((rc = dev_alloc(c, &k.io_np, (size_t)probs))) return rc;
    if ((rc = dev_alloc(c, &k.io_it, (size_t)probs))) return rc;
    if ((rc = dev_alloc(c, &k.io_fc, (size_t)probs))) return rc;
    if ((rc = dev_alloc(c, &k.io_conv, (size_t)probs))) return rc;
    k.io_probs = probs;
  }
  if (want_R && k.io_R_probs < probs) {
    HIP_TRY(c, hipDeviceSynchronize());
    if ((rc = dev_alloc(c, &k.io_R, 9 * P * (size_t)probs))) return rc;
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

// what both forms refuse
int shoot_check(tr_ctx *c, int64_t n, int64_t wrench_ld, int64_t dist_ld) {
  if (n < 0) return fail(c, TR_ERR_INVALID_ARG, "bad argument");
  if (wrench_ld != 0 && wrench_ld < 6) return fail(c, TR_ERR_INVALID_ARG, "bad argument (wrench_ld: 0 or >= 6)");
  if (dist_ld != 0 && dist_ld < 6) return fail(c, TR_ERR_INVALID_ARG, "bad argument (dist_ld: 0 or >= 6)");
  if (c->K.enable_retraction)
    return fail(c, TR_ERR_UNSUPPORTED, "loaded FK (general_shape) is not built for robots with retraction");
  return TR_OK;
}

// `lanes` integrations: lane t is problem list[t / Q] (list null: t / Q) of d_states from strains vu[t]
int shoot_fk(tr_ctx *c, const double *d_states, int64_t lanes, int64_t ld, const trk::FkOut &out, trk::LoadedIn in, hipStream_t s) {
  in.tip_route = c->shoot.tip_route;
  const trk::FkLaunch a{d_states, lanes, ld, c->K, (bool)c->K.enable_rotation, out.R != nullptr, c->d_tab, c->d_steps,
                        (int)c->steps.size(), c->d_poly, c->k_first, c->d_tgrid, c->d_hl, out, s};
  switch (c->K.n_tendons) {
#define TRK_CASE(N) case N: trk::launch_fk_loaded<N>(a, in); break;
    TRK_CASE(1) TRK_CASE(2) TRK_CASE(3) TRK_CASE(4) TRK_CASE(5) TRK_CASE(6) TRK_CASE(7) TRK_CASE(8)
#undef TRK_CASE
    default: return fail(c, TR_ERR_OUT_OF_RANGE, "n_tendons out of range");
  }
  HIP_TRY(c, hipGetLastError());
  return TR_OK;
}

// One chunk of m problems to the end.  d_wrench / d_dist / d_guess: the chunk's first row (d_wrench never null here).  `out`: K1's
// outputs with column 0 = the chunk's first problem; the other outputs may be null.
int shoot_chunk_solve(tr_ctx *c, const trk::ShootParams &prm, const double *d_states, int64_t m, int64_t ld, const double *d_wrench,
                      int64_t wrench_ld, const double *d_dist, int64_t dist_ld, const double *d_guess, const trk::FkOut &out,
                      uint8_t *d_conv, double *d_vu0, double *d_vuL, double *d_res, int32_t *d_iters, int32_t *d_calls, hipStream_t s,
                      int64_t &rounds, bool final_launch = true) {
  tr_ctx::ShootDev &k = c->shoot;
  constexpr int Q = trk::kShootQ;
  const trk::ShootState st{k.p, k.pn, k.e, k.J, k.err2, k.mu, k.nu, k.iters, k.calls};
  const trk::FkOut none{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  const trk::LoadedIn base{d_wrench, wrench_ld, d_dist, dist_ld, nullptr, nullptr, 1, nullptr, k.res, k.lanes, nullptr};
  int rc;
  {
    const trk::FkLaunch a{d_states, m, ld, c->K, (bool)c->K.enable_rotation, false, c->d_tab, c->d_steps, (int)c->steps.size(),
                          c->d_poly, c->k_first, c->d_tgrid, c->d_hl, none, s};
    switch (c->K.n_tendons) {
#define TRK_CASE(N) case N: trk::launch_shoot_start<N>(a, d_guess, k.pn); break;
      TRK_CASE(1) TRK_CASE(2) TRK_CASE(3) TRK_CASE(4) TRK_CASE(5) TRK_CASE(6) TRK_CASE(7) TRK_CASE(8)
#undef TRK_CASE
      default: return fail(c, TR_ERR_OUT_OF_RANGE, "n_tendons out of range");
    }
    HIP_TRY(c, hipGetLastError());
  }
  auto read_count = [&](int slot, int64_t &active) -> int {
    HIP_TRY(c, hipMemcpyAsync(k.h_count, k.d_count + slot, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    active = (int64_t)*k.h_count;
    rounds++;
    return TR_OK;
  };
  // the start of every problem: one lane each
  int cur = 0;
  int64_t active = 0;
  HIP_TRY(c, hipMemsetAsync(k.d_count + cur, 0, sizeof(uint32_t), s));
  {
    trk::LoadedIn in = base;
    in.vu = k.pn;
    if ((rc = shoot_fk(c, d_states, m, ld, none, in, s))) return rc;
  }
  hipLaunchKernelGGL(trk::shoot_begin, dim3(ik_grid(m, 64)), dim3(64), 0, s, prm, st, m, (const double *)k.res, k.lanes, k.list[cur],
                     k.d_count + cur);
  HIP_TRY(c, hipGetLastError());
  if ((rc = read_count(cur, active))) return rc;
  while (active > 0) {
    const int nxt = cur ^ 1;
    HIP_TRY(c, hipMemsetAsync(k.d_count + nxt, 0, sizeof(uint32_t), s));
    hipLaunchKernelGGL(trk::ik_expand, dim3(ik_grid(active * Q, 256)), dim3(256), 0, s, (const double *)k.pn, (const int32_t *)k.list[cur],
                       active, 6, prm.delta, k.xs);
    HIP_TRY(c, hipGetLastError());
    trk::LoadedIn in = base;
    in.vu = k.xs; in.list = k.list[cur]; in.Q = Q;
    if ((rc = shoot_fk(c, d_states, active * Q, ld, none, in, s))) return rc;
    hipLaunchKernelGGL(trk::shoot_lm_step, dim3(ik_grid(active, 64)), dim3(64), 0, s, prm, st, (const int32_t *)k.list[cur], active,
                       (const double *)k.res, k.lanes, k.list[nxt], k.d_count + nxt);
    HIP_TRY(c, hipGetLastError());
    if ((rc = read_count(nxt, active))) return rc;
    cur = nxt;
  }
  // the outputs: every problem once more at its final strains (final_launch false: the caller wants the strains and flags only)
  if (final_launch) {
    trk::LoadedIn in = base;
    in.vu = k.p; in.res = nullptr; in.vu_tip = d_vuL;
    if ((rc = shoot_fk(c, d_states, m, ld, out, in, s))) return rc;
  }
  hipLaunchKernelGGL(trk::shoot_finish, dim3(ik_grid(m, 64)), dim3(64), 0, s, prm, st, m, d_vu0, d_res, d_iters, d_calls, d_conv);
  HIP_TRY(c, hipGetLastError());
  return TR_OK;
}

}  // namespace

extern "C" {

int tr_fk_loaded_batch_dev(tr_ctx *c, const tr_shoot_params *params, const double *d_states, int64_t n, int64_t ld,
                           const double *d_wrench, int64_t wrench_ld, const double *d_dist, int64_t dist_ld, const double *d_guess,
                           double *d_px, double *d_py, double *d_pz, double *d_R, double *d_L, double *d_Li, uint8_t *d_converged,
                           int32_t *d_n_points, double *d_vu0_out, double *d_vuL_out, double *d_residual_out, int32_t *d_iters_out,
                           int32_t *d_fk_calls_out, int64_t *rounds_out, void *stream) {
  if (!c) return TR_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lock_(c->mu);
  if (rounds_out) *rounds_out = 0;
  int rc;
  if ((rc = shoot_check(c, n, wrench_ld, dist_ld))) return rc;
  if (ld < n || (ld & 63)) return fail(c, TR_ERR_INVALID_ARG, "ld must be a multiple of 64 and >= n");
  if (n == 0) return TR_OK;
  if (!d_states) return fail(c, TR_ERR_INVALID_ARG, "null device pointer");
  if ((d_px || d_py || d_pz) && !(d_px && d_py && d_pz)) return fail(c, TR_ERR_INVALID_ARG, "d_px, d_py, d_pz: all or none");
  if (d_R && !d_px) return fail(c, TR_ERR_INVALID_ARG, "d_R needs the point planes");
  HIP_TRY(c, hipSetDevice(c->device));
  const hipStream_t s = (hipStream_t)stream;
  const int S = c->K.state_size;
  trk::ShootParams prm;
  if ((rc = shoot_params(c, params, prm))) return rc;
  if ((rc = begin_dev_work(c, s))) return rc;
  if ((rc = shoot_reserve(c, n))) return rc;
  const int64_t chunk = shoot_chunk_size(c);
  int64_t rounds = 0;
  for (int64_t off = 0; off < n; off += chunk) {
    const int64_t m = std::min(chunk, n - off);
    const trk::FkOut out{d_px ? d_px + off : nullptr, d_py ? d_py + off : nullptr, d_pz ? d_pz + off : nullptr, d_R ? d_R + off : nullptr,
                         d_L ? d_L + off : nullptr, d_Li ? d_Li + off : nullptr, nullptr, nullptr, d_n_points ? d_n_points + off : nullptr,
                         nullptr};
    if ((rc = shoot_chunk_solve(c, prm, d_states + off * S, m, ld, d_wrench ? d_wrench + off * wrench_ld : c->shoot.zero6,
                                d_wrench ? wrench_ld : 0, d_dist ? d_dist + off * dist_ld : nullptr, dist_ld,
                                d_guess ? d_guess + off * 6 : nullptr, out, d_converged ? d_converged + off : nullptr,
                                d_vu0_out ? d_vu0_out + off * 6 : nullptr, d_vuL_out ? d_vuL_out + off * 6 : nullptr,
                                d_residual_out ? d_residual_out + off : nullptr,
                                d_iters_out ? d_iters_out + off : nullptr, d_fk_calls_out ? d_fk_calls_out + off : nullptr, s, rounds)))
      return rc;
  }
  if (rounds_out) *rounds_out = rounds;
  return note_dev_work(c, s);
}

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
  const int64_t chunk = shoot_io_chunk(c);
  if ((rc = shoot_reserve(c, std::min(n, chunk)))) return rc;
  if ((rc = shoot_reserve_io(c, n, R != nullptr))) return rc;
  tr_ctx::ShootDev &k = c->shoot;
  // rows of a strided host array, packed to 6 doubles each (ld == 0: the one row)
  std::vector<double> rows;
  auto upload_rows = [&](double *d_dst, const double *src, int64_t src_ld, int64_t off, int64_t m) -> int {
    if (src_ld == 0) { HIP_TRY(c, hipMemcpy(d_dst, src, 6 * sizeof(double), hipMemcpyHostToDevice)); return TR_OK; }
    rows.resize((size_t)(m * 6));
    for (int64_t i = 0; i < m; i++) for (int q = 0; q < 6; q++) rows[(size_t)(i * 6 + q)] = src[(off + i) * src_ld + q];
    HIP_TRY(c, hipMemcpy(d_dst, rows.data(), rows.size() * sizeof(double), hipMemcpyHostToDevice));
    return TR_OK;
  };
  std::vector<double> hx, hy, hz, hR, hLi;
  int64_t rounds = 0;
  for (int64_t off = 0; off < n; off += chunk) {
    const int64_t m = std::min(chunk, n - off), ld = round_up(m, 64);
    HIP_TRY(c, hipMemcpy(k.io_states, states + off * S, (size_t)m * S * sizeof(double), hipMemcpyHostToDevice));
    if (wrench && (rc = upload_rows(k.io_w, wrench, wrench_ld, off, m))) return rc;
    if (dist && (rc = upload_rows(k.io_d, dist, dist_ld, off, m))) return rc;
    if (guess) HIP_TRY(c, hipMemcpy(k.io_g, guess + off * 6, (size_t)m * 6 * sizeof(double), hipMemcpyHostToDevice));
    const trk::FkOut out{p || R ? k.io_px : nullptr, p || R ? k.io_py : nullptr, p || R ? k.io_pz : nullptr, R ? k.io_R : nullptr, k.io_L, k.io_Li,
                         nullptr, nullptr, k.io_np, nullptr};
    if ((rc = shoot_chunk_solve(c, prm, k.io_states, m, ld, wrench ? k.io_w : k.zero6, wrench && wrench_ld ? 6 : 0, dist ? k.io_d : nullptr,
                                dist_ld ? 6 : 0, guess ? k.io_g : nullptr, out, k.io_conv, k.io_vu, k.io_vuL, k.io_e, k.io_it, k.io_fc, nullptr, rounds)))
      return rc;
    HIP_TRY(c, hipDeviceSynchronize());
    // device planes are [P][ld]; only the first m columns are copied (2-D copies, host pitch m)
    if (p) {
      hx.resize((size_t)P * m); hy.resize((size_t)P * m); hz.resize((size_t)P * m);
      HIP_TRY(c, hipMemcpy2D(hx.data(), (size_t)m * 8, k.io_px, (size_t)ld * 8, (size_t)m * 8, (size_t)P, hipMemcpyDeviceToHost));
      HIP_TRY(c, hipMemcpy2D(hy.data(), (size_t)m * 8, k.io_py, (size_t)ld * 8, (size_t)m * 8, (size_t)P, hipMemcpyDeviceToHost));
      HIP_TRY(c, hipMemcpy2D(hz.data(), (size_t)m * 8, k.io_pz, (size_t)ld * 8, (size_t)m * 8, (size_t)P, hipMemcpyDeviceToHost));
      for (int64_t i = 0; i < m; i++)
        for (int j = 0; j < P; j++) {
          double *o = p + ((size_t)(off + i) * P + j) * 3;
          o[0] = hx[(size_t)j * m + i]; o[1] = hy[(size_t)j * m + i]; o[2] = hz[(size_t)j * m + i];
        }
    }
    if (R) {
      hR.resize((size_t)9 * P * m);
      HIP_TRY(c, hipMemcpy2D(hR.data(), (size_t)m * 8, k.io_R, (size_t)ld * 8, (size_t)m * 8, (size_t)9 * P, hipMemcpyDeviceToHost));
      for (int64_t i = 0; i < m; i++)
        for (int j = 0; j < P; j++)
          for (int q = 0; q < 9; q++) R[((size_t)(off + i) * P + j) * 9 + q] = hR[((size_t)q * P + j) * m + i];
    }
    if (L) HIP_TRY(c, hipMemcpy(L + off, k.io_L, (size_t)m * sizeof(double), hipMemcpyDeviceToHost));
    if (L_i) {
      hLi.resize((size_t)N * m);
      HIP_TRY(c, hipMemcpy2D(hLi.data(), (size_t)m * 8, k.io_Li, (size_t)ld * 8, (size_t)m * 8, (size_t)N, hipMemcpyDeviceToHost));
      for (int64_t i = 0; i < m; i++) for (int j = 0; j < N; j++) L_i[(size_t)(off + i) * N + j] = hLi[(size_t)j * m + i];
    }
    if (converged) HIP_TRY(c, hipMemcpy(converged + off, k.io_conv, (size_t)m, hipMemcpyDeviceToHost));
    if (n_points) HIP_TRY(c, hipMemcpy(n_points + off, k.io_np, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (vu0_out) HIP_TRY(c, hipMemcpy(vu0_out + off * 6, k.io_vu, (size_t)m * 6 * sizeof(double), hipMemcpyDeviceToHost));
    if (vuL_out) HIP_TRY(c, hipMemcpy(vuL_out + off * 6, k.io_vuL, (size_t)m * 6 * sizeof(double), hipMemcpyDeviceToHost));
    if (residual_out) HIP_TRY(c, hipMemcpy(residual_out + off, k.io_e, (size_t)m * sizeof(double), hipMemcpyDeviceToHost));
    if (iters_out) HIP_TRY(c, hipMemcpy(iters_out + off, k.io_it, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (fk_calls_out) HIP_TRY(c, hipMemcpy(fk_calls_out + off, k.io_fc, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost));
  }
  if (rounds_out) *rounds_out = rounds;
  return TR_OK;
}

}  // extern "C"
