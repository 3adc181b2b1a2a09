// loaded_ik_host.inc -- tip inverse kinematics on loaded shapes behind the C ABI (tr_ik_loaded_batch*): tr_ik_batch's outer loop
// (ik_host.inc) with the loaded rod's tip and the implicit-function tip Jacobian (loaded_ik_kernel.hpp).  Every problem's state
// stays on the device.  Per outer round: one gather of the active problems' trial states, load rows and predicted strains; the
// shooting of loaded_host.inc on those rows (shoot_chunk_solve without its output launch: the host reads one 4-byte count per
// shooting round); one launch of 13 + 2 S lanes per active problem (fk_loaded_lin); one LM-step launch, after which the host reads
// the 4-byte active count of the next round.
// Included at the end of tendon_hip.hip (needs tr_ctx, ik_host.inc's and loaded_host.inc's helpers).
namespace {

// problems per chunk: what the shooting workspace takes in one go (TENDON_HIP_SHOOT_CHUNK is honoured) and what kIkLanes holds of
// the linearisation's lanes; each chunk is solved to the end (a problem's iterates do not depend on the others)
int64_t ikl_chunk(const tr_ctx *c) { return std::min<int64_t>(shoot_chunk_size(c), kIkLanes / (13 + 2 * c->K.state_size)); }

void ikl_release(tr_ctx *c) {
  tr_ctx::IklDev &k = c->ikl;
  void *p[] = {k.lin, k.p, k.pn, k.y, k.W, k.J, k.f, k.des, k.err2, k.mu, k.nu, k.iters, k.calls, k.list[0], k.list[1], k.eq, k.row_s, k.row_w,
               k.row_d, k.row_g, k.row_vu, k.row_conv, k.row_calls, k.d_count, k.io_s, k.io_3, k.io_g, k.io_e, k.io_vu, k.io_i, k.io_c, k.io_eq,
               k.sens_c, k.sens_b, k.sens_n};
  for (void *q : p) if (q) (void)hipFree(q);
  if (k.h_count) (void)hipHostFree(k.h_count);
  k = tr_ctx::IklDev{};
}

// the workspace for chunks of up to `n` problems (grow-only, released with the context)
int ikl_reserve(tr_ctx *c, int64_t n) {
  tr_ctx::IklDev &k = c->ikl;
  const int64_t S = c->K.state_size, Q = 13 + 2 * S;
  const int64_t probs = round_up(std::max<int64_t>(1, std::min(n, ikl_chunk(c))), 64), lanes = round_up(probs * Q, 64);
  int rc;
  if (!k.d_count) {
    if ((rc = dev_alloc(c, &k.d_count, 2))) return rc;
    HIP_TRY(c, hipHostMalloc((void **)&k.h_count, sizeof(uint32_t), hipHostMallocDefault));
  }
  if (k.probs >= probs) return TR_OK;
  HIP_TRY(c, hipDeviceSynchronize());
  if ((rc = dev_alloc(c, &k.lin, (size_t)(lanes * 9)))) return rc;
  if ((rc = dev_alloc(c, &k.p, (size_t)(probs * S)))) return rc;
  if ((rc = dev_alloc(c, &k.pn, (size_t)(probs * S)))) return rc;
  if ((rc = dev_alloc(c, &k.y, (size_t)(probs * 6)))) return rc;
  if ((rc = dev_alloc(c, &k.W, (size_t)(probs * 6 * S)))) return rc;
  if ((rc = dev_alloc(c, &k.J, (size_t)(probs * 3 * S)))) return rc;
  if ((rc = dev_alloc(c, &k.f, (size_t)(probs * 3)))) return rc;
  if ((rc = dev_alloc(c, &k.des, (size_t)(probs * 3)))) return rc;
  if ((rc = dev_alloc(c, &k.err2, (size_t)probs))) return rc;
  if ((rc = dev_alloc(c, &k.mu, (size_t)probs))) return rc;
  if ((rc = dev_alloc(c, &k.nu, (size_t)probs))) return rc;
  if ((rc = dev_alloc(c, &k.iters, (size_t)probs))) return rc;
  if ((rc = dev_alloc(c, &k.calls, (size_t)probs))) return rc;
  if ((rc = dev_alloc(c, &k.eq, (size_t)probs))) return rc;
  for (int q = 0; q < 2; q++) if ((rc = dev_alloc(c, &k.list[q], (size_t)probs))) return rc;
  if ((rc = dev_alloc(c, &k.row_s, (size_t)(probs * S)))) return rc;
  if ((rc = dev_alloc(c, &k.row_w, (size_t)(probs * 6)))) return rc;
  if ((rc = dev_alloc(c, &k.row_d, (size_t)(probs * 6)))) return rc;
  if ((rc = dev_alloc(c, &k.row_g, (size_t)(probs * 6)))) return rc;
  if ((rc = dev_alloc(c, &k.row_vu, (size_t)(probs * 6)))) return rc;
  if ((rc = dev_alloc(c, &k.row_conv, (size_t)probs))) return rc;
  if ((rc = dev_alloc(c, &k.row_calls, (size_t)probs))) return rc;
  // staging of the host-array form
  if ((rc = dev_alloc(c, &k.io_s, (size_t)(probs * S)))) return rc;
  if ((rc = dev_alloc(c, &k.io_3, (size_t)(probs * 3)))) return rc;
  if ((rc = dev_alloc(c, &k.io_g, (size_t)(probs * 6)))) return rc;
  if ((rc = dev_alloc(c, &k.io_vu, (size_t)(probs * 6)))) return rc;
  if ((rc = dev_alloc(c, &k.io_e, (size_t)probs))) return rc;
  if ((rc = dev_alloc(c, &k.io_i, (size_t)probs))) return rc;
  if ((rc = dev_alloc(c, &k.io_c, (size_t)probs))) return rc;
  if ((rc = dev_alloc(c, &k.io_eq, (size_t)probs))) return rc;
  k.probs = probs;
  k.lanes = lanes;
  return TR_OK;
}

// everything one call fixes before its first chunk
struct IklCall {
  trk::IkParams prm;
  trk::ShootParams sprm;
  trk::IklLoads loads;
  bool has_loads;
};

// what both forms refuse, and the call's parameters
int ikl_begin(tr_ctx *c, const tr_ik_params *params, const tr_shoot_params *shoot, const tr_edge_loads *loads, int64_t n, int64_t des_ld,
              const double *lo, const double *hi, IklCall &call) {
  int rc;
  if ((rc = shoot_check(c, n, 0, 0))) return rc;
  call.loads = trk::IklLoads{};
  call.has_loads = loads != nullptr;
  if (loads) {
    if (loads->frame != TR_LOAD_FRAME_BASE && loads->frame != TR_LOAD_FRAME_WORLD)
      return fail(c, TR_ERR_INVALID_ARG, "bad argument (frame: TR_LOAD_FRAME_BASE or TR_LOAD_FRAME_WORLD)");
    for (int q = 0; q < 6; q++) { call.loads.wrench[q] = loads->wrench[q]; call.loads.dist[q] = loads->dist[q]; }
    call.loads.world = loads->frame == TR_LOAD_FRAME_WORLD;
  }
  if (des_ld != 0 && des_ld < 3) return fail(c, TR_ERR_INVALID_ARG, "bad argument (des_ld: 0 or >= 3)");
  if ((rc = ik_params(c, params, lo, hi, call.prm))) return rc;
  for (int d = 0; d < call.prm.S; d++)
    if (!(call.prm.lo[d] <= call.prm.hi[d])) return fail(c, TR_ERR_INVALID_ARG, "bad argument (bounds: lo <= hi)");
  // shoot == NULL: tr_fk_loaded_batch's defaults without the relative-step stop.  A trial starts from predicted strains, so the
  // shooting's steps are small from the first; with stop_threshold_Dp = 1e-4 it then ends trials short of the threshold, which are
  // rejected steps of the outer iteration (config1 under gravity: up to 31 outer iterations where 6 do).
  const tr_shoot_params warm{100, 0.1, 1e-9, 0.0, 1e-6};
  return shoot_params(c, shoot ? shoot : &warm, call.sprm);
}

// one chunk of m problems to the end: d_init m x S, goals d_des (row stride des_ld, 0 = one row), d_guess m x 6 or null; outputs may
// be null.  rounds[0] counts the outer rounds, rounds[1] the shooting's.
int ikl_chunk_solve(tr_ctx *c, const IklCall &call, const double *d_init, int64_t m, const double *d_des, int64_t des_ld,
                    const double *d_guess, double *d_states, double *d_tips, double *d_err, int32_t *d_iters, int32_t *d_calls, double *d_vu0,
                    uint8_t *d_eq, hipStream_t s, int64_t rounds[2]) {
  tr_ctx::IklDev &k = c->ikl;
  const trk::IkParams &prm = call.prm;
  const int S = prm.S, Q = 13 + 2 * S;
  const trk::IklState st{k.p, k.pn, k.y, k.W, k.J, k.f, k.des, k.err2, k.mu, k.nu, k.iters, k.calls, k.eq};
  const trk::IklRows rows{k.row_s, k.row_w, k.row_d, k.row_g, k.row_vu, k.row_conv, k.row_calls};
  const trk::FkOut none{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  trk::LinIn lin{};
  lin.states = k.row_s; lin.vu = k.row_vu;
  for (int q = 0; q < 6; q++) { lin.wrench[q] = call.loads.wrench[q]; lin.dist[q] = call.loads.dist[q]; }
  lin.world = call.loads.world; lin.Q = Q;
  lin.delta_y = call.sprm.delta; lin.delta_p = prm.delta;
  lin.tip_route = c->shoot.tip_route;
  lin.out = k.lin; lin.ldr = k.lanes;
  hipLaunchKernelGGL(trk::ikl_init, dim3(ik_grid(m, 64)), dim3(64), 0, s, d_init, m, d_des, des_ld, prm, st);
  HIP_TRY(c, hipGetLastError());
  int64_t active = m;
  int cur = 0, rc;
  for (bool init = true; active > 0; init = false) {
    const int nxt = cur ^ 1;
    const int32_t *list = init ? nullptr : k.list[cur];
    HIP_TRY(c, hipMemsetAsync(k.d_count + nxt, 0, sizeof(uint32_t), s));
    hipLaunchKernelGGL(trk::ikl_gather, dim3(ik_grid(active, 64)), dim3(64), 0, s, prm, st, list, active, call.loads, d_guess, rows);
    HIP_TRY(c, hipGetLastError());
    if ((rc = shoot_chunk_solve(c, call.sprm, k.row_s, active, round_up(active, 64), k.row_w, 6, call.has_loads ? k.row_d : nullptr, 6,
                                (init && !d_guess) ? nullptr : k.row_g, none, k.row_conv, k.row_vu, nullptr, nullptr, nullptr, k.row_calls,
                                s, rounds[1], false)))
      return rc;
    const trk::FkLaunch a{nullptr, active * Q, round_up(active * Q, 64), c->K, (bool)c->K.enable_rotation, false, c->d_tab, c->d_steps,
                          (int)c->steps.size(), c->d_poly, c->k_first, c->d_tgrid, c->d_hl, none, s};
    switch (c->K.n_tendons) {
#define TRK_CASE(N) case N: trk::launch_fk_loaded_lin<N>(a, lin); break;
      TRK_CASE(1) TRK_CASE(2) TRK_CASE(3) TRK_CASE(4) TRK_CASE(5) TRK_CASE(6) TRK_CASE(7) TRK_CASE(8)
#undef TRK_CASE
      default: return fail(c, TR_ERR_OUT_OF_RANGE, "n_tendons out of range");
    }
    HIP_TRY(c, hipGetLastError());
    switch (S) {
#define TRK_CASE(SS) case SS: hipLaunchKernelGGL((trk::ikl_lm_step<SS>), dim3(ik_grid(active, 64)), dim3(64), 0, s, prm, call.sprm.delta, st, list, \
                                                 active, (const double *)k.lin, k.lanes, rows, (int)init, k.list[nxt], k.d_count + nxt); break;
      TRK_CASE(1) TRK_CASE(2) TRK_CASE(3) TRK_CASE(4) TRK_CASE(5) TRK_CASE(6) TRK_CASE(7) TRK_CASE(8) TRK_CASE(9) TRK_CASE(10)
#undef TRK_CASE
      default: return fail(c, TR_ERR_OUT_OF_RANGE, "state size out of range");
    }
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(k.h_count, k.d_count + nxt, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    active = (int64_t)*k.h_count;
    cur = nxt;
    rounds[0]++;
  }
  hipLaunchKernelGGL(trk::ikl_finish, dim3(ik_grid(m, 64)), dim3(64), 0, s, prm, st, m, d_states, d_tips, d_err, d_iters, d_calls, d_vu0, d_eq);
  HIP_TRY(c, hipGetLastError());
  return TR_OK;
}

}  // namespace

extern "C" {

int tr_ik_loaded_batch_dev(tr_ctx *c, const tr_ik_params *params, const tr_shoot_params *shoot, const tr_edge_loads *loads,
                           const double *d_initial_states, int64_t n, const double *d_des, int64_t des_ld, const double *lo,
                           const double *hi, const double *d_guess, double *d_states_out, double *d_tips_out, double *d_error_out,
                           int32_t *d_iters_out, int32_t *d_fk_calls_out, double *d_vu0_out, uint8_t *d_equilibrium_out,
                           int64_t *rounds_out, void *stream) {
  if (!c) return TR_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lock_(c->mu);
  if (rounds_out) rounds_out[0] = rounds_out[1] = 0;
  IklCall call;
  int rc;
  if ((rc = ikl_begin(c, params, shoot, loads, n, des_ld, lo, hi, call))) return rc;
  if (n == 0) return TR_OK;
  if (!d_initial_states || !d_des) return fail(c, TR_ERR_INVALID_ARG, "null device pointer");
  HIP_TRY(c, hipSetDevice(c->device));
  const hipStream_t s = (hipStream_t)stream;
  const int S = c->K.state_size;
  if ((rc = begin_dev_work(c, s))) return rc;
  const int64_t chunk = ikl_chunk(c);
  if ((rc = shoot_reserve(c, std::min(n, chunk)))) return rc;
  if ((rc = ikl_reserve(c, n))) return rc;
  int64_t rounds[2] = {0, 0};
  for (int64_t off = 0; off < n; off += chunk) {
    const int64_t m = std::min(chunk, n - off);
    if ((rc = ikl_chunk_solve(c, call, d_initial_states + off * S, m, d_des + off * des_ld, des_ld, d_guess ? d_guess + off * 6 : nullptr,
                              d_states_out ? d_states_out + off * S : nullptr, d_tips_out ? d_tips_out + off * 3 : nullptr,
                              d_error_out ? d_error_out + off : nullptr, d_iters_out ? d_iters_out + off : nullptr,
                              d_fk_calls_out ? d_fk_calls_out + off : nullptr, d_vu0_out ? d_vu0_out + off * 6 : nullptr,
                              d_equilibrium_out ? d_equilibrium_out + off : nullptr, s, rounds))) return rc;
  }
  HIP_TRY(c, hipStreamSynchronize(s));
  if (rounds_out) { rounds_out[0] = rounds[0]; rounds_out[1] = rounds[1]; }
  return note_dev_work(c, s);
}

int tr_ik_loaded_batch(tr_ctx *c, const tr_ik_params *params, const tr_shoot_params *shoot, const tr_edge_loads *loads,
                       const double *initial_states, int64_t n, const double *des, int64_t des_ld, const double *lo, const double *hi,
                       const double *guess, double *states_out, double *tips_out, double *error_out, int32_t *iters_out,
                       int32_t *fk_calls_out, double *vu0_out, uint8_t *equilibrium_out, int64_t *rounds_out) {
  if (!c) return TR_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lock_(c->mu);
  if (rounds_out) rounds_out[0] = rounds_out[1] = 0;
  IklCall call;
  int rc;
  if ((rc = ikl_begin(c, params, shoot, loads, n, des_ld, lo, hi, call))) return rc;
  if (n == 0) return TR_OK;
  if (!initial_states || !des) return fail(c, TR_ERR_INVALID_ARG, "bad argument");
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipDeviceSynchronize());          // the workspace is shared with *_dev calls that may still run on other streams
  const int S = c->K.state_size;
  const int64_t chunk = ikl_chunk(c);
  if ((rc = shoot_reserve(c, std::min(n, chunk)))) return rc;
  if ((rc = ikl_reserve(c, n))) return rc;
  tr_ctx::IklDev &k = c->ikl;
  std::vector<double> dbuf;
  int64_t rounds[2] = {0, 0};
  for (int64_t off = 0; off < n; off += chunk) {
    const int64_t m = std::min(chunk, n - off);
    HIP_TRY(c, hipMemcpy(k.io_s, initial_states + off * S, (size_t)(m * S) * sizeof(double), hipMemcpyHostToDevice));
    if (des_ld == 0) {
      HIP_TRY(c, hipMemcpy(k.io_3, des, 3 * sizeof(double), hipMemcpyHostToDevice));
    } else {
      dbuf.resize((size_t)(m * 3));
      for (int64_t i = 0; i < m; i++) for (int q = 0; q < 3; q++) dbuf[(size_t)(i * 3 + q)] = des[(off + i) * des_ld + q];
      HIP_TRY(c, hipMemcpy(k.io_3, dbuf.data(), (size_t)(m * 3) * sizeof(double), hipMemcpyHostToDevice));
    }
    if (guess) HIP_TRY(c, hipMemcpy(k.io_g, guess + off * 6, (size_t)(m * 6) * sizeof(double), hipMemcpyHostToDevice));
    // (io_s / io_3 are read by ikl_init, io_g by the first gather, before ikl_finish overwrites io_s / io_3 with the results)
    if ((rc = ikl_chunk_solve(c, call, k.io_s, m, k.io_3, des_ld ? 3 : 0, guess ? k.io_g : nullptr, k.io_s, k.io_3, k.io_e, k.io_i, k.io_c,
                              k.io_vu, k.io_eq, nullptr, rounds))) return rc;
    if (states_out) HIP_TRY(c, hipMemcpy(states_out + off * S, k.io_s, (size_t)(m * S) * sizeof(double), hipMemcpyDeviceToHost));
    if (tips_out) HIP_TRY(c, hipMemcpy(tips_out + off * 3, k.io_3, (size_t)(m * 3) * sizeof(double), hipMemcpyDeviceToHost));
    if (error_out) HIP_TRY(c, hipMemcpy(error_out + off, k.io_e, (size_t)m * sizeof(double), hipMemcpyDeviceToHost));
    if (iters_out) HIP_TRY(c, hipMemcpy(iters_out + off, k.io_i, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (fk_calls_out) HIP_TRY(c, hipMemcpy(fk_calls_out + off, k.io_c, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (vu0_out) HIP_TRY(c, hipMemcpy(vu0_out + off * 6, k.io_vu, (size_t)(m * 6) * sizeof(double), hipMemcpyDeviceToHost));
    if (equilibrium_out) HIP_TRY(c, hipMemcpy(equilibrium_out + off, k.io_eq, (size_t)m, hipMemcpyDeviceToHost));
  }
  if (rounds_out) { rounds_out[0] = rounds[0]; rounds_out[1] = rounds[1]; }
  return TR_OK;
}

}  // extern "C"
