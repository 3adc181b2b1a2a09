// loaded_jacobian_host.inc -- the loaded tip Jacobian and tip compliance behind the C ABI (tr_tip_jacobian_loaded*): one round of
// the loaded IK's loop (loaded_ik_host.inc) without a goal.  Per chunk of problems: one gather of the states, their load rows and the
// caller's guess rows (ikl_gather); the shooting of loaded_host.inc on those rows (shoot_chunk_solve without its output launch: the
// host reads one 4-byte count per shooting round and nothing else); one launch of 13 + 2 S lanes per problem (fk_loaded_lin); one
// launch of loaded_tip_sens (loaded_sens_kernel.hpp), one lane per problem, which writes the outputs.  The workspace is the loaded
// IK's (ikl_reserve) and the shooting's (shoot_reserve).
// Included at the end of tendon_hip.hip, after loaded_ik_host.inc.
namespace {

// staging of the host-array form's outputs that the loaded IK's workspace has no room for
int sens_reserve_io(tr_ctx *c) {
  tr_ctx::IklDev &k = c->ikl;
  if (k.sens_probs >= k.probs) return TR_OK;
  const int64_t S = c->K.state_size;
  int rc;
  HIP_TRY(c, hipDeviceSynchronize());
  if ((rc = dev_alloc(c, &k.sens_c, (size_t)(k.probs * 18)))) return rc;
  if ((rc = dev_alloc(c, &k.sens_b, (size_t)(k.probs * (69 + 9 * S))))) return rc;
  if ((rc = dev_alloc(c, &k.sens_n, (size_t)k.probs))) return rc;
  k.sens_probs = k.probs;
  return TR_OK;
}

// everything one call fixes before its first chunk
struct SensCall {
  trk::IkParams prm;          // S, rot_index and delta are read
  trk::ShootParams sprm;
  trk::IklLoads loads;
  bool has_loads;
};

// what both forms refuse, and the call's parameters
int sens_begin(tr_ctx *c, const tr_shoot_params *shoot, const tr_edge_loads *loads, int64_t n, double delta, SensCall &call) {
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
  if (!(delta > 0.0)) return fail(c, TR_ERR_INVALID_ARG, "bad argument (delta must be > 0)");
  if ((rc = ik_params(c, nullptr, nullptr, nullptr, call.prm))) return rc;
  call.prm.delta = delta;
  return shoot_params(c, shoot, call.sprm);
}

// one chunk of m problems: d_states m x S, d_guess m x 6 or null; `out`: the chunk's first row of every wanted output
int sens_chunk_solve(tr_ctx *c, const SensCall &call, const double *d_states, int64_t m, const double *d_guess, const trk::SensOut &out,
                     hipStream_t s, int64_t &rounds) {
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
  int rc;
  // the states are the gather's trial points as they stand (no bounds here)
  HIP_TRY(c, hipMemcpyAsync(k.pn, d_states, (size_t)(m * S) * sizeof(double), hipMemcpyDeviceToDevice, s));
  hipLaunchKernelGGL(trk::ikl_gather, dim3(ik_grid(m, 64)), dim3(64), 0, s, prm, st, (const int32_t *)nullptr, m, call.loads, d_guess, rows);
  HIP_TRY(c, hipGetLastError());
  if ((rc = shoot_chunk_solve(c, call.sprm, k.row_s, m, round_up(m, 64), k.row_w, 6, call.has_loads ? k.row_d : nullptr, 6,
                              d_guess ? k.row_g : nullptr, none, k.row_conv, k.row_vu, nullptr, nullptr, nullptr, k.row_calls, s, rounds,
                              false)))
    return rc;
  const trk::FkLaunch a{nullptr, m * Q, round_up(m * Q, 64), c->K, (bool)c->K.enable_rotation, false, c->d_tab, c->d_steps,
                        (int)c->steps.size(), c->d_poly, c->k_first, c->d_tgrid, c->d_hl, none, s};
  switch (c->K.n_tendons) {
#define TRK_CASE(N) case N: trk::launch_fk_loaded_lin<N>(a, lin); break;
    TRK_CASE(1) TRK_CASE(2) TRK_CASE(3) TRK_CASE(4) TRK_CASE(5) TRK_CASE(6) TRK_CASE(7) TRK_CASE(8)
#undef TRK_CASE
    default: return fail(c, TR_ERR_OUT_OF_RANGE, "n_tendons out of range");
  }
  HIP_TRY(c, hipGetLastError());
  switch (S) {
#define TRK_CASE(SS) case SS: hipLaunchKernelGGL((trk::loaded_tip_sens<SS>), dim3(ik_grid(m, 64)), dim3(64), 0, s, prm.delta, call.sprm.delta, \
                                                 (int)prm.rot_index, (int)call.loads.world, m, (const double *)k.lin, k.lanes, rows, out); break;
    TRK_CASE(1) TRK_CASE(2) TRK_CASE(3) TRK_CASE(4) TRK_CASE(5) TRK_CASE(6) TRK_CASE(7) TRK_CASE(8) TRK_CASE(9) TRK_CASE(10)
#undef TRK_CASE
    default: return fail(c, TR_ERR_OUT_OF_RANGE, "state size out of range");
  }
  HIP_TRY(c, hipGetLastError());
  return TR_OK;
}

}  // namespace

extern "C" {

int tr_tip_jacobian_loaded_dev(tr_ctx *c, const tr_shoot_params *shoot, const tr_edge_loads *loads, const double *d_states, int64_t n,
                               double delta, const double *d_guess, double *d_tips, double *d_J, double *d_compliance, double *d_W,
                               double *d_vu0, uint8_t *d_equilibrium, double *d_blocks, int64_t *d_n_integrations, int64_t *rounds_out,
                               void *stream) {
  if (!c) return TR_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lock_(c->mu);
  if (rounds_out) *rounds_out = 0;
  SensCall call;
  int rc;
  if ((rc = sens_begin(c, shoot, loads, n, delta, call))) return rc;
  if (n == 0) return TR_OK;
  if (!d_states) return fail(c, TR_ERR_INVALID_ARG, "null device pointer");
  HIP_TRY(c, hipSetDevice(c->device));
  const hipStream_t s = (hipStream_t)stream;
  const int64_t S = c->K.state_size, NB = 69 + 9 * S;
  if ((rc = begin_dev_work(c, s))) return rc;
  const int64_t chunk = ikl_chunk(c);
  if ((rc = shoot_reserve(c, std::min(n, chunk)))) return rc;
  if ((rc = ikl_reserve(c, n))) return rc;
  int64_t rounds = 0;
  for (int64_t off = 0; off < n; off += chunk) {
    const int64_t m = std::min(chunk, n - off);
    const trk::SensOut out{d_tips ? d_tips + off * 3 : nullptr, d_vu0 ? d_vu0 + off * 6 : nullptr, d_J ? d_J + off * 3 * S : nullptr,
                           d_W ? d_W + off * 6 * S : nullptr, d_compliance ? d_compliance + off * 18 : nullptr,
                           d_blocks ? d_blocks + off * NB : nullptr, d_equilibrium ? d_equilibrium + off : nullptr,
                           d_n_integrations ? d_n_integrations + off : nullptr};
    if ((rc = sens_chunk_solve(c, call, d_states + off * S, m, d_guess ? d_guess + off * 6 : nullptr, out, s, rounds))) return rc;
  }
  HIP_TRY(c, hipStreamSynchronize(s));
  if (rounds_out) *rounds_out = rounds;
  return note_dev_work(c, s);
}

int tr_tip_jacobian_loaded(tr_ctx *c, const tr_shoot_params *shoot, const tr_edge_loads *loads, const double *states, int64_t n,
                           double delta, const double *guess, double *tips, double *J, double *compliance, double *W, double *vu0,
                           uint8_t *equilibrium, double *blocks, int64_t *n_integrations, int64_t *rounds_out) {
  if (!c) return TR_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lock_(c->mu);
  if (rounds_out) *rounds_out = 0;
  SensCall call;
  int rc;
  if ((rc = sens_begin(c, shoot, loads, n, delta, call))) return rc;
  if (n == 0) return TR_OK;
  if (!states) return fail(c, TR_ERR_INVALID_ARG, "bad argument");
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipDeviceSynchronize());          // the workspace is shared with *_dev calls that may still run on other streams
  const int64_t S = c->K.state_size, NB = 69 + 9 * S;
  const int64_t chunk = ikl_chunk(c);
  if ((rc = shoot_reserve(c, std::min(n, chunk)))) return rc;
  if ((rc = ikl_reserve(c, n))) return rc;
  if ((rc = sens_reserve_io(c))) return rc;
  tr_ctx::IklDev &k = c->ikl;
  int64_t rounds = 0;
  for (int64_t off = 0; off < n; off += chunk) {
    const int64_t m = std::min(chunk, n - off);
    HIP_TRY(c, hipMemcpy(k.io_s, states + off * S, (size_t)(m * S) * sizeof(double), hipMemcpyHostToDevice));
    if (guess) HIP_TRY(c, hipMemcpy(k.io_g, guess + off * 6, (size_t)(m * 6) * sizeof(double), hipMemcpyHostToDevice));
    // the problem-indexed rows of the loaded IK's state that this call does not use stage J, W and the strains
    const trk::SensOut out{tips ? k.io_3 : nullptr, vu0 ? k.io_vu : nullptr, J ? k.J : nullptr, W ? k.W : nullptr,
                           compliance ? k.sens_c : nullptr, blocks ? k.sens_b : nullptr, equilibrium ? k.io_eq : nullptr,
                           n_integrations ? k.sens_n : nullptr};
    if ((rc = sens_chunk_solve(c, call, k.io_s, m, guess ? k.io_g : nullptr, out, nullptr, rounds))) return rc;
    if (tips) HIP_TRY(c, hipMemcpy(tips + off * 3, k.io_3, (size_t)(m * 3) * sizeof(double), hipMemcpyDeviceToHost));
    if (vu0) HIP_TRY(c, hipMemcpy(vu0 + off * 6, k.io_vu, (size_t)(m * 6) * sizeof(double), hipMemcpyDeviceToHost));
    if (J) HIP_TRY(c, hipMemcpy(J + off * 3 * S, k.J, (size_t)(m * 3 * S) * sizeof(double), hipMemcpyDeviceToHost));
    if (W) HIP_TRY(c, hipMemcpy(W + off * 6 * S, k.W, (size_t)(m * 6 * S) * sizeof(double), hipMemcpyDeviceToHost));
    if (compliance) HIP_TRY(c, hipMemcpy(compliance + off * 18, k.sens_c, (size_t)(m * 18) * sizeof(double), hipMemcpyDeviceToHost));
    if (blocks) HIP_TRY(c, hipMemcpy(blocks + off * NB, k.sens_b, (size_t)(m * NB) * sizeof(double), hipMemcpyDeviceToHost));
    if (equilibrium) HIP_TRY(c, hipMemcpy(equilibrium + off, k.io_eq, (size_t)m, hipMemcpyDeviceToHost));
    if (n_integrations) HIP_TRY(c, hipMemcpy(n_integrations + off, k.sens_n, (size_t)m * sizeof(int64_t), hipMemcpyDeviceToHost));
  }
  if (rounds_out) *rounds_out = rounds;
  return TR_OK;
}

}  // extern "C"
