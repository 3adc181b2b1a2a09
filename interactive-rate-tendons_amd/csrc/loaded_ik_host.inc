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
  k.chunk.release(); k.once.release(); k.sens.release(); k.count.release();
  k = tr_ctx::IklDev{};
}

// the workspace for chunks of up to `n` problems (grow-only, released with the context)
int ikl_reserve(tr_ctx *c, int64_t n) {
  tr_ctx::IklDev &k = c->ikl;
  const int64_t S = c->K.state_size, Q = 13 + 2 * S;
  const int64_t probs = round_up(std::max<int64_t>(1, std::min(n, ikl_chunk(c))), 64), lanes = round_up(probs * Q, 64);
  int rc;
  if ((rc = k.count.reserve(c, k.once))) return rc;
  if (k.probs >= probs) return TR_OK;
  HIP_TRY(c, hipDeviceSynchronize());
  DevOwner &o = k.chunk;
  o.release();
  k.probs = k.lanes = 0;                       // (no buffer is usable until all of them exist again)
  if ((rc = o.alloc(c, &k.lin, (size_t)(lanes * 9)))) return rc;
  // per problem, by shape (row_*: the rows of one round in list order; io_*: the staging of the host-array form)
  if ((rc = o.alloc_all(c, {&k.p, &k.pn, &k.row_s, &k.io_s}, (size_t)(probs * S)))) return rc;
  if ((rc = o.alloc_all(c, {&k.y, &k.row_w, &k.row_d, &k.row_g, &k.row_vu, &k.io_g, &k.io_vu}, (size_t)(probs * 6)))) return rc;
  if ((rc = o.alloc(c, &k.W, (size_t)(probs * 6 * S))) || (rc = o.alloc(c, &k.J, (size_t)(probs * 3 * S)))) return rc;
  if ((rc = o.alloc_all(c, {&k.f, &k.des, &k.io_3}, (size_t)(probs * 3)))) return rc;
  if ((rc = o.alloc_all(c, {&k.err2, &k.mu, &k.nu, &k.io_e}, (size_t)probs))) return rc;
  if ((rc = o.alloc_all(c, {&k.iters, &k.calls, &k.list[0], &k.list[1], &k.row_calls, &k.io_i, &k.io_c}, (size_t)probs))) return rc;
  if ((rc = o.alloc_all(c, {&k.eq, &k.row_conv, &k.io_eq}, (size_t)probs))) return rc;
  k.probs = probs;
  k.lanes = lanes;
  return TR_OK;
}

// everything one call fixes before its first chunk (the loaded Jacobian's calls too: of prm they read S, rot_index and delta)
struct IklCall {
  trk::IkParams prm;
  trk::ShootParams sprm;
  trk::IklLoads loads;
  bool has_loads;
};

// what every call on loaded tips refuses first (`what` names the call to a robot with retraction), and its load set
int ikl_begin_loads(tr_ctx *c, const tr_edge_loads *loads, int64_t n, IklCall &call, const char *what) {
  int rc;
  if ((rc = shoot_check(c, n, 0, 0)) || (rc = refuse_retraction(c, what))) return rc;
  call.has_loads = loads != nullptr;
  return parse_loads(c, loads, call.loads);
}

// what both forms refuse, and the call's parameters
int ikl_begin(tr_ctx *c, const tr_ik_params *params, const tr_shoot_params *shoot, const tr_edge_loads *loads, int64_t n, int64_t des_ld,
              const double *lo, const double *hi, IklCall &call) {
  int rc;
  if ((rc = ikl_begin_loads(c, loads, n, call, "loaded tip IK (tr_ik_loaded_batch*)"))) return rc;
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

trk::IklState ikl_state(tr_ctx *c) {
  tr_ctx::IklDev &k = c->ikl;
  return trk::IklState{k.p, k.pn, k.y, k.W, k.J, k.f, k.des, k.err2, k.mu, k.nu, k.iters, k.calls, k.eq};
}
trk::IklRows ikl_rows(tr_ctx *c) {
  tr_ctx::IklDev &k = c->ikl;
  return trk::IklRows{k.row_s, k.row_w, k.row_d, k.row_g, k.row_vu, k.row_conv, k.row_calls};
}

// One linearisation round over the `active` problems of `list` (null: problems 0 .. active - 1, a chunk's first round), at their trial
// states pn: the gather of their states, load rows and start strains (d_guess: the caller's m x 6 rows or null; without them a
// first round starts cold, a later one from the predicted strains); the shooting on those rows, without its output launch (its
// rounds are added to shoot_rounds); the launch of 13 + 2 S lanes per problem into the planes k.lin.
int ikl_linearise(tr_ctx *c, const IklCall &call, const int32_t *list, int64_t active, const double *d_guess, hipStream_t s,
                  int64_t &shoot_rounds) {
  tr_ctx::IklDev &k = c->ikl;
  const int Q = 13 + 2 * call.prm.S;
  trk::LinIn lin{};
  lin.states = k.row_s; lin.vu = k.row_vu;
  for (int q = 0; q < 6; q++) { lin.wrench[q] = call.loads.wrench[q]; lin.dist[q] = call.loads.dist[q]; }
  lin.world = call.loads.world; lin.Q = Q;
  lin.delta_y = call.sprm.delta; lin.delta_p = call.prm.delta;
  lin.tip_route = c->shoot.tip_route;
  lin.weights = profile_weights(c);
  lin.out = k.lin; lin.ldr = k.lanes;
  hipLaunchKernelGGL(trk::ikl_gather, dim3(ik_grid(active, 64)), dim3(64), 0, s, call.prm, ikl_state(c), list, active, call.loads, d_guess,
                     ikl_rows(c));
  HIP_TRY(c, hipGetLastError());
  if (const int rc = shoot_chunk_solve(c, call.sprm, k.row_s, active, round_up(active, 64), k.row_w, 6, call.has_loads ? k.row_d : nullptr, 6,
                                       (!list && !d_guess) ? nullptr : k.row_g, kFkOutNone, k.row_conv, k.row_vu, nullptr, nullptr, nullptr,
                                       k.row_calls, s, shoot_rounds, false))
    return rc;
  const trk::FkLaunch a = fk_launch_args(c, nullptr, active * Q, round_up(active * Q, 64), kFkOutNone, false, s);
  TRK_FOR_TENDONS(c, trk::launch_fk_loaded_lin<N>(a, lin));
  HIP_TRY(c, hipGetLastError());
  return TR_OK;
}

// one chunk of m problems to the end: d_init m x S, goals d_des (row stride des_ld, 0 = one row), d_guess m x 6 or null; outputs may
// be null.  rounds[0] counts the outer rounds, rounds[1] the shooting's.
int ikl_chunk_solve(tr_ctx *c, const IklCall &call, const double *d_init, int64_t m, const double *d_des, int64_t des_ld,
                    const double *d_guess, double *d_states, double *d_tips, double *d_err, int32_t *d_iters, int32_t *d_calls, double *d_vu0,
                    uint8_t *d_eq, hipStream_t s, int64_t rounds[2]) {
  tr_ctx::IklDev &k = c->ikl;
  const trk::IkParams &prm = call.prm;
  const int S = prm.S;
  const trk::IklState st = ikl_state(c);
  const trk::IklRows rows = ikl_rows(c);
  hipLaunchKernelGGL(trk::lm_init, dim3(ik_grid(m, 64)), dim3(64), 0, s, d_init, m, d_des, des_ld, prm, st.pn, st.des);
  HIP_TRY(c, hipGetLastError());
  int64_t active = m;
  int cur = 0, rc;
  for (bool init = true; active > 0; init = false) {
    const int nxt = cur ^ 1;
    const int32_t *list = init ? nullptr : k.list[cur];
    if ((rc = k.count.zero(nxt, s))) return rc;
    if ((rc = ikl_linearise(c, call, list, active, d_guess, s, rounds[1]))) return rc;
    TRK_FOR_STATE_SIZE(c, S, hipLaunchKernelGGL((trk::ikl_lm_step<SS>), dim3(ik_grid(active, 64)), dim3(64), 0, s, prm, call.sprm.delta, st, list,
                                                active, (const double *)k.lin, k.lanes, rows, (int)init, k.list[nxt], k.count.d + nxt));
    HIP_TRY(c, hipGetLastError());
    if ((rc = k.count.read(nxt, s, active))) return rc;
    cur = nxt;
    rounds[0]++;
  }
  hipLaunchKernelGGL(trk::ikl_finish, dim3(ik_grid(m, 64)), dim3(64), 0, s, prm, st, m, d_states, d_tips, d_err, d_iters, d_calls, d_vu0, d_eq);
  HIP_TRY(c, hipGetLastError());
  return TR_OK;
}

// tr_ik_loaded_batch*'s body: n device problems in chunks, each to the end (d_guess and the outputs may be null); adds its outer and
// shooting rounds to rounds[0] and rounds[1]
int ikl_run(tr_ctx *c, const IklCall &call, const double *d_init, int64_t n, const double *d_des, int64_t des_ld, const double *d_guess,
            double *d_states, double *d_tips, double *d_err, int32_t *d_iters, int32_t *d_calls, double *d_vu0, uint8_t *d_eq, hipStream_t s,
            int64_t rounds[2]) {
  const int S = call.prm.S;
  int rc;
  const int64_t chunk = ikl_chunk(c);
  if ((rc = shoot_reserve(c, std::min(n, chunk)))) return rc;
  if ((rc = ikl_reserve(c, n))) return rc;
  for (int64_t off = 0; off < n; off += chunk) {
    const int64_t m = std::min(chunk, n - off);
    if ((rc = ikl_chunk_solve(c, call, d_init + off * S, m, d_des + off * des_ld, des_ld, rows_at(d_guess, off, 6), rows_at(d_states, off, S),
                              rows_at(d_tips, off, 3), rows_at(d_err, off), rows_at(d_iters, off), rows_at(d_calls, off), rows_at(d_vu0, off, 6),
                              rows_at(d_eq, off), s, rounds))) return rc;
  }
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
  if ((rc = begin_dev_work(c, s))) return rc;
  int64_t rounds[2] = {0, 0};
  if ((rc = ikl_run(c, call, d_initial_states, n, d_des, des_ld, d_guess, d_states_out, d_tips_out, d_error_out, d_iters_out, d_fk_calls_out,
                    d_vu0_out, d_equilibrium_out, s, rounds))) return rc;
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
  if ((rc = ikl_reserve(c, n))) return rc;       // (the staging is part of it)
  tr_ctx::IklDev &k = c->ikl;
  int64_t rounds[2] = {0, 0};
  for (int64_t off = 0; off < n; off += chunk) {
    const int64_t m = std::min(chunk, n - off);
    if ((rc = upload_rows(c, k.io_s, initial_states, S, off, m, S)) || (rc = upload_rows(c, k.io_3, des, des_ld, off, m, 3))) return rc;
    if (guess && (rc = upload_rows(c, k.io_g, guess, 6, off, m, 6))) return rc;
    // (io_s / io_3 are read by lm_init, io_g by the first gather, before ikl_finish overwrites io_s / io_3 with the results)
    if ((rc = ikl_run(c, call, k.io_s, m, k.io_3, des_ld ? 3 : 0, guess ? k.io_g : nullptr, k.io_s, k.io_3, k.io_e, k.io_i, k.io_c, k.io_vu,
                      k.io_eq, nullptr, rounds))) return rc;
    if ((rc = download_rows(c, states_out, k.io_s, off, m, S)) || (rc = download_rows(c, tips_out, k.io_3, off, m, 3)) ||
        (rc = download_rows(c, error_out, k.io_e, off, m)) || (rc = download_rows(c, iters_out, k.io_i, off, m)) ||
        (rc = download_rows(c, fk_calls_out, k.io_c, off, m)) || (rc = download_rows(c, vu0_out, k.io_vu, off, m, 6)) ||
        (rc = download_rows(c, equilibrium_out, k.io_eq, off, m))) return rc;
  }
  if (rounds_out) { rounds_out[0] = rounds[0]; rounds_out[1] = rounds[1]; }
  return TR_OK;
}

}  // extern "C"
