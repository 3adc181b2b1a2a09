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
  DevOwner &o = k.sens;
  o.release();
  k.sens_probs = 0;
  if ((rc = o.alloc(c, &k.sens_c, (size_t)(k.probs * 18)))) return rc;
  if ((rc = o.alloc(c, &k.sens_b, (size_t)(k.probs * (69 + 9 * S))))) return rc;
  if ((rc = o.alloc(c, &k.sens_n, (size_t)k.probs))) return rc;
  k.sens_probs = k.probs;
  return TR_OK;
}

// what both forms refuse, and the call's parameters: the loaded IK's call (ikl_begin's head) without a goal, bounds or an outer
// iteration, at the caller's difference step and tr_fk_loaded_batch's shooting defaults
int sens_params(tr_ctx *c, const tr_shoot_params *shoot, const tr_edge_loads *loads, int64_t n, double delta, IklCall &call) {
  int rc;
  if ((rc = ikl_begin_loads(c, loads, n, call, "loaded tip Jacobian and compliance (tr_tip_jacobian_loaded*)"))) return rc;
  if (!(delta > 0.0)) return fail(c, TR_ERR_INVALID_ARG, "bad argument (delta must be > 0)");
  if ((rc = ik_params(c, nullptr, nullptr, nullptr, call.prm))) return rc;
  call.prm.delta = delta;
  return shoot_params(c, shoot, call.sprm);
}

// one chunk of m problems: d_states m x S, d_guess m x 6 or null; `out`: the chunk's first row of every wanted output
int sens_chunk_solve(tr_ctx *c, const IklCall &call, const double *d_states, int64_t m, const double *d_guess, const trk::SensOut &out,
                     hipStream_t s, int64_t &rounds) {
  tr_ctx::IklDev &k = c->ikl;
  const trk::IkParams &prm = call.prm;
  const int S = prm.S;
  const trk::IklRows rows = ikl_rows(c);
  // the states are the gather's trial points as they stand (no bounds here)
  HIP_TRY(c, hipMemcpyAsync(k.pn, d_states, (size_t)(m * S) * sizeof(double), hipMemcpyDeviceToDevice, s));
  if (const int rc = ikl_linearise(c, call, nullptr, m, d_guess, s, rounds)) return rc;
  TRK_FOR_STATE_SIZE(c, S, hipLaunchKernelGGL((trk::loaded_tip_sens<SS>), dim3(ik_grid(m, 64)), dim3(64), 0, s, prm.delta, call.sprm.delta,
                                              (int)prm.rot_index, (int)call.loads.world, m, (const double *)k.lin, k.lanes, rows, out));
  HIP_TRY(c, hipGetLastError());
  return TR_OK;
}

// tr_tip_jacobian_loaded*'s body: n device rows in chunks; `out`: row 0 of every wanted output.  Adds its shooting rounds to `rounds`.
int sens_run(tr_ctx *c, const IklCall &call, const double *d_states, int64_t n, const double *d_guess, const trk::SensOut &out,
             hipStream_t s, int64_t &rounds) {
  const int64_t S = call.prm.S, NB = 69 + 9 * S;
  int rc;
  const int64_t chunk = ikl_chunk(c);
  if ((rc = shoot_reserve(c, std::min(n, chunk)))) return rc;
  if ((rc = ikl_reserve(c, n))) return rc;
  for (int64_t off = 0; off < n; off += chunk) {
    const int64_t m = std::min(chunk, n - off);
    const trk::SensOut o{rows_at(out.tips, off, 3), rows_at(out.vu0, off, 6), rows_at(out.J, off, 3 * S), rows_at(out.W, off, 6 * S),
                         rows_at(out.C, off, 18), rows_at(out.blocks, off, NB), rows_at(out.eq, off), rows_at(out.nint, off)};
    if ((rc = sens_chunk_solve(c, call, d_states + off * S, m, rows_at(d_guess, off, 6), o, s, rounds))) return rc;
  }
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
  IklCall call;
  int rc;
  if ((rc = sens_params(c, shoot, loads, n, delta, call))) return rc;
  if (n == 0) return TR_OK;
  if (!d_states) return fail(c, TR_ERR_INVALID_ARG, "null device pointer");
  HIP_TRY(c, hipSetDevice(c->device));
  const hipStream_t s = (hipStream_t)stream;
  if ((rc = begin_dev_work(c, s))) return rc;
  const trk::SensOut out{d_tips, d_vu0, d_J, d_W, d_compliance, d_blocks, d_equilibrium, d_n_integrations};
  int64_t rounds = 0;
  if ((rc = sens_run(c, call, d_states, n, d_guess, out, s, rounds))) return rc;
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
  IklCall call;
  int rc;
  if ((rc = sens_params(c, shoot, loads, n, delta, call))) return rc;
  if (n == 0) return TR_OK;
  if (!states) return fail(c, TR_ERR_INVALID_ARG, "bad argument");
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipDeviceSynchronize());          // the workspace is shared with *_dev calls that may still run on other streams
  const int64_t S = c->K.state_size, NB = 69 + 9 * S;
  const int64_t chunk = ikl_chunk(c);
  if ((rc = ikl_reserve(c, n))) return rc;       // (the staging is part of it, and sizes the rest)
  if ((rc = sens_reserve_io(c))) return rc;
  tr_ctx::IklDev &k = c->ikl;
  int64_t rounds = 0;
  for (int64_t off = 0; off < n; off += chunk) {
    const int64_t m = std::min(chunk, n - off);
    if ((rc = upload_rows(c, k.io_s, states, S, off, m, S))) return rc;
    if (guess && (rc = upload_rows(c, k.io_g, guess, 6, off, m, 6))) return rc;
    // the problem-indexed rows of the loaded IK's state that this call does not use stage J, W and the strains
    const trk::SensOut out{tips ? k.io_3 : nullptr, vu0 ? k.io_vu : nullptr, J ? k.J : nullptr, W ? k.W : nullptr,
                           compliance ? k.sens_c : nullptr, blocks ? k.sens_b : nullptr, equilibrium ? k.io_eq : nullptr,
                           n_integrations ? k.sens_n : nullptr};
    if ((rc = sens_run(c, call, k.io_s, m, guess ? k.io_g : nullptr, out, nullptr, rounds))) return rc;
    if ((rc = download_rows(c, tips, k.io_3, off, m, 3)) || (rc = download_rows(c, vu0, k.io_vu, off, m, 6)) ||
        (rc = download_rows(c, J, k.J, off, m, 3 * S)) || (rc = download_rows(c, W, k.W, off, m, 6 * S)) ||
        (rc = download_rows(c, compliance, k.sens_c, off, m, 18)) || (rc = download_rows(c, blocks, k.sens_b, off, m, NB)) ||
        (rc = download_rows(c, equilibrium, k.io_eq, off, m)) || (rc = download_rows(c, n_integrations, k.sens_n, off, m))) return rc;
  }
  if (rounds_out) *rounds_out = rounds;
  return TR_OK;
}

}  // extern "C"
