// ik_host.inc -- tip positions, the tip Jacobian and batched tip IK behind the C ABI (tr_fk_tips*, tr_tip_jacobian*, tr_ik_batch*).
// The FK of every form is one K1 launch with only the tips stored (launch_fk, the instantiation tr_fk_batch runs); the Jacobian and
// the LM iteration are ik_kernel.hpp.  The IK loop keeps every problem's state on the device: per round one expansion, one K1
// launch of m (2S + 1) lanes and one LM-step launch, and the host reads the 4-byte active count from pinned memory.
// Included at the end of tendon_hip.hip (needs tr_ctx).
namespace {

// lanes of one K1 launch of the Jacobian / IK paths, at most: problems are solved in chunks of kIkLanes / (2S + 1), each chunk to
// the end (a problem's iterates do not depend on the others, so the chunking changes no result)
constexpr int64_t kIkLanes = 1 << 19;

int64_t ik_chunk(const tr_ctx *c) { return kIkLanes / (2 * c->K.state_size + 1); }

void ik_release(tr_ctx *c) {
  tr_ctx::IkDev &k = c->ik;
  k.chunk.release(); k.once.release(); k.count.release();
  k = tr_ctx::IkDev{};
}

// the workspace for chunks of up to `n` problems (grow-only, released with the context)
int ik_reserve(tr_ctx *c, int64_t n) {
  tr_ctx::IkDev &k = c->ik;
  const int64_t S = c->K.state_size, Q = 2 * S + 1;
  const int64_t probs = round_up(std::max<int64_t>(1, std::min(n, ik_chunk(c))), 64), lanes = round_up(probs * Q, 64);
  int rc;
  if ((rc = k.count.reserve(c, k.once))) return rc;
  if (k.probs >= probs) return TR_OK;
  HIP_TRY(c, hipDeviceSynchronize());
  DevOwner &o = k.chunk;
  o.release();
  k.probs = k.lanes = 0;                       // (no buffer is usable until all of them exist again)
  if ((rc = o.alloc(c, &k.xs, (size_t)(lanes * S))) || (rc = o.alloc(c, &k.tips, (size_t)(lanes * 3)))) return rc;
  // per problem, by shape (io_*: the staging of the host-array forms)
  if ((rc = o.alloc_all(c, {&k.p, &k.pn, &k.io_s}, (size_t)(probs * S)))) return rc;
  if ((rc = o.alloc_all(c, {&k.f, &k.des, &k.io_3}, (size_t)(probs * 3)))) return rc;
  if ((rc = o.alloc(c, &k.J, (size_t)(probs * 3 * S)))) return rc;
  if ((rc = o.alloc_all(c, {&k.err2, &k.mu, &k.nu, &k.io_e}, (size_t)probs))) return rc;
  if ((rc = o.alloc_all(c, {&k.iters, &k.calls, &k.list[0], &k.list[1], &k.io_i, &k.io_c}, (size_t)probs))) return rc;
  k.probs = probs;
  k.lanes = lanes;
  return TR_OK;
}

// ---- what the host-array forms of this file and the loaded_*_host.inc files share: a host-array entry point stages chunks of its
// arrays around the body its _dev twin runs (the same body, on the staging pointers and the null stream) --------------------------

// the chunk's first row of an optional array of row width w (null stays null)
template <typename T>
T *rows_at(T *p, int64_t row, int64_t w = 1) { return p ? p + row * w : nullptr; }

// rows [off, off + m) of a host array of row stride ld, packed to width w and uploaded (ld == 0: the one row there is)
int upload_rows(tr_ctx *c, double *d_dst, const double *src, int64_t ld, int64_t off, int64_t m, int64_t w) {
  const int64_t rows = ld == 0 ? 1 : m;
  const double *from = src + off * ld;
  std::vector<double> packed;
  if (ld != w && rows > 1) {
    packed.resize((size_t)(rows * w));
    for (int64_t i = 0; i < rows; i++) for (int64_t q = 0; q < w; q++) packed[(size_t)(i * w + q)] = from[i * ld + q];
    from = packed.data();
  }
  HIP_TRY(c, hipMemcpy(d_dst, from, (size_t)(rows * w) * sizeof(double), hipMemcpyHostToDevice));
  return TR_OK;
}

// if the caller wants the array: m staged rows of width w down to its rows [off, off + m)
template <typename T>
int download_rows(tr_ctx *c, T *dst, const T *d_src, int64_t off, int64_t m, int64_t w = 1) {
  if (dst) HIP_TRY(c, hipMemcpy(dst + off * w, d_src, (size_t)(m * w) * sizeof(T), hipMemcpyDeviceToHost));
  return TR_OK;
}

trk::IkState ik_state(tr_ctx *c) {
  tr_ctx::IkDev &k = c->ik;
  return trk::IkState{k.p, k.pn, k.f, k.J, k.des, k.err2, k.mu, k.nu, k.iters, k.calls};
}

unsigned ik_grid(int64_t n, int block) { return (unsigned)((n + block - 1) / block); }

// K1 over `lanes` expanded states: tips only
int ik_fk(tr_ctx *c, int64_t lanes, hipStream_t s) {
  return launch_fk(c, c->ik.xs, lanes, round_up(lanes, 64), fk_out_tips(c->ik.tips), s);
}

// f and J of m <= ik_chunk states (device rows)
int jacobian_chunk(tr_ctx *c, const double *d_states, int64_t m, double delta, double *d_tips, double *d_J, hipStream_t s) {
  const int S = c->K.state_size;
  const int64_t lanes = m * (2 * S + 1);
  hipLaunchKernelGGL(trk::ik_expand, dim3(ik_grid(lanes, 256)), dim3(256), 0, s, d_states, (const int32_t *)nullptr, m, S, delta, c->ik.xs);
  HIP_TRY(c, hipGetLastError());
  int rc;
  if ((rc = ik_fk(c, lanes, s))) return rc;
  hipLaunchKernelGGL(trk::ik_jacobian, dim3(ik_grid(m, 64)), dim3(64), 0, s, d_states, (const double *)c->ik.tips, m, S, delta,
                     (int)c->K.enable_retraction, c->K.L, d_tips, d_J);
  HIP_TRY(c, hipGetLastError());
  return TR_OK;
}

int ik_params(tr_ctx *c, const tr_ik_params *ip, const double *lo, const double *hi, trk::IkParams &prm) {
  const int N = c->K.n_tendons, S = c->K.state_size;
  if (S > TRK_IK_MAX_S) return fail(c, TR_ERR_OUT_OF_RANGE, "state size out of range");
  const tr_ik_params def{100, 0.1, 1e-9, 1e-4, 1e-4, 1e-6};                           // tip_control.h:88-100
  const tr_ik_params &q = ip ? *ip : def;
  if (q.max_iters < 0) return fail(c, TR_ERR_INVALID_ARG, "max_iters must be >= 0");
  prm = trk::IkParams{};
  prm.S = S; prm.max_iters = q.max_iters;
  prm.rot_index = c->K.enable_rotation ? N : -1;
  prm.retraction = c->K.enable_retraction;
  prm.L = c->K.L;
  prm.delta = q.finite_difference_delta;
  prm.mu_init = q.mu_init;
  prm.eps1 = q.stop_threshold_JT_err_inf;
  prm.eps2_sq = q.stop_threshold_Dp * q.stop_threshold_Dp;
  prm.eps3_sq = q.stop_threshold_err * q.stop_threshold_err;
  for (int d = 0; d < S; d++) {                      // Bounds::from_robot (tip_control.cpp:160-185)
    double a = 0.0, b = 0.0;
    if (d < N) b = c->max_tension[(size_t)d];
    else if (c->K.enable_rotation && d == N) { a = -std::numeric_limits<double>::max(); b = std::numeric_limits<double>::max(); }
    else b = c->K.L;
    prm.lo[d] = lo ? lo[d] : a;
    prm.hi[d] = hi ? hi[d] : b;
  }
  return TR_OK;
}

// one chunk of m problems to the end: d_init m x S, goals d_des (row stride des_ld, 0 = one row); outputs may be null
int ik_chunk_solve(tr_ctx *c, const trk::IkParams &prm, const double *d_init, int64_t m, const double *d_des, int64_t des_ld,
                   double *d_states, double *d_tips, double *d_err, int32_t *d_iters, int32_t *d_calls, hipStream_t s, int64_t &rounds) {
  tr_ctx::IkDev &k = c->ik;
  const int S = prm.S, Q = 2 * S + 1;
  const trk::IkState st = ik_state(c);
  hipLaunchKernelGGL(trk::lm_init, dim3(ik_grid(m, 64)), dim3(64), 0, s, d_init, m, d_des, des_ld, prm, st.pn, st.des);
  HIP_TRY(c, hipGetLastError());
  int64_t active = m;
  int cur = 0, rc;
  for (bool init = true; active > 0; init = false) {
    const int nxt = cur ^ 1;
    const int32_t *list = init ? nullptr : k.list[cur];
    if ((rc = k.count.zero(nxt, s))) return rc;
    hipLaunchKernelGGL(trk::ik_expand, dim3(ik_grid(active * Q, 256)), dim3(256), 0, s, (const double *)k.pn, list, active, S, prm.delta, k.xs);
    HIP_TRY(c, hipGetLastError());
    if ((rc = ik_fk(c, active * Q, s))) return rc;
    TRK_FOR_STATE_SIZE(c, S, hipLaunchKernelGGL((trk::ik_lm_step<SS>), dim3(ik_grid(active, 64)), dim3(64), 0, s, prm, st, list, active,
                                                (const double *)k.tips, (int)init, k.list[nxt], k.count.d + nxt));
    HIP_TRY(c, hipGetLastError());
    if ((rc = k.count.read(nxt, s, active))) return rc;
    cur = nxt;
    rounds++;
  }
  hipLaunchKernelGGL(trk::ik_finish, dim3(ik_grid(m, 64)), dim3(64), 0, s, prm, st, m, d_states, d_tips, d_err, d_iters, d_calls);
  HIP_TRY(c, hipGetLastError());
  return TR_OK;
}

// tr_tip_jacobian*'s body: n device rows in chunks (d_tips may be null)
int jacobian_run(tr_ctx *c, const double *d_states, int64_t n, double delta, double *d_tips, double *d_J, hipStream_t s) {
  const int S = c->K.state_size;
  int rc;
  if ((rc = ik_reserve(c, n))) return rc;
  const int64_t chunk = ik_chunk(c);
  for (int64_t off = 0; off < n; off += chunk) {
    const int64_t m = std::min(chunk, n - off);
    if ((rc = jacobian_chunk(c, d_states + off * S, m, delta, rows_at(d_tips, off, 3), d_J + off * 3 * S, s))) return rc;
  }
  return TR_OK;
}

// tr_ik_batch*'s body: n device problems in chunks, each to the end (outputs may be null); adds its rounds to `rounds`
int ik_run(tr_ctx *c, const trk::IkParams &prm, const double *d_init, int64_t n, const double *d_des, int64_t des_ld, double *d_states,
           double *d_tips, double *d_err, int32_t *d_iters, int32_t *d_calls, hipStream_t s, int64_t &rounds) {
  const int S = prm.S;
  int rc;
  if ((rc = ik_reserve(c, n))) return rc;
  const int64_t chunk = ik_chunk(c);
  for (int64_t off = 0; off < n; off += chunk) {
    const int64_t m = std::min(chunk, n - off);
    if ((rc = ik_chunk_solve(c, prm, d_init + off * S, m, d_des + off * des_ld, des_ld, rows_at(d_states, off, S), rows_at(d_tips, off, 3),
                             rows_at(d_err, off), rows_at(d_iters, off), rows_at(d_calls, off), s, rounds))) return rc;
  }
  return TR_OK;
}

}  // namespace

extern "C" {

int tr_fk_tips_dev(tr_ctx *c, const double *d_states, int64_t n, double *d_tips, uint8_t *d_converged, void *stream) {
  if (!c) return TR_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lock_(c->mu);
  if (n < 0) return fail(c, TR_ERR_INVALID_ARG, "bad argument");
  if (n == 0) return TR_OK;
  if (!d_states || !d_tips) return fail(c, TR_ERR_INVALID_ARG, "null device pointer");
  HIP_TRY(c, hipSetDevice(c->device));
  const hipStream_t s = (hipStream_t)stream;
  int rc;
  if ((rc = begin_dev_work(c, s))) return rc;
  if ((rc = launch_fk(c, d_states, n, round_up(n, 64), fk_out_tips(d_tips, d_converged), s))) return rc;
  return note_dev_work(c, s);
}

int tr_fk_tips(tr_ctx *c, const double *states, int64_t n, double *tips, uint8_t *converged) {
  if (!c) return TR_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lock_(c->mu);
  if (n < 0 || (n > 0 && (!states || !tips))) return fail(c, TR_ERR_INVALID_ARG, "bad argument");
  if (n == 0) return TR_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipDeviceSynchronize());          // the staging is shared with *_dev calls that may still run on other streams
  const int S = c->K.state_size;
  const int64_t chunk_max = std::min<int64_t>(c->max_chunk, 1 << 16);      // tr_fk_batch's chunk
  int rc;
  if ((rc = ensure_staging(c, std::min(n, chunk_max)))) return rc;
  Workspace &w = c->ws;
  for (int64_t off = 0; off < n; off += chunk_max) {
    const int64_t m = std::min(chunk_max, n - off);
    HIP_TRY(c, hipMemcpy(w.states, states + off * S, (size_t)m * S * sizeof(double), hipMemcpyHostToDevice));
    if ((rc = launch_fk(c, w.states, m, round_up(m, 64), fk_out_tips(w.tips, converged ? w.flags : nullptr), nullptr))) return rc;
    HIP_TRY(c, hipMemcpy(tips + off * 3, w.tips, (size_t)m * 3 * sizeof(double), hipMemcpyDeviceToHost));
    if (converged) HIP_TRY(c, hipMemcpy(converged + off, w.flags, (size_t)m, hipMemcpyDeviceToHost));
  }
  return TR_OK;
}

int tr_tip_jacobian_dev(tr_ctx *c, const double *d_states, int64_t n, double delta, double *d_tips, double *d_J, void *stream) {
  if (!c) return TR_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lock_(c->mu);
  if (n < 0) return fail(c, TR_ERR_INVALID_ARG, "bad argument");
  if (n == 0) return TR_OK;
  if (!d_states || !d_J) return fail(c, TR_ERR_INVALID_ARG, "null device pointer");
  HIP_TRY(c, hipSetDevice(c->device));
  const hipStream_t s = (hipStream_t)stream;
  int rc;
  if ((rc = begin_dev_work(c, s))) return rc;
  if ((rc = jacobian_run(c, d_states, n, delta, d_tips, d_J, s))) return rc;
  return note_dev_work(c, s);
}

int tr_tip_jacobian(tr_ctx *c, const double *states, int64_t n, double delta, double *tips, double *J) {
  if (!c) return TR_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lock_(c->mu);
  if (n < 0 || (n > 0 && (!states || !J))) return fail(c, TR_ERR_INVALID_ARG, "bad argument");
  if (n == 0) return TR_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipDeviceSynchronize());
  const int S = c->K.state_size;
  int rc;
  if ((rc = ik_reserve(c, n))) return rc;
  tr_ctx::IkDev &k = c->ik;
  const int64_t chunk = ik_chunk(c);
  for (int64_t off = 0; off < n; off += chunk) {
    const int64_t m = std::min(chunk, n - off);
    if ((rc = upload_rows(c, k.io_s, states, S, off, m, S))) return rc;
    if ((rc = jacobian_run(c, k.io_s, m, delta, tips ? k.io_3 : nullptr, k.J, nullptr))) return rc;
    if ((rc = download_rows(c, J, k.J, off, m, 3 * S)) || (rc = download_rows(c, tips, k.io_3, off, m, 3))) return rc;
  }
  return TR_OK;
}

int tr_ik_batch_dev(tr_ctx *c, const tr_ik_params *params, const double *d_initial_states, int64_t n, const double *d_des, int64_t des_ld,
                    const double *lo, const double *hi, double *d_states_out, double *d_tips_out, double *d_error_out,
                    int32_t *d_iters_out, int32_t *d_fk_calls_out, int64_t *rounds_out, void *stream) {
  if (!c) return TR_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lock_(c->mu);
  if (rounds_out) *rounds_out = 0;
  if (n < 0 || (des_ld != 0 && des_ld < 3)) return fail(c, TR_ERR_INVALID_ARG, "bad argument (des_ld: 0 or >= 3)");
  if (n == 0) return TR_OK;
  if (!d_initial_states || !d_des) return fail(c, TR_ERR_INVALID_ARG, "null device pointer");
  HIP_TRY(c, hipSetDevice(c->device));
  const hipStream_t s = (hipStream_t)stream;
  trk::IkParams prm;
  int rc;
  if ((rc = ik_params(c, params, lo, hi, prm))) return rc;
  if ((rc = begin_dev_work(c, s))) return rc;
  int64_t rounds = 0;
  if ((rc = ik_run(c, prm, d_initial_states, n, d_des, des_ld, d_states_out, d_tips_out, d_error_out, d_iters_out, d_fk_calls_out, s,
                   rounds))) return rc;
  if (rounds_out) *rounds_out = rounds;
  return note_dev_work(c, s);
}

int tr_ik_batch(tr_ctx *c, const tr_ik_params *params, const double *initial_states, int64_t n, const double *des, int64_t des_ld,
                const double *lo, const double *hi, double *states_out, double *tips_out, double *error_out, int32_t *iters_out,
                int32_t *fk_calls_out, int64_t *rounds_out) {
  if (!c) return TR_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lock_(c->mu);
  if (rounds_out) *rounds_out = 0;
  if (n < 0 || (des_ld != 0 && des_ld < 3)) return fail(c, TR_ERR_INVALID_ARG, "bad argument (des_ld: 0 or >= 3)");
  if (n == 0) return TR_OK;
  if (!initial_states || !des) return fail(c, TR_ERR_INVALID_ARG, "bad argument");
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipDeviceSynchronize());
  const int S = c->K.state_size;
  trk::IkParams prm;
  int rc;
  if ((rc = ik_params(c, params, lo, hi, prm))) return rc;
  if ((rc = ik_reserve(c, n))) return rc;
  tr_ctx::IkDev &k = c->ik;
  const int64_t chunk = ik_chunk(c);
  int64_t rounds = 0;
  for (int64_t off = 0; off < n; off += chunk) {
    const int64_t m = std::min(chunk, n - off);
    if ((rc = upload_rows(c, k.io_s, initial_states, S, off, m, S)) || (rc = upload_rows(c, k.io_3, des, des_ld, off, m, 3))) return rc;
    // (io_s / io_3 are read by lm_init before ik_finish overwrites them with the results)
    if ((rc = ik_run(c, prm, k.io_s, m, k.io_3, des_ld ? 3 : 0, k.io_s, k.io_3, k.io_e, k.io_i, k.io_c, nullptr, rounds))) return rc;
    if ((rc = download_rows(c, states_out, k.io_s, off, m, S)) || (rc = download_rows(c, tips_out, k.io_3, off, m, 3)) ||
        (rc = download_rows(c, error_out, k.io_e, off, m)) || (rc = download_rows(c, iters_out, k.io_i, off, m)) ||
        (rc = download_rows(c, fk_calls_out, k.io_c, off, m))) return rc;
  }
  if (rounds_out) *rounds_out = rounds;
  return TR_OK;
}

}  // extern "C"
