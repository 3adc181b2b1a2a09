// launch_host.inc -- the kernel launch layer behind every state-validity check, edge sample and roadmap vertex: the argument rings
// (ArgRing), the per-lane scratch growers, this context's trk::FkLaunch / trk::VerdictArgs, the dispatch over the tendon count and the
// launches themselves (launch_fk, launch_sweep, launch_fused, launch_verdict, launch_edge_queue, launch_fk_sweep).  Host code only.
// Included in tendon_hip.hip behind tr_ctx and its allocation helpers, inside the anonymous namespace (the entry points below it
// and the other *_host.inc files call into it).

struct ProfScope {
  tr_ctx *ctx; int slot; hipStream_t s; EventPair ev{};
  bool on;
  ProfScope(tr_ctx *c, int slot_, hipStream_t s_) : ctx(c), slot(slot_), s(s_), on(c->profiling) {
    if (on) {
      (void)hipEventCreate(&ev.a); (void)hipEventCreate(&ev.b);
      (void)hipEventRecord(ev.a, s);
    }
  }
  ~ProfScope() {
    if (on) { (void)hipEventRecord(ev.b, s); ctx->events[slot].push_back(ev); }
  }
};

// The *_dev entry points that use per-context scratch (fallback list and counter, workspace columns, ordering buffers, argument
// rings, the sampler's batch) bracket their work with these two.  Calls on ONE stream are ordered by the stream; a call that
// arrives on a DIFFERENT stream than the previous one first makes its stream wait for that call's work (a device-side
// dependency, no host synchronisation), so two caller streams can never run on the shared scratch at once -- calls on one
// context execute in the order they were issued, whichever streams they name.
int begin_dev_work(tr_ctx *ctx, hipStream_t s) {
  if (ctx->last_dev_used && ctx->last_dev_stream != s) HIP_TRY(ctx, hipStreamWaitEvent(s, ctx->last_dev_ev, 0));
  return TR_OK;
}
// ... and this after enqueueing their work
int note_dev_work(tr_ctx *ctx, hipStream_t s) {
  if (!ctx->last_dev_ev) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->last_dev_ev, hipEventDisableTiming));
  HIP_TRY(ctx, hipEventRecord(ctx->last_dev_ev, s));
  ctx->last_dev_used = true;
  ctx->last_dev_stream = s;
  return TR_OK;
}

// ---- ArgRing (declared above tr_ctx) -----------------------------------------------------------
// The next slot's host image, zeroed, in *image: creates the ring at the first call, and waits until the slot's previous launch
// (kSlots launches ago, possibly on another stream) is done before the image is rewritten and its device copy replaced
template <typename T>
int ArgRing<T>::acquire(tr_ctx *ctx, int *slot, T **image) {
  if (!d_slots) {
    HIP_TRY(ctx, hipMalloc((void **)&d_slots, sizeof(T) * kSlots));
    HIP_TRY(ctx, hipHostMalloc((void **)&h_slots, sizeof(T) * kSlots, hipHostMallocDefault));
    for (auto &e : ev) HIP_TRY(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
  }
  *slot = next;
  next = (next + 1) % kSlots;
  if (used[*slot]) HIP_TRY(ctx, hipEventSynchronize(ev[*slot]));
  *image = h_slots + *slot;
  **image = T{};
  return TR_OK;
}
// the filled image to the device slot, on the launch stream (pinned source: asynchronous)
template <typename T>
int ArgRing<T>::push(tr_ctx *ctx, int slot, hipStream_t s) {
  HIP_TRY(ctx, hipMemcpyAsync(d_slots + slot, h_slots + slot, sizeof(T), hipMemcpyHostToDevice, s));
  return TR_OK;
}
// behind the launch(es) that read the slot
template <typename T>
int ArgRing<T>::commit(tr_ctx *ctx, int slot, hipStream_t s) {
  HIP_TRY(ctx, hipEventRecord(ev[slot], s));
  used[slot] = true;
  return TR_OK;
}
template <typename T>
void ArgRing<T>::release() {
  if (!d_slots) return;
  (void)hipFree(d_slots); (void)hipHostFree(h_slots);
  for (auto &e : ev) (void)hipEventDestroy(e);
  d_slots = h_slots = nullptr;
}

// A lane's fallback list (with its counter), its ordering buffers and its hand-over planes, grown to hold n entries: the caller says how
// much room it wants (whole waves; the lanes of an edge bisection ask for their share of the pool up front, since growing mid-run would
// stall all streams)
int ensure_lane_fallback(tr_ctx *ctx, int lane, int64_t n) {
  tr_ctx::EdgeLaneDev &ln = ctx->lane[lane];
  if (ln.fb_list_cap >= n) return TR_OK;
  HIP_TRY(ctx, hipDeviceSynchronize());
  int rc;
  if ((rc = dev_alloc(ctx, &ln.fb_list, (size_t)n))) return rc;
  if (!ln.fb_count && (rc = dev_alloc(ctx, &ln.fb_count, 1))) return rc;
  ln.fb_list_cap = n;
  return TR_OK;
}
int ensure_lane_order(tr_ctx *ctx, int lane, int64_t n) {
  tr_ctx::RetractOrder &ro = ctx->lane[lane].ro;
  if (ro.cap >= n) return TR_OK;
  HIP_TRY(ctx, hipDeviceSynchronize());
  int rc;
  for (int q = 0; q < 2; q++) {
    if ((rc = dev_alloc(ctx, &ro.keys[q], (size_t)n))) return rc;
    if ((rc = dev_alloc(ctx, &ro.vals[q], (size_t)n))) return rc;
  }
  if ((rc = dev_alloc(ctx, &ro.kbegin, (size_t)n / 64 + 1))) return rc;
  ro.cap = n;
  return TR_OK;
}
// the prologue kernel's hand-over planes (fk_retract_prologue -> fk_verdict_retract) for hld columns, one set per lane of the edge bisection
int ensure_lane_handoff(tr_ctx *ctx, int lane, int64_t hld) {
  tr_ctx::RetractOrder &ro = ctx->lane[lane].ro;
  if (ro.handoff_cap >= hld) return TR_OK;
  HIP_TRY(ctx, hipDeviceSynchronize());
  const int64_t want = hld + hld / 8;
  if (const int rc = dev_alloc(ctx, &ro.handoff, (size_t)want * (19 + 2 * TRK_MAX_TENDONS + 3))) return rc;     // R, v, u, p | L_i | converged | state | L
  ro.handoff_cap = want;
  return TR_OK;
}

// radix-sort scratch of a lane's ordering: lane 0 sorts in the context's (cache_merge.hip), lanes 1 .. in their own
trk::MergeScratch &order_scratch(tr_ctx *ctx, int lane) { return lane == 0 ? ctx->merge : ctx->lane[lane].ro.ms; }

// A large batch of a retraction robot (retract_sort_min configurations or more) is taken in the order of its backbone lengths
// (cache_merge.hpp: retraction_order; a lane of the edge bisection has its own buffers and sort scratch): *perm receives the order and
// *kbegin, per wave of it, the step its tip-aligned loop may start at.  Both stay null for every other batch: arrival order.
int lane_retraction_order(tr_ctx *ctx, int lane, const double *d_states, int64_t n, hipStream_t s, const int32_t **perm,
                          const int32_t **kbegin) {
  *perm = *kbegin = nullptr;
  if (!ctx->K.enable_retraction || ctx->retract_sort_min <= 0 || n < ctx->retract_sort_min) return TR_OK;
  tr_ctx::RetractOrder &ro = ctx->lane[lane].ro;
  if (const int rc = ensure_lane_order(ctx, lane, round_up(n, 64))) return rc;
  const hipError_t e = trk::retraction_order(order_scratch(ctx, lane), d_states, n, ctx->K.state_size, ctx->K.L, ro.keys, ro.vals, perm, s,
                                             ctx->K.dL, ctx->k_first, ctx->rows_one_step, ro.kbegin);
  if (e != hipSuccess) return fail(ctx, TR_ERR_HIP, std::string("retraction order: ") + hipGetErrorString(e));
  if (ctx->retract_wave_start) *kbegin = ro.kbegin;
  return TR_OK;
}

// The point workspace from column `col` on, as K1 writes it and as K2 reads it (stored points, no frames, lengths or tips)
trk::FkOut ws_fk_out(const tr_ctx *ctx, int64_t col) {
  const Workspace &w = ctx->ws;
  const bool ret = ctx->K.enable_retraction;
  return trk::FkOut{w.px + col, w.py + col, w.pz + col, nullptr, nullptr, w.Li + col, nullptr, w.conv + col, ret ? w.np + col : nullptr,
                    ret ? w.homeLi + col : nullptr};
}
trk::SweepIn ws_sweep_in(const tr_ctx *ctx, int64_t col) {
  const Workspace &w = ctx->ws;
  const bool ret = ctx->K.enable_retraction;
  return trk::SweepIn{w.px + col, w.py + col, w.pz + col, ret ? w.np + col : nullptr, w.Li + col, w.conv + col, ret ? w.homeLi + col : nullptr,
                      w.acc + col};
}

// ---- K1 launch (instantiations live in fk_inst.hip objects) ------------------------------------
// this context's launch arguments of a K1-family kernel over n states (the verdict launch sets further fields)
trk::FkLaunch fk_launch_args(const tr_ctx *ctx, const double *d_states, int64_t n, int64_t ld, const trk::FkOut &out, bool write_R,
                             hipStream_t s) {
  return trk::FkLaunch{d_states, n, ld, ctx->K, (bool)ctx->K.enable_rotation, write_R, ctx->d_tab, ctx->d_steps,
                       (int)ctx->steps.size(), ctx->d_poly, ctx->k_first, ctx->d_tgrid, ctx->d_hl, out, s};
}

// a launch that stores nothing through FkOut
const trk::FkOut kFkOutNone{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
// ... and one that stores the tips (and, where given, the convergence flags) alone
trk::FkOut fk_out_tips(double *d_tips, uint8_t *d_converged = nullptr) {
  trk::FkOut out = kFkOutNone;
  out.tips = d_tips; out.converged = d_converged;
  return out;
}

// The statement(s) given, once per tendon count with N a constant expression: the dispatch to the kernels' instantiations.
// TRK_FOR_TENDONS returns from the enclosing function when the context's count has none; TRK_FOR_TENDONS_OR does OTHERWISE instead.
#define TRK_TENDONS_CASE(COUNT, ...) case COUNT: { constexpr int N = COUNT; __VA_ARGS__; } break;
#define TRK_FOR_TENDONS_OR(ctx, OTHERWISE, ...)                                                                            \
  switch ((ctx)->K.n_tendons) {                                                                                            \
    TRK_TENDONS_CASE(1, __VA_ARGS__) TRK_TENDONS_CASE(2, __VA_ARGS__) TRK_TENDONS_CASE(3, __VA_ARGS__) TRK_TENDONS_CASE(4, __VA_ARGS__) \
    TRK_TENDONS_CASE(5, __VA_ARGS__) TRK_TENDONS_CASE(6, __VA_ARGS__) TRK_TENDONS_CASE(7, __VA_ARGS__) TRK_TENDONS_CASE(8, __VA_ARGS__) \
    default: OTHERWISE;                                                                                                    \
  }
#define TRK_FOR_TENDONS(ctx, ...) TRK_FOR_TENDONS_OR(ctx, return fail(ctx, TR_ERR_OUT_OF_RANGE, "n_tendons out of range"), __VA_ARGS__)

// The same over the state size S (1 .. TRK_IK_MAX_S), with SS the constant expression: the step kernels' instantiations.
#define TRK_STATE_SIZE_CASE(SIZE, ...) case SIZE: { constexpr int SS = SIZE; __VA_ARGS__; } break;
#define TRK_FOR_STATE_SIZE(ctx, S, ...)                                                                                    \
  switch (S) {                                                                                                             \
    TRK_STATE_SIZE_CASE(1, __VA_ARGS__) TRK_STATE_SIZE_CASE(2, __VA_ARGS__) TRK_STATE_SIZE_CASE(3, __VA_ARGS__)              \
    TRK_STATE_SIZE_CASE(4, __VA_ARGS__) TRK_STATE_SIZE_CASE(5, __VA_ARGS__) TRK_STATE_SIZE_CASE(6, __VA_ARGS__)              \
    TRK_STATE_SIZE_CASE(7, __VA_ARGS__) TRK_STATE_SIZE_CASE(8, __VA_ARGS__) TRK_STATE_SIZE_CASE(9, __VA_ARGS__)              \
    TRK_STATE_SIZE_CASE(10, __VA_ARGS__)                                                                                    \
    default: return fail(ctx, TR_ERR_OUT_OF_RANGE, "state size out of range");                                             \
  }

int launch_fk(tr_ctx *ctx, const double *d_states, int64_t n, int64_t ld, const trk::FkOut &out, hipStream_t s, int lane = 0) {
  if (n <= 0) return TR_OK;
  ProfScope ps(ctx, 0, s);
  const bool ret = ctx->K.enable_retraction;
  trk::FkLaunch a = fk_launch_args(ctx, d_states, n, ld, out, out.R != nullptr, s);
  // A large batch of a retraction robot is integrated in the order of its backbone lengths, as the verdict-only kernels do
  // (a wave runs from its LONGEST backbone's base to the tip, the shorter ones idle: in arrival order half of the lane-steps
  // are masked), and every stored output goes to its configuration's own column: same planes, bit for bit.
  if (const int rc = lane_retraction_order(ctx, lane, d_states, n, s, &a.d_perm, &a.d_wave_k_begin)) return rc;
  TRK_FOR_TENDONS(ctx, if (ret) trk::launch_fk_retract<N>(a); else trk::launch_fk_uniform<N>(a));
  HIP_TRY(ctx, hipGetLastError());
  return TR_OK;
}

// milestone spacing for the LDS self-collision proof: about two robot radii of arc per chunk,
// coarser if needed to keep the per-wave LDS image (4 * NM * 64 floats) within 48 KiB
void sweep_geometry(const tr_ctx *ctx, int &CH, int &NM, size_t &lds) {
  const int P = ctx->K.n_points;
  CH = (int)std::lround(ctx->ch_scale * ctx->K.radius / ctx->K.dL);
  if (CH < 1) CH = 1;
  while ((P - 1 + CH - 1) / CH + 1 > 48) CH++;
  NM = (P - 1 + CH - 1) / CH + 1;
  lds = (size_t)4 * NM * 64 * sizeof(float) + (128 + 64) * sizeof(uint32_t) + (size_t)6 * 128 * sizeof(double);   // milestones + deferred-walk ring, flags and the ring's end points
}

int launch_sweep(tr_ctx *ctx, const trk::SweepIn &in, int64_t n, int64_t ld, int check_voxels,
                 uint64_t *d_bits, uint8_t *d_flags, hipStream_t s) {
  if (n <= 0) return TR_OK;
  if (check_voxels && !ctx->has_grid) return fail(ctx, TR_ERR_INVALID_ARG, "no obstacle grid set (tr_set_grid)");
  ProfScope ps(ctx, 1, s);
  int CH, NM; size_t lds;
  sweep_geometry(ctx, CH, NM, lds);
  const unsigned grid = (unsigned)((n + 63) / 64);
  hipLaunchKernelGGL(trk::backbone_voxel_sweep, dim3(grid), dim3(64), lds, s, in, n, ld, ctx->K.n_points, CH, NM, ctx->K,
                     ctx->G, ctx->d_grid, ctx->d_near, check_voxels, ctx->debug, d_bits, d_flags);
  HIP_TRY(ctx, hipGetLastError());
  return TR_OK;
}

// A device copy of the sweep's arguments for one fused launch, in a slot of the context's ring (asynchronous copy on the launch
// stream).  *slot_out receives the slot: ctx->fused.commit(ctx, slot, s) after the launch.
int fused_args_slot(tr_ctx *ctx, const trk::SweepIn &in, int check_voxels, uint64_t *d_bits, uint8_t *d_flags, hipStream_t s,
                    const trk::FusedSweepArgs **d_args, size_t *lds, int *slot_out, uint32_t *sig = nullptr, int64_t sig_stride = 0) {
  trk::FusedSweepArgs *a;
  if (const int rc = ctx->fused.acquire(ctx, slot_out, &a)) return rc;
  a->in = in;
  sweep_geometry(ctx, a->CH, a->NM, *lds);
  if (sig) *lds = std::max(*lds, (size_t)trk::SIG_LDS_WORDS * 4);       // the signature tile shares the sweep's image (sweep_kernel.hpp: SigStage)
  a->P = ctx->K.n_points; a->check_voxels = check_voxels; a->debug = ctx->debug;
  a->g = ctx->G; a->grid = ctx->d_grid; a->near_grid = ctx->d_near; a->valid_bits = d_bits; a->flags = d_flags;
  a->sig = sig; a->sig_stride = sig_stride;
  *d_args = ctx->fused.dev(*slot_out);
  return ctx->fused.push(ctx, *slot_out, s);
}

// K1 + K2 in one launch (fused_kernel.hpp; shared arc-length grid only).
int launch_fused(tr_ctx *ctx, const double *d_states, int64_t n, int64_t ld, const trk::FkOut &out, const trk::SweepIn &in,
                 int check_voxels, uint64_t *d_bits, uint8_t *d_flags, hipStream_t s, uint32_t *sig = nullptr, int64_t sig_stride = 0) {
  if (n <= 0) return TR_OK;
  if (check_voxels && !ctx->has_grid) return fail(ctx, TR_ERR_INVALID_ARG, "no obstacle grid set (tr_set_grid)");
  const trk::FusedSweepArgs *d_args; size_t lds; int slot, rc;
  if ((rc = fused_args_slot(ctx, in, check_voxels, d_bits, d_flags, s, &d_args, &lds, &slot, sig, sig_stride))) return rc;
  {
    ProfScope ps(ctx, 4, s);
    const trk::FkLaunch fl = fk_launch_args(ctx, d_states, n, ld, out, false, s);
    TRK_FOR_TENDONS(ctx, trk::launch_fk_sweep_fused<N>(fl, d_args, lds));
    HIP_TRY(ctx, hipGetLastError());
  }
  return ctx->fused.commit(ctx, slot, s);
}

// sweep_body's margin box on the host: the limits -+ 1e-6 of the extent, same expressions (this file is compiled without contraction)
void margin_box(const GridK &g, double (&box)[6]) {
  box[0] = g.xmin + 1e-6 * (g.xmax - g.xmin); box[1] = g.xmax - 1e-6 * (g.xmax - g.xmin);
  box[2] = g.ymin + 1e-6 * (g.ymax - g.ymin); box[3] = g.ymax - 1e-6 * (g.ymax - g.ymin);
  box[4] = g.zmin + 1e-6 * (g.zmax - g.zmin); box[5] = g.zmax - 1e-6 * (g.zmax - g.zmin);
}

// What the arguments of every verdict-only launch share: the sweep's geometry, the obstacle grid and its margin box, the radius and
// the tendons' length limits.  The caller sets what is its own and calls finish_hot() last.
void verdict_args_common(const tr_ctx *ctx, trk::VerdictArgs &a) {
  size_t lds_k2;
  sweep_geometry(ctx, a.CH, a.NM, lds_k2);
  a.P = ctx->K.n_points; a.debug = ctx->debug;
  a.g = ctx->G; a.grid = ctx->d_grid; a.near_grid = ctx->d_near;
  margin_box(ctx->G, a.box);
  a.radius = ctx->K.radius;
  for (int j = 0; j < TRK_MAX_TENDONS; j++) { a.home_Li[j] = ctx->K.home_Li[j]; a.min_len[j] = ctx->K.min_len[j]; a.max_len[j] = ctx->K.max_len[j]; }
}

// The verdict path of tr_validate_batch* (verdict_kernel.hpp): fk_verdict over the n configurations -- no backbone point
// is stored -- then ONE launch of fk_sweep_fused_list, which integrates again, with stored points, the configurations whose
// self-collision test needs the exact pairwise sweep (their indices and count stay on the device; with an empty list its
// blocks return at once).  d_bits / d_flags / d_tips as in tr_validate_batch_dev; n <= 2^31.
int ensure_sphere_near(tr_ctx *c, hipStream_t s);
int launch_verdict(tr_ctx *ctx, const double *d_states, int64_t n, uint64_t *d_bits, double *d_tips, uint8_t *d_flags, hipStream_t s,
                   uint32_t *sig = nullptr, int64_t sig_stride = 0, bool spheres = false, int32_t *np_out = nullptr, int lane = 0) {
  if (n <= 0) return TR_OK;
  if (!ctx->has_grid) return fail(ctx, TR_ERR_INVALID_ARG, "no obstacle grid set (tr_set_grid)");
  int rc;
  if (spheres && (rc = ensure_sphere_near(ctx, s))) return rc;
  Workspace &w = ctx->ws;
  // lanes 1 .. (the further lanes of an edge bisection, running concurrently on their own streams): their own list and counter, and
  // the workspace columns [lane fb_cap, (lane + 1) fb_cap) for their fallback pass
  if (lane < 0 || lane >= tr_ctx::kMaxLanes) return fail(ctx, TR_ERR_RUNTIME, "bad lane");
  if ((rc = ensure_lane_fallback(ctx, lane, round_up(n, 64)))) return rc;
  int32_t *const fb_list = ctx->lane[lane].fb_list;
  uint32_t *const fb_count = ctx->lane[lane].fb_count;
  const int64_t cap = std::min<int64_t>(ctx->fb_cap, round_up(n, 64));
  if ((rc = ensure_workspace(ctx, lane == 0 ? cap : (lane + 1) * ctx->fb_cap))) return rc;
  const int64_t fcol = lane * ctx->fb_cap;                        // first workspace column of this lane's fallback pass
  trk::VerdictArgs *va; int vslot;
  if ((rc = ctx->vring.acquire(ctx, &vslot, &va))) return rc;
  trk::VerdictArgs &a = *va;
  verdict_args_common(ctx, a);
  a.valid_bits = d_bits; a.flags = d_flags;
  a.fb_list = fb_list; a.fb_count = fb_count;
  a.sig = sig; a.sig_stride = sig_stride; a.np_out = np_out;
  if (spheres) {                       // classification thresholds (verdict_kernel.hpp: PointSweep<true>)
    a.field = ctx->d_sph_near;
    a.r_lo = (float)ctx->K.radius - 2e-6f; a.r_hi = (float)ctx->K.radius + 2e-6f;
  }
  // waves of one backbone length: see retraction_order.  The mask is filled by atomic ORs, so it starts from zero.
  if ((rc = lane_retraction_order(ctx, lane, d_states, n, s, &a.perm, &a.wave_k_begin))) return rc;
  if (a.perm) HIP_TRY(ctx, hipMemsetAsync(d_bits, 0, (size_t)((n + 63) / 64) * sizeof(uint64_t), s));
  a.finish_hot();
  if ((rc = ctx->vring.push(ctx, vslot, s))) return rc;
  HIP_TRY(ctx, hipMemsetAsync(fb_count, 0, sizeof(uint32_t), s));
  // the fallback pass sweeps columns of the small point workspace
  const bool ret = ctx->K.enable_retraction;      // K1r's body in both launches, tip-aligned rows in the fallback workspace
  const trk::FusedSweepArgs *d_fargs; size_t lds_f; int fslot;
  if ((rc = fused_args_slot(ctx, ws_sweep_in(ctx, fcol), spheres ? 2 : 1, d_bits, d_flags, s, &d_fargs, &lds_f, &fslot))) return rc;
  trk::FkLaunch vl = fk_launch_args(ctx, d_states, n, 0, fk_out_tips(d_tips), false, s);
  if (ret) {
    const int64_t hld = round_up(n, 64);
    if ((rc = ensure_lane_handoff(ctx, lane, hld))) return rc;
    vl.d_handoff = ctx->lane[lane].ro.handoff; vl.handoff_ld = hld; vl.d_perm = a.perm;
  }
  const trk::FkLaunch fl = fk_launch_args(ctx, d_states, cap, w.ld, ws_fk_out(ctx, fcol), false, s);
  const trk::VerdictArgs *d_vargs = ctx->vring.dev(vslot);
  const size_t lds_v = trk::verdict_lds_bytes(a.NM, sig != nullptr);
  {
    ProfScope ps(ctx, 5, s);
    TRK_FOR_TENDONS(ctx, if (ret) trk::launch_fk_verdict_retract<N>(vl, d_vargs, lds_v, spheres, sig != nullptr);
                         else trk::launch_fk_verdict<N>(vl, d_vargs, lds_v, spheres, sig != nullptr));
    HIP_TRY(ctx, hipGetLastError());
  }
  {
    ProfScope ps(ctx, 4, s);
    TRK_FOR_TENDONS(ctx, if (ret) trk::launch_fk_sweep_retract_list<N>(fl, d_fargs, lds_f, fb_list, fb_count);
                         else trk::launch_fk_sweep_fused_list<N>(fl, d_fargs, lds_f, fb_list, fb_count));
    HIP_TRY(ctx, hipGetLastError());
  }
  if ((rc = ctx->vring.commit(ctx, vslot, s))) return rc;
  return ctx->fused.commit(ctx, fslot, s);
}

// the LDS image of one wave of the edge queue: the verdict-only body's with signatures and the waves' stash (edge_queue_kernel.hpp),
// or the in-wave fallback's sweep image where that is larger
size_t edge_queue_lds_bytes(int NM, size_t lds_sweep) {
  return std::max(trk::verdict_lds_bytes(NM, true) + (size_t)trk::EQ_STASH_WORDS * 4, lds_sweep);
}

// The edge queue's launch (edge_queue_kernel.hpp: fk_edge_queue): the verdict-only body's arguments as launch_verdict forms them
// (backbone checker, signature rows into `sig`), the in-wave fallback's sweep arguments over the waves' own workspace columns, and
// `waves` persistent workgroups.  qa: the queue's arguments, already on the device.  The workspace must hold 64 x waves columns.
int launch_edge_queue(tr_ctx *ctx, hipStream_t s, uint32_t *sig, int64_t sig_stride, const trk::EdgeQueueArgs *qa, unsigned waves) {
  if (!ctx->has_grid) return fail(ctx, TR_ERR_INVALID_ARG, "no obstacle grid set (tr_set_grid)");
  if (ctx->ws.ld < (int64_t)waves * 64) return fail(ctx, TR_ERR_RUNTIME, "edge queue: workspace smaller than the launch");
  int rc;
  trk::VerdictArgs *a; int vslot;
  if ((rc = ctx->vring.acquire(ctx, &vslot, &a))) return rc;
  verdict_args_common(ctx, *a);
  a->sig = sig; a->sig_stride = sig_stride;
  a->finish_hot();
  if ((rc = ctx->vring.push(ctx, vslot, s))) return rc;
  const trk::FusedSweepArgs *d_fargs; size_t lds_f; int fslot;
  if ((rc = fused_args_slot(ctx, ws_sweep_in(ctx, 0), 1, nullptr, nullptr, s, &d_fargs, &lds_f, &fslot))) return rc;
  const size_t lds_v = edge_queue_lds_bytes(a->NM, lds_f);
  const trk::FkLaunch fl = fk_launch_args(ctx, nullptr, 0, 0, kFkOutNone, false, s);
  const trk::VerdictArgs *d_vargs = ctx->vring.dev(vslot);
  {
    ProfScope ps(ctx, 5, s);
    TRK_FOR_TENDONS(ctx, trk::launch_fk_edge_queue<N>(fl, d_vargs, lds_v, qa, d_fargs, waves));
    HIP_TRY(ctx, hipGetLastError());
  }
  if ((rc = ctx->vring.commit(ctx, vslot, s))) return rc;
  return ctx->fused.commit(ctx, fslot, s);
}

// persistent workgroups of the edge queue's launch: what the device holds at once (occupancy x CUs); 0 when that is not known
int edge_queue_waves(tr_ctx *ctx) {
  if (ctx->edge_queue_waves > 0) return ctx->edge_queue_waves;
  int CH, NM; size_t lds_k2;
  sweep_geometry(ctx, CH, NM, lds_k2);
  const size_t lds_v = edge_queue_lds_bytes(NM, lds_k2);
  int per_cu = 0;
  TRK_FOR_TENDONS_OR(ctx, break, per_cu = trk::fk_edge_queue_waves_per_cu<N>(ctx->K, lds_v));
  hipDeviceProp_t prop;
  if (per_cu <= 0 || hipGetDeviceProperties(&prop, ctx->device) != hipSuccess) return 0;
  ctx->edge_queue_waves = per_cu * prop.multiProcessorCount;
  return ctx->edge_queue_waves;
}

// Distance from every cell centre to the nearest occupied cell centre, exact within the window that matters
// (r + a cell diagonal), TRK_EDT_FAR beyond: three separable min-plus passes (x on the bit grid, then y, z).
int ensure_sphere_near(tr_ctx *c, hipStream_t s) {
  if (c->sph_near_valid) return TR_OK;
  HIP_TRY(c, hipDeviceSynchronize());
  const size_t ncell = (size_t)c->G.N * c->G.N * c->G.N;
  if (c->d_sph_near) { (void)hipFree(c->d_sph_near); c->d_sph_near = nullptr; }
  if (c->d_sph_tmp) { (void)hipFree(c->d_sph_tmp); c->d_sph_tmp = nullptr; }
  HIP_TRY(c, hipMalloc((void **)&c->d_sph_near, ncell * sizeof(float)));
  HIP_TRY(c, hipMalloc((void **)&c->d_sph_tmp, ncell * sizeof(float)));
  const double reach = c->K.radius + std::sqrt(c->G.dx * c->G.dx + c->G.dy * c->G.dy + c->G.dz * c->G.dz);
  const int R[3] = {(int)std::ceil(reach / c->G.dx) + 1, (int)std::ceil(reach / c->G.dy) + 1, (int)std::ceil(reach / c->G.dz) + 1};
  const unsigned gcell = (unsigned)((ncell + 255) / 256);
  hipLaunchKernelGGL(trk::obstacle_distance_x, dim3(c->n_blocks), dim3(64), 0, s, c->d_grid, c->d_sph_near, c->G.Nb, R[0], (float)c->G.dx);
  hipLaunchKernelGGL(trk::obstacle_distance_axis, dim3(gcell), dim3(256), 0, s, c->d_sph_near, c->d_sph_tmp, c->G.N, 1, R[1], (float)c->G.dy, 0);
  hipLaunchKernelGGL(trk::obstacle_distance_axis, dim3(gcell), dim3(256), 0, s, c->d_sph_tmp, c->d_sph_near, c->G.N, 2, R[2], (float)c->G.dz, 1);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(s));
  c->sph_near_valid = true;
  return TR_OK;
}

// K1 then K2 on one stream: a single fused launch when the robot uses the shared arc-length grid.
// voxel_test: 0 = is_valid_shape only, 1 = backbone voxels (VoxelBackboneValidityChecker), 2 = sphere-swept
// robot (VoxelValidityChecker: K2 without the voxel test, then K8 on the survivors).
// sig (optional, edge samples): the fused launch also writes the samples' cell signatures; use edge_signatures(ctx, ..) to
// learn whether this context's fused path is active (the separate kernels write none).  points_unused: the caller will not
// read the points of this launch (out.px .. may then stay unwritten).
// with_points: the caller also needs the samples' stored points (voxel caches).  Retraction robots then run K1r -> K2 as
// separate launches, which write no signatures (the interval test reads the points); without points their samples go
// through fk_verdict_retract, which does.
bool edge_signatures(const tr_ctx *ctx, bool with_points) {
  return ctx->K.enable_retraction ? (ctx->fuse == 2 && !with_points) : ctx->fuse != 0;
}

int launch_fk_sweep(tr_ctx *ctx, const double *d_states, int64_t n, int64_t ld, const trk::FkOut &out, const trk::SweepIn &in,
                    int voxel_test, uint64_t *d_bits, uint8_t *d_flags, hipStream_t s, uint32_t *sig = nullptr, int64_t sig_stride = 0,
                    bool points_unused = false, int32_t *sig_np = nullptr /* retraction: the samples' point counts, next to sig */,
                    int lane = 0) {
  const int check_voxels = voxel_test == 1 ? 1 : 0;
  int rc;
  if (voxel_test == 2) {
    if (!ctx->has_grid) return fail(ctx, TR_ERR_INVALID_ARG, "no obstacle grid set (tr_set_grid)");
    if ((rc = ensure_sphere_near(ctx, s))) return rc;
  }
  if (ctx->fuse == 2 && voxel_test != 0 && points_unused && !out.R && !out.L && !out.tips) {
    // nobody reads this launch's backbone points (edge samples of the checkMotion forms: the bisection compares cell
    // signatures -- of tip-aligned rows for retraction robots, hence the point counts): the verdict-only kernel, which stores none
    return launch_verdict(ctx, d_states, n, d_bits, nullptr, d_flags, s, sig, sig_stride, voxel_test == 2, sig ? sig_np : nullptr, lane);
  }
  if (ctx->fuse != 0 && !ctx->K.enable_retraction && !out.R && !out.L) {      // the fused kernel integrates neither R output nor L
    if ((rc = launch_fused(ctx, d_states, n, ld, out, in, check_voxels, d_bits, d_flags, s, sig, sig_stride))) return rc;
  } else {
    if ((rc = launch_fk(ctx, d_states, n, ld, out, s, lane))) return rc;
    if ((rc = launch_sweep(ctx, in, n, ld, check_voxels, d_bits, d_flags, s))) return rc;
  }
  if (voxel_test == 2) {
    ProfScope ps(ctx, 3, s);
    hipLaunchKernelGGL(trk::spheres_vs_grid, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, in.px, in.py, in.pz, in.n_points, n, ld,
                       (int)ctx->K.n_points, ctx->K.radius, ctx->G, ctx->d_grid, ctx->d_sph_near, d_bits, d_flags);
    HIP_TRY(ctx, hipGetLastError());
  }
  return TR_OK;
}
