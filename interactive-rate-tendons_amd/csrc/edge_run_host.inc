// edge_run_host.inc -- the machinery of tr_validate_edges* / tr_voxelize_edges* (edge_pairs_host.inc, edge_indexed_host.inc): batched AbstractVoxelMotionValidator::checkMotion
// (motion-planning/AbstractVoxelMotionValidator.h:143-151) as a level-synchronous bisection.
//
// The reference bisects each edge depth-first (VoxelEnvironment.cpp:343-398): FK at the midpoint of
// an interval, push the halves whose end shapes differ by more than a voxel somewhere
// (should_subdivide), stop at width <= 1/validSegmentCount, skip intervals beyond the first invalid
// sample; the edge is valid iff no sample is shape-invalid and the union of the sampled backbones
// misses the obstacles.  Because an interval is only ever skipped AFTER an invalid sample has been
// found (which already decides the verdict), the verdict equals
//     AND over the un-pruned bisection tree of [ is_valid_shape(sample) && !collides(sample) ],
// and a union of voxel sets hits an obstacle iff one of its members does.  So every level is one
// K1 + K2 pass over all open midpoints of all edges, plus K3's pair test to decide the next level.
// Edges leave the frontier as soon as one sample is invalid.
//
// State-space arithmetic (OMPL 1.5.0, third party, restated from its published behaviour as wired
// by motion-planning/Problem.cpp:101-163): CompoundStateSpace{RealVector tension, SO2 rotation}
// validSegmentCount = max over subspaces of ceil(distance / (maxExtent * fraction)); interpolate is
// linear per tension and shortest-arc on SO2.
namespace {

// Device-resident state of one chunk of edges; lives in the context so repeated calls do not reallocate.
int ensure_edge_dev(tr_ctx *c, int64_t cap) {
  EdgeDev &d = c->edge;
  if (d.cap >= cap) return TR_OK;
  HIP_TRY(c, hipDeviceSynchronize());
  const size_t S = (size_t)c->K.state_size, ecap = (size_t)cap / 2 + 1;
  int rc;
  if ((rc = dev_alloc(c, &d.lvl_states, (size_t)cap * S))) return rc;
  if ((rc = dev_alloc(c, &d.bits, (size_t)cap / 64 + 1))) return rc;
  if ((rc = dev_alloc(c, &d.sample_edge, (size_t)cap))) return rc;
  if ((rc = dev_alloc(c, &d.sample_t, (size_t)cap))) return rc;
  if ((rc = dev_alloc(c, &d.open, (size_t)cap))) return rc;
  if ((rc = dev_alloc(c, &d.frontier, (size_t)2 * cap))) return rc;
  if ((rc = dev_alloc(c, &d.A, ecap * S))) return rc;
  if ((rc = dev_alloc(c, &d.B, ecap * S))) return rc;
  if ((rc = dev_alloc(c, &d.rel, ecap))) return rc;
  if ((rc = dev_alloc(c, &d.edge_ok, ecap))) return rc;
  if ((rc = dev_alloc(c, &d.nfk, ecap))) return rc;
  if ((rc = dev_alloc(c, &d.first_inv, ecap))) return rc;
  if ((rc = dev_alloc(c, &d.last_t, ecap))) return rc;
  if ((rc = dev_alloc(c, &c->lane[0].counters, (size_t)trk::EC_COUNT))) return rc;
  if ((rc = dev_alloc(c, &d.nd, ecap))) return rc;
  if ((rc = dev_alloc(c, &d.cnt, ecap + 1))) return rc;
  if (edge_signatures(c, false)) {
    d.sig_stride = round_up(c->K.n_points, 16);          // rows start on 64-byte boundaries (SigStage writes 32-byte pieces of them)
    if ((rc = dev_alloc(c, &d.sig, (size_t)cap * d.sig_stride))) return rc;
    if (c->K.enable_retraction && (rc = dev_alloc(c, &d.sig_np, (size_t)cap))) return rc;
  }
  if (c->K.enable_retraction) {
    if ((rc = dev_alloc(c, &d.open2, (size_t)cap))) return rc;
    if ((rc = dev_alloc(c, &d.lvl_states2, (size_t)cap * S))) return rc;
  } else {
    // the edge queue's per-edge level records (edge_queue_kernel.hpp), its control words and arguments
    if ((rc = dev_alloc(c, &d.q_remaining, ecap))) return rc;
    if ((rc = dev_alloc(c, &d.q_lvl_base, ecap))) return rc;
    if ((rc = dev_alloc(c, &d.q_lvl_cnt, ecap))) return rc;
    if (!d.q_ctl) {
      if ((rc = dev_alloc(c, &d.q_ctl, (size_t)trk::EQ_WORDS))) return rc;
      if ((rc = dev_alloc(c, &d.q_args, (size_t)1))) return rc;
      HIP_TRY(c, hipHostMalloc((void **)&d.q_hctl, trk::EQ_WORDS * sizeof(uint32_t), hipHostMallocDefault));
      HIP_TRY(c, hipHostMalloc((void **)&d.q_hargs, sizeof(trk::EdgeQueueArgs), hipHostMallocDefault));
    }
  }
  d.cap = cap;
  return TR_OK;
}

// streams, pinned counter images and device counters of the lanes of the edge bisection (lane 0's counters: ensure_edge_dev)
int ensure_edge_lanes(tr_ctx *c) {
  if (c->lane[0].hc) return TR_OK;
  int rc;
  for (int q = tr_ctx::kMaxLanes - 1; q >= 0; q--) {               // (lane[0].hc, the "done" mark, last)
    tr_ctx::EdgeLaneDev &ln = c->lane[q];
    if (!ln.stream) HIP_TRY(c, hipStreamCreateWithFlags(&ln.stream, hipStreamNonBlocking));
    if (q > 0 && (rc = dev_alloc(c, &ln.counters, (size_t)trk::EC_COUNT))) return rc;
    if (!ln.hc) HIP_TRY(c, hipHostMalloc((void **)&ln.hc, trk::EC_COUNT * sizeof(uint32_t), hipHostMallocDefault));
  }
  return TR_OK;
}

int ensure_indexed_inputs(tr_ctx *c, int64_t n_states, int64_t n_edges) {
  EdgeDev &d = c->edge;
  int rc;
  if (d.ix_states_cap < n_states) {
    HIP_TRY(c, hipDeviceSynchronize());
    const int64_t want = n_states + n_states / 4 + 64;
    if ((rc = dev_alloc(c, &d.ix_states, (size_t)want * c->K.state_size))) return rc;
    d.ix_states_cap = want;
  }
  if (d.ix_idx_cap < n_edges) {
    HIP_TRY(c, hipDeviceSynchronize());
    const int64_t want = n_edges + n_edges / 4 + 64;
    if ((rc = dev_alloc(c, &d.ix_idx, (size_t)want * 2))) return rc;
    d.ix_idx_cap = want;
  }
  return TR_OK;
}

trk::EdgeSpaceK edge_space(const tr_ctx *c, const tr_space_params *sp) {
  const int N = c->K.n_tendons;
  double ext2 = 0;
  for (int i = 0; i < N; i++) ext2 += (c->max_tension[i] - 0.0) * (c->max_tension[i] - 0.0);
  const double ext = std::sqrt(ext2);
  trk::EdgeSpaceK sk{N, c->K.enable_rotation, c->K.enable_retraction, c->K.state_size, 1.0, 1.0, 1.0};
  sk.lvs_tension = ext * (sp->min_tension_change / ext);                       // Problem.cpp:118-120, StateSpace::setup
  sk.lvs_rot = M_PI * (sp->min_rotation_change / (2 * M_PI));                  // Problem.cpp:131-132, SO2 extent = pi
  sk.lvs_retr = c->K.L * std::min(0.01, sp->min_retraction_change / c->K.L);   // Problem.cpp:144-145, extent of [0, L]
  return sk;
}

// the per-edge arrays from edge `eoff` on (a lane's part of them) and the per-sample arrays of the whole pool
trk::EdgeState edge_state(tr_ctx *c, int64_t eoff, uint32_t *counters) {
  EdgeDev &d = c->edge;
  const int S = c->K.state_size;
  return trk::EdgeState{d.A + eoff * S, d.B + eoff * S, d.rel + eoff, d.edge_ok + eoff, d.nfk + eoff, d.first_inv + eoff, d.last_t + eoff,
                        d.sample_edge, d.sample_t, d.bits, counters};
}

// TENDON_HIP_EDGE_TIMING=1: where the time of an edge call goes (stderr; tuning only)
bool edge_timing() { static const bool on = std::getenv("TENDON_HIP_EDGE_TIMING") != nullptr; return on; }
struct EdgeLaps {                       // ... on the host, in tr_validate_edges_indexed*: one line per lap
  double prev = 0.0;
  void operator()(const char *what) {
    if (!edge_timing()) return;
    timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts);
    const double t = 1e3 * (double)ts.tv_sec + 1e-6 * (double)ts.tv_nsec;
    if (prev > 0.0) std::fprintf(stderr, "[edges_indexed] %-28s %7.3f ms\n", what, t - prev);
    prev = t;
  }
};

// What an edge call may add to the verdicts.  With EdgeVoxOut the samples are only tested for shape validity
// (AbstractVoxelMotionValidator::voxelize, VoxelBackboneMotionValidator.cpp:76-81), the union voxel set of every fully valid edge is
// appended to the context's block-list store with per-edge counts in `count`
// (the lists themselves stay on the device: tr_ctx::vstore)  collide: samples are also tested against the obstacles, as
// checkMotion does -- the edge's verdict is then checkMotion's and only collision-free edges get a voxel set
struct EdgeVoxOut { std::vector<int32_t> count; bool collide = false; };
// indexed edges: end states are vertices already evaluated into pool slots [0, pool_base)
struct EdgeIndexed { const double *d_states; const int32_t *d_idx; int64_t pool_base; };

// Where one run of the bisection lives: its stream, its share of the sample pool and of the per-edge / per-level arrays.  The
// default is the whole pool on the null stream; tr_validate_edges_indexed may run the parts of a chunk as two to four lanes on as many
// streams, alternating between them on one host thread, so that the partial last round of waves of one lane's FK launch is
// filled by the other lane's (profiles/probe_two_streams.py).
struct EdgeLane {
  hipStream_t s = nullptr;
  int lane = 0;                   // selects the verdict path's fallback list and workspace columns (launch_verdict)
  int64_t slot_lo = 0, slot_hi = 0;   // pool slots of this run's own samples
  int64_t eoff = 0;               // first edge's position in the per-edge device arrays
  int64_t level_off = 0;          // offset (in samples) into lvl_states / open, twice that into frontier
  uint32_t *counters = nullptr;   // device [EC_COUNT]
  uint32_t *hc = nullptr;         // pinned host image of the counters
};

// One chunk of edges [e0, e1) as a resumable run: start() enqueues level 0 up to the first edge_open and the copy of its
// counters; after the lane's stream has drained, resume() reads them and enqueues the next level (returns EDGE_MORE while the
// bisection goes on, TR_OK when done and the results are in place, EDGE_OVERFLOW when the sample pool overflowed, > 0 = error status).
// With `vox` the samples are only tested for shape validity (AbstractVoxelMotionValidator::voxelize,
// VoxelBackboneMotionValidator.cpp:76-81) and the union voxel set of every fully valid edge is
// appended to the context's block-list store (device) with per-edge counts in vox->count.
// What EdgeRun::start / resume return besides a tr_status (>= 0): negative, so that no status can be read as one of them.
constexpr int EDGE_MORE = -2;         // the bisection continues: synchronise the lane's stream, then resume()
constexpr int EDGE_OVERFLOW = -1;     // the lane's share of the sample pool is too small for the chunk: the caller retries with fewer edges

struct EdgeRun {
  tr_ctx *c; const tr_space_params *sp; const double *A, *B; int64_t e0, e1;
  std::vector<uint8_t> *edge_ok; std::vector<int32_t> *edge_nfk; int64_t *n_domain; EdgeVoxOut *vox; double *last_valid; const EdgeIndexed *ix;
  EdgeLane L;
  // direct results (the lanes of tr_validate_edges_indexed; e0 a multiple of 64): the verdicts are packed on the device and land
  // as whole words of the caller's mask, the FK counts in the caller's array (or nowhere) -- no per-edge pass on the host
  uint64_t *mask_out = nullptr; int32_t *nfk_out = nullptr; bool direct = false;
  int64_t own_samples = 0;        // samples of this run's own levels (sizes the next call's lanes)
  // derived
  int S = 0, P = 0; int64_t cap = 0, E = 0, base = 0; bool ret = false; int until = 0, sample_test = 1;
  trk::EdgeSpaceK sk{}; trk::EdgeState st{}; uint32_t *sig = nullptr; const int32_t *filter_np = nullptr; const int32_t *lvl0_idx = nullptr;
  double *lvl_states = nullptr; trk::EdgeIv *open = nullptr, *frontier = nullptr;
  int64_t pool = 0, n_bound = 0;
  bool slots_only = false;      // the samples go through the verdict-only kernels and nobody reads their points: the pool is EdgeDev's arrays
  // A sample evaluator in the place of launch_fk_sweep (loaded_edges_host.inc: the loaded FK, then K2 on the stored planes): it leaves
  // the points of the m level states in workspace columns [s0, s0 + m) and their verdicts in bits.  Such a run lives in the point
  // workspace and compares stored points (no signatures)
  std::function<int(EdgeRun &, int64_t, int64_t)> eval;

  static dim3 blocks(int64_t n) { return dim3((unsigned)((n + 255) / 256)); }

  // K1 + K2 on the m level states -> pool samples [s0, s0 + m) (s0 multiple of 64), verdicts folded into the edges
  int run_samples(int64_t s0, int64_t m) {
    EdgeDev &d = c->edge;
    int r;
    trk::FkOut out{};
    trk::SweepIn in{};
    if (!slots_only) { out = ws_fk_out(c, s0); in = ws_sweep_in(c, s0); }    // (a slots-only pool may be larger than the workspace: no plane is addressed by slot then)
    if (eval) { if ((r = eval(*this, s0, m))) return r; }
    else if ((r = launch_fk_sweep(c, lvl_states, m, cap, out, in, sample_test, d.bits + s0 / 64, nullptr, L.s,
                                  sig ? sig + s0 * d.sig_stride : nullptr, d.sig_stride, /*points_unused=*/sig != nullptr && !vox,
                                  (sig && ret) ? d.sig_np + s0 : nullptr, L.lane))) return r;
    ProfScope ps(c, 3, L.s);
    hipLaunchKernelGGL(trk::edge_fold, blocks(m), dim3(256), 0, L.s, st, s0, m, until);
    HIP_TRY(c, hipGetLastError());
    return TR_OK;
  }

  int enqueue_open() {                    // pop the frontier: midpoint states + pool slots, then the counters to the host
    {
      ProfScope ps(c, 3, L.s);
      HIP_TRY(c, hipMemsetAsync(L.counters + trk::EC_OPEN, 0, sizeof(uint32_t), L.s));
      hipLaunchKernelGGL(trk::edge_open, blocks(n_bound), dim3(256), 0, L.s, st, sk, frontier, n_bound, pool, L.slot_hi, until, open, lvl_states);
      HIP_TRY(c, hipGetLastError());
    }
    HIP_TRY(c, hipMemcpyAsync(L.hc, L.counters, trk::EC_COUNT * sizeof(uint32_t), hipMemcpyDeviceToHost, L.s));   // the one sync per level
    return TR_OK;
  }

  int start() {
    Workspace &w = c->ws;
    S = c->K.state_size; P = c->K.n_points;
    cap = w.ld; E = e1 - e0;
    base = ix ? ix->pool_base : 0;
    slots_only = !eval && c->edge_slots_now > 0 && !vox && c->fuse == 2 && edge_signatures(c, false);
    if (!slots_only && L.slot_hi > cap) return fail(c, TR_ERR_RUNTIME, "pool slots beyond the point workspace");
    if (!ix && L.slot_lo != 0) return fail(c, TR_ERR_RUNTIME, "pairwise edges start at pool slot 0");
    if (ix ? (L.slot_lo < base || 2 * E > L.slot_hi) : (2 * E > L.slot_hi - L.slot_lo)) return EDGE_OVERFLOW;
    int rc;
    if ((rc = ensure_edge_dev(c, std::max(cap, L.slot_hi)))) return rc;
    EdgeDev &d = c->edge;
    ret = c->K.enable_retraction;
    until = last_valid ? 1 : 0;
    // What decides a sample (launch_fk_sweep's voxel_test).  voxelize() tests is_valid_shape only (`do_nothing`,
    // VoxelBackboneMotionValidator.cpp:76-81); checkMotion(s1, s2) then tests the swept BACKBONE volume against the
    // validator's voxels whatever state checker is installed (AbstractVoxelMotionValidator.h:143-151) -- per sample
    // that is the backbone test; checkMotion(s1, s2, last_valid) asks the installed state checker, _vc->collides(shape)
    // (VoxelBackboneMotionValidator.cpp:83-91), which is the sphere-swept robot under TR_CHECKER_SPHERES.
    sample_test = vox ? (vox->collide ? 1 : 0) : ((until && c->checker == TR_CHECKER_SPHERES) ? 2 : 1);
    sk = edge_space(c, sp);
    const int64_t eo = L.eoff;
    st = edge_state(c, eo, L.counters);
    sig = (!eval && edge_signatures(c, vox != nullptr)) ? d.sig : nullptr;      // the fused launches write them, edge_filter compares them
    filter_np = ret ? (sig ? d.sig_np : w.np) : nullptr;             // point counts next to what the interval test reads
    lvl_states = d.lvl_states + L.level_off * S; open = d.open + L.level_off; frontier = d.frontier + 2 * L.level_off;

    if (!ix) {
      HIP_TRY(c, hipMemcpyAsync(d.A + eo * S, A + e0 * S, (size_t)E * S * sizeof(double), hipMemcpyHostToDevice, L.s));
      HIP_TRY(c, hipMemcpyAsync(d.B + eo * S, B + e0 * S, (size_t)E * S * sizeof(double), hipMemcpyHostToDevice, L.s));
    }
    HIP_TRY(c, hipMemsetAsync(d.sample_edge + L.slot_lo, 0xff, (size_t)(L.slot_hi - L.slot_lo) * sizeof(int32_t), L.s));
    HIP_TRY(c, hipMemsetAsync(L.counters, 0, trk::EC_COUNT * sizeof(uint32_t), L.s));

    // level 0: both end states of every edge (or the vertices evaluated once by the caller), then should_subdivide
    // on the whole edges
    lvl0_idx = ix ? ix->d_idx + 2 * e0 : nullptr;
    if (ix) {
      ProfScope ps(c, 3, L.s);
      hipLaunchKernelGGL(trk::edge_init_indexed, blocks(E), dim3(256), 0, L.s, st, sk, E, ix->d_states, lvl0_idx, d.A + eo * S, d.B + eo * S);
      HIP_TRY(c, hipGetLastError());
      pool = L.slot_lo;
    } else {
      {
        ProfScope ps(c, 3, L.s);
        hipLaunchKernelGGL(trk::edge_init, blocks(E), dim3(256), 0, L.s, st, sk, E, lvl_states);
        HIP_TRY(c, hipGetLastError());
      }
      if ((rc = run_samples(0, 2 * E))) return rc;
      pool = round_up(2 * E, 64);
    }
    {
      ProfScope ps(c, 3, L.s);
      hipLaunchKernelGGL((trk::edge_filter<true>), blocks(E), dim3(256), 0, L.s, st, (const trk::EdgeIv *)nullptr, lvl0_idx, E, (int64_t)0,
                         w.px, w.py, w.pz, cap, P, filter_np, c->G, until, frontier, sig, d.sig_stride);
      HIP_TRY(c, hipGetLastError());
    }
    n_bound = E;                            // upper bound of the frontier size (the exact count stays on the device)
    return enqueue_open() == TR_OK ? EDGE_MORE : TR_ERR_HIP;
  }

  // the lane's stream has drained: the counters of the last edge_open are on the host
  int resume() {
    Workspace &w = c->ws; EdgeDev &d = c->edge;
    int rc;
    const int64_t m = L.hc[trk::EC_OPEN];
    if (edge_timing()) {
      // ... and how many samples of the level just evaluated went through the fallback pass (exact self-collision sweep)
      uint32_t fb = 0;
      if (const uint32_t *fbc = c->lane[L.lane].fb_count) (void)hipMemcpy(&fb, fbc, sizeof(fb), hipMemcpyDeviceToHost);
      std::fprintf(stderr, "[edge lane %d] level of %lld samples (pool at %lld; previous level: %u through the fallback pass)\n", L.lane, (long long)m,
                   (long long)pool, fb);
    }
    if (m > 0) {
      if (pool + round_up(m, 64) > L.slot_hi) return EDGE_OVERFLOW;            // pool overflow: caller retries with a smaller chunk
      own_samples += m;
      const int64_t s0 = pool;
      if (ret && vox && c->retract_sort_min > 0 && m >= c->retract_sort_min) {
        // stored-point forms of a retraction robot (K1r -> K2 -> K5; the verdict-only path orders its launches itself): deal
        // the level's samples in the order of their backbone lengths
        EdgeDev &dd = c->edge;
        tr_ctx::RetractOrder &ro = c->lane[0].ro;
        if (ro.cap < m && (rc = ensure_lane_order(c, 0, round_up(m + m / 4, 64)))) return rc;
        const int32_t *perm = nullptr;
        const hipError_t e = trk::retraction_order(c->merge, lvl_states, m, S, c->K.L, ro.keys, ro.vals, &perm, L.s);
        if (e != hipSuccess) return fail(c, TR_ERR_HIP, std::string("retraction order (edge level): ") + hipGetErrorString(e));
        trk::EdgeIv *open_to = (open == dd.open2) ? dd.open : dd.open2;
        double *lvl_to = (lvl_states == dd.lvl_states2) ? dd.lvl_states : dd.lvl_states2;
        ProfScope ps(c, 3, L.s);
        hipLaunchKernelGGL(trk::edge_level_gather, blocks(m), dim3(256), 0, L.s, st, perm, m, S, s0, (const trk::EdgeIv *)open, (const double *)lvl_states,
                           open_to, lvl_to);
        HIP_TRY(c, hipGetLastError());
        open = open_to; lvl_states = lvl_to;
      }
      if ((rc = run_samples(s0, m))) return rc;
      pool = s0 + round_up(m, 64);
      {
        ProfScope ps(c, 3, L.s);
        HIP_TRY(c, hipMemsetAsync(L.counters + trk::EC_FRONT, 0, sizeof(uint32_t), L.s));
        hipLaunchKernelGGL((trk::edge_filter<false>), blocks(2 * m), dim3(256), 0, L.s, st, (const trk::EdgeIv *)open, (const int32_t *)nullptr, 2 * m, s0,
                           w.px, w.py, w.pz, cap, P, filter_np, c->G, until, frontier, sig, d.sig_stride);
        HIP_TRY(c, hipGetLastError());
      }
      n_bound = 2 * m;
      return enqueue_open() == TR_OK ? EDGE_MORE : TR_ERR_HIP;
    }
    // ---- the bisection is over ----
    if (last_valid) {
      hipLaunchKernelGGL(trk::edge_last_valid_t, blocks(pool - L.slot_lo), dim3(256), 0, L.s, st, L.slot_lo, pool);
      HIP_TRY(c, hipGetLastError());
      HIP_TRY(c, hipMemcpyAsync(last_valid + e0, st.last_t, (size_t)E * sizeof(double), hipMemcpyDeviceToHost, L.s));   // bits of non-negative doubles
    }
    std::vector<uint32_t> hok;          // (host-side results only)
    if (direct) {
      uint64_t *d_words = reinterpret_cast<uint64_t *>(d.nd) + L.eoff / 64;     // (the discrete variant's array: idle here)
      hipLaunchKernelGGL(trk::edge_ok_bits, blocks(E), dim3(256), 0, L.s, (const uint32_t *)st.edge_ok, E, d_words);
      HIP_TRY(c, hipGetLastError());
      HIP_TRY(c, hipMemcpyAsync(mask_out + e0 / 64, d_words, (size_t)((E + 63) / 64) * sizeof(uint64_t), hipMemcpyDeviceToHost, L.s));
      if (nfk_out) HIP_TRY(c, hipMemcpyAsync(nfk_out + e0, st.nfk, (size_t)E * sizeof(int32_t), hipMemcpyDeviceToHost, L.s));
    } else {
      hok.resize((size_t)E);
      HIP_TRY(c, hipMemcpyAsync(hok.data(), st.edge_ok, (size_t)E * sizeof(uint32_t), hipMemcpyDeviceToHost, L.s));
      HIP_TRY(c, hipMemcpyAsync(&(*edge_nfk)[(size_t)e0], st.nfk, (size_t)E * sizeof(int32_t), hipMemcpyDeviceToHost, L.s));
    }
    HIP_TRY(c, hipMemcpyAsync(L.hc, L.counters, trk::EC_COUNT * sizeof(uint32_t), hipMemcpyDeviceToHost, L.s));
    HIP_TRY(c, hipStreamSynchronize(L.s));
    for (size_t k = 0; k < hok.size(); k++) (*edge_ok)[(size_t)e0 + k] = hok[k] ? 1 : 0;
    if (n_domain) *n_domain += L.hc[trk::EC_DOMAIN];
    if (vox) {
      // union of the sampled backbones of every fully valid edge (VoxelEnvironment.cpp:406-422); whole pool, null stream only
      if ((rc = ensure_vox_scratch(c, cap))) return rc;
      hipLaunchKernelGGL(trk::edge_sample_bits, blocks(pool), dim3(256), 0, nullptr, st, pool, c->d_vbits);
      HIP_TRY(c, hipGetLastError());
      {
        // block lists of this chunk's own samples, pool slots [base, pool) (base = 0 unless the edges are indexed: then the
        // vertices' lists in slots [0, base) were built once by the caller)
        ProfScope ps(c, 3, nullptr);
        const int64_t m = pool - base;
        if (m > 0)
          hipLaunchKernelGGL(trk::backbone_voxelize, dim3((unsigned)((m + 63) / 64)), dim3(64), 0, nullptr, w.px + base, w.py + base, w.pz + base,
                             ret ? w.np + base : nullptr, c->d_vbits + base / 64, m, cap, P, c->G, vox_max_blocks(c), c->d_vids + base,
                             c->d_vmasks + base, c->d_vcounts + base);
        HIP_TRY(c, hipGetLastError());
      }
      // merge the samples of each edge on the device: (edge, block id) sorted, masks OR-ed (cache_merge.hip)
      int64_t nu = 0;
      int ovf = 0;
      if (ix) {
        const int64_t items = pool + 2 * E;
        if (c->vox_items_cap < items) {
          HIP_TRY(c, hipDeviceSynchronize());
          if ((rc = dev_alloc(c, &c->d_item_src, (size_t)items + items / 4))) return rc;
          if ((rc = dev_alloc(c, &c->d_item_edge, (size_t)items + items / 4))) return rc;
          c->vox_items_cap = items + items / 4;
        }
        ProfScope ps(c, 3, nullptr);
        hipLaunchKernelGGL(trk::edge_cache_items, blocks(items), dim3(256), 0, nullptr, st, pool, E, lvl0_idx, c->d_item_src, c->d_item_edge);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, trk::merge_edge_caches(c->merge, c->d_vids, c->d_vmasks, c->d_vcounts, c->d_item_src, c->d_item_edge, items, cap, c->n_blocks, E, &nu, &ovf, nullptr));
      } else {
        ProfScope ps(c, 3, nullptr);
        HIP_TRY(c, trk::merge_edge_caches(c->merge, c->d_vids, c->d_vmasks, c->d_vcounts, nullptr, d.sample_edge, pool, cap, c->n_blocks, E, &nu, &ovf, nullptr));
      }
      if (ovf) return fail(c, TR_ERR_RUNTIME, "voxel set of a configuration exceeds the block-list capacity or leaves the domain");
      if ((rc = vstore_append(c, c->merge.uids, c->merge.uvals, nu))) return rc;
      HIP_TRY(c, hipMemcpy(&vox->count[(size_t)e0], c->merge.ecount, (size_t)E * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    return 0;
  }
};

// The edge queue's arguments (edge_queue_kernel.hpp) over the whole of EdgeDev, slots up to slot_hi: the pinned image filled, its
// copy to the device enqueued on the null stream.  (No retraction robot comes here: the workspace views hold no point counts.)
int fill_queue_args(tr_ctx *c, const trk::EdgeSpaceK &sk, int32_t slot_hi) {
  EdgeDev &d = c->edge;
  trk::EdgeQueueArgs &qa = *d.q_hargs;
  qa = trk::EdgeQueueArgs{};
  qa.ctl = d.q_ctl; qa.slot_hi = slot_hi; qa.P = c->K.n_points; qa.sk = sk;
  qa.A = d.A; qa.B = d.B; qa.rel = d.rel; qa.edge_ok = d.edge_ok; qa.nfk = d.nfk;
  qa.remaining = d.q_remaining; qa.lvl_base = d.q_lvl_base; qa.lvl_cnt = d.q_lvl_cnt;
  qa.iv = d.open; qa.states = d.lvl_states; qa.sample_edge = d.sample_edge; qa.sig = d.sig; qa.sig_stride = d.sig_stride;
  qa.fb_out = ws_fk_out(c, 0);
  qa.fb_in = ws_sweep_in(c, 0);
  qa.fb_ld = c->ws.ld;
  HIP_TRY(c, hipMemcpyAsync(d.q_args, &qa, sizeof(qa), hipMemcpyHostToDevice, nullptr));
  return TR_OK;
}

// The indexed edges [0, E) as ONE persistent launch over a device work queue (edge_kernel.hpp: "the edge queue",
// edge_queue_kernel.hpp): level 0 -- should_subdivide on the whole edges, from the vertices' signature rows in pool slots
// [0, ix.pool_base) -- by the level-synchronous helpers, their open intervals seed the queue, and everything after that is the
// queue's: no counter comes back to the host before the end, no launch waits for another.  Null stream; the mask words and the FK
// counts go straight to the caller's arrays.  Returns TR_OK, EDGE_OVERFLOW (the pool -- or an edge level -- is larger than the
// queue takes: the caller falls back to the level-synchronous lanes) or an error.
int edges_queue_run(tr_ctx *c, const tr_space_params *sp, const EdgeIndexed &ix, int64_t E, int64_t cap, uint64_t *mask_out,
                    int32_t *nfk_out, int64_t *n_domain, int64_t *own_samples, int waves) {
  const bool timing = edge_timing();
  EdgeDev &d = c->edge; Workspace &w = c->ws;
  const int S = c->K.state_size, P = c->K.n_points;
  const int64_t s0 = ix.pool_base;
  if (!d.q_ctl || cap > d.cap || s0 + 64 > cap || cap >= ((int64_t)1 << 30)) return EDGE_OVERFLOW;
  hipStream_t s = nullptr;

  const trk::EdgeSpaceK sk = edge_space(c, sp);
  const trk::EdgeState st = edge_state(c, 0, c->lane[0].counters);
  auto blocks = [](int64_t n) { return dim3((unsigned)((n + 255) / 256)); };
  HIP_TRY(c, hipMemsetAsync(st.counters, 0, trk::EC_COUNT * sizeof(uint32_t), s));
  HIP_TRY(c, hipMemsetAsync(d.q_ctl, 0, trk::EQ_WORDS * sizeof(uint32_t), s));
  {
    ProfScope ps(c, 3, s);
    hipLaunchKernelGGL(trk::edge_init_indexed, blocks(E), dim3(256), 0, s, st, sk, E, ix.d_states, ix.d_idx, d.A, d.B);
    hipLaunchKernelGGL((trk::edge_filter<true>), blocks(E), dim3(256), 0, s, st, (const trk::EdgeIv *)nullptr, ix.d_idx, E, (int64_t)0,
                       w.px, w.py, w.pz, w.ld, P, (const int32_t *)nullptr, c->G, 0, d.frontier, d.sig, d.sig_stride);
    // the open intervals' records at their slots' own positions: slot s0 + q holds interval q and its midpoint state
    hipLaunchKernelGGL(trk::edge_open, blocks(E), dim3(256), 0, s, st, sk, (const trk::EdgeIv *)d.frontier, E, s0, cap, 0, d.open + s0, d.lvl_states + s0 * S);
    hipLaunchKernelGGL(trk::edge_queue_seed, blocks(E), dim3(256), 0, s, st, (const trk::EdgeIv *)d.open, s0, cap, d.q_remaining, d.q_lvl_base,
                       d.q_lvl_cnt, d.q_ctl);
    HIP_TRY(c, hipGetLastError());
  }
  int rc;
  if ((rc = fill_queue_args(c, sk, (int32_t)cap))) return rc;
  hipEvent_t tev[2] = {nullptr, nullptr};
  if (timing) { (void)hipEventCreate(&tev[0]); (void)hipEventCreate(&tev[1]); (void)hipEventRecord(tev[0], s); }
  if ((rc = launch_edge_queue(c, s, d.sig, d.sig_stride, d.q_args, (unsigned)waves))) return rc;
  if (timing) (void)hipEventRecord(tev[1], s);
  uint64_t *d_words = reinterpret_cast<uint64_t *>(d.nd);       // (the discrete variant's array: idle here)
  hipLaunchKernelGGL(trk::edge_ok_bits, blocks(E), dim3(256), 0, s, (const uint32_t *)d.edge_ok, E, d_words);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(d.q_hctl, d.q_ctl, trk::EQ_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  const uint32_t flags = d.q_hctl[trk::EQ_FLAGS];
  c->edge_queue_last[0] = d.q_hctl[trk::EQ_TAIL] - (uint32_t)s0; c->edge_queue_last[1] = d.q_hctl[trk::EQ_BATCHES];
  c->edge_queue_last[2] = d.q_hctl[trk::EQ_PENDING]; c->edge_queue_last[3] = flags;
  if (timing) {
    std::fprintf(stderr, "[edge queue] %u waves, %u samples in %u rounds (%.1f per round), %u through the exact sweep, flags %u\n", (unsigned)waves,
                 c->edge_queue_last[0], c->edge_queue_last[1], c->edge_queue_last[1] ? (double)c->edge_queue_last[0] / c->edge_queue_last[1] : 0.0,
                 c->edge_queue_last[2], flags);
    float kms = 0.0f;
    (void)hipEventElapsedTime(&kms, tev[0], tev[1]);
    (void)hipEventDestroy(tev[0]); (void)hipEventDestroy(tev[1]);
    std::fprintf(stderr, "[edge queue] launch %.3f ms\n", kms);
    const unsigned long long *t64 = reinterpret_cast<const unsigned long long *>(d.q_hctl);
    const double tot = (double)(t64[trk::EQ_T_CLAIM / 2] + t64[trk::EQ_T_READY / 2] + t64[trk::EQ_T_FK / 2] + t64[trk::EQ_T_EXACT / 2] + t64[trk::EQ_T_FOLD / 2]);
    std::fprintf(stderr, "[edge queue] levels finished %u, candidates %u; wave time %.1f ms per wave: claim %.1f %%, records %.1f %%, integration %.1f %%, exact sweep %.1f %%, fold + finish %.1f %%\n",
                 d.q_hctl[trk::EQ_FINISHED], d.q_hctl[trk::EQ_CAND], 1e-5 * tot / waves, 100.0 * t64[trk::EQ_T_CLAIM / 2] / tot, 100.0 * t64[trk::EQ_T_READY / 2] / tot,
                 100.0 * t64[trk::EQ_T_FK / 2] / tot, 100.0 * t64[trk::EQ_T_EXACT / 2] / tot, 100.0 * t64[trk::EQ_T_FOLD / 2] / tot);
    std::fprintf(stderr, "[edge queue] rounds of 64 / 32..63 / 2..31 / 1 samples: %u / %u / %u / %u\n", d.q_hctl[trk::EQ_SIZES], d.q_hctl[trk::EQ_SIZES + 1], d.q_hctl[trk::EQ_SIZES + 2], d.q_hctl[trk::EQ_SIZES + 3]);
    std::fprintf(stderr, "[edge queue] inside fold + finish, us per round: release + decrement %.1f, acquire + records %.1f, candidates %.1f, allocation + records %.1f, release + publish %.1f\n",
                 1e-2 * t64[trk::EQ_T_F0 / 2] / d.q_hctl[trk::EQ_BATCHES], 1e-2 * t64[trk::EQ_T_F1 / 2] / d.q_hctl[trk::EQ_BATCHES], 1e-2 * t64[trk::EQ_T_F2 / 2] / d.q_hctl[trk::EQ_BATCHES],
                 1e-2 * t64[trk::EQ_T_F3 / 2] / d.q_hctl[trk::EQ_BATCHES], 1e-2 * t64[trk::EQ_T_F4 / 2] / d.q_hctl[trk::EQ_BATCHES]);
  }
#ifdef TRK_EQ_TRACE
  if (timing) {
    uint32_t t0 = 0xffffffffu;
    for (int wv = 0; wv < 8; wv++) if (d.q_hctl[trk::EQ_TRACE + wv * 256 + 3]) t0 = std::min(t0, d.q_hctl[trk::EQ_TRACE + wv * 256]);
    for (int wv = 0; wv < 8; wv++) {
      std::fprintf(stderr, "[edge queue] wave %4d, rounds (start, integration, fold in us; shader MHz):", wv * 256);
      for (int rd = 0; rd < 64; rd++) {
        const uint32_t *tw = d.q_hctl + trk::EQ_TRACE + (wv * 64 + rd) * 4;
        if (!tw[3]) break;
        std::fprintf(stderr, " %.0f/%.0f/%.0f/%u", 1e-2 * (double)(tw[0] - t0), 1e-2 * (double)(tw[1] - tw[0]), 1e-2 * (double)(tw[2] - tw[1]), tw[3]);
      }
      std::fprintf(stderr, "\n");
    }
  }
#endif
  if (flags & trk::EQF_STUCK) return fail(c, TR_ERR_RUNTIME, "edge queue: a wait made no progress (launch abandoned)");
  if (flags) return EDGE_OVERFLOW;
  if (d.q_hctl[trk::EQ_DONE] != d.q_hctl[trk::EQ_TAIL]) return fail(c, TR_ERR_RUNTIME, "edge queue: launch ended with samples in flight");
  if ((rc = download_staged(c, mask_out, d_words, (size_t)((E + 63) / 64) * sizeof(uint64_t), s))) return rc;
  if (nfk_out && (rc = download_staged(c, nfk_out, d.nfk, (size_t)E * sizeof(int32_t), s))) return rc;     // (d.nfk holds cap / 2 + 1 entries: the padding word exists)
  if (n_domain) *n_domain = d.q_hctl[trk::EQ_DOMAIN] + 0;
  if (own_samples) *own_samples = (int64_t)c->edge_queue_last[0];
  return TR_OK;
}

// One chunk of edges [e0, e1) on the whole pool and the null stream.  Returns TR_OK, an error, or EDGE_OVERFLOW when the sample pool
// overflowed (caller halves the chunk).
int edges_chunk(tr_ctx *c, const tr_space_params *sp, const double *A, const double *B, int64_t e0, int64_t e1,
                std::vector<uint8_t> &edge_ok, std::vector<int32_t> &edge_nfk, int64_t *n_domain,
                EdgeVoxOut *vox, double *last_valid /* per edge (global index) or null */, const EdgeIndexed *ix = nullptr) {
  int rc;
  const int64_t slots = (c->edge_slots_now > 0 && !vox) ? c->edge_slots_now : c->ws.ld;
  if ((rc = ensure_edge_dev(c, std::max(slots, c->ws.ld)))) return rc;
  if ((rc = ensure_edge_lanes(c))) return rc;
  EdgeRun r{c, sp, A, B, e0, e1, &edge_ok, &edge_nfk, n_domain, vox, last_valid, ix};
  r.L = EdgeLane{nullptr, 0, ix ? ix->pool_base : 0, slots, 0, 0, c->lane[0].counters, c->lane[0].hc};
  int stt = r.start();
  while (stt == EDGE_MORE) {
    HIP_TRY(c, hipStreamSynchronize(nullptr));
    stt = r.resume();
  }
  return stt;
}

int edges_range(tr_ctx *c, const tr_space_params *sp, const double *A, const double *B, int64_t e0, int64_t e1,
                std::vector<uint8_t> &edge_ok, std::vector<int32_t> &edge_nfk, int64_t *n_domain, EdgeVoxOut *vox, double *last_valid = nullptr,
                const EdgeIndexed *ix = nullptr) {
  // reset partial results of a retried range
  for (int64_t e = e0; e < e1; e++) { edge_ok[(size_t)e] = 1; edge_nfk[(size_t)e] = 0; }
  int64_t nd = 0;
  const int64_t vox_mark = c->vstore.n;
  int rc = edges_chunk(c, sp, A, B, e0, e1, edge_ok, edge_nfk, &nd, vox, last_valid, ix);
  if (rc == EDGE_OVERFLOW) {
    if (vox) c->vstore.n = vox_mark;
    if (e1 - e0 <= 1) return fail(c, TR_ERR_RUNTIME, "an edge needs more FK samples than the workspace holds");
    const int64_t mid = e0 + (e1 - e0) / 2;
    if ((rc = edges_range(c, sp, A, B, e0, mid, edge_ok, edge_nfk, n_domain, vox, last_valid, ix))) return rc;
    return edges_range(c, sp, A, B, mid, e1, edge_ok, edge_nfk, n_domain, vox, last_valid, ix);
  }
  if (rc == TR_OK && n_domain) *n_domain += nd;
  return rc;
}

// Chunks of edges sized for the sample pool (edge_plan.hpp): `avail` pool samples for a chunk's own samples, `guess` samples per
// edge assumed for the first chunk; later chunks use what the previous one needed (the reference's per-edge FK counts)
template <class Run>
int for_edge_chunks(int64_t n_edges, int64_t avail, double guess, int ends, const std::vector<int32_t> &nfk, Run &&run) {
  double rate = guess;
  for (int64_t e0 = 0; e0 < n_edges;) {
    const int64_t e1 = edge_plan::chunk_end(e0, n_edges, avail, rate);
    const int rc = run(e0, e1);
    if (rc) return rc;
    double sum = 0;
    for (int64_t e = e0; e < e1; e++) sum += nfk[(size_t)e];
    rate = edge_plan::chunk_rate(sum / (double)(e1 - e0), ends);
    e0 = e1;
  }
  return TR_OK;
}

int ensure_edge_pool(tr_ctx *c, int64_t n_edges) {
  const int64_t grown = edge_plan::pool_growth(c->edge_rate_seen, n_edges, c->ws.ld, c->edge_pool_max);
  if (!grown) return TR_OK;
  const int64_t keep = c->max_chunk;
  c->max_chunk = std::max(c->max_chunk, grown);       // ensure_workspace clamps to max_chunk
  const int rc = ensure_workspace(c, grown);
  c->max_chunk = keep;
  return rc;
}

// Every lane's fallback list sized for a whole share of the pool, R slots, before the lanes start (growing one mid-run would stall
// all streams) and, with `order` (a retraction robot's run), every lane's ordering buffers
int reserve_lanes(tr_ctx *c, int NL, int64_t R, bool order) {
  int rc;
  for (int l = 0; l < NL; l++)
    if ((rc = ensure_lane_fallback(c, l, R)) || (order && (rc = ensure_lane_order(c, l, R)))) return rc;
  return TR_OK;
}

}  // namespace
