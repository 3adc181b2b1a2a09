// fk_inst.hip -- one K1 instantiation set per object file: compiled once per tendon count and
// kernel with -DTRK_INST_N=<1..8> -DTRK_INST_KIND=<0 uniform | 1 retract | 2 fused with K2 | 3 verdict-only | 4 verdict-only, retraction | 5 edge queue | 6 loaded | 7 loaded under a load profile | 8 loaded, retraction>
// (see _lib.py: build()).
#include "fk_launch.hpp"
#include "fk_kernel.hpp"
#if TRK_INST_KIND == 1
#include "fk_retract_kernel.hpp"
#elif TRK_INST_KIND == 2
#include "fused_kernel.hpp"
#elif TRK_INST_KIND == 3
#include "verdict_kernel.hpp"
#elif TRK_INST_KIND == 4
#define TRK_WITH_RETRACT_VERDICT
#include "fk_retract_kernel.hpp"
#include "verdict_kernel.hpp"
#elif TRK_INST_KIND == 5
#include "edge_queue_kernel.hpp"
#elif TRK_INST_KIND == 6 || TRK_INST_KIND == 7
#define TRK_LOADED_WITH_INTEGRATOR
#include "fk_loaded_kernel.hpp"
#elif TRK_INST_KIND == 8
#include "fk_loaded_retract_kernel.hpp"
#endif

namespace trk {

// The routing form of a launch of the unloaded shared-grid kernels: the context's one decision (RobotK::routing_form, tr_create).
// UniformHelix is instantiated only where K1's two-wave allocation exists; a wider robot's context never asks for it.
using HelixForm = std::conditional_t<(TRK_INST_N <= TRK_K1_TWO_WAVE_MAXN), UniformHelix, TableRouting>;
[[maybe_unused]] static bool helix_form(const RobotK &K) { return TRK_INST_N <= TRK_K1_TWO_WAVE_MAXN && K.routing_form == TRK_ROUTING_HELIX; }

#if TRK_INST_KIND == 5
template <class Form>
static void go_queue(const FkLaunch &a, const VerdictArgs *va, size_t lds, const EdgeQueueArgs *qa, const FusedSweepArgs *sweep, unsigned waves) {
  if (a.rotation)
    hipLaunchKernelGGL((fk_edge_queue<TRK_INST_N, true, Form>), dim3(waves), dim3(64), lds, a.stream, a.K, a.d_tab, a.d_steps, a.n_steps, va, qa, sweep);
  else
    hipLaunchKernelGGL((fk_edge_queue<TRK_INST_N, false, Form>), dim3(waves), dim3(64), lds, a.stream, a.K, a.d_tab, a.d_steps, a.n_steps, va, qa, sweep);
}
template <class Form>
static int queue_waves_per_cu(bool rotation, size_t lds) {
  int nb = 0;
  const hipError_t e = rotation ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fk_edge_queue<TRK_INST_N, true, Form>, 64, lds)
                                : hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fk_edge_queue<TRK_INST_N, false, Form>, 64, lds);
  return e == hipSuccess ? nb : 0;
}
template <> void launch_fk_edge_queue<TRK_INST_N>(const FkLaunch &a, const VerdictArgs *va, size_t lds, const EdgeQueueArgs *qa,
                                                  const FusedSweepArgs *sweep, unsigned waves) {
  if (helix_form(a.K)) go_queue<HelixForm>(a, va, lds, qa, sweep, waves); else go_queue<TableRouting>(a, va, lds, qa, sweep, waves);
}
template <> int fk_edge_queue_waves_per_cu<TRK_INST_N>(const RobotK &K, size_t lds) {
  return helix_form(K) ? queue_waves_per_cu<HelixForm>((bool)K.enable_rotation, lds) : queue_waves_per_cu<TableRouting>((bool)K.enable_rotation, lds);
}
#endif

#if TRK_INST_KIND == 5
#elif TRK_INST_KIND == 6
template <bool ROT, bool WR>
static void go(const FkLaunch &a, const LoadedIn &in) {
  const unsigned grid = (unsigned)((a.n + 63) / 64);
  hipLaunchKernelGGL((fk_loaded_uniform<TRK_INST_N, ROT, WR>), dim3(grid), dim3(64), 0, a.stream, a.d_states, a.n, a.ld, a.K,
                     a.d_tab, a.d_steps, a.n_steps, a.out, in);
}
template <> void launch_fk_loaded<TRK_INST_N>(const FkLaunch &a, const LoadedIn &in) {
  if (in.weights) return launch_fk_loaded_profile<TRK_INST_N>(a, in);
  if (a.rotation) { if (a.write_R) go<true, true>(a, in); else go<true, false>(a, in); }
  else            { if (a.write_R) go<false, true>(a, in); else go<false, false>(a, in); }
}
template <> void launch_shoot_start<TRK_INST_N>(const FkLaunch &a, const double *guess, double *vu) {
  const unsigned grid = (unsigned)((a.n + 63) / 64);
  hipLaunchKernelGGL((shoot_start<TRK_INST_N>), dim3(grid), dim3(64), 0, a.stream, a.d_states, a.n, a.K, a.d_tab, guess, vu);
}
#elif TRK_INST_KIND == 7
template <bool ROT, bool WR>
static void go(const FkLaunch &a, const LoadedIn &in) {
  const unsigned grid = (unsigned)((a.n + 63) / 64);
  hipLaunchKernelGGL((fk_loaded_profile<TRK_INST_N, ROT, WR>), dim3(grid), dim3(64), 0, a.stream, a.d_states, a.n, a.ld, a.K,
                     a.d_tab, a.d_steps, a.n_steps, a.out, in);
}
template <> void launch_fk_loaded_profile<TRK_INST_N>(const FkLaunch &a, const LoadedIn &in) {
  if (a.rotation) { if (a.write_R) go<true, true>(a, in); else go<true, false>(a, in); }
  else            { if (a.write_R) go<false, true>(a, in); else go<false, false>(a, in); }
}
#elif TRK_INST_KIND == 8
template <bool ROT, bool WR>
static void go(const FkLaunch &a, const LoadedIn &in) {
  const unsigned grid = (unsigned)((a.n + 63) / 64);
  hipLaunchKernelGGL((fk_loaded_retract<TRK_INST_N, ROT, WR>), dim3(grid), dim3(64), 0, a.stream, a.d_states, a.n, a.ld, a.K, a.d_poly,
                     a.d_tab, a.d_steps, a.n_steps, a.k_first, a.d_tgrid, a.d_hl, a.out, in);
}
template <> void launch_fk_loaded_retract<TRK_INST_N>(const FkLaunch &a, const LoadedIn &in) {
  if (a.rotation) { if (a.write_R) go<true, true>(a, in); else go<true, false>(a, in); }
  else            { if (a.write_R) go<false, true>(a, in); else go<false, false>(a, in); }
}
template <> void launch_shoot_start_retract<TRK_INST_N>(const FkLaunch &a, const double *guess, double *vu, const int32_t *perm) {
  const unsigned grid = (unsigned)((a.n + 63) / 64);
  hipLaunchKernelGGL((shoot_start_retract<TRK_INST_N>), dim3(grid), dim3(64), 0, a.stream, a.d_states, a.n, a.K, a.d_poly, guess, vu, perm);
}
#elif TRK_INST_KIND == 4
template <bool ROT, bool SPH, bool SIG>
static void go(const FkLaunch &a, const VerdictArgs *va, size_t lds) {
  const unsigned grid = (unsigned)((a.n + 63) / 64);
  const RetractHandoff ho{a.d_handoff, a.handoff_ld};
  hipLaunchKernelGGL((fk_retract_prologue<TRK_INST_N, ROT>), dim3(grid), dim3(64), 0, a.stream, a.d_states, a.n, a.K, a.d_poly, a.d_tab, a.d_steps,
                     a.n_steps, a.k_first, a.d_tgrid, a.d_hl, a.d_perm, ho);
  hipLaunchKernelGGL((fk_verdict_retract<TRK_INST_N, ROT, SPH, SIG>), dim3(grid), dim3(64), lds, a.stream, a.d_states, a.n, a.K, a.d_poly,
                     a.d_tab, a.d_steps, a.n_steps, a.k_first, a.d_tgrid, a.d_hl, a.out.tips, va, ho);
}
template <bool SPH, bool SIG>
static void go_rot(const FkLaunch &a, const VerdictArgs *va, size_t lds) {
  if (a.rotation) go<true, SPH, SIG>(a, va, lds); else go<false, SPH, SIG>(a, va, lds);
}
template <> void launch_fk_verdict_retract<TRK_INST_N>(const FkLaunch &a, const VerdictArgs *va, size_t lds, bool spheres, bool with_sig) {
  if (spheres) { if (with_sig) go_rot<true, true>(a, va, lds); else go_rot<true, false>(a, va, lds); }
  else         { if (with_sig) go_rot<false, true>(a, va, lds); else go_rot<false, false>(a, va, lds); }
}
template <bool ROT>
static void go_list(const FkLaunch &a, const FusedSweepArgs *sweep, size_t lds, const int32_t *list, const uint32_t *count) {
  const unsigned grid = (unsigned)((a.n + 63) / 64);                       // a.n = columns of the fallback workspace (multiple of 64)
  hipLaunchKernelGGL((fk_sweep_retract_list<TRK_INST_N, ROT>), dim3(grid), dim3(64), lds, a.stream, a.d_states, a.n, a.ld, a.K,
                     a.d_poly, a.d_tab, a.d_steps, a.n_steps, a.k_first, a.d_tgrid, a.d_hl, a.out, sweep, list, count);
}
template <> void launch_fk_sweep_retract_list<TRK_INST_N>(const FkLaunch &a, const FusedSweepArgs *sweep, size_t lds, const int32_t *list,
                                                          const uint32_t *count) {
  if (a.rotation) go_list<true>(a, sweep, lds, list, count); else go_list<false>(a, sweep, lds, list, count);
}
#elif TRK_INST_KIND == 3
template <bool ROT, bool SPH, bool SIG, class Form>
static void go(const FkLaunch &a, const VerdictArgs *va, size_t lds) {
  const unsigned grid = (unsigned)((a.n + 63) / 64);
  hipLaunchKernelGGL((fk_verdict<TRK_INST_N, ROT, SPH, SIG, Form>), dim3(grid), dim3(64), lds, a.stream, a.d_states, a.n, a.K, a.d_tab, a.d_steps,
                     a.n_steps, a.out.tips, va);
}
template <bool SPH, bool SIG>
static void go_rot(const FkLaunch &a, const VerdictArgs *va, size_t lds) {
  if (helix_form(a.K)) { if (a.rotation) go<true, SPH, SIG, HelixForm>(a, va, lds); else go<false, SPH, SIG, HelixForm>(a, va, lds); }
  else                 { if (a.rotation) go<true, SPH, SIG, TableRouting>(a, va, lds); else go<false, SPH, SIG, TableRouting>(a, va, lds); }
}
template <> void launch_fk_verdict<TRK_INST_N>(const FkLaunch &a, const VerdictArgs *va, size_t lds, bool spheres, bool with_sig) {
  if (spheres) { if (with_sig) go_rot<true, true>(a, va, lds); else go_rot<true, false>(a, va, lds); }
  else         { if (with_sig) go_rot<false, true>(a, va, lds); else go_rot<false, false>(a, va, lds); }
}
#elif TRK_INST_KIND == 2
template <bool ROT, class Form>
static void go_list(const FkLaunch &a, const FusedSweepArgs *sweep, size_t lds, const int32_t *list, const uint32_t *count) {
  const unsigned grid = (unsigned)((a.n + 63) / 64);                       // a.n = columns of the fallback workspace (multiple of 64)
  hipLaunchKernelGGL((fk_sweep_fused_list<TRK_INST_N, ROT, Form>), dim3(grid), dim3(64), lds, a.stream, a.d_states, a.n, a.ld, a.K,
                     a.d_tab, a.d_steps, a.n_steps, a.out, sweep, list, count);
}
template <> void launch_fk_sweep_fused_list<TRK_INST_N>(const FkLaunch &a, const FusedSweepArgs *sweep, size_t lds, const int32_t *list,
                                                        const uint32_t *count) {
  if (helix_form(a.K)) { if (a.rotation) go_list<true, HelixForm>(a, sweep, lds, list, count); else go_list<false, HelixForm>(a, sweep, lds, list, count); }
  else                 { if (a.rotation) go_list<true, TableRouting>(a, sweep, lds, list, count); else go_list<false, TableRouting>(a, sweep, lds, list, count); }
}
template <bool ROT, class Form>
static void go(const FkLaunch &a, const FusedSweepArgs *sweep, size_t lds) {
  const unsigned grid = (unsigned)((a.n + 63) / 64);
  hipLaunchKernelGGL((fk_sweep_fused<TRK_INST_N, ROT, Form>), dim3(grid), dim3(64), lds, a.stream, a.d_states, a.n, a.ld, a.K,
                     a.d_tab, a.d_steps, a.n_steps, a.out, sweep);
}
template <> void launch_fk_sweep_fused<TRK_INST_N>(const FkLaunch &a, const FusedSweepArgs *sweep, size_t lds) {
  if (helix_form(a.K)) { if (a.rotation) go<true, HelixForm>(a, sweep, lds); else go<false, HelixForm>(a, sweep, lds); }
  else                 { if (a.rotation) go<true, TableRouting>(a, sweep, lds); else go<false, TableRouting>(a, sweep, lds); }
}
#else
#if TRK_INST_KIND == 1
template <bool ROT, bool WR>
static void go(const FkLaunch &a) {
  const unsigned grid = (unsigned)((a.n + 63) / 64);
  hipLaunchKernelGGL((fk_rk4_batch_retract<TRK_INST_N, ROT, WR>), dim3(grid), dim3(64), 0, a.stream, a.d_states, a.n, a.ld, a.K,
                     a.d_poly, a.d_tab, a.d_steps, a.n_steps, a.k_first, a.d_tgrid, a.d_hl, a.out, a.d_perm, a.d_wave_k_begin);
}
template <> void launch_fk_retract<TRK_INST_N>(const FkLaunch &a) {
#else
template <bool ROT, bool WR>
static void go(const FkLaunch &a) {
  const unsigned grid = (unsigned)((a.n + 63) / 64);
  if (helix_form(a.K))
    hipLaunchKernelGGL((fk_rk4_batch_uniform<TRK_INST_N, ROT, WR, HelixForm>), dim3(grid), dim3(64), 0, a.stream, a.d_states, a.n, a.ld, a.K,
                       a.d_tab, a.d_steps, a.n_steps, a.out);
  else
    hipLaunchKernelGGL((fk_rk4_batch_uniform<TRK_INST_N, ROT, WR>), dim3(grid), dim3(64), 0, a.stream, a.d_states, a.n, a.ld, a.K,
                       a.d_tab, a.d_steps, a.n_steps, a.out);
}
template <> void launch_fk_uniform<TRK_INST_N>(const FkLaunch &a) {
#endif
  if (a.rotation) { if (a.write_R) go<true, true>(a); else go<true, false>(a); }
  else            { if (a.write_R) go<false, true>(a); else go<false, false>(a); }
}
#endif

}  // namespace trk
