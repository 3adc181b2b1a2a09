// fk_lin_launch.hpp -- host-side launch interface of the linearisation kernel of the loaded IK (fk_loaded_lin_kernel.hpp).  As with K1
// (fk_launch.hpp) every tendon count is its own translation unit (fk_lin_inst.hip compiled with -DTRK_INST_N=..); tendon_hip.hip only
// sees this declaration.  The units are files of their own so that the 56 units of fk_inst.hip keep their dependencies.
#pragma once
#include "fk_launch.hpp"

namespace trk {

// Lane t of the launch belongs to row t / Q of the round (q = t % Q): q = 0 the row's point, q = 1 + 2j / 2 + 2j its base strain j
// moved by -+ delta_y, q = 13 + 2k / 14 + 2k its state entry k moved by -+ max(|1e-4 p_k|, delta_p).
struct LinIn {
  const double *states;                        // [rows][S] the trial states of the round
  const double *vu;                            // [rows][6] their equilibrated base strains (v0, u0)
  double wrench[6], dist[6];                   // the call's one load set
  int32_t world;                               // 1: the set is fixed behind rotate_z -- every lane turns it by Rz(-theta) of ITS theta
  int32_t Q;                                   // 13 + 2 S
  double delta_y, delta_p;                     // finite_difference_delta of the shooting and of the IK
  const double *tip_route;                     // [N][6] routing at s = L
  double *out; int64_t ldr;                    // [9][ldr]: 6 residual planes, then 3 planes of the tip after rotate_z
  const double *weights = nullptr;             // the load profile's table (fk_launch.hpp: LoadedIn::weights); null: none
};

// a.n lanes; of `a` the kernel reads n, K, rotation, d_tab, d_steps, n_steps and stream
// (in.weights null: fk_loaded_lin; else fk_loaded_lin_profile, compiled from fk_lin_inst.hip with -DTRK_LIN_PROFILE into objects of
// its own)
template <int N> void launch_fk_loaded_lin(const FkLaunch &a, const LinIn &in);
template <int N> void launch_fk_loaded_lin_profile(const FkLaunch &a, const LinIn &in);

#define TRK_DECL_LIN(N) template <> void launch_fk_loaded_lin<N>(const FkLaunch &, const LinIn &); \
  template <> void launch_fk_loaded_lin_profile<N>(const FkLaunch &, const LinIn &);
TRK_DECL_LIN(1) TRK_DECL_LIN(2) TRK_DECL_LIN(3) TRK_DECL_LIN(4) TRK_DECL_LIN(5) TRK_DECL_LIN(6) TRK_DECL_LIN(7) TRK_DECL_LIN(8)
#undef TRK_DECL_LIN

}  // namespace trk
