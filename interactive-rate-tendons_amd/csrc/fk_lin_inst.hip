// fk_lin_inst.hip -- the linearisation kernel of the loaded IK, one object per tendon count: compiled with -DTRK_INST_N=<1..8>,
// and once more with -DTRK_LIN_PROFILE for its form under a load profile (see _lib.py: build()).
#include "fk_lin_launch.hpp"
#include "fk_loaded_lin_kernel.hpp"

namespace trk {

#ifdef TRK_LIN_PROFILE
template <> void launch_fk_loaded_lin_profile<TRK_INST_N>(const FkLaunch &a, const LinIn &in) {
  const unsigned grid = (unsigned)((a.n + 63) / 64);
  if (a.rotation)
    hipLaunchKernelGGL((fk_loaded_lin_profile<TRK_INST_N, true>), dim3(grid), dim3(64), 0, a.stream, a.n, a.K, a.d_tab, a.d_steps, a.n_steps, in);
  else
    hipLaunchKernelGGL((fk_loaded_lin_profile<TRK_INST_N, false>), dim3(grid), dim3(64), 0, a.stream, a.n, a.K, a.d_tab, a.d_steps, a.n_steps, in);
}
#else
template <> void launch_fk_loaded_lin<TRK_INST_N>(const FkLaunch &a, const LinIn &in) {
  if (in.weights) return launch_fk_loaded_lin_profile<TRK_INST_N>(a, in);
  const unsigned grid = (unsigned)((a.n + 63) / 64);
  if (a.rotation)
    hipLaunchKernelGGL((fk_loaded_lin<TRK_INST_N, true>), dim3(grid), dim3(64), 0, a.stream, a.n, a.K, a.d_tab, a.d_steps, a.n_steps, in);
  else
    hipLaunchKernelGGL((fk_loaded_lin<TRK_INST_N, false>), dim3(grid), dim3(64), 0, a.stream, a.n, a.K, a.d_tab, a.d_steps, a.n_steps, in);
}
#endif

}  // namespace trk
