// fk_loaded_lin_kernel.hpp -- the linearisation launch of the loaded tip IK (loaded_ik_host.inc): per round and active problem
// 13 + 2 S integrations of the loaded rod from one point, whose central differences give the four blocks of the implicit-function
// tip Jacobian dx/dp = X_p - X_y J_y^-1 J_p (loaded_ik_kernel.hpp: ikl_lm_step).
//
// fk_loaded_lin is fk_loaded_uniform's loop and tip balance (fk_loaded_kernel.hpp) with three differences: the lane applies its own
// perturbation to one base strain or one state entry of its row (LinIn, fk_lin_launch.hpp); no backbone point is stored; the tip
// after rotate_z is written beside the 6 residuals, as [9][ldr] planes.  With the load set fixed in the world frame a lane turns
// the set by Rz(-theta) of its own, possibly perturbed, rotation through edge_sincos -- the operation sequence of
// loaded_sample_loads, so the host can restate the rows bit for bit (Engine.sample_loads).  A problem's lanes may lie in two
// waves: no lane looks at another.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "fk_lin_launch.hpp"
#include "edge_sincos.hpp"
#define TRK_LOADED_WITH_INTEGRATOR
#include "fk_loaded_kernel.hpp"

namespace trk {

// ik_step_size's rule (ik_kernel.hpp): np.maximum(|1e-4 z|, delta)
__device__ __forceinline__ double lin_step_size(double z, double delta) {
#pragma clang fp contract(off)
  const double a = fabs(1e-4 * z);
  return a < delta ? delta : a;
}

template <int N, bool ROT>
__global__ __launch_bounds__(64, (N <= TRK_K1_TWO_WAVE_MAXN ? 2 : 1)) void fk_loaded_lin(
    int64_t n, RobotK K, const double *__restrict__ tab, const StepK *__restrict__ steps, int nsteps, LinIn in) {
#define TRK_STAGE_ROW TRK_STAGE_ROW_CONSTANT
#include "fk_loaded_lin_body.inc"
#undef TRK_STAGE_ROW
}

// the same under a load profile (in.weights, never null here): the weight applies to the lane's row after its own world-frame turn
template <int N, bool ROT>
__global__ __launch_bounds__(64, (N <= TRK_K1_TWO_WAVE_MAXN ? 2 : 1)) void fk_loaded_lin_profile(
    int64_t n, RobotK K, const double *__restrict__ tab, const StepK *__restrict__ steps, int nsteps, LinIn in) {
#define TRK_STAGE_ROW TRK_STAGE_ROW_PROFILE
#include "fk_loaded_lin_body.inc"
#undef TRK_STAGE_ROW
}

}  // namespace trk
