// fk_loaded_kernel.hpp -- the loaded forward kinematics: TendonRobot::general_tension_shape (tendon/TendonRobot.cpp:689-952) for a
// batch.  The rod carries a tip wrench (F_e, L_e) and a distributed load (f_e, l_e) per unit length besides its tendons; the
// shape is the solution of a boundary-value problem, found by single shooting on the base strains (v0, u0).
//
//   fk_loaded_uniform  one lane integrates the rod from given base strains (K1's RK4 loop on the shared routing table, the
//                      right-hand side with the two load terms of tendon_deriv's loaded overload, tendon_deriv.cpp:331-332) and
//                      evaluates the tip residual e = (F_e_est - F_e, L_e_est - L_e) in-lane (PointForces::calc_point_forces at the
//                      tip, TendonRobot.cpp:188-217,785-812); stores 6 residual doubles per lane and / or K1's outputs
//   shoot_start        the start of every problem: the caller's guess, or the unloaded solution of its tensions (K1's
//                      initial_bending) -- exact at zero load, where the reference's straight rod (e3, 0) is not
//   shoot_begin        the residual of the start; a problem that meets the threshold there is done with zero iterations
//   shoot_lm_step      one Levenberg-Marquardt iteration per active problem from the 13 residual rows of its trial point and the
//                      point's 12 central-difference neighbours (ik_expand's layout, ik_kernel.hpp): J, gain ratio, accept / reject,
//                      the stop tests, the step damped by mu diag(J^T J) (mu starts at mu_init) through a 6 x 6 Cholesky in
//                      registers, the next active list
//   shoot_finish       strains, |e|, counters and the converged flag of every problem
// The distributed load is a constant vector per problem in the robot's base frame (gravity), scaled by the context's load profile
// w(s) where one is installed (fk_loaded_profile); the reference takes functions of (t, p).
// Robots with retraction have an integrator of their own (fk_loaded_retract_kernel.hpp: per-lane first interval, point count and
// tip-aligned rows) and share the per-problem kernels below, which never look at the grid.  The LM iteration is this library's own (the scheme of
// ik_lm_step without bounds; the Cholesky solve and the mu / nu updates are lm_dense.hpp's, whose header lists what differs), not
// levmar's code path; it is compiled without contraction.
// The file has two halves: the per-problem kernels (included by tendon_hip.hip), and, under TRK_LOADED_WITH_INTEGRATOR, the kernels that
// need the tendon count at compile time (fk_inst.hip, kind 6: one object per tendon count).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#ifndef TRK_LOADED_WITH_INTEGRATOR
#include "ik_kernel.hpp"

namespace trk {

constexpr int kShootQ = 13;          // lanes per problem in a round: the trial point, then -d_j e_j, +d_j e_j for j = 0 .. 5

struct ShootParams {
  int32_t max_iters, pad_;
  double delta;                      // finite_difference_delta
  double mu_init, eps1, eps2_sq, eps3_sq;   // mu_init, |J^T e|_inf, |Dp|^2 (relative), |e|^2 (residual_threshold^2)
};

// per-problem state of one chunk
struct ShootState {
  double *p;        // [n][6] the accepted strains (v0, u0)
  double *pn;       // [n][6] the trial point (first: the start)
  double *e;        // [n][6] residual at p
  double *J;        // [n][6][6] d e / d (v0, u0) at p
  double *err2, *mu, *nu;      // [n]; mu < 0: the problem has no Jacobian yet
  int32_t *iters, *calls;      // [n]
};

__device__ __forceinline__ bool shoot_finite(double x) { return x - x == 0.0; }

// D_jj = (J^T J)_jj, or 1 where that is not positive
__device__ __forceinline__ double shoot_scale(const double (&J)[36], int j) {
#pragma clang fp contract(off)
  double a = 0.0;
#pragma unroll
  for (int k = 0; k < 6; k++) a += J[k * 6 + j] * J[k * 6 + j];
  return a > 0.0 ? a : 1.0;
}

// res: [6][ldr] residual rows of a one-lane-per-problem launch at the start strains st.pn
__global__ void shoot_begin(ShootParams prm, ShootState st, int64_t m, const double *__restrict__ res, int64_t ldr,
                            int32_t *__restrict__ next_list, uint32_t *__restrict__ next_count) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  double err2 = 0.0;
  for (int k = 0; k < 6; k++) {
    const double e = res[k * ldr + i];
    st.e[i * 6 + k] = e;
    err2 += e * e;
    st.p[i * 6 + k] = st.pn[i * 6 + k];
  }
  st.err2[i] = err2; st.mu[i] = -1.0; st.nu[i] = 2.0; st.iters[i] = 0; st.calls[i] = 1;
  if (shoot_finite(err2) && err2 > prm.eps3_sq && prm.max_iters > 0) next_list[atomicAdd(next_count, 1u)] = (int32_t)i;
}

// One LM iteration of every listed problem.  res: [6][ldr], lane r * 13 + q of the round's launch is problem list[r]'s trial
// point (q = 0) or its neighbour (q = 1 + 2j: -d_j, q = 2 + 2j: +d_j).
__global__ __launch_bounds__(64) void shoot_lm_step(ShootParams prm, ShootState st, const int32_t *__restrict__ list, int64_t m,
                                                    const double *__restrict__ res, int64_t ldr, int32_t *__restrict__ next_list,
                                                    uint32_t *__restrict__ next_count) {
#pragma clang fp contract(off)
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= m) return;
  const int64_t i = (int64_t)list[r];
  const double *__restrict__ row = res + r * kShootQ;       // row[k * ldr + q]
  double x[6], p[6], e[6], J[36], g[6];
#pragma unroll
  for (int j = 0; j < 6; j++) x[j] = st.pn[i * 6 + j];
  double en[6], err2n = 0.0;
#pragma unroll
  for (int k = 0; k < 6; k++) { en[k] = row[k * ldr]; err2n += en[k] * en[k]; }
  // J(x)[k][j] = (e(x + d_j e_j) - e(x - d_j e_j))_k * (0.5 / d_j)
  auto jac_from_rows = [&]() {
#pragma unroll
    for (int j = 0; j < 6; j++) {
      const double sc = 0.5 / ik_step_size(x[j], prm.delta);
#pragma unroll
      for (int k = 0; k < 6; k++) J[k * 6 + j] = (row[k * ldr + 2 + 2 * j] - row[k * ldr + 1 + 2 * j]) * sc;
    }
  };
  // g = -J^T e: the right-hand side of the normal equations
  auto grad = [&]() {
#pragma unroll
    for (int j = 0; j < 6; j++) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < 6; k++) s += J[k * 6 + j] * e[k];
      g[j] = -s;
    }
  };
  auto moving = [&]() {
    double mx = 0.0;
#pragma unroll
    for (int j = 0; j < 6; j++) { const double a = fabs(g[j]); if (!(a <= mx)) mx = a; }     // a NaN wins
    return mx > prm.eps1;
  };
  double err2, mu = st.mu[i], nu = st.nu[i];
  const bool last = nu < 0.0;                        // the step to this trial point was small: evaluate it, then stop
  if (last) nu = -nu;
  int iters = st.iters[i];
  const int calls = st.calls[i] + kShootQ;
  bool active, accepted;
  if (mu < 0.0) {                                    // the start: its residual is known (shoot_begin), its Jacobian is not
    accepted = true;
#pragma unroll
    for (int j = 0; j < 6; j++) { p[j] = x[j]; e[j] = en[j]; }
    err2 = err2n;
    jac_from_rows();
    grad();
    mu = prm.mu_init;                                // relative to diag(J^T J): see the step below
    nu = 2.0;
    active = shoot_finite(err2) && err2 > prm.eps3_sq && moving();
  } else {
#pragma unroll
    for (int j = 0; j < 6; j++) { p[j] = st.p[i * 6 + j]; e[j] = st.e[i * 6 + j]; }
#pragma unroll
    for (int q = 0; q < 36; q++) J[q] = st.J[i * 36 + q];
    err2 = st.err2[i];
    grad();
    // gain ratio of the step dp = x - p against the model's predicted decrease dp . (mu D dp + g), D = diag(J^T J)
    double pred = 0.0;
#pragma unroll
    for (int j = 0; j < 6; j++) {
      const double dp = x[j] - p[j];
      pred += dp * (mu * shoot_scale(J, j) * dp + g[j]);
    }
    const double rho = pred > 0.0 ? (err2 - err2n) / pred : -1.0;
    accepted = rho > 0.0;                            // (a non-finite trial residual makes rho NaN: not accepted)
    if (accepted) {
#pragma unroll
      for (int j = 0; j < 6; j++) { p[j] = x[j]; e[j] = en[j]; }
      err2 = err2n;
      jac_from_rows();
      grad();
      const double t = 2.0 * rho - 1.0;
      mu *= lm_shrink(t * t * t);
      nu = 2.0;
      active = err2 > prm.eps3_sq && moving();
    } else {
      lm_reject(mu, nu);
      active = shoot_finite(err2n) && shoot_finite(mu) && mu < 1e300;     // a non-finite residual ends the problem (levmar's reason 7)
    }
  }
  if (accepted) {
#pragma unroll
    for (int j = 0; j < 6; j++) { st.p[i * 6 + j] = p[j]; st.e[i * 6 + j] = e[j]; }
#pragma unroll
    for (int q = 0; q < 36; q++) st.J[i * 36 + q] = J[q];
    st.err2[i] = err2;
  }
  if (last) active = false;
  if (active && iters < prm.max_iters) {
    // the damped normal equations (J^T J + mu D) dp = -J^T e, D = diag(J^T J) (Marquardt's scaling: the unknowns are strains and
    // curvatures, the residuals forces and moments -- diag(J^T J) spans nine decades, and a multiple of the identity that damps the
    // stiffest direction freezes the bending ones); Cholesky of the packed lower triangle, in registers
    double A[21];
#pragma unroll
    for (int a = 0; a < 6; a++) {
#pragma unroll
      for (int b = 0; b <= a; b++) {
        double s = a == b ? mu * shoot_scale(J, a) : 0.0;
#pragma unroll
        for (int k = 0; k < 6; k++) s += J[k * 6 + a] * J[k * 6 + b];
        A[a * (a + 1) / 2 + b] = s;
      }
    }
    double y[6];
    const bool spd = chol_solve_packed<6>(A, g, y);
    double dd = 0.0, pp = 0.0;
#pragma unroll
    for (int j = 0; j < 6; j++) { dd += y[j] * y[j]; pp += p[j] * p[j]; x[j] = p[j] + y[j]; }
    iters++;
    // A matrix that is not positive definite (mu overflowed, NaN in J) ends the problem, as the mu-overflow stop does.  A step with
    // |Dp| <= eps2 |p| is the problem's last: it is still evaluated (the rod is soft -- 1e-4 in a curvature is 1e-5 N at the tip,
    // twice residual_threshold -- so the step that stop test judges small is often the one that reaches the threshold), then the
    // problem ends whatever the residual, converged or not by the first test alone.
    if (spd) {
      if (!(dd > prm.eps2_sq * pp)) nu = -nu;
#pragma unroll
      for (int j = 0; j < 6; j++) st.pn[i * 6 + j] = x[j];
      next_list[atomicAdd(next_count, 1u)] = (int32_t)i;
    }
  }
  st.mu[i] = mu; st.nu[i] = nu; st.iters[i] = iters; st.calls[i] = calls;
}

// results of a chunk (any output may be null); converged: |e| <= residual_threshold at the accepted strains.  perm (a robot with
// retraction solved in backbone-length order, loaded_host.inc: shoot_run): problem i's results go to row perm[i] of the outputs
__global__ void shoot_finish(ShootParams prm, ShootState st, int64_t n, double *__restrict__ vu0, double *__restrict__ residual,
                             int32_t *__restrict__ iters, int32_t *__restrict__ fk_calls, uint8_t *__restrict__ converged,
                             const int32_t *__restrict__ perm) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t o = perm ? (int64_t)perm[i] : i;
  if (vu0) for (int j = 0; j < 6; j++) vu0[o * 6 + j] = st.p[i * 6 + j];
  const double err2 = st.err2[i];
  if (residual) residual[o] = sqrt(err2);
  if (iters) iters[o] = st.iters[i];
  if (fk_calls) fk_calls[o] = st.calls[i];
  if (converged) converged[o] = err2 <= prm.eps3_sq ? 1 : 0;
}

// A robot with retraction: a problem whose s_start is negative lies outside the state space's bounds and integrates nothing (its
// residual row is zero); it is reported unconverged, as the unloaded kernels report it (fk_retract_kernel.hpp).
__global__ void shoot_negative_start(const double *__restrict__ states, int S, int64_t n, uint8_t *__restrict__ converged,
                                     const int32_t *__restrict__ perm) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t o = perm ? (int64_t)perm[i] : i;       // (perm: the chunk's problems as rows of the caller's arrays)
  if (states[o * S + S - 1] < 0.0) converged[o] = 0;
}

}  // namespace trk

#else  // TRK_LOADED_WITH_INTEGRATOR
#include "fk_launch.hpp"
#include "fk_kernel.hpp"

namespace trk {

// The distributed load of one stage in the body frame: c -= R^T l_e, d -= R^T f_e
struct BodyLoad {
  double f[3], l[3];
  __device__ __forceinline__ void operator()(double &cx, double &cy, double &cz, double &dx, double &dy, double &dz) const {
    cx -= l[0]; cy -= l[1]; cz -= l[2];
    dx -= f[0]; dy -= f[1]; dz -= f[2];
  }
};

template <int N>
__global__ __launch_bounds__(64) void shoot_start(const double *__restrict__ states, int64_t n, RobotK K, const double *__restrict__ tab,
                                                  const double *__restrict__ guess, double *__restrict__ vu) {
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
  const bool live = i < n;
  const int64_t il = live ? i : (n - 1);       // tail lanes repeat the last problem (initial_bending votes across the wave)
  double v[3], u[3];
  if (guess) {
#pragma unroll
    for (int q = 0; q < 3; q++) { v[q] = guess[il * 6 + q]; u[q] = guess[il * 6 + 3 + q]; }
  } else {
    double tau[N];
#pragma unroll
    for (int j = 0; j < N; j++) tau[j] = states[il * K.state_size + j];
    bool conv;
    initial_bending<N>(tau, tab, K, v, u, conv);
  }
  if (live) {
#pragma unroll
    for (int q = 0; q < 3; q++) { vu[i * 6 + q] = v[q]; vu[i * 6 + 3 + q] = u[q]; }
  }
}

// The row (f_e, l_e) a stage of the RK4 loop sees, before the stage's frame turns it into the body.  The two integrators' bodies
// (fk_loaded_body.inc, fk_loaded_lin_body.inc) are compiled once per form; TRK_STAGE_ROW(entry, fs, ls) names the stage's row fs, ls,
// `entry` being the stage's entry of the routing table (1 + 3 k at t_k, + 1 at t_k + h / 2, + 2 at t_k + h).
//   constant   the problem's row as it is
//   profile    the row times the load profile's weight at the stage's abscissa (tr_set_load_profile: the host's table of 1 + 3 nsteps
//              weights, indexed like the routing table).  The index is the same in every lane, so the weight arrives through a scalar
//              load, as the routing rows do.  Each product is rounded once and never fused into the rotation that follows: a constant
//              weight c is the row c * d of the host, bit for bit.
#define TRK_STAGE_ROW_CONSTANT(entry, fs, ls) const double (&fs)[3] = fe; const double (&ls)[3] = le;
#define TRK_STAGE_ROW_PROFILE(entry, fs, ls) double fs[3], ls[3]; profile_row(in.weights, (entry), fe, le, fs, ls);
__device__ __forceinline__ void profile_row(const double *__restrict__ w, int entry, const double (&fe)[3], const double (&le)[3],
                                            double (&f)[3], double (&l)[3]) {
#pragma clang fp contract(off)
  const double ws = w[entry];
#pragma unroll
  for (int q = 0; q < 3; q++) { f[q] = ws * fe[q]; l[q] = ws * le[q]; }
}

// The tip residual e = (F_e_est - F_e, L_e_est - L_e) of one lane from its tip frame R (column-major) and tip strains v, u:
// PointForces::calc_point_forces at the tip, every term in the base frame as the reference forms it: n = R K_se (v - e3),
// m = R K_bt u, F_t = sum -tau_i unit(R pd_i), L_t = sum (R r_i) x F_t,i.  rb: [N][6] the routing at s = L; wrench: the lane's row
// (F_e, L_e).  The tendon directions are normalised AFTER the rotation: the integrated frame is orthonormal to ~3e-9 only, and a unit
// vector rotated by it is that far from unit length -- 2e-7 N at 56 N of tension, which the balance of a converged problem
// (|e| <= 5e-6 N) would see.  Without contraction, whatever the caller compiles with.  The statements are those of the tip block of
// fk_loaded_body.inc, which keeps them inline: as a call the shared-grid kernels' register allocation moved (fk_loaded_profile<8> spilled
// 20 VGPRs where tests/test_load_profile_kernel_resources.py budgets 16); fk_loaded_retract (fk_loaded_retract_kernel.hpp) calls this.
template <int N>
__device__ __forceinline__ void tip_residual(const double (&R)[9], const double (&v)[3], const double (&u)[3], const double (&tau)[N],
                                             const RobotK &K, const double *__restrict__ rb, const double *__restrict__ wrench,
                                             double (&e)[6]) {
#pragma clang fp contract(off)
  auto rot = [&](double x, double y, double z, double (&o)[3]) {       // o = R (x, y, z)
#pragma unroll
    for (int r = 0; r < 3; r++) o[r] = R[0 + r] * x + R[3 + r] * y + R[6 + r] * z;
  };
  double Ft[3] = {0, 0, 0}, Lt[3] = {0, 0, 0};
#pragma unroll
  for (int k = 0; k < N; k++) {
    const double rx = rb[6 * k + 0], ry = rb[6 * k + 1], rdx = rb[6 * k + 2], rdy = rb[6 * k + 3];
    double pd[3], rw[3];
    rot((-u[2] * ry) + rdx + v[0], (u[2] * rx) + rdy + v[1], (u[0] * ry - u[1] * rx) + v[2], pd);
    rot(rx, ry, 0.0, rw);
    const double z = pd[0] * pd[0] + pd[1] * pd[1] + pd[2] * pd[2];
    if (z > 0.0) { const double s = sqrt(z); pd[0] = pd[0] / s; pd[1] = pd[1] / s; pd[2] = pd[2] / s; }
    const double fx = -tau[k] * pd[0], fy = -tau[k] * pd[1], fz = -tau[k] * pd[2];
    Ft[0] += fx; Ft[1] += fy; Ft[2] += fz;
    Lt[0] += rw[1] * fz - rw[2] * fy; Lt[1] += rw[2] * fx - rw[0] * fz; Lt[2] += rw[0] * fy - rw[1] * fx;
  }
  double nw[3], mw[3];
  rot(K.ks0 * v[0], K.ks0 * v[1], K.ks2 * (v[2] - 1.0), nw);
  rot(K.kb0 * u[0], K.kb0 * u[1], K.kb2 * u[2], mw);
#pragma unroll
  for (int r = 0; r < 3; r++) {
    e[r] = (nw[r] - Ft[r]) - wrench[r];
    e[3 + r] = (mw[r] - Lt[r]) - wrench[3 + r];
  }
}

// K1's loop (fk_kernel.hpp: fk_uniform_body) from given base strains, with the distributed load in the right-hand side and the tip
// residual behind it.  Lane t of n: problem in.list[t / in.Q] (list null: t / in.Q); outputs go to column t.  A problem's lanes may
// lie in two waves: no lane looks at another.
template <int N, bool ROT, bool WRITE_R>
__global__ __launch_bounds__(64, (N <= TRK_K1_TWO_WAVE_MAXN ? 2 : 1)) void fk_loaded_uniform(
    const double *__restrict__ states, int64_t n, int64_t ld, RobotK K,
    const double *__restrict__ tab, const StepK *__restrict__ steps, int nsteps, FkOut out, LoadedIn in) {
#define TRK_STAGE_ROW TRK_STAGE_ROW_CONSTANT
#include "fk_loaded_body.inc"
#undef TRK_STAGE_ROW
}

// the same under a load profile: the row of every stage is scaled by in.weights' entry of the stage (never null here)
template <int N, bool ROT, bool WRITE_R>
__global__ __launch_bounds__(64, (N <= TRK_K1_TWO_WAVE_MAXN ? 2 : 1)) void fk_loaded_profile(
    const double *__restrict__ states, int64_t n, int64_t ld, RobotK K,
    const double *__restrict__ tab, const StepK *__restrict__ steps, int nsteps, FkOut out, LoadedIn in) {
#define TRK_STAGE_ROW TRK_STAGE_ROW_PROFILE
#include "fk_loaded_body.inc"
#undef TRK_STAGE_ROW
}

}  // namespace trk
#endif
