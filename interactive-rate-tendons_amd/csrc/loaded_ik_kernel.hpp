// loaded_ik_kernel.hpp -- the per-problem kernels of tip inverse kinematics on LOADED shapes (tr_ik_loaded_batch*,
// loaded_ik_host.inc): tip_control::inverse_kinematics with TendonRobot::general_shape as its FK.
//
// The tip of the loaded rod is x(y, p) at base strains y = (v0, u0) that balance the tip, e_w(y, p) = 0.  At such an equilibrium
// the tip moves with the state as dx/dp = X_p - X_y J_y^-1 J_p (J_y = de_w/dy, J_p = de_w/dp, X_y = dx/dy, X_p = dx/dp): the four
// blocks are central differences of 13 + 2 S integrations from one point (fk_loaded_lin_kernel.hpp), none of them a shooting
// solve.  Per round of the host loop and still-active problem:
//   ikl_gather    the trial state, its load rows (frame WORLD: turned by Rz(-theta) of the trial state, loaded_sample_loads' sequence)
//                 and the predicted strains y - W (p_trial - p), W = J_y^-1 J_p, in list order: the input of the shooting
//   (shooting)    loaded_host.inc's rounds on those rows from that guess
//   fk_loaded_lin the 13 + 2 S lanes at the equilibrated trial
//   ikl_lm_step   one lane per problem: LU of J_y with partial pivoting in registers; one Newton step on the trial's strains and
//                 tip with it (the shooting stops at the threshold, not at the equilibrium); accept / reject on |des - x|^2 (a
//                 trial whose shooting did not converge is rejected); when accepted the new W and reduced Jacobian J_r, column by
//                 column over the state; ik_lm_step's stop tests and damped step, the next trial point and the next active list
// The strain steps of J_y and X_y are the shooting's finite_difference_delta itself, not levmar's max(|1e-4 y|, delta): see
// ikl_lm_step.
// The LU, the Cholesky solve and the outer iteration's bookkeeping are lm_dense.hpp's, shared with ik_lm_step and loaded_tip_sens.
// The scheme is tests/loaded_ik_reference.py's, which is the specification.  Compiled without contraction, as ik_kernel.hpp is.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ik_kernel.hpp"
#include "edge_sincos.hpp"

namespace trk {

struct IklLoads { double wrench[6], dist[6]; int32_t world, pad_; };

// per-problem state, problem-indexed (one chunk of problems)
struct IklState {
  double *p;        // [n][S] the accepted point
  double *pn;       // [n][S] the trial point (first round: the clipped start)
  double *y;        // [n][6] base strains of the accepted point's equilibrium
  double *W;        // [n][6][S] J_y^-1 J_p at the accepted point
  double *J;        // [n][3][S] the reduced tip Jacobian at the accepted point
  double *f;        // [n][3] tip at the accepted point
  double *des;      // [n][3]
  double *err2, *mu, *nu;   // [n]
  int32_t *iters, *calls;   // [n]
  uint8_t *eq;      // [n] the start reached an equilibrium
};

// the rows of one round, in list order
struct IklRows {
  double *states;   // [m][S]
  double *wrench, *dist, *guess;   // [m][6]
  double *vu;       // [m][6] the shooting's strains
  uint8_t *conv;    // [m] the shooting converged
  int32_t *calls;   // [m] its integrations
};

// rows of the m listed problems (list null: problems 0 .. m-1, the first round, whose guess rows are the caller's or unused)
__global__ void ikl_gather(IkParams prm, IklState st, const int32_t *__restrict__ list, int64_t m, IklLoads ld,
                           const double *__restrict__ start_guess, IklRows rows) {
#pragma clang fp contract(off)
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= m) return;
  const int64_t i = list ? (int64_t)list[r] : r;
  const int S = prm.S;
  for (int j = 0; j < S; j++) rows.states[r * S + j] = st.pn[i * S + j];
  if (ld.world && prm.rot_index >= 0) {
    double s, c;
    edge_sincos(st.pn[i * S + prm.rot_index], s, c);
    edge_turn_row(ld.wrench, s, c, rows.wrench + r * 6);
    edge_turn_row(ld.dist, s, c, rows.dist + r * 6);
  } else {
    for (int q = 0; q < 6; q++) { rows.wrench[r * 6 + q] = ld.wrench[q]; rows.dist[r * 6 + q] = ld.dist[q]; }
  }
  if (!list) {
    if (start_guess) for (int q = 0; q < 6; q++) rows.guess[r * 6 + q] = start_guess[i * 6 + q];
    return;
  }
  // the predictor: y - W (p_trial - p)
  for (int a = 0; a < 6; a++) {
    double s = 0.0;
    for (int k = 0; k < S; k++) s += st.W[(i * 6 + a) * S + k] * (st.pn[i * S + k] - st.p[i * S + k]);
    rows.guess[r * 6 + a] = st.y[i * 6 + a] - s;
  }
}

// One outer LM iteration of every listed problem (list null: problems 0 .. m-1, the first round).  lin: [9][ldr] planes of the
// round's linearisation launch, lane r (13 + 2 S) + q (fk_lin_launch.hpp: LinIn).
template <int S>
__global__ __launch_bounds__(64) void ikl_lm_step(IkParams prm, double delta_y, IklState st, const int32_t *__restrict__ list, int64_t m,
                                                  const double *__restrict__ lin, int64_t ldr, IklRows rows, int init,
                                                  int32_t *__restrict__ next_list, uint32_t *__restrict__ next_count) {
#pragma clang fp contract(off)
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= m) return;
  const int64_t i = list ? (int64_t)list[r] : r;
  constexpr int Q = 13 + 2 * S;
  const double *__restrict__ row = lin + r * Q;              // row[plane * ldr + q]
  const bool conv = rows.conv[r] != 0;
  double x[S], p[S], J[3 * S], f[3], e[3], des[3], g[S];
#pragma unroll
  for (int j = 0; j < S; j++) x[j] = st.pn[i * S + j];
#pragma unroll
  for (int k = 0; k < 3; k++) des[k] = st.des[i * 3 + k];
  // J_y and X_y of the trial point: central differences with the shooting's absolute step (a step relative to the strain, levmar's
  // 1e-4 |y_j|, is 1e-4 for v_3 ~ 1, and the moment balance is curved enough in v_3 to put 2e-4 of truncation into J_y)
  double A[36], Xy[18];
  {
    const double sc = 0.5 / delta_y;
#pragma unroll
    for (int j = 0; j < 6; j++) {
#pragma unroll
      for (int k = 0; k < 6; k++) A[k * 6 + j] = (row[k * ldr + 2 + 2 * j] - row[k * ldr + 1 + 2 * j]) * sc;
#pragma unroll
      for (int k = 0; k < 3; k++) Xy[k * 6 + j] = (row[(6 + k) * ldr + 2 + 2 * j] - row[(6 + k) * ldr + 1 + 2 * j]) * sc;
    }
  }
  // P A = L U in place (unit L below the diagonal); piv[c]: the row exchanged with row c.  A zero pivot leaves inf / NaN in what is
  // solved with it: the trial is then not accepted, or (W, J_r) make the next damped matrix indefinite, which ends the problem.
  int piv[6];
  lu6_factor(A, piv);
  // The shooting stops at |e_w| <= residual_threshold, which leaves the tip up to ~1e-5 m from the equilibrium's.  One Newton step
  // on the strains, dy = -J_y^-1 e_w, costs nothing here: the trial's strains become y + dy and its tip x + X_y dy.
  double yn[6], fn[3], en[3];
  {
    double b[6];
#pragma unroll
    for (int a = 0; a < 6; a++) b[a] = row[a * ldr];
    lu6_solve(A, piv, b);
#pragma unroll
    for (int a = 0; a < 6; a++) yn[a] = rows.vu[r * 6 + a] - b[a];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      double t = 0.0;
#pragma unroll
      for (int a = 0; a < 6; a++) t += Xy[k * 6 + a] * b[a];
      fn[k] = row[(6 + k) * ldr] - t;
      en[k] = des[k] - fn[k];
    }
  }
  const double err2n = en[0] * en[0] + en[1] * en[1] + en[2] * en[2];
  double err2, mu, nu;
  int iters;
  const int calls = (init ? 0 : st.calls[i]) + rows.calls[r] + Q;
  bool active, accepted;
  // J_r = X_p - X_y J_y^-1 J_p of the trial point into J, W = J_y^-1 J_p into the problem's row
  auto reduce = [&]() {
#pragma unroll
    for (int k = 0; k < S; k++) {
      const double sc = 0.5 / ik_step_size(x[k], prm.delta);
      double b[6];
#pragma unroll
      for (int a = 0; a < 6; a++) b[a] = (row[a * ldr + 14 + 2 * k] - row[a * ldr + 13 + 2 * k]) * sc;
      lu6_solve(A, piv, b);
#pragma unroll
      for (int a = 0; a < 6; a++) st.W[(i * 6 + a) * S + k] = b[a];
#pragma unroll
      for (int q = 0; q < 3; q++) {
        double s = 0.0;
#pragma unroll
        for (int a = 0; a < 6; a++) s += Xy[q * 6 + a] * b[a];
        J[q * S + k] = (row[(6 + q) * ldr + 14 + 2 * k] - row[(6 + q) * ldr + 13 + 2 * k]) * sc - s;
      }
    }
  };
  auto take_trial = [&]() {
#pragma unroll
    for (int j = 0; j < S; j++) p[j] = x[j];
#pragma unroll
    for (int k = 0; k < 3; k++) { f[k] = fn[k]; e[k] = en[k]; }
    err2 = err2n;
    reduce();
    lm_grad<S>(J, e, g);
  };
  if (init) {
    nu = 2.0;
    iters = 0;
#pragma unroll
    for (int a = 0; a < 6; a++) st.y[i * 6 + a] = yn[a];
    st.eq[i] = conv ? 1 : 0;
    if (!conv) {                                    // no equilibrium at the start: the problem ends here, error = inf
      const double nan = __builtin_nan("");
#pragma unroll
      for (int j = 0; j < S; j++) st.p[i * S + j] = x[j];
#pragma unroll
      for (int k = 0; k < 3; k++) st.f[i * 3 + k] = nan;
      st.err2[i] = __builtin_inf();
      st.mu[i] = prm.mu_init; st.nu[i] = nu; st.iters[i] = 0; st.calls[i] = calls;
      return;
    }
    accepted = true;
    take_trial();
    double dmax = 0.0;                              // mu = mu_init * max diag(J^T J), or mu_init when that is not positive
#pragma unroll
    for (int j = 0; j < S; j++) {
      const double a = J[0 * S + j] * J[0 * S + j] + J[1 * S + j] * J[1 * S + j] + J[2 * S + j] * J[2 * S + j];
      if (!(a <= dmax)) dmax = a;
    }
    mu = prm.mu_init * dmax;
    if (!(mu > 0.0)) mu = prm.mu_init;
    active = err2 > prm.eps3_sq && lm_moving<S>(p, g, prm);
  } else {
#pragma unroll
    for (int j = 0; j < S; j++) p[j] = st.p[i * S + j];
#pragma unroll
    for (int q = 0; q < 3 * S; q++) J[q] = st.J[i * 3 * S + q];
#pragma unroll
    for (int k = 0; k < 3; k++) { f[k] = st.f[i * 3 + k]; e[k] = des[k] - f[k]; }
    err2 = st.err2[i]; mu = st.mu[i]; nu = st.nu[i]; iters = st.iters[i];
    lm_grad<S>(J, e, g);
    const double rho = lm_gain_ratio<S>(x, p, g, mu, err2, err2n);
    accepted = conv && rho > 0.0;
    if (accepted) {
      take_trial();
#pragma unroll
      for (int a = 0; a < 6; a++) st.y[i * 6 + a] = yn[a];
      const double t = 2.0 * rho - 1.0;
      mu *= lm_shrink(t * t * t);
      nu = 2.0;
      active = err2 > prm.eps3_sq && lm_moving<S>(p, g, prm);
    } else {
      lm_reject(mu, nu);
      active = isfinite(mu) && mu < 1e300;
    }
  }
  if (accepted) {
#pragma unroll
    for (int j = 0; j < S; j++) st.p[i * S + j] = p[j];
#pragma unroll
    for (int q = 0; q < 3 * S; q++) st.J[i * 3 * S + q] = J[q];
#pragma unroll
    for (int k = 0; k < 3; k++) st.f[i * 3 + k] = f[k];
    st.err2[i] = err2;
  }
  if (active && iters < prm.max_iters) {
    // the damped normal equations (J^T J + mu I) dp = J^T e: Cholesky of the packed lower triangle, in registers (ik_lm_step's)
    double A[S * (S + 1) / 2];
#pragma unroll
    for (int a = 0; a < S; a++) {
#pragma unroll
      for (int b = 0; b <= a; b++)
        A[a * (a + 1) / 2 + b] = J[0 * S + a] * J[0 * S + b] + J[1 * S + a] * J[1 * S + b] + J[2 * S + a] * J[2 * S + b] + (a == b ? mu : 0.0);
    }
    double y[S];
    const bool spd = chol_solve_packed<S>(A, g, y);
    // projected onto the box; the relative-step test on the step actually taken
    double dd = 0.0, pp = 0.0;
#pragma unroll
    for (int j = 0; j < S; j++) {
      const double pn = ik_clip(p[j] + y[j], prm.lo[j], prm.hi[j]);
      const double dpe = pn - p[j];
      dd += dpe * dpe;
      pp += p[j] * p[j];
      x[j] = pn;
    }
    iters++;
    // a matrix that is not positive definite (mu overflowed, inf / NaN in J) ends the problem, as the mu-overflow stop does
    const bool small = !spd || !(dd > prm.eps2_sq * pp);
    if (!small) {
#pragma unroll
      for (int j = 0; j < S; j++) st.pn[i * S + j] = x[j];
      next_list[atomicAdd(next_count, 1u)] = (int32_t)i;
    }
  }
  st.mu[i] = mu; st.nu[i] = nu; st.iters[i] = iters; st.calls[i] = calls;
}

// results of a chunk (any output may be null): state with the rotation canonical, tip, error (inf without an equilibrium at the
// start), outer iterations, integrations, the base strains of the returned state's equilibrium, the equilibrium flag
__global__ void ikl_finish(IkParams prm, IklState st, int64_t n, double *__restrict__ states, double *__restrict__ tips,
                           double *__restrict__ error, int32_t *__restrict__ iters, int32_t *__restrict__ calls, double *__restrict__ vu0,
                           uint8_t *__restrict__ eq) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  lm_write_result(prm, i, st.p, st.f, st.err2, st.iters, st.calls, states, tips, error, iters, calls);
  if (vu0) for (int a = 0; a < 6; a++) vu0[i * 6 + a] = st.y[i * 6 + a];
  if (eq) eq[i] = st.eq[i];
}

}  // namespace trk
