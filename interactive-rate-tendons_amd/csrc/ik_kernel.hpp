// ik_kernel.hpp -- the tip Jacobian and batched tip inverse kinematics on the device (tip_control::inverse_kinematics,
// tip-control/tip_control.cpp:35-140; VoxelCachedLazyPRM::roadmapIk's IK leg, motion-planning/VoxelCachedLazyPRM.cpp:3164-3205).
//
// The FK is K1 itself (fk_rk4_batch_uniform / fk_rk4_batch_retract with only the tips stored): these kernels build its input
// and read its output.  Per round of the host loop (ik_host.inc):
//   ik_expand    trial point p of every active problem and its 2 S central-difference perturbations, problem-major:
//                lane r (2S+1) + q is p (q = 0), p - d_j e_j (q = 1 + 2j), p + d_j e_j (q = 2 + 2j); d_j = max(|1e-4 p_j|, delta)
//                (levmar's step, 3rdparty/levmar-2.6/misc_core.c:175-211) -- a problem's lanes are adjacent, so the retraction
//                kernel's length ordering sees near-equal backbones
//   K1           tips of those m (2S+1) lanes
//   ik_lm_step   one lane per problem: f and J through tip_control's FK wrapper, gain ratio, accept / reject, the stop tests, the
//                next damped step (S x S Cholesky in registers), the next trial point into the problem's row and the problem into
//                the next active list
// The step kernel's algebra and bookkeeping, the start kernel (lm_init) and the parameters (IkParams) are lm_dense.hpp's, shared
// with the loaded IK.
// The scheme is tip_control.inverse_kinematics_batch's (tip_control.py), which is the specification.  Everything here is
// compiled without contraction, so f, J and the perturbed states are the bits numpy forms from the same tips.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "lm_dense.hpp"

namespace trk {

// per-problem state, problem-indexed (one chunk of problems)
struct IkState {
  double *p;        // [n][S] the accepted point
  double *pn;       // [n][S] the trial point (round 0: the clipped start)
  double *f;        // [n][3] f(p) through the wrapper
  double *J;        // [n][3][S] J(p)
  double *des;      // [n][3]
  double *err2, *mu, *nu;   // [n]
  int32_t *iters, *fk_calls;   // [n]
};

__device__ __forceinline__ double ik_step_size(double pj, double delta) {
#pragma clang fp contract(off)
  const double a = fabs(1e-4 * pj);
  return a < delta ? delta : a;      // np.maximum(|1e-4 p|, delta) (a NaN stays NaN)
}

// tip_control's FK wrapper (tip_control.cpp:96-104): a retraction beyond L returns (0, 0, L - s_start)
__device__ __forceinline__ void ik_wrap(const double *__restrict__ tip, double s, bool ret, double L, double o[3]) {
#pragma clang fp contract(off)
  if (ret && s > L) { o[0] = 0.0; o[1] = 0.0; o[2] = L - s; }
  else { o[0] = tip[0]; o[1] = tip[1]; o[2] = tip[2]; }
}

// the 2S + 1 FK inputs of each of m points: rows list[r] of src (list null: row r)
__global__ void ik_expand(const double *__restrict__ src, const int32_t *__restrict__ list, int64_t m, int S, double delta,
                          double *__restrict__ xs) {
#pragma clang fp contract(off)
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int Q = 2 * S + 1;
  if (t >= m * Q) return;
  const int64_t r = t / Q;
  const int q = (int)(t - r * Q);
  const double *__restrict__ p = src + (list ? (int64_t)list[r] : r) * S;
  double *__restrict__ o = xs + t * S;
  for (int k = 0; k < S; k++) o[k] = p[k];
  if (q > 0) {
    const int j = (q - 1) >> 1;
    const double d = ik_step_size(p[j], delta);
    o[j] = (q & 1) ? p[j] - d : p[j] + d;
  }
}

// tr_tip_jacobian: f(p) and J(p) of m states from the tips of their expansion, as TendonRobot.tip_jacobian_batch forms them:
// J[k][j] = (tip(p + d_j e_j) - tip(p - d_j e_j))_k * (0.5 / d_j)
__device__ __forceinline__ void ik_f_and_J(const double *__restrict__ x /* the point */, const double *__restrict__ T /* its 2S+1 tips */,
                                           int S, double delta, bool ret, double L, double f[3], double *J /* [3][S] */) {
#pragma clang fp contract(off)
  ik_wrap(T, x[S - 1], ret, L, f);
  for (int j = 0; j < S; j++) {
    const double d = ik_step_size(x[j], delta);
    // the wrapper looks at s_start of the perturbed state: only column S - 1 moves it
    const double sm = j == S - 1 ? x[j] - d : x[S - 1], sp = j == S - 1 ? x[j] + d : x[S - 1];
    double tm[3], tp[3];
    ik_wrap(T + (1 + 2 * j) * 3, sm, ret, L, tm);
    ik_wrap(T + (2 + 2 * j) * 3, sp, ret, L, tp);
    const double sc = 0.5 / d;
    for (int k = 0; k < 3; k++) J[k * S + j] = (tp[k] - tm[k]) * sc;
  }
}

__global__ void ik_jacobian(const double *__restrict__ states, const double *__restrict__ tips, int64_t m, int S, double delta, int ret,
                            double L, double *__restrict__ f, double *__restrict__ J) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  double fo[3];
  ik_f_and_J(states + i * S, tips + i * (2 * S + 1) * 3, S, delta, ret != 0, L, fo, J + i * 3 * S);
  if (f) for (int k = 0; k < 3; k++) f[i * 3 + k] = fo[k];
}

// One LM iteration of every listed problem (list null: problems 0 .. m-1, round 0).  `tips` holds the K1 tips of the expansion of
// the problems' trial points, in list order.  Round 0 (init) evaluates the clipped start; later rounds evaluate the trial point
// and accept or reject it.  Then the problem either stops or takes its next step, which goes to st.pn and into next_list.
template <int S>
__global__ __launch_bounds__(64) void ik_lm_step(IkParams prm, IkState st, const int32_t *__restrict__ list, int64_t m,
                                                 const double *__restrict__ tips, int init, int32_t *__restrict__ next_list,
                                                 uint32_t *__restrict__ next_count) {
#pragma clang fp contract(off)
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= m) return;
  const int64_t i = list ? (int64_t)list[r] : r;
  constexpr int Q = 2 * S + 1;
  const bool ret = prm.retraction != 0;
  double x[S], p[S], J[3 * S], f[3], e[3], des[3];
#pragma unroll
  for (int j = 0; j < S; j++) x[j] = st.pn[i * S + j];
#pragma unroll
  for (int k = 0; k < 3; k++) des[k] = st.des[i * 3 + k];
  double fn[3], Jn[3 * S];
  ik_f_and_J(x, tips + r * Q * 3, S, prm.delta, ret, prm.L, fn, Jn);
  double en[3];
#pragma unroll
  for (int k = 0; k < 3; k++) en[k] = des[k] - fn[k];
  const double err2n = en[0] * en[0] + en[1] * en[1] + en[2] * en[2];
  double err2, mu, nu;
  int iters, calls;
  bool active, accepted;
  double g[S];
  if (init) {
    accepted = true;
#pragma unroll
    for (int j = 0; j < S; j++) p[j] = x[j];
#pragma unroll
    for (int q = 0; q < 3 * S; q++) J[q] = Jn[q];
#pragma unroll
    for (int k = 0; k < 3; k++) { f[k] = fn[k]; e[k] = en[k]; }
    err2 = err2n;
    lm_grad<S>(J, e, g);
    double dmax = 0.0;                              // mu = mu_init * max diag(J^T J), or mu_init when that is not positive
#pragma unroll
    for (int j = 0; j < S; j++) {
      const double a = J[0 * S + j] * J[0 * S + j] + J[1 * S + j] * J[1 * S + j] + J[2 * S + j] * J[2 * S + j];
      if (!(a <= dmax)) dmax = a;
    }
    mu = prm.mu_init * dmax;
    if (!(mu > 0.0)) mu = prm.mu_init;
    nu = 2.0;
    iters = 0;
    calls = Q;
    active = err2 > prm.eps3_sq && lm_moving<S>(p, g, prm);
  } else {
#pragma unroll
    for (int j = 0; j < S; j++) p[j] = st.p[i * S + j];
#pragma unroll
    for (int q = 0; q < 3 * S; q++) J[q] = st.J[i * 3 * S + q];
#pragma unroll
    for (int k = 0; k < 3; k++) { f[k] = st.f[i * 3 + k]; e[k] = des[k] - f[k]; }
    err2 = st.err2[i]; mu = st.mu[i]; nu = st.nu[i]; iters = st.iters[i]; calls = st.fk_calls[i] + Q;
    lm_grad<S>(J, e, g);
    const double rho = lm_gain_ratio<S>(x, p, g, mu, err2, err2n);
    accepted = rho > 0.0;
    if (accepted) {
#pragma unroll
      for (int j = 0; j < S; j++) p[j] = x[j];
#pragma unroll
      for (int q = 0; q < 3 * S; q++) J[q] = Jn[q];
#pragma unroll
      for (int k = 0; k < 3; k++) { f[k] = fn[k]; e[k] = en[k]; }
      err2 = err2n;
      lm_grad<S>(J, e, g);
      const double t = 2.0 * rho - 1.0;
      mu *= lm_shrink(pow(t, 3.0));
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
    // the damped normal equations (J^T J + mu I) dp = J^T e: Cholesky of the packed lower triangle, in registers
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
    // a matrix that is not positive definite (mu overflowed to inf / NaN in J) ends the problem, as the mu-overflow stop does
    const bool small = !spd || dd <= prm.eps2_sq * pp;
    if (!small) {
#pragma unroll
      for (int j = 0; j < S; j++) st.pn[i * S + j] = x[j];
      next_list[atomicAdd(next_count, 1u)] = (int32_t)i;
    }
  }
  st.mu[i] = mu; st.nu[i] = nu; st.iters[i] = iters; st.fk_calls[i] = calls;
}

// results of a chunk: state (rotation canonical, util/angles.h:13-34), tip, error, iters, FK calls (any output may be null)
__global__ void ik_finish(IkParams prm, IkState st, int64_t n, double *__restrict__ states, double *__restrict__ tips,
                          double *__restrict__ error, int32_t *__restrict__ iters, int32_t *__restrict__ fk_calls) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  lm_write_result(prm, i, st.p, st.f, st.err2, st.iters, st.fk_calls, states, tips, error, iters, fk_calls);
}

}  // namespace trk
