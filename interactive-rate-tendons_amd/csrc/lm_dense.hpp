// lm_dense.hpp -- the small dense algebra and the Levenberg-Marquardt bookkeeping that the one-lane-per-problem step kernels share:
// ik_lm_step<S> (ik_kernel.hpp), ikl_lm_step<S> (loaded_ik_kernel.hpp), loaded_tip_sens<S> (loaded_sens_kernel.hpp) and
// shoot_lm_step (fk_loaded_kernel.hpp).  Every function works on fixed-size array references, so that after inlining everything
// stays in registers, and is compiled without contraction: a kernel that calls one of them runs the floating-point operations of
// every other caller, in the same order.  The functions also compile for the host (tests/cpp/lm_dense_test.cpp).
//
// Where the kernels differ.  Each of these can change a bit of a result, none of them is shared, and each stays in its kernel:
//   ik_lm_step     cubes the gain-ratio term with pow(t, 3.0), the other two with t * t * t (lm_shrink takes the cube);
//                  ends a problem on dd <= eps2_sq * pp, the other two on !(dd > eps2_sq * pp): a NaN step goes on in ik_lm_step
//                  alone
//   ikl_lm_step    accepts a trial only if its shooting converged (accepted = conv && rho > 0), and ends a problem in the first
//                  round when its start has no equilibrium
//   shoot_lm_step  solves for g = -J^T e (its residual is e, not des - f), with its own grad over 6 x 6 and no box in its gradient
//                  test; damps with Marquardt's scaling mu diag(J^T J), in the normal matrix and in the predicted decrease of its
//                  gain ratio; starts the sum of a normal-matrix entry from the damping term and adds six products, where the two
//                  IK kernels add the damping to three products last; takes the step unprojected; and still evaluates the step
//                  its relative-step test judges small (the sign of nu carries that to the next round)
// So shoot_lm_step shares chol_solve_packed<6>, lm_shrink and lm_reject, and nothing else of the 3 x S functions.
//
// What is still written twice, because the compiler's register allocation follows the text.  Each of these was tried as a function
// here; the operations stayed the same and the figures that tests/test_loaded_*_kernel_resources.py hold did not:
//   the start value of mu, the build of the normal matrix and the projection of the step onto the box (ik_lm_step, ikl_lm_step):
//                  as functions, ikl_lm_step<10> takes 16 more AGPRs (mu), or spills 12 SGPRs (matrix, projection)
//   the strain blocks J_y, X_y, the Newton correction and the column-by-column reduction (ikl_lm_step, loaded_tip_sens): as
//                  functions, loaded_tip_sens<3> and <5> take 250 and 254 VGPRs where 178 and 180 are pinned
// These keep one text per kernel, the same in both; what they call (lu6_factor, lu6_solve, chol_solve_packed) is shared.
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define TRK_LM_FN __host__ __device__ __forceinline__
#else
#define TRK_LM_FN inline
#endif
#include <math.h>
#include <stdint.h>

#define TRK_IK_MAX_S 10      // TRK_MAX_TENDONS + rotation + retraction

namespace trk {

struct IkParams {
  int32_t S, max_iters;
  int32_t rot_index;                 // state index of the rotation (-1: none); canonicalised by the finish kernels
  int32_t retraction;                // tip_control's FK wrapper applies to the last state entry
  double L;                          // backbone length (the wrapper's threshold)
  double delta;                      // finite_difference_delta
  double mu_init, eps1, eps2_sq, eps3_sq;   // mu_init, |J^T e|_inf, |Dp|^2 (relative), |e|^2
  double lo[TRK_IK_MAX_S], hi[TRK_IK_MAX_S];
};

TRK_LM_FN double ik_clip(double x, double lo, double hi) {
  const double v = x < lo ? lo : x;  // np.clip: minimum(maximum(x, lo), hi) (a NaN stays NaN)
  return v > hi ? hi : v;
}

// ---- S x S, symmetric: the damped normal equations ---------------------------------------------------------------------------------

// A y = g by the Cholesky factorisation of the packed lower triangle A[a (a + 1) / 2 + b], b <= a, in place, then the forward and
// the back substitution.  Returns whether every pivot was positive; one that is not is replaced by 1, so y holds no NaN of the
// factorisation's own making.
template <int S>
TRK_LM_FN bool chol_solve_packed(double (&A)[S * (S + 1) / 2], const double (&g)[S], double (&y)[S]) {
#pragma clang fp contract(off)
  bool spd = true;
#pragma unroll
  for (int a = 0; a < S; a++) {
#pragma unroll
    for (int b = 0; b <= a; b++) {
      double s = A[a * (a + 1) / 2 + b];
#pragma unroll
      for (int k = 0; k < b; k++) s -= A[a * (a + 1) / 2 + k] * A[b * (b + 1) / 2 + k];
      if (a == b) {
        spd = spd && s > 0.0;
        A[a * (a + 1) / 2 + a] = sqrt(s > 0.0 ? s : 1.0);
      } else {
        A[a * (a + 1) / 2 + b] = s / A[b * (b + 1) / 2 + b];
      }
    }
  }
#pragma unroll
  for (int a = 0; a < S; a++) {
    double s = g[a];
#pragma unroll
    for (int k = 0; k < a; k++) s -= A[a * (a + 1) / 2 + k] * y[k];
    y[a] = s / A[a * (a + 1) / 2 + a];
  }
#pragma unroll
  for (int a = S - 1; a >= 0; a--) {
    double s = y[a];
#pragma unroll
    for (int k = a + 1; k < S; k++) s -= A[k * (k + 1) / 2 + a] * y[k];
    y[a] = s / A[a * (a + 1) / 2 + a];
  }
  return spd;
}

// ---- 6 x 6, general: J_y of the loaded rod -----------------------------------------------------------------------------------------

// P A = L U in place (unit L below the diagonal) with partial pivoting; piv[c]: the row exchanged with row c.  Returns whether a
// pivot was zero: what is then solved with the factors holds inf / NaN.
TRK_LM_FN bool lu6_factor(double (&A)[36], int (&piv)[6]) {
#pragma clang fp contract(off)
  bool singular = false;
#pragma unroll
  for (int c = 0; c < 6; c++) {
    int pr = c;
    double best = fabs(A[c * 6 + c]);
#pragma unroll
    for (int a = c + 1; a < 6; a++) { const double t = fabs(A[a * 6 + c]); if (t > best) { best = t; pr = a; } }
    piv[c] = pr;
#pragma unroll
    for (int a = c + 1; a < 6; a++) {
      if (pr == a) {
#pragma unroll
        for (int b = 0; b < 6; b++) { const double t = A[c * 6 + b]; A[c * 6 + b] = A[a * 6 + b]; A[a * 6 + b] = t; }
      }
    }
    const double d = A[c * 6 + c];
    singular = singular || d == 0.0;
#pragma unroll
    for (int a = c + 1; a < 6; a++) {
      const double l = A[a * 6 + c] / d;
      A[a * 6 + c] = l;
#pragma unroll
      for (int b = c + 1; b < 6; b++) A[a * 6 + b] -= l * A[c * 6 + b];
    }
  }
  return singular;
}

// b <- A^-1 b with lu6_factor's factors
TRK_LM_FN void lu6_solve(const double (&A)[36], const int (&piv)[6], double (&b)[6]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int c = 0; c < 6; c++) {
#pragma unroll
    for (int a = c + 1; a < 6; a++)
      if (piv[c] == a) { const double t = b[c]; b[c] = b[a]; b[a] = t; }
  }
#pragma unroll
  for (int a = 1; a < 6; a++) {
#pragma unroll
    for (int c = 0; c < a; c++) b[a] -= A[a * 6 + c] * b[c];
  }
#pragma unroll
  for (int a = 5; a >= 0; a--) {
#pragma unroll
    for (int c = a + 1; c < 6; c++) b[a] -= A[a * 6 + c] * b[c];
    b[a] = b[a] / A[a * 6 + a];
  }
}

// ---- 3 x S: the outer iteration of the tip IK, unloaded and loaded (tip_control.inverse_kinematics_batch's scheme) ------------------

// g = J^T e
template <int S>
TRK_LM_FN void lm_grad(const double (&J)[3 * S], const double (&e)[3], double (&g)[S]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int j = 0; j < S; j++) g[j] = J[0 * S + j] * e[0] + J[1 * S + j] * e[1] + J[2 * S + j] * e[2];
}

// components of J^T e that can still move the state inside the box (tip_control.py: free_gradient) -> max |.| > eps1
template <int S>
TRK_LM_FN bool lm_moving(const double (&p)[S], const double (&g)[S], const IkParams &prm) {
#pragma clang fp contract(off)
  double mx = 0.0;
#pragma unroll
  for (int j = 0; j < S; j++) {
    const bool blocked = (p[j] <= prm.lo[j] && g[j] < 0.0) || (p[j] >= prm.hi[j] && g[j] > 0.0);
    const double a = blocked ? 0.0 : fabs(g[j]);
    if (!(a <= mx)) mx = a;                       // a NaN wins, as in np.max
  }
  return mx > prm.eps1;
}

// gain ratio of the step dp = x - p against the model's predicted decrease dp . (mu dp + g); -1 when that is not positive
template <int S>
TRK_LM_FN double lm_gain_ratio(const double (&x)[S], const double (&p)[S], const double (&g)[S], double mu, double err2, double err2n) {
#pragma clang fp contract(off)
  double pred = 0.0;
#pragma unroll
  for (int j = 0; j < S; j++) { const double dp = x[j] - p[j]; pred += dp * (mu * dp + g[j]); }
  return pred > 0.0 ? (err2 - err2n) / pred : -1.0;
}

// mu's factor after an accepted step, from cube = (2 rho - 1)^3 as the kernel forms it: max(1/3, 1 - cube)
TRK_LM_FN double lm_shrink(double cube) {
#pragma clang fp contract(off)
  const double sh = 1.0 - cube;
  return (1.0 / 3.0) > sh ? (1.0 / 3.0) : sh;
}

// after a rejected step
TRK_LM_FN void lm_reject(double &mu, double &nu) {
#pragma clang fp contract(off)
  mu *= nu;
  nu *= 2.0;
}

// ---- start and end of a chunk ------------------------------------------------------------------------------------------------------

// util/angles.h:13-34: [-pi, pi)
TRK_LM_FN double canonical_angle(double v) {
#pragma clang fp contract(off)
  const double pi = 3.141592653589793, two_pi = 2.0 * pi;
  return fmod(fmod(v + pi, two_pi) + two_pi, two_pi) - pi;
}

// what both IKs return of problem i (any output may be null): the state with the rotation canonical, the tip, the error, the
// iterations and the FK calls / integrations
TRK_LM_FN void lm_write_result(const IkParams &prm, int64_t i, const double *p, const double *f, const double *err2, const int32_t *iters,
                               const int32_t *calls, double *states_out, double *tips_out, double *error_out, int32_t *iters_out,
                               int32_t *calls_out) {
#pragma clang fp contract(off)
  const int S = prm.S;
  if (states_out) {
    for (int j = 0; j < S; j++) states_out[i * S + j] = j == prm.rot_index ? canonical_angle(p[i * S + j]) : p[i * S + j];
  }
  if (tips_out) for (int k = 0; k < 3; k++) tips_out[i * 3 + k] = f[i * 3 + k];
  if (error_out) error_out[i] = sqrt(err2[i]);
  if (iters_out) iters_out[i] = iters[i];
  if (calls_out) calls_out[i] = calls[i];
}

#ifdef __HIPCC__
// clipped start (into pn) and goal (into des_out) of every problem of a chunk (des_ld = 0: one goal row for all)
__global__ void lm_init(const double *__restrict__ init, int64_t n, const double *__restrict__ des, int64_t des_ld, IkParams prm,
                        double *__restrict__ pn, double *__restrict__ des_out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int S = prm.S;
  for (int j = 0; j < S; j++) pn[i * S + j] = ik_clip(init[i * S + j], prm.lo[j], prm.hi[j]);
  for (int k = 0; k < 3; k++) des_out[i * 3 + k] = des[i * des_ld + k];
}
#endif

}  // namespace trk
