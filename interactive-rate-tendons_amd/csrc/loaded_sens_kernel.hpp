// loaded_sens_kernel.hpp -- the per-problem kernel of the loaded tip Jacobian and tip compliance (tr_tip_jacobian_loaded*,
// loaded_jacobian_host.inc): what ikl_lm_step (loaded_ik_kernel.hpp) forms of the linearisation launch inside the loaded IK's loop,
// handed to the caller.
//
// At base strains y that balance the tip of the loaded rod, e_w(y, p) = balance(y, p) - w = 0, the tip x(y, p) moves
//   with the state   as dx/dp = J = X_p - X_y W,  W = J_y^-1 J_p   (the implicit-function theorem; -W = dy/dp)
//   with the wrench  as dx/dw = C = X_y J_y^-1 T                  (de_w/dw = -T, so dy/dw = J_y^-1 T)
// with J_y = de_w/dy, J_p = de_w/dp, X_y = dx/dy, X_p = dx/dp the central differences of the 13 + 2 S lanes of one fk_loaded_lin
// launch (fk_lin_launch.hpp: LinIn).  T is the identity for a wrench given in the frame before the state's rotation; a wrench fixed
// in the world frame enters the residual turned by Rz(-theta), T = blockdiag(Rz(-theta), Rz(-theta)), so that C is the derivative
// with respect to the wrench as the caller gave it.  The shooting stops at the threshold, not at the equilibrium: one Newton step
// with J_y gives the strains y_c = y - J_y^-1 e_w and the tip x_c = x - X_y J_y^-1 e_w that are returned.
//
// The LU of J_y with partial pivoting in registers and the solves are the functions ikl_lm_step calls (lm_dense.hpp: lu6_factor,
// lu6_solve); the differences, the Newton step and the reduction around them are ikl_lm_step's text, operation by operation (the
// header says why they are not functions too): W and J are the bits the loaded IK uses from the same planes.  The specification
// is tests/loaded_jacobian_reference.py.  Compiled without contraction.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "loaded_ik_kernel.hpp"

namespace trk {

// outputs of one chunk, row r = problem r of the chunk; each is written only where its pointer is not null
struct SensOut {
  double *tips;        // [m][3] x_c
  double *vu0;         // [m][6] y_c
  double *J;           // [m][3][S]
  double *W;           // [m][6][S]
  double *C;           // [m][3][6]
  double *blocks;      // [m][69 + 9 S]: y(6), x(3), e(6), J_y(36), J_p(6 S), X_y(18), X_p(3 S), row-major each
  uint8_t *eq;         // [m] the shooting converged and J_y has no zero pivot
  int64_t *nint;       // [m] integrations: the shooting's and the 13 + 2 S lanes
};

// One lane per problem.  lin: the [9][ldr] planes of the linearisation launch, lane r (13 + 2 S) + q; rows: the launch's states and
// strains and the shooting's flags.  A problem whose shooting did not converge gets NaN in every double output.
template <int S>
__global__ __launch_bounds__(64) void loaded_tip_sens(double delta_p, double delta_y, int rot_index, int world, int64_t m,
                                                      const double *__restrict__ lin, int64_t ldr, IklRows rows, SensOut o) {
#pragma clang fp contract(off)
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= m) return;
  constexpr int Q = 13 + 2 * S;
  constexpr int NB = 69 + 9 * S;
  const double *__restrict__ row = lin + r * Q;              // row[plane * ldr + q]
  const bool conv = rows.conv[r] != 0;
  const double nan = __builtin_nan("");
  auto put = [&](double *dst, double v) { *dst = conv ? v : nan; };
  double x[S];
#pragma unroll
  for (int j = 0; j < S; j++) x[j] = rows.states[r * S + j];
  double *__restrict__ blk = o.blocks ? o.blocks + r * NB : nullptr;
  // J_y and X_y: central differences with the shooting's absolute step (ikl_lm_step)
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
  if (blk) {
#pragma unroll
    for (int a = 0; a < 6; a++) { put(blk + a, rows.vu[r * 6 + a]); put(blk + 9 + a, row[a * ldr]); }
#pragma unroll
    for (int k = 0; k < 3; k++) put(blk + 6 + k, row[(6 + k) * ldr]);
#pragma unroll
    for (int q = 0; q < 36; q++) put(blk + 15 + q, A[q]);
#pragma unroll
    for (int q = 0; q < 18; q++) put(blk + 51 + 6 * S + q, Xy[q]);
  }
  // the LU factors of J_y; a zero pivot clears the problem's flag
  int piv[6];
  const bool singular = lu6_factor(A, piv);
  // the Newton step on the strains: y_c = y - J_y^-1 e_w, x_c = x - X_y J_y^-1 e_w
  {
    double b[6];
#pragma unroll
    for (int a = 0; a < 6; a++) b[a] = row[a * ldr];
    lu6_solve(A, piv, b);
    if (o.vu0) {
#pragma unroll
      for (int a = 0; a < 6; a++) put(o.vu0 + r * 6 + a, rows.vu[r * 6 + a] - b[a]);
    }
    if (o.tips) {
#pragma unroll
      for (int k = 0; k < 3; k++) {
        double t = 0.0;
#pragma unroll
        for (int a = 0; a < 6; a++) t += Xy[k * 6 + a] * b[a];
        put(o.tips + r * 3 + k, row[(6 + k) * ldr] - t);
      }
    }
  }
  // W = J_y^-1 J_p and J = X_p - X_y W, column by column over the state
#pragma unroll
  for (int k = 0; k < S; k++) {
    const double sc = 0.5 / ik_step_size(x[k], delta_p);
    double b[6];
#pragma unroll
    for (int a = 0; a < 6; a++) b[a] = (row[a * ldr + 14 + 2 * k] - row[a * ldr + 13 + 2 * k]) * sc;
    if (blk) {
#pragma unroll
      for (int a = 0; a < 6; a++) put(blk + 51 + a * S + k, b[a]);
    }
    lu6_solve(A, piv, b);
    if (o.W) {
#pragma unroll
      for (int a = 0; a < 6; a++) put(o.W + (r * 6 + a) * S + k, b[a]);
    }
#pragma unroll
    for (int q = 0; q < 3; q++) {
      double s = 0.0;
#pragma unroll
      for (int a = 0; a < 6; a++) s += Xy[q * 6 + a] * b[a];
      const double xp = (row[(6 + q) * ldr + 14 + 2 * k] - row[(6 + q) * ldr + 13 + 2 * k]) * sc;
      if (blk) put(blk + 69 + 6 * S + q * S + k, xp);
      if (o.J) put(o.J + (r * 3 + q) * S + k, xp - s);
    }
  }
  // C = X_y J_y^-1 T, column by column over the wrench: column 3 h + g of T is Rz(-theta) e_g in block h
  if (o.C) {
    const bool turn = world && rot_index >= 0 && rot_index < S;
    double sn = 0.0, cs = 1.0;
    if (turn) edge_sincos(rows.states[r * S + rot_index], sn, cs);
#pragma unroll
    for (int j = 0; j < 6; j++) {
      const int h = j < 3 ? 0 : 3, g = j - h;
      double b[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      // Rz(-theta) = [c s 0; -s c 0; 0 0 1]
      if (g == 0) { b[h + 0] = cs; if (turn) b[h + 1] = -sn; }
      else if (g == 1) { if (turn) b[h + 0] = sn; b[h + 1] = cs; }
      else b[h + 2] = 1.0;
      lu6_solve(A, piv, b);
#pragma unroll
      for (int q = 0; q < 3; q++) {
        double s = 0.0;
#pragma unroll
        for (int a = 0; a < 6; a++) s += Xy[q * 6 + a] * b[a];
        put(o.C + (r * 3 + q) * 6 + j, s);
      }
    }
  }
  if (o.eq) o.eq[r] = (conv && !singular) ? 1 : 0;
  if (o.nint) o.nint[r] = (int64_t)rows.calls[r] + Q;
}

}  // namespace trk
