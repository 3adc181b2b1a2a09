// fk_loaded_retract_kernel.hpp -- the loaded forward kinematics of retraction-enabled robots (state ends with s_start):
// TendonRobot::general_tension_shape(tau, s_start, f_e, l_e, F_e, L_e) (tendon/TendonRobot.cpp:689-952), which truncates s_start to L,
// returns a one-point result at s_start == L and otherwise shoots on t_range(s_start, L, dL).
//
//   fk_loaded_retract    the loaded counterpart of fk_retract_body (fk_retract_kernel.hpp) with fk_loaded_uniform's calling convention
//                        (fk_loaded_kernel.hpp): lane t is problem in.list[t / in.Q], its base strains are in.vu[t], outputs go to
//                        column t, in.res receives the six residual rows.  A lane covers its own first interval with per-lane routing
//                        (route_tendon), then the wave runs tip-aligned over the shared grid with the routing from K1's scalar table;
//                        both right-hand sides carry c -= R^T l_e, d -= R^T f_e with the STAGE's frame.  The lane's point j is stored
//                        in row j + (P - P_lane), as every kernel of a retraction robot stores it.
//   shoot_start_retract  the start of every problem: the caller's guess, or the unloaded solution of its tensions at the LANE's s_start
//                        (route_anchor, route_tendon, initial_bending: fk_retract_body's prologue).  A kernel of its own, so that the
//                        integrator takes its strains from memory and never holds the fixed-point solve and the per-lane routing
//                        together -- the combination that made the unloaded kernel split into two phases.
//
// Lanes with s_start >= L (or negative) integrate nothing: one point at the origin in row P - 1, L = L_i = 0, n_points = 1 and a
// residual row of exact zeros, so shoot_begin retires them with zero iterations (the reference's early return keeps TendonResult's
// default converged = true; the host clears the flag of a negative s_start, which the unloaded kernels report unconverged).  A lane
// whose s_start lies within dL / 2 of L has one point and no interval; its residual is the tip balance at R = I with its start
// strains, as the reference's `integrate` evaluates it when res.t has one entry.
// The load profile's table has no entries for a lane's own first interval: there is no _profile form (tr_set_load_profile refuses
// retraction robots).  Included by fk_inst.hip, kind 8: one object per tendon count.
#pragma once
#define TRK_LOADED_WITH_INTEGRATOR
#include "fk_loaded_kernel.hpp"
#include "fk_retract_kernel.hpp"

namespace trk {

// Waves per SIMD (measured, round 29: ms per call of tr_fk_loaded_batch_dev on 2^14 problems, s_start ~ U[0, 0.6 L], gravity and a tip
// force, rotation and general routing, dL = L / 40; median of 7, two alternations in one job; two waves | one wave).  Started from
// TRK_K1R_TWO_WAVE_MAXN's split (4): N=1 3.14, 3.12 | 3.13, 3.13; N=2 3.54, 3.59 | 3.58, 3.59; N=3 4.62, 4.62 | 4.47, 4.48; N=4 5.52,
// 5.47 | 5.36, 5.37.  Two waves spill 670 - 870 B of scratch per lane at N = 3, 4 (the first interval's per-lane routing beside the load
// terms) and lose 2 - 3 %, outside both runs' min - max ranges; at N = 1, 2 the two widths tie.  The results are the same bits.
#ifndef TRK_LR_TWO_WAVE_MAXN
#define TRK_LR_TWO_WAVE_MAXN 2
#endif

// R^T f_e, R^T l_e with the stage's frame sR (the explicit FMAs of fk_loaded_body.inc): rk4_step_routed's stage_load hook
struct FrameLoad {
  const double (&fe)[3];
  const double (&le)[3];
  __device__ __forceinline__ BodyLoad operator()(const double (&sR)[9]) const {
    BodyLoad load;
#pragma unroll
    for (int c = 0; c < 3; c++) {
      load.f[c] = __builtin_fma(sR[c * 3 + 2], fe[2], __builtin_fma(sR[c * 3 + 1], fe[1], sR[c * 3 + 0] * fe[0]));
      load.l[c] = __builtin_fma(sR[c * 3 + 2], le[2], __builtin_fma(sR[c * 3 + 1], le[1], sR[c * 3 + 0] * le[0]));
    }
    return load;
  }
};

template <int N>
__global__ __launch_bounds__(64) void shoot_start_retract(const double *__restrict__ states, int64_t n, RobotK K, const PolyK *__restrict__ pk,
                                                          const double *__restrict__ guess, double *__restrict__ vu,
                                                          const int32_t *__restrict__ perm) {
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
  const bool live = i < n;
  const int64_t il = live ? i : (n - 1);       // tail lanes repeat the last problem (initial_bending votes across the wave)
  const int64_t ig = perm ? (int64_t)perm[il] : il;      // the caller's row of this problem (the clamped index: perm holds n entries)
  double v[3], u[3];
  if (guess) {
#pragma unroll
    for (int q = 0; q < 3; q++) { v[q] = guess[ig * 6 + q]; u[q] = guess[ig * 6 + 3 + q]; }
  } else {
    const int S = K.state_size;
    double tau[N];
#pragma unroll
    for (int j = 0; j < N; j++) tau[j] = states[ig * S + j];
    double s = states[ig * S + S - 1];
    if (s > K.L) s = K.L;                      // TendonRobot.cpp:359
    RouteCarry<N> rcy;
    route_anchor<N>(pk, K.n_a, s, rcy);
    double rloc[N * 6];
#pragma unroll
    for (int j = 0; j < N; j++) {
      double r6[6];
      route_tendon<N>(pk, K.n_a, K.n_m, j, s, rcy, r6);
#pragma unroll
      for (int q = 0; q < 6; q++) rloc[6 * j + q] = r6[q];
    }
    bool conv;
    initial_bending<N>(tau, rloc, K, v, u, conv);
  }
  if (live) {
#pragma unroll
    for (int q = 0; q < 3; q++) { vu[i * 6 + q] = v[q]; vu[i * 6 + 3 + q] = u[q]; }
  }
}

template <int N, bool ROT, bool WRITE_R>
__global__ __launch_bounds__(64, (N <= TRK_LR_TWO_WAVE_MAXN ? 2 : 1)) void fk_loaded_retract(
    const double *__restrict__ states, int64_t n, int64_t ld, RobotK K, const PolyK *__restrict__ pk,
    const double *__restrict__ tab /* K1's routing table of the s_start = 0 grid */, const StepK *__restrict__ steps, int nsteps,
    int k_first /* first step after the grid's own first interval */, const double *__restrict__ tgrid /* [P] shared abscissae */,
    const double *__restrict__ hl /* [P][N] home-length integrand at the shared abscissae */, FkOut out, LoadedIn in) {
#pragma clang fp contract(fast)
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
  const bool live = i < n;
  const int64_t il = live ? i : (n - 1);       // tail lanes recompute the last lane, stores masked
  const int64_t ir = il / in.Q;
  const int64_t iq = in.list ? (int64_t)in.list[ir] : ir;      // the launch's problem (chunk-local, from the clamped lane)
  const int64_t ic = in.perm ? (int64_t)in.perm[iq] : iq;      // ... and its column of the caller's arrays
  // outputs (one lane per problem: iq == i on live lanes) go to the caller's column; the launch's own arrays (vu, res) stay on i
  const int64_t io = in.perm ? ic : i;
  const int S = K.state_size, Pmax = K.n_points;
  const double L = K.L, dL = K.dL;
  double tau[N];
#pragma unroll
  for (int j = 0; j < N; j++) tau[j] = states[ic * S + j];
  double rc = 1.0, rs = 0.0, r22 = 1.0;
  if (ROT) {
    const double th = states[ic * S + N];
    rs = sin(th); rc = cos(th);
    r22 = (1.0 - rc) + rc;
  }
  // the lane's geometry, as fk_retract_body forms it
  const double s_raw = states[ic * S + S - 1];
  const bool negative = s_raw < 0.0;
  double s = s_raw;
  if (s > L) s = L;                                  // TendonRobot.cpp:359
  const bool single = (s == L) || negative;          // :361-372
  // forward pass of util::range: p_0 = s, p_{k+1} = p_k + dL while p <= L - dL/2 -> number of points
  int m = 0;
  {
    double q = s;
    for (int k = 0; k < Pmax; k++) {
      const bool go = !single && (q <= L - (dL / 2)) && k < Pmax - 1;
      if (!__any(go)) break;
      if (go) { m = k + 1; q += dL; }
    }
  }
  const int P_lane = single ? 1 : m + 1;
  const int shift = Pmax - P_lane;                   // lane point j = shared grid point j + shift (j >= 1)

  double fe[3] = {0, 0, 0}, le[3] = {0, 0, 0};
  if (in.dist) {
#pragma unroll
    for (int q = 0; q < 3; q++) { fe[q] = in.dist[ic * in.dist_ld + q]; le[q] = in.dist[ic * in.dist_ld + 3 + q]; }
  }
  const FrameLoad stage_load{fe, le};
  double v[3], u[3];
#pragma unroll
  for (int q = 0; q < 3; q++) { v[q] = in.vu[il * 6 + q]; u[q] = in.vu[il * 6 + 3 + q]; }

  double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};   // column-major: R[c*3+r]
  double p[3] = {0, 0, 0};
  double Lb = 0;
  double Li[N];
#pragma unroll
  for (int j = 0; j < N; j++) Li[j] = 0;

  // `row` may differ from lane to lane (the lane's first two points) or be wave-uniform (the tip-aligned loop); always in [0, P)
  auto store_point = [&](int row, bool on) {
    if (!(on && live) || !out.px) return;
    const int64_t o = (int64_t)row * ld + io;
    double x = p[0], y = p[1], z = p[2];
    if (ROT) { const double x2 = __builtin_fma(rc, x, -(rs * y)), y2 = __builtin_fma(rs, x, rc * y); x = x2; y = y2; z = r22 * z; }
    out.px[o] = x; out.py[o] = y; out.pz[o] = z;
    if (WRITE_R) {
      const int64_t PS = (int64_t)Pmax * ld;
#pragma unroll
      for (int c = 0; c < 3; c++) {
        double a = R[c * 3 + 0], b = R[c * 3 + 1], cc = R[c * 3 + 2];
        if (ROT) { const double a2 = rc * a - rs * b, b2 = rs * a + rc * b; a = a2; b = b2; cc = r22 * cc; }
        out.R[(c * 3 + 0) * PS + o] = a; out.R[(c * 3 + 1) * PS + o] = b; out.R[(c * 3 + 2) * PS + o] = cc;
      }
    }
  };
  store_point(shift, true);                          // rows are aligned at the tip (a single lane: the origin in row P - 1)

  // the lane's own first interval: s -> shared grid point shift + 1, steps of min(dL, remaining) while remaining > eps
  // (integrate_times), routing evaluated per lane
  const bool first = !single && P_lane >= 2;
  if (__any(first)) {
    RouteCarry<N> rcy;
    route_anchor<N>(pk, K.n_a, s, rcy);
    double cur = L - (L - s);                        // t[0]: the mirrored `end` sample of t_range
    double tn = cur;
    if (first) tn = tgrid[shift + 1];                // (first: 0 <= shift <= P - 2)
    for (int sub = 0; sub < 4; sub++) {
      const bool go = first && (tn - cur > 2.220446049250313e-16);
      if (!__any(go)) break;
      if (go) {
        const double h = (dL < tn - cur) ? dL : (tn - cur);
        rk4_step_routed<N>(R, v, u, p, Lb, Li, tau, K, cur, h,
                           [&](double tt, int j, double (&r6)[6]) { route_tendon<N>(pk, K.n_a, K.n_m, j, tt, rcy, r6); }, stage_load);
        cur += h;
      }
    }
    store_point(shift + 1, first);
  }

  // tip-aligned: step k of the shared grid ends at its point steps[k].obs = the lane's point obs - shift.  k_first is a kernel
  // argument: the loop counter is wave-uniform and the routing rows arrive through scalar loads (fk_retract_kernel.hpp tells what
  // happened when it was not).
  for (int k = k_first; k < nsteps; k++) {
    const int obs = steps[k].obs;
    const bool act = !single && obs - shift >= 2;
    if (!__any(act)) continue;
    if (act) {
      const double h = steps[k].h;
      const double *__restrict__ rt = tab + (size_t)(1 + 3 * k) * (N * 6);
      const double hh = h * 0.5;
      const double b1 = h * (1.0 / 6.0), b2 = h * (1.0 / 3.0);
      double aR[9], av[3], au[3];
#pragma unroll
      for (int q = 0; q < 3; q++) { av[q] = v[q]; au[q] = u[q]; }
      double sR[9], sv[3], su[3], qs[3], qm[3];
#pragma unroll
      for (int q = 0; q < 9; q++) sR[q] = R[q];
#pragma unroll
      for (int q = 0; q < 3; q++) { sv[q] = v[q]; su[q] = u[q]; }
#pragma unroll
      for (int st = 0; st < 4; st++) {
        const double *__restrict__ ri = rt + (st == 0 ? 0 : (st == 3 ? 2 : 1)) * (N * 6);
        const double bw = (st == 0 || st == 3) ? b1 : b2;
        const double aw = (st == 2) ? h : hh;
        double dv[3], du[3], sd[N];
        strain_rates<N>(sv, su, tau, ri, K, dv, du, sd, stage_load(sR));
        position_quadrature(st, sR, sv, b1, qs, qm, p);
        {
          const double v2 = sv[0] * sv[0] + sv[1] * sv[1] + sv[2] * sv[2];
          Lb += bw * (v2 * fast_rsqrt(v2));
        }
#pragma unroll
        for (int j = 0; j < N; j++) Li[j] += bw * sd[j];
        double dR[9];
        frame_rate(st, sR, su, dR, aR);
#pragma unroll
        for (int q = 0; q < 3; q++) { av[q] += bw * dv[q]; au[q] += bw * du[q]; }
        if (st < 3) {
#pragma unroll
          for (int q = 0; q < 9; q++) sR[q] = R[q] + aw * dR[q];
#pragma unroll
          for (int q = 0; q < 3; q++) { sv[q] = v[q] + aw * dv[q]; su[q] = u[q] + aw * du[q]; }
        }
      }
#pragma unroll
      for (int q = 0; q < 9; q++) R[q] = __builtin_fma(b1, aR[q], R[q]);
#pragma unroll
      for (int q = 0; q < 3; q++) { v[q] = av[q]; u[q] = au[q]; }
    }
    store_point(obs, act);                           // (obs < P: the table's own rows)
  }

  if (in.res) {
    double e[6];
    tip_residual<N>(R, v, u, tau, K, in.tip_route, in.wrench + ic * in.wrench_ld, e);
    if (live) {
#pragma unroll
      for (int r = 0; r < 6; r++) in.res[(int64_t)r * in.ldr + i] = single ? 0.0 : e[r];
    }
  }
  double home[N];
  if (out.home_Li) home_lengths_lane<N>(pk, K, hl, s_raw, s, single, P_lane, shift, true, home);
  if (live) {
    if (out.L) out.L[io] = Lb;
    if (out.Li) {
#pragma unroll
      for (int j = 0; j < N; j++) out.Li[(int64_t)j * ld + io] = Li[j];
    }
    if (out.n_points) out.n_points[io] = P_lane;
    if (out.home_Li) {
#pragma unroll
      for (int j = 0; j < N; j++) out.home_Li[(int64_t)j * ld + io] = home[j];
    }
    if (in.vu_tip) {
#pragma unroll
      for (int q = 0; q < 3; q++) { in.vu_tip[io * 6 + q] = v[q]; in.vu_tip[io * 6 + 3 + q] = u[q]; }
    }
  }
}

}  // namespace trk
