// fk_loaded_body.inc -- the body of fk_loaded_uniform and fk_loaded_profile (fk_loaded_kernel.hpp), which includes it once per form
// of the stage's load row (TRK_STAGE_ROW).  A fragment, not a header: it stands between a kernel's braces and names the kernel's
// parameters and template arguments as they are spelt there --
//   template arguments  N, ROT, WRITE_R
//   parameters          states, n, ld, K, tab, steps, nsteps, out (FkOut), in (LoadedIn; the profile form reads in.weights)
//   macro               TRK_STAGE_ROW(entry, fs, ls): declares the stage's row fs[3], ls[3] from fe, le of this body
// The fp-contract pragma below must be the first thing in the kernel's compound statement: the including kernel may put nothing
// but preprocessor lines between its opening brace and the #include.
#pragma clang fp contract(fast)
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
  const bool live = i < n;
  const int64_t il = live ? i : (n - 1);       // tail lanes recompute the last lane, stores masked
  const int64_t ir = il / in.Q;
  const int64_t ic = in.list ? (int64_t)in.list[ir] : ir;
  const int S = K.state_size;
  double tau[N];
#pragma unroll
  for (int j = 0; j < N; j++) tau[j] = states[ic * S + j];
  double rc = 1.0, rs = 0.0, r22 = 1.0;
  if (ROT) {
    const double th = states[ic * S + N];
    rs = sin(th); rc = cos(th);
    r22 = (1.0 - rc) + rc;
  }
  double fe[3] = {0, 0, 0}, le[3] = {0, 0, 0};
  if (in.dist) {
#pragma unroll
    for (int q = 0; q < 3; q++) { fe[q] = in.dist[ic * in.dist_ld + q]; le[q] = in.dist[ic * in.dist_ld + 3 + q]; }
  }
  double v[3], u[3];
#pragma unroll
  for (int q = 0; q < 3; q++) { v[q] = in.vu[il * 6 + q]; u[q] = in.vu[il * 6 + 3 + q]; }

  double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};   // column-major: R[c*3+r]
  double p[3] = {0, 0, 0};
  double Lb = 0;
  double Li[N];
#pragma unroll
  for (int j = 0; j < N; j++) Li[j] = 0;

  auto store_point = [&](int j) {
    if (!live || !out.px) return;
    const int64_t o = (int64_t)j * ld + i;
    double x = p[0], y = p[1], z = p[2];
    if (ROT) { const double x2 = __builtin_fma(rc, x, -(rs * y)), y2 = __builtin_fma(rs, x, rc * y); x = x2; y = y2; z = r22 * z; }
    out.px[o] = x; out.py[o] = y; out.pz[o] = z;
    if (WRITE_R) {
      const int64_t PS = (int64_t)K.n_points * ld;
#pragma unroll
      for (int c = 0; c < 3; c++) {
        double a = R[c * 3 + 0], b = R[c * 3 + 1], cc = R[c * 3 + 2];
        if (ROT) { const double a2 = rc * a - rs * b, b2 = rs * a + rc * b; a = a2; b = b2; cc = r22 * cc; }
        out.R[(c * 3 + 0) * PS + o] = a; out.R[(c * 3 + 1) * PS + o] = b; out.R[(c * 3 + 2) * PS + o] = cc;
      }
    }
  };
  store_point(0);

  for (int k = 0; k < nsteps; k++) {
    const double h = steps[k].h;
    const int obs = steps[k].obs;
    const double *__restrict__ rt = tab + (size_t)(1 + 3 * k) * (N * 6);
    const double hh = h * 0.5;
    const double b1 = h * (1.0 / 6.0), b2 = h * (1.0 / 3.0);
    double aR[9], av[3], au[3];
#pragma unroll
    for (int q = 0; q < 3; q++) { av[q] = v[q]; au[q] = u[q]; }
    double sR[9], sv[3], su[3];
    double qs[3], qm[3];
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
      TRK_STAGE_ROW(1 + 3 * k + (st == 0 ? 0 : (st == 3 ? 2 : 1)), fs, ls)   // the row (f_e, l_e) this stage sees
      BodyLoad load;                                          // R^T f_e, R^T l_e with the stage's frame
#pragma unroll
      for (int c = 0; c < 3; c++) {
        load.f[c] = __builtin_fma(sR[c * 3 + 2], fs[2], __builtin_fma(sR[c * 3 + 1], fs[1], sR[c * 3 + 0] * fs[0]));
        load.l[c] = __builtin_fma(sR[c * 3 + 2], ls[2], __builtin_fma(sR[c * 3 + 1], ls[1], sR[c * 3 + 0] * ls[0]));
      }
      strain_rates<N>(sv, su, tau, ri, K, dv, du, sd, load);
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
    if (obs >= 0) store_point(obs);
  }

  if (in.res) {
    // PointForces::calc_point_forces at the tip, every term in the base frame as the reference forms it: n = R K_se (v - e3),
    // m = R K_bt u, F_t = sum -tau_i unit(R pd_i), L_t = sum (R r_i) x F_t,i.  The tendon directions are normalised AFTER the
    // rotation: the integrated frame is orthonormal to ~3e-9 only, and a unit vector rotated by it is that far from unit length --
    // 2e-7 N at 56 N of tension, which the balance of a converged problem (|e| <= 5e-6 N) would see.
#pragma clang fp contract(off)
    const double *__restrict__ rb = in.tip_route;
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
    if (live) {
#pragma unroll
      for (int r = 0; r < 3; r++) {
        in.res[(int64_t)r * in.ldr + i] = (nw[r] - Ft[r]) - in.wrench[ic * in.wrench_ld + r];
        in.res[(int64_t)(3 + r) * in.ldr + i] = (mw[r] - Lt[r]) - in.wrench[ic * in.wrench_ld + 3 + r];
      }
    }
  }
  if (live) {
    if (out.L) out.L[i] = Lb;
    if (out.Li) {
#pragma unroll
      for (int j = 0; j < N; j++) out.Li[(int64_t)j * ld + i] = Li[j];
    }
    if (out.n_points) out.n_points[i] = K.n_points;
    if (in.vu_tip) {
#pragma unroll
      for (int q = 0; q < 3; q++) { in.vu_tip[i * 6 + q] = v[q]; in.vu_tip[i * 6 + 3 + q] = u[q]; }
    }
  }
