// fk_loaded_lin_body.inc -- the body of fk_loaded_lin and fk_loaded_lin_profile (fk_loaded_lin_kernel.hpp), which includes it once per
// form of the stage's load row (TRK_STAGE_ROW, fk_loaded_kernel.hpp).  A fragment, not a header: it stands between a kernel's braces
// and names the kernel's parameters and template arguments as they are spelt there --
//   template arguments  N, ROT
//   parameters          n, K, tab, steps, nsteps, in (LinIn; the profile form reads in.weights)
//   macro               TRK_STAGE_ROW(entry, fs, ls): declares the stage's row fs[3], ls[3] from fe, le of this body
// The fp-contract pragma below must be the first thing in the kernel's compound statement: the including kernel may put nothing
// but preprocessor lines between its opening brace and the #include.
#pragma clang fp contract(fast)
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
  const bool live = i < n;
  const int64_t il = live ? i : (n - 1);       // tail lanes recompute the last lane, stores masked
  const int64_t ir = il / in.Q;
  const int q = (int)(il - ir * in.Q);
  const int S = K.state_size;
  double tau[N], th = 0.0;
#pragma unroll
  for (int j = 0; j < N; j++) tau[j] = in.states[ir * S + j];
  if (ROT) th = in.states[ir * S + N];
  double v[3], u[3];
#pragma unroll
  for (int c = 0; c < 3; c++) { v[c] = in.vu[ir * 6 + c]; u[c] = in.vu[ir * 6 + 3 + c]; }
  double fe[3], le[3], Fe[3], Le[3];
  {
    // the lane's own point: -d on the odd lane of a pair, +d on the even one
#pragma clang fp contract(off)
    if (q >= 1 && q <= 12) {
      const int j = (q - 1) >> 1;
      const bool minus = (q & 1) != 0;
#pragma unroll
      for (int c = 0; c < 3; c++) {
        if (j == c) { const double d = in.delta_y; v[c] = minus ? v[c] - d : v[c] + d; }
        if (j == 3 + c) { const double d = in.delta_y; u[c] = minus ? u[c] - d : u[c] + d; }
      }
    } else if (q >= 13) {
      const int k = (q - 13) >> 1;
      const bool minus = ((q - 13) & 1) == 0;
#pragma unroll
      for (int j = 0; j < N; j++)
        if (k == j) { const double d = lin_step_size(tau[j], in.delta_p); tau[j] = minus ? tau[j] - d : tau[j] + d; }
      if (ROT && k == N) { const double d = lin_step_size(th, in.delta_p); th = minus ? th - d : th + d; }
    }
    double w6[6], d6[6];
    if (ROT && in.world) {
      double s, c;
      edge_sincos(th, s, c);
      edge_turn_row(in.wrench, s, c, w6);
      edge_turn_row(in.dist, s, c, d6);
    } else {
#pragma unroll
      for (int c = 0; c < 6; c++) { w6[c] = in.wrench[c]; d6[c] = in.dist[c]; }
    }
#pragma unroll
    for (int c = 0; c < 3; c++) { Fe[c] = w6[c]; Le[c] = w6[3 + c]; fe[c] = d6[c]; le[c] = d6[3 + c]; }
  }
  double rc = 1.0, rs = 0.0, r22 = 1.0;
  if (ROT) {
    rs = sin(th); rc = cos(th);
    r22 = (1.0 - rc) + rc;
  }

  double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};   // column-major: R[c*3+r]
  double p[3] = {0, 0, 0};

  for (int k = 0; k < nsteps; k++) {
    const double h = steps[k].h;
    const double *__restrict__ rt = tab + (size_t)(1 + 3 * k) * (N * 6);
    const double hh = h * 0.5;
    const double b1 = h * (1.0 / 6.0), b2 = h * (1.0 / 3.0);
    double aR[9], av[3], au[3];
#pragma unroll
    for (int c = 0; c < 3; c++) { av[c] = v[c]; au[c] = u[c]; }
    double sR[9], sv[3], su[3];
    double qs[3], qm[3];
#pragma unroll
    for (int c = 0; c < 9; c++) sR[c] = R[c];
#pragma unroll
    for (int c = 0; c < 3; c++) { sv[c] = v[c]; su[c] = u[c]; }

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
      double dR[9];
      frame_rate(st, sR, su, dR, aR);
#pragma unroll
      for (int c = 0; c < 3; c++) { av[c] += bw * dv[c]; au[c] += bw * du[c]; }
      if (st < 3) {
#pragma unroll
        for (int c = 0; c < 9; c++) sR[c] = R[c] + aw * dR[c];
#pragma unroll
        for (int c = 0; c < 3; c++) { sv[c] = v[c] + aw * dv[c]; su[c] = u[c] + aw * du[c]; }
      }
    }
#pragma unroll
    for (int c = 0; c < 9; c++) R[c] = __builtin_fma(b1, aR[c], R[c]);
#pragma unroll
    for (int c = 0; c < 3; c++) { v[c] = av[c]; u[c] = au[c]; }
  }

  {
    // the tip balance of fk_loaded_uniform, term for term
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
        in.out[(int64_t)r * in.ldr + i] = (nw[r] - Ft[r]) - Fe[r];
        in.out[(int64_t)(3 + r) * in.ldr + i] = (mw[r] - Lt[r]) - Le[r];
      }
    }
  }
  if (live) {
    double x = p[0], y = p[1], z = p[2];
    if (ROT) { const double x2 = __builtin_fma(rc, x, -(rs * y)), y2 = __builtin_fma(rs, x, rc * y); x = x2; y = y2; z = r22 * z; }
    in.out[(int64_t)6 * in.ldr + i] = x;
    in.out[(int64_t)7 * in.ldr + i] = y;
    in.out[(int64_t)8 * in.ldr + i] = z;
  }
