// routing_form.hpp -- host side of the tendon routing of the shared arc-length grid: the row of the routing table at one
// abscissa, and the one decision per context which form of the right-hand side the robot's unloaded shared-grid kernels take
// (fk_kernel.hpp: TableRouting | UniformHelix).  No HIP header: tests/cpp/routing_form_test.cpp drives it with plain g++.
#pragma once
#include <cmath>
#include <cstring>
#include "tr_types.hpp"

namespace routing_form {

// a robot's routing polynomials: theta_j(t) = sum C[j n_a + i] t^i, rho_j(t) = sum D[j n_m + i] t^i (tendon/TendonSpecs.h:26-27)
struct Spec {
  int n_tendons, n_a, n_m;
  const double *C, *D;
  bool enable_retraction;
};

struct Form {
  int form;                   // TRK_ROUTING_TABLE | TRK_ROUTING_HELIX
  double omega, rho;          // the pitch and the radius every tendon shares (helix form only; 0 otherwise)
};

// {rx, ry, rdx, rdy, rddx, rddy} of every tendon at t: r = rho (sin theta, cos theta) and its first two derivatives
// (tendon/get_r_info.cpp:105-144); out: [n_tendons][6]
inline void row(const Spec &s, double t, double *out) {
  const int N_a = s.n_a, N_m = s.n_m, N_s = N_a > N_m ? N_a : N_m;
  double S[TRK_MAX_COEF], Sd[TRK_MAX_COEF], Sdd[TRK_MAX_COEF];
  S[0] = 1; Sd[0] = 0; Sdd[0] = 0;
  if (N_s >= 2) { S[1] = t; Sd[1] = 1; Sdd[1] = 0; }
  for (int i = 2; i < N_s; i++) { S[i] = t * S[i - 1]; Sd[i] = i * S[i - 1]; Sdd[i] = i * (i - 1) * S[i - 2]; }
  for (int j = 0; j < s.n_tendons; j++) {
    const double *Cj = s.C + (size_t)j * N_a, *Dj = s.D + (size_t)j * N_m;
    double C_a = 0, C_ad = 0, C_add = 0, D_m = 0, D_md = 0, D_mdd = 0;
    for (int i = 0; i < N_a; i++) { C_a += Cj[i] * S[i]; C_ad += Cj[i] * Sd[i]; C_add += Cj[i] * Sdd[i]; }
    for (int i = 0; i < N_m; i++) { D_m += Dj[i] * S[i]; D_md += Dj[i] * Sd[i]; D_mdd += Dj[i] * Sdd[i]; }
    const double sa = std::sin(C_a), ca = std::cos(C_a);
    double *o = out + 6 * j;
    o[0] = D_m * sa;
    o[1] = D_m * ca;
    o[2] = D_md * sa + D_m * (ca * C_ad);
    o[3] = D_md * ca + D_m * (-sa * C_ad);
    o[4] = D_mdd * sa + 2 * D_md * (ca * C_ad) - D_m * (sa * C_ad * C_ad) + D_m * (ca * C_add);
    o[5] = D_mdd * ca + 2 * D_md * (-sa * C_ad) - D_m * (ca * C_ad * C_ad) + D_m * (-sa * C_add);
  }
}

inline int degree(const double *c, int n) {
  for (int i = n - 1; i > 0; i--) if (std::fabs(c[i]) > 0.0) return i;
  return 0;
}

// Uniform helix: no retraction, every tendon of constant radius and at most linear angle, and ONE pitch and ONE radius on all
// tendons, compared bit for bit (exact comparisons, no tolerance: the identities the form relies on hold exactly or not at
// all); straight tendons are the pitch 0.  `forced` is the value of TENDON_HIP_ROUTING (null: unset): "table" keeps the table form.
// max_tendons: the widest robot the helix form is instantiated for (TRK_K1_TWO_WAVE_MAXN).
inline Form classify(const Spec &s, const char *forced, int max_tendons) {
  const Form table{TRK_ROUTING_TABLE, 0.0, 0.0};
  if (forced && std::strcmp(forced, "table") == 0) return table;
  if (s.enable_retraction || s.n_tendons < 1 || s.n_tendons > max_tendons) return table;
  const double omega = s.n_a > 1 ? s.C[1] : 0.0, rho = s.D[0];
  if (!std::isfinite(omega) || !std::isfinite(rho)) return table;
  for (int j = 0; j < s.n_tendons; j++) {
    const double *Cj = s.C + (size_t)j * s.n_a, *Dj = s.D + (size_t)j * s.n_m;
    if (degree(Dj, s.n_m) != 0 || degree(Cj, s.n_a) > 1) return table;
    const double w = s.n_a > 1 ? Cj[1] : 0.0;
    if (std::memcmp(&w, &omega, sizeof(double)) != 0 || std::memcmp(&Dj[0], &rho, sizeof(double)) != 0) return table;
  }
  return Form{TRK_ROUTING_HELIX, omega, rho};
}

}  // namespace routing_form
