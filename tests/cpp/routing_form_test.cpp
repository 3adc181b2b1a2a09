// The one decision per context which routing form a robot's unloaded shared-grid kernels take (csrc/routing_form.hpp), on its own:
// no device, no library.
//   (a) config 2 (three helical tendons, one pitch, one radius) -> uniform helix, omega = 5, rho = 0.01;
//   (b) three straight tendons -> uniform helix, omega = 0;
//   (c) config 3 (quadratic angle, linear radius), two pitches, two radii, a retraction robot, a robot wider than the form is
//       instantiated for -> table;
//   (d) TENDON_HIP_ROUTING=table -> table for config 2 (any other value: no effect);
//   (e) the sign convention: for the robots classified as helix every row of the host routing table satisfies
//       r'_x = omega r_y, r'_y = -omega r_x and r_x^2 + r_y^2 = rho^2 to within 4 ulp of the larger side, at the stage abscissae
//       of the 128-step grid.
#include <cmath>
#include <cstdio>
#include <vector>

#include "routing_form.hpp"

namespace {

int failures = 0;
#define CHECK(c)                                                            \
  do {                                                                      \
    if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } \
  } while (0)

constexpr double kPi = 3.14159265358979323846;
constexpr int kMaxN = TRK_K1_TWO_WAVE_MAXN;

struct Robot {
  int N, n_a, n_m;
  std::vector<double> C, D;
  bool retraction = false;
  routing_form::Spec spec() const { return routing_form::Spec{N, n_a, n_m, C.data(), D.data(), retraction}; }
};

Robot helix(int N, double omega, double rho) {
  Robot r{N, 2, 1, {}, {}};
  for (int k = 0; k < N; k++) { r.C.push_back(2 * kPi * k / N); r.C.push_back(omega); r.D.push_back(rho); }
  return r;
}
Robot straight(int N) {
  Robot r{N, 1, 1, {}, {}};
  for (int k = 0; k < N; k++) { r.C.push_back(2 * kPi * k / N); r.D.push_back(0.01); }
  return r;
}
Robot config3() {
  const double c1[4] = {3.0, -2.0, 4.0, -5.0}, c2[4] = {10.0, 15.0, -12.0, 8.0}, d1[4] = {-0.01, 0.005, 0.0, -0.005};
  Robot r{4, 3, 3, {}, {}};
  for (int k = 0; k < 4; k++) {
    r.C.push_back(kPi * k / 2); r.C.push_back(c1[k]); r.C.push_back(c2[k]);
    r.D.push_back(0.01); r.D.push_back(d1[k]); r.D.push_back(0.0);
  }
  return r;
}

bool within_ulps(double a, double b, int ulps) {
  const double big = std::fmax(std::fabs(a), std::fabs(b));
  if (big == 0.0) return true;
  const double ulp = std::nextafter(big, INFINITY) - big;
  return std::fabs(a - b) <= ulps * ulp;
}

// every row of the table tr_create builds for L = 0.2, dL = L / 128: the base row and three stage abscissae per step
void identities(const Robot &r, const routing_form::Form &f) {
  const double L = 0.2, dL = L / 128;
  std::vector<double> out((size_t)r.N * 6);
  double worst = 0.0;
  for (int k = 0; k < 128; k++)
    for (int q = 0; q < 3; q++) {
      const double t = k * dL + 0.5 * q * dL;
      routing_form::row(r.spec(), t, out.data());
      for (int j = 0; j < r.N; j++) {
        const double rx = out[6 * j], ry = out[6 * j + 1], rdx = out[6 * j + 2], rdy = out[6 * j + 3];
        CHECK(within_ulps(rdx, f.omega * ry, 4));
        CHECK(within_ulps(rdy, -f.omega * rx, 4));
        CHECK(within_ulps(rx * rx + ry * ry, f.rho * f.rho, 4));
        worst = std::fmax(worst, std::fabs(rx * rx + ry * ry - f.rho * f.rho) / (f.rho * f.rho));
      }
    }
  std::printf("  N=%d omega=%g: worst |rx^2 + ry^2 - rho^2| / rho^2 = %.3g\n", r.N, f.omega, worst);
}

}  // namespace

int main() {
  using routing_form::classify;
  {
    const Robot r = helix(3, 5.0, 0.01);                       // config 2
    const routing_form::Form f = classify(r.spec(), nullptr, kMaxN);
    CHECK(f.form == TRK_ROUTING_HELIX && f.omega == 5.0 && f.rho == 0.01);
    identities(r, f);
    CHECK(classify(r.spec(), "table", kMaxN).form == TRK_ROUTING_TABLE);
    CHECK(classify(r.spec(), "helix", kMaxN).form == TRK_ROUTING_HELIX);
    CHECK(classify(r.spec(), "", kMaxN).form == TRK_ROUTING_HELIX);
    Robot rr = r; rr.retraction = true;
    CHECK(classify(rr.spec(), nullptr, kMaxN).form == TRK_ROUTING_TABLE);
    Robot p2 = r; p2.C[2 * 1 + 1] = 4.0;                       // two pitches
    CHECK(classify(p2.spec(), nullptr, kMaxN).form == TRK_ROUTING_TABLE);
    Robot p3 = r; p3.C[2 * 2 + 1] = std::nextafter(5.0, 6.0);  // ... one ulp apart: the comparison is exact
    CHECK(classify(p3.spec(), nullptr, kMaxN).form == TRK_ROUTING_TABLE);
    Robot r2 = r; r2.D[1] = 0.012;                             // two radii
    CHECK(classify(r2.spec(), nullptr, kMaxN).form == TRK_ROUTING_TABLE);
    Robot r3 = r; r3.D[2] = std::nextafter(0.01, 1.0);
    CHECK(classify(r3.spec(), nullptr, kMaxN).form == TRK_ROUTING_TABLE);
  }
  {
    const Robot r = straight(3);
    const routing_form::Form f = classify(r.spec(), nullptr, kMaxN);
    CHECK(f.form == TRK_ROUTING_HELIX && f.omega == 0.0 && f.rho == 0.01);
    identities(r, f);
  }
  {
    const Robot r = helix(4, -3.0, 0.008);                     // four tendons, common (negative) pitch
    const routing_form::Form f = classify(r.spec(), nullptr, kMaxN);
    CHECK(f.form == TRK_ROUTING_HELIX && f.omega == -3.0 && f.rho == 0.008);
    identities(r, f);
  }
  {
    const Robot r = helix(1, 7.0, 0.01);
    const routing_form::Form f = classify(r.spec(), nullptr, kMaxN);
    CHECK(f.form == TRK_ROUTING_HELIX && f.omega == 7.0);
    identities(r, f);
  }
  {
    // the robots of the truth fixtures helix2, helix5, helix6 (tests/golden/make_fk_truth.py) and the common-pitch 7-tendon robot
    // of tests/test_gpu_rhs_helix.py: 2, 5 and 6 tendons take the helix form, 7 is wider than it is instantiated for
    const int n[3] = {2, 5, 6};
    const double omega[3] = {5.0, -4.0, 3.0};
    for (int q = 0; q < 3; q++) {
      const Robot r = helix(n[q], omega[q], 0.01);
      const routing_form::Form f = classify(r.spec(), nullptr, kMaxN);
      CHECK(f.form == TRK_ROUTING_HELIX && f.omega == omega[q] && f.rho == 0.01);
      identities(r, f);
      CHECK(classify(r.spec(), "table", kMaxN).form == TRK_ROUTING_TABLE);
    }
    const routing_form::Form f7 = classify(helix(7, 2.0, 0.01).spec(), nullptr, kMaxN);
    CHECK(kMaxN == 6 && f7.form == TRK_ROUTING_TABLE && f7.omega == 0.0 && f7.rho == 0.0);
  }
  {
    // polynomials padded with zero coefficients are what they are without the padding
    Robot r{3, 3, 2, {}, {}};
    for (int k = 0; k < 3; k++) { r.C.insert(r.C.end(), {2 * kPi * k / 3, 5.0, 0.0}); r.D.insert(r.D.end(), {0.01, 0.0}); }
    CHECK(classify(r.spec(), nullptr, kMaxN).form == TRK_ROUTING_HELIX);
    r.C[2] = 1e-300;                                           // any quadratic term at all: general
    CHECK(classify(r.spec(), nullptr, kMaxN).form == TRK_ROUTING_TABLE);
    r.C[2] = 0.0; r.D[1] = -1e-300;                            // any taper at all: general
    CHECK(classify(r.spec(), nullptr, kMaxN).form == TRK_ROUTING_TABLE);
  }
  CHECK(classify(config3().spec(), nullptr, kMaxN).form == TRK_ROUTING_TABLE);
  CHECK(classify(helix(kMaxN, 5.0, 0.01).spec(), nullptr, kMaxN).form == TRK_ROUTING_HELIX);
  CHECK(classify(helix(kMaxN + 1, 5.0, 0.01).spec(), nullptr, kMaxN).form == TRK_ROUTING_TABLE);   // no helix instantiation that wide
  if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
  std::printf("routing form ok\n");
  return 0;
}
