// The dense algebra the LM step kernels share (csrc/lm_dense.hpp) on its own, compiled for the host without contraction: no
// device, no library.  u = 2^-53.
//   (a) chol_solve_packed<S>, S = 1, 3, 6, 10, on A = J^T J + mu I with J 3 x S, entries over five decades: the normwise backward
//       error |A y - g|_inf / (|A|_inf |y|_inf + |g|_inf) is at most S (3 S + 1) u (Higham, Accuracy and Stability of Numerical
//       Algorithms, 2nd ed., theorem 10.4 with the substitutions: |dA| <= gamma_{3n+1} |R^T| |R|, and | |R^T| |R| |_inf <= n |A|_inf);
//   (b) a matrix with a negative eigenvalue: spd == false and no NaN in y;
//   (c) lu6_factor / lu6_solve on 6 x 6 matrices with a zero diagonal (every column pivots): the same backward error is at most
//       3 n u 2^(n-1) = 18 * 32 u (Higham, theorem 9.5 with the worst growth factor of partial pivoting at n = 6);
//   (d) a zero column: singular == true;
//   (e) the cyclic permutation matrix, worked by hand: A x = b has x = (b_5, b_0, ..., b_4), exactly;
//   (f) the 3 x S helpers and canonical_angle on values worked by hand.
// The residuals are formed in long double, so that their own rounding does not count.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>

#include "lm_dense.hpp"

namespace {

using namespace trk;

int failures = 0;
#define CHECK(c)                                                            \
  do {                                                                      \
    if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); failures++; } \
  } while (0)

const double kU = std::ldexp(1.0, -53);
std::mt19937_64 rng(20240613);

double decades(double lo, double hi) {     // +- 10^uniform(lo, hi)
  std::uniform_real_distribution<double> e(lo, hi), s(-1.0, 1.0);
  return (s(rng) < 0.0 ? -1.0 : 1.0) * std::pow(10.0, e(rng));
}

// |M x - b|_inf / (|M|_inf |x|_inf + |b|_inf) of the n x n row-major M
template <int n>
double backward_error(const double (&M)[n * n], const double (&x)[n], const double (&b)[n]) {
  long double res = 0.0L, nm = 0.0L, nx = 0.0L, nb = 0.0L;
  for (int a = 0; a < n; a++) {
    long double r = -(long double)b[a], row = 0.0L;
    for (int c = 0; c < n; c++) { r += (long double)M[a * n + c] * x[c]; row += std::fabs((long double)M[a * n + c]); }
    res = std::fmax(res, std::fabs(r));
    nm = std::fmax(nm, row);
    nx = std::fmax(nx, std::fabs((long double)x[a]));
    nb = std::fmax(nb, std::fabs((long double)b[a]));
  }
  return (double)(res / (nm * nx + nb));
}

template <int S>
double cholesky_cases(int cases) {
  double worst = 0.0;
  for (int t = 0; t < cases; t++) {
    double J[3 * S], full[S * S], A[S * (S + 1) / 2], g[S], y[S];
    for (double &v : J) v = decades(-3.0, 2.0);
    double dmax = 0.0;
    for (int a = 0; a < S; a++) {
      for (int b = 0; b <= a; b++) {
        const double s = J[0 * S + a] * J[0 * S + b] + J[1 * S + a] * J[1 * S + b] + J[2 * S + a] * J[2 * S + b];
        full[a * S + b] = full[b * S + a] = s;
      }
      dmax = std::fmax(dmax, full[a * S + a]);
    }
    const double mu = std::fabs(decades(-6.0, 0.0)) * dmax;
    for (int a = 0; a < S; a++) {
      full[a * S + a] += mu;
      for (int b = 0; b <= a; b++) A[a * (a + 1) / 2 + b] = full[a * S + b];
      g[a] = decades(-3.0, 2.0);
    }
    const bool spd = chol_solve_packed<S>(A, g, y);
    CHECK(spd);
    const double err = backward_error<S>(full, y, g);
    CHECK(err <= S * (3 * S + 1) * kU);
    worst = std::fmax(worst, err);
  }
  return worst;
}

void cholesky_refuses_an_indefinite_matrix() {
  // [1 2 0; 2 1 0; 0 0 1]: eigenvalues -1, 3, 1
  double A[6] = {1.0, 2.0, 1.0, 0.0, 0.0, 1.0}, y[3];
  const double g[3] = {1.0, -2.0, 3.0};
  CHECK(!chol_solve_packed<3>(A, g, y));
  for (double v : y) CHECK(std::isfinite(v));
  double B[1] = {-4.0}, z[1];
  const double h[1] = {2.0};
  CHECK(!chol_solve_packed<1>(B, h, z));
  CHECK(z[0] == 2.0);                              // the pivot's place is taken by 1
}

double lu_cases(int cases) {
  double worst = 0.0;
  for (int t = 0; t < cases; t++) {
    double M[36], A[36], b[6], x[6];
    int piv[6];
    for (int a = 0; a < 6; a++) {
      for (int c = 0; c < 6; c++) A[a * 6 + c] = M[a * 6 + c] = a == c ? 0.0 : decades(-2.0, 2.0);
      x[a] = b[a] = decades(-3.0, 2.0);
    }
    CHECK(!lu6_factor(A, piv));
    CHECK(piv[0] != 0);                            // the zero on the diagonal is never the pivot
    lu6_solve(A, piv, x);
    const double err = backward_error<6>(M, x, b);
    CHECK(err <= 18.0 * 32.0 * kU);
    worst = std::fmax(worst, err);
  }
  return worst;
}

void lu_flags_a_zero_column() {
  double A[36];
  int piv[6];
  for (int a = 0; a < 6; a++)
    for (int c = 0; c < 6; c++) A[a * 6 + c] = c == 2 ? 0.0 : decades(-1.0, 1.0);
  CHECK(lu6_factor(A, piv));
}

void lu_solves_a_permutation_exactly() {
  // row a holds its 1 in column (a + 1) mod 6: (A x)_a = x_{a+1}, so x_{a+1} = b_a and x_0 = b_5
  double A[36] = {}, x[6] = {1.0, 2.0, 3.0, 4.0, 5.0, 6.0};
  int piv[6];
  for (int a = 0; a < 6; a++) A[a * 6 + (a + 1) % 6] = 1.0;
  CHECK(!lu6_factor(A, piv));
  lu6_solve(A, piv, x);
  const double want[6] = {6.0, 1.0, 2.0, 3.0, 4.0, 5.0};
  for (int a = 0; a < 6; a++) CHECK(x[a] == want[a]);
}

void small_helpers() {
  // J = [1 2; 3 4; 5 6], e = (1, 1, 1): g = (9, 12)
  const double J[6] = {1.0, 2.0, 3.0, 4.0, 5.0, 6.0}, e[3] = {1.0, 1.0, 1.0};
  double g[2];
  lm_grad<2>(J, e, g);
  CHECK(g[0] == 9.0 && g[1] == 12.0);
  IkParams prm{};
  prm.eps1 = 10.0;
  prm.lo[0] = prm.lo[1] = 0.0;
  prm.hi[0] = prm.hi[1] = 1.0;
  const double inside[2] = {0.5, 0.5}, at_hi[2] = {0.5, 1.0}, at_lo[2] = {0.5, 0.0};
  CHECK(lm_moving<2>(inside, g, prm));             // max |g| = 12 > 10
  CHECK(!lm_moving<2>(at_hi, g, prm));             // g_1 > 0 pushes out of the box at its upper bound: 9 is left
  CHECK(lm_moving<2>(at_lo, g, prm));              // ... and into the box at its lower bound
  // dp = (1, 1) from p = 0, mu = 2: predicted decrease 1 (2 + 9) + 1 (2 + 12) = 25; actual 50 - 25
  const double x[2] = {1.0, 1.0}, p[2] = {0.0, 0.0};
  CHECK(lm_gain_ratio<2>(x, p, g, 2.0, 50.0, 25.0) == 1.0);
  const double back[2] = {-9.0, -12.0};
  CHECK(lm_gain_ratio<2>(x, p, back, 2.0, 50.0, 25.0) == -1.0);
  CHECK(lm_shrink(1.0) == 1.0 / 3.0 && lm_shrink(-1.0) == 2.0);
  double mu = 3.0, nu = 2.0;
  lm_reject(mu, nu);
  CHECK(mu == 6.0 && nu == 4.0);
  CHECK(ik_clip(2.0, 0.0, 1.0) == 1.0 && ik_clip(-2.0, 0.0, 1.0) == 0.0 && ik_clip(0.25, 0.0, 1.0) == 0.25);
  const double pi = 3.141592653589793;
  CHECK(canonical_angle(pi) == -pi && canonical_angle(0.25) == 0.25);
  CHECK(std::fabs(canonical_angle(3.0 * pi + 0.25) - (-pi + 0.25)) < 1e-12);
}

}  // namespace

int main() {
  const double c1 = cholesky_cases<1>(2000), c3 = cholesky_cases<3>(2000), c6 = cholesky_cases<6>(2000), c10 = cholesky_cases<10>(2000);
  cholesky_refuses_an_indefinite_matrix();
  const double lu = lu_cases(4000);
  lu_flags_a_zero_column();
  lu_solves_a_permutation_exactly();
  small_helpers();
  std::printf("worst backward error / u: cholesky S=1 %.2f, 3 %.2f, 6 %.2f, 10 %.2f; lu %.2f\n", c1 / kU, c3 / kU, c6 / kU, c10 / kU, lu / kU);
  if (failures) return 1;
  std::printf("lm dense ok\n");
  return 0;
}
