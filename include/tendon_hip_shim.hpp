// tendon_hip_shim.hpp -- header-only C++17 host shim over the C ABI (tendon_hip.h) that keeps the
// reference's class and method names for the hot path, so reference-side code can switch with a
// namespace alias.  STL only (the reference's Eigen / OMPL types are adapted in INTEGRATION.md).
//
//   tendon::TendonRobot / BackboneSpecs / TendonSpecs / TendonResult   tendon/*.h
//   collision::VoxelOctree (dense view)                                 collision/VoxelOctree.h:68-330
//   motion_planning::VoxelEnvironment                                   motion-planning/VoxelEnvironment.h:31-49
//   motion_planning::VoxelBackboneValidityChecker                       motion-planning/VoxelBackboneValidityChecker.h:28-58
//   motion_planning::VoxelValidityChecker                               motion-planning/VoxelValidityChecker.h:18-26
//   motion_planning::VoxelBackboneMotionValidator                       motion-planning/VoxelBackboneMotionValidator.h
//   motion_planning::VoxelBackboneDiscreteMotionValidator               motion-planning/VoxelBackboneDiscreteMotionValidator.h
//   motion_planning::VoxelCaches, voxelize_states, caches_collide       the cache loops of VoxelCachedLazyPRM.cpp
//   motion_planning::VoxelCachedLazyPRM                                  createRoadmap / precompute* (the build) and solveWithRoadmap
//                                                                        for a batch of queries (motion-planning/VoxelCachedLazyPRM.h:469-514)
//
// Error behaviour: every tr_status is rethrown as the C++ exception type the reference throws at
// the same condition (std::invalid_argument, std::out_of_range, std::domain_error,
// std::length_error, std::runtime_error).
#pragma once
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <limits>
#include <memory>
#include <optional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "tendon_hip.h"

namespace tendon_hip {

inline void check(const tr_ctx *ctx, int status) {
  if (status == TR_OK) return;
  const std::string msg = tr_last_error(ctx);
  switch (status) {
    case TR_ERR_INVALID_ARG: throw std::invalid_argument(msg);
    case TR_ERR_OUT_OF_RANGE: throw std::out_of_range(msg);
    case TR_ERR_DOMAIN: throw std::domain_error(msg);
    case TR_ERR_LENGTH: throw std::length_error(msg);
    default: throw std::runtime_error(msg);
  }
}

namespace detail {
// The library's sine and cosine for turning WORLD load rows (csrc/edge_sincos.hpp), restated: k = rint(x 2/pi), r = (x - k hi) -
// k lo, Taylor polynomials in Horner form -- the same IEEE operations in the same order, so the same bits (compile without
// floating-point contraction: the baseline x86-64 target has no fused multiply-add).
inline void edge_sincos(double x, double &s, double &c) {
  const double k = std::rint(x * 0.63661977236758138);
  const double r = (x - k * 1.57079632673412561417e+00) - k * 6.07710050650619224932e-11;
  const double z = r * r;
  static const double cs[8] = {1.0 / 355687428096000.0, -1.0 / 1307674368000.0, 1.0 / 6227020800.0, -1.0 / 39916800.0,
                               1.0 / 362880.0, -1.0 / 5040.0, 1.0 / 120.0, -1.0 / 6.0};
  static const double cc[9] = {-1.0 / 6402373705728000.0, 1.0 / 20922789888000.0, -1.0 / 87178291200.0, 1.0 / 479001600.0,
                               -1.0 / 3628800.0, 1.0 / 40320.0, -1.0 / 720.0, 1.0 / 24.0, -0.5};
  double ps = cs[0], pc = cc[0];
  for (int i = 1; i < 8; i++) ps = cs[i] + z * ps;
  for (int i = 1; i < 9; i++) pc = cc[i] + z * pc;
  const double sr = r + r * (z * ps), cr = 1.0 + z * pc;
  const int q = (int)((long long)k & 3);
  s = q == 0 ? sr : (q == 1 ? cr : (q == 2 ? -sr : -cr));
  c = q == 0 ? cr : (q == 1 ? -sr : (q == 2 ? -cr : sr));
}
// a load row (force, moment) turned by Rz(-theta): (x, y, z) -> (c x + s y, c y - s x, z)
inline void edge_turn_row(const double *w, double s, double c, double *o) {
  for (int h = 0; h < 2; h++) {
    o[3 * h + 0] = c * w[3 * h + 0] + s * w[3 * h + 1];
    o[3 * h + 1] = c * w[3 * h + 1] - s * w[3 * h + 0];
    o[3 * h + 2] = w[3 * h + 2];
  }
}
}  // namespace detail

namespace tendon {

struct BackboneSpecs {              // tendon/BackboneSpecs.h:14-20
  double L = 0.2, dL = 0.005, ro = 0.01, ri = 0.0, E = 2.1e6, nu = 0.3;
};

struct TendonSpecs {                // tendon/TendonSpecs.h:25-30
  std::vector<double> C{0.0}, D{0.01};
  double max_tension = 20.0, min_length = -0.015, max_length = 0.035;
};

struct TendonResult {               // tendon/TendonResult.h:17-40
  std::vector<double> t;
  std::vector<std::array<double, 3>> p;
  std::vector<std::array<double, 9>> R;   // column-major, as Eigen::Matrix3d stores it
  double L = 0.0;
  std::vector<double> L_i;
  bool converged = true;
  // base and tip strains; filled by general_shape (u_i, v_i: the solved base strains)
  std::array<double, 3> u_i{}, v_i{}, u_f{}, v_f{};
};

/// the arguments of TendonRobot::general_shape after the loads and the guess (tendon/TendonRobot.h:199-203)
struct ShootOptions {
  int max_iters = 100;
  double mu_init = 0.1, stop_threshold_JT_err_inf = 1e-9, stop_threshold_Dp = 1e-4, finite_difference_delta = 1e-6;
};

/// What tip_jacobian_loaded_batch returns: J n x 3 x S (d tip / d state), tips n x 3 and vu0 n x 6 (the tip and base strains
/// one Newton step past the shooting's stop), compliance n x 3 x 6 (d tip / d (F_e, L_e), the wrench as given), equilibrium n,
/// n_integrations n.  A state without an equilibrium has equilibrium = 0 and NaN in its rows.
struct LoadedTipJacobian {
  std::vector<double> J, tips, vu0, compliance;
  std::vector<uint8_t> equilibrium;
  std::vector<int64_t> n_integrations;
};
/// Arguments of tip_jacobian_loaded_batch after the loads: the shooting's, the state's difference step, the load's frame
struct LoadedJacobianOptions {
  ShootOptions shoot{};
  double delta = 1e-6;
  bool world = false;             // the load is fixed in the frame after the state's rotation (gravity), else before it
};

class TendonRobot {                 // tendon/TendonRobot.h:52-355
 public:
  double r = 0.015;
  BackboneSpecs specs{};
  std::vector<TendonSpecs> tendons;
  bool enable_rotation = false, enable_retraction = false;
  double residual_threshold = 5e-6;

  TendonRobot() = default;
  /// value semantics as in the reference; a copy gets its own GPU context on first use
  TendonRobot(const TendonRobot &o)
      : r(o.r), specs(o.specs), tendons(o.tendons), enable_rotation(o.enable_rotation), enable_retraction(o.enable_retraction),
        residual_threshold(o.residual_threshold) {}
  TendonRobot &operator=(const TendonRobot &o) {
    r = o.r; specs = o.specs; tendons = o.tendons; enable_rotation = o.enable_rotation; enable_retraction = o.enable_retraction;
    residual_threshold = o.residual_threshold; ctx_.reset();
    return *this;
  }

  size_t state_size() const { return tendons.size() + (enable_rotation ? 1 : 0) + (enable_retraction ? 1 : 0); }

  /// The GPU context holding this robot's constants; (re)created on first use on `device`.
  tr_ctx *context(int device = 0) const {
    if (!ctx_) {
      const size_t n = tendons.size();
      if (n == 0) throw std::out_of_range("tendons and tau are not the same length");
      const size_t na = tendons[0].C.size(), nm = tendons[0].D.size();
      std::vector<double> C, D, mt, mn, mx;
      for (auto &t : tendons) {
        if (t.C.size() != na || t.D.size() != nm) throw std::invalid_argument("tendons must share C.size() and D.size()");
        C.insert(C.end(), t.C.begin(), t.C.end());
        D.insert(D.end(), t.D.begin(), t.D.end());
        mt.push_back(t.max_tension); mn.push_back(t.min_length); mx.push_back(t.max_length);
      }
      tr_robot_desc d{};
      d.r = r; d.L = specs.L; d.dL = specs.dL; d.ro = specs.ro; d.ri = specs.ri; d.E = specs.E; d.nu = specs.nu;
      d.n_tendons = (int32_t)n; d.n_a = (int32_t)na; d.n_m = (int32_t)nm;
      d.C = C.data(); d.D = D.data(); d.max_tension = mt.data(); d.min_length = mn.data(); d.max_length = mx.data();
      d.enable_rotation = enable_rotation; d.enable_retraction = enable_retraction;
      d.residual_threshold = residual_threshold;
      tr_ctx *c = nullptr;
      check(nullptr, tr_create(&d, device, &c));
      ctx_ = std::shared_ptr<tr_ctx>(c, tr_destroy);
    }
    return ctx_.get();
  }

  /// TendonRobot::shape(state), TendonRobot.h:105-115
  TendonResult shape(const std::vector<double> &state) const {
    if (state.size() != state_size()) throw std::invalid_argument("State is not the right size");
    return std::move(shape_batch(state, 1)[0]);
  }

  /// Central-difference tip Jacobians of n states through tip_control's FK wrapper (tr_tip_jacobian): n x 3 x S row-major;
  /// `tips` (optional) receives f(p), n x 3
  std::vector<double> tip_jacobian_batch(const std::vector<double> &states, size_t n, double delta = 1e-6,
                                         std::vector<double> *tips = nullptr) const {
    const size_t S = state_size();
    if (states.size() != n * S) throw std::invalid_argument("State is not the right size");
    tr_ctx *c = context();
    std::vector<double> J(n * 3 * S);
    if (tips) tips->resize(3 * n);
    check(c, tr_tip_jacobian(c, states.data(), (int64_t)n, delta, tips ? tips->data() : nullptr, J.data()));
    return J;
  }

  /// forward_kinematics(state), TendonRobot.h:68-72
  std::vector<std::array<double, 3>> forward_kinematics(const std::vector<double> &state) const { return shape(state).p; }

  /// n shapes in one launch (the omp loop of apps/estimate_length_discretization.cpp:62-71)
  std::vector<TendonResult> shape_batch(const std::vector<double> &states, size_t n) const {
    tr_ctx *c = context();
    const size_t S = state_size(), P = (size_t)tr_num_points(c), N = tendons.size();
    if (states.size() != n * S) throw std::invalid_argument("State is not the right size");
    std::vector<double> p(n * P * 3), R(n * P * 9), L(n), Li(n * N);
    std::vector<uint8_t> conv(n);
    std::vector<int32_t> np(n);
    check(c, tr_fk_batch(c, states.data(), (int64_t)n, p.data(), R.data(), L.data(), Li.data(), conv.data(), np.data()));
    const std::vector<double> tg = t_grid();
    std::vector<TendonResult> out(n);
    for (size_t i = 0; i < n; i++) {
      TendonResult &res = out[i];
      const size_t m = (size_t)np[i];
      res.t.assign(tg.begin(), tg.begin() + m);
      res.p.resize(m); res.R.resize(m);
      for (size_t j = 0; j < m; j++) {
        for (int k = 0; k < 3; k++) res.p[j][k] = p[(i * P + j) * 3 + k];
        for (int k = 0; k < 9; k++) res.R[j][k] = R[(i * P + j) * 9 + k];
      }
      res.L = L[i];
      res.L_i.assign(Li.begin() + i * N, Li.begin() + (i + 1) * N);
      res.converged = conv[i] != 0;
    }
    return out;
  }

  using V3 = std::array<double, 3>;

  /// general_shape for n states in one call (tr_fk_loaded_batch): `wrench` holds (F_e, L_e) once (6 values) or per state (6 n);
  /// `dist` holds (f_e, l_e) the same way, or is empty; `guess` holds n rows (v, u) or is empty = start from the unloaded solution.
  /// Loads are in the base frame before the state's rotation.  iters / fk_calls (optional) receive the per-state counters.
  std::vector<TendonResult> generalShapeBatch(const std::vector<double> &states, size_t n, const std::vector<double> &wrench,
                                              const std::vector<double> &dist = {}, const std::vector<double> &guess = {},
                                              const ShootOptions &opt = ShootOptions(), std::vector<int32_t> *iters = nullptr,
                                              std::vector<int32_t> *fk_calls = nullptr) const {
    tr_ctx *c = context();
    const size_t S = state_size(), P = (size_t)tr_num_points(c), N = tendons.size();
    if (states.size() != n * S) throw std::invalid_argument("State is not the right size");
    if (wrench.size() != 6 && wrench.size() != 6 * n) throw std::invalid_argument("wrench: 6 values, or 6 per state");
    if (!dist.empty() && dist.size() != 6 && dist.size() != 6 * n) throw std::invalid_argument("dist: empty, 6 values, or 6 per state");
    if (!guess.empty() && guess.size() != 6 * n) throw std::invalid_argument("guess: empty, or 6 per state");
    const tr_shoot_params prm{opt.max_iters, opt.mu_init, opt.stop_threshold_JT_err_inf, opt.stop_threshold_Dp, opt.finite_difference_delta};
    std::vector<double> p(n * P * 3), R(n * P * 9), L(n), Li(n * N), vu0(6 * n), vuL(6 * n);
    std::vector<uint8_t> conv(n);
    std::vector<int32_t> np(n);
    if (iters) iters->resize(n);
    if (fk_calls) fk_calls->resize(n);
    // (a retraction-enabled robot: TR_ERR_UNSUPPORTED, rethrown as std::runtime_error, unless set_loaded_retraction() opened the
    // context to it; then every result has the state's own point count np[i], its points from row 0)
    check(c, tr_fk_loaded_batch(c, &prm, states.data(), (int64_t)n, wrench.data(), wrench.size() == 6 ? 0 : 6,
                                dist.empty() ? nullptr : dist.data(), dist.size() == 6 ? 0 : 6,
                                guess.empty() ? nullptr : guess.data(), p.data(), R.data(), L.data(), Li.data(), conv.data(), np.data(),
                                vu0.data(), vuL.data(), nullptr, iters ? iters->data() : nullptr, fk_calls ? fk_calls->data() : nullptr,
                                nullptr));
    const std::vector<double> tg = t_grid();
    std::vector<TendonResult> out(n);
    for (size_t i = 0; i < n; i++) {
      TendonResult &res = out[i];
      const size_t m = (size_t)np[i];
      if (enable_retraction) {
        // t_range(s_start, L, dL) spaces its abscissae from the tip: the shared grid's last m - 1 behind the state's own s_start
        res.t.assign(tg.end() - m, tg.end());
        res.t[0] = std::min(states[i * S + S - 1], specs.L);
      } else {
        res.t.assign(tg.begin(), tg.begin() + m);
      }
      res.p.resize(m); res.R.resize(m);
      for (size_t j = 0; j < m; j++) {
        for (int k = 0; k < 3; k++) res.p[j][k] = p[(i * P + j) * 3 + k];
        for (int k = 0; k < 9; k++) res.R[j][k] = R[(i * P + j) * 9 + k];
      }
      res.L = L[i];
      res.L_i.assign(Li.begin() + i * N, Li.begin() + (i + 1) * N);
      res.converged = conv[i] != 0;
      for (int k = 0; k < 3; k++) {
        res.v_i[k] = vu0[6 * i + k]; res.u_i[k] = vu0[6 * i + 3 + k];
        res.v_f[k] = vuL[6 * i + k]; res.u_f[k] = vuL[6 * i + 3 + k];
      }
    }
    return out;
  }

  /// tr_set_loaded_retraction: opens (or closes) this robot's context to LOADED shapes of a robot with retraction -- general_shape,
  /// generalShapeBatch and loaded_tips_batch then take it; the loaded calls above them keep throwing std::runtime_error.
  /// edges: the loaded edge checks as well (TR_LOADED_RETRACTION_EDGES) -- checkMotion of the motion validators on a checker of this
  /// robot after setLoads.  loaded_retraction() returns the level (0, 1 or 2).
  void set_loaded_retraction(bool on = true, bool edges = false) const {
    tr_ctx *c = context();
    check(c, tr_set_loaded_retraction(c, on ? (edges ? TR_LOADED_RETRACTION_EDGES : TR_LOADED_RETRACTION_FK) : TR_LOADED_RETRACTION_OFF));
  }
  int loaded_retraction() const { return tr_loaded_retraction(context()); }

  /// A load profile (tr_set_load_profile): the piecewise-linear weight w(arc length) over the knots (s[k], w[k]) that every loaded
  /// call of this robot's context applies to its distributed load from now on: general_shape, generalShapeBatch, the loaded tip
  /// Jacobian, IK and tips, and the loaded checks of a checker built on this robot.  The tip wrench is not scaled.  Knots that are
  /// not strictly increasing, a non-finite number or sizes that differ: std::invalid_argument; a retraction-enabled robot:
  /// std::runtime_error.
  void set_load_profile(const std::vector<double> &s, const std::vector<double> &w) const {
    if (s.size() != w.size()) throw std::invalid_argument("load profile: one weight per knot");
    tr_ctx *c = context();
    check(c, tr_set_load_profile(c, (int64_t)s.size(), s.data(), w.data()));
  }
  void clear_load_profile() const { tr_ctx *c = context(); check(c, tr_clear_load_profile(c)); }
  /// the installed table of weights at the RK4 stages' abscissae (tr_get_load_profile); empty: no profile installed
  std::vector<double> load_profile_table() const {
    tr_ctx *c = context();
    int64_t n = 0;
    check(c, tr_get_load_profile(c, nullptr, 0, &n));
    std::vector<double> out((size_t)n);
    if (n > 0) check(c, tr_get_load_profile(c, out.data(), n, &n));
    return out;
  }

  /// tip_jacobian_batch on the shapes of generalShapeBatch (tr_tip_jacobian_loaded): one shooting solve and 13 + 2 S integrations
  /// per state.  `wrench` holds (F_e, L_e), `dist` (f_e, l_e) per unit length, 6 values each or empty (zero), ONE set per call;
  /// `guess` holds n rows (v, u) or is empty.  rounds (optional): shooting rounds.
  LoadedTipJacobian tip_jacobian_loaded_batch(const std::vector<double> &states, size_t n, const std::vector<double> &wrench,
                                              const std::vector<double> &dist = {},
                                              const LoadedJacobianOptions &opt = LoadedJacobianOptions(),
                                              const std::vector<double> &guess = {}, int64_t *rounds = nullptr) const {
    const size_t S = state_size();
    if (states.size() != n * S) throw std::invalid_argument("State is not the right size");
    if ((!wrench.empty() && wrench.size() != 6) || (!dist.empty() && dist.size() != 6)) throw std::invalid_argument("loads: 6 values or none");
    if (!guess.empty() && guess.size() != 6 * n) throw std::invalid_argument("guess: empty, or 6 per state");
    tr_ctx *c = context();
    const tr_shoot_params prm{opt.shoot.max_iters, opt.shoot.mu_init, opt.shoot.stop_threshold_JT_err_inf, opt.shoot.stop_threshold_Dp,
                              opt.shoot.finite_difference_delta};
    tr_edge_loads ld{};
    for (size_t q = 0; q < wrench.size(); q++) ld.wrench[q] = wrench[q];
    for (size_t q = 0; q < dist.size(); q++) ld.dist[q] = dist[q];
    ld.frame = opt.world ? TR_LOAD_FRAME_WORLD : TR_LOAD_FRAME_BASE;
    LoadedTipJacobian out;
    out.J.resize(n * 3 * S); out.tips.resize(n * 3); out.vu0.resize(n * 6); out.compliance.resize(n * 18);
    out.equilibrium.resize(n); out.n_integrations.resize(n);
    // (a retraction-enabled robot: TR_ERR_UNSUPPORTED, rethrown as std::runtime_error)
    check(c, tr_tip_jacobian_loaded(c, &prm, (wrench.empty() && dist.empty()) ? nullptr : &ld, states.data(), (int64_t)n, opt.delta,
                                    guess.empty() ? nullptr : guess.data(), out.tips.data(), out.J.data(), out.compliance.data(), nullptr,
                                    out.vu0.data(), out.equilibrium.data(), nullptr, out.n_integrations.data(), rounds));
    return out;
  }

  struct LoadedTips {
    std::vector<double> tips;          // n x 3: fk_shape.p.back() of the loaded shapes
    std::vector<double> vu0;           // n x 6: the accepted base strains (v0, u0)
    std::vector<uint8_t> converged;    // the shooting reached the residual threshold
    int64_t rounds = 0, n_integrations = 0;
  };
  /// The tips of generalShapeBatch's shapes alone (tr_fk_loaded_tips: the shapes stay on the device), cold, under ONE load set as
  /// VoxelBackboneValidityChecker::setLoads holds it (checker.loads()): frame BASE gives every state the same rows, WORLD turns them
  /// by Rz(-theta) of the state's rotation with the library's own sine and cosine (detail::edge_sincos), so the rows are those of
  /// the loaded edge calls bit for bit.
  LoadedTips loaded_tips_batch(const std::vector<double> &states, size_t n, const tr_edge_loads &loads,
                               const ShootOptions &opt = ShootOptions()) const {
    const size_t S = state_size(), N = tendons.size();
    if (states.size() != n * S) throw std::invalid_argument("State is not the right size");
    tr_ctx *c = context();
    const tr_shoot_params prm{opt.max_iters, opt.mu_init, opt.stop_threshold_JT_err_inf, opt.stop_threshold_Dp, opt.finite_difference_delta};
    const bool turn = loads.frame == TR_LOAD_FRAME_WORLD && enable_rotation;
    std::vector<double> w(loads.wrench, loads.wrench + 6), d(loads.dist, loads.dist + 6);
    if (turn) {
      w.resize(6 * n); d.resize(6 * n);
      for (size_t i = 0; i < n; i++) {
        double s, co;
        detail::edge_sincos(states[i * S + N], s, co);
        detail::edge_turn_row(loads.wrench, s, co, &w[6 * i]);
        detail::edge_turn_row(loads.dist, s, co, &d[6 * i]);
      }
    }
    LoadedTips out;
    out.tips.resize(3 * n); out.vu0.resize(6 * n); out.converged.resize(n);
    int64_t r2[2] = {0, 0};
    // (a retraction-enabled robot: as in generalShapeBatch; opened, s_start >= L gives the origin)
    check(c, tr_fk_loaded_tips(c, &prm, states.data(), (int64_t)n, w.data(), turn ? 6 : 0, d.data(), turn ? 6 : 0, nullptr, out.tips.data(),
                               out.converged.data(), out.vu0.data(), r2));
    out.rounds = r2[0]; out.n_integrations = r2[1];
    return out;
  }

  /// TendonRobot::general_shape(state, f_e, l_e, F_e, L_e, u_guess, v_guess, max_iters, ...), TendonRobot.h:155-219, with two
  /// differences: f_e, l_e are constant vectors (per unit length, base frame), not functions of (t, p); and without a guess the
  /// shooting starts from the unloaded solution of the tensions, where the reference starts from the straight rod -- pass
  /// u_guess = {0, 0, 0}, v_guess = {0, 0, 1} for that.  `verbose` is accepted and ignored.
  TendonResult general_shape(const std::vector<double> &state, const V3 &f_e, const V3 &l_e, const V3 &F_e, const V3 &L_e,
                             const std::optional<V3> &u_guess = std::nullopt, const std::optional<V3> &v_guess = std::nullopt,
                             int max_iters = 100, double mu_init = 0.1, double stop_threshold_JT_err_inf = 1e-9,
                             double stop_threshold_Dp = 1e-4, double finite_difference_delta = 1e-6, bool verbose = false) const {
    (void)verbose;
    if (state.size() != state_size()) throw std::invalid_argument("State is not the right size");
    const std::vector<double> wrench{F_e[0], F_e[1], F_e[2], L_e[0], L_e[1], L_e[2]}, dist{f_e[0], f_e[1], f_e[2], l_e[0], l_e[1], l_e[2]};
    std::vector<double> guess;
    if (u_guess || v_guess) {
      const V3 v = v_guess.value_or(V3{0.0, 0.0, 1.0}), u = u_guess.value_or(V3{0.0, 0.0, 0.0});
      guess = {v[0], v[1], v[2], u[0], u[1], u[2]};
    }
    const ShootOptions opt{max_iters, mu_init, stop_threshold_JT_err_inf, stop_threshold_Dp, finite_difference_delta};
    return std::move(generalShapeBatch(state, 1, wrench, dist, guess, opt)[0]);
  }

  /// home_shape(0).L_i, TendonRobot.cpp:249-314
  std::vector<double> home_lengths() const {
    std::vector<double> Li(tendons.size());
    check(context(), tr_home_lengths(context(), Li.data()));
    return Li;
  }

  std::vector<double> calc_dl(const std::vector<double> &home_l, const std::vector<double> &other_l) const {   // :247-259
    if (home_l.size() != other_l.size()) throw std::out_of_range("vector size mismatch");
    std::vector<double> dl(home_l.size());
    for (size_t i = 0; i < dl.size(); i++) dl[i] = home_l[i] - other_l[i];
    return dl;
  }
  bool is_within_length_limits(const std::vector<double> &dl) const {                                          // :268-278
    if (dl.size() != tendons.size()) throw std::out_of_range("length mismatch");
    for (size_t i = 0; i < dl.size(); i++)
      if (dl[i] < tendons[i].min_length || tendons[i].max_length < dl[i]) return false;
    return true;
  }

  /// util::range + t_range (TendonRobot.cpp:69-84) for s_start = 0: only to fill TendonResult::t
  std::vector<double> t_grid() const {
    std::vector<double> v;
    for (double q = 0.0; q <= specs.L - specs.dL / 2; q += specs.dL) v.push_back(q);
    v.push_back(specs.L);
    std::vector<double> t(v.size());
    for (size_t i = 0; i < v.size(); i++) t[v.size() - 1 - i] = specs.L - (v[i] - 0.0);
    return t;
  }

 private:
  mutable std::shared_ptr<tr_ctx> ctx_;
};

}  // namespace tendon

/// tip_control (tip-control/tip_control.h:27-107) on the device: the FK callback is the engine's own (tr_ik_batch)
namespace tip_control {

struct IKResult {                   // tip_control.h:40-46
  std::vector<double> state;        // solved robot state (rotation canonical in [-pi, pi))
  std::array<double, 3> tip{};      // achieved tip
  double error = 0.0;               // tip position error
  int iters = 0;                    // LM iterations
  int num_fk_calls = 0;             // forward-kinematics evaluations (a multiple of 2 S + 1)
};

struct Bounds {                     // tip_control.h:48-58
  std::vector<double> lower, upper;
  /// tip_control.cpp:160-185: tensions in [0, max_tension], rotation unbounded, retraction in [0, L]
  static Bounds from_robot(const tendon::TendonRobot &robot) {
    Bounds b;
    const size_t N = robot.tendons.size(), S = robot.state_size();
    b.lower.assign(S, 0.0); b.upper.assign(S, 0.0);
    for (size_t i = 0; i < N; i++) b.upper[i] = robot.tendons[i].max_tension;
    if (robot.enable_rotation) { b.lower[N] = std::numeric_limits<double>::lowest(); b.upper[N] = std::numeric_limits<double>::max(); }
    if (robot.enable_retraction) b.upper[S - 1] = robot.specs.L;
    return b;
  }
  void center_about_state(const std::vector<double> &state) {
    for (size_t i = 0; i < lower.size() && i < state.size(); i++) { lower[i] -= state[i]; upper[i] -= state[i]; }
  }
};

/// inverse_kinematics for n start states at once (rows of `initial_states`), to one goal (`des` of size 1) or one goal each
/// (size n); all problems advance together, one K1 launch per round.  `bounds` null = Bounds::from_robot.
inline std::vector<IKResult> inverse_kinematics_batch(const tendon::TendonRobot &robot, const std::vector<double> &initial_states, size_t n,
                                                      const std::vector<std::array<double, 3>> &des, int max_iters = 100,
                                                      double mu_init = 0.1, double stop_threshold_JT_err_inf = 1e-9,
                                                      double stop_threshold_Dp = 1e-4, double stop_threshold_err = 1e-4,
                                                      double finite_difference_delta = 1e-6, const Bounds *bounds = nullptr,
                                                      int64_t *rounds = nullptr) {
  const size_t S = robot.state_size();
  if (initial_states.size() != n * S) throw std::invalid_argument("State is not the right size");
  if (des.size() != 1 && des.size() != n) throw std::invalid_argument("one goal, or one goal per start state");
  if (bounds && (bounds->lower.size() != S || bounds->upper.size() != S)) throw std::invalid_argument("State is not the right size");
  tr_ctx *c = robot.context();
  const tr_ik_params prm{max_iters, mu_init, stop_threshold_JT_err_inf, stop_threshold_Dp, stop_threshold_err, finite_difference_delta};
  std::vector<double> d(3 * des.size()), st(n * S), tips(3 * n), err(n);
  for (size_t i = 0; i < des.size(); i++) for (int k = 0; k < 3; k++) d[3 * i + k] = des[i][k];
  std::vector<int32_t> iters(n), calls(n);
  check(c, tr_ik_batch(c, &prm, initial_states.data(), (int64_t)n, d.data(), des.size() == 1 ? 0 : 3,
                       bounds ? bounds->lower.data() : nullptr, bounds ? bounds->upper.data() : nullptr, st.data(), tips.data(),
                       err.data(), iters.data(), calls.data(), rounds));
  std::vector<IKResult> out(n);
  for (size_t i = 0; i < n; i++) {
    out[i].state.assign(st.begin() + i * S, st.begin() + (i + 1) * S);
    out[i].tip = {tips[3 * i], tips[3 * i + 1], tips[3 * i + 2]};
    out[i].error = err[i]; out[i].iters = iters[i]; out[i].num_fk_calls = calls[i];
  }
  return out;
}

/// tip_control::inverse_kinematics (tip_control.h:88-100) without the FKFunc: the engine's FK through tip_control's wrapper
inline IKResult inverse_kinematics(const tendon::TendonRobot &robot, const std::vector<double> &initial_state, const std::array<double, 3> &des,
                                   int max_iters = 100, double mu_init = 0.1, double stop_threshold_JT_err_inf = 1e-9,
                                   double stop_threshold_Dp = 1e-4, double stop_threshold_err = 1e-4,
                                   double finite_difference_delta = 1e-6, bool verbose = false) {
  (void)verbose;
  if (initial_state.size() != robot.state_size()) throw std::invalid_argument("State is not the right size");
  return inverse_kinematics_batch(robot, initial_state, 1, {des}, max_iters, mu_init, stop_threshold_JT_err_inf, stop_threshold_Dp,
                                  stop_threshold_err, finite_difference_delta)[0];
}

/// What inverseKinematicsLoaded* return per problem beyond IKResult: the base strains (v0, u0) of the returned state's equilibrium
/// (generalShape's guess for it) and whether the start reached one (false: error = inf, no iteration was made)
struct LoadedIKResult : IKResult {
  std::array<double, 6> vu0{};
  bool equilibrium = false;
};

/// Solver arguments of inverseKinematicsLoaded*: tip_control.h:88-100's, and the load's frame
struct LoadedIKOptions {
  int max_iters = 100;
  double mu_init = 0.1, stop_threshold_JT_err_inf = 1e-9, stop_threshold_Dp = 1e-4, stop_threshold_err = 1e-4, finite_difference_delta = 1e-6;
  bool world = false;               // the load is fixed in the frame after the state's rotation (gravity), else before it
  const Bounds *bounds = nullptr;   // null = Bounds::from_robot
};

/// inverse_kinematics with TendonRobot::general_shape as its FKFunc, for n start states at once (tr_ik_loaded_batch): `wrench` holds
/// (F_e, L_e), `dist` (f_e, l_e) per unit length, 6 values each or empty (zero), ONE set per call.  One goal (`des` of size 1) or one
/// per start.  rounds (optional): outer rounds, shooting rounds.
inline std::vector<LoadedIKResult> inverseKinematicsLoadedBatch(const tendon::TendonRobot &robot, const std::vector<double> &initial_states,
                                                                size_t n, const std::vector<std::array<double, 3>> &des,
                                                                const std::vector<double> &wrench, const std::vector<double> &dist,
                                                                const LoadedIKOptions &opt = LoadedIKOptions(), int64_t *rounds = nullptr) {
  const size_t S = robot.state_size();
  if (initial_states.size() != n * S) throw std::invalid_argument("State is not the right size");
  if (des.size() != 1 && des.size() != n) throw std::invalid_argument("one goal, or one goal per start state");
  if ((!wrench.empty() && wrench.size() != 6) || (!dist.empty() && dist.size() != 6)) throw std::invalid_argument("loads: 6 values or none");
  if (opt.bounds && (opt.bounds->lower.size() != S || opt.bounds->upper.size() != S)) throw std::invalid_argument("State is not the right size");
  tr_ctx *c = robot.context();
  const tr_ik_params prm{opt.max_iters, opt.mu_init, opt.stop_threshold_JT_err_inf, opt.stop_threshold_Dp, opt.stop_threshold_err,
                         opt.finite_difference_delta};
  tr_edge_loads ld{};
  for (size_t q = 0; q < wrench.size(); q++) ld.wrench[q] = wrench[q];
  for (size_t q = 0; q < dist.size(); q++) ld.dist[q] = dist[q];
  ld.frame = opt.world ? TR_LOAD_FRAME_WORLD : TR_LOAD_FRAME_BASE;
  std::vector<double> d(3 * des.size()), st(n * S), tips(3 * n), err(n), vu(6 * n);
  for (size_t i = 0; i < des.size(); i++) for (int k = 0; k < 3; k++) d[3 * i + k] = des[i][k];
  std::vector<int32_t> iters(n), calls(n);
  std::vector<uint8_t> eq(n);
  int64_t r2[2] = {0, 0};
  check(c, tr_ik_loaded_batch(c, &prm, nullptr, (wrench.empty() && dist.empty()) ? nullptr : &ld, initial_states.data(), (int64_t)n, d.data(),
                              des.size() == 1 ? 0 : 3, opt.bounds ? opt.bounds->lower.data() : nullptr,
                              opt.bounds ? opt.bounds->upper.data() : nullptr, nullptr, st.data(), tips.data(), err.data(), iters.data(),
                              calls.data(), vu.data(), eq.data(), r2));
  if (rounds) { rounds[0] = r2[0]; rounds[1] = r2[1]; }
  std::vector<LoadedIKResult> out(n);
  for (size_t i = 0; i < n; i++) {
    out[i].state.assign(st.begin() + i * S, st.begin() + (i + 1) * S);
    out[i].tip = {tips[3 * i], tips[3 * i + 1], tips[3 * i + 2]};
    out[i].error = err[i]; out[i].iters = iters[i]; out[i].num_fk_calls = calls[i];
    for (int q = 0; q < 6; q++) out[i].vu0[q] = vu[6 * i + q];
    out[i].equilibrium = eq[i] != 0;
  }
  return out;
}

/// ... for one start state
inline LoadedIKResult inverseKinematicsLoaded(const tendon::TendonRobot &robot, const std::vector<double> &initial_state,
                                              const std::array<double, 3> &des, const std::vector<double> &wrench,
                                              const std::vector<double> &dist, const LoadedIKOptions &opt = LoadedIKOptions()) {
  if (initial_state.size() != robot.state_size()) throw std::invalid_argument("State is not the right size");
  return inverseKinematicsLoadedBatch(robot, initial_state, 1, {des}, wrench, dist, opt)[0];
}

/// tip_control::damped_resolved_rate_update (tip_control.cpp:418-483) without the FKFunc: the next state for the tip displacement
/// v_times_dt.  The reference runs ONE Levenberg-Marquardt iteration towards fk(q) + v_times_dt with mu_init = lambda, all three
/// stop thresholds at 1e-9 and Bounds::from_robot centred on q; here that is the tip through tip_control's wrapper followed by
/// tr_ik_batch with max_iters = 1.  A step that LM rejects leaves the state where it is.  `verbose` is accepted and ignored.
inline std::vector<double> damped_resolved_rate_update(const tendon::TendonRobot &robot, const std::vector<double> &current_state,
                                                       const std::array<double, 3> &v_times_dt, double lambda = 0.1,
                                                       double finite_difference_delta = 1e-6, bool verbose = false) {
  (void)verbose;
  const size_t S = robot.state_size();
  if (current_state.size() != S) throw std::invalid_argument("State is not the right size");
  tr_ctx *c = robot.context();
  std::array<double, 3> tip{};
  if (robot.enable_retraction && current_state[S - 1] > robot.specs.L) {
    tip = {0.0, 0.0, robot.specs.L - current_state[S - 1]};           // tip_control.cpp:96-104
  } else {
    check(c, tr_fk_tips(c, current_state.data(), 1, tip.data(), nullptr));
  }
  const std::array<double, 3> des{tip[0] + v_times_dt[0], tip[1] + v_times_dt[1], tip[2] + v_times_dt[2]};
  return inverse_kinematics_batch(robot, current_state, 1, {des}, 1, lambda, 1e-9, 1e-9, 1e-9, finite_difference_delta)[0].state;
}

/// ... on the LOADED shape: the loaded tip and its strains from tr_tip_jacobian_loaded (one shooting solve), then tr_ik_loaded_batch
/// with max_iters = 1 from those strains.  opt.max_iters, mu_init and the stop thresholds are not read; opt.world is.
inline std::vector<double> damped_resolved_rate_updateLoaded(const tendon::TendonRobot &robot, const std::vector<double> &current_state,
                                                             const std::array<double, 3> &v_times_dt, const std::vector<double> &wrench,
                                                             const std::vector<double> &dist, double lambda = 0.1,
                                                             double finite_difference_delta = 1e-6,
                                                             const LoadedIKOptions &opt = LoadedIKOptions()) {
  const size_t S = robot.state_size();
  if (current_state.size() != S) throw std::invalid_argument("State is not the right size");
  tendon::LoadedJacobianOptions jo;
  jo.delta = finite_difference_delta; jo.world = opt.world;
  const auto at = robot.tip_jacobian_loaded_batch(current_state, 1, wrench, dist, jo);
  if (!at.equilibrium[0]) return current_state;
  tr_ctx *c = robot.context();
  const tr_ik_params prm{1, lambda, 1e-9, 1e-9, 1e-9, finite_difference_delta};
  tr_edge_loads ld{};
  for (size_t q = 0; q < wrench.size(); q++) ld.wrench[q] = wrench[q];
  for (size_t q = 0; q < dist.size(); q++) ld.dist[q] = dist[q];
  ld.frame = opt.world ? TR_LOAD_FRAME_WORLD : TR_LOAD_FRAME_BASE;
  const double des[3] = {at.tips[0] + v_times_dt[0], at.tips[1] + v_times_dt[1], at.tips[2] + v_times_dt[2]};
  std::vector<double> next(S);
  check(c, tr_ik_loaded_batch(c, &prm, nullptr, (wrench.empty() && dist.empty()) ? nullptr : &ld, current_state.data(), 1, des, 0, nullptr,
                              nullptr, at.vu0.data(), next.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
  return next;
}

}  // namespace tip_control

namespace collision {

/// Dense view of collision::VoxelOctree: what the engine consumes as the obstacle set.
class VoxelOctree {
 public:
  explicit VoxelOctree(size_t Ndim = 4) : N_(Ndim) {
    if (Ndim < 4 || Ndim > 512 || (Ndim & (Ndim - 1)))
      throw std::invalid_argument("unsupported voxel dimension: " + std::to_string(Ndim));     // VoxelOctree.cpp:113-115
    blocks_.assign((Ndim / 4) * (Ndim / 4) * (Ndim / 4), 0);
  }
  size_t Nx() const { return N_; }
  size_t Nbx() const { return N_ / 4; }
  void set_xlim(double lo, double hi) { set(0, lo, hi, "x"); }
  void set_ylim(double lo, double hi) { set(1, lo, hi, "y"); }
  void set_zlim(double lo, double hi) { set(2, lo, hi, "z"); }
  double dx() const { return (lim_[1] - lim_[0]) / N_; }
  double dy() const { return (lim_[3] - lim_[2]) / N_; }
  double dz() const { return (lim_[5] - lim_[4]) / N_; }
  const double *limits() const { return lim_; }
  static uint64_t bitmask(unsigned x, unsigned y, unsigned z) { return uint64_t(1) << (x * 16 + y * 4 + z); }   // :1501-1503
  uint64_t block(size_t bx, size_t by, size_t bz) const { return blocks_[(bx * Nbx() + by) * Nbx() + bz]; }
  void set_block(size_t bx, size_t by, size_t bz, uint64_t v) { blocks_[(bx * Nbx() + by) * Nbx() + bz] = v; }
  bool cell(size_t ix, size_t iy, size_t iz) const { return block(ix / 4, iy / 4, iz / 4) & bitmask(ix % 4, iy % 4, iz % 4); }
  bool set_cell(size_t ix, size_t iy, size_t iz) {                                                               // :256-265
    uint64_t &b = blocks_[((ix / 4) * Nbx() + iy / 4) * Nbx() + iz / 4];
    const uint64_t m = bitmask(ix % 4, iy % 4, iz % 4), old = b;
    b |= m;
    return old & m;
  }
  const std::vector<uint64_t> &blocks() const { return blocks_; }
  std::vector<uint64_t> &blocks() { return blocks_; }

 private:
  void set(int a, double lo, double hi, const char *name) {
    if (lo >= hi) throw std::length_error(std::string(name) + "limits must be positive in size");              // :152-177
    lim_[2 * a] = lo; lim_[2 * a + 1] = hi;
  }
  size_t N_;
  double lim_[6] = {0, 1, 0, 1, 0, 1};
  std::vector<uint64_t> blocks_;
};

}  // namespace collision

namespace motion_planning {

struct VoxelEnvironment {           // motion-planning/VoxelEnvironment.h:46-49 (fields the hot path reads)
  double inv_rotation[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};   // row-major
};

/// VoxelBackboneValidityChecker: isValid(state) and its batched form.
class VoxelBackboneValidityChecker {
 public:
  VoxelBackboneValidityChecker(const tendon::TendonRobot &robot, const VoxelEnvironment &venv,
                               const collision::VoxelOctree &voxels, int device = 0, int checker = TR_CHECKER_BACKBONE)
      : robot_(robot), ctx_(robot.context(device)) {
    check(ctx_, tr_set_checker(ctx_, checker));
    // throws std::invalid_argument when robot.specs.dL exceeds the largest voxel edge (VoxelBackboneValidityChecker.h:37-45)
    check(ctx_, tr_set_grid(ctx_, (uint32_t)voxels.Nx(), voxels.limits(), voxels.blocks().data(), venv.inv_rotation));
  }
  const tendon::TendonRobot &robot() const { return robot_; }

  /// AbstractValidityChecker::isValid on a robot state (AbstractValidityChecker.cpp:124-133)
  bool isValid(const std::vector<double> &robot_state) const {
    if (robot_state.size() != robot_.state_size()) throw std::invalid_argument("State is not the right size");
    uint64_t bits = 0;
    check(ctx_, tr_validate_batch(ctx_, robot_state.data(), 1, &bits, nullptr, nullptr));
    return bits & 1u;
  }

  /// n states in one K1 + K2 pass; tips (optional) receive fk_shape.p.back()
  std::vector<bool> isValidBatch(const std::vector<double> &states, size_t n, std::vector<double> *tips = nullptr,
                                 std::vector<uint8_t> *flags = nullptr) const {
    if (states.size() != n * robot_.state_size()) throw std::invalid_argument("State is not the right size");
    std::vector<uint64_t> bits((n + 63) / 64);
    if (tips) tips->resize(3 * n);
    if (flags) flags->resize(n);
    check(ctx_, tr_validate_batch(ctx_, states.data(), (int64_t)n, bits.data(), tips ? tips->data() : nullptr,
                                  flags ? flags->data() : nullptr));
    std::vector<bool> out(n);
    for (size_t i = 0; i < n; i++) out[i] = (bits[i >> 6] >> (i & 63)) & 1u;
    return out;
  }
  tr_ctx *context() const { return ctx_; }

  // ---- loads: AbstractValidityChecker::set_fk_func with TendonRobot::general_shape under a load
  // (apps/profile_chained_plan.cpp:407-451).  Once set, the motion validators on this checker take every FK sample from the
  // loaded FK (tr_validate_edges_loaded*); clearLoads() restores the unloaded checks. ----
  /// wrench = (F_e, L_e), dist = (f_e, l_e) per unit length, 6 values each (empty: zero); world: the loads are fixed behind the
  /// state's rotation (every sample's rows are turned by Rz(-theta)), else before it (tr_fk_loaded_batch's frame)
  /// A robot with retraction: std::runtime_error unless its context is open to the loaded edge checks
  /// (robot.set_loaded_retraction(true, true)) -- the motion validators behind a loaded checker must be able to judge its edges.
  void setLoads(const std::vector<double> &wrench, const std::vector<double> &dist, bool world = false, bool warm_start = false) {
    check_load_sizes(wrench, dist);
    check_retraction_open();
    if (has_profile_) check(ctx_, tr_clear_load_profile(ctx_));     // (a profile belongs to the setLoads that gave it)
    has_profile_ = false;
    store_loads(wrench, dist, world, warm_start);
  }
  /// the same with a load profile (tr_set_load_profile) on `dist`: the weight w(arc length) over the knots (profile_s[k],
  /// profile_w[k]), installed on this checker's context until clearLoads() or the next setLoads.  A call that throws (sizes, bad
  /// knots: std::invalid_argument; a retraction robot: std::runtime_error) leaves the checker's loads and profile as they were: the
  /// profile is checked and installed before the load set is replaced.
  void setLoads(const std::vector<double> &wrench, const std::vector<double> &dist, const std::vector<double> &profile_s,
                const std::vector<double> &profile_w, bool world = false, bool warm_start = false) {
    if (profile_s.size() != profile_w.size()) throw std::invalid_argument("load profile: one weight per knot");
    check_load_sizes(wrench, dist);
    check_retraction_open();
    check(ctx_, tr_set_load_profile(ctx_, (int64_t)profile_s.size(), profile_s.data(), profile_w.data()));
    has_profile_ = true;
    store_loads(wrench, dist, world, warm_start);
  }
  void clearLoads() {
    has_loads_ = false;
    if (has_profile_) check(ctx_, tr_clear_load_profile(ctx_));
    has_profile_ = false;
  }
  /// true while a setLoads with a profile is in force
  bool hasLoadProfile() const { return has_profile_; }
  /// the load set, or nullptr when none is set
  const tr_edge_loads *loads() const { return has_loads_ ? &loads_ : nullptr; }

  // ---- edits of the obstacle set where it lives (collision::VoxelOctree's add_sphere / dilate* /
  // remove_interior, VoxelOctree.cpp:434-469, :533-952, as apps/prepare_voxel_env.cpp:269-315 applies them) ----
  /// VoxelOctree::add_capsule on the resident obstacle set (collision/VoxelOctree.cpp:471-515)
  void add_capsules(const std::vector<double> &capsules /* n x (ax, ay, az, bx, by, bz, r) */) const {
    check(ctx_, tr_grid_add_capsules(ctx_, capsules.data(), (int64_t)(capsules.size() / 7)));
  }
  void add_spheres(const std::vector<double> &spheres /* n x (cx, cy, cz, r) */) const {
    check(ctx_, tr_grid_add_spheres(ctx_, spheres.data(), (int64_t)(spheres.size() / 4)));
  }
  void dilate(int num = 1, bool use_diagonal = false) const { check(ctx_, tr_grid_dilate(ctx_, num, use_diagonal)); }
  void dilate_sphere(double r) const { check(ctx_, tr_grid_dilate_sphere(ctx_, r)); }
  void remove_interior(bool keep_diagonal = true) const { check(ctx_, tr_grid_remove_interior(ctx_, keep_diagonal)); }
  /// the obstacle set as it is on the device now, into a VoxelOctree of the same dimension
  void obstacles(collision::VoxelOctree &out) const { check(ctx_, tr_get_grid(ctx_, out.blocks().data())); }

  /// connectionStrategy_(v) for every state at once (VoxelCachedLazyPRM.cpp:1491-1502): the k nearest states
  /// (self included) in the compound state-space metric of Problem.cpp:112-152; idx is n x k, -1 = none in range
  void nearest_k(const std::vector<double> &states, size_t n, int k, std::vector<int32_t> &idx, std::vector<double> &dist,
                 double max_distance = 1e300) const {
    if (states.size() != n * robot_.state_size()) throw std::invalid_argument("State is not the right size");
    idx.resize(n * (size_t)k); dist.resize(n * (size_t)k);
    check(ctx_, tr_knn(ctx_, states.data(), (int64_t)n, k, max_distance, idx.data(), dist.data()));
  }

 private:
  const tendon::TendonRobot &robot_;
  tr_ctx *ctx_;
  tr_edge_loads loads_{};
  bool has_loads_ = false, has_profile_ = false;
  static void check_load_sizes(const std::vector<double> &wrench, const std::vector<double> &dist) {
    if ((!wrench.empty() && wrench.size() != 6) || (!dist.empty() && dist.size() != 6))
      throw std::invalid_argument("wrench and dist hold 6 values each: one load set");
  }
  void check_retraction_open() const {
    if (robot_.enable_retraction && tr_loaded_retraction(ctx_) < TR_LOADED_RETRACTION_EDGES)
      throw std::runtime_error("checker.setLoads: loaded FK (general_shape) is not built for robots with retraction in this call "
                               "(TendonRobot::set_loaded_retraction(true, true) opens the loaded edge checks)");
  }
  void store_loads(const std::vector<double> &wrench, const std::vector<double> &dist, bool world, bool warm_start) {
    loads_ = tr_edge_loads{};
    for (size_t q = 0; q < wrench.size(); q++) loads_.wrench[q] = wrench[q];
    for (size_t q = 0; q < dist.size(); q++) loads_.dist[q] = dist[q];
    loads_.frame = world ? TR_LOAD_FRAME_WORLD : TR_LOAD_FRAME_BASE;
    loads_.warm_start = warm_start ? 1 : 0;
    has_loads_ = true;
  }
};

/// VoxelValidityChecker (motion-planning/VoxelValidityChecker.h:18-26): the same interface; the robot is
/// voxelised as a sphere of its radius at every backbone point and tested against the raw environment.
/// The GPU context belongs to the TendonRobot object: give this checker its own copy of the robot if a
/// backbone checker on the same robot is alive at the same time.
class VoxelValidityChecker : public VoxelBackboneValidityChecker {
 public:
  VoxelValidityChecker(const tendon::TendonRobot &robot, const VoxelEnvironment &venv, const collision::VoxelOctree &voxels,
                       int device = 0)
      : VoxelBackboneValidityChecker(robot, venv, voxels, device, TR_CHECKER_SPHERES) {}
};

/// Sparse voxel set as the roadmap caches store it (VoxelCachedLazyPRM.h:165-179; CSR over items).
struct VoxelCaches {
  std::vector<int64_t> offsets{0};          // [items + 1]
  std::vector<uint32_t> block_ids;          // ((bx * Nb) + by) * Nb + bz
  std::vector<uint64_t> masks;              // bit x*16 + y*4 + z
  std::vector<bool> usable;                 // shape-valid vertex / fully valid edge
  size_t items() const { return offsets.size() - 1; }
};

namespace detail {
inline std::vector<bool> unpack(const std::vector<uint64_t> &bits, size_t n) {
  std::vector<bool> out(n);
  for (size_t i = 0; i < n; i++) out[i] = (bits[i >> 6] >> (i & 63)) & 1u;
  return out;
}
inline void fetch(tr_ctx *c, VoxelCaches &vc) {
  const size_t nnz = (size_t)vc.offsets.back();
  vc.block_ids.resize(nnz); vc.masks.resize(nnz);
  check(c, tr_voxelize_fetch(c, vc.block_ids.data(), vc.masks.data(), (int64_t)nnz));
}
}  // namespace detail

/// AbstractVoxelValidityChecker::voxelize for a batch of states (VoxelCachedLazyPRM.cpp:2816-2823):
/// the backbone voxel set of every shape-valid state, plus fk_shape.p.back() as the vertex tip.  After setLoads the shapes are the
/// loaded ones (tr_voxelize_batch_loaded).
inline VoxelCaches voxelize_states(const VoxelBackboneValidityChecker &vc, const std::vector<double> &states, size_t n,
                                   std::vector<double> *tips = nullptr) {
  if (states.size() != n * vc.robot().state_size()) throw std::invalid_argument("State is not the right size");
  VoxelCaches out;
  out.offsets.assign(n + 1, 0);
  std::vector<uint64_t> bits((n + 63) / 64);
  if (tips) tips->resize(3 * n);
  if (const tr_edge_loads *ld = vc.loads())               // the checker's FK is the loaded one (setLoads)
    check(vc.context(), tr_voxelize_batch_loaded(vc.context(), nullptr, ld, states.data(), (int64_t)n, out.offsets.data(), bits.data(),
                                                 tips ? tips->data() : nullptr, nullptr, nullptr));
  else
    check(vc.context(), tr_voxelize_batch(vc.context(), states.data(), (int64_t)n, out.offsets.data(), bits.data(),
                                          tips ? tips->data() : nullptr));
  out.usable = detail::unpack(bits, n);
  detail::fetch(vc.context(), out);
  return out;
}

/// obstacles.collides(*cached_voxels) for every cached item against the checker's current grid
/// (VoxelCachedLazyPRM.cpp:2397-2411, :2497-2509).
inline std::vector<bool> caches_collide(const VoxelBackboneValidityChecker &vc, const VoxelCaches &caches) {
  const size_t n = caches.items();
  std::vector<uint64_t> bits((n + 63) / 64);
  check(vc.context(), tr_check_cached(vc.context(), caches.block_ids.data(), caches.masks.data(), caches.offsets.data(),
                                      (int64_t)n, bits.data()));
  return detail::unpack(bits, n);
}

/// VoxelBackboneMotionValidator: checkMotion(s1, s2), checkMotion(s1, s2, last_valid), voxelize(a, b)
/// and their batched forms.
class VoxelBackboneMotionValidator {
 public:
  explicit VoxelBackboneMotionValidator(const VoxelBackboneValidityChecker &vc) : vc_(vc) {}
  virtual ~VoxelBackboneMotionValidator() = default;
  tr_space_params space{0.02, 0.01, 0.0001};      // Problem.h:59-62

  bool checkMotion(const std::vector<double> &a, const std::vector<double> &b) const {   // AbstractVoxelMotionValidator.h:143-151
    return checkMotionBatch(a, b, 1)[0];
  }
  /// AbstractVoxelMotionValidator.h:153-169: last_valid = (interpolate(a, b, t), t) with t = PartialVoxelization::t
  bool checkMotion(const std::vector<double> &a, const std::vector<double> &b,
                   std::pair<std::vector<double>, double> &last_valid) const {
    std::vector<double> t;
    const bool ok = checkMotionBatch(a, b, 1, nullptr, &t)[0];
    last_valid.second = t[0];
    last_valid.first = interpolate(a, b, t[0]);
    return ok;
  }
  std::vector<bool> checkMotionBatch(const std::vector<double> &a, const std::vector<double> &b, size_t n,
                                     std::vector<int32_t> *n_fk = nullptr, std::vector<double> *last_valid_t = nullptr) const {
    const size_t S = vc_.robot().state_size();
    if (a.size() != n * S || b.size() != n * S) throw std::invalid_argument("start and end are different sizes");
    std::vector<uint64_t> bits((n + 63) / 64);
    if (n_fk) n_fk->resize(n);
    if (last_valid_t) last_valid_t->resize(n);
    check(vc_.context(), run(a.data(), b.data(), (int64_t)n, bits.data(), n_fk ? n_fk->data() : nullptr,
                             last_valid_t ? last_valid_t->data() : nullptr));
    return detail::unpack(bits, n);
  }
  /// Roadmap form (the loops of VoxelCachedLazyPRM.cpp:1520-1542, :1621-1641): edge e joins rows edges[2e] and
  /// edges[2e + 1] of `states`; every vertex is evaluated once for all of its edges.
  std::vector<bool> checkMotionIndexed(const std::vector<double> &states, size_t n_states, const std::vector<int32_t> &edges,
                                       std::vector<int32_t> *n_fk = nullptr) const {
    if (states.size() != n_states * vc_.robot().state_size()) throw std::invalid_argument("State is not the right size");
    const size_t n = edges.size() / 2;
    std::vector<uint64_t> bits((n + 63) / 64);
    if (n_fk) n_fk->resize(n);
    if (const tr_edge_loads *ld = vc_.loads()) {            // the checker's FK is the loaded one (setLoads)
      check(vc_.context(), tr_validate_edges_loaded_indexed(vc_.context(), &space, nullptr, ld, states.data(), (int64_t)n_states, edges.data(),
                                                            (int64_t)n, bits.data(), n_fk ? n_fk->data() : nullptr, nullptr, nullptr, nullptr));
      return detail::unpack(bits, n);
    }
    check(vc_.context(), tr_validate_edges_indexed(vc_.context(), &space, states.data(), (int64_t)n_states, edges.data(), (int64_t)n,
                                                   bits.data(), n_fk ? n_fk->data() : nullptr, nullptr));
    return detail::unpack(bits, n);
  }
  /// AbstractVoxelMotionValidator::voxelize(a, b) for a batch of edges (VoxelCachedLazyPRM.cpp:2890-2898):
  /// the swept voxel set of every fully valid edge.
  VoxelCaches voxelizeBatch(const std::vector<double> &a, const std::vector<double> &b, size_t n) const {
    const size_t S = vc_.robot().state_size();
    if (a.size() != n * S || b.size() != n * S) throw std::invalid_argument("start and end are different sizes");
    VoxelCaches out;
    out.offsets.assign(n + 1, 0);
    std::vector<uint64_t> bits((n + 63) / 64);
    check(vc_.context(), tr_voxelize_edges(vc_.context(), &space, a.data(), b.data(), (int64_t)n, out.offsets.data(), bits.data(), nullptr));
    out.usable = detail::unpack(bits, n);
    detail::fetch(vc_.context(), out);
    return out;
  }
  /// The same for roadmap edges given as index pairs into one vertex array (VoxelCachedLazyPRM.cpp:1751-1775): every
  /// vertex is integrated and voxelised once for all of its edges.
  /// `validate`: also checkMotion on the same samples (tr_connect_edges_indexed): `usable` is then checkMotion's verdict and
  /// only accepted edges own a voxel set -- createRoadmap's connectVertices + voxelizeEdge in one traversal.
  VoxelCaches voxelizeIndexed(const std::vector<double> &states, size_t n_states, const std::vector<int32_t> &edges,
                              bool validate = false) const {
    if (states.size() != n_states * vc_.robot().state_size()) throw std::invalid_argument("State is not the right size");
    const size_t n = edges.size() / 2;
    VoxelCaches out;
    out.offsets.assign(n + 1, 0);
    std::vector<uint64_t> bits((n + 63) / 64);
    check(vc_.context(), indexed_lists(vc_, space, states.data(), (int64_t)n_states, edges.data(), (int64_t)n, validate, out.offsets.data(),
                                       bits.data(), nullptr));
    out.usable = detail::unpack(bits, n);
    detail::fetch(vc_.context(), out);
    return out;
  }
  /// tr_voxelize_edges_indexed / tr_connect_edges_indexed (validate), or after setLoads their loaded forms (n_unconverged and
  /// n_integrations, optional, are theirs; without loads they stay as they are)
  static int indexed_lists(const VoxelBackboneValidityChecker &vc, const tr_space_params &sp, const double *states, int64_t n_states,
                           const int32_t *edges, int64_t n, bool validate, int64_t *offsets, uint64_t *bits, int32_t *n_fk,
                           int64_t *n_unconverged = nullptr, int64_t *n_integrations = nullptr) {
    if (const tr_edge_loads *ld = vc.loads())             // the checker's FK is the loaded one (setLoads)
      return (validate ? tr_connect_edges_loaded_indexed : tr_voxelize_edges_loaded_indexed)(vc.context(), &sp, nullptr, ld, states, n_states, edges, n,
                                                                                             offsets, bits, n_fk, n_unconverged, n_integrations);
    return (validate ? tr_connect_edges_indexed : tr_voxelize_edges_indexed)(vc.context(), &sp, states, n_states, edges, n, offsets, bits, n_fk);
  }
  /// CompoundStateSpace::interpolate as wired by Problem.cpp:101-163: linear, shortest arc on the SO2 rotation
  std::vector<double> interpolate(const std::vector<double> &a, const std::vector<double> &b, double t) const {
    const auto &rb = vc_.robot();
    const size_t N = rb.tendons.size();
    std::vector<double> out(a.size());
    for (size_t i = 0; i < a.size(); i++) out[i] = a[i] + (b[i] - a[i]) * t;
    if (rb.enable_rotation) {
      const double kPi = 3.14159265358979323846;
      double diff = b[N] - a[N];
      if (std::fabs(diff) > kPi) {
        diff = diff > 0.0 ? 2.0 * kPi - diff : -2.0 * kPi - diff;
        double v = a[N] - diff * t;
        if (v > kPi) v -= 2.0 * kPi; else if (v < -kPi) v += 2.0 * kPi;
        out[N] = v;
      }
    }
    return out;
  }

 protected:
  virtual int run(const double *a, const double *b, int64_t n, uint64_t *bits, int32_t *n_fk, double *t) const {
    if (const tr_edge_loads *ld = vc_.loads())            // the checker's FK is the loaded one (setLoads)
      return tr_validate_edges_loaded(vc_.context(), &space, nullptr, ld, a, b, n, bits, t, n_fk, nullptr, nullptr, nullptr);
    if (t) return tr_validate_edges_last_valid(vc_.context(), &space, a, b, n, bits, t, n_fk);
    return tr_validate_edges(vc_.context(), &space, a, b, n, bits, n_fk, nullptr);
  }
  const VoxelBackboneValidityChecker &vc_;
};

/// VoxelBackboneDiscreteMotionValidator (motion-planning/VoxelBackboneDiscreteMotionValidator.cpp:9-79):
/// same interface, samples at a, i / validSegmentCount, b.
class VoxelBackboneDiscreteMotionValidator : public VoxelBackboneMotionValidator {
 public:
  using VoxelBackboneMotionValidator::VoxelBackboneMotionValidator;

 protected:
  int run(const double *a, const double *b, int64_t n, uint64_t *bits, int32_t *n_fk, double *t) const override {
    if (vc_.loads()) throw std::logic_error("the discrete motion validator is not built for loaded shapes (setLoads)");
    return tr_validate_edges_discrete(vc_.context(), &space, a, b, n, bits, t, n_fk);
  }
};

namespace detail {
inline std::vector<uint64_t> pack(const std::vector<bool> &b) {
  std::vector<uint64_t> w((b.size() + 63) / 64, 0);
  for (size_t i = 0; i < b.size(); i++) if (b[i]) w[i >> 6] |= (uint64_t)1 << (i & 63);
  return w;
}
/// n items without a cache
inline VoxelCaches empty_items(size_t n) {
  VoxelCaches c;
  c.offsets.assign(n + 1, 0);
  c.usable.assign(n, false);
  return c;
}
/// out item i = item keep[i] of c
inline VoxelCaches select_items(const VoxelCaches &c, const std::vector<size_t> &keep) {
  VoxelCaches out;
  out.offsets.assign(keep.size() + 1, 0);
  out.usable.resize(keep.size());
  for (size_t i = 0; i < keep.size(); i++) out.offsets[i + 1] = out.offsets[i] + (c.offsets[keep[i] + 1] - c.offsets[keep[i]]);
  out.block_ids.resize((size_t)out.offsets.back()); out.masks.resize((size_t)out.offsets.back());
  for (size_t i = 0; i < keep.size(); i++) {
    const size_t a = (size_t)c.offsets[keep[i]], b = (size_t)c.offsets[keep[i] + 1], o = (size_t)out.offsets[i];
    std::copy(c.block_ids.begin() + a, c.block_ids.begin() + b, out.block_ids.begin() + o);
    std::copy(c.masks.begin() + a, c.masks.begin() + b, out.masks.begin() + o);
    out.usable[i] = c.usable[keep[i]];
  }
  return out;
}
/// b's items after a's
inline void append_items(VoxelCaches &a, const VoxelCaches &b) {
  const int64_t base = a.offsets.back();
  for (size_t i = 0; i < b.items(); i++) a.offsets.push_back(base + b.offsets[i + 1]);
  a.block_ids.insert(a.block_ids.end(), b.block_ids.begin(), b.block_ids.begin() + b.offsets.back());
  a.masks.insert(a.masks.end(), b.masks.begin(), b.masks.begin() + b.offsets.back());
  a.usable.insert(a.usable.end(), b.usable.begin(), b.usable.end());
}
/// item idx[i] of dst becomes item i of src (idx ascending)
inline void replace_items(VoxelCaches &dst, const std::vector<size_t> &idx, const VoxelCaches &src) {
  if (idx.empty()) return;
  VoxelCaches out;
  out.offsets.assign(dst.items() + 1, 0);
  out.usable = dst.usable;
  std::vector<int64_t> from(dst.items(), -1);
  for (size_t i = 0; i < idx.size(); i++) from[idx[i]] = (int64_t)i;
  for (size_t v = 0; v < dst.items(); v++) {
    const VoxelCaches &c = from[v] < 0 ? dst : src;
    const size_t it = from[v] < 0 ? v : (size_t)from[v];
    out.offsets[v + 1] = out.offsets[v] + (c.offsets[it + 1] - c.offsets[it]);
    out.block_ids.insert(out.block_ids.end(), c.block_ids.begin() + c.offsets[it], c.block_ids.begin() + c.offsets[it + 1]);
    out.masks.insert(out.masks.end(), c.masks.begin() + c.offsets[it], c.masks.begin() + c.offsets[it + 1]);
    if (from[v] >= 0) out.usable[v] = src.usable[it];
  }
  dst = std::move(out);
}
}  // namespace detail

/// motion_planning::VoxelCachedLazyPRM (motion-planning/VoxelCachedLazyPRM.h:195-830) on the batched engine: the roadmap BUILD --
/// createRoadmap with its CreateRoadmapOption flags (.h:469-497, .cpp:1380-1561), precompute{Vertex,Edge}Validity (:1563-1648),
/// precompute{Vertex,Edge}VoxelCache (:1692-1789), clear*VoxelCache, clearDisconnectedVertices (:1665-1690), the connection
/// strategies (:1327-1364) -- as apps/create_roadmap.cpp:252-331 drives it, and the QUERY side: solveWithRoadmap (:1977-2096 ->
/// constructSolution :2689-2771) for a batch of (start, goal) roadmap vertices, clearValidity (:1656-1663), the eager
/// re-validation of every cached set.  The graph (states, edges, voxel sets, validity) lives in this object on the host and in
/// a tr_roadmap in HBM that is rebuilt when the graph was edited; every loop over vertices or edges is one batched call.
///
/// Differences a caller sees: vertices are numbered 0 .. milestoneCount() - 1 in creation order (the reference's indexProperty_);
/// new milestones come from ONE reproducible candidate sequence (seed, candidate index), not from thread-local OMPL samplers;
/// items found invalid by a query stay in the arrays with status 2 instead of leaving the graph (the searches skip them), and
/// clearValidity() makes them unknown again; queries name roadmap vertices (the reference adds start / goal states first).
class VoxelCachedLazyPRM {
 public:
  enum CreateRoadmapOption {             // VoxelCachedLazyPRM.h:469-482
    LazyRoadmap = 0x0, VoxelizeVertices = 0x1, ValidateVertices = 0x2, VoxelizeEdges = 0x4, ValidateEdges = 0x8
  };
  struct Solution { std::vector<int32_t> status; std::vector<double> cost; std::vector<std::vector<int32_t>> paths; tr_roadmap_stats stats; };
  /// what the last createRoadmap did: the candidate edges of the connection loop with checkMotion's verdict (or is_fully_valid)
  /// and the reference's count of FK evaluations per edge, the candidates consumed by the vertex phase
  struct BuildReport {
    std::vector<int32_t> candidate_edges; std::vector<bool> accepted; std::vector<int32_t> n_fk;
    int64_t candidates_tried = 0; std::vector<int64_t> candidate_index; int32_t k = 0; double max_distance = 0;
    /// a build under setLoads: shootings that did not converge (invalid candidates / samples) and integrations, vertex phase + edge phase
    int64_t n_unconverged = 0, n_integrations = 0;
  };

  /// a planner with an empty roadmap: createRoadmap / precompute* build it (`mv` supplies checkMotion and the space resolution)
  VoxelCachedLazyPRM(const VoxelBackboneValidityChecker &vc, const VoxelBackboneMotionValidator &mv, uint64_t seed = 0)
      : vc_(vc), mv_(&mv), S_(vc.robot().state_size()), seed_(seed) {
    vcache_ = detail::empty_items(0); ecache_ = detail::empty_items(0);
  }
  /// a loaded roadmap (fromRoadmapParser :2357-2580): states, edge index pairs, optional weights (NULL = state-space distance)
  VoxelCachedLazyPRM(const VoxelBackboneValidityChecker &vc, const std::vector<double> &states, size_t n_states,
                     const std::vector<int32_t> &edges, const std::vector<double> *weights = nullptr,
                     const VoxelBackboneMotionValidator *mv = nullptr)
      : vc_(vc), mv_(mv), S_(vc.robot().state_size()) {
    if (states.size() != n_states * S_) throw std::invalid_argument("State is not the right size");
    if (weights && weights->size() != edges.size() / 2) throw std::invalid_argument("one weight per edge");
    states_ = states; edges_ = edges;
    if (weights) weights_ = *weights;
    tips_.assign(3 * n_states, std::nan("")); has_tip_.assign(n_states, 0);
    vstat_.assign(n_states, 0); estat_.assign(edges.size() / 2, 0);
    vcache_ = detail::empty_items(n_states); ecache_ = detail::empty_items(edges.size() / 2);
    create_device_graph();                               // (an edge outside the roadmap throws here, as before)
  }
  ~VoxelCachedLazyPRM() { tr_roadmap_destroy(rm_); }
  VoxelCachedLazyPRM(const VoxelCachedLazyPRM &) = delete;
  VoxelCachedLazyPRM &operator=(const VoxelCachedLazyPRM &) = delete;

  // ---- the graph ----
  size_t milestoneCount() const { return vstat_.size(); }                       // .h:449
  size_t edgeCount() const { return estat_.size(); }                            // .h:452
  const std::vector<double> &states() const { return states_; }                 // milestoneCount() x state_size
  const std::vector<double> &tipPositions() const { return tips_; }             // x 3; NaN where tipPositionProperty_ is empty
  const std::vector<int32_t> &edges() const { return edges_; }                  // edgeCount() x 2
  const VoxelCaches &vertexVoxels() const { return vcache_; }                   // vertexVoxelsProperty_; usable[v] = has a cache
  const VoxelCaches &edgeVoxels() const { return ecache_; }
  const BuildReport &lastBuild() const { return report_; }
  /// 0 unknown, 1 VALIDITY_TRUE, 2 found invalid
  void validity(std::vector<uint8_t> &vertex_status, std::vector<uint8_t> &edge_status) { absorb(); vertex_status = vstat_; edge_status = estat_; }

  // ---- connection strategy (:1316-1364) ----
  void setMaxNearestNeighbors(size_t k) {                                        // KBoundedStrategy(k, maxDistance_) :1327-1344
    if (star_) throw std::runtime_error("Cannot set the maximum nearest neighbors for VoxelCachedLazyPRM");
    k_ = k;
  }
  void setStarConnectionStrategy() { star_ = true; }                             // KStarStrategy :1346-1356
  void setRange(double distance) { max_distance_ = distance; }                   // :1319-1326
  /// maxDistance_: 0.2 of the space's maximum extent unless set (SelfConfig::configurePlannerRange, :1242)
  double getRange() const {
    if (max_distance_ > 0) return max_distance_;
    double w_rot = 0, w_ret = 0, ext2 = 0;
    tr_space_weights(vc_.context(), &w_rot, &w_ret);
    const auto &rb = vc_.robot();
    for (auto &t : rb.tendons) ext2 += t.max_tension * t.max_tension;
    return 0.2 * (std::sqrt(ext2) + (rb.enable_rotation ? w_rot * 3.14159265358979323846 : 0.0) + (rb.enable_retraction ? w_ret * rb.specs.L : 0.0));
  }
  /// the box new milestones are drawn from (default: the planner's state-space bounds, Problem.cpp:101-163)
  void setSamplingBounds(const std::vector<double> &lo, const std::vector<double> &hi) {
    if (lo.size() != S_ || hi.size() != S_) throw std::invalid_argument("State is not the right size");
    lo_ = lo; hi_ = hi;
  }

  // ---- createRoadmap (:1380-1561) ----
  /// Brings the roadmap up to N milestones.  New milestones: the next candidates of the sequence that pass what `opt` asks of a
  /// vertex (nothing | is_valid_shape | is_valid_shape and no collision, :1412-1440); every new milestone is connected to its
  /// connection-strategy neighbours among ALL milestones (:1491-1502: nearestK on a structure that already holds the milestone, so
  /// k counts the milestone itself); with VoxelizeEdges / ValidateEdges the new edges are voxelised / checked (voxelizeEdge :2879 /
  /// computeEdgeValidity :2621) in one batched pass and the failing ones removed (:1508-1551).
  void createRoadmap(size_t N, int opt = LazyRoadmap) {
    const size_t Nv = milestoneCount();
    if (N <= Nv) return;                                                         // :1387-1391
    need_validators("createRoadmap");
    absorb();
    tr_ctx *c = vc_.context();
    const bool validate_verts = opt & ValidateVertices, validate_edges = opt & ValidateEdges;
    const bool voxelize_verts = validate_verts || (opt & VoxelizeVertices), voxelize_edges = validate_edges || (opt & VoxelizeEdges);
    const size_t add = N - Nv;
    const double *lo = lo_.empty() ? nullptr : lo_.data(), *hi = hi_.empty() ? nullptr : hi_.data();
    report_ = BuildReport{};
    std::vector<double> st(add * S_), tips(3 * add, std::nan(""));
    report_.candidate_index.resize(add);
    const uint64_t first = next_candidate_;
    if (!voxelize_verts) {                                                       // sampleUniform, accepted as it is (:1417-1419)
      check(c, tr_candidate_states(c, seed_, first, (int64_t)add, lo, hi, st.data()));
      for (size_t i = 0; i < add; i++) report_.candidate_index[i] = (int64_t)(first + i);
      next_candidate_ += add;
    } else if (validate_verts) {                                                 // ... until valid shape and no collision (:1421-1436)
      int64_t acc = 0, tried = 0;
      if (const tr_edge_loads *ld = vc_.loads())          // the checker's FK is the loaded one (setLoads)
        check(c, tr_sample_valid_vertices_loaded(c, nullptr, ld, seed_, first, lo, hi, (int64_t)add, 0, st.data(), tips.data(),
                                                 report_.candidate_index.data(), nullptr, &acc, &tried, &report_.n_unconverged, &report_.n_integrations));
      else
        check(c, tr_sample_valid_vertices(c, seed_, first, lo, hi, (int64_t)add, 0, st.data(), tips.data(), report_.candidate_index.data(), &acc, &tried));
      if ((size_t)acc < add) throw std::runtime_error("createRoadmap: only " + std::to_string(acc) + " valid milestones in " + std::to_string(tried) + " candidates");
      next_candidate_ += (uint64_t)tried;
    } else {                                                                     // ... until valid shape (:1421-1426)
      size_t have = 0;
      while (have < add) {
        const size_t m = std::max<size_t>(4096, (add - have) + (add - have) / 2);
        std::vector<double> cand(m * S_);
        std::vector<uint64_t> bits((m + 63) / 64);
        std::vector<uint8_t> flags(m);
        check(c, tr_candidate_states(c, seed_, next_candidate_, (int64_t)m, lo, hi, cand.data()));
        const tr_edge_loads *ld = vc_.loads();
        if (ld) {                                         // is_valid_shape of the LOADED shapes: voxelizeVertex's own test
          std::vector<int64_t> off(m + 1);
          int64_t nu = 0, ni = 0;
          check(c, tr_voxelize_batch_loaded(c, nullptr, ld, cand.data(), (int64_t)m, off.data(), bits.data(), nullptr, &nu, &ni));
          report_.n_unconverged += nu; report_.n_integrations += ni;
        } else {
          check(c, tr_validate_batch(c, cand.data(), (int64_t)m, bits.data(), nullptr, flags.data()));
        }
        const unsigned shape_ok = TR_FLAG_CONVERGED | TR_FLAG_LENGTH_OK | TR_FLAG_NO_SELFCOL;
        size_t used = m;
        for (size_t i = 0; i < m; i++) {
          if (ld ? !((bits[i >> 6] >> (i & 63)) & 1u) : (flags[i] & (shape_ok | TR_FLAG_DOMAIN)) != shape_ok) continue;
          std::copy(cand.begin() + i * S_, cand.begin() + (i + 1) * S_, st.begin() + have * S_);
          report_.candidate_index[have] = (int64_t)(next_candidate_ + i);
          if (++have == add) { used = i + 1; break; }
        }
        next_candidate_ += used;
        if (next_candidate_ - first > 64 * (uint64_t)add + (1u << 20)) throw std::runtime_error("createRoadmap: too few shape-valid candidates");
      }
    }
    report_.candidates_tried = (int64_t)(next_candidate_ - first);
    // the milestones join the graph before any of them is connected (:1463-1483)
    VoxelCaches vnew = detail::empty_items(add);
    if (voxelize_verts) {
      vnew = voxelize_states(vc_, st, add, &tips);
      for (size_t i = 0; i < add; i++) if (!vnew.usable[i]) throw std::runtime_error("createRoadmap: an accepted milestone has no valid shape");
    }
    states_.insert(states_.end(), st.begin(), st.end());
    tips_.insert(tips_.end(), tips.begin(), tips.end());
    has_tip_.insert(has_tip_.end(), add, voxelize_verts ? 1 : 0);
    vstat_.insert(vstat_.end(), add, validate_verts ? 1 : 0);
    detail::append_items(vcache_, vnew);
    dirty_ = true;
    // connectionStrategy_(v) for every new v; an edge exists once (:1491-1502)
    const int64_t kk = std::min<int64_t>((int64_t)N, star_ ? (int64_t)tr_kstar_k(c, (int64_t)N) : (int64_t)k_);
    const double maxd = star_ ? HUGE_VAL : getRange();
    report_.k = (int32_t)kk; report_.max_distance = maxd;
    std::vector<int32_t> cand((size_t)(2 * (int64_t)N * kk));
    int64_t ne = 0;
    if (kk >= 1 && Nv == 0) {
      check(c, tr_knn_edges(c, states_.data(), (int64_t)N, (int32_t)kk, maxd, cand.data(), (int64_t)N * kk, &ne));
    } else if (kk >= 1) {
      std::vector<int32_t> table((size_t)((int64_t)N * kk), -1);                  // rows of the old milestones stay empty: they do not connect again
      std::vector<double> dist((size_t)((int64_t)add * kk));
      check(c, tr_knn_range(c, states_.data(), (int64_t)N, (int64_t)Nv, (int64_t)add, (int32_t)kk, maxd, table.data() + Nv * (size_t)kk, dist.data()));
      check(c, tr_knn_table_edges(c, table.data(), (int64_t)N, (int32_t)kk, cand.data(), (int64_t)N * kk, &ne));
    }
    cand.resize((size_t)(2 * ne));
    report_.candidate_edges = cand;
    report_.accepted.assign((size_t)ne, true);
    VoxelCaches enew = detail::empty_items((size_t)ne);
    std::vector<size_t> keep;
    if (voxelize_edges && ne > 0) {
      enew.offsets.assign((size_t)ne + 1, 0);
      std::vector<uint64_t> bits((size_t)(ne + 63) / 64);
      report_.n_fk.resize((size_t)ne);
      int64_t nu = 0, ni = 0;
      check(c, VoxelBackboneMotionValidator::indexed_lists(vc_, mv_->space, states_.data(), (int64_t)N, cand.data(), ne, validate_edges,
                                                          enew.offsets.data(), bits.data(), report_.n_fk.data(), &nu, &ni));
      report_.n_unconverged += nu; report_.n_integrations += ni;
      enew.usable = detail::unpack(bits, (size_t)ne);
      detail::fetch(c, enew);
      report_.accepted = enew.usable;
      for (size_t e = 0; e < (size_t)ne; e++) if (enew.usable[e]) keep.push_back(e);
      enew = detail::select_items(enew, keep);
    } else {
      for (size_t e = 0; e < (size_t)ne; e++) keep.push_back(e);
    }
    for (size_t e : keep) {
      edges_.push_back(cand[2 * e]); edges_.push_back(cand[2 * e + 1]);
      if (!weights_.empty()) weights_.push_back(distance(&states_[(size_t)cand[2 * e] * S_], &states_[(size_t)cand[2 * e + 1] * S_]));
    }
    estat_.insert(estat_.end(), keep.size(), validate_edges ? 1 : 0);
    detail::append_items(ecache_, enew);
  }

  // ---- precompute* (:1563-1648, :1692-1789) ----
  /// voxelizeVertex for every vertex without a cache or a tip; vertices without a valid shape leave the roadmap
  void precomputeVertexVoxelCache() {
    need_validators("precomputeVertexVoxelCache");
    absorb();
    remove_vertices(voxelize_missing_vertices(nullptr));
  }
  /// voxelizeEdge for every edge without a cache; edges that are not fully valid leave the roadmap
  void precomputeEdgeVoxelCache() {
    need_validators("precomputeEdgeVoxelCache");
    absorb();
    std::vector<size_t> miss;
    for (size_t e = 0; e < edgeCount(); e++) if (!ecache_.usable[e]) miss.push_back(e);
    remove_edges(edge_pass(miss, false));
  }
  void precomputeVoxelCache() { precomputeVertexVoxelCache(); precomputeEdgeVoxelCache(); }
  /// computeVertexValidity for every vertex not known valid (voxelise if needed, then against the obstacles); the others leave
  void precomputeVertexValidity() {
    need_validators("precomputeVertexValidity");
    absorb();
    std::vector<bool> todo(milestoneCount());
    for (size_t v = 0; v < milestoneCount(); v++) todo[v] = vstat_[v] != 1;
    std::vector<size_t> gone = voxelize_missing_vertices(&todo);
    const std::vector<bool> hit = caches_collide(vc_, vcache_);
    std::vector<bool> out(milestoneCount(), false);
    for (size_t v : gone) out[v] = true;
    for (size_t v = 0; v < milestoneCount(); v++) {
      if (!todo[v] || out[v]) continue;
      if (hit[v]) out[v] = true; else vstat_[v] = 1;
    }
    gone.clear();
    for (size_t v = 0; v < milestoneCount(); v++) if (out[v]) gone.push_back(v);
    remove_vertices(gone);
  }
  /// computeEdgeValidity for every edge not known valid; the others leave
  void precomputeEdgeValidity() {
    need_validators("precomputeEdgeValidity");
    absorb();
    std::vector<size_t> miss, have;
    for (size_t e = 0; e < edgeCount(); e++) if (estat_[e] != 1) (ecache_.usable[e] ? have : miss).push_back(e);
    std::vector<size_t> gone = edge_pass(miss, true);                            // voxelise + collide in one traversal of the samples
    std::vector<bool> out(edgeCount(), false);
    for (size_t e : gone) out[e] = true;
    for (size_t e : miss) if (!out[e]) estat_[e] = 1;
    if (!have.empty()) {
      const std::vector<bool> hit = caches_collide(vc_, ecache_);
      for (size_t e : have) { if (hit[e]) out[e] = true; else estat_[e] = 1; }
    }
    gone.clear();
    for (size_t e = 0; e < edgeCount(); e++) if (out[e]) gone.push_back(e);
    remove_edges(gone);
  }
  void precomputeValidity() { precomputeVertexValidity(); precomputeEdgeValidity(); }
  void clearVertexVoxelCache() { absorb(); vcache_ = detail::empty_items(milestoneCount()); dirty_ = true; }    // :1791-1795
  void clearEdgeVoxelCache() { absorb(); ecache_ = detail::empty_items(edgeCount()); dirty_ = true; }           // :1797-1801
  void clearVoxelCache() { clearVertexVoxelCache(); clearEdgeVoxelCache(); }
  /// vertices outside the largest connected component leave the roadmap (:1665-1690)
  void clearDisconnectedVertices() {
    absorb();
    const size_t V = milestoneCount();
    std::vector<int32_t> parent(V);
    for (size_t v = 0; v < V; v++) parent[v] = (int32_t)v;
    auto find = [&](int32_t x) { while (parent[x] != x) { parent[x] = parent[parent[x]]; x = parent[x]; } return x; };
    for (size_t e = 0; e < edgeCount(); e++) {
      const int32_t a = find(edges_[2 * e]), b = find(edges_[2 * e + 1]);
      if (a != b) parent[std::max(a, b)] = std::min(a, b);
    }
    std::vector<size_t> size(V, 0);
    for (size_t v = 0; v < V; v++) size[(size_t)find((int32_t)v)]++;
    size_t best = 0;
    for (size_t v = 0; v < V; v++) if (size[v] > size[best]) best = v;
    std::vector<size_t> gone;
    for (size_t v = 0; v < V; v++) if ((size_t)find((int32_t)v) != best) gone.push_back(v);
    remove_vertices(gone);
  }

  // ---- queries ----
  /// vertexVoxelsProperty_ / edgeVoxelsProperty_ as CSR; `usable` = which items have a cache at all (empty = all of them)
  void setCaches(const VoxelCaches &vertices, const VoxelCaches &edges) {
    if (vertices.items() != milestoneCount() || edges.items() != edgeCount()) throw std::invalid_argument("cache offsets do not match the roadmap");
    absorb();
    vcache_ = vertices; ecache_ = edges;
    if (vcache_.usable.empty()) vcache_.usable.assign(milestoneCount(), true);
    if (ecache_.usable.empty()) ecache_.usable.assign(edgeCount(), true);
    caches_given_ = true;
    dirty_ = true;
  }
  /// landmark lower bounds for the searches (0 = the reference's heuristic alone); paths and costs do not depend on it
  void prepare(int n_landmarks = 16, int n_threads = 0) { lm_ = n_landmarks; lm_threads_ = n_threads; sync(); }
  void clearValidity() {                                                         // :1656-1663
    std::fill(vstat_.begin(), vstat_.end(), 0); std::fill(estat_.begin(), estat_.end(), 0);
    if (rm_ && !dirty_) rcheck(tr_roadmap_clear_validity(rm_));
  }
  /// every cached set against the checker's current obstacle grid -> (#invalid vertices, #invalid edges)
  std::pair<int64_t, int64_t> revalidate() {
    sync();
    int64_t nv = 0, ne = 0;
    rcheck(tr_roadmap_revalidate(rm_, &nv, &ne));
    return {nv, ne};
  }
  Solution solveWithRoadmap(const std::vector<int32_t> &starts, const std::vector<int32_t> &goals, int n_threads = 0) {
    if (starts.size() != goals.size()) throw std::invalid_argument("starts and goals differ in length");
    sync();
    const size_t n = starts.size();
    Solution s;
    s.status.resize(n); s.cost.resize(n);
    std::vector<int64_t> off(n + 1, 0);
    rcheck(tr_roadmap_solve(rm_, starts.data(), goals.data(), (int64_t)n, n_threads, s.status.data(), s.cost.data(), off.data(), &s.stats));
    std::vector<int32_t> pv((size_t)off[n]);
    rcheck(tr_roadmap_fetch_paths(rm_, pv.data(), (int64_t)pv.size()));
    s.paths.resize(n);
    for (size_t q = 0; q < n; q++) s.paths[q].assign(pv.begin() + off[q], pv.begin() + off[q + 1]);
    return s;
  }
  // Where the graph searches of the last solveWithRoadmap ran (tr_roadmap_search_stats): the kernel, the host threads, the component labels.
  struct SearchStats { int64_t on_device, handed_back, on_host_meanwhile, list_moves, expanded_on_device, expanded_on_host, answered_by_components; };
  SearchStats searchStats() const {
    int64_t o[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (rm_) rcheck(tr_roadmap_search_stats(rm_, o));
    return SearchStats{o[0], o[1], o[2], o[3], o[4], o[5], o[6]};
  }
  /// Device memory the graph searches hold for this planner between calls, and handing it back (tr_roadmap_release_search_state;
  /// the next large batch of queries allocates it again).
  int64_t searchStateBytes() const { int64_t b = 0; if (rm_) rcheck(tr_roadmap_search_state_bytes(rm_, &b)); return b; }
  void reserveSearchState(int64_t n_queries) { sync(); rcheck(tr_roadmap_reserve_search_state(rm_, n_queries)); }
  // ---- roadmapIk (VoxelCachedLazyPRM.h:356-446, .cpp:3095-3430) ----
  enum RoadmapIkOpts { RMAP_IK_SIMPLE = 0x0, RMAP_IK_AUTO_ADD = 0x1, RMAP_IK_ACCURATE = 0x2, RMAP_IK_LAZY_ADD = 0x4 };
  struct IKResult {
    std::vector<double> controls;          // valid state at or close to the request
    std::array<double, 3> tip_position{};  // tip position obtained by controls
    std::vector<double> neighbor;          // the vertex state IK started from
    size_t neighbor_vertex = 0;            // ... and its vertex number
    double error = 0.0;                    // |tip_position - request|
  };
  /// RMAP_IK_SIMPLE: IK from the k vertices whose tips are nearest the request (vertices with a tip and not known invalid; the
  /// unknown ones among them are checked, the invalid dropped and the search repeated), all k problems in ONE tr_ik_batch; the
  /// solutions are validated in one isValidBatch; the first in neighbour order that is valid and within tolerance is returned,
  /// else the valid one with the least error; if none is valid, each solution is replaced by the last valid state of
  /// checkMotion(neighbor, solution) and the one whose tip is nearest the request is returned.  std::nullopt: no vertex to start
  /// from.  AUTO_ADD, ACCURATE and LAZY_ADD are not offered (std::invalid_argument).  Vertices found invalid here are not
  /// removed from the roadmap.
  std::optional<IKResult> roadmapIk(const std::array<double, 3> &request, double tolerance = 1e-4, size_t k = 5, int opts = RMAP_IK_SIMPLE) {
    if (opts != RMAP_IK_SIMPLE) throw std::invalid_argument("roadmapIk: only RMAP_IK_SIMPLE is supported");
    refuse_loaded("roadmapIk");
    absorb();
    const auto &rb = vc_.robot();
    auto tip_dist2 = [&](const double *t) {
      double s = 0.0;
      for (int q = 0; q < 3; q++) s += (t[q] - request[q]) * (t[q] - request[q]);
      return s;
    };
    // 1-2. the k nearest vertices by tip among the valid ones
    std::vector<size_t> cand;
    for (size_t v = 0; v < milestoneCount(); v++) if (has_tip_[v] && vstat_[v] != 2) cand.push_back(v);
    std::stable_sort(cand.begin(), cand.end(), [&](size_t a, size_t b) { return tip_dist2(&tips_[3 * a]) < tip_dist2(&tips_[3 * b]); });
    std::vector<size_t> near;
    std::vector<uint8_t> known(milestoneCount(), 0);
    for (size_t v = 0; v < milestoneCount(); v++) known[v] = vstat_[v];
    size_t next = 0;
    while (near.size() < k && next < cand.size()) {
      std::vector<size_t> unknown;
      while (near.size() + unknown.size() < k && next < cand.size()) {
        const size_t v = cand[next++];
        if (known[v] == 1) near.push_back(v); else unknown.push_back(v);
      }
      if (unknown.empty()) continue;
      std::vector<double> st(unknown.size() * S_);
      for (size_t i = 0; i < unknown.size(); i++) std::copy(states_.begin() + unknown[i] * S_, states_.begin() + (unknown[i] + 1) * S_, st.begin() + i * S_);
      const std::vector<bool> ok = vc_.isValidBatch(st, unknown.size());
      for (size_t i = 0; i < unknown.size(); i++) { known[unknown[i]] = ok[i] ? 1 : 2; if (ok[i]) near.push_back(unknown[i]); }
    }
    if (near.empty()) return std::nullopt;
    std::stable_sort(near.begin(), near.end(), [&](size_t a, size_t b) { return tip_dist2(&tips_[3 * a]) < tip_dist2(&tips_[3 * b]); });
    const size_t m = near.size();
    std::vector<double> starts(m * S_);
    for (size_t i = 0; i < m; i++) std::copy(states_.begin() + near[i] * S_, states_.begin() + (near[i] + 1) * S_, starts.begin() + i * S_);
    // 3. IK from all of them in one batch
    const std::vector<tip_control::IKResult> ik =
        tip_control::inverse_kinematics_batch(rb, starts, m, {request}, 100, 0.1, 1e-9, 1e-4, tolerance, 1e-6);
    // 4. one validity batch
    std::vector<double> sol(m * S_);
    for (size_t i = 0; i < m; i++) std::copy(ik[i].state.begin(), ik[i].state.end(), sol.begin() + i * S_);
    const std::vector<bool> valid = vc_.isValidBatch(sol, m);
    auto result = [&](size_t i, const std::vector<double> &x, const std::array<double, 3> &tip, double err) {
      IKResult r;
      r.controls = x; r.tip_position = tip; r.error = err; r.neighbor_vertex = near[i];
      r.neighbor.assign(starts.begin() + i * S_, starts.begin() + (i + 1) * S_);
      return r;
    };
    // 5. the first valid one within tolerance, else the valid one with the least error
    for (size_t i = 0; i < m; i++) if (valid[i] && ik[i].error <= tolerance) return result(i, ik[i].state, ik[i].tip, ik[i].error);
    size_t best = m;
    for (size_t i = 0; i < m; i++) if (valid[i] && (best == m || ik[i].error < ik[best].error)) best = i;
    if (best < m) return result(best, ik[best].state, ik[best].tip, ik[best].error);
    // 6. none valid: the last valid state towards each solution, the one whose tip is nearest the request
    need_validators("roadmapIk");
    std::vector<double> t;
    mv_->checkMotionBatch(starts, sol, m, nullptr, &t);
    std::vector<double> lv(m * S_), tips(3 * m);
    for (size_t i = 0; i < m; i++) {
      const std::vector<double> a(starts.begin() + i * S_, starts.begin() + (i + 1) * S_), b(sol.begin() + i * S_, sol.begin() + (i + 1) * S_);
      const std::vector<double> x = mv_->interpolate(a, b, t[i]);
      std::copy(x.begin(), x.end(), lv.begin() + i * S_);
    }
    check(vc_.context(), tr_fk_tips(vc_.context(), lv.data(), (int64_t)m, tips.data(), nullptr));
    best = 0;
    for (size_t i = 1; i < m; i++) if (tip_dist2(&tips[3 * i]) < tip_dist2(&tips[3 * best])) best = i;
    const std::vector<double> x(lv.begin() + best * S_, lv.begin() + (best + 1) * S_);
    return result(best, x, {tips[3 * best], tips[3 * best + 1], tips[3 * best + 2]}, std::sqrt(tip_dist2(&tips[3 * best])));
  }

  // ---- roadmapIk + solveWithRoadmap for a batch of tip requests (tr_roadmap_ik_batch / tr_roadmap_solve_tips) ----
  enum TipOutcome { TIP_REACHED = TR_TIPQ_REACHED, TIP_CLOSEST = TR_TIPQ_CLOSEST, TIP_NO_NEIGHBOR = TR_TIPQ_NO_NEIGHBOR };
  struct TipResults {
    std::vector<double> controls;          // n x state size: the goal states (NaN where the outcome is TIP_NO_NEIGHBOR)
    std::vector<double> tip_positions;     // n x 3
    std::vector<double> error;             // |tip_position - request|
    std::vector<int32_t> neighbor_vertex;  // the vertex IK started from = where the goal state joins the roadmap (-1: none)
    std::vector<int32_t> outcome;          // TipOutcome
    std::vector<double> last_valid_t;      // 1 when reached, else where checkMotion(neighbor, solution) stopped
  };
  struct TipSolution { TipResults ik; Solution roadmap; };   // roadmap.paths[q]: start ... connection vertex; ik.controls follows it
  /// roadmapIk for every request in ONE call (the rule in include/tendon_hip.h: what RMAP_IK_AUTO_ADD without ACCURATE finds, with
  /// nothing added to the graph): IK from the k vertices with the nearest tips, all n k problems in one device batch; per request the
  /// first solution in neighbour order within tolerance whose edge from its neighbour is valid, else the last valid state towards the
  /// solutions whose tip is nearest the request.
  TipResults roadmapIkBatch(const std::vector<std::array<double, 3>> &requests, double tolerance = 1e-4, size_t k = 5) {
    need_validators("roadmapIkBatch");
    refuse_loaded("roadmapIkBatch");
    sync_tips();
    const size_t n = requests.size();
    TipResults r = tip_results(n);
    const tr_tip_query_params prm = tip_params(tolerance, k);
    rcheck(tr_roadmap_ik_batch(rm_, &mv_->space, &prm, n ? requests[0].data() : nullptr, (int64_t)n, r.controls.data(), r.tip_positions.data(),
                               r.error.data(), r.neighbor_vertex.data(), r.outcome.data(), r.last_valid_t.data()));
    return r;
  }
  /// ... followed by solveWithRoadmap from starts[q] to request q's connection vertex; cost = roadmap cost + distance(connection
  /// vertex, goal state).  A request without a neighbour ends TR_QUERY_INVALID_GOAL.
  TipSolution solveToTips(const std::vector<int32_t> &starts, const std::vector<std::array<double, 3>> &requests, double tolerance = 1e-4,
                          size_t k = 5, int n_threads = 0) {
    if (starts.size() != requests.size()) throw std::invalid_argument("starts and requests differ in length");
    need_validators("solveToTips");
    refuse_loaded("solveToTips");
    sync_tips();
    const size_t n = requests.size();
    TipSolution s;
    s.ik = tip_results(n);
    s.roadmap.status.resize(n); s.roadmap.cost.resize(n);
    std::vector<int64_t> off(n + 1, 0);
    const tr_tip_query_params prm = tip_params(tolerance, k);
    rcheck(tr_roadmap_solve_tips(rm_, &mv_->space, &prm, starts.data(), n ? requests[0].data() : nullptr, (int64_t)n, n_threads, s.ik.controls.data(),
                                 s.ik.tip_positions.data(), s.ik.error.data(), s.ik.neighbor_vertex.data(), s.ik.outcome.data(),
                                 s.ik.last_valid_t.data(), s.roadmap.status.data(), s.roadmap.cost.data(), off.data(), &s.roadmap.stats));
    std::vector<int32_t> pv((size_t)off[n]);
    rcheck(tr_roadmap_fetch_paths(rm_, pv.data(), (int64_t)pv.size()));
    s.roadmap.paths.resize(n);
    for (size_t q = 0; q < n; q++) s.roadmap.paths[q].assign(pv.begin() + off[q], pv.begin() + off[q + 1]);
    return s;
  }

  // ---- RMAP_IK_ACCURATE for a batch (tr_roadmap_nearest_states / tr_roadmap_ik_batch_connect / tr_roadmap_solve_tips_connect) ----
  struct NearestStates {
    std::vector<int32_t> vertices;         // n x k, -1 padded
    std::vector<double> distance;          // n x k, +inf where padded
  };
  /// connectionStrategy_ for states that are not in the roadmap: per query (n x state size, flat) the k nearest vertices in state
  /// space among those not known invalid, in the order (distance, vertex index), none farther than max_distance.
  NearestStates nearestStates(const std::vector<double> &queries, size_t k, double max_distance = std::numeric_limits<double>::infinity()) {
    if (queries.size() % S_ != 0) throw std::invalid_argument("nearestStates: queries must be n x state size");
    sync_tips();
    const size_t n = queries.size() / S_;
    NearestStates r;
    r.vertices.assign(n * k, -1); r.distance.assign(n * k, std::numeric_limits<double>::infinity());
    rcheck(tr_roadmap_nearest_states(rm_, queries.data(), (int64_t)n, (int32_t)k, max_distance, r.vertices.data(), r.distance.data()));
    return r;
  }
  // ---- queries between arbitrary states (tr_roadmap_attach_states / tr_roadmap_solve_seeded / tr_roadmap_solve_states) ----
  enum AttachDirection { ATTACH_OUT = TR_ATTACH_OUT, ATTACH_IN = TR_ATTACH_IN };
  struct Attachments {
    std::vector<uint8_t> valid;            // n: the state is valid (solvePrep only admits such)
    std::vector<int32_t> vertices;         // n x k, -1 padded: nearestStates' rows; all -1 for an invalid state
    std::vector<double> cost;              // n x k, +inf where padded
    std::vector<uint8_t> edge_ok;          // n x k: checkMotion(state, vertex) for ATTACH_OUT, checkMotion(vertex, state) for ATTACH_IN
    std::vector<int32_t> n_fk;             // n x k
    int64_t n_domain_errors = 0;
  };
  /// addMilestone(state, connect = true) for a batch of states (n x state size, flat) without editing the graph: rules A1 - A4 of
  /// include/tendon_hip.h in one device-resident pass.
  Attachments attachStates(const std::vector<double> &states, AttachDirection direction = ATTACH_OUT, size_t k = 10,
                           double max_distance = std::numeric_limits<double>::infinity()) {
    if (states.size() % S_ != 0) throw std::invalid_argument("attachStates: states must be n x state size");
    need_validators("attachStates");
    refuse_loaded("attachStates");
    sync_tips();
    const size_t n = states.size() / S_;
    Attachments a;
    a.valid.assign(n, 0); a.vertices.assign(n * k, -1); a.cost.assign(n * k, std::numeric_limits<double>::infinity());
    a.edge_ok.assign(n * k, 0); a.n_fk.assign(n * k, 0);
    const tr_attach_params prm{(int32_t)k, max_distance};
    rcheck(tr_roadmap_attach_states(rm_, &mv_->space, &prm, (int32_t)direction, states.data(), (int64_t)n, a.valid.data(), a.vertices.data(),
                                    a.cost.data(), a.edge_ok.data(), a.n_fk.data(), &a.n_domain_errors));
    return a;
  }
  struct Seeds {                           // per query a list of (vertex, cost) seeds, as CSR
    std::vector<int64_t> offsets{0};
    std::vector<int32_t> vertices;
    std::vector<double> costs;
    void add_query(const std::vector<int32_t> &v, const std::vector<double> &c) {
      if (v.size() != c.size()) throw std::invalid_argument("Seeds: a query's vertices and costs differ in length");
      vertices.insert(vertices.end(), v.begin(), v.end()); costs.insert(costs.end(), c.begin(), c.end());
      offsets.push_back((int64_t)vertices.size());
    }
    size_t queries() const { return offsets.size() - 1; }
  };
  struct SeededSolution : Solution {
    std::vector<int32_t> src_pick, dst_pick;   // indices into the query's seed lists; -1: the direct connection won, or no path
  };
  /// Searches from several weighted sources to several weighted targets per query (rules S1 - S4): the answer minimises
  /// c_i + dist(u_i, v_j) + d_j; direct_cost (empty: none; +inf per query: none) is a connection that bypasses the roadmap and wins ties.
  SeededSolution solveSeeded(const Seeds &src, const Seeds &dst, const std::vector<double> &direct_cost = {}, int n_threads = 0) {
    if (src.queries() != dst.queries()) throw std::invalid_argument("solveSeeded: src and dst differ in their number of queries");
    const size_t n = src.queries();
    if (!direct_cost.empty() && direct_cost.size() != n) throw std::invalid_argument("solveSeeded: one direct cost per query");
    refuse_loaded("solveSeeded");
    sync();
    SeededSolution s;
    s.status.resize(n); s.cost.resize(n); s.src_pick.resize(n); s.dst_pick.resize(n);
    std::vector<int64_t> off(n + 1, 0);
    rcheck(tr_roadmap_solve_seeded(rm_, (int64_t)n, src.offsets.data(), src.vertices.data(), src.costs.data(), dst.offsets.data(),
                                   dst.vertices.data(), dst.costs.data(), direct_cost.empty() ? nullptr : direct_cost.data(), n_threads,
                                   s.status.data(), s.cost.data(), s.src_pick.data(), s.dst_pick.data(), off.data(), &s.stats));
    fetch_paths(s, off);
    return s;
  }
  struct StateSolution : SeededSolution {      // src_pick / dst_pick: the picked slots of the attach rows
    std::vector<int32_t> start_vertex, goal_vertex;   // the picked connection vertices; -1 for a direct answer or none
    std::vector<uint8_t> direct;                      // the query is answered by the edge start state -> goal state
  };
  /// solvePrep + solveWithRoadmap between arbitrary start and goal STATES (n x state size each, flat; rules T1 - T3): the motion of a
  /// solved query is start state, paths[q], goal state, and cost includes both connections.  Nothing is inserted into the graph.
  StateSolution solveStates(const std::vector<double> &starts, const std::vector<double> &goals, size_t k = 10,
                            double max_distance = std::numeric_limits<double>::infinity(), int n_threads = 0) {
    if (starts.size() % S_ != 0 || starts.size() != goals.size()) throw std::invalid_argument("solveStates: starts and goals must both be n x state size");
    need_validators("solveStates");
    refuse_loaded("solveStates");
    sync_tips();
    const size_t n = starts.size() / S_;
    StateSolution s;
    s.status.resize(n); s.cost.resize(n); s.src_pick.resize(n); s.dst_pick.resize(n); s.start_vertex.resize(n); s.goal_vertex.resize(n);
    s.direct.resize(n);
    std::vector<int64_t> off(n + 1, 0);
    const tr_attach_params prm{(int32_t)k, max_distance};
    rcheck(tr_roadmap_solve_states(rm_, &mv_->space, &prm, starts.data(), goals.data(), (int64_t)n, n_threads, s.status.data(), s.cost.data(),
                                   s.start_vertex.data(), s.goal_vertex.data(), s.direct.data(), s.src_pick.data(), s.dst_pick.data(), off.data(),
                                   &s.stats));
    fetch_paths(s, off);
    return s;
  }
  struct AccurateTipResults : TipResults {   // neighbor_vertex: the connection vertex, a state-space neighbour of the goal state
    std::vector<int32_t> ik_vertex;          // the vertex IK started from
    std::array<int64_t, 4> connect_stats{};  // pairs checked, reached, connection vertex != ik_vertex, reached only by this rule
  };
  struct AccurateTipSolution { AccurateTipResults ik; Solution roadmap; };
  /// roadmapIkBatch under RMAP_IK_ACCURATE (rules 3' - 5' in include/tendon_hip.h): every IK answer is tried from its k_connect
  /// state-space neighbours and then from the vertex IK started from; nothing is added to the graph.
  AccurateTipResults roadmapIkBatchAccurate(const std::vector<std::array<double, 3>> &requests, double tolerance = 1e-4, size_t k = 5,
                                            size_t k_connect = 10, double max_distance = std::numeric_limits<double>::infinity()) {
    need_validators("roadmapIkBatchAccurate");
    refuse_loaded("roadmapIkBatchAccurate");
    sync_tips();
    const size_t n = requests.size();
    AccurateTipResults r;
    static_cast<TipResults &>(r) = tip_results(n);
    r.ik_vertex.resize(n);
    const tr_tip_query_params prm = tip_params(tolerance, k);
    const tr_tip_connect_params cp{(int32_t)k_connect, max_distance};
    rcheck(tr_roadmap_ik_batch_connect(rm_, &mv_->space, &prm, &cp, n ? requests[0].data() : nullptr, (int64_t)n, r.controls.data(),
                                       r.tip_positions.data(), r.error.data(), r.neighbor_vertex.data(), r.ik_vertex.data(), r.outcome.data(),
                                       r.last_valid_t.data()));
    rcheck(tr_roadmap_tip_connect_stats(rm_, r.connect_stats.data()));
    return r;
  }
  /// ... followed by solveWithRoadmap from starts[q] to request q's connection vertex, as solveToTips.
  AccurateTipSolution solveToTipsAccurate(const std::vector<int32_t> &starts, const std::vector<std::array<double, 3>> &requests,
                                          double tolerance = 1e-4, size_t k = 5, size_t k_connect = 10, int n_threads = 0,
                                          double max_distance = std::numeric_limits<double>::infinity()) {
    if (starts.size() != requests.size()) throw std::invalid_argument("starts and requests differ in length");
    need_validators("solveToTipsAccurate");
    refuse_loaded("solveToTipsAccurate");
    sync_tips();
    const size_t n = requests.size();
    AccurateTipSolution s;
    static_cast<TipResults &>(s.ik) = tip_results(n);
    s.ik.ik_vertex.resize(n);
    s.roadmap.status.resize(n); s.roadmap.cost.resize(n);
    std::vector<int64_t> off(n + 1, 0);
    const tr_tip_query_params prm = tip_params(tolerance, k);
    const tr_tip_connect_params cp{(int32_t)k_connect, max_distance};
    rcheck(tr_roadmap_solve_tips_connect(rm_, &mv_->space, &prm, &cp, starts.data(), n ? requests[0].data() : nullptr, (int64_t)n, n_threads,
                                         s.ik.controls.data(), s.ik.tip_positions.data(), s.ik.error.data(), s.ik.neighbor_vertex.data(),
                                         s.ik.ik_vertex.data(), s.ik.outcome.data(), s.ik.last_valid_t.data(), s.roadmap.status.data(),
                                         s.roadmap.cost.data(), off.data(), &s.roadmap.stats));
    rcheck(tr_roadmap_tip_connect_stats(rm_, s.ik.connect_stats.data()));
    std::vector<int32_t> pv((size_t)off[n]);
    rcheck(tr_roadmap_fetch_paths(rm_, pv.data(), (int64_t)pv.size()));
    s.roadmap.paths.resize(n);
    for (size_t q = 0; q < n; q++) s.roadmap.paths[q].assign(pv.begin() + off[q], pv.begin() + off[q + 1]);
    return s;
  }

  // ---- tip queries on LOADED shapes (tr_roadmap_ik_batch_loaded / tr_roadmap_solve_tips_loaded / tr_roadmap_set_tips_loaded; rules
  // 1L - 5'L in include/tendon_hip.h).  The load set is given explicitly, in the struct VoxelBackboneValidityChecker::setLoads holds
  // (checker.loads()); roadmapIk* and solveToTips* on a checker with loads keep throwing. ----
  struct LoadedTipResults : AccurateTipResults {
    std::vector<double> vu0;                 // n x 6: the base strains (v0, u0) of the goal state's equilibrium
    std::array<int64_t, 4> counts{};         // pairs checked, IK answers without an equilibrium, last valid states unconverged, integrations
  };
  struct LoadedTipSolution { LoadedTipResults ik; Solution roadmap; };
  /// The vertices' tips from cold loaded solves of the roadmap's states (a vertex without an equilibrium has no tip).  A roadmap
  /// built by createRoadmap after setLoads holds loaded tips already.
  void setTipsLoaded(const tr_edge_loads &loads) {
    sync_tips();
    std::vector<bool> has(milestoneCount());
    for (size_t v = 0; v < milestoneCount(); v++) has[v] = has_tip_[v] != 0;
    const auto bits = detail::pack(has);
    rcheck(tr_roadmap_set_tips_loaded(rm_, nullptr, &loads, bits.data()));
  }
  /// roadmapIkBatch (k_connect = 0) or roadmapIkBatchAccurate on loaded shapes under `loads`, every solve cold.
  LoadedTipResults roadmapIkBatchLoaded(const std::vector<std::array<double, 3>> &requests, const tr_edge_loads &loads, double tolerance = 1e-4,
                                        size_t k = 5, size_t k_connect = 0, double max_distance = std::numeric_limits<double>::infinity()) {
    need_validators("roadmapIkBatchLoaded");
    sync_tips();
    const size_t n = requests.size();
    LoadedTipResults r;
    static_cast<TipResults &>(r) = tip_results(n);
    r.ik_vertex.resize(n); r.vu0.resize(6 * n);
    const tr_tip_query_params prm = tip_params(tolerance, k);
    const tr_tip_connect_params cp{(int32_t)k_connect, max_distance};
    rcheck(tr_roadmap_ik_batch_loaded(rm_, &mv_->space, &prm, &cp, nullptr, &loads, n ? requests[0].data() : nullptr, (int64_t)n, r.controls.data(),
                                      r.tip_positions.data(), r.error.data(), r.neighbor_vertex.data(), r.ik_vertex.data(), r.outcome.data(),
                                      r.last_valid_t.data(), r.vu0.data(), r.counts.data()));
    rcheck(tr_roadmap_tip_connect_stats(rm_, r.connect_stats.data()));
    return r;
  }
  /// ... followed by solveWithRoadmap from starts[q] to request q's connection vertex, as solveToTips.
  LoadedTipSolution solveToTipsLoaded(const std::vector<int32_t> &starts, const std::vector<std::array<double, 3>> &requests,
                                      const tr_edge_loads &loads, double tolerance = 1e-4, size_t k = 5, size_t k_connect = 0, int n_threads = 0,
                                      double max_distance = std::numeric_limits<double>::infinity()) {
    if (starts.size() != requests.size()) throw std::invalid_argument("starts and requests differ in length");
    need_validators("solveToTipsLoaded");
    sync_tips();
    const size_t n = requests.size();
    LoadedTipSolution s;
    static_cast<TipResults &>(s.ik) = tip_results(n);
    s.ik.ik_vertex.resize(n); s.ik.vu0.resize(6 * n);
    s.roadmap.status.resize(n); s.roadmap.cost.resize(n);
    std::vector<int64_t> off(n + 1, 0);
    const tr_tip_query_params prm = tip_params(tolerance, k);
    const tr_tip_connect_params cp{(int32_t)k_connect, max_distance};
    rcheck(tr_roadmap_solve_tips_loaded(rm_, &mv_->space, &prm, &cp, nullptr, &loads, starts.data(), n ? requests[0].data() : nullptr, (int64_t)n,
                                        n_threads, s.ik.controls.data(), s.ik.tip_positions.data(), s.ik.error.data(),
                                        s.ik.neighbor_vertex.data(), s.ik.ik_vertex.data(), s.ik.outcome.data(), s.ik.last_valid_t.data(),
                                        s.ik.vu0.data(), s.ik.counts.data(), s.roadmap.status.data(), s.roadmap.cost.data(), off.data(),
                                        &s.roadmap.stats));
    rcheck(tr_roadmap_tip_connect_stats(rm_, s.ik.connect_stats.data()));
    std::vector<int32_t> pv((size_t)off[n]);
    rcheck(tr_roadmap_fetch_paths(rm_, pv.data(), (int64_t)pv.size()));
    s.roadmap.paths.resize(n);
    for (size_t q = 0; q < n; q++) s.roadmap.paths[q].assign(pv.begin() + off[q], pv.begin() + off[q + 1]);
    return s;
  }

  int64_t releaseSearchState() { int64_t b = 0; if (rm_) rcheck(tr_roadmap_release_search_state(rm_, &b)); return b; }
  /// CompoundStateSpace::distance with the weights of Problem.cpp:112-152 (the edge cost connectVertices stores, :2857-2861)
  double distance(const double *a, const double *b) const {
    const auto &rb = vc_.robot();
    const size_t N = rb.tendons.size();
    double w_rot = 0, w_ret = 0, s = 0;
    tr_space_weights(vc_.context(), &w_rot, &w_ret);
    for (size_t i = 0; i < N; i++) s += (a[i] - b[i]) * (a[i] - b[i]);
    double d = std::sqrt(s);
    size_t k = N;
    if (rb.enable_rotation) { double r = std::fabs(a[k] - b[k]); if (r > 3.14159265358979323846) r = 2 * 3.14159265358979323846 - r; d += w_rot * r; k++; }
    if (rb.enable_retraction) d += w_ret * std::fabs(a[k] - b[k]);
    return d;
  }

 private:
  void rcheck(int st) const {
    if (st == TR_OK) return;
    const std::string m = tr_roadmap_last_error(rm_);
    if (st == TR_ERR_OUT_OF_RANGE) throw std::out_of_range(m);
    if (st == TR_ERR_INVALID_ARG) throw std::invalid_argument(m);
    throw std::runtime_error(m);
  }
  /// the vertex paths of the last solve call into s.paths
  void fetch_paths(Solution &s, const std::vector<int64_t> &off) const {
    const size_t n = off.size() - 1;
    std::vector<int32_t> pv((size_t)off[n]);
    rcheck(tr_roadmap_fetch_paths(rm_, pv.data(), (int64_t)pv.size()));
    s.paths.resize(n);
    for (size_t q = 0; q < n; q++) s.paths[q].assign(pv.begin() + off[q], pv.begin() + off[q + 1]);
  }
  void need_validators(const char *what) const {
    if (!mv_) throw std::runtime_error(std::string(what) + ": missing voxel motion validator");      // the reference's setup_ == false (:1286-1298)
  }
  /// tip inverse kinematics under load does not exist: a checker with loads (setLoads) would be answered with unloaded shapes
  void refuse_loaded(const char *what) const {
    if (vc_.loads()) throw std::logic_error(std::string(what) + " is not built for a checker with loads (setLoads): tip inverse kinematics under load does not exist");
  }
  TipResults tip_results(size_t n) const {
    TipResults r;
    r.controls.resize(n * S_); r.tip_positions.resize(n * 3); r.error.resize(n); r.neighbor_vertex.resize(n); r.outcome.resize(n); r.last_valid_t.resize(n);
    return r;
  }
  static tr_tip_query_params tip_params(double tolerance, size_t k) {
    return tr_tip_query_params{(int32_t)k, tolerance, tr_ik_params{100, 0.1, 1e-9, 1e-4, tolerance, 1e-6}};   // what roadmapIk hands to IK
  }
  /// the device image and, once per image, the vertices' tips (tipPositionProperty_; a vertex without one is no neighbour)
  void sync_tips() {
    sync();
    if (tips_synced_) return;
    std::vector<bool> has(milestoneCount());
    std::vector<double> t(tips_);
    for (size_t v = 0; v < milestoneCount(); v++) {
      has[v] = has_tip_[v] != 0;
      if (!has[v]) t[3 * v] = t[3 * v + 1] = t[3 * v + 2] = 0.0;
    }
    const auto bits = detail::pack(has);
    rcheck(tr_roadmap_set_tips(rm_, t.data(), bits.data()));
    tips_synced_ = true;
  }
  void create_device_graph() {
    tr_roadmap_destroy(rm_); rm_ = nullptr;
    const int st = tr_roadmap_create(vc_.context(), states_.data(), (int64_t)milestoneCount(), edges_.data(),
                                     weights_.empty() ? nullptr : weights_.data(), (int64_t)edgeCount(), &rm_);
    if (st == TR_ERR_OUT_OF_RANGE) throw std::out_of_range("edge refers to a state outside the roadmap");
    if (st != TR_OK) throw std::invalid_argument("tr_roadmap_create failed");
    dirty_ = false;
    tips_synced_ = false;
  }
  /// validity the query loop discovered since the last edit comes back into this object
  void absorb() {
    if (rm_ && !dirty_ && milestoneCount()) rcheck(tr_roadmap_get_validity(rm_, vstat_.data(), estat_.empty() ? nullptr : estat_.data()));
  }
  /// the device image follows the host graph: graph, caches (computed where a builder left them out: the reference voxelises such
  /// items when a query first meets them, computeVertexValidity :2607-2618), known validity, landmark tables
  void sync() {
    if (rm_ && !dirty_) return;
    if (mv_ && !caches_given_) {
      std::vector<size_t> gone = voxelize_missing_vertices(nullptr);
      for (size_t v : gone) vstat_[v] = 2;                                       // no valid shape: invalid in every environment
      std::vector<size_t> miss;
      for (size_t e = 0; e < edgeCount(); e++) if (!ecache_.usable[e] && estat_[e] != 2) miss.push_back(e);
      for (size_t e : edge_pass(miss, false)) estat_[e] = 2;
    }
    create_device_graph();
    const auto vp = detail::pack(vcache_.usable), ep = detail::pack(ecache_.usable);
    rcheck(tr_roadmap_set_caches(rm_, vcache_.offsets.data(), vcache_.block_ids.data(), vcache_.masks.data(), vp.data(),
                                 ecache_.offsets.data(), ecache_.block_ids.data(), ecache_.masks.data(), ep.data()));
    if (milestoneCount()) rcheck(tr_roadmap_set_validity(rm_, vstat_.data(), estat_.empty() ? nullptr : estat_.data()));
    if (lm_ >= 0) rcheck(tr_roadmap_prepare(rm_, lm_, lm_threads_));
  }
  /// voxelizeVertex (:2803-2837) for the vertices (of `only`, if given) without a cache or a tip -> those without a valid shape
  std::vector<size_t> voxelize_missing_vertices(const std::vector<bool> *only) {
    std::vector<size_t> miss, gone;
    for (size_t v = 0; v < milestoneCount(); v++)
      if ((!vcache_.usable[v] || !has_tip_[v]) && vstat_[v] != 2 && (!only || (*only)[v])) miss.push_back(v);
    if (miss.empty()) return gone;
    std::vector<double> st(miss.size() * S_), tips;
    for (size_t i = 0; i < miss.size(); i++) std::copy(states_.begin() + miss[i] * S_, states_.begin() + (miss[i] + 1) * S_, st.begin() + i * S_);
    VoxelCaches got = voxelize_states(vc_, st, miss.size(), &tips);
    detail::replace_items(vcache_, miss, got);
    for (size_t i = 0; i < miss.size(); i++) {
      if (!got.usable[i]) { gone.push_back(miss[i]); continue; }
      std::copy(tips.begin() + 3 * i, tips.begin() + 3 * i + 3, tips_.begin() + 3 * miss[i]);
      has_tip_[miss[i]] = 1;
    }
    dirty_ = true;
    return gone;
  }
  /// voxelizeEdge (collide = false, :2879-2902) or computeEdgeValidity (collide = true, :2621-2631) for the listed edges, which have
  /// no cache yet -> the ones that fail; the others own their voxel set afterwards
  std::vector<size_t> edge_pass(const std::vector<size_t> &list, bool collide) {
    std::vector<size_t> gone;
    if (list.empty()) return gone;
    tr_ctx *c = vc_.context();
    std::vector<int32_t> sub(2 * list.size());
    for (size_t i = 0; i < list.size(); i++) { sub[2 * i] = edges_[2 * list[i]]; sub[2 * i + 1] = edges_[2 * list[i] + 1]; }
    VoxelCaches got;
    got.offsets.assign(list.size() + 1, 0);
    std::vector<uint64_t> bits((list.size() + 63) / 64);
    check(c, VoxelBackboneMotionValidator::indexed_lists(vc_, mv_->space, states_.data(), (int64_t)milestoneCount(), sub.data(), (int64_t)list.size(),
                                                        collide, got.offsets.data(), bits.data(), nullptr));
    got.usable = detail::unpack(bits, list.size());
    detail::fetch(c, got);
    detail::replace_items(ecache_, list, got);
    for (size_t i = 0; i < list.size(); i++) if (!got.usable[i]) gone.push_back(list[i]);
    dirty_ = true;
    return gone;
  }
  /// removeVertices (:2904-2948): the vertices and every edge at them leave; the others are renumbered in order
  void remove_vertices(const std::vector<size_t> &gone) {
    if (gone.empty()) return;
    const size_t V = milestoneCount();
    std::vector<int32_t> renum(V, 0);
    for (size_t v : gone) renum[v] = -1;
    std::vector<size_t> keep;
    for (size_t v = 0; v < V; v++) if (renum[v] == 0) { renum[v] = (int32_t)keep.size(); keep.push_back(v); }
    std::vector<size_t> egone;
    for (size_t e = 0; e < edgeCount(); e++) if (renum[(size_t)edges_[2 * e]] < 0 || renum[(size_t)edges_[2 * e + 1]] < 0) egone.push_back(e);
    remove_edges(egone);
    for (int32_t &x : edges_) x = renum[(size_t)x];
    std::vector<double> st(keep.size() * S_), tp(keep.size() * 3);
    std::vector<uint8_t> ht(keep.size()), vs(keep.size());
    for (size_t i = 0; i < keep.size(); i++) {
      std::copy(states_.begin() + keep[i] * S_, states_.begin() + (keep[i] + 1) * S_, st.begin() + i * S_);
      std::copy(tips_.begin() + keep[i] * 3, tips_.begin() + keep[i] * 3 + 3, tp.begin() + i * 3);
      ht[i] = has_tip_[keep[i]]; vs[i] = vstat_[keep[i]];
    }
    states_.swap(st); tips_.swap(tp); has_tip_.swap(ht); vstat_.swap(vs);
    vcache_ = detail::select_items(vcache_, keep);
    dirty_ = true;
  }
  void remove_edges(const std::vector<size_t> &gone) {
    if (gone.empty()) return;
    std::vector<bool> out(edgeCount(), false);
    for (size_t e : gone) out[e] = true;
    std::vector<size_t> keep;
    for (size_t e = 0; e < edgeCount(); e++) if (!out[e]) keep.push_back(e);
    std::vector<int32_t> ed(2 * keep.size());
    std::vector<double> w(weights_.empty() ? 0 : keep.size());
    std::vector<uint8_t> es(keep.size());
    for (size_t i = 0; i < keep.size(); i++) {
      ed[2 * i] = edges_[2 * keep[i]]; ed[2 * i + 1] = edges_[2 * keep[i] + 1];
      if (!weights_.empty()) w[i] = weights_[keep[i]];
      es[i] = estat_[keep[i]];
    }
    edges_.swap(ed); weights_.swap(w); estat_.swap(es);
    ecache_ = detail::select_items(ecache_, keep);
    dirty_ = true;
  }

  const VoxelBackboneValidityChecker &vc_;
  const VoxelBackboneMotionValidator *mv_ = nullptr;
  size_t S_ = 0;
  uint64_t seed_ = 0, next_candidate_ = 0;
  std::vector<double> lo_, hi_;
  std::vector<double> states_, tips_, weights_;
  std::vector<uint8_t> has_tip_, vstat_, estat_;
  std::vector<int32_t> edges_;
  VoxelCaches vcache_, ecache_;
  bool caches_given_ = false;
  bool star_ = false;
  size_t k_ = 5;                       // magic::DEFAULT_NEAREST_NEIGHBORS_LAZY (:125)
  double max_distance_ = 0.0;
  int lm_ = -1, lm_threads_ = 0;
  BuildReport report_;
  tr_roadmap *rm_ = nullptr;
  bool dirty_ = true;
  bool tips_synced_ = false;
};

}  // namespace motion_planning
}  // namespace tendon_hip
