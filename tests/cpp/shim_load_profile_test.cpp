// Load profiles through the C++ shim (include/tendon_hip_shim.hpp): TendonRobot::set_load_profile / clear_load_profile and what
// general_shape and generalShapeBatch return under a profile, printed as hexadecimal floats so that
// tests/test_cpp_shim_load_profile.py can compare them with the Python interface bit for bit.
// With a file (tests/test_cpp_shim_loaded_edges.py's layout, written by the test) it then builds a checker and prints checkMotionBatch
// with last_valid_t under setLoads(wrench, dist, profile_s, profile_w, world): after the call, after a refused call (the loads and
// the profile must be the ones before it), after a setLoads without a profile, and after clearLoads.
//   shim_load_profile_test --no-gpu   only the argument check that needs no device
//   shim_load_profile_test [file]     int64 n_tendons, n_coef, n_edges, grid N; double half, dL; C [n_tendons][n_coef]; D likewise;
//                                     uint64 blocks [(N / 4)^3]; a [n_edges][n_tendons + 1]; b likewise; wrench [6]; dist [6];
//                                     profile knots [3]; weights [3]
#include <cstdio>
#include <cstring>
#include <stdexcept>

#include "tendon_hip_shim.hpp"

using namespace tendon_hip;

static tendon::TendonRobot config1(bool rotation) {
  tendon::TendonRobot r;
  const double pi = 3.14159265358979323846;
  for (int k = 0; k < 3; k++) {
    tendon::TendonSpecs t;
    t.C = {2 * pi * k / 3};
    t.D = {0.01};
    r.tendons.push_back(t);
  }
  r.enable_rotation = rotation;
  return r;
}

static void print(const char *tag, const tendon::TendonResult &res) {
  std::printf("%s %d", tag, res.converged ? 1 : 0);
  for (int k = 0; k < 3; k++) std::printf(" %a", res.v_i[k]);
  for (int k = 0; k < 3; k++) std::printf(" %a", res.u_i[k]);
  std::printf(" %a", res.L);
  for (double l : res.L_i) std::printf(" %a", l);
  for (auto &q : res.p) std::printf(" %a %a %a", q[0], q[1], q[2]);
  std::printf("\n");
}

template <class T>
static void rd(std::FILE *f, T *p, size_t n) {
  if (std::fread(p, sizeof(T), n, f) != n) throw std::runtime_error("short input file");
}

static void print_edges(const char *tag, motion_planning::VoxelBackboneMotionValidator &mv, const std::vector<double> &a,
                        const std::vector<double> &b, size_t E) {
  std::vector<int32_t> nfk;
  std::vector<double> t;
  const std::vector<bool> ok = mv.checkMotionBatch(a, b, E, &nfk, &t);
  std::printf("%s", tag);
  for (size_t i = 0; i < ok.size(); i++) std::printf(" %d:%d:%a", ok[i] ? 1 : 0, nfk[i], t[i]);
  std::printf("\n");
}

template <class F>
static void expect_invalid(const char *what, bool no_gpu, F call) {
  try {
    call();
    std::printf("%s: no exception\n", what);
  } catch (const std::invalid_argument &) {
    std::printf("%s: invalid_argument\n", what);
  } catch (const std::exception &e) {
    if (!no_gpu) throw;
    std::printf("%s: %s\n", what, e.what());
  }
}

// the checker's side: setLoads with a profile, its failure modes, clearLoads
static int checker_part(const char *path) {
  std::FILE *f = std::fopen(path, "rb");
  if (!f) return 2;
  int64_t hd[4];
  double hf[2];
  rd(f, hd, 4);
  rd(f, hf, 2);
  const size_t N = (size_t)hd[0], nc = (size_t)hd[1], E = (size_t)hd[2], G = (size_t)hd[3], S = N + 1;
  std::vector<double> C(N * nc), D(N * nc);
  rd(f, C.data(), C.size());
  rd(f, D.data(), D.size());
  collision::VoxelOctree vox(G);
  vox.set_xlim(-hf[0], hf[0]); vox.set_ylim(-hf[0], hf[0]); vox.set_zlim(-hf[0], hf[0]);
  rd(f, vox.blocks().data(), vox.blocks().size());
  std::vector<double> a(E * S), b(E * S), wrench(6), dist(6), ps(3), pw(3);
  rd(f, a.data(), a.size());
  rd(f, b.data(), b.size());
  rd(f, wrench.data(), 6);
  rd(f, dist.data(), 6);
  rd(f, ps.data(), 3);
  rd(f, pw.data(), 3);
  std::fclose(f);
  tendon::TendonRobot robot;
  robot.specs.dL = hf[1];
  robot.enable_rotation = true;
  for (size_t k = 0; k < N; k++) {
    tendon::TendonSpecs t;
    t.C.assign(C.begin() + k * nc, C.begin() + (k + 1) * nc);
    t.D.assign(D.begin() + k * nc, D.begin() + (k + 1) * nc);
    robot.tendons.push_back(t);
  }
  motion_planning::VoxelEnvironment venv;
  motion_planning::VoxelBackboneValidityChecker vc(robot, venv, vox);
  motion_planning::VoxelBackboneMotionValidator mv(vc);
  print_edges("edges_unloaded", mv, a, b, E);
  vc.setLoads(wrench, dist, ps, pw, true);
  std::printf("has_profile %d\n", vc.hasLoadProfile() ? 1 : 0);
  print_edges("edges_profile", mv, a, b, E);
  // refused calls leave the world-frame loads and the profile in force
  expect_invalid("checker order", false, [&] { vc.setLoads({}, dist, {0.1, 0.1, 0.2}, pw, false); });
  expect_invalid("checker sizes", false, [&] { vc.setLoads({}, dist, ps, {1.0}, false); });
  expect_invalid("checker loads", false, [&] { vc.setLoads(std::vector<double>(5, 0.0), dist, ps, pw, false); });
  std::printf("has_profile %d frame %d\n", vc.hasLoadProfile() ? 1 : 0, (int)vc.loads()->frame);
  print_edges("edges_kept", mv, a, b, E);
  vc.setLoads(wrench, dist, true);                       // a load set without a profile removes the earlier one's
  std::printf("has_profile %d\n", vc.hasLoadProfile() ? 1 : 0);
  print_edges("edges_plain", mv, a, b, E);
  vc.setLoads(wrench, dist, ps, pw, true);
  vc.clearLoads();
  std::printf("has_profile %d loads %d\n", vc.hasLoadProfile() ? 1 : 0, vc.loads() ? 1 : 0);
  print_edges("edges_cleared", mv, a, b, E);
  return 0;
}

int main(int argc, char **argv) {
  const bool no_gpu = argc > 1 && !std::strcmp(argv[1], "--no-gpu");
  tendon::TendonRobot robot = config1(true);
  expect_invalid("sizes", no_gpu, [&] { robot.set_load_profile({0.0, 0.1}, {1.0}); });      // refused before any device call
  if (no_gpu) return 0;
  expect_invalid("order", false, [&] { robot.set_load_profile({0.1, 0.1}, {1.0, 2.0}); });
  expect_invalid("finite", false, [&] { robot.set_load_profile({0.0, 0.1}, {1.0, 1.0 / 0.0}); });
  expect_invalid("none", false, [&] { robot.set_load_profile({}, {}); });
  std::printf("table %zu\n", robot.load_profile_table().size());
  const tendon::TendonRobot::V3 f_e{0.0, -2.4525, 0.0}, l_e{0.0, 0.0, 0.0}, F_e{0.05, -0.03, 0.02}, L_e{1e-3, -2e-3, 5e-4};
  const std::vector<double> state{3.0, 7.0, 1.0, 0.4};
  const std::vector<double> states{3.0, 7.0, 1.0, 0.4, 0.0, 0.0, 0.0, -1.0, 12.0, 0.5, 5.0, 2.0};
  const std::vector<double> wrench{0.05, -0.03, 0.02, 1e-3, -2e-3, 5e-4, 0, 0, 0, 0, 0, 0, -0.02, 0.01, 0.0, 0, 1e-3, 0};
  const std::vector<double> dist{0.0, -2.4525, 0.0, 0.0, 0.0, 0.0};
  robot.set_load_profile({0.0, 0.15, 0.2}, {1.0, 1.0, 3.0});
  const std::vector<double> tab = robot.load_profile_table();
  std::printf("weights");
  for (double w : tab) std::printf(" %a", w);
  std::printf("\n");
  print("single", robot.general_shape(state, f_e, l_e, F_e, L_e));
  for (const auto &res : robot.generalShapeBatch(states, 3, wrench, dist)) print("batch", res);
  robot.clear_load_profile();
  std::printf("table %zu\n", robot.load_profile_table().size());
  print("cleared", robot.general_shape(state, f_e, l_e, F_e, L_e));
  tendon::TendonRobot ret = config1(false);
  ret.enable_retraction = true;
  try {
    ret.set_load_profile({0.0, 0.2}, {1.0, 2.0});
    std::printf("retraction: no exception\n");
  } catch (const std::invalid_argument &) {
    std::printf("retraction: invalid_argument\n");
  } catch (const std::runtime_error &) {
    std::printf("retraction: runtime_error\n");
  }
  return argc > 1 ? checker_part(argv[1]) : 0;
}
