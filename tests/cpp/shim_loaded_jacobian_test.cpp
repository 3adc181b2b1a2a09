// The loaded tip Jacobian through the C++ shim (include/tendon_hip_shim.hpp): TendonRobot::tip_jacobian_loaded_batch and
// tip_control::damped_resolved_rate_update* print what they return as hexadecimal floats, so
// tests/test_cpp_shim_loaded_jacobian.py can compare them with the Python interface bit for bit.
//   shim_loaded_jacobian_test --no-gpu    only the argument checks that need no device
//   shim_loaded_jacobian_test FILE        FILE: n, then n x 3 states, the 6 numbers of the wrench, the 6 of the distributed load and
//                                         the 3 of a tip displacement
#include <cstdio>
#include <cstring>
#include <stdexcept>

#include "tendon_hip_shim.hpp"

using namespace tendon_hip;

static tendon::TendonRobot config1() {
  tendon::TendonRobot r;
  const double pi = 3.14159265358979323846;
  for (int k = 0; k < 3; k++) {
    tendon::TendonSpecs t;
    t.C = {2 * pi * k / 3};
    t.D = {0.01};
    r.tendons.push_back(t);
  }
  return r;
}

static void row(const char *tag, const double *x, size_t m) {
  std::printf("%s", tag);
  for (size_t q = 0; q < m; q++) std::printf(" %a", x[q]);
  std::printf("\n");
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  const bool no_gpu = !std::strcmp(argv[1], "--no-gpu");
  tendon::TendonRobot robot = config1();
  try {
    robot.tip_jacobian_loaded_batch({1.0, 2.0}, 1, {});
    std::printf("no exception\n");
  } catch (const std::invalid_argument &) {
    std::printf("caught invalid_argument\n");
  }
  try {
    robot.tip_jacobian_loaded_batch({1.0, 2.0, 3.0}, 1, {1.0, 2.0});
    std::printf("no exception\n");
  } catch (const std::invalid_argument &) {
    std::printf("caught invalid_argument (loads)\n");
  }
  try {
    tip_control::damped_resolved_rate_update(robot, {1.0, 2.0}, {0, 0, 1e-3});
    std::printf("no exception\n");
  } catch (const std::invalid_argument &) {
    std::printf("caught invalid_argument (update)\n");
  }
  if (no_gpu) return 0;
  std::FILE *f = std::fopen(argv[1], "r");
  if (!f) return 2;
  int n = 0;
  if (std::fscanf(f, "%d", &n) != 1 || n < 1) return 2;
  std::vector<double> states(3 * (size_t)n), wrench(6), dist(6);
  std::array<double, 3> v{};
  bool ok = true;
  for (double &x : states) ok = ok && std::fscanf(f, "%la", &x) == 1;
  for (double &x : wrench) ok = ok && std::fscanf(f, "%la", &x) == 1;
  for (double &x : dist) ok = ok && std::fscanf(f, "%la", &x) == 1;
  for (double &x : v) ok = ok && std::fscanf(f, "%la", &x) == 1;
  std::fclose(f);
  if (!ok) return 2;
  int64_t rounds = 0;
  const auto out = robot.tip_jacobian_loaded_batch(states, (size_t)n, wrench, dist, tendon::LoadedJacobianOptions(), {}, &rounds);
  for (int i = 0; i < n; i++) {
    std::printf("state %d %d %lld\n", i, (int)out.equilibrium[(size_t)i], (long long)out.n_integrations[(size_t)i]);
    row("J", out.J.data() + (size_t)i * 9, 9);
    row("compliance", out.compliance.data() + (size_t)i * 18, 18);
    row("tips", out.tips.data() + (size_t)i * 3, 3);
    row("vu0", out.vu0.data() + (size_t)i * 6, 6);
  }
  std::printf("rounds %lld\n", (long long)rounds);
  const std::vector<double> q{states[0], states[1], states[2]};
  const auto next = tip_control::damped_resolved_rate_update(robot, q, v);
  row("update", next.data(), next.size());
  const auto next_loaded = tip_control::damped_resolved_rate_updateLoaded(robot, q, v, wrench, dist);
  row("update_loaded", next_loaded.data(), next_loaded.size());
  tendon::TendonRobot ret = config1();
  ret.enable_retraction = true;
  try {
    ret.tip_jacobian_loaded_batch({1.0, 2.0, 3.0, 0.0}, 1, wrench, dist);
    std::printf("no exception\n");
  } catch (const std::invalid_argument &) {
    std::printf("retraction invalid_argument\n");
  } catch (const std::runtime_error &e) {
    std::printf("retraction runtime_error: %s\n", e.what());
  }
  return 0;
}
