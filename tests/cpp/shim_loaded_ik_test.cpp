// Tip IK on loaded shapes through the C++ shim (include/tendon_hip_shim.hpp): inverseKinematicsLoadedBatch and
// inverseKinematicsLoaded print what they return as hexadecimal floats, so tests/test_cpp_shim_loaded_ik.py can compare them with
// the Python interface bit for bit.
//   shim_loaded_ik_test --no-gpu    only the argument checks that need no device
//   shim_loaded_ik_test FILE        FILE: n, then n x 3 start states, n x 3 goals and the 6 numbers of the distributed load
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

static void print(const char *tag, const tip_control::LoadedIKResult &r) {
  std::printf("%s %d %d %d %a", tag, r.equilibrium ? 1 : 0, r.iters, r.num_fk_calls, r.error);
  for (double x : r.state) std::printf(" %a", x);
  for (double x : r.tip) std::printf(" %a", x);
  for (double x : r.vu0) std::printf(" %a", x);
  std::printf("\n");
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  const bool no_gpu = !std::strcmp(argv[1], "--no-gpu");
  tendon::TendonRobot robot = config1();
  try {
    tip_control::inverseKinematicsLoaded(robot, {1.0, 2.0}, {0, 0, 0.2}, {}, {});
    std::printf("no exception\n");
  } catch (const std::invalid_argument &) {
    std::printf("caught invalid_argument\n");
  }
  try {
    tip_control::inverseKinematicsLoadedBatch(robot, {1.0, 2.0, 3.0}, 1, {{0, 0, 0.2}}, {1.0, 2.0}, {});
    std::printf("no exception\n");
  } catch (const std::invalid_argument &) {
    std::printf("caught invalid_argument (loads)\n");
  }
  if (no_gpu) return 0;
  std::FILE *f = std::fopen(argv[1], "r");
  if (!f) return 2;
  int n = 0;
  if (std::fscanf(f, "%d", &n) != 1 || n < 1) return 2;
  std::vector<double> starts(3 * (size_t)n), dist(6);
  std::vector<std::array<double, 3>> goals((size_t)n);
  bool ok = true;
  for (double &x : starts) ok = ok && std::fscanf(f, "%la", &x) == 1;
  for (auto &g : goals) for (double &x : g) ok = ok && std::fscanf(f, "%la", &x) == 1;
  for (double &x : dist) ok = ok && std::fscanf(f, "%la", &x) == 1;
  std::fclose(f);
  if (!ok) return 2;
  int64_t rounds[2] = {0, 0};
  const auto batch = tip_control::inverseKinematicsLoadedBatch(robot, starts, (size_t)n, goals, {}, dist, tip_control::LoadedIKOptions(), rounds);
  for (const auto &r : batch) print("batch", r);
  std::printf("rounds %lld %lld\n", (long long)rounds[0], (long long)rounds[1]);
  print("single", tip_control::inverseKinematicsLoaded(robot, {starts[0], starts[1], starts[2]}, goals[0], {}, dist));
  tip_control::LoadedIKOptions one;
  one.max_iters = 1;
  print("one_iter", tip_control::inverseKinematicsLoaded(robot, {starts[0], starts[1], starts[2]}, goals[0], {}, dist, one));
  tendon::TendonRobot ret = config1();
  ret.enable_retraction = true;
  try {
    tip_control::inverseKinematicsLoaded(ret, {1.0, 2.0, 3.0, 0.0}, goals[0], {}, dist);
    std::printf("no exception\n");
  } catch (const std::invalid_argument &) {
    std::printf("retraction invalid_argument\n");
  } catch (const std::runtime_error &) {
    std::printf("retraction runtime_error\n");
  }
  return 0;
}
