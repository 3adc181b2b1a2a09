// The loaded FK through the C++ shim (include/tendon_hip_shim.hpp): general_shape and generalShapeBatch print what they return as
// hexadecimal floats, so tests/test_cpp_shim_loaded.py can compare them with the Python interface bit for bit.
//   shim_loaded_test --no-gpu   only the argument checks that need no device
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

int main(int argc, char **argv) {
  const bool no_gpu = argc > 1 && !std::strcmp(argv[1], "--no-gpu");
  tendon::TendonRobot robot = config1(true);
  try {
    robot.general_shape({1.0, 2.0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0});
    std::printf("no exception\n");
  } catch (const std::invalid_argument &) {
    std::printf("caught invalid_argument\n");
  } catch (const std::exception &e) {
    if (!no_gpu) throw;
    std::printf("caught %s\n", e.what());
  }
  if (no_gpu) return 0;
  const tendon::TendonRobot::V3 f_e{0.0, -2.4525, 0.0}, l_e{0.0, 0.0, 0.0}, F_e{0.05, -0.03, 0.02}, L_e{1e-3, -2e-3, 5e-4};
  const std::vector<double> state{3.0, 7.0, 1.0, 0.4};
  print("single", robot.general_shape(state, f_e, l_e, F_e, L_e));
  print("straight", robot.general_shape(state, f_e, l_e, F_e, L_e, tendon::TendonRobot::V3{0, 0, 0}, tendon::TendonRobot::V3{0, 0, 1}));
  const std::vector<double> states{3.0, 7.0, 1.0, 0.4, 0.0, 0.0, 0.0, -1.0, 12.0, 0.5, 5.0, 2.0};
  const std::vector<double> wrench{0.05, -0.03, 0.02, 1e-3, -2e-3, 5e-4, 0, 0, 0, 0, 0, 0, -0.02, 0.01, 0.0, 0, 1e-3, 0};
  const std::vector<double> dist{0.0, -2.4525, 0.0, 0.0, 0.0, 0.0};
  std::vector<int32_t> iters, calls;
  const auto batch = robot.generalShapeBatch(states, 3, wrench, dist, {}, tendon::ShootOptions(), &iters, &calls);
  for (size_t i = 0; i < batch.size(); i++) {
    print("batch", batch[i]);
    std::printf("counters %d %d\n", iters[i], calls[i]);
  }
  tendon::TendonRobot ret = config1(false);
  ret.enable_retraction = true;
  try {
    ret.general_shape({1.0, 2.0, 3.0, 0.0}, f_e, l_e, F_e, L_e);
    std::printf("no exception\n");
  } catch (const std::invalid_argument &) {
    std::printf("retraction invalid_argument\n");
  } catch (const std::runtime_error &) {
    std::printf("retraction runtime_error\n");
  }
  return 0;
}
