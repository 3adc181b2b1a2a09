// The loaded FK of a robot WITH retraction through the C++ shim (include/tendon_hip_shim.hpp): general_shape, generalShapeBatch and
// loaded_tips_batch print what they return as hexadecimal floats, so tests/test_cpp_shim_loaded_retraction.py can compare them with
// the Python interface bit for bit.  Every result has the state's own point count.
//   shim_loaded_retraction_test --no-gpu   only the argument checks that need no device
#include <cstdio>
#include <cstring>
#include <stdexcept>

#include "tendon_hip_shim.hpp"

using namespace tendon_hip;

// config 1's robot with rotation and retraction: states are (tau_1, tau_2, tau_3, theta, s_start)
static tendon::TendonRobot robot_with_retraction() {
  tendon::TendonRobot r;
  const double pi = 3.14159265358979323846;
  for (int k = 0; k < 3; k++) {
    tendon::TendonSpecs t;
    t.C = {2 * pi * k / 3};
    t.D = {0.01};
    r.tendons.push_back(t);
  }
  r.enable_rotation = true;
  r.enable_retraction = true;
  return r;
}

static void print(const char *tag, const tendon::TendonResult &res) {
  std::printf("%s %d %zu %zu %zu", tag, res.converged ? 1 : 0, res.t.size(), res.p.size(), res.R.size());
  std::printf(" %a %a", res.t.front(), res.t.back());
  for (int k = 0; k < 3; k++) std::printf(" %a", res.v_i[k]);
  for (int k = 0; k < 3; k++) std::printf(" %a", res.u_i[k]);
  std::printf(" %a", res.L);
  for (double l : res.L_i) std::printf(" %a", l);
  for (auto &q : res.p) std::printf(" %a %a %a", q[0], q[1], q[2]);
  std::printf("\n");
}

int main(int argc, char **argv) {
  const bool no_gpu = argc > 1 && !std::strcmp(argv[1], "--no-gpu");
  tendon::TendonRobot robot = robot_with_retraction();
  try {
    robot.general_shape({1.0, 2.0, 3.0, 0.0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0});      // no s_start
    std::printf("no exception\n");
  } catch (const std::invalid_argument &) {
    std::printf("caught invalid_argument\n");
  } catch (const std::exception &e) {
    if (!no_gpu) throw;
    std::printf("caught %s\n", e.what());
  }
  if (no_gpu) return 0;
  try {                                                       // a context that was never opened refuses, as it always did
    robot.general_shape({3.0, 7.0, 1.0, 0.4, 0.0731}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0});
    std::printf("closed: no exception\n");
  } catch (const std::runtime_error &) {
    std::printf("closed: runtime_error\n");
  }
  robot.set_loaded_retraction();
  const tendon::TendonRobot::V3 f_e{0.0, -2.4525, 0.0}, l_e{0.0, 0.0, 0.0}, F_e{0.05, -0.03, 0.02}, L_e{1e-3, -2e-3, 5e-4};
  print("single", robot.general_shape({3.0, 7.0, 1.0, 0.4, 0.0731}, f_e, l_e, F_e, L_e));
  // a retracted state, an unretracted one, a two-point backbone, s_start beyond L (one point at the origin)
  const std::vector<double> states{3.0, 7.0, 1.0, 0.4, 0.0731, 0.0, 0.0, 0.0, -1.0, 0.0, 12.0, 0.5, 5.0, 2.0, 0.1972, 1.0, 2.0, 3.0, 0.0, 0.25};
  const std::vector<double> wrench{0.05, -0.03, 0.02, 1e-3, -2e-3, 5e-4};
  const std::vector<double> dist{0.0, -2.4525, 0.0, 0.0, 0.0, 0.0};
  const auto batch = robot.generalShapeBatch(states, 4, wrench, dist);
  for (size_t i = 0; i < batch.size(); i++) print("batch", batch[i]);
  tr_edge_loads ld{};
  for (int q = 0; q < 6; q++) { ld.wrench[q] = wrench[q]; ld.dist[q] = dist[q]; }
  ld.frame = TR_LOAD_FRAME_BASE;
  const auto tips = robot.loaded_tips_batch(states, 4, ld);
  for (size_t i = 0; i < 4; i++) std::printf("tip %d %a %a %a\n", (int)tips.converged[i], tips.tips[3 * i], tips.tips[3 * i + 1], tips.tips[3 * i + 2]);
  return 0;
}
