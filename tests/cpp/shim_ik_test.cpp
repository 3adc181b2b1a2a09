// Exercises the tip-IK side of include/tendon_hip_shim.hpp the way reference-side C++ would: tip_control::inverse_kinematics,
// TendonRobot::tip_jacobian_batch and VoxelCachedLazyPRM::roadmapIk (RMAP_IK_SIMPLE).  Prints results for
// tests/test_cpp_shim_ik.py to compare with the oracle.
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "tendon_hip_shim.hpp"

using namespace tendon_hip;

static tendon::TendonRobot config3() {                  // workloads.robot_config3
  const double c1[4] = {3.0, -2.0, 4.0, -5.0}, c2[4] = {10.0, 15.0, -12.0, 8.0}, d1[4] = {-0.01, 0.005, 0.0, -0.005};
  tendon::TendonRobot robot;
  robot.specs.dL = 0.2 / 128;
  for (int k = 0; k < 4; k++) {
    tendon::TendonSpecs t;
    t.C = {M_PI * k / 2, c1[k], c2[k]};
    t.D = {0.01, d1[k], 0.0};
    robot.tendons.push_back(t);
  }
  return robot;
}

static void print_state(const char *tag, const std::vector<double> &x) {
  std::printf("%s", tag);
  for (double v : x) std::printf(" %.17g", v);
}

int main(int argc, char **argv) {
  const bool compile_only = argc > 1 && std::string(argv[1]) == "--no-gpu";
  tendon::TendonRobot robot = config3();
  // a wrong state size is std::invalid_argument before anything touches the device
  int caught = 0;
  try { tip_control::inverse_kinematics(robot, {1.0, 2.0}, {0.0, 0.0, 0.2}); } catch (const std::invalid_argument &e) {
    caught += std::string(e.what()) == "State is not the right size";
  }
  try { robot.tip_jacobian_batch({1.0, 2.0, 3.0}, 1); } catch (const std::invalid_argument &) { caught++; }
  const tip_control::Bounds b = tip_control::Bounds::from_robot(robot);
  std::printf("caught %d bounds %zu %g %g\n", caught, b.upper.size(), b.lower[0], b.upper[3]);
  if (compile_only) return caught == 2 ? 0 : 1;

  // inverse_kinematics to the tips of known states, from perturbed starts
  const std::vector<std::vector<double>> goals = {{3, 8, 1, 5}, {10, 2, 6, 0.5}, {1, 1, 12, 9}, {7, 7, 7, 7}};
  const double kick[4] = {1.2, -0.8, 0.9, -1.1};
  for (auto &g : goals) {
    const auto tip = robot.shape(g).p.back();
    std::vector<double> start(g);
    for (int j = 0; j < 4; j++) start[j] = std::max(0.0, g[j] + kick[j]);
    const auto r = tip_control::inverse_kinematics(robot, start, {tip[0], tip[1], tip[2]}, 60, 0.1, 1e-16, 1e-12, 1e-6);
    print_state("ik", g);
    print_state(" |", r.state);
    std::printf(" | %.17g %.17g %.17g %.17g %d %d\n", r.tip[0], r.tip[1], r.tip[2], r.error, r.iters, r.num_fk_calls);
  }
  {
    std::vector<double> tips;
    const auto J = robot.tip_jacobian_batch({3, 8, 1, 5}, 1, 1e-6, &tips);
    std::printf("jac %zu %.17g %.17g\n", J.size(), J[0], tips[2]);
  }

  // roadmapIk on a 2000-milestone roadmap in free space
  collision::VoxelOctree vox(256);
  vox.set_xlim(-0.25, 0.25); vox.set_ylim(-0.25, 0.25); vox.set_zlim(-0.25, 0.25);
  motion_planning::VoxelEnvironment env;
  motion_planning::VoxelBackboneValidityChecker vc(robot, env, vox);
  motion_planning::VoxelBackboneMotionValidator mv(vc);
  motion_planning::VoxelCachedLazyPRM prm(vc, mv, 5);
  prm.createRoadmap(2000, motion_planning::VoxelCachedLazyPRM::ValidateVertices);
  const auto &vt = prm.tipPositions();
  const std::array<double, 3> req = {vt[3 * 123] + 0.002, vt[3 * 123 + 1] - 0.001, vt[3 * 123 + 2] + 0.0015};
  std::printf("request %.17g %.17g %.17g\n", req[0], req[1], req[2]);
  try { prm.roadmapIk(req, 1e-4, 5, motion_planning::VoxelCachedLazyPRM::RMAP_IK_AUTO_ADD); } catch (const std::invalid_argument &) {
    std::printf("auto_add unsupported\n");
  }
  auto res = prm.roadmapIk(req, 1e-4, 5);
  if (res) {
    print_state("rmap", res->controls);
    std::printf(" | %.17g %.17g %.17g %.17g %zu\n", res->tip_position[0], res->tip_position[1], res->tip_position[2], res->error,
                res->neighbor_vertex);
  }
  // a block of obstacles around the request: every IK solution collides; the answer is the last valid state towards one
  const double h = 0.006, dx = 0.5 / 256;
  int lo[3], hi[3];
  for (int a = 0; a < 3; a++) { lo[a] = (int)std::floor((req[a] - h + 0.25) / dx); hi[a] = (int)std::floor((req[a] + h + 0.25) / dx); }
  collision::VoxelOctree blocked(256);
  blocked.set_xlim(-0.25, 0.25); blocked.set_ylim(-0.25, 0.25); blocked.set_zlim(-0.25, 0.25);
  for (int ix = lo[0]; ix <= hi[0]; ix++) for (int iy = lo[1]; iy <= hi[1]; iy++) for (int iz = lo[2]; iz <= hi[2]; iz++) blocked.set_cell(ix, iy, iz);
  std::printf("box %d %d %d %d %d %d\n", lo[0], hi[0], lo[1], hi[1], lo[2], hi[2]);
  motion_planning::VoxelBackboneValidityChecker vc2(robot, env, blocked);   // the robot's context: the planner now sees the block
  prm.clearValidity();
  res = prm.roadmapIk(req, 1e-4, 5);
  if (res) {
    print_state("blocked", res->controls);
    std::printf(" | %.17g %.17g %.17g %.17g %zu\n", res->tip_position[0], res->tip_position[1], res->tip_position[2], res->error,
                res->neighbor_vertex);
  }
  return 0;
}
