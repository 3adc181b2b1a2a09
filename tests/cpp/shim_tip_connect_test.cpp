// The accurate connection rule through include/tendon_hip_shim.hpp only: motion_planning::VoxelCachedLazyPRM::nearestStates,
// roadmapIkBatchAccurate and solveToTipsAccurate on a roadmap built by createRoadmap, written as raw arrays for
// tests/test_cpp_shim_tip_connect.py to compare with what the Python API returns on the same roadmap.
//
//   shim_tip_connect_test <grid file: 64^3 uint64 blocks of a 256^3 grid over [-0.25, 0.25]^3> <output directory>
#include <array>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>

#include "tendon_hip_shim.hpp"

using namespace tendon_hip;
using Planner = motion_planning::VoxelCachedLazyPRM;

static std::string g_dir;

template <class T> static void dump(const std::string &name, const std::vector<T> &v) {
  const std::string path = g_dir + "/" + name;
  FILE *f = std::fopen(path.c_str(), "wb");
  if (!f) { std::perror(path.c_str()); std::exit(2); }
  if (!v.empty() && std::fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) { std::perror(path.c_str()); std::exit(2); }
  std::fclose(f);
}
static void dump_caches(const std::string &tag, const motion_planning::VoxelCaches &c) {
  std::vector<uint8_t> usable(c.usable.size());
  for (size_t i = 0; i < usable.size(); i++) usable[i] = c.usable[i];
  dump(tag + "_off.i64", c.offsets); dump(tag + "_ids.u32", c.block_ids); dump(tag + "_masks.u64", c.masks); dump(tag + "_usable.u8", usable);
}
static void dump_ik(const std::string &tag, const Planner::AccurateTipResults &r) {
  dump(tag + "_controls.f64", r.controls); dump(tag + "_tips.f64", r.tip_positions); dump(tag + "_error.f64", r.error);
  dump(tag + "_vertex.i32", r.neighbor_vertex); dump(tag + "_ikvertex.i32", r.ik_vertex); dump(tag + "_outcome.i32", r.outcome);
  dump(tag + "_t.f64", r.last_valid_t);
  dump(tag + "_stats.i64", std::vector<int64_t>(r.connect_stats.begin(), r.connect_stats.end()));
}

int main(int argc, char **argv) {
  if (argc < 3) { std::fprintf(stderr, "usage: %s <grid file> <output directory>\n", argv[0]); return 2; }
  g_dir = argv[2];
  // workloads.robot_config3
  tendon::TendonRobot robot;
  robot.specs.dL = 0.2 / 128;
  const double c1[4] = {3.0, -2.0, 4.0, -5.0}, c2[4] = {10.0, 15.0, -12.0, 8.0}, d1[4] = {-0.01, 0.005, 0.0, -0.005};
  for (int k = 0; k < 4; k++) {
    tendon::TendonSpecs t;
    t.C = {M_PI * k / 2, c1[k], c2[k]};
    t.D = {0.01, d1[k], 0.0};
    robot.tendons.push_back(t);
  }
  collision::VoxelOctree vox(256);
  vox.set_xlim(-0.25, 0.25); vox.set_ylim(-0.25, 0.25); vox.set_zlim(-0.25, 0.25);
  {
    FILE *f = std::fopen(argv[1], "rb");
    if (!f || std::fread(vox.blocks().data(), sizeof(uint64_t), vox.blocks().size(), f) != vox.blocks().size()) { std::perror(argv[1]); return 2; }
    std::fclose(f);
  }
  motion_planning::VoxelEnvironment env;
  motion_planning::VoxelBackboneValidityChecker vc(robot, env, vox);
  motion_planning::VoxelBackboneMotionValidator mv(vc);
  Planner prm(vc, mv, /*seed=*/11);
  prm.setMaxNearestNeighbors(8);
  prm.setRange(1e9);
  prm.createRoadmap(2000, Planner::ValidateVertices | Planner::ValidateEdges);
  if (prm.milestoneCount() != 2000) { std::fprintf(stderr, "%zu milestones\n", prm.milestoneCount()); return 3; }
  dump("states.f64", prm.states()); dump("tips.f64", prm.tipPositions()); dump("edges.i32", prm.edges());
  dump_caches("vc", prm.vertexVoxels()); dump_caches("ec", prm.edgeVoxels());

  // requests near the tips of some vertices, and some well away from every tip
  const std::vector<double> &vt = prm.tipPositions();
  const size_t n = 96;
  std::vector<std::array<double, 3>> requests(n);
  std::vector<int32_t> starts(n);
  std::vector<double> flat;
  for (size_t j = 0; j < n; j++) {
    const size_t v = (j * 17 + 123) % 2000;
    const double far = j % 3 == 2 ? 0.03 : 0.0;
    requests[j] = {vt[3 * v] + 0.002 + far, vt[3 * v + 1] - 0.001 - far, vt[3 * v + 2] + 0.0015 + far};
    starts[j] = (int32_t)((j * 131 + 7) % 2000);
    flat.insert(flat.end(), requests[j].begin(), requests[j].end());
  }
  dump("requests.f64", flat); dump("starts.i32", starts);

  // the state-space neighbours of states off the roadmap: midpoints of vertex pairs, and the vertices themselves
  std::vector<double> queries;
  const std::vector<double> &st = prm.states();
  for (size_t j = 0; j < 200; j++) {
    const size_t a = (j * 29 + 5) % 2000, b = (j * 31 + 11) % 2000;
    for (size_t d = 0; d < 4; d++) queries.push_back(j % 4 == 3 ? st[4 * a + d] : 0.5 * (st[4 * a + d] + st[4 * b + d]));
  }
  dump("queries.f64", queries);
  const Planner::NearestStates near = prm.nearestStates(queries, 7);
  dump("near_vertices.i32", near.vertices); dump("near_distance.f64", near.distance);
  const Planner::NearestStates near_b = prm.nearestStates(queries, 7, near.distance[3]);
  dump("nearb_vertices.i32", near_b.vertices); dump("nearb_distance.f64", near_b.distance);

  const Planner::AccurateTipResults ik = prm.roadmapIkBatchAccurate(requests, 1e-4, 5, 6);
  dump_ik("ik", ik);
  const Planner::AccurateTipSolution sol = prm.solveToTipsAccurate(starts, requests, 1e-4, 5, 6);
  dump_ik("sol", sol.ik);
  dump("sol_status.i32", sol.roadmap.status); dump("sol_cost.f64", sol.roadmap.cost);
  std::vector<int64_t> off(1, 0);
  std::vector<int32_t> pv;
  for (const auto &p : sol.roadmap.paths) { pv.insert(pv.end(), p.begin(), p.end()); off.push_back((int64_t)pv.size()); }
  dump("sol_path_off.i64", off); dump("sol_path_v.i32", pv);

  int caught = 0;
  try { prm.solveToTipsAccurate({0, 1}, requests); } catch (const std::invalid_argument &) { caught++; }
  try { prm.roadmapIkBatchAccurate(requests, 1e-4, 5, 65); } catch (const std::invalid_argument &) { caught++; }
  try { prm.nearestStates(queries, 0); } catch (const std::invalid_argument &) { caught++; }
  try { prm.roadmapIk(requests[0], 1e-4, 5, Planner::RMAP_IK_ACCURATE); } catch (const std::invalid_argument &) { caught++; }
  if (caught != 4) { std::fprintf(stderr, "%d of 4 errors\n", caught); return 3; }
  std::printf("tip connect queries written\n");
  return 0;
}
