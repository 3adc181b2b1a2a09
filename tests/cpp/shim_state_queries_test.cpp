// Queries between arbitrary states through include/tendon_hip_shim.hpp only: motion_planning::VoxelCachedLazyPRM::attachStates,
// solveSeeded and solveStates on a roadmap built by createRoadmap, written as raw arrays for tests/test_cpp_shim_state_queries.py to
// compare with what the Python API returns on the same roadmap.
//
//   shim_state_queries_test <grid file: 64^3 uint64 blocks of a 256^3 grid over [-0.25, 0.25]^3> <output directory>
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
static void dump_attach(const std::string &tag, const Planner::Attachments &a) {
  dump(tag + "_valid.u8", a.valid); dump(tag + "_vertices.i32", a.vertices); dump(tag + "_cost.f64", a.cost); dump(tag + "_ok.u8", a.edge_ok);
  dump(tag + "_nfk.i32", a.n_fk);
}
static void dump_solution(const std::string &tag, const Planner::SeededSolution &s) {
  dump(tag + "_status.i32", s.status); dump(tag + "_cost.f64", s.cost); dump(tag + "_src.i32", s.src_pick); dump(tag + "_dst.i32", s.dst_pick);
  std::vector<int64_t> off(1, 0);
  std::vector<int32_t> pv;
  for (const auto &p : s.paths) { pv.insert(pv.end(), p.begin(), p.end()); off.push_back((int64_t)pv.size()); }
  dump(tag + "_path_off.i64", off); dump(tag + "_path_v.i32", pv);
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
  const size_t V = 500;
  Planner prm(vc, mv, /*seed=*/11);
  prm.setMaxNearestNeighbors(6);
  prm.setRange(1e9);
  prm.createRoadmap(V, Planner::ValidateVertices | Planner::ValidateEdges);
  if (prm.milestoneCount() != V) { std::fprintf(stderr, "%zu milestones\n", prm.milestoneCount()); return 3; }
  dump("states.f64", prm.states()); dump("tips.f64", prm.tipPositions()); dump("edges.i32", prm.edges());
  dump_caches("vc", prm.vertexVoxels()); dump_caches("ec", prm.edgeVoxels());

  // states off the roadmap: midpoints of vertex pairs (some collide), the vertices themselves, and goals next to their starts
  const std::vector<double> &st = prm.states();
  const size_t n = 96;
  std::vector<double> starts, goals;
  for (size_t j = 0; j < n; j++) {
    const size_t a = (j * 29 + 5) % V, b = (j * 31 + 11) % V, c = (j * 37 + 3) % V, d = (j * 41 + 17) % V;
    for (size_t x = 0; x < 4; x++) {
      const double s = j % 4 == 3 ? st[4 * a + x] : 0.5 * (st[4 * a + x] + st[4 * b + x]);
      starts.push_back(s);
      goals.push_back(j % 3 == 1 ? s + 0.05 * (double)(x + 1) : 0.5 * (st[4 * c + x] + st[4 * d + x]));
    }
  }
  dump("starts.f64", starts); dump("goals.f64", goals);
  dump_attach("out", prm.attachStates(starts, Planner::ATTACH_OUT, 5));
  dump_attach("in", prm.attachStates(goals, Planner::ATTACH_IN, 5, 4.0));

  // seeded queries: a few vertices at made-up costs on each side, a direct cost for every third
  Planner::Seeds src, dst;
  std::vector<double> direct;
  for (size_t q = 0; q < 64; q++) {
    std::vector<int32_t> sv, dv;
    std::vector<double> sc, dc;
    for (size_t i = 0; i < q % 5; i++) { sv.push_back((int32_t)((q * 53 + i * 97 + 1) % V)); sc.push_back(0.125 * (double)((q + 3 * i) % 11)); }
    for (size_t i = 0; i < (q + 2) % 4; i++) { dv.push_back((int32_t)((q * 59 + i * 89 + 7) % V)); dc.push_back(0.25 * (double)((q + 5 * i) % 7)); }
    src.add_query(sv, sc); dst.add_query(dv, dc);
    direct.push_back(q % 3 == 0 ? 2.0 + (double)(q % 17) : std::numeric_limits<double>::infinity());
  }
  dump("src_off.i64", src.offsets); dump("src_v.i32", src.vertices); dump("src_c.f64", src.costs);
  dump("dst_off.i64", dst.offsets); dump("dst_v.i32", dst.vertices); dump("dst_c.f64", dst.costs);
  dump("direct.f64", direct);
  dump_solution("seeded", prm.solveSeeded(src, dst, direct));

  const Planner::StateSolution ss = prm.solveStates(starts, goals, 5);
  dump_solution("states", ss);
  dump("states_start_vertex.i32", ss.start_vertex); dump("states_goal_vertex.i32", ss.goal_vertex); dump("states_direct.u8", ss.direct);

  int caught = 0;
  try { prm.attachStates(starts, Planner::ATTACH_OUT, 65); } catch (const std::invalid_argument &) { caught++; }
  try { prm.attachStates({0.0, 1.0, 2.0}); } catch (const std::invalid_argument &) { caught++; }
  try { prm.solveStates(starts, {0.0, 1.0, 2.0, 3.0}); } catch (const std::invalid_argument &) { caught++; }
  {
    Planner::Seeds bad, one;
    bad.add_query({(int32_t)V}, {0.0}); one.add_query({0}, {0.0});
    try { prm.solveSeeded(bad, one); } catch (const std::out_of_range &) { caught++; }
    Planner::Seeds neg;
    neg.add_query({0}, {-1.0});
    try { prm.solveSeeded(neg, one); } catch (const std::invalid_argument &) { caught++; }
  }
  // a checker with loads: the three calls would answer with unloaded shapes
  vc.setLoads({0.0, 0.0, -0.05, 0.0, 0.0, 0.0}, std::vector<double>(6, 0.0), false);
  try { prm.attachStates(starts); } catch (const std::logic_error &) { caught++; }
  try { prm.solveSeeded(src, dst); } catch (const std::logic_error &) { caught++; }
  try { prm.solveStates(starts, goals); } catch (const std::logic_error &) { caught++; }
  vc.clearLoads();
  if (caught != 8) { std::fprintf(stderr, "%d of 8 errors\n", caught); return 3; }
  std::printf("state queries written\n");
  return 0;
}
