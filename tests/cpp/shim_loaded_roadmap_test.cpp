// The roadmap build under loads through the C++ shim (include/tendon_hip_shim.hpp): after VoxelBackboneValidityChecker::setLoads,
// VoxelCachedLazyPRM::createRoadmap (first call and growth), precomputeVertexValidity / precomputeEdgeValidity and
// precomputeVertexVoxelCache / precomputeEdgeVoxelCache take every shape from the loaded FK.  Every stage is written as raw arrays, so
// tests/test_cpp_shim_loaded_roadmap.py can compare them with the Python engine's loaded calls bit for bit.
//   shim_loaded_roadmap_test --no-gpu        compiles, links, prints the option flags
//   shim_loaded_roadmap_test <file> <dir>    the robot and the obstacle blocks written by the test:
//       int64 n_tendons, n_coef, grid N; double half, dL; C [n_tendons][n_coef]; D [n_tendons][n_coef];
//       uint64 blocks [(N / 4)^3]; wrench [6]; dist [6]
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>

#include "tendon_hip_shim.hpp"

using namespace tendon_hip;
using PRM = motion_planning::VoxelCachedLazyPRM;

template <class T>
static void rd(std::FILE *f, T *p, size_t n) {
  if (std::fread(p, sizeof(T), n, f) != n) throw std::runtime_error("short input file");
}

static std::string g_dir;

template <class T>
static void dump(const std::string &name, const std::vector<T> &v) {
  std::FILE *f = std::fopen((g_dir + "/" + name).c_str(), "wb");
  if (!f) throw std::runtime_error("cannot write " + name);
  if (!v.empty() && std::fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) throw std::runtime_error("short write");
  std::fclose(f);
}
static std::vector<uint8_t> bytes(const std::vector<bool> &b) { return std::vector<uint8_t>(b.begin(), b.end()); }

static void dump_graph(const std::string &tag, PRM &prm) {
  dump(tag + "_states.f64", prm.states());
  dump(tag + "_tips.f64", prm.tipPositions());
  dump(tag + "_edges.i32", prm.edges());
  dump(tag + "_vc_off.i64", prm.vertexVoxels().offsets);
  dump(tag + "_vc_ids.u32", prm.vertexVoxels().block_ids);
  dump(tag + "_vc_masks.u64", prm.vertexVoxels().masks);
  dump(tag + "_ec_off.i64", prm.edgeVoxels().offsets);
  dump(tag + "_ec_ids.u32", prm.edgeVoxels().block_ids);
  dump(tag + "_ec_masks.u64", prm.edgeVoxels().masks);
}
static void dump_report(const std::string &tag, const PRM &prm) {
  const PRM::BuildReport &r = prm.lastBuild();
  dump(tag + "_cand.i32", r.candidate_edges);
  dump(tag + "_acc.u8", bytes(r.accepted));
  dump(tag + "_nfk.i32", r.n_fk);
  dump(tag + "_cidx.i64", r.candidate_index);
  dump(tag + "_meta.i64", std::vector<int64_t>{r.candidates_tried, (int64_t)r.k, r.n_unconverged, r.n_integrations});
  dump(tag + "_maxd.f64", std::vector<double>{r.max_distance});
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  if (!std::strcmp(argv[1], "--no-gpu")) {              // a checker needs a context: without a device only the header's constants
    std::printf("options %d %d %d %d\n", (int)PRM::VoxelizeVertices, (int)PRM::ValidateVertices, (int)PRM::VoxelizeEdges, (int)PRM::ValidateEdges);
    return 0;
  }
  if (argc < 3) return 2;
  g_dir = argv[2];
  std::FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int64_t hd[3];
  double hf[2];
  rd(f, hd, 3);
  rd(f, hf, 2);
  const size_t N = (size_t)hd[0], nc = (size_t)hd[1], G = (size_t)hd[2];
  std::vector<double> C(N * nc), D(N * nc);
  rd(f, C.data(), C.size());
  rd(f, D.data(), D.size());
  collision::VoxelOctree vox(G);
  vox.set_xlim(-hf[0], hf[0]); vox.set_ylim(-hf[0], hf[0]); vox.set_zlim(-hf[0], hf[0]);
  rd(f, vox.blocks().data(), vox.blocks().size());
  std::vector<double> wrench(6), dist(6);
  rd(f, wrench.data(), 6);
  rd(f, dist.data(), 6);
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
  const int both = PRM::ValidateVertices | PRM::ValidateEdges;

  vc.setLoads(wrench, dist, /*world=*/true, /*warm_start=*/true);
  {
    // A: createRoadmap(48) with validated vertices and edges; B: its growth to 64 with shape checks only
    PRM prm(vc, mv, 0);
    prm.setMaxNearestNeighbors(5);
    prm.setRange(1e6);                                  // (the default range, 0.2 of the extent, leaves these few milestones almost unconnected)
    prm.createRoadmap(48, both);
    dump_graph("A", prm);
    dump_report("A", prm);
    prm.createRoadmap(64, PRM::VoxelizeVertices | PRM::VoxelizeEdges);
    dump_graph("B", prm);
    dump_report("B", prm);
    try {
      prm.roadmapIkBatch({{0.0, 0.0, 0.1}});
      std::printf("no exception\n");
    } catch (const std::logic_error &) {
      std::printf("roadmapIkBatch logic_error\n");
    }
    try {
      prm.solveToTips({0}, {{0.0, 0.0, 0.1}});
      std::printf("no exception\n");
    } catch (const std::logic_error &) {
      std::printf("solveToTips logic_error\n");
    }
  }
  {
    // C: a lazy roadmap (raw candidates, every k-nearest edge), then precomputeValidity
    PRM prm(vc, mv, 0);
    prm.setMaxNearestNeighbors(5);
    prm.setRange(1e6);                                  // (the default range, 0.2 of the extent, leaves these few milestones almost unconnected)
    prm.createRoadmap(48, PRM::LazyRoadmap);
    dump_graph("C0", prm);
    prm.precomputeVertexValidity();
    prm.precomputeEdgeValidity();
    dump_graph("C", prm);
  }
  {
    // D: the same lazy roadmap, then precomputeVoxelCache
    PRM prm(vc, mv, 0);
    prm.setMaxNearestNeighbors(5);
    prm.setRange(1e6);                                  // (the default range, 0.2 of the extent, leaves these few milestones almost unconnected)
    prm.createRoadmap(48, PRM::LazyRoadmap);
    prm.precomputeVertexVoxelCache();
    prm.precomputeEdgeVoxelCache();
    dump_graph("D", prm);
  }
  vc.clearLoads();
  {
    PRM prm(vc, mv, 0);
    prm.setMaxNearestNeighbors(5);
    prm.setRange(1e6);                                  // (the default range, 0.2 of the extent, leaves these few milestones almost unconnected)
    prm.createRoadmap(48, both);
    dump_graph("U", prm);
    dump_report("U", prm);
  }
  std::printf("stages written\n");
  return 0;
}
