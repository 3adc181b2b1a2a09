// Tip queries on loaded shapes through the C++ shim (include/tendon_hip_shim.hpp): VoxelCachedLazyPRM::roadmapIkBatchLoaded,
// solveToTipsLoaded and setTipsLoaded, TendonRobot::loaded_tips_batch, on a roadmap that createRoadmap built after setLoads.  Every
// result is written as raw arrays, so tests/test_cpp_shim_loaded_tipq.py can compare them with the Python calls byte for byte.
//   shim_loaded_tipq_test --no-gpu        compiles, links, prints the outcome codes
//   shim_loaded_tipq_test <file> <dir>    the world written by the test:
//       int64 n_tendons, n_coef, grid N, n_requests; double half, dL; C [n_tendons][n_coef]; D [n_tendons][n_coef];
//       uint64 blocks [(N / 4)^3]; wrench [6]; dist [6]; requests [n_requests][3]; int32 starts [n_requests]
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

static void dump_tips(const std::string &tag, const PRM::LoadedTipResults &r) {
  dump(tag + "_controls.f64", r.controls);
  dump(tag + "_tip.f64", r.tip_positions);
  dump(tag + "_error.f64", r.error);
  dump(tag + "_neighbor_vertex.i32", r.neighbor_vertex);
  dump(tag + "_ik_vertex.i32", r.ik_vertex);
  dump(tag + "_outcome.i32", r.outcome);
  dump(tag + "_last_valid_t.f64", r.last_valid_t);
  dump(tag + "_vu0.f64", r.vu0);
  dump(tag + "_counts.i64", std::vector<int64_t>(r.counts.begin(), r.counts.end()));
  dump(tag + "_connect_stats.i64", std::vector<int64_t>(r.connect_stats.begin(), r.connect_stats.end()));
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  if (!std::strcmp(argv[1], "--no-gpu")) {              // a checker needs a context: without a device only the header's constants
    std::printf("outcomes %d %d %d\n", (int)PRM::TIP_REACHED, (int)PRM::TIP_CLOSEST, (int)PRM::TIP_NO_NEIGHBOR);
    return 0;
  }
  if (argc < 3) return 2;
  g_dir = argv[2];
  std::FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int64_t hd[4];
  double hf[2];
  rd(f, hd, 4);
  rd(f, hf, 2);
  const size_t N = (size_t)hd[0], nc = (size_t)hd[1], G = (size_t)hd[2], nq = (size_t)hd[3];
  std::vector<double> C(N * nc), D(N * nc);
  rd(f, C.data(), C.size());
  rd(f, D.data(), D.size());
  collision::VoxelOctree vox(G);
  vox.set_xlim(-hf[0], hf[0]); vox.set_ylim(-hf[0], hf[0]); vox.set_zlim(-hf[0], hf[0]);
  rd(f, vox.blocks().data(), vox.blocks().size());
  std::vector<double> wrench(6), dist(6);
  rd(f, wrench.data(), 6);
  rd(f, dist.data(), 6);
  std::vector<std::array<double, 3>> requests(nq);
  for (auto &q : requests) rd(f, q.data(), 3);
  std::vector<int32_t> starts(nq);
  rd(f, starts.data(), nq);
  std::fclose(f);

  tendon::TendonRobot robot;
  robot.specs.dL = hf[1];
  for (size_t k = 0; k < N; k++) {
    tendon::TendonSpecs t;
    t.C.assign(C.begin() + k * nc, C.begin() + (k + 1) * nc);
    t.D.assign(D.begin() + k * nc, D.begin() + (k + 1) * nc);
    robot.tendons.push_back(t);
  }
  motion_planning::VoxelEnvironment venv;
  motion_planning::VoxelBackboneValidityChecker vc(robot, venv, vox);
  motion_planning::VoxelBackboneMotionValidator mv(vc);

  vc.setLoads(wrench, dist, /*world=*/false, /*warm_start=*/false);
  PRM prm(vc, mv, 0);
  prm.setMaxNearestNeighbors(5);
  prm.setRange(1e6);                                    // (the default range, 0.2 of the extent, leaves these few milestones almost unconnected)
  prm.createRoadmap(48, PRM::ValidateVertices | PRM::ValidateEdges);
  dump("A_states.f64", prm.states());
  dump("A_tips.f64", prm.tipPositions());
  dump("A_edges.i32", prm.edges());
  dump("A_vc_off.i64", prm.vertexVoxels().offsets);
  dump("A_vc_ids.u32", prm.vertexVoxels().block_ids);
  dump("A_vc_masks.u64", prm.vertexVoxels().masks);
  dump("A_ec_off.i64", prm.edgeVoxels().offsets);
  dump("A_ec_ids.u32", prm.edgeVoxels().block_ids);
  dump("A_ec_masks.u64", prm.edgeVoxels().masks);
  const tr_edge_loads loads = *vc.loads();

  try {
    prm.roadmapIkBatch(requests, 1e-4, 3);              // the checker-routed call keeps refusing a checker with loads
    std::printf("no exception\n");
  } catch (const std::logic_error &) {
    std::printf("roadmapIkBatch logic_error\n");
  }
  dump_tips("q0", prm.roadmapIkBatchLoaded(requests, loads, 1e-4, 3));
  dump_tips("q3", prm.roadmapIkBatchLoaded(requests, loads, 1e-4, 3, 3));
  const PRM::LoadedTipSolution s = prm.solveToTipsLoaded(starts, requests, loads, 1e-4, 3, 3);
  dump_tips("s3", s.ik);
  dump("s3_status.i32", s.roadmap.status);
  dump("s3_cost.f64", s.roadmap.cost);
  std::vector<int32_t> pv;
  std::vector<int64_t> off{0};
  for (const auto &p : s.roadmap.paths) { pv.insert(pv.end(), p.begin(), p.end()); off.push_back((int64_t)pv.size()); }
  dump("s3_path_vertices.i32", pv);
  dump("s3_path_offsets.i64", off);
  const tendon::TendonRobot::LoadedTips lt = robot.loaded_tips_batch(prm.states(), prm.milestoneCount(), loads);
  dump("L_tips.f64", lt.tips);
  dump("L_vu0.f64", lt.vu0);
  dump("L_conv.u8", lt.converged);
  prm.setTipsLoaded(loads);                             // the same tips, made by the roadmap itself
  dump_tips("t0", prm.roadmapIkBatchLoaded(requests, loads, 1e-4, 3));
  std::printf("stages written\n");
  return 0;
}
