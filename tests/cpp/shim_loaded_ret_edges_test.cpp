// Loaded edges of a robot WITH retraction through the C++ shim (include/tendon_hip_shim.hpp): TendonRobot::set_loaded_retraction(on,
// edges) and loaded_retraction(), VoxelBackboneValidityChecker::setLoads -- refused until the robot's context is open to the loaded
// edge checks -- then VoxelBackboneMotionValidator::checkMotionBatch / checkMotionIndexed / checkMotion print their verdicts, FK
// counts and last_valid_t (hexadecimal floats), so tests/test_cpp_shim_loaded_ret_edges.py can compare them with the Python engine.
//   shim_loaded_ret_edges_test --no-gpu     compiles, links, prints the level constants
//   shim_loaded_ret_edges_test <file>       the robot (no rotation), the obstacle blocks and the edges written by the test:
//       int64 n_tendons, n_coef, n_edges, grid N; double half, dL; C [n_tendons][n_coef]; D [n_tendons][n_coef];
//       uint64 blocks [(N / 4)^3]; a [n_edges][n_tendons + 1]; b likewise; wrench [6]; dist [6]
#include <cstdio>
#include <cstring>
#include <stdexcept>

#include "tendon_hip_shim.hpp"

using namespace tendon_hip;

template <class T>
static void rd(std::FILE *f, T *p, size_t n) {
  if (std::fread(p, sizeof(T), n, f) != n) throw std::runtime_error("short input file");
}

static void print(const char *tag, const std::vector<bool> &ok, const std::vector<int32_t> &nfk, const std::vector<double> *t) {
  std::printf("%s", tag);
  for (size_t i = 0; i < ok.size(); i++) {
    std::printf(" %d:%d", ok[i] ? 1 : 0, nfk[i]);
    if (t) std::printf(":%a", (*t)[i]);
  }
  std::printf("\n");
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  if (!std::strcmp(argv[1], "--no-gpu")) {              // a checker needs a context: without a device only the header's constants
    std::printf("levels %d %d %d\n", (int)TR_LOADED_RETRACTION_OFF, (int)TR_LOADED_RETRACTION_FK, (int)TR_LOADED_RETRACTION_EDGES);
    return 0;
  }
  std::FILE *f = std::fopen(argv[1], "rb");
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
  std::vector<double> a(E * S), b(E * S), wrench(6), dist(6);
  rd(f, a.data(), a.size());
  rd(f, b.data(), b.size());
  rd(f, wrench.data(), 6);
  rd(f, dist.data(), 6);
  std::fclose(f);

  tendon::TendonRobot robot;
  robot.specs.dL = hf[1];
  robot.enable_retraction = true;
  for (size_t k = 0; k < N; k++) {
    tendon::TendonSpecs t;
    t.C.assign(C.begin() + k * nc, C.begin() + (k + 1) * nc);
    t.D.assign(D.begin() + k * nc, D.begin() + (k + 1) * nc);
    robot.tendons.push_back(t);
  }
  motion_planning::VoxelEnvironment venv;
  motion_planning::VoxelBackboneValidityChecker vc(robot, venv, vox);
  motion_planning::VoxelBackboneMotionValidator mv(vc);
  std::vector<int32_t> nfk;
  std::vector<double> t;

  print("unloaded", mv.checkMotionBatch(a, b, E, &nfk), nfk, nullptr);
  // never opened, and opened to the loaded FK only: setLoads refuses and leaves no load set behind
  for (int level = 0; level < 2; level++) {
    if (level) robot.set_loaded_retraction();
    try {
      vc.setLoads(wrench, dist);
      std::printf("level %d: no exception\n", robot.loaded_retraction());
    } catch (const std::runtime_error &) {
      std::printf("level %d: runtime_error, loads %d\n", robot.loaded_retraction(), vc.loads() ? 1 : 0);
    }
  }
  robot.set_loaded_retraction(true, true);
  std::printf("level %d\n", robot.loaded_retraction());
  for (int warm = 0; warm < 2; warm++) {
    vc.setLoads(wrench, dist, true, warm != 0);
    char tag[64];
    std::snprintf(tag, sizeof tag, "batch %d", warm);
    print(tag, mv.checkMotionBatch(a, b, E, &nfk), nfk, nullptr);
    std::snprintf(tag, sizeof tag, "until %d", warm);
    print(tag, mv.checkMotionBatch(a, b, E, &nfk, &t), nfk, &t);
  }
  // the roadmap form on the gathered pairs, and the single-edge overloads on edge 0
  std::vector<double> states(a);
  states.insert(states.end(), b.begin(), b.end());
  std::vector<int32_t> edges;
  for (size_t e = 0; e < E; e++) { edges.push_back((int32_t)e); edges.push_back((int32_t)(E + e)); }
  print("indexed", mv.checkMotionIndexed(states, 2 * E, edges, &nfk), nfk, nullptr);
  const std::vector<double> a0(a.begin(), a.begin() + S), b0(b.begin(), b.begin() + S);
  std::pair<std::vector<double>, double> lv;
  const bool ok1 = mv.checkMotion(a0, b0);
  const bool ok2 = mv.checkMotion(a0, b0, lv);
  std::printf("single %d %d %a\n", ok1 ? 1 : 0, ok2 ? 1 : 0, lv.second);
  motion_planning::VoxelBackboneDiscreteMotionValidator dv(vc);
  try {
    dv.checkMotionBatch(a, b, E);
    std::printf("no exception\n");
  } catch (const std::logic_error &) {
    std::printf("discrete logic_error\n");
  }
  vc.clearLoads();
  print("cleared", mv.checkMotionBatch(a, b, E, &nfk), nfk, nullptr);
  robot.set_loaded_retraction(false);
  std::printf("level %d\n", robot.loaded_retraction());
  return 0;
}
