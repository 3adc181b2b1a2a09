"""The accurate connection rule of the C++ shim (include/tendon_hip_shim.hpp: VoxelCachedLazyPRM::nearestStates /
roadmapIkBatchAccurate / solveToTipsAccurate) compiled with g++ against libtendon_hip.so.  CPU: tests/cpp/shim_tip_connect_test.cpp
compiles with -Wall -Werror and links.  GPU: on the roadmap it builds, the shim returns what the Python API returns, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "interactive-rate-tendons_amd")


def _build(tmp_path, irt):
    irt.build()
    exe = str(tmp_path / "shim_tip_connect_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "shim_tip_connect_test.cpp"), "-o", exe, "-L", PKG, "-ltendon_hip",
                           "-Wl,-rpath-link,/opt/rocm/lib", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_shim_tip_connect_compiles(tmp_path, irt):
    assert os.path.exists(_build(tmp_path, irt))


@pytest.mark.gpu
def test_shim_tip_connect_returns_what_python_returns(tmp_path, irt):
    exe = _build(tmp_path, irt)
    W = irt.workloads
    robot = W.robot_config3()
    vox, _ = W.reach_environment(seed=7, n_spheres=64)
    grid_file, out = tmp_path / "grid.u64", tmp_path / "out"
    np.ascontiguousarray(vox.blocks, dtype=np.uint64).tofile(grid_file)
    out.mkdir()
    assert "tip connect queries written" in subprocess.check_output([exe, str(grid_file), str(out)], text=True)
    ld = lambda name, dt: np.fromfile(out / name, dtype=dt)
    caches = lambda t: dict(offsets=ld(t + "_off.i64", np.int64), block_ids=ld(t + "_ids.u32", np.uint32), masks=ld(t + "_masks.u64", np.uint64),
                            present=ld(t + "_usable.u8", np.uint8).astype(bool))
    states, tips, edges = ld("states.f64", np.float64).reshape(-1, 4), ld("tips.f64", np.float64).reshape(-1, 3), ld("edges.i32", np.int32).reshape(-1, 2)
    requests, starts = ld("requests.f64", np.float64).reshape(-1, 3), ld("starts.i32", np.int32)
    chk = irt.VoxelBackboneValidityChecker(robot, irt.VoxelEnvironment(), vox)
    mv = irt.VoxelBackboneMotionValidator(chk)
    prm = irt.VoxelCachedLazyPRM(chk, states, edges)
    prm.set_caches(caches("vc"), caches("ec"))
    prm.set_tips(tips)
    prm.set_validity(np.ones(len(states), np.uint8), np.ones(len(edges), np.uint8))     # createRoadmap validated both
    names = (("controls", "controls.f64", np.float64), ("tip", "tips.f64", np.float64), ("error", "error.f64", np.float64),
             ("neighbor_vertex", "vertex.i32", np.int32), ("ik_vertex", "ikvertex.i32", np.int32), ("outcome", "outcome.i32", np.int32), ("last_valid_t", "t.f64", np.float64))

    def same(tag, res):
        for key, name, dt in names:
            got = ld(tag + "_" + name, dt)
            assert np.array_equal(got.view(np.uint8), np.ascontiguousarray(res[key]).reshape(-1).view(np.uint8)), (tag, key)

    def same_stats(tag, res):
        st = res["connect_stats"]
        assert ld(tag + "_stats.i64", np.int64).tolist() == [st["pairs_checked"], st["reached"], st["moved"], st["gained"]]

    queries = ld("queries.f64", np.float64).reshape(-1, 4)
    idx, dist = prm.nearest_states(queries, 7)
    assert np.array_equal(ld("near_vertices.i32", np.int32).reshape(-1, 7), idx)
    assert np.array_equal(ld("near_distance.f64", np.float64).view(np.uint64).reshape(-1, 7), dist.view(np.uint64))
    assert (dist[3::4, 0] == 0.0).all() and (dist[0::4, 0] > 0.0).all()
    idx_b, dist_b = prm.nearest_states(queries, 7, max_distance=dist[0, 3])
    assert np.array_equal(ld("nearb_vertices.i32", np.int32).reshape(-1, 7), idx_b) and (idx_b == -1).any() and idx_b[0, 3] >= 0
    assert np.array_equal(ld("nearb_distance.f64", np.float64).view(np.uint64).reshape(-1, 7), dist_b.view(np.uint64))
    ik = prm.roadmap_ik_batch(requests, tolerance=1e-4, k=5, motion_validator=mv, connect_k=6)
    same("ik", ik)
    same_stats("ik", ik)
    print("outcomes", np.bincount(ik["outcome"], minlength=3), ik["connect_stats"])
    assert (ik["outcome"] != 2).all() and (ik["outcome"] == 0).any() and ik["connect_stats"]["moved"] > 0
    sol = prm.solve_to_tips(starts, requests, tolerance=1e-4, k=5, motion_validator=mv, connect_k=6)
    same("sol", sol)
    same_stats("sol", sol)
    assert np.array_equal(ld("sol_status.i32", np.int32), sol["status"])
    assert np.array_equal(ld("sol_cost.f64", np.float64).view(np.uint64), sol["cost"].view(np.uint64))
    assert np.array_equal(ld("sol_path_off.i64", np.int64), sol["path_offsets"]) and np.array_equal(ld("sol_path_v.i32", np.int32), sol["path_vertices"])
    assert (sol["status"] == 0).any()
