"""Queries between arbitrary states through the C++ shim (include/tendon_hip_shim.hpp: VoxelCachedLazyPRM::attachStates / solveSeeded /
solveStates) compiled with g++ against libtendon_hip.so.  CPU: tests/cpp/shim_state_queries_test.cpp compiles with -Wall -Werror and
links.  GPU: on the roadmap it builds, the shim returns what the Python API returns, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "interactive-rate-tendons_amd")


def _build(tmp_path, irt):
    irt.build()
    exe = str(tmp_path / "shim_state_queries_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "shim_state_queries_test.cpp"), "-o", exe, "-L", PKG, "-ltendon_hip",
                           "-Wl,-rpath-link,/opt/rocm/lib", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_shim_state_queries_compiles(tmp_path, irt):
    assert os.path.exists(_build(tmp_path, irt))


@pytest.mark.gpu
def test_shim_state_queries_return_what_python_returns(tmp_path, irt):
    exe = _build(tmp_path, irt)
    W = irt.workloads
    robot = W.robot_config3()
    vox, _ = W.reach_environment(seed=7, n_spheres=64)
    grid_file, out = tmp_path / "grid.u64", tmp_path / "out"
    np.ascontiguousarray(vox.blocks, dtype=np.uint64).tofile(grid_file)
    out.mkdir()
    assert "state queries written" in subprocess.check_output([exe, str(grid_file), str(out)], text=True)
    ld = lambda name, dt: np.fromfile(out / name, dtype=dt)
    caches = lambda t: dict(offsets=ld(t + "_off.i64", np.int64), block_ids=ld(t + "_ids.u32", np.uint32), masks=ld(t + "_masks.u64", np.uint64),
                            present=ld(t + "_usable.u8", np.uint8).astype(bool))
    states, tips, edges = ld("states.f64", np.float64).reshape(-1, 4), ld("tips.f64", np.float64).reshape(-1, 3), ld("edges.i32", np.int32).reshape(-1, 2)
    chk = irt.VoxelBackboneValidityChecker(robot, irt.VoxelEnvironment(), vox)
    mv = irt.VoxelBackboneMotionValidator(chk)
    prm = irt.VoxelCachedLazyPRM(chk, states, edges)
    prm.set_caches(caches("vc"), caches("ec"))
    prm.set_tips(tips)
    prm.set_validity(np.ones(len(states), np.uint8), np.ones(len(edges), np.uint8))     # createRoadmap validated both
    starts, goals = ld("starts.f64", np.float64).reshape(-1, 4), ld("goals.f64", np.float64).reshape(-1, 4)

    def bits(x):
        return np.ascontiguousarray(x).reshape(-1).view(np.uint8)

    def same_attach(tag, res):
        for key, name, dt in (("valid", "valid.u8", np.uint8), ("vertices", "vertices.i32", np.int32), ("cost", "cost.f64", np.float64),
                              ("edge_ok", "ok.u8", np.uint8), ("n_fk", "nfk.i32", np.int32)):
            want = res[key].astype(np.uint8) if res[key].dtype == bool else res[key]
            assert np.array_equal(bits(ld(tag + "_" + name, dt)), bits(want)), (tag, key)

    def same_solution(tag, res):
        for key, name, dt in (("status", "status.i32", np.int32), ("cost", "cost.f64", np.float64), ("src_pick", "src.i32", np.int32),
                              ("dst_pick", "dst.i32", np.int32), ("path_offsets", "path_off.i64", np.int64), ("path_vertices", "path_v.i32", np.int32)):
            assert np.array_equal(bits(ld(tag + "_" + name, dt)), bits(res[key])), (tag, key)

    a_out = prm.attach_states(starts, "out", k=5, motion_validator=mv)
    a_in = prm.attach_states(goals, "in", k=5, max_distance=4.0, motion_validator=mv)
    same_attach("out", a_out)
    same_attach("in", a_in)
    assert a_out["valid"].any() and not a_out["valid"].all() and a_out["edge_ok"].any() and (a_in["vertices"] == -1).any()
    src = (ld("src_off.i64", np.int64), ld("src_v.i32", np.int32), ld("src_c.f64", np.float64))
    dst = (ld("dst_off.i64", np.int64), ld("dst_v.i32", np.int32), ld("dst_c.f64", np.float64))
    seeded = prm.solve_seeded(src, dst, ld("direct.f64", np.float64))
    same_solution("seeded", seeded)
    assert seeded["direct"].any() and ((seeded["status"] == 0) & ~seeded["direct"]).any() and (seeded["status"] == 1).any()
    sol = prm.solve_states(starts, goals, k=5, motion_validator=mv)
    same_solution("states", sol)
    assert np.array_equal(ld("states_start_vertex.i32", np.int32), sol["start_vertex"])
    assert np.array_equal(ld("states_goal_vertex.i32", np.int32), sol["goal_vertex"])
    assert np.array_equal(ld("states_direct.u8", np.uint8).astype(bool), sol["direct"])
    print("statuses", np.bincount(sol["status"], minlength=4), "direct", int(sol["direct"].sum()))
    assert (sol["status"] == 0).any() and sol["direct"].any()
