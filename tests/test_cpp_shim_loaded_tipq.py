"""Tip queries on loaded shapes through the C++ shim (include/tendon_hip_shim.hpp: roadmapIkBatchLoaded, solveToTipsLoaded,
setTipsLoaded, TendonRobot::loaded_tips_batch) compiled with g++ against libtendon_hip.so.  CPU: it compiles with -Wall -Werror and
links.  GPU: on the config1 world of tests/loaded_edges_common.py the shim's calls give the Python calls' bytes on the roadmap the shim
built under setLoads, and roadmapIkBatch on a checker with loads still throws."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "interactive-rate-tendons_amd")
HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.join(HERE, "golden")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import loaded_edges_common as lec                                    # noqa: E402

FIELDS = (("controls", np.float64), ("tip", np.float64), ("error", np.float64), ("neighbor_vertex", np.int32), ("ik_vertex", np.int32),
          ("outcome", np.int32), ("last_valid_t", np.float64), ("vu0", np.float64), ("counts", np.int64))


def _build(tmp_path, irt):
    irt.build()
    exe = str(tmp_path / "shim_loaded_tipq_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "shim_loaded_tipq_test.cpp"), "-o", exe, "-L", PKG, "-ltendon_hip",
                           "-Wl,-rpath-link,/opt/rocm/lib", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_shim_loaded_tipq_compiles_and_links(tmp_path, irt):
    out = subprocess.check_output([_build(tmp_path, irt), "--no-gpu"], text=True)
    assert out.split() == ["outcomes", "0", "1", "2"]


@pytest.mark.gpu
def test_shim_loaded_tip_queries_equal_the_python_calls(tmp_path, irt):
    import make_fk_truth as mft
    robot = mft.fixture_robot(irt, "config1")[0]
    _, _, _, gseed, count, radius = lec.FIXTURES["config1"]
    vox = lec.make_grid(irt, robot.specs.dL, gseed, count, radius)
    N = len(robot.tendons)
    C = np.array([t.C for t in robot.tendons], dtype=np.float64)
    D = np.array([t.D for t in robot.tendons], dtype=np.float64)
    assert C.shape == D.shape
    chk = irt.VoxelBackboneValidityChecker(robot, irt.VoxelEnvironment(), vox)
    eng = chk.engine
    loads = dict(wrench=lec.WRENCH, dist=lec.DIST, frame="base")
    sv = eng.sample_valid_vertices_loaded(48, seed=0, warm_start=False, **loads)
    rng = np.random.default_rng(7)
    nq = 12
    requests = sv["tips"][rng.integers(0, 48, nq)] + rng.normal(size=(nq, 3)) * 0.003
    requests[nq // 2:] = rng.uniform(-0.12, 0.12, (nq - nq // 2, 3)) + np.array([0.0, 0.0, 0.1])
    requests = np.ascontiguousarray(requests)
    starts = rng.integers(0, 48, nq).astype(np.int32)
    path, out = str(tmp_path / "world.bin"), tmp_path / "out"
    out.mkdir()
    with open(path, "wb") as f:
        f.write(np.array([N, C.shape[1], vox.Nx(), nq], dtype=np.int64).tobytes())
        f.write(np.array([lec.HALF, robot.specs.dL], dtype=np.float64).tobytes())
        for x in (C, D, np.ascontiguousarray(vox.blocks, dtype=np.uint64), lec.WRENCH, lec.DIST, requests, starts):
            f.write(np.ascontiguousarray(x).tobytes())
    text = subprocess.check_output([_build(tmp_path, irt), path, str(out)], text=True)
    assert "stages written" in text and "roadmapIkBatch logic_error" in text and "no exception" not in text
    ld = lambda name, dt: np.fromfile(out / name, dtype=dt)
    cache = lambda t: dict(offsets=ld("A_%s_off.i64" % t, np.int64), block_ids=ld("A_%s_ids.u32" % t, np.uint32),
                           masks=ld("A_%s_masks.u64" % t, np.uint64))
    states, tips = ld("A_states.f64", np.float64).reshape(-1, N), ld("A_tips.f64", np.float64).reshape(-1, 3)
    assert np.array_equal(states, sv["states"]) and np.array_equal(tips, sv["tips"])
    # the same roadmap on the Python side
    prm = irt.VoxelCachedLazyPRM(chk, states, ld("A_edges.i32", np.int32).reshape(-1, 2))
    prm.set_caches(cache("vc"), cache("ec"))
    prm.set_tips(tips)
    mv = irt.VoxelBackboneMotionValidator(chk)

    def same(tag, want):
        for key, dt in FIELDS:
            got = ld("%s_%s" % (tag, key) + {np.float64: ".f64", np.int32: ".i32", np.int64: ".i64"}[dt], dt)
            w = want[key] if key in want else want["neighbor_vertex"]          # (connect_k = 0: ik_vertex is the connection vertex)
            assert np.array_equal(got.view(np.uint8), np.ascontiguousarray(w).reshape(-1).view(np.uint8)), (tag, key)

    kw = dict(tolerance=1e-4, k=3, motion_validator=mv, **loads)
    r0 = prm.roadmap_ik_loaded_batch(requests, **kw)
    same("q0", r0)
    same("t0", r0)                                                      # after setTipsLoaded: the same tips, the same answers
    r3 = prm.roadmap_ik_loaded_batch(requests, connect_k=3, **kw)
    same("q3", r3)
    cs = ld("q3_connect_stats.i64", np.int64)
    assert list(cs) == [r3["connect_stats"][k] for k in ("pairs_checked", "reached", "moved", "gained")]
    assert (r0["outcome"] == 0).sum() >= 3 and (r0["outcome"] == 1).sum() >= 2
    s3 = prm.solve_to_tips_loaded(starts, requests, connect_k=3, **kw)
    same("s3", s3)
    assert np.array_equal(ld("s3_status.i32", np.int32), s3["status"]) and np.array_equal(ld("s3_cost.f64", np.float64), s3["cost"])
    assert np.array_equal(ld("s3_path_vertices.i32", np.int32), s3["path_vertices"])
    assert np.array_equal(ld("s3_path_offsets.i64", np.int64), s3["path_offsets"])
    lt = eng.fk_loaded_tips(states, **loads)
    assert np.array_equal(ld("L_tips.f64", np.float64).reshape(-1, 3), lt["tips"]) and np.array_equal(lt["tips"], tips)
    assert np.array_equal(ld("L_vu0.f64", np.float64).reshape(-1, 6), lt["vu0"]) and ld("L_conv.u8", np.uint8).all()
