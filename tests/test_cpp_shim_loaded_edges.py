"""Loaded edges through the C++ shim (include/tendon_hip_shim.hpp: VoxelBackboneValidityChecker::setLoads / clearLoads, then the motion
validator's checkMotion forms) compiled with g++ against libtendon_hip.so.  CPU: it compiles with -Wall -Werror and links.  GPU:
setLoads followed by checkMotionBatch, checkMotionIndexed or checkMotion reproduces the Python engine's bits on the config3_rot edges
of tests/test_gpu_loaded_edges.py, both frames, cold and warm; clearLoads restores the unloaded answers."""
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


def _build(tmp_path, irt):
    irt.build()
    exe = str(tmp_path / "shim_loaded_edges_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "shim_loaded_edges_test.cpp"), "-o", exe, "-L", PKG, "-ltendon_hip",
                           "-Wl,-rpath-link,/opt/rocm/lib", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_shim_loaded_edges_compiles_and_links(tmp_path, irt):
    out = subprocess.check_output([_build(tmp_path, irt), "--no-gpu"], text=True)
    assert out.split() == ["frames", str(irt._lib.TR_LOAD_FRAME_BASE), str(irt._lib.TR_LOAD_FRAME_WORLD)]


@pytest.mark.gpu
def test_shim_loaded_edges_return_pythons_bits(tmp_path, irt):
    import make_fk_truth as mft
    robot = mft.fixture_robot(irt, "config3_rot")[0]
    n, eseed, cap, gseed, count, radius = lec.FIXTURES["config3_rot"]
    a, b = lec.make_edges(robot, n, eseed, cap)
    vox = lec.make_grid(irt, robot.specs.dL, gseed, count, radius)
    N = len(robot.tendons)
    C = np.array([t.C for t in robot.tendons], dtype=np.float64)
    D = np.array([t.D for t in robot.tendons], dtype=np.float64)
    assert C.shape == D.shape
    path = str(tmp_path / "edges.bin")
    with open(path, "wb") as f:
        f.write(np.array([N, C.shape[1], n, vox.Nx()], dtype=np.int64).tobytes())
        f.write(np.array([lec.HALF, robot.specs.dL], dtype=np.float64).tobytes())
        for x in (C, D, np.ascontiguousarray(vox.blocks, dtype=np.uint64), a, b, lec.WRENCH, lec.DIST):
            f.write(np.ascontiguousarray(x).tobytes())
    out = subprocess.check_output([_build(tmp_path, irt), path], text=True).splitlines()

    def row(tag):
        (line,) = [l for l in out if l.startswith(tag + " ")]
        cells = [c.split(":") for c in line[len(tag) + 1:].split()]
        ok = np.array([c[0] == "1" for c in cells])
        nfk = np.array([int(c[1]) for c in cells], dtype=np.int32)
        t = np.array([float.fromhex(c[2]) for c in cells]) if len(cells[0]) == 3 else None
        return ok, nfk, t

    chk = irt.VoxelBackboneValidityChecker(robot, irt.VoxelEnvironment(), vox)
    eng = chk.engine
    un = eng.validate_edges(a, b)
    for tag in ("unloaded", "cleared"):
        ok, nfk, _ = row(tag)
        assert np.array_equal(ok, un["valid"]) and np.array_equal(nfk, un["n_fk"]), tag
    assert "caught invalid_argument" in out and "discrete logic_error" in out
    moved = 0
    for world in (0, 1):
        for warm in (0, 1):
            kw = dict(wrench=lec.WRENCH, dist=lec.DIST, frame="world" if world else "base", warm_start=bool(warm))
            want = eng.validate_edges_loaded(a, b, **kw)
            ok, nfk, _ = row("batch %d %d" % (world, warm))
            assert np.array_equal(ok, want["valid"]) and np.array_equal(nfk, want["n_fk"]), (world, warm)
            moved += int((ok != un["valid"]).sum())
            want = eng.validate_edges_loaded(a, b, last_valid=True, **kw)
            ok, nfk, t = row("until %d %d" % (world, warm))
            assert np.array_equal(ok, want["valid"]) and np.array_equal(nfk, want["n_fk"]) and np.array_equal(t, want["last_valid_t"]), (world, warm)
    assert moved > 0                                            # the loads are not a no-op on these edges
    kw = dict(wrench=lec.WRENCH, dist=lec.DIST, frame="world", warm_start=True)
    states = np.vstack([a, b])
    edges = np.stack([np.arange(n), n + np.arange(n)], 1).astype(np.int32)
    want = eng.validate_edges_loaded_indexed(states, edges, **kw)
    ok, nfk, _ = row("indexed")
    assert np.array_equal(ok, want["valid"]) and np.array_equal(nfk, want["n_fk"])
    (single,) = [l.split() for l in out if l.startswith("single ")]
    one = eng.validate_edges_loaded(a[:1], b[:1], **kw)
    one_u = eng.validate_edges_loaded(a[:1], b[:1], last_valid=True, **kw)
    assert int(single[1]) == int(one["valid"][0]) and int(single[2]) == int(one_u["valid"][0])
    assert float.fromhex(single[3]) == one_u["last_valid_t"][0]
