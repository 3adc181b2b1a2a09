"""Loaded edges of a retraction robot through the C++ shim (include/tendon_hip_shim.hpp: TendonRobot::set_loaded_retraction(on, edges),
loaded_retraction(), VoxelBackboneValidityChecker::setLoads / clearLoads, then the motion validator's checkMotion forms) compiled with
g++ against libtendon_hip.so.  CPU: it compiles with -Wall -Werror, links and prints the header's level constants.  GPU: setLoads
refuses at levels 0 and 1; at level 2 checkMotionBatch, checkMotionIndexed and checkMotion reproduce the Python engine's bits on the
config3_ret_edges edges of tests/test_gpu_loaded_ret_edges.py, cold and warm; clearLoads restores the unloaded answers."""
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
import loaded_ret_edges_common as rec                                # noqa: E402


def _build(tmp_path, irt):
    irt.build()
    exe = str(tmp_path / "shim_loaded_ret_edges_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "shim_loaded_ret_edges_test.cpp"), "-o", exe, "-L", PKG, "-ltendon_hip",
                           "-Wl,-rpath-link,/opt/rocm/lib", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_shim_loaded_ret_edges_compiles_and_links(tmp_path, irt):
    out = subprocess.check_output([_build(tmp_path, irt), "--no-gpu"], text=True)
    assert out.split() == ["levels", "0", "1", "2"]


@pytest.mark.gpu
def test_shim_loaded_ret_edges_return_pythons_bits(tmp_path, irt):
    robot, a, b, vox = rec.world(irt, "config3_ret_edges")
    n = len(a)
    dist = rec.dist_of(robot)
    N = len(robot.tendons)
    C = np.array([t.C for t in robot.tendons], dtype=np.float64)
    D = np.array([t.D for t in robot.tendons], dtype=np.float64)
    assert C.shape == D.shape
    path = str(tmp_path / "edges.bin")
    with open(path, "wb") as f:
        f.write(np.array([N, C.shape[1], n, vox.Nx()], dtype=np.int64).tobytes())
        f.write(np.array([lec.HALF, robot.specs.dL], dtype=np.float64).tobytes())
        for x in (C, D, np.ascontiguousarray(vox.blocks, dtype=np.uint64), a, b, rec.WRENCH, dist):
            f.write(np.ascontiguousarray(x).tobytes())
    out = subprocess.check_output([_build(tmp_path, irt), path], text=True).splitlines()

    def row(tag):
        (line,) = [l for l in out if l.startswith(tag + " ")]
        cells = [c.split(":") for c in line[len(tag) + 1:].split()]
        ok = np.array([c[0] == "1" for c in cells])
        nfk = np.array([int(c[1]) for c in cells], dtype=np.int32)
        t = np.array([float.fromhex(c[2]) for c in cells]) if len(cells[0]) == 3 else None
        return ok, nfk, t

    assert "level 0: runtime_error, loads 0" in out and "level 1: runtime_error, loads 0" in out and "discrete logic_error" in out
    assert [l for l in out if l.startswith("level ") and ":" not in l] == ["level 2", "level 0"]
    chk = irt.VoxelBackboneValidityChecker(robot, irt.VoxelEnvironment(), vox)
    eng = chk.engine
    eng.set_loaded_retraction(edges=True)
    un = eng.validate_edges(a, b)
    for tag in ("unloaded", "cleared"):
        ok, nfk, _ = row(tag)
        assert np.array_equal(ok, un["valid"]) and np.array_equal(nfk, un["n_fk"]), tag
    moved = 0
    for warm in (0, 1):
        kw = dict(wrench=rec.WRENCH, dist=dist, frame="world", warm_start=bool(warm))
        want = eng.validate_edges_loaded(a, b, **kw)
        ok, nfk, _ = row("batch %d" % warm)
        assert np.array_equal(ok, want["valid"]) and np.array_equal(nfk, want["n_fk"]), warm
        moved += int((nfk != un["n_fk"]).sum())
        want = eng.validate_edges_loaded(a, b, last_valid=True, **kw)
        ok, nfk, t = row("until %d" % warm)
        assert np.array_equal(ok, want["valid"]) and np.array_equal(nfk, want["n_fk"]) and np.array_equal(t, want["last_valid_t"]), warm
    assert moved > 0                                            # the loads are not a no-op on these edges
    kw = dict(wrench=rec.WRENCH, dist=dist, frame="world", warm_start=True)
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
