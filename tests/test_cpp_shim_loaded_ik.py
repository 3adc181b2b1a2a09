"""The loaded-IK side of the C++ shim (include/tendon_hip_shim.hpp: inverseKinematicsLoaded, inverseKinematicsLoadedBatch) compiled
with g++ against libtendon_hip.so.  CPU: it compiles with -Wall -Werror, links, and wrong sizes are std::invalid_argument.  GPU: on
config1 under gravity (case B of tests/golden/loaded_fk_config1.npz) it returns what the Python interface returns, bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "interactive-rate-tendons_amd")
for _p in (HERE, os.path.join(HERE, "golden")):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def _build(tmp_path, irt):
    irt.build()
    exe = str(tmp_path / "shim_loaded_ik_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "shim_loaded_ik_test.cpp"), "-o", exe, "-L", PKG, "-ltendon_hip",
                           "-Wl,-rpath-link,/opt/rocm/lib", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_shim_loaded_ik_compiles_and_rejects_wrong_sizes(tmp_path, irt):
    out = subprocess.check_output([_build(tmp_path, irt), "--no-gpu"], text=True)
    assert "caught invalid_argument\n" in out and "caught invalid_argument (loads)" in out


@pytest.mark.gpu
def test_shim_loaded_ik_returns_pythons_bits(tmp_path, irt, orc):
    import loaded_ik_reference as ikr
    import make_loaded_fk as gen
    robot, rob, st = gen.fixture("config1")
    fx = dict(np.load(gen.path("config1")))
    starts = ikr.offset_starts(rob, st, 3.0)
    goals, dist = np.ascontiguousarray(fx["p_B"][:, -1]), fx["dist_B"][0]
    n = len(starts)
    data = tmp_path / "problems.txt"
    data.write_text("%d\n%s\n" % (n, " ".join(float(x).hex() for a in (starts, goals, dist) for x in a.reshape(-1))))
    out = subprocess.check_output([_build(tmp_path, irt), str(data)], text=True).splitlines()
    rows = lambda tag: [l.split()[1:] for l in out if l.startswith(tag + " ")]
    py = robot.engine(0).ik_loaded_batch(starts, goals, dist=dist)

    def same(row, r, i):
        assert [int(x) for x in row[:3]] == [int(r["equilibrium"][i]), int(r["iters"][i]), int(r["num_fk_calls"][i])]
        got = np.array([float.fromhex(x) for x in row[3:]])
        assert np.array_equal(got, np.concatenate([[r["error"][i]], r["state"][i], r["tip"][i], r["vu0"][i]]))
    batch = rows("batch")
    assert len(batch) == n
    for i in range(n):
        same(batch[i], py, i)
    assert [int(x) for x in rows("rounds")[0]] == [py["rounds"], py["shoot_rounds"]]
    same(rows("single")[0], py, 0)
    same(rows("one_iter")[0], robot.engine(0).ik_loaded_batch(starts[:1], goals[:1], dist=dist, max_iters=1), 0)
    assert (py["error"] <= 1e-4).all()
    assert "retraction runtime_error" in out
