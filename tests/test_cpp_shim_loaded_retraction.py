"""The loaded FK of a retraction robot through the C++ shim (include/tendon_hip_shim.hpp: general_shape, generalShapeBatch,
loaded_tips_batch) compiled with g++ against libtendon_hip.so.  CPU: it compiles with -Wall -Werror, links, and a wrong state size is
std::invalid_argument.  GPU: a context that was never opened (set_loaded_retraction) refuses; opened, every result has the state's own point count and Python's bits."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "interactive-rate-tendons_amd")


def _build(tmp_path, irt):
    irt.build()
    exe = str(tmp_path / "shim_loaded_retraction_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "shim_loaded_retraction_test.cpp"), "-o", exe, "-L", PKG, "-ltendon_hip",
                           "-Wl,-rpath-link,/opt/rocm/lib", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_shim_compiles_and_rejects_wrong_state_size(tmp_path, irt):
    out = subprocess.check_output([_build(tmp_path, irt), "--no-gpu"], text=True)
    assert "caught invalid_argument" in out


@pytest.mark.gpu
def test_shim_returns_pythons_bits(tmp_path, irt):
    out = subprocess.check_output([_build(tmp_path, irt)], text=True).splitlines()
    rows = lambda tag: [np.array([float.fromhex(x) if "x" in x or "n" in x else float(x) for x in l.split()[1:]]) for l in out if l.startswith(tag + " ")]
    robot = irt.workloads.robot_config1()
    robot.enable_rotation = robot.enable_retraction = True
    robot.engine(0).set_loaded_retraction()
    assert "closed: runtime_error" in out
    L = robot.specs.L
    f_e, l_e, F_e, L_e = (0.0, -2.4525, 0.0), (0.0, 0.0, 0.0), (0.05, -0.03, 0.02), (1e-3, -2e-3, 5e-4)
    states = np.array([[3.0, 7.0, 1.0, 0.4, 0.0731], [0.0, 0.0, 0.0, -1.0, 0.0], [12.0, 0.5, 5.0, 2.0, 0.1972], [1.0, 2.0, 3.0, 0.0, 0.25]])
    py = robot.general_shape_batch(states, f_e=f_e, l_e=l_e, F_e=F_e, L_e=L_e)
    assert py["n_points"][1] == robot.engine(0).num_points and py["n_points"][2] == 2 and py["n_points"][3] == 1

    def want(i):
        k = int(py["n_points"][i])
        return np.concatenate([[float(py["converged"][i]), k, k, k, min(states[i, -1], L), L], py["vu0"][i], [py["L"][i]], py["L_i"][i],
                               py["p"][i, :k].reshape(-1)])
    got = rows("batch")
    assert len(got) == 4
    for i in range(4):
        assert np.array_equal(got[i], want(i)), i
    assert np.array_equal(rows("single")[0], want(0))
    tips = rows("tip")
    pt = robot.engine(0).fk_loaded_tips(states, wrench=np.r_[F_e, L_e], dist=np.r_[f_e, l_e])
    for i in range(4):
        assert np.array_equal(tips[i], np.r_[float(pt["converged"][i]), pt["tips"][i]]), i
