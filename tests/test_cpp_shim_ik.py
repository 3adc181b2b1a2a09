"""The tip-IK side of the C++ shim (include/tendon_hip_shim.hpp: tip_control::inverse_kinematics, TendonRobot::tip_jacobian_batch,
VoxelCachedLazyPRM::roadmapIk) compiled with g++ against libtendon_hip.so.  CPU: it compiles with -Wall -Werror, links, and a wrong
state size is std::invalid_argument.  GPU: its answers hold up against the oracle."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "interactive-rate-tendons_amd")


def _build(tmp_path, irt):
    irt.build()
    exe = str(tmp_path / "shim_ik_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "shim_ik_test.cpp"), "-o", exe, "-L", PKG, "-ltendon_hip",
                           "-Wl,-rpath-link,/opt/rocm/lib", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_shim_ik_compiles_and_rejects_wrong_state_size(tmp_path, irt):
    out = subprocess.check_output([_build(tmp_path, irt), "--no-gpu"], text=True)
    assert "caught 2 bounds 4 0 20" in out


def _rows(out, tag):
    rows = []
    for line in out:
        if line.startswith(tag + " "):
            rows.append([np.array(part.split(), float) for part in line[len(tag):].split("|")])
    return rows


@pytest.mark.gpu
def test_shim_ik_matches_oracle(tmp_path, irt, orc, helpers):
    out = subprocess.check_output([_build(tmp_path, irt)], text=True).splitlines()
    robot = irt.workloads.robot_config3()
    orb = helpers.oracle_robot(orc, robot)
    tip = lambda s: orb.shape(s)["p"][-1]
    ik = _rows(out, "ik")
    assert len(ik) == 4
    reached = 0
    for goal_state, state, rest in ik:
        goal = tip(goal_state)
        got = tip(state)
        assert np.abs(got - rest[:3]).max() <= 1e-9
        assert abs(np.linalg.norm(goal - got) - rest[3]) <= 1e-9
        assert rest[4] <= 60 and rest[5] % 9 == 0
        assert (state >= 0).all() and (state <= 20).all()
        reached += rest[3] <= 1e-6
    assert reached >= 3
    assert any(l.startswith("jac 12 ") for l in out)
    assert "auto_add unsupported" in out
    req = np.array([l.split()[1:] for l in out if l.startswith("request")][0], float)
    # free space: a valid state within tolerance
    (ctl, rest), = [(r[0], r[1]) for r in _rows(out, "rmap")]
    vox = irt.VoxelOctree(256)
    vox.set_xlim(-0.25, 0.25); vox.set_ylim(-0.25, 0.25); vox.set_zlim(-0.25, 0.25)
    og = helpers.oracle_grid(orc, vox)
    assert orc.is_valid_state(orb, og, ctl)[0]
    assert rest[3] <= 1e-4 and np.linalg.norm(tip(ctl) - req) <= 1e-4 + 1e-9
    # the request walled in: every IK solution collides, the answer is a valid state short of it
    box = [int(v) for v in [l.split()[1:] for l in out if l.startswith("box")][0]]
    for ix in range(box[0], box[1] + 1):
        for iy in range(box[2], box[3] + 1):
            for iz in range(box[4], box[5] + 1):
                og.set_cell(ix, iy, iz)
    (ctl, rest), = [(r[0], r[1]) for r in _rows(out, "blocked")]
    assert orc.is_valid_state(orb, og, ctl)[0]
    t = tip(ctl)
    assert np.abs(t - rest[:3]).max() <= 1e-9
    assert abs(rest[3] - np.linalg.norm(t - req)) <= 1e-9 and rest[3] > 1e-4
