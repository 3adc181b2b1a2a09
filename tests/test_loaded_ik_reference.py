"""The numpy specification of the loaded tip IK (tests/loaded_ik_reference.py) on the CPU: it reaches the fixtures' loaded tips, and
its implicit-function Jacobian is the derivative of the loaded tip.

Goals are the loaded tips of the fixtures (tests/golden/loaded_fk_<name>.npz), starts the fixture states plus seeded normal offsets
(seed 5), clipped to the bounds."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.join(HERE, "golden")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import loaded_fk_reference as ref                                    # noqa: E402
import loaded_ik_reference as ikr                                    # noqa: E402

GRAVITY = np.array([0.0, -2.4525, 0.0, 0.0, 0.0, 0.0])

# |J_r - J_fd| / |J_fd| (Frobenius) per state, J_fd: central differences with steps of 1e-3 N through solves stopped at 1e-11 N.
# Over config1's 24 states under case B the figure was 1.32e-7 in the median and 1.09e-6 at most when this file was written (the test
# prints it).  The bound is the largest figure times 10.  (With levmar's relative step on the strains the figure was 2.1e-3: see
# loaded_ik_reference.py.)
JACOBIAN_BOUND = 1.09e-5


@pytest.fixture(scope="module")
def gen(orc):
    import make_loaded_fk
    return make_loaded_fk


def _case(gen, name, case):
    robot, rob, st = gen.fixture(name)
    fx = dict(np.load(gen.path(name)))
    return rob, st, fx, np.ascontiguousarray(fx["p_" + case][:, -1])


@pytest.mark.parametrize("name,case,sigma_tension,sigma_rotation", [("config1", "B", 3.0, 0.0), ("config1", "C", 3.0, 0.0), ("n1", "B", 1.5, 0.3)])
def test_it_reaches_the_loaded_tips(gen, name, case, sigma_tension, sigma_rotation):
    rob, st, fx, goals = _case(gen, name, case)
    starts = ikr.offset_starts(rob, st, sigma_tension, sigma_rotation)
    if rob.c.enable_rotation:
        loads = dict(dist=GRAVITY, frame="world")                 # the fixture's rows are gravity turned by Rz(-theta)
    else:
        loads = dict(wrench=fx["wrench_" + case], dist=fx["dist_" + case])
    out = ikr.inverse_kinematics_loaded_batch(rob, starts, goals, max_iters=10, **loads)
    print("%s %s: reached %d of 24, outer iterations <= %d, integrations %.0f per problem"
          % (name, case, (out["error"] <= 1e-4).sum(), out["iters"].max(), out["integrations"].mean()))
    assert out["equilibrium"].all()
    assert (out["error"] <= 1e-4).all()
    lo, hi = ikr.bounds(rob)
    assert ((out["state"] >= lo) & (out["state"] <= hi)).all()
    # the returned strains are an equilibrium of the returned state, and the returned tip is its tip: both carry the last Newton
    # step of the scheme without an integration behind it, which is second order in a displacement of at most 1e-5 m -- 1e-9 m,
    # the project's interface tolerance, is orders above that
    w, d = ikr.load_rows(rob, out["state"], loads.get("wrench"), loads["dist"], loads.get("frame", "base"))
    x, e = ikr.tips_and_residuals(rob, out["state"], out["vu0"], w, d)
    assert (np.linalg.norm(e, axis=1) <= rob.c.residual_threshold).all()
    assert np.abs(x - out["tip"]).max() <= 1e-9


def test_it_reaches_the_tips_under_a_full_distributed_row(gen):
    """config1 under one distributed row with a z component and a moment per unit length (the set config1_full of
    tests/test_gpu_loaded_ik.py): goals are the numpy shooting's tips under that row, and the scheme reaches FULL_REACHED = 24 of 24,
    every row an equilibrium whose tip is the returned one."""
    from loaded_edges_common import DIST_FULL
    rob, st, fx, _ = _case(gen, "config1", "B")
    assert DIST_FULL.all()
    goals = ikr.loaded_tips(rob, st, dist=DIST_FULL)
    moved = np.linalg.norm(goals - fx["p_B"][:, -1], axis=1)
    starts = ikr.offset_starts(rob, st, 3.0, 0.0)
    out = ikr.inverse_kinematics_loaded_batch(rob, starts, goals, max_iters=10, dist=DIST_FULL)
    reached = out["error"] <= 1e-4
    print("config1 under the full row: reached %d of 24, outer iterations <= %d; the row moves the tips of case B by %.3g .. %.3g m"
          % (reached.sum(), out["iters"].max(), moved.min(), moved.max()))
    assert out["equilibrium"].all()
    assert reached.sum() == ikr.FULL_REACHED == 24
    assert moved.min() > 10 * 1e-4                                       # the row matters at the stop threshold
    w, d = ikr.load_rows(rob, out["state"], None, DIST_FULL)
    x, e = ikr.tips_and_residuals(rob, out["state"], out["vu0"], w, d)
    assert (np.linalg.norm(e, axis=1) <= rob.c.residual_threshold).all()
    assert np.abs(x - out["tip"]).max() <= 1e-9


@pytest.mark.parametrize("name", ["n5", "n6", "n8"])
def test_it_reaches_the_loaded_tips_at_wider_state_sizes(gen, name):
    """S = 6, 7, 9 under gravity in the world frame at 25 outer iterations: at least 21 of 24 reached (measured: 24, 22, 21; rows
    20 - 22 start and end on the tension box), and the rows this scheme ends at half the stop threshold are the recorded ones."""
    rob, st, fx, goals = _case(gen, name, "B")
    starts = ikr.offset_starts(rob, st, *ikr.WIDE_SIGMA)
    out = ikr.inverse_kinematics_loaded_batch(rob, starts, goals, max_iters=ikr.WIDE_MAX_ITERS, dist=GRAVITY, frame="world")
    reached = out["error"] <= 1e-4
    print("%s: reached %d of 24 (not: %s), outer iterations <= %d" % (name, reached.sum(), np.flatnonzero(~reached).tolist(), out["iters"].max()))
    assert out["equilibrium"].all()
    assert reached.sum() >= 21
    assert tuple(np.flatnonzero(out["error"] <= 0.5e-4)) == ikr.WIDE_HALF_TOL_ROWS[name]
    lo, hi = ikr.bounds(rob)
    assert ((out["state"] >= lo) & (out["state"] <= hi)).all()


def test_the_reduced_jacobian_is_the_derivative_of_the_loaded_tip(gen):
    rob, st, fx, _ = _case(gen, "config1", "B")
    dist = fx["dist_B"][0]
    y = fx["vu0_B"]                                                   # the fixture's equilibria, |e| <= 1e-11
    lin = ikr.linearise(rob, st, y, dist=dist)
    n, S = st.shape
    h = 1e-3
    fd = np.zeros((n, 3, S))
    for k in range(S):
        tips = []
        for sign in (-1.0, 1.0):
            s2 = st.copy()
            s2[:, k] += sign * h
            sol = ref.shoot(rob, s2, f_e=dist[:3], l_e=dist[3:], guess=y, tol=1e-11, max_iters=20)
            assert sol["converged"].all()
            tips.append(sol["p"][:, -1])
        fd[:, :, k] = (tips[1] - tips[0]) / (2 * h)
    rel = np.linalg.norm((lin["J_r"] - fd).reshape(n, -1), axis=1) / np.linalg.norm(fd.reshape(n, -1), axis=1)
    print("reduced Jacobian against differences of solves: relative difference median %.3g, max %.3g" % (np.median(rel), rel.max()))
    assert rel.max() <= JACOBIAN_BOUND
