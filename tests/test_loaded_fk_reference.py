"""The numpy reference of the loaded FK (tests/loaded_fk_reference.py) against what can be known without it: the oracle's unloaded
right-hand side and shape, closed-form beams, and its own fixtures.  No GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.join(HERE, "golden")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import loaded_fk_reference as ref                                    # noqa: E402


@pytest.fixture(scope="module")
def gen(orc):
    import make_loaded_fk
    return make_loaded_fk


@pytest.fixture(scope="module")
def rob40(orc):
    """config 1's routing (three straight tendons) at dL = L / 40"""
    return orc.Robot([[2 * np.pi * k / 3] for k in range(3)], [[0.01]] * 3, dL=0.2 / 40)


def _random_rotation(rng):
    a, b, c, d = (lambda q: q / np.linalg.norm(q))(rng.normal(size=4))
    return np.array([[a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)],
                     [2 * (b * c + a * d), a * a - b * b + c * c - d * d, 2 * (c * d - a * b)],
                     [2 * (b * d - a * c), 2 * (c * d + a * b), a * a - b * b - c * c + d * d]])


@pytest.mark.parametrize("name", ["config1", "n8", "config3_rot"])
def test_rhs_equals_the_oracles_at_zero_load(gen, name):
    """1e-12 relative: both are fp64 evaluations of the same formulas, one by block inverses, one by a 6 x 6 solve (measured 5e-16)"""
    robot, rob, _ = gen.fixture(name)
    rng = np.random.default_rng(5)
    N = rob.n_tendons
    worst = 0.0
    for _ in range(20):
        tau = rng.uniform(0.0, 10.0, N)
        x = np.zeros(19 + N)
        x[:3] = rng.normal(size=3) * 0.1
        x[3:12] = _random_rotation(rng).T.reshape(9)
        x[12:15] = np.array([0.0, 0.0, 1.0]) + rng.normal(size=3) * 0.01
        x[15:18] = rng.normal(size=3) * 3.0
        t = rng.uniform(0.0, rob.c.L)
        want, got = rob.deriv(tau, x, t), ref.deriv_flat(rob, tau, x, t)
        worst = max(worst, np.abs(got - want).max() / np.abs(want).max())
    print("rhs: %.3g relative" % worst)
    assert worst <= 1e-12


@pytest.mark.parametrize("name", ["config1", "n1", "config3_rot"])
def test_zero_load_takes_no_iteration_and_returns_shape(gen, name):
    """The unloaded solution balances the tip to the robot's own residual_threshold -- the threshold the device stops at -- so
    with that tolerance the shooting starts converged.  (To 1e-11 it does not: solve_initial_bending itself stops at the
    threshold.)  Points within 1e-14 m of Robot.shape's: the same scheme from the same strains (measured < 1e-15)."""
    robot, rob, st = gen.fixture(name)
    out = ref.shoot(rob, st, tol=robot.residual_threshold)
    conv = np.array([rob.shape(s)["converged"] for s in st])
    assert conv.any()
    assert (out["iters"][conv] == 0).all(), out["iters"]
    worst = max(np.abs(out["p"][i] - rob.shape(st[i])["p"]).max() for i in np.nonzero(conv)[0])
    print("zero load: %.3g m" % worst)
    assert worst <= 1e-14


def test_pure_moment_bends_the_untensioned_rod_into_an_arc(rob40):
    """L_e = (5 EI, 0, 0): curvature 5 / m about x, tip at (0, -(1 - cos 1) / 5, sin(1) / 5).  RK4's own error at dL = L / 40 is
    6.5e-10 m; the bound is twice that plus the 1e-9 m interface tolerance: 2e-9 m (rounded down)."""
    _, Kbt = ref.stiffness(rob40)
    out = ref.shoot(rob40, np.zeros((1, 3)), L_e=[5 * Kbt[0], 0.0, 0.0])
    assert out["converged"][0]
    assert np.abs(out["vu0"][0] - [0, 0, 1, 5, 0, 0]).max() <= 1e-9
    err = np.abs(out["p"][0, -1] - [0.0, -(1 - np.cos(1.0)) / 5, np.sin(1.0) / 5]).max()
    print("arc: %.3g m" % err)
    assert err <= 2e-9


def test_small_tip_force_deflects_like_a_timoshenko_cantilever(rob40):
    Kse, Kbt = ref.stiffness(rob40)
    F, L = 1e-3, rob40.c.L
    out = ref.shoot(rob40, np.zeros((1, 3)), F_e=[F, 0.0, 0.0])
    rel = out["p"][0, -1, 0] / (F * L ** 3 / (3 * Kbt[0]) + F * L / Kse[0]) - 1
    print("cantilever: %.3g relative" % rel)
    assert out["converged"][0] and abs(rel) <= 1e-6


@pytest.mark.parametrize("name", ["config1", "n1", "n8", "config3_rot", "n5", "n6"])
def test_generator_reproduces_its_fixture(gen, name):
    """two states per fixture, every case; 1e-12 m / 1e-9 relative: the same arithmetic on, perhaps, another LAPACK"""
    fx = np.load(gen.path(name))
    robot, rob, st = gen.fixture(name)
    assert np.array_equal(st, fx["states"])
    rows = [3, 17]
    for case in gen.CASES:
        got = gen.solve_case(name, robot, rob, st, case, rows)
        for k in ("wrench", "dist"):
            assert np.array_equal(got[k], fx["%s_%s" % (k, case)][rows])
        assert np.abs(got["p"] - fx["p_" + case][rows]).max() <= 1e-12
        assert np.abs(got["vu0"] - fx["vu0_" + case][rows]).max() <= 1e-9
        assert np.allclose(got["bound"], fx["bound_" + case][rows], rtol=1e-6)
        assert (fx["e_ref_" + case] <= 1e-11).all()


def test_library_exports_the_loaded_fk(irt):
    irt.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", irt.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert {"tr_fk_loaded_batch", "tr_fk_loaded_batch_dev"} <= exported
