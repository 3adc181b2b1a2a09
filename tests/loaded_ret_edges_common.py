"""What tests/test_gpu_loaded_ret_edges.py, tests/test_cpp_shim_loaded_ret_edges.py and tests/golden/make_loaded_ret_edges.py share:
the robots of the loaded-retraction fixtures (fk_truth_common.robot_from_fixture), their seeded edges BETWEEN STATES WITH RETRACTION,
the loads and the sphere grids (loaded_edges_common.make_grid).

Edges: |d tau| <= 1 N, |d theta| <= 0.3 (a robot with rotation), |d s_start| <= DS_MAX dL, s_start of the start state in
[0, S_MAX L]; the last seeded edge (NEAR) ends within dL / 4 of L: a backbone of one point and no interval, whose residual is the tip
balance at R = I.  Behind the seeded set, in this order:
  AT_L   ends at s_start = L: one point at the origin, converged
  NEG    ends at s_start < 0: outside the state space's bounds, an unconverged sample, so the edge is invalid
Loads: the gravity of a 50 g robot along -y, 0.05 * 9.81 / L N/m, plus loaded_edges_common's tip force."""
import numpy as np

import fk_truth_common as ftc
from loaded_edges_common import WRENCH, make_grid                     # noqa: F401

#        seeded edges, their seed, tension cap of the start states, seed and count of the spheres, their radius
FIXTURES = {"config3_ret_edges": (31, 3, 12.0, 7, 60, 0.02), "config2_ret_edges": (31, 5, 12.0, 5, 60, 0.02),
            "config3_rot_ret": (5, 3, 12.0, 7, 60, 0.02)}
S_MAX, DS_MAX = 0.6, 8.0
NEAR, AT_L, NEG = -3, -2, -1          # rows of the special edges


def robot(irt, name):
    return ftc.robot_from_fixture(irt, ftc.load(name))


def dist_of(robot):
    """the gravity of a 50 g robot per unit length, along -y"""
    return np.array([0.0, -0.05 * 9.81 / robot.specs.L, 0.0, 0.0, 0.0, 0.0])


def make_edges(robot, n, seed, cap):
    """n seeded edges, NEAR and the two special ones: (a, b), (n + 3, S) each"""
    N, S = len(robot.tendons), robot.state_size()
    L, dL = robot.specs.L, robot.specs.dL
    rng = np.random.default_rng(seed)
    E = n + 3
    a = np.zeros((E, S))
    a[:, :N] = rng.uniform(0.0, cap, (E, N))
    d = rng.normal(size=(E, N))
    b = a.copy()
    b[:, :N] = np.clip(a[:, :N] + d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.3, 1.0, (E, 1)), 0.0, None)
    if robot.enable_rotation:
        a[:, N] = rng.uniform(-np.pi, np.pi, E)
        b[:, N] = a[:, N] + rng.choice([-1.0, 1.0], E) * rng.uniform(0.2, 0.3, E)
        b[b[:, N] > np.pi, N] -= 2 * np.pi
        b[b[:, N] < -np.pi, N] += 2 * np.pi
    a[:, -1] = rng.uniform(0.0, S_MAX * L, E)
    b[:, -1] = np.clip(a[:, -1] + rng.choice([-1.0, 1.0], E) * rng.uniform(0.5, DS_MAX, E) * dL, 0.0, L - 2 * dL)
    a[NEAR, -1], b[NEAR, -1] = L - 2.6 * dL, L - dL / 4
    a[AT_L, -1], b[AT_L, -1] = L - 3.0 * dL, L
    a[NEG, -1], b[NEG, -1] = 2.0 * dL, -dL
    assert (np.linalg.norm(b[:, :N] - a[:, :N], axis=1) <= 1.0).all()
    assert (np.abs(b[:n, -1] - a[:n, -1]) <= DS_MAX * dL * (1 + 1e-12)).all()
    return np.ascontiguousarray(a), np.ascontiguousarray(b)


def world(irt, name):
    """(robot, a, b, voxels) of a fixture"""
    n, eseed, cap, gseed, count, radius = FIXTURES[name]
    rb = robot(irt, name)
    a, b = make_edges(rb, n, eseed, cap)
    return rb, a, b, make_grid(irt, rb.specs.dL, gseed, count, radius)
