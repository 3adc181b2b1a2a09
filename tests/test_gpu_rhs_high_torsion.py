"""The Cosserat right-hand side where the terms its rewrite removed are largest.

fk_kernel.hpp forms the moment balance c = -u x (K_bt u) - v x (K_se (v - e3)) - b from the two factors that survive when
K_bt = diag(kb0, kb0, kb2) and K_se = diag(ks0, ks0, ks2): (kb2 - kb0) u2 and ks2 (v2 - 1) - ks0 v2.  What that drops grows
with the torsion u2 and with shear and stretch, so a slip in the algebra shows where every tendon pulls with close to its
largest tension the same way round the backbone -- not in a batch of uniform tensions, whose torsion mostly cancels.
States: seeded, tensions in the top 15 % of each tendon's range for the tendons that wind one way (the rest slack, or all of
them taut); robots: BASELINE configs 2 and 3 and the 4-tendon robot with rotation and retraction.  Reference: the CPU oracle.
Tolerances: those of tests/test_gpu_golden.py (points 1e-9 m, lengths 1e-10, converged equal)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
TIP_TOL = 1e-9
LEN_TOL = 1e-10


def _robot(irt, kind):
    W = irt.workloads
    if kind == "config2":
        return W.robot_config2()
    r = W.robot_config3()
    if kind == "config3_rot_retract":
        r.enable_rotation = True
        r.enable_retraction = True
    return r


def _taut_states(robot, n, seed):
    """n states per group; group g: the tendons of one winding sense (sign of the angle's linear coefficient) in the top 15 %
    of their range and the others below 5 % of it -- then one group with every tendon taut."""
    rng = np.random.default_rng(seed)
    sense = np.array([np.sign(t.C[1]) if len(t.C) > 1 else 0.0 for t in robot.tendons])
    tmax = np.array([t.max_tension for t in robot.tendons])
    groups = [sense > 0, sense < 0, np.ones(len(tmax), bool)]
    rows = []
    for taut in groups:
        if not taut.any():
            continue
        tau = np.where(taut, rng.uniform(0.85, 1.0, (n, len(tmax))), rng.uniform(0.0, 0.05, (n, len(tmax)))) * tmax
        cols = [tau]
        if robot.enable_rotation:
            cols.append(rng.uniform(-np.pi, np.pi, (n, 1)))
        if robot.enable_retraction:
            cols.append(rng.uniform(0.0, 0.6 * robot.specs.L, (n, 1)))       # long backbones: the torsion has length to act on
        rows.append(np.hstack(cols))
    return np.ascontiguousarray(np.vstack(rows))


@pytest.mark.parametrize("kind", ["config2", "config3", "config3_rot_retract"])
def test_fk_against_oracle_at_high_torsion(irt, orc, helpers, kind):
    robot = _robot(irt, kind)
    states = _taut_states(robot, 192, seed=97)
    got = robot.shape_batch(states)
    want = helpers.oracle_robot(orc, robot).fk_batch(states)
    P = got["p"].shape[1]
    wp = want["p"][:, :P]
    assert np.array_equal(np.isnan(got["p"]), np.isnan(wp))
    err = np.nanmax(np.abs(got["p"] - wp))
    len_err = np.abs(got["L_i"] - want["L_i"]).max()
    print("%s: %d states, max point error %.3g m, max L_i error %.3g, %d converged" %
          (kind, len(states), err, len_err, int(want["converged"].sum())))
    assert err <= TIP_TOL
    assert len_err <= LEN_TOL
    assert np.array_equal(got["converged"], want["converged"])
    # the states do what they are for: the backbone leaves its axis by centimetres
    assert np.nanmax(np.abs(got["p"][:, :, :2])) > 0.01
