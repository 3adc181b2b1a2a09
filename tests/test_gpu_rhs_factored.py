"""The Cosserat right-hand side in its factored form, where the factors vanish or are largest.

fk_kernel.hpp forms a_i = A_i w as cs2 p with p = pd (pd.w)/|pd|^2 - w and cs2 = -tau/|pd|, and b from (cs2 rx, cs2 ry, 0) x p:
a tension of exactly 0 makes cs2 (and c, t1, t2) a signed zero that multiplies everything of its tendon, all tensions 0 leave
the bare rod, all tensions at their maximum make every term as large as the robot allows.  States: 256 in four groups of 64 --
one tendon (in turn) at exactly 0 and the others seeded; all 0; all at max_tension; all seeded -- on the robots of
tests/test_gpu_rhs_high_torsion.py: BASELINE configs 2 and 3 and the 4-tendon robot with rotation and retraction.
Reference: the CPU oracle, with the margins of that test (points 1e-9 m, lengths 1e-10, converged equal).  And for the same
states the tips fk_verdict / fk_verdict_retract report are the last stored point of fk_rk4_batch bit for bit: every kernel
that holds the right-hand side forms the same bits."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
TIP_TOL = 1e-9
LEN_TOL = 1e-10
KINDS = ["config2", "config3", "config3_rot_retract"]
_cache = {}


def _robot(irt, kind):
    W = irt.workloads
    if kind == "config2":
        return W.robot_config2()
    r = W.robot_config3()
    if kind == "config3_rot_retract":
        r.enable_rotation = True
        r.enable_retraction = True
    return r


def _states(robot, seed):
    rng = np.random.default_rng(seed)
    tmax = np.array([t.max_tension for t in robot.tendons])
    N, g = len(tmax), 64
    one_zero = rng.uniform(0.0, 1.0, (g, N)) * tmax
    one_zero[np.arange(g), np.arange(g) % N] = 0.0
    tau = np.vstack([one_zero, np.zeros((g, N)), np.tile(tmax, (g, 1)), rng.uniform(0.0, 1.0, (g, N)) * tmax])
    cols = [tau]
    if robot.enable_rotation:
        cols.append(rng.uniform(-np.pi, np.pi, (4 * g, 1)))
    if robot.enable_retraction:
        cols.append(rng.uniform(0.0, 0.6 * robot.specs.L, (4 * g, 1)))
    st = np.ascontiguousarray(np.hstack(cols))
    assert st.shape[0] == 256 and (st[:g, :N] == 0).sum(axis=1).min() == 1 and not st[g:2 * g, :N].any()
    return st


def _fk(irt, kind):
    """robot, states and the stored-point result (computed once per robot)."""
    if kind not in _cache:
        robot = _robot(irt, kind)
        states = _states(robot, seed=131)
        _cache[kind] = (robot, states, robot.shape_batch(states))
    return _cache[kind]


@pytest.mark.parametrize("kind", KINDS)
def test_fk_against_oracle_with_vanishing_and_largest_tensions(irt, orc, helpers, kind):
    robot, states, got = _fk(irt, kind)
    want = helpers.oracle_robot(orc, robot).fk_batch(states)
    P = got["p"].shape[1]
    wp = want["p"][:, :P]
    assert np.array_equal(np.isnan(got["p"]), np.isnan(wp))
    err = np.nanmax(np.abs(got["p"] - wp), axis=(1, 2)).reshape(4, 64).max(axis=1)
    len_err = np.abs(got["L_i"] - want["L_i"]).max(axis=1).reshape(4, 64).max(axis=1)
    print("%s: max point error per group (one 0 / all 0 / all max / seeded) %s m, max L_i error %s, %d of %d converged" %
          (kind, ["%.3g" % e for e in err], ["%.3g" % e for e in len_err], int(want["converged"].sum()), len(states)))
    assert err.max() <= TIP_TOL
    assert len_err.max() <= LEN_TOL
    assert np.array_equal(got["converged"], want["converged"])


@pytest.mark.parametrize("kind", KINDS)
def test_verdict_tips_are_the_last_stored_point(irt, kind):
    robot, states, got = _fk(irt, kind)
    vox = irt.VoxelOctree(256)
    vox.set_xlim(-0.3, 0.3); vox.set_ylim(-0.3, 0.3); vox.set_zlim(-0.3, 0.3)
    chk = irt.VoxelBackboneValidityChecker(robot, irt.VoxelEnvironment(), vox)
    det = chk.is_valid_detail(states)
    chk.engine.close()
    last = got["p"][np.arange(len(states)), got["n_points"] - 1]
    assert not np.isnan(last).any()
    assert np.array_equal((det["flags"] & 1) != 0, got["converged"].astype(bool))
    diff = np.flatnonzero((det["tips"] != last).any(axis=1))
    print("%s: %d of %d tips differ from the last stored point" % (kind, diff.size, len(states)))
    assert np.array_equal(det["tips"], last), (diff[:8], np.abs(det["tips"] - last).max())
