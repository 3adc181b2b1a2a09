"""Tip positions, the tip Jacobian and batched tip IK on the device (tr_fk_tips, tr_tip_jacobian, tr_ik_batch; csrc/ik_kernel.hpp):
the tips are fk_batch's last point bit for bit, the Jacobian is TendonRobot.tip_jacobian_batch's bit for bit and the oracle's to
1e-12 m of tip, and the device IK keeps the contract of tip_control.inverse_kinematics_batch, whose scheme it runs.

State sizes: config2 (S = 3), config3 (4), rot_ret (config2 with rotation and retraction, 5) and, from the robots of the truth
fixtures (tests/golden/make_fk_truth.py: fixture_robot), n1 (2), n6 (7), n8 (9) and n8_ret (10 = TRK_IK_MAX_S): ik_lm_step<S> and
the 2 S + 1 lanes of the Jacobian at the smallest and the largest S and two sizes between."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

pytestmark = pytest.mark.gpu
OLD_KINDS = ["config2", "config3", "rot_ret"]
NEW_KINDS = ["n1", "n6", "n8", "n8_ret"]
KINDS = OLD_KINDS + NEW_KINDS


def _cap(robot, kind, old):
    """Tension cap of the random states: `old` for the first three kinds, 12 / sqrt(N) for the robots of the truth fixtures."""
    return old if kind in OLD_KINDS else 12.0 / np.sqrt(len(robot.tendons))


def _robot(irt, kind):
    if kind in NEW_KINDS:
        import make_fk_truth
        return make_fk_truth.fixture_robot(irt, kind)[0]
    W = irt.workloads
    robot = W.robot_config3() if kind == "config3" else W.robot_config2()
    if kind == "rot_ret":
        robot.enable_rotation = True
        robot.enable_retraction = True
    return robot


def _states(irt, robot, n, seed, cap=15.0):
    st = irt.workloads.random_states(robot, n, seed=seed, tau_max=cap)
    if robot.enable_retraction:
        rng = np.random.default_rng(seed + 1)
        st[:, -1] = rng.uniform(0.0, robot.specs.L, n)
        st[::7, -1] = robot.specs.L - rng.uniform(0.0, 3 * robot.specs.dL, len(st[::7]))    # short backbones
    return st


@pytest.mark.parametrize("kind", KINDS)
def test_fk_tips_are_fk_batch_last_point(irt, kind):
    robot = _robot(irt, kind)
    eng = robot.engine(0)
    for n in (1, 63, 64, 65, 70000):
        st = _states(irt, robot, n, seed=n, cap=_cap(robot, kind, 15.0))
        ref = eng.fk_batch(st)
        want = ref["p"][np.arange(n), ref["n_points"] - 1]
        tips, conv = eng.fk_tips(st)
        assert np.array_equal(tips.view(np.uint64), want.view(np.uint64)), (kind, n)
        assert np.array_equal(conv, ref["converged"])


def _jacobian_inputs(irt, robot, delta=1e-6, cap=15.0):
    st = _states(irt, robot, 200, seed=5, cap=cap)
    st[:10, : len(robot.tendons)] = 0.0                          # zero tensions: d = delta
    if robot.enable_rotation:
        N = len(robot.tendons)
        st[10:20, N] = np.pi - np.linspace(0, 1e-9, 10)
        st[20:30, N] = -np.pi + np.linspace(0, 1e-9, 10)
    if robot.enable_retraction:
        L = robot.specs.L
        d = np.maximum(np.abs(1e-4 * L), delta)
        st[30:40, -1] = L - np.linspace(0.0, 0.9, 10) * d        # p + d crosses the FK wrapper's threshold
    return st


@pytest.mark.parametrize("kind", KINDS)
def test_jacobian_equals_python_path_and_dev_equals_host(irt, kind):
    import torch
    robot = _robot(irt, kind)
    st = _jacobian_inputs(irt, robot, cap=_cap(robot, kind, 15.0))
    want = robot.tip_jacobian_batch(st, delta=1e-6)
    J, tips = robot.engine(0).tip_jacobian(st, delta=1e-6, want_tips=True)
    assert np.array_equal(J.view(np.uint64), want.view(np.uint64))
    f = irt.tip_control._tips(robot, st, 0)
    assert np.array_equal(tips.view(np.uint64), f.view(np.uint64))
    n, S = st.shape
    d_st = torch.from_numpy(st).cuda()
    d_J = torch.empty(n * 3 * S, dtype=torch.float64, device="cuda")
    d_t = torch.empty(n * 3, dtype=torch.float64, device="cuda")
    robot.engine(0).tip_jacobian_dev(d_st, n, d_J, delta=1e-6, d_tips=d_t)
    torch.cuda.synchronize()
    assert np.array_equal(d_J.cpu().numpy().reshape(n, 3, S), J) and np.array_equal(d_t.cpu().numpy().reshape(n, 3), tips)


@pytest.mark.parametrize("kind", KINDS)
def test_jacobian_matches_oracle_differences(irt, orc, helpers, kind):
    robot = _robot(irt, kind)
    st = _jacobian_inputs(irt, robot, cap=_cap(robot, kind, 15.0))[::10][:20]
    delta = 1e-6
    J = robot.engine(0).tip_jacobian(st, delta=delta)
    orb = helpers.oracle_robot(orc, robot)
    L = robot.specs.L

    def tip(x):
        if robot.enable_retraction and x[-1] > L:
            return np.array([0.0, 0.0, L - x[-1]])
        return orb.shape(x)["p"][-1]

    for i, p in enumerate(st):
        d = np.maximum(np.abs(1e-4 * p), delta)
        for j in range(len(p)):
            a, b = p.copy(), p.copy()
            a[j] -= d[j]
            b[j] += d[j]
            Jo = (tip(b) - tip(a)) * (0.5 / d[j])
            assert (np.abs(J[i, :, j] - Jo) <= 1e-12 / d[j]).all(), (i, j, J[i, :, j], Jo)


def _ik_case(irt, orc, helpers, kind):
    """test_gpu_ik.py::test_reachable_targets_are_reached's targets and starts"""
    W, T = irt.workloads, irt.tip_control
    robot = _robot(irt, kind)
    n = 48
    goal_states = W.random_states(robot, n, seed=11, tau_max=_cap(robot, kind, 12.0))
    sigma = 1.5 if kind in OLD_KINDS else 1.5 / np.sqrt(len(robot.tendons))
    if robot.enable_retraction:
        goal_states[:, -1] = np.random.default_rng(1).uniform(0.0, 0.08, n)
    orb = helpers.oracle_robot(orc, robot)
    goals = np.array([orb.shape(s)["p"][-1] for s in goal_states])
    rng = np.random.default_rng(12)
    start = goal_states + rng.normal(size=goal_states.shape) * (np.array([sigma] * len(robot.tendons) + ([0.3] if robot.enable_rotation else [])
                                                                         + ([0.01] if robot.enable_retraction else [])))
    b = T.Bounds.from_robot(robot)
    start = np.clip(start, np.maximum(b.lower, -10), np.minimum(b.upper, 25))
    return robot, orb, goals, start, b


LM = dict(stop_threshold_err=1e-6, stop_threshold_Dp=1e-12, stop_threshold_JT_err_inf=1e-16, max_iters=60)


@pytest.mark.parametrize("kind", KINDS)
def test_device_ik_reaches_targets_and_agrees_with_python(irt, orc, helpers, kind):
    """Floor on the reached fraction: 0.9 for the first three kinds.  For n1, n6, n8, n8_ret (48 problems, tension offsets of sigma =
    1.5 / sqrt(N) from goal states capped at 12 / sqrt(N)) the Python scheme with the oracle as its FK reaches 0.958, 0.938, 0.875 and
    1.000 of the goals at LM's settings, so the floor is 0.85 on both paths, and the device must reach every problem the Python
    path ends at 0.5e-6 m or less."""
    T = irt.tip_control
    robot, orb, goals, start, b = _ik_case(irt, orc, helpers, kind)
    floor = 0.9 if kind in OLD_KINDS else 0.85
    r = T.inverse_kinematics_batch_device(robot, start, goals, **LM)
    print("%s: device reaches %.3f of %d" % (kind, (r["error"] <= 1e-6).mean(), len(goals)))
    assert (r["error"] <= 1e-6).mean() > floor, np.sort(r["error"])[-8:]
    assert (r["state"] >= b.lower).all() and (r["state"] <= b.upper).all()
    if robot.enable_rotation:
        rot = r["state"][:, len(robot.tendons)]
        assert (rot >= -np.pi).all() and (rot < np.pi).all()
    for i in (0, 7, 23, 40):
        tip = orb.shape(r["state"][i])["p"][-1]
        assert np.abs(tip - r["tip"][i]).max() <= 1e-9
        assert abs(np.linalg.norm(goals[i] - tip) - r["error"][i]) <= 1e-9
    S = robot.state_size()
    assert (r["num_fk_calls"] % (2 * S + 1) == 0).all() and (r["iters"] <= 60).all()
    assert r["launches"] <= r["iters"].max() + 1
    py = T.inverse_kinematics_batch(robot, start, goals, **LM)
    tol = 1e-6 * (1 + np.abs(py["state"]).max(1))
    same = (np.abs(r["state"] - py["state"]).max(1) <= tol).mean()
    print("%s: Python path reaches %.3f; states of the two paths agree on %.3f" % (kind, (py["error"] <= 1e-6).mean(), same))
    if kind in OLD_KINDS:
        assert same >= 0.9
    else:
        assert (py["error"] <= 1e-6).mean() > floor, np.sort(py["error"])[-8:]
        must = py["error"] <= 0.5e-6
        assert (r["error"][must] <= 1e-6).all(), (np.flatnonzero(must & ~(r["error"] <= 1e-6)), r["error"][must].max())


@pytest.mark.parametrize("kind", ["config3", "rot_ret"])
def test_device_ik_result_does_not_depend_on_the_batch(irt, orc, helpers, kind):
    robot, orb, goals, start, b = _ik_case(irt, orc, helpers, kind)
    eng = robot.engine(0)
    i0 = 5
    alone = eng.ik_batch(start[i0:i0 + 1], goals[i0], **LM)
    rng = np.random.default_rng(3)
    big_s = np.concatenate([start] * 11)[:500]
    big_g = np.concatenate([goals] * 11)[:500]
    perm = rng.permutation(500)
    where = int(np.flatnonzero(perm == i0)[0])
    big = eng.ik_batch(big_s[perm], big_g[perm], **LM)
    again = eng.ik_batch(big_s[perm], big_g[perm], **LM)
    for key in ("state", "tip", "error", "iters", "num_fk_calls"):
        assert np.array_equal(np.asarray(big[key][where]), np.asarray(alone[key][0])), key
        assert np.array_equal(big[key], again[key]), key


def test_device_ik_dev_form_equals_host_form(irt, orc, helpers):
    import torch
    robot, orb, goals, start, b = _ik_case(irt, orc, helpers, "rot_ret")
    eng = robot.engine(0)
    host = eng.ik_batch(start, goals, **LM)
    n, S = start.shape
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d_out = torch.empty(n * S, dtype=torch.float64, device="cuda")
    d_tip = torch.empty(n * 3, dtype=torch.float64, device="cuda")
    d_err = torch.empty(n, dtype=torch.float64, device="cuda")
    d_it = torch.empty(n, dtype=torch.int32, device="cuda")
    d_fk = torch.empty(n, dtype=torch.int32, device="cuda")
    rounds = eng.ik_batch_dev(dev(start), n, dev(goals), d_out, d_tip, d_err, d_it, d_fk, **LM)
    torch.cuda.synchronize()
    assert rounds == host["rounds"]
    assert np.array_equal(d_out.cpu().numpy().reshape(n, S), host["state"])
    assert np.array_equal(d_tip.cpu().numpy().reshape(n, 3), host["tip"])
    assert np.array_equal(d_err.cpu().numpy(), host["error"])
    assert np.array_equal(d_it.cpu().numpy(), host["iters"]) and np.array_equal(d_fk.cpu().numpy(), host["num_fk_calls"])


def test_device_ik_edge_cases(irt):
    T = irt.tip_control
    robot = irt.workloads.robot_config2()
    start = np.array([[-3.0, 25.0, 4.0], [1.0, 2.0, 3.0]])
    r = T.inverse_kinematics_batch_device(robot, start, [0.01, 0.0, 0.19], max_iters=0)
    assert np.array_equal(r["state"], np.clip(start, 0.0, 20.0)) and (r["iters"] == 0).all() and r["launches"] == 1
    assert (r["num_fk_calls"] == 7).all()
    res = T.inverse_kinematics_device(robot, [2.0, 2.0, 2.0], [0.5, 0.0, 0.0], max_iters=25)
    assert isinstance(res, T.IKResult) and res.iters <= 25 and np.isfinite(res.error) and res.error > 0.25
    assert np.isfinite(res.state).all() and (res.state >= 0).all() and (res.state <= 20).all()
    with pytest.raises(irt.InvalidArgument, match="State is not the right size"):
        T.inverse_kinematics_device(robot, [1.0, 2.0], [0, 0, 0.2])
    with pytest.raises(irt.InvalidArgument, match="State is not the right size"):
        robot.engine(0).tip_jacobian([[1.0, 2.0]])
