"""Load profiles on the CPU: the table of stage weights in numpy (irt.load_profile_table, the bits tr_set_load_profile installs), the
new names of every layer, the reference helper (tests/load_profile_reference.py), and the rows its IK sets reach.

The table is held to the header's formula evaluated per entry, written out here a second time:
  x <= s_0: w_0;  x >= s_K-1: w_K-1;  else, k the last knot at or below x,  w_k + (w_k+1 - w_k) * ((x - s_k) / (s_k+1 - s_k))
at the abscissae of loaded_fk_reference.step_list (entry 0 at s = 0; 1 + 3k, + 1, + 2 at t_k, t_k + h * 0.5, t_k + h)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.join(HERE, "golden")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import load_profile_reference as lpr                                 # noqa: E402
import loaded_fk_reference as ref                                    # noqa: E402

NEW_ABI = ("tr_set_load_profile", "tr_clear_load_profile", "tr_get_load_profile")


@pytest.fixture(scope="module")
def gen(orc):
    import make_loaded_fk
    return make_loaded_fk


def formula(s, w, x):
    if x <= s[0]:
        return w[0]
    if x >= s[-1]:
        return w[-1]
    k = max(i for i in range(len(s) - 1) if s[i] <= x)
    return w[k] + (w[k + 1] - w[k]) * ((x - s[k]) / (s[k + 1] - s[k]))


def abscissae(rob):
    out = [0.0]
    for cur, h, _ in ref.step_list(rob)[1]:
        out += [cur, cur + h * 0.5, cur + h]
    return out


def test_new_calls_are_exported(irt):
    assert set(NEW_ABI) <= set(irt._lib.ABI_SYMBOLS)
    header = open(irt._lib.HEADER).read()
    for name in NEW_ABI:
        assert "int %s(" % name in header, name
    assert "load_profile_table" in irt.__all__ and callable(irt.load_profile_table)
    for name in ("set_load_profile", "clear_load_profile", "load_profile_table", "load_profile"):
        assert callable(getattr(irt.Engine, name)), name
    assert callable(irt.VoxelBackboneValidityChecker.load_profile)
    import inspect
    for fn in (irt.TendonRobot.general_shape, irt.TendonRobot.general_shape_batch, irt.TendonRobot.tip_jacobian_loaded_batch,
               irt.tip_control.inverse_kinematics_loaded_batch_device, irt.tip_control.tip_compliance_loaded,
               irt.tip_control.loaded_tips_batch_device, irt.tip_control.damped_resolved_rate_update_batch_device):
        assert "load_profile" in inspect.signature(fn).parameters, fn
    assert "profile" in inspect.signature(irt.VoxelBackboneValidityChecker.set_loads).parameters


@pytest.mark.parametrize("name", ["config1", "config3_rot", "n1"])
def test_the_table_is_the_formula_at_the_stage_abscissae(gen, irt, name):
    robot, rob, _ = gen.fixture(name)
    L = robot.specs.L
    xs = abscissae(rob)
    on_a_stage = xs[1 + 3 * 7]                                         # a knot exactly on a stage abscissa
    profiles = [lpr.profile("tip", L), lpr.profile("zig", L),
                (np.array([0.3 * L]), np.array([1.7])),                # K = 1: the one weight everywhere
                (np.array([0.2 * L, 0.6 * L]), np.array([2.0, -1.0])),  # the end values hold on both sides of the knots
                (np.array([-1.0, 2.0 * L]), np.array([0.5, 4.0])),     # knots outside the backbone: no clamping at all
                (np.array([0.0, on_a_stage, L]), np.array([1.0, 0.37, 2.0]))]
    for s, w in profiles:
        tab = irt.load_profile_table(robot, s, w)
        assert tab.shape == (len(xs),) and tab.dtype == np.float64
        want = np.array([formula(s, w, x) for x in xs])
        assert np.array_equal(tab, want)
    s, w = profiles[2]
    assert (irt.load_profile_table(robot, s, w) == 1.7).all()
    s, w = profiles[3]
    tab, x = irt.load_profile_table(robot, s, w), np.array(xs)
    assert (tab[x <= 0.2 * L] == 2.0).all() and (tab[x >= 0.6 * L] == -1.0).all() and (x <= 0.2 * L).sum() > 3 and (x >= 0.6 * L).sum() > 3
    s, w = profiles[5]
    tab = irt.load_profile_table(robot, s, w)
    assert tab[1 + 3 * 7] == 0.37 and tab[0] == 1.0 and tab[-1] == 2.0


def test_argument_errors(gen, irt):
    robot, _, _ = gen.fixture("config1")
    L = robot.specs.L
    for s, w in (([], []), ([0.0, L], [1.0]), ([0.0, 0.0], [1.0, 2.0]), ([0.1, 0.05], [1.0, 2.0]), ([0.0, np.nan], [1.0, 2.0]),
                 ([0.0, np.inf], [1.0, 2.0]), ([0.0, L], [1.0, np.inf]), ([0.0, L], [np.nan, 1.0])):
        with pytest.raises(irt.InvalidArgument):
            irt.load_profile_table(robot, s, w)
    ret = irt.workloads.robot_config1()
    ret.enable_retraction = True
    with pytest.raises(irt.Unsupported):
        irt.load_profile_table(ret, [0.0, L], [1.0, 2.0])


def test_the_helper_scales_the_row_and_restores_the_references(gen):
    """Under the helper a constant weight c is the row c * d (bit for bit, c a power of two), weights of one change nothing, and the
    `tip` profile moves the tips of case B by millimetres; afterwards the references are the plain ones again."""
    robot, rob, st = gen.fixture("config1")
    fx = dict(np.load(gen.path("config1")))
    st, d, y = st[:4], fx["dist_B"][:4], fx["vu0_B"][:4]
    plain = ref.evaluate(rob, st, y, f_e=d[:, :3], l_e=d[:, 3:])
    rhs, routing = ref.rhs, ref.Routing
    with lpr.under([0.0, 0.1], [1.0, 1.0]):
        ones = ref.evaluate(rob, st, y, f_e=d[:, :3], l_e=d[:, 3:])
    with lpr.under([0.05], [0.5]):
        half = ref.evaluate(rob, st, y, f_e=d[:, :3], l_e=d[:, 3:])
    with pytest.raises(ZeroDivisionError):
        with lpr.under([0.05], [0.5]):
            1 / 0
    assert ref.rhs is rhs and ref.Routing is routing
    scaled = ref.evaluate(rob, st, y, f_e=0.5 * d[:, :3], l_e=0.5 * d[:, 3:])
    for k in ("p", "L", "L_i", "e"):
        assert np.array_equal(ones[k], plain[k]) and np.array_equal(half[k], scaled[k]), k
    with lpr.under(*lpr.profile("tip", robot.specs.L)):
        tip = ref.shoot(rob, st, f_e=d[:, :3], l_e=d[:, 3:])
    assert tip["converged"].all()
    moved = np.linalg.norm(tip["p"][:, -1] - fx["p_B"][:4, -1], axis=1)
    print("tip profile: the solved tips of case B move by %.3g .. %.3g m" % (moved.min(), moved.max()))
    assert moved.min() > 3e-3                                         # (millimetres: hundreds of the fixtures' bound_B)


@pytest.mark.parametrize("name", sorted(lpr.IK_SETS))
def test_the_ik_sets_reach_their_recorded_rows(gen, name):
    """The numpy IK under the `tip` profile (max_iters = 25) reaches 24 of 24 at 1e-4 m; the rows it ends at <= 0.5e-4 m are the
    recorded ones, which the device must reach (tests/test_gpu_load_profile.py).  The same goals without the profile end at other
    states."""
    _, rob, st = gen.fixture(name)
    out = lpr.ik_reference(name, rob, st)
    reached = out["error"] <= 1e-4
    print("%s: reached %d of 24, worst %.3g m, outer iterations <= %d; <= 0.5e-4 m: %s"
          % (name, reached.sum(), out["error"].max(), out["iters"].max(), np.flatnonzero(out["error"] <= 0.5e-4).tolist()))
    assert out["equilibrium"].all() and reached.all()
    assert tuple(np.flatnonzero(out["error"] <= 0.5e-4)) == lpr.IK_REACHED[name]
    plain = lpr.ik_reference(name, rob, st, with_profile=False)
    apart = np.abs(plain["state"] - out["state"]).max(axis=1)
    print("%s: without the profile %d of 24 reached, states apart by >= %.3g" % (name, (plain["error"] <= 1e-4).sum(), apart.min()))
    assert apart.min() >= lpr.IK_APART[name]
