"""The loaded tip Jacobian and tip compliance on the device (tr_tip_jacobian_loaded*, csrc/loaded_jacobian_host.inc,
csrc/loaded_sens_kernel.hpp) against the 40-digit truth of the linearisation's lanes (tests/golden/loaded_lin_truth_<name>.npz),
the numpy specification (tests/loaded_jacobian_reference.py) and recorded differenced solves
(tests/golden/loaded_jacobian_fd_<name>.npz).

The C ABI takes one load set per call; case C's and D's rows differ per state, so those states are solved one per call.
Tolerances: the blocks are held to the truth's difference bounds (make_loaded_lin_truth.truth_blocks); everything else to 4 x what
tests/test_loaded_jacobian_reference.py measured on the reference alone (END_TO_END, REDUCTION, ZERO_LOAD there).

Of W and J nothing is observable through ik_loaded_batch: with max_iters = 0 it returns the Newton-corrected tip and strains of its
first linearisation (x_c, y_c) and keeps W and J to itself.  So the clause `W and J bit for bit the IK's` is held through x_c and
y_c, which come out of the same LU and solves: they equal tips and vu0 of this call bit for bit."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.join(HERE, "golden")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import fk_truth_common as ftc                                        # noqa: E402
import loaded_jacobian_reference as ljr                              # noqa: E402
import make_loaded_jacobian_fd as mfd                                # noqa: E402
import make_loaded_lin_truth as mlt                                  # noqa: E402
import test_loaded_jacobian_reference as cpu                         # noqa: E402  (the measured tolerances)

pytestmark = pytest.mark.gpu

ARRAYS = ("J", "tips", "vu0", "compliance", "W")
BLOCKS = ("y", "x", "e", "J_y", "J_p", "X_y", "X_p")
ALL = ("compliance", "W", "blocks")


@pytest.fixture(scope="module")
def gen(orc):
    import make_loaded_fk
    return make_loaded_fk


@pytest.fixture(scope="module")
def world(gen, irt):
    """name -> (robot, oracle robot, loaded-FK fixture arrays, engine), built on first use"""
    cache = {}

    def get(name):
        if name not in cache:
            robot, rob, st = gen.fixture(name)
            fx = dict(np.load(gen.path(name)))
            assert np.array_equal(st, fx["states"])
            cache[name] = (robot, rob, fx, robot.engine(0))
        return cache[name]
    return get


def per_state(eng, st, w, d, frame, guess=None, **kw):
    """tip_jacobian_loaded with one call per state: (n, 6) load rows that differ per state"""
    outs = [eng.tip_jacobian_loaded(st[i:i + 1], wrench=w[i], dist=d[i], frame=frame, guess=None if guess is None else guess[i:i + 1],
                                    want=ALL, **kw) for i in range(len(st))]
    out = {k: np.concatenate([o[k] for o in outs]) for k in ARRAYS + ("equilibrium", "n_integrations")}
    out["blocks"] = {k: np.concatenate([o["blocks"][k] for o in outs]) for k in BLOCKS}
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_same(a, b, keys=ARRAYS + ("equilibrium", "n_integrations")):
    for k in keys:
        assert same_bits(a[k], b[k]), k
    if "blocks" in a and "blocks" in b:
        for k in BLOCKS:
            assert same_bits(a["blocks"][k], b["blocks"][k]), k


@pytest.fixture(scope="module")
def at_truth(world):
    """name -> (truth fixture, the device's linearisation exactly at the fixture's strains), computed once"""
    cache = {}

    def get(name):
        if name not in cache:
            _, _, _, eng = world(name)
            lt = mlt.load(name)
            cache[name] = (lt, per_state(eng, lt["states"], lt["wrench"], lt["dist"], mlt.NAMES[name], guess=lt["vu0"], max_iters=0,
                                         delta=float(lt["delta"]), finite_difference_delta=float(lt["delta_y"])))
        return cache[name]
    return get


@pytest.mark.parametrize("name", list(mlt.NAMES))
def test_blocks_lie_within_the_truths_difference_bounds(world, at_truth, name):
    lt, out = at_truth(name)
    n, S = lt["states"].shape
    assert out["equilibrium"].all()
    assert same_bits(out["blocks"]["y"], lt["vu0"])
    assert (out["n_integrations"] == 1 + 13 + 2 * S).all()
    tb = mlt.truth_blocks(lt)
    worst = 0.0
    for key in ("J_y", "J_p", "X_y", "X_p", "x", "e"):
        want, bound = tb[key]
        ratio = np.abs(out["blocks"][key] - want) / bound
        worst = max(worst, float(ratio.max()))
        assert (ratio <= 1.0).all(), (name, key, float(ratio.max()))
    print("%s: worst error / bound of the device's blocks %.3f" % (name, worst))


@pytest.mark.parametrize("name", list(mlt.NAMES))
def test_reduction_of_the_devices_own_blocks(world, at_truth, name):
    robot, rob, _, eng = world(name)
    lt, out = at_truth(name)
    b = out["blocks"]
    T = ljr.wrench_turn(rob, lt["states"], mlt.NAMES[name])
    want = ljr.reduce_blocks(b["y"], b["x"], b["e"], b["J_y"], b["J_p"], b["X_y"], b["X_p"], T)
    got = dict(W=out["W"], J=out["J"], C=out["compliance"], y_c=out["vu0"], x_c=out["tips"])
    eps = np.finfo(float).eps
    for i in range(len(lt["states"])):
        kappa = np.linalg.cond(b["J_y"][i], np.inf)
        for k in got:
            tol = cpu.FACTOR * cpu.REDUCTION * kappa * eps * np.abs(want[k][i]).max()
            assert np.abs(got[k][i] - want[k][i]).max() <= tol, (name, i, k, np.abs(got[k][i] - want[k][i]).max(), tol)
    # what the loaded IK leaves observable of the same linearisation: its Newton-corrected tip and strains, bit for bit
    for i in range(len(lt["states"])):
        ik = eng.ik_loaded_batch(lt["states"][i:i + 1], np.zeros(3), wrench=lt["wrench"][i], dist=lt["dist"][i], frame=mlt.NAMES[name],
                                 guess=lt["vu0"][i:i + 1], max_iters=0, shoot_max_iters=0, shoot_stop_threshold_Dp=1e-4)
        assert ik["equilibrium"].all()
        assert same_bits(ik["tip"], out["tips"][i:i + 1]) and same_bits(ik["vu0"], out["vu0"][i:i + 1])


@pytest.mark.parametrize("name", list(mfd.NAMES))
def test_cold_start_against_differenced_solves(world, name):
    robot, rob, fx, eng = world(name)
    fd = mfd.load(name)
    st = fx["states"]
    frame = mlt.NAMES[name]
    tol = cpu.END_TO_END[name]
    for case in mfd.CASES:
        w, d = fd["wrench_" + case], fd["dist_" + case]
        if (w == w[0]).all() and (d == d[0]).all():
            out = eng.tip_jacobian_loaded(st, wrench=w[0], dist=d[0], frame=frame, want=("compliance",))
        else:
            out = per_state(eng, st, w, d, frame)
        assert out["equilibrium"].all(), (name, case)
        tip_gap = np.abs(out["tips"] - fx["p_" + case][:, -1]).max()
        gJ, gC = ljr.relative_gap(out["J"], fd["J_" + case]), ljr.relative_gap(out["compliance"], fd["C_" + case])
        print("%s %s: tips within %.3g m; J %.3g (tolerance %.3g), C %.3g (%.3g)"
              % (name, case, tip_gap, gJ.max(), cpu.FACTOR * tol["J"], gC.max(), cpu.FACTOR * tol["C"]))
        assert tip_gap <= 1e-9
        assert (gJ <= cpu.FACTOR * tol["J"]).all() and (gC <= cpu.FACTOR * tol["C"]).all()


@pytest.mark.parametrize("name", list(cpu.ZERO_LOAD))
def test_zero_load_is_the_unloaded_jacobian(world, name):
    """All 24 states.  At the state of zero tensions the central differences of Engine.tip_jacobian straddle tau = 0, where the
    unloaded FK changes branch (config1: the straight rod on both sides, J exactly zero; config3_rot: tension columns a tenth of
    the rod's); the rod integration has no such branch, so that row is held to the numpy helper at the device's own strains instead
    (the same tolerance)."""
    _, rob, fx, eng = world(name)
    st = fx["states"]
    N = rob.n_tendons
    out = eng.tip_jacobian_loaded(st, want=("compliance", "blocks"))
    assert out["equilibrium"].all() and np.isfinite(out["compliance"]).all()
    want = eng.tip_jacobian(st)
    flat = ~st[:, :N].any(axis=1)
    assert flat.sum() <= 1
    if flat.any():
        want[flat] = ljr.sensitivities(rob, st[flat], out["blocks"]["y"][flat])["J"]
    gap = ljr.relative_gap(out["J"], want)
    print("%s: zero load against tip_jacobian %.3g (tolerance %.3g)" % (name, gap.max(), cpu.FACTOR * cpu.ZERO_LOAD[name]))
    assert (gap <= cpu.FACTOR * cpu.ZERO_LOAD[name]).all()


def test_results_do_not_depend_on_batch_order_or_chunking(world, gen):
    robot, rob, fx, eng = world("config3_rot")
    st = np.ascontiguousarray(np.tile(fx["states"], (3, 1))[:65])
    N = len(robot.tendons)
    # one set for the whole batch: state 0's case D rows as a world-frame set
    w = mlt.world_set(fx["wrench_D"][:1], fx["states"][:1, N])[0]
    d = mlt.world_set(fx["dist_D"][:1], fx["states"][:1, N])[0]
    run = lambda e, s: e.tip_jacobian_loaded(s, wrench=w, dist=d, frame="world", want=ALL)
    whole = run(eng, st)
    assert whole["equilibrium"].all()
    rows = lambda out, sel: {k: ({q: a[sel] for q, a in v.items()} if k == "blocks" else v[sel]) for k, v in out.items() if k != "rounds"}
    assert_same(rows(whole, slice(0, 24)), rows(whole, slice(24, 48)))   # the tiles repeat
    with ftc.with_env(TENDON_HIP_SHOOT_CHUNK=7):
        chunked = run(gen.fixture("config3_rot")[0].engine(0), st)
    assert_same(whole, chunked)
    assert_same(whole, rows(run(eng, np.ascontiguousarray(st[::-1])), slice(None, None, -1)))
    for i in range(3):
        assert_same(rows(whole, slice(i, i + 1)), run(eng, st[i:i + 1]))


def test_device_form_on_a_stream_equals_the_host_form(world):
    import torch
    robot, rob, fx, eng = world("config3_rot")
    st = fx["states"]
    n, S = st.shape
    N = len(robot.tendons)
    w = mlt.world_set(fx["wrench_D"][:1], st[:1, N])[0]
    d = mlt.world_set(fx["dist_D"][:1], st[:1, N])[0]
    host = eng.tip_jacobian_loaded(st, wrench=w, dist=d, frame="world")
    d_st = torch.from_numpy(st).cuda()
    d_J = torch.empty(n * 3 * S, dtype=torch.float64, device="cuda")
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        rounds = eng.tip_jacobian_loaded_dev(d_st, n, d_J=d_J, wrench=w, dist=d, frame="world", stream=stream)
    stream.synchronize()
    assert rounds == host["rounds"]
    assert same_bits(d_J.cpu().numpy().reshape(n, 3, S), host["J"])


def test_unconverged_state_is_nan_and_leaves_the_others_alone(world):
    robot, rob, fx, eng = world("config1")
    st = np.ascontiguousarray(fx["states"][:4])
    w, d = fx["wrench_D"][1], fx["dist_D"][1]                           # config1: frame BASE, one set for the call
    good = eng.tip_jacobian_loaded(st, wrench=w, dist=d)
    assert good["equilibrium"].all()
    # from the Newton-corrected strains every state is at the threshold at once; from the straight rod one LM iteration is not enough
    ref1 = eng.tip_jacobian_loaded(st, wrench=w, dist=d, want=ALL, guess=good["vu0"], max_iters=1)
    assert ref1["equilibrium"].all()
    guess = good["vu0"].copy()
    guess[1] = (0, 0, 1, 0, 0, 0)
    out = eng.tip_jacobian_loaded(st, wrench=w, dist=d, want=ALL, guess=guess, max_iters=1)
    assert list(out["equilibrium"]) == [True, False, True, True]
    assert same_bits(out["n_integrations"][[0, 2, 3]], ref1["n_integrations"][[0, 2, 3]])
    for k in ARRAYS:
        assert np.isnan(out[k][1]).all(), k
        keep = [0, 2, 3]
        assert same_bits(out[k][keep], ref1[k][keep]), k
    for k in BLOCKS:
        assert np.isnan(out["blocks"][k][1]).all(), k
        assert same_bits(out["blocks"][k][[0, 2, 3]], ref1["blocks"][k][[0, 2, 3]]), k


def test_resolved_rate_update_is_one_lm_iteration(irt, world):
    """damped_resolved_rate_update_batch_device against the Python paths of one LM iteration with mu_init = lambda and all stop
    thresholds at 1e-9: tip_control.inverse_kinematics_batch (unloaded), loaded_ik_reference.inverse_kinematics_loaded_batch from
    the same start strains (case C, whose rows differ per state: one call per state).  States agree within test_gpu_loaded_ik.py's
    1e-6 (1 + |state|)."""
    import loaded_ik_reference as ikr
    T = irt.tip_control
    robot, rob, fx, eng = world("config3_rot")
    st = np.ascontiguousarray(fx["states"][:8])
    v = np.array([1e-3, -5e-4, 3e-4])
    lm = dict(max_iters=1, mu_init=0.1, stop_threshold_JT_err_inf=1e-9, stop_threshold_Dp=1e-9, stop_threshold_err=1e-9)
    close = lambda a, b: (np.abs(a - b) <= 1e-6 * (1 + np.abs(b))).all()
    # unloaded
    tips, _ = eng.fk_tips(st)
    nxt = T.damped_resolved_rate_update_batch_device(robot, st, v)
    want = T.inverse_kinematics_batch(robot, st, tips + v, **lm)["state"]
    assert close(nxt, want)
    assert same_bits(T.damped_resolved_rate_update_device(robot, st[2], v), nxt[2])
    moved = (nxt != st).any(axis=1)
    new_tips, _ = eng.fk_tips(nxt)
    assert moved.any()
    assert (np.linalg.norm(new_tips - (tips + v), axis=1)[moved] < np.linalg.norm(v)).all()
    # under case C
    w, d = fx["wrench_C"][:8], fx["dist_C"][:8]
    moved = 0
    for i in range(len(st)):
        start = eng.fk_loaded_batch(st[i:i + 1], wrench=w[i], dist=d[i])
        tip = start["p"][0, start["n_points"][0] - 1]
        nxt = T.damped_resolved_rate_update_batch_device(robot, st[i:i + 1], v, wrench=w[i], dist=d[i])
        want = ikr.inverse_kinematics_loaded_batch(rob, st[i:i + 1], tip + v, wrench=w[i], dist=d[i], guess=start["vu0"], **lm)
        assert close(nxt, want["state"]), (i, nxt, want["state"])
        if (nxt != st[i]).any():
            moved += 1
            new = eng.fk_loaded_batch(nxt, wrench=w[i], dist=d[i])
            assert np.linalg.norm(new["p"][0, new["n_points"][0] - 1] - (tip + v)) < np.linalg.norm(v), i
    assert moved > 0


def test_errors_and_the_c_abi(irt, world):
    L = irt._lib
    robot, rob, fx, eng = world("config1")
    st = np.ascontiguousarray(fx["states"][:2])
    ret = ftc.robot_from_fixture(irt, ftc.load("config3_rot_ret"))
    ret_st = ftc.load("config3_rot_ret")["states"][:2]
    with pytest.raises(irt.Unsupported) as a:
        ret.engine(0).tip_jacobian_loaded(ret_st)
    with pytest.raises(irt.Unsupported) as b:
        ret.engine(0).fk_loaded_batch(ret_st)
    assert str(a.value) == str(b.value)
    with pytest.raises(irt.InvalidArgument):
        eng.tip_jacobian_loaded(st, frame="tool")
    with pytest.raises(irt.InvalidArgument):
        eng.tip_jacobian_loaded(st, delta=0.0)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    ld = L.TrEdgeLoads()
    ld.frame = 2
    J = np.empty((2, 3, st.shape[1]))
    tail = (None, None, None, None, None, None, None)
    call = lambda loads, states, n, delta: eng.lib.tr_tip_jacobian_loaded(eng._ctx, None, loads, states, n, delta, None, None, dp(J), *tail)
    assert call(C.byref(ld), dp(st), 2, 1e-6) == L.TR_ERR_INVALID_ARG
    assert call(None, None, 2, 1e-6) == L.TR_ERR_INVALID_ARG
    assert call(None, dp(st), 2, 1e-6) == L.TR_OK                       # null loads: no load
    assert same_bits(J, eng.tip_jacobian_loaded(st)["J"])
    # n = 0 on a context on which nothing else was ever asked for
    new = ftc.robot_from_fixture(irt, ftc.load("config1"))
    e2 = new.engine(0)
    assert e2.lib.tr_tip_jacobian_loaded(e2._ctx, None, None, None, 0, 1e-6, None, None, None, *tail) == L.TR_OK
