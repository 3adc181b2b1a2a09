"""The loaded FK on the device (tr_fk_loaded_batch*, csrc/fk_loaded_kernel.hpp) against the numpy reference and its fixtures
(tests/loaded_fk_reference.py, tests/golden/loaded_fk_<name>.npz, written by tests/golden/make_loaded_fk.py).

Tolerances: 1e-9 m is the project's interface tolerance (device points against a CPU integration from the SAME base strains);
bound_i of the fixtures is the displacement a solution may have whose tip wrench misses by residual_threshold (see the generator);
1 % of residual_threshold separates the two arithmetics' residuals: stiffness <= 7e2 N times a 1e-13 strain difference is 1e-10 N,
two orders below 5e-8 N.

Load cases (make_loaded_fk.py): A one wrench, B gravity, C gravity and a wrench per state, D case C plus a distributed force of any
direction (0.3 .. 1 N/m, with a z component) and a distributed moment l_e (0.003 .. 0.01 N) per state -- the one case in which all
twelve load numbers are non-zero.  The integration itself is held to ~1e-13 m in tests/test_gpu_loaded_fk_truth.py; the checks here
stay beside it."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.join(HERE, "golden")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import loaded_fk_reference as ref                                    # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = ("config1", "n1", "n8", "config3_rot", "n5", "n6")          # n5, n6: fk_loaded_uniform<5>, <6>, the widest at two waves
CASES = ("A", "B", "C", "D")
KEYS = ("p", "L", "L_i", "vu0", "vuL", "residual", "iters", "num_fk_calls", "converged")


@pytest.fixture(scope="module")
def gen(orc):
    import make_loaded_fk
    return make_loaded_fk


@pytest.fixture(scope="module")
def world(gen, irt):
    """name -> (robot, oracle robot, fixture arrays, engine), built on first use"""
    cache = {}

    def get(name):
        if name not in cache:
            robot, rob, st = gen.fixture(name)
            fx = dict(np.load(gen.path(name)))
            assert np.array_equal(st, fx["states"])
            cache[name] = (robot, rob, fx, robot.engine(0))
        return cache[name]
    return get


@pytest.fixture(scope="module")
def solved(world):
    """(name, case) -> the device's result for the fixture's 24 states, computed once"""
    cache = {}

    def get(name, case):
        if (name, case) not in cache:
            _, _, fx, eng = world(name)
            cache[name, case] = eng.fk_loaded_batch(fx["states"], wrench=fx["wrench_" + case], dist=fx["dist_" + case], want_R=True)
        return cache[name, case]
    return get


def _same(a, b, rows_a=slice(None), rows_b=slice(None)):
    for k in KEYS:
        assert np.array_equal(a[k][rows_a], b[k][rows_b], equal_nan=True), k


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("name", NAMES)
def test_it_is_a_solution(world, solved, name, case):
    robot, rob, fx, _ = world(name)
    out = solved(name, case)
    thr = robot.residual_threshold
    assert out["converged"].all(), np.nonzero(~out["converged"])[0]
    w, d = fx["wrench_" + case], fx["dist_" + case]
    cpu = ref.evaluate(rob, fx["states"], out["vu0"], F_e=w[:, :3], L_e=w[:, 3:], f_e=d[:, :3], l_e=d[:, 3:])
    e = np.linalg.norm(cpu["e"], axis=1)
    figures = (np.abs(out["p"] - cpu["p"]).max(), np.abs(out["L"] - cpu["L"]).max(), np.abs(out["L_i"] - cpu["L_i"]).max(), e.max() / thr,
               np.abs(out["residual"] - e).max() / thr)
    print("%s %s: points %.3g m, L %.3g m, L_i %.3g m, |e| %.4f thr, residual_out off by %.3g thr; iters <= %d, rounds %d"
          % ((name, case) + figures + (out["iters"].max(), out["rounds"])))
    assert figures[0] <= 1e-9 and figures[1] <= 1e-9 and figures[2] <= 1e-9
    assert (e <= 1.01 * thr).all()
    assert (np.abs(out["residual"] - e) <= 0.01 * thr).all()
    assert (out["num_fk_calls"] == 1 + 13 * (out["rounds"] - 1)).any() and (out["num_fk_calls"] % 13 == 1).all()


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("name", NAMES)
def test_it_is_the_solution(world, solved, name, case):
    _, _, fx, _ = world(name)
    out = solved(name, case)
    bound = fx["bound_" + case]
    err = np.linalg.norm(out["p"] - fx["p_" + case], axis=2).max(axis=1)
    Rtip = out["R"][:, -1].reshape(-1, 3, 3).transpose(0, 2, 1)                 # column-major storage
    errR = np.abs(Rtip - fx["R_tip_" + case]).reshape(len(err), -1).max(axis=1)
    print("%s %s: points %.3g of bound (bound <= %.3g m), tip frame %.3g of bound / dL"
          % (name, case, (err / bound).max(), bound.max(), (errR / (bound / float(fx["dL"]))).max()))
    assert (err <= bound).all()
    assert (errR <= bound / float(fx["dL"])).all()


@pytest.mark.parametrize("name", NAMES)
def test_zero_load_is_the_unloaded_shape_without_an_iteration(world, name):
    _, _, fx, eng = world(name)
    un = eng.fk_batch(fx["states"])
    out = eng.fk_loaded_batch(fx["states"])
    conv = un["converged"]
    assert conv.sum() >= 20
    print("%s: %.3g m" % (name, np.abs(out["p"] - un["p"]).max()))
    assert np.abs(out["p"] - un["p"]).max() <= 1e-9
    assert (out["iters"][conv] == 0).all() and (out["num_fk_calls"][conv] == 1).all()
    assert out["converged"][conv].all()


@pytest.fixture(scope="module")
def config1_C(world, solved):
    _, _, fx, _ = world("config1")
    return fx["states"], fx["wrench_C"], fx["dist_C"], solved("config1", "C")


def test_shapes_of_the_launch_do_not_change_a_bit(world, config1_C, irt, monkeypatch):
    """13 lanes; 65 lanes (problem 4 lies across two waves); all 24; reversed; 300 problems in chunks of 7 and in one chunk"""
    robot, _, _, eng = world("config1")
    st, w, d, full = config1_C
    for n in (1, 5):
        _same(eng.fk_loaded_batch(st[:n], wrench=w[:n], dist=d[:n]), full, rows_b=slice(0, n))
    _same(eng.fk_loaded_batch(st[::-1], wrench=w[::-1], dist=d[::-1]), full, rows_b=slice(None, None, -1))
    idx = np.arange(300) % 24
    monkeypatch.setenv("TENDON_HIP_SHOOT_CHUNK", "7")
    chunked = irt.Engine(robot, 0)
    monkeypatch.delenv("TENDON_HIP_SHOOT_CHUNK")
    a = chunked.fk_loaded_batch(st[idx], wrench=w[idx], dist=d[idx])
    chunked.close()
    b = eng.fk_loaded_batch(st[idx], wrench=w[idx], dist=d[idx])
    assert a["rounds"] > b["rounds"]
    _same(a, full, rows_b=idx)
    _same(b, full, rows_b=idx)


def test_straight_rod_guess_reaches_the_same_shape(world, solved):
    robot, _, fx, eng = world("config1")
    st = fx["states"]
    straight = np.tile([0.0, 0.0, 1.0, 0.0, 0.0, 0.0], (len(st), 1))
    # cases A, B, C: under case D's distributed moment three of the taut states do not reach the threshold from the straight rod in 100
    # LM iterations (CHANGELOG, round 20) -- a limit of the LM iteration from a far start, not of the integration under test here
    for case in ("A", "B", "C"):
        out = eng.fk_loaded_batch(st, wrench=fx["wrench_" + case], dist=fx["dist_" + case], guess=straight)
        err = np.linalg.norm(out["p"] - fx["p_" + case], axis=2).max(axis=1)
        print("case %s: %.3g of 2 bound, iters <= %d" % (case, (err / (2 * fx["bound_" + case])).max(), out["iters"].max()))
        assert out["converged"].all()
        assert (err <= 2 * fx["bound_" + case]).all()
    one = eng.fk_loaded_batch(st, wrench=fx["wrench_A"], dist=fx["dist_A"], guess=straight, max_iters=1)
    assert not one["converged"].any()
    assert (one["iters"] == 1).all()


def test_a_hopeless_problem_does_not_touch_the_others(world, config1_C):
    _, _, _, eng = world("config1")
    st, w, d, full = config1_C
    w = w.copy()
    w[11] = [1e6, 0.0, 0.0, 0.0, 0.0, 0.0]
    out = eng.fk_loaded_batch(st, wrench=w, dist=d)                  # returns: no stop is an error of the call
    assert not out["converged"][11]
    keep = np.arange(24) != 11
    _same(out, full, keep, keep)


def test_gravity_moves_the_verdicts(world, orc):
    """config3_rot under its own weight: a sphere on the loaded tip stops the loaded robot and not the unloaded one, a sphere on
    the unloaded tip the reverse (the generator checked 2 voxels of clearance on the oracle grid)"""
    _, _, fx, eng = world("config3_rot")
    N, half = int(fx["verdict_grid"][0]), float(fx["verdict_grid"][1])
    lim = (-half, half) * 3
    for k, i in enumerate(fx["verdict_states"]):
        st, dist = fx["states"][i:i + 1], fx["dist_B"][i:i + 1]
        for sphere, loaded_valid in ((fx["verdict_sphere_loaded"][k], False), (fx["verdict_sphere_unloaded"][k], True)):
            g = orc.Grid(N, lim)
            g.add_sphere(sphere[:3], sphere[3])
            eng.set_grid(N, lim, g.blocks())
            assert bool(eng.validate_loaded(st, dist=dist)["valid"][0]) == loaded_valid
            assert bool(eng.validate_batch(st)["valid"][0]) == (not loaded_valid)


def test_device_form_feeds_validate_shapes(world, orc, irt):
    import torch
    _, _, fx, eng = world("config3_rot")
    N, half = int(fx["verdict_grid"][0]), float(fx["verdict_grid"][1])
    lim = (-half, half) * 3
    g = orc.Grid(N, lim)
    for s in fx["verdict_sphere_loaded"]:
        g.add_sphere(s[:3], s[3])
    eng.set_grid(N, lim, g.blocks())
    st, dist = fx["states"], fx["dist_B"]
    n, P, ld = len(st), eng.num_points, 64
    want = eng.validate_loaded(st, dist=dist)
    assert not want["valid"][fx["verdict_states"]].any() and want["valid"].any()
    dev = "cuda:0"
    planes = torch.empty((3, P, ld), dtype=torch.float64, device=dev)
    Li = torch.empty((eng.n_tendons, ld), dtype=torch.float64, device=dev)
    conv = torch.empty(n, dtype=torch.uint8, device=dev)
    vu0 = torch.empty((n, 6), dtype=torch.float64, device=dev)
    bits = torch.zeros(1, dtype=torch.int64, device=dev)
    flags = torch.zeros(n, dtype=torch.uint8, device=dev)
    eng.fk_loaded_batch_dev(torch.from_numpy(st).to(dev), n, ld, planes[0], planes[1], planes[2], d_dist=torch.from_numpy(dist).to(dev),
                            d_Li=Li, d_conv=conv, d_vu0=vu0)
    eng.validate_shapes_dev(n, ld, planes[0], planes[1], planes[2], Li, conv, bits, flags)
    torch.cuda.synchronize()
    assert np.array_equal(bits.cpu().numpy().view(np.uint64), want["bits"])
    assert np.array_equal(flags.cpu().numpy(), want["flags"])
    host = eng.fk_loaded_batch(st, dist=dist)
    assert np.array_equal(vu0.cpu().numpy(), host["vu0"])
    assert np.array_equal(planes[:, :, :n].cpu().numpy().transpose(2, 1, 0), host["p"])


def test_errors(world, irt):
    import ctypes as C
    robot, _, fx, eng = world("config1")
    ret = irt.workloads.robot_config1()
    ret.enable_retraction = True
    with pytest.raises(irt.Unsupported):
        irt.Engine(ret, 0).fk_loaded_batch(np.zeros((2, 4)))
    st = np.ascontiguousarray(fx["states"][:2])
    w = np.zeros((2, 6))
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    rc = eng.lib.tr_fk_loaded_batch(eng._ctx, None, dp(st), 2, dp(w), 5, None, 0, None, None, None, None, None, None, None, None, None, None,
                                    None, None, None)
    assert rc == irt._lib.TR_ERR_INVALID_ARG
    with pytest.raises(irt.InvalidArgument):
        eng.fk_loaded_batch(st, wrench=np.zeros((3, 6)))
