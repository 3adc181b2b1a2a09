"""The loaded FK of a retraction robot solves a call's problems in backbone-length order (csrc/loaded_host.inc: shoot_run; the
`perm` of fk_loaded_retract, shoot_start_retract, shoot_finish and shoot_negative_start): every input row is read and every output
row written at the caller's index, so the results are the bits of the arrival-order solve.

An engine created under TENDON_HIP_LOADED_RETRACT_SORT=1 (every call ordered) against one created under =0 (never), on the 24-state
loaded-retraction fixtures with every special row (s_start >= L, one point, two points; a negative s_start is planted), both load
cases: fk_loaded_batch with the frames, fk_loaded_batch_retraction_dev, fk_loaded_tips, validate_loaded; again with chunks of 7 (the
order crosses four chunks), with per-state guess and load rows, and with one row for all (wrench_ld = 0).  loaded_order_last() says
that the ordering engaged on the first engine and not on the second."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.join(HERE, "golden")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import fk_truth_common as ftc                                        # noqa: E402
import loaded_ret_common as lrc                                      # noqa: E402
from loaded_edges_common import make_grid                            # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = ("config3_ret_edges", "config3_rot_ret")
KEYS = ("p", "R", "L", "L_i", "converged", "n_points", "vu0", "vuL", "residual", "iters", "num_fk_calls")
_cache = {}


def _engines(irt, name, chunk=None):
    """(fixture, states with a negative s_start planted in row 5, ordered engine, arrival-order engine)"""
    key = (name, chunk)
    if key not in _cache:
        fx = lrc.load(name)
        robot = ftc.robot_from_fixture(irt, fx)
        st = fx["states"].copy()
        st[5, -1] = -0.01
        engs = []
        for sort in ("1", "0"):
            env = dict(TENDON_HIP_LOADED_RETRACT_SORT=sort)
            if chunk:
                env["TENDON_HIP_SHOOT_CHUNK"] = str(chunk)
            with ftc.with_env(**env):
                eng = irt.Engine(robot, 0)
            eng.set_loaded_retraction()
            engs.append(eng)
        _cache[key] = (fx, st, engs[0], engs[1])
    return _cache[key]


def _same(a, b, keys=KEYS):
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    assert a["rounds"] == b["rounds"]


def _engaged(ordered, arrival, n):
    """n: the problems of the last shooting run (the host-array forms stage a call in chunks of the shooting's: the last chunk's)"""
    assert ordered.loaded_order_last() == dict(problems=n, ordered=n)
    assert arrival.loaded_order_last() == dict(problems=n, ordered=0)


def _last(n, chunk):
    return n if not chunk else (n % chunk or chunk)


@pytest.mark.parametrize("chunk", [None, 7])
@pytest.mark.parametrize("case", lrc.CASES)
@pytest.mark.parametrize("name", NAMES)
def test_the_order_does_not_change_a_bit(irt, name, case, chunk):
    fx, st, on, off = _engines(irt, name, chunk)
    n = len(st)
    d = lrc.dist_of(fx, case)
    kw = dict(wrench=fx["wrench_" + case], dist=d)
    a, b = on.fk_loaded_batch(st, want_R=True, **kw), off.fk_loaded_batch(st, want_R=True, **kw)
    _engaged(on, off, _last(n, chunk))
    _same(a, b)
    # the special rows are there, and the order has something to do
    assert not b["converged"][5] and b["n_points"][5] == 1 and b["converged"].sum() >= n - 2
    if name in ftc.NEW_RETRACTION:
        assert (st[:, -1] >= fx["consts"][0]).sum() == 2 and (b["n_points"] == 1).sum() >= 4 and (b["n_points"] == 2).any()
    assert len(set(b["n_points"])) >= 8 and (np.diff(st[:, -1]) < 0).any()
    # a per-state guess, per-state load rows
    g = b["vu0"] + 1e-4
    _same(on.fk_loaded_batch(st, want_R=True, guess=g, **kw), off.fk_loaded_batch(st, want_R=True, guess=g, **kw))
    # one row for all (wrench_ld = dist_ld = 0)
    one = dict(wrench=fx["wrench_" + case][3], dist=None if d is None else d[3])
    _same(on.fk_loaded_batch(st, **one), off.fk_loaded_batch(st, **one), keys=tuple(k for k in KEYS if k != "R"))
    # the tips (ordered per chunk of the workspace) and the validity of loaded shapes
    ta, tb = on.fk_loaded_tips(st, **kw), off.fk_loaded_tips(st, **kw)
    _engaged(on, off, _last(n, chunk))
    for k in ("tips", "converged", "vu0"):
        assert np.array_equal(ta[k], tb[k], equal_nan=True), k
    assert np.array_equal(tb["tips"], b["p"][np.arange(n), b["n_points"] - 1])


@pytest.mark.parametrize("chunk", [None, 7])
@pytest.mark.parametrize("name", NAMES)
def test_device_form_and_validity(irt, name, chunk):
    """The device forms hand the whole call to one shooting run: with chunks of 7 the order of the 24 problems crosses four chunks."""
    import torch
    fx, st, on, off = _engines(irt, name, chunk)
    n, P, Nt, ld, dev = len(st), on.num_points, on.n_tendons, 64, "cuda:0"
    w, d = fx["wrench_D"], fx["dist_D"]
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    res = []
    for eng in (on, off):
        planes = torch.full((3, P, ld), float("nan"), dtype=torch.float64, device=dev)
        Li, home = (torch.full((Nt, ld), float("nan"), dtype=torch.float64, device=dev) for _ in range(2))
        npts, conv = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev)
        vu0, vuL = (torch.zeros((n, 6), dtype=torch.float64, device=dev) for _ in range(2))
        eng.fk_loaded_batch_retraction_dev(up(st), n, ld, planes[0], planes[1], planes[2], Li, conv, npts, home, d_wrench=up(w), d_dist=up(d),
                                           d_vu0=vu0, d_vuL=vuL)
        torch.cuda.synchronize()
        res.append([t.cpu().numpy() for t in (planes, Li, home, npts, conv, vu0, vuL)])
    _engaged(on, off, n)
    for x, y in zip(*res):
        assert np.array_equal(x, y, equal_nan=True)
    assert np.isnan(res[1][0][:, :, n:]).all() and np.isnan(res[0][0][:, :, n:]).all()       # nothing written past the call's columns
    vox = make_grid(irt, float(fx["consts"][1]), 7, 40, 0.03)             # (the finest grid the backbone checker takes for the robot's dL)
    for eng in (on, off):
        eng.set_grid(vox.Nx(), vox.limits(), vox.blocks)
    va, vb = on.validate_loaded(st, wrench=w, dist=d), off.validate_loaded(st, wrench=w, dist=d)
    _engaged(on, off, n)
    assert np.array_equal(va["valid"], vb["valid"]) and np.array_equal(va["flags"], vb["flags"])
    assert va["valid"].any() and not va["valid"].all()


def test_a_threshold_above_the_call_keeps_arrival_order(irt):
    fx = lrc.load("config3_ret_edges")
    robot = ftc.robot_from_fixture(irt, fx)
    with ftc.with_env(TENDON_HIP_LOADED_RETRACT_SORT="25"):
        eng = irt.Engine(robot, 0)
    eng.set_loaded_retraction()
    eng.fk_loaded_batch(fx["states"])
    assert eng.loaded_order_last() == dict(problems=24, ordered=0)
    eng.fk_loaded_batch(np.vstack([fx["states"], fx["states"][:1]]))
    assert eng.loaded_order_last() == dict(problems=25, ordered=25)
    eng.close()
