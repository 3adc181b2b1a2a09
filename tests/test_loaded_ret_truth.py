"""The fixtures of the loaded rod with retraction (tests/golden/loaded_ret_truth_<name>.npz, make_loaded_ret_truth.py) against the numpy
reference that the device tests lean on (tests/loaded_ret_reference.py), without a GPU:

  - the reference lies within the fixtures' bounds on every row and case (the bounds are fk_truth_common.loaded_bounds);
  - three planted faults are each outside them on at least one row of EVERY fixture, shown by running the reference with the fault: a
    load term off by 1 + 1e-8, the load rotated with the previous stage's frame, the first interval integrated with the shared
    table's routing instead of the state's own abscissae -- so a kernel with one of them cannot pass tests/test_gpu_loaded_retraction.py;
  - at zero load and from (v0, u0) of the UNLOADED truth the reference meets fk_truth_common.compare: the two fixture families agree
    on what a retraction robot's integration is.
Rows 12 and 13 of the dL = L / 40 fixtures (s_start >= L) integrate nothing and have no truth; they are the only rows left out."""
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
import loaded_ret_reference as ref                                   # noqa: E402


@pytest.fixture(scope="module")
def world(orc, irt):
    """name -> (oracle robot, fixture), built on first use"""
    import make_fk_truth as mft
    cache = {}

    def get(name):
        if name not in cache:
            fx = lrc.load(name)
            cache[name] = (mft.oracle_robot(ftc.robot_from_fixture(irt, fx)), fx)
        return cache[name]
    return get


def _ratios(rob, fx, case, fault=None):
    w, d = fx["wrench_" + case], fx["dist_" + case]
    ev = ref.evaluate(rob, fx["states"], fx["vu0_" + case], F_e=w[:, :3], L_e=w[:, 3:], f_e=d[:, :3], l_e=d[:, 3:], fault=fault)
    assert np.array_equal(ev["n_points"], fx["n_points"])
    errs = lrc.errors(fx, case, ev["p"], lrc.tip_frames(ev["R"], ev["n_points"]), ev["L"], ev["L_i"], ev["vuL"], ev["e"])
    return lrc.ratios(fx, case, errs)


def test_the_rows_without_a_truth_are_the_ones_known_in_advance():
    for name in lrc.NAMES:
        fx = lrc.load(name)
        assert list(fx["no_truth"]) == ([] if name == "config3_rot_ret" else [12, 13])
        L = fx["consts"][0]
        assert np.array_equal(np.flatnonzero(fx["states"][:, -1] >= L), fx["no_truth"])
        for case in lrc.CASES:
            assert (fx["dist_" + case] != 0).all() == (case == "D") and (fx["wrench_" + case] != 0).all()
            assert not fx["dist_A"].any()


@pytest.mark.parametrize("case", lrc.CASES)
@pytest.mark.parametrize("name", lrc.NAMES)
def test_the_reference_lies_within_the_bounds(world, name, case):
    rob, fx = world(name)
    r = _ratios(rob, fx, case)
    print("%s %s: worst error / bound %.3f" % (name, case, r.max()))
    assert (r <= 1.0).all(), np.argwhere(r > 1.0)


@pytest.mark.parametrize("fault", ref.FAULTS)
@pytest.mark.parametrize("name", lrc.NAMES)
def test_a_planted_fault_is_outside_the_bounds(world, name, fault):
    rob, fx = world(name)
    r = _ratios(rob, fx, "D", fault)                    # case D: the one with a distributed load to get wrong
    print("%s %s: worst error / bound %.3g on row %d" % (name, fault, r.max(), r.max(axis=1).argmax()))
    assert r.max() > 1.0


@pytest.mark.parametrize("name", lrc.NAMES)
def test_zero_load_meets_the_unloaded_truth(world, name):
    rob, _ = world(name)
    un = ftc.load(name)
    ev = ref.evaluate(rob, un["states"], np.hstack([un["v0"], un["u0"]]))
    assert np.array_equal(ev["n_points"], un["n_points"])
    worst, ok = ftc.compare(un, ev["p"], lrc.tip_frames(ev["R"], ev["n_points"]), ev["L"], ev["L_i"])
    print("%s: worst error / bound %.3f" % (name, worst))
    assert ok.all(), np.flatnonzero(~ok)
