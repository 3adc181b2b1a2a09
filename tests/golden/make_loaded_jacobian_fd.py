#!/usr/bin/env python3
"""Generates tests/golden/loaded_jacobian_fd_<name>.npz: the loaded tip Jacobian dx/dp and the tip compliance dx/dw of the 24
states of config1 (frame BASE), config3_rot and n8 (frame WORLD) under the load cases A, C, D of loaded_fk_<name>.npz, by central
differences of shooting solves taken to 1e-12 N (tests/loaded_jacobian_reference.differenced_solves): 2 S + 13 solves per state in
plain numpy, minutes per robot -- recorded so that the device test reads them.

    python tests/golden/make_loaded_jacobian_fd.py [name ...]

The call's one load set of a state is the fixture's rows (BASE), or those rows turned by Rz(theta) in fp64 (WORLD;
make_loaded_lin_truth.world_set), as in loaded_lin_truth_<name>.npz.  Per case X: wrench_X, dist_X (24, 6) the set of every state,
y_X (24, 6) the equilibrium's strains, tip_X (24, 3), J_X (24, 3, S), C_X (24, 3, 6).  The generator fails if a solve misses 1e-12 N.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
for _p in (ROOT, TESTS, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import loaded_jacobian_reference as ljr                              # noqa: E402
import make_loaded_lin_truth as mlt                                  # noqa: E402

NAMES = ("config1", "config3_rot", "n8")
CASES = ("A", "C", "D")


def path(name):
    return os.path.join(HERE, "loaded_jacobian_fd_%s.npz" % name)


def load(name):
    with np.load(path(name)) as d:
        return {k: d[k] for k in d.files}


def call_sets(name, lf, st, case, n_tendons):
    """(wrench (n, 6), dist (n, 6), frame): the call's load set of every state"""
    frame = mlt.NAMES[name]
    w, d = lf["wrench_" + case], lf["dist_" + case]
    if frame == "world":
        w, d = mlt.world_set(w, st[:, n_tendons]), mlt.world_set(d, st[:, n_tendons])
    return w, d, frame


def build(name):
    import make_fk_truth as mft
    import make_loaded_fk as mlf
    robot, rob, st = mlf.fixture(name)
    lf = dict(np.load(mlf.path(name)))
    out = dict(states=st)
    for case in CASES:
        w, d, frame = call_sets(name, lf, st, case, len(robot.tendons))
        fd = ljr.differenced_solves(rob, st, w, d, frame)
        assert fd["converged"].all(), (name, case, np.flatnonzero(~fd["converged"]))
        out.update({"wrench_" + case: w, "dist_" + case: d, "y_" + case: fd["y"], "tip_" + case: fd["tip"], "J_" + case: fd["J"],
                    "C_" + case: fd["C"]})
        print("%-12s %s |J| <= %.3g  |C| <= %.3g" % (name, case, np.abs(fd["J"]).max(), np.abs(fd["C"]).max()), flush=True)
    mft.save_npz(path(name), out)


if __name__ == "__main__":
    for n in sys.argv[1:] or NAMES:
        build(n)
