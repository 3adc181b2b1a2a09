"""tests/golden/loaded_ret_edges_config3_ret_edges.npz against its generator (tests/golden/make_loaded_ret_edges.py), on the CPU: the
file is the generator's candidates under its own rule, and the numpy shooting and the oracle reproduce the verdicts of two of its
edges -- one that the load makes valid and one that it makes invalid -- against the file's spheres."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.join(HERE, "golden")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import loaded_ret_edges_common as rec                                 # noqa: E402
import make_loaded_ret_edges as gen                                   # noqa: E402


def test_the_generator_reproduces_two_edges(irt):
    assert os.path.getsize(gen.PATH) < 1 << 20
    fx = dict(np.load(gen.PATH))
    robot = rec.robot(irt, gen.NAME)
    loaded, un = fx["valid_loaded"].astype(bool), fx["valid_unloaded"].astype(bool)
    assert (loaded & ~un).sum() >= 3 and (~loaded & un).sum() >= 3
    assert np.array_equal(fx["grid"], [gen.GRID_N, gen.HALF]) and np.array_equal(fx["wrench"], rec.WRENCH)
    assert np.array_equal(fx["dist"], rec.dist_of(robot))
    a, b = gen.candidate_edges(robot)
    assert all((a == fx["a"][k]).all(axis=1).any() for k in range(len(fx["a"])))       # the file's edges are candidates of the generator
    assert (fx["b"][:, -1] > fx["a"][:, -1]).all()                                     # ... between states of different s_start
    rows = [int(np.flatnonzero(loaded & ~un)[0]), int(np.flatnonzero(~loaded & un)[0])]
    decided, got_loaded, got_un, _ = gen.verdicts(robot, fx["a"][rows], fx["b"][rows], fx["spheres"])
    assert decided.all() and np.array_equal(got_loaded, loaded[rows]) and np.array_equal(got_un, un[rows])
