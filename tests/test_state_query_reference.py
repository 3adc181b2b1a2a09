"""Pins tests/state_query_reference.py (the restatement the GPU tests of the seeded search compare against) on a hand-made
8-vertex graph whose answers can be checked by eye:

    0 --1-- 1 --1-- 2 --1-- 3          6 --2-- 7     (vertex 5 invalid; edge 1-4 invalid)
    |               |
    4 (4-0: 1.5)    5 (2-5: 1, 5-3: 0.25)
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import state_query_reference as ref          # noqa: E402

EDGES = np.array([[0, 1], [1, 2], [2, 3], [0, 4], [1, 4], [2, 5], [5, 3], [6, 7]])
W = np.array([1.0, 1.0, 1.0, 1.5, 0.125, 1.0, 0.25, 2.0])
VV = np.array([1, 1, 1, 1, 1, 0, 1, 1], dtype=bool)
EV = np.array([1, 1, 1, 1, 0, 1, 1, 1], dtype=bool)


def _solve(src, dst, direct=None):
    return ref.solve_seeded(8, EDGES, W, VV, EV, src, dst, direct)


def test_nearest_seeds_are_not_the_optimal_ones():
    # the cheaper source seed (vertex 4 at 0.1) sits behind the 1.5 edge; vertex 1 at 0.5 wins: 0.5 + 2 + 0.2
    r = _solve([([4, 1], [0.1, 0.5])], [([0, 3], [5.0, 0.2])])
    assert r["status"][0] == ref.SOLVED and (r["src_pick"][0], r["dst_pick"][0]) == (1, 1) and not r["direct"][0]
    assert r["cost"][0] == (0.5 + 2.0) + 0.2


def test_invalid_items_are_not_part_of_the_graph():
    # 4 -> 1 must go round by 0 (edge 1-4 is invalid): 1.5 + 1; 2 -> 3 may not cut through vertex 5
    r = _solve([([4], [0.0]), ([2], [0.0])], [([1], [0.0]), ([3], [0.0])])
    assert list(r["cost"]) == [2.5, 1.0]
    # a seed on the invalid vertex is no seed
    r = _solve([([5, 2], [0.0, 0.0])], [([3], [0.0])])
    assert r["src_pick"][0] == 1 and r["cost"][0] == 1.0


def test_source_and_target_on_one_vertex():
    r = _solve([([2, 0], [0.75, 0.0])], [([2], [0.5])])
    assert (r["src_pick"][0], r["dst_pick"][0]) == (0, 0) and r["cost"][0] == 1.25        # against 0 + 2 + 0.5


def test_direct_answer_wins_a_tie_and_loses_when_dearer():
    src, dst = [([0], [0.25])] * 3, [([2], [0.25])] * 3
    r = _solve(src, dst, np.array([2.5, 2.5000001, np.inf]))
    assert list(r["direct"]) == [True, False, False]
    assert list(r["src_pick"]) == [-1, 0, 0] and list(r["dst_pick"]) == [-1, 0, 0]
    assert list(r["cost"]) == [2.5, 2.5, 2.5] and (r["status"] == ref.SOLVED).all()


def test_no_path():
    # different components; an empty seed list; an empty list with a direct cost is a direct answer
    r = _solve([([0], [0.0]), ([], []), ([], [])], [([7], [0.0]), ([3], [0.0]), ([3], [0.0])], np.array([np.inf, np.inf, 4.0]))
    assert list(r["status"]) == [ref.NO_PATH, ref.NO_PATH, ref.SOLVED]
    assert np.isinf(r["cost"][:2]).all() and r["cost"][2] == 4.0 and r["direct"][2]
    assert list(r["src_pick"]) == [-1, -1, -1]


def test_path_cost_sums_left_to_right():
    w = {(0, 1): 0.1, (1, 2): 0.2, (2, 3): 0.3}
    got = ref.path_cost(lambda a, b: w[(a, b)], 0.7, [0, 1, 2, 3], 0.9)
    assert got == (((0.7 + 0.1) + 0.2) + 0.3) + 0.9
