"""tests/state_metric_reference.py on the CPU, for all 32 state layouts: its restatement of the compound metric against the oracle's
orc_state_distance, its partition-based selection against a stable sort of the whole row, and the inputs it generates for
tests/test_gpu_neighbour_layouts.py against what they are for (exact ties inside the first 11 neighbours and across position 11,
a cluster of coincident states, neighbours across the +-pi cut, a distance bound that cuts some rows and not others).  No GPU."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import state_metric_reference as R          # noqa: E402

# Worst |restatement - orc_state_distance| / orc_state_distance over the 300 pairs of every layout, MEASURED: 0.0 at all 32.  The
# oracle forms the same sums in the same order and is built without contraction (oracle/Makefile: -ffp-contract=off), so the two
# agree to the bit; the test holds 4 x the figure, the project's factor -- here: equality.
RESTATEMENT_VS_ORACLE = 0.0

K = R.K_TABLE


def host_weights(robot):
    """Engine.space_weights() written out: ext = sqrt(sum max_tension_i^2) summed left to right, ext / 4 pi and 2 ext / L"""
    ext2 = 0.0
    for t in robot.tendons:
        ext2 += t.max_tension * t.max_tension
    ext = math.sqrt(ext2)
    return ext / (4.0 * math.pi), 2.0 * ext / robot.specs.L


@pytest.fixture(scope="module", params=R.LAYOUTS, ids=R.layout_id)
def lay(request, irt):
    nt, rot, ret = request.param
    robot = R.layout_robot(irt, nt, rot, ret)
    return (nt, rot, ret) + host_weights(robot), robot


def test_the_32_layouts_and_the_robot():
    assert len(R.LAYOUTS) == 32 == len(set(R.LAYOUTS))
    assert {nt + rot + ret for nt, rot, ret in R.LAYOUTS} == set(range(1, 11))


def test_restatement_equals_the_oracle_s_distance(lay, orc, helpers):
    metric, robot = lay
    caps = [t.max_tension for t in robot.tendons]
    assert len(set(caps)) == len(caps) and robot.specs.dL == robot.specs.L / 128
    st = R.layout_states(robot, 600, seed=8000)
    a, b = st[:300], st[300:]
    orb = helpers.oracle_robot(orc, robot)
    f = orb.lib.orc_state_distance
    want = np.array([f(C.byref(orb.c), orc._dp(np.ascontiguousarray(x)), orc._dp(np.ascontiguousarray(y))) for x, y in zip(a, b)])
    got = R.distances(*metric, a, b)                                        # (rows against rows)
    assert (want > 0).sum() > 250 and (got[want == 0] == 0).all()         # (coincident pairs: the cluster, lattice sites)
    worst = float((np.abs(got - want)[want > 0] / want[want > 0]).max())
    print("restatement vs oracle, worst relative difference: %.3g" % worst)
    assert worst <= 4 * RESTATEMENT_VS_ORACLE
    # a block of queries against all rows, and one pair: the bits of one query against all rows
    assert np.array_equal(R.distances(*metric, a[:7, None, :], b).view(np.uint64), np.stack([R.distances(*metric, x, b) for x in a[:7]]).view(np.uint64))
    assert all(R.distances(*metric, a[i], b[i]) == got[i] == R.distances(*metric, a[i], b)[i] for i in range(7))
    if metric[1]:
        # |d theta| = pi exactly keeps the plain difference (the branch is strict); just past it the arc is the short way round
        x, y = st[0].copy(), st[0].copy()
        x[metric[0]], y[metric[0]] = -np.pi, 0.0
        assert R.distances(*metric, x, y[None, :])[0] == f(C.byref(orb.c), orc._dp(x), orc._dp(y)) == metric[3] * np.pi
        x[metric[0]], y[metric[0]] = -np.pi + 1e-4, np.pi - 1e-4
        assert R.distances(*metric, x, y[None, :])[0] == metric[3] * (2.0 * np.pi - np.abs(x[metric[0]] - y[metric[0]])) < 1e-3 * metric[3]


def test_partition_selection_equals_a_stable_sort_of_the_whole_row(irt):
    robot = R.layout_robot(irt, 3, True, True)
    metric = (3, True, True) + host_weights(robot)
    st = R.layout_states(robot, 900, seed=8001)
    ok = np.random.default_rng(1).random(900) > 0.1
    for k, bound in ((1, np.inf), (11, np.inf), (64, np.inf), (11, 9.0), (1000, np.inf)):
        fast = R.nearest(*metric, st, ok, st[:300], k, bound)
        slow = R.nearest(*metric, st, ok, st[:300], k, bound, whole_row_sort=True)
        assert R.same(fast, slow), (k, bound)
    idx, dist = R.nearest(*metric, st, ok, st[:300], 1000)
    assert (idx[:, :ok.sum()] >= 0).all() and (idx[:, ok.sum():] == -1).all() and np.isinf(dist[:, ok.sum():]).all()
    idx, dist = R.nearest(*metric, st, np.zeros(900, dtype=bool), st[:5], 4)
    assert (idx == -1).all() and np.isinf(dist).all()
    # an entry AT the bound stays (and whatever ties with it), every larger one goes
    full = R.nearest(*metric, st, ok, st[:20], 11)
    for r in range(20):
        m = float(full[1][r, 6])
        cut = R.nearest(*metric, st, ok, st[r:r + 1], 11, max_distance=m)
        stays = full[1][r] <= m
        assert stays[6] and np.array_equal(cut[0][0], np.where(stays, full[0][r], -1)) and np.array_equal(cut[1][0], np.where(stays, full[1][r], np.inf))
    assert (full[1][:, 7] > full[1][:, 6]).any() and (full[1][:, 7] == full[1][:, 6]).any()


def _ties(dist, rows):
    inside = (dist[rows, :K - 1] == dist[rows, 1:K]).any(axis=1)
    across = dist[rows, K - 1] == dist[rows, K]
    return inside, across


def _adequate(metric, robot, states, ok, queries, q_rows, free_rows, what):
    """the properties the inputs exist for, on the reference's own tables of the query rows q_rows; free_rows: positions in q_rows
    of the queries that are no member of a cluster (the ties and the cut must not come from the cluster alone)"""
    idx, dist = R.nearest(*metric, states, ok, queries[q_rows], K + 1)
    inside, across = _ties(dist, free_rows)
    assert inside.any(), what + ": no exact tie inside the first %d entries" % K
    assert across.any(), what + ": no exact tie across position %d" % K
    m, row = R.exact_bound(dist[free_rows])
    bounded = R.nearest(*metric, states, ok, queries[q_rows], K, max_distance=m)
    assert bounded[0][free_rows[row], 5] >= 0 and bounded[1][free_rows[row], 5] == m              # the entry at the bound stayed
    full = bounded[0][free_rows, K - 1] >= 0
    assert full.any() and (~full).any(), what + ": the bound cuts all rows or none"
    if metric[1]:
        c = metric[0]
        th_q = queries[q_rows, c]
        th_n = states[idx[:, :K], c]
        edge = np.abs(th_q) > np.pi - 1e-3
        other = edge[:, None] & (np.abs(th_n) > 0.5 * np.pi) & (np.sign(th_n) != np.sign(th_q)[:, None])
        assert other.sum() > 20, what + ": %d neighbours across the cut" % other.sum()
    if metric[1] and metric[2]:
        # the order of the two last terms shows in the bits: a kernel that adds the retraction term first fails the comparison
        nt, w_rot, w_ret = metric[0], metric[3], metric[4]
        q, v = queries[q_rows][:, None, :], states[idx[:, :K]]
        tension = R.distances(nt, False, False, 0.0, 0.0, np.zeros(nt), (q - v)[..., :nt].reshape(-1, nt)).reshape(idx[:, :K].shape)
        arc = np.abs(q[..., nt] - v[..., nt])
        arc = np.where(arc > np.pi, 2.0 * np.pi - arc, arc)
        t = q[..., nt + 1] - v[..., nt + 1]
        assert np.array_equal((tension + w_rot * arc) + w_ret * np.sqrt(t * t), dist[:, :K])
        assert ((tension + w_ret * np.sqrt(t * t)) + w_rot * arc != dist[:, :K]).sum() > 20, what + ": the order of the terms does not show"
    return idx, dist


def test_knn_inputs_do_what_they_are_for(lay):
    metric, robot = lay
    st = R.knn_inputs(robot)
    where = R.layout_rows(R.N_KNN)
    rows = R.sample_rows(R.N_KNN)
    assert len(st) == R.N_KNN and len(rows) == 256 and np.isin(where["cluster"], rows).all()
    assert len(where["cluster"]) > 65 and (st[where["cluster"]] == st[where["cluster"][0]]).all()
    assert (st[where["tension_min"], 0] == st[:, 0].min()).all() and (st[where["tension_max"], 0] == st[:, 0].max()).all()
    c = metric[0]
    if metric[1]:
        th = st[:, c]
        assert (th >= -np.pi).all() and (th < np.pi).all() and 0.4 < (np.abs(th) > np.pi - 1e-3).mean() < 0.7
        assert (th[where["theta_minus_pi"]] == -np.pi).all() and (th[where["theta_zero"]] == 0.0).all()
        c += 1
    if metric[2]:
        assert (st[where["s_zero"], c] == 0.0).all() and (st[where["s_full"], c] == robot.specs.L).all()
    free = np.flatnonzero(~np.isin(rows, where["cluster"]))
    idx, dist = _adequate(metric, robot, st, None, st, rows, free, "knn")
    in_cluster = np.flatnonzero(np.isin(rows, where["cluster"]))
    assert (dist[in_cluster, :K] == 0.0).all() and (idx[in_cluster, :K] == where["cluster"][:K]).all()


def test_roadmap_inputs_do_what_they_are_for(lay):
    metric, robot = lay
    states, status, queries = R.roadmap_inputs(robot)
    assert len(states) == R.V_ROADMAP and len(queries) == R.N_QUERIES and 0.05 < (status == 2).mean() < 0.15
    rows = R.sample_rows(R.N_QUERIES)
    rows = np.union1d(rows, [22])
    free = np.flatnonzero(rows != 22)
    idx, dist = _adequate(metric, robot, states, status == 1, queries, rows, free, "roadmap")
    # query 22 sits on the vertices' cluster: its row starts with the cluster's VALID vertices, in index order
    cl = R.layout_rows(R.V_ROADMAP)["cluster"]
    cl = cl[status[cl] == 1]
    at = int(np.flatnonzero(rows == 22)[0])
    assert len(cl) > K and (dist[at, :K] == 0.0).all() and (idx[at, :K] == cl[:K]).all()
    # queries that equal a vertex: distance 0 to it where it is valid
    hit = np.arange(20, R.N_QUERIES, 37)
    assert (queries[hit] == states[R.nearest(*metric, states, None, queries[hit], 1)[0][:, 0]]).all()
