"""tr_roadmap_nearest_states / VoxelCachedLazyPRM.nearest_states(_dev): the k nearest valid roadmap vertices of arbitrary states in
the order (dist, vertex index), bit for bit against a restatement of CompoundStateSpace::distance in the library's arithmetic
(tension differences squared and summed column by column, then the root, then the rotation and the retraction term), on every launch
shape (the vertex array whole, cut into slices, a last wave short of queries), on exact ties, across the shortest-arc branch, on
small roadmaps, under a distance bound, and against the table tr_knn gives for the roadmap's own states."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from state_metric_reference import distances          # noqa: E402

pytestmark = pytest.mark.gpu


def _free_space(irt):
    vox = irt.VoxelOctree(256)
    vox.set_xlim(-0.25, 0.25); vox.set_ylim(-0.25, 0.25); vox.set_zlim(-0.25, 0.25)
    return vox


def _rot_ret_robot(irt):
    tendons = [irt.TendonSpecs(C=[np.pi * k / 2, 1.0 + k], D=[0.01], max_tension=15.0) for k in range(4)]
    return irt.TendonRobot(tendons=tendons, specs=irt.BackboneSpecs(dL=0.2 / 128), enable_rotation=True, enable_retraction=True)


def _roadmap(irt, robot, states, status=None):
    chk = irt.VoxelBackboneValidityChecker(robot, irt.VoxelEnvironment(), _free_space(irt))
    prm = irt.VoxelCachedLazyPRM(chk, states, np.zeros((0, 2), dtype=np.int32))
    prm.set_tips(np.zeros((len(states), 3)))                            # (the tips play no part; this uploads the states)
    prm.set_validity(np.ones(len(states), dtype=np.uint8) if status is None else status)
    return chk, prm


def _distances(eng, vertices, q):
    """distance(q, every row of `vertices`) as the header states it (tests/state_metric_reference.py)"""
    return distances(*eng.state_layout(), *eng.space_weights(), q, vertices)


def _nearest(eng, states, ok, queries, k, max_distance=np.inf):
    """(dist, index) order over the vertices `ok` marks: (n, k) indices padded with -1, distances padded with +inf"""
    cand = np.flatnonzero(ok)
    idx = np.full((len(queries), k), -1, dtype=np.int32)
    dist = np.full((len(queries), k), np.inf)
    for i, q in enumerate(queries):
        d = _distances(eng, states[cand], q)
        order = np.argsort(d, kind="stable")[:k]                        # (cand ascends: a stable sort by dist is the order (dist, index))
        order = order[d[order] <= max_distance]
        idx[i, :len(order)] = cand[order]
        dist[i, :len(order)] = d[order]
    return idx, dist


def _same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint64), want[1].view(np.uint64))


def _check_all_launch_shapes(irt, prm, eng, states, ok, queries, ks):
    """k in ks on the batch (some slices), then the batch five times over plus one (the array whole, a last wave of one query), 5
    queries and 1 (many slices), and the device form"""
    want_idx, want_d = _nearest(eng, states, ok, queries, 64)           # (the rows for a smaller k are prefixes)
    for k in ks:
        got = prm.nearest_states(queries, k)
        assert np.array_equal(got[0], want_idx[:, :k]), (k, np.flatnonzero((got[0] != want_idx[:, :k]).any(1))[:5])
        assert np.array_equal(got[1].view(np.uint64), want_d[:, :k].view(np.uint64)), k
    big = np.concatenate([np.tile(queries, (5, 1)), queries[:1]])
    got = prm.nearest_states(big, 5)
    assert _same(got, (np.concatenate([np.tile(want_idx[:, :5], (5, 1)), want_idx[:1, :5]]),
                       np.concatenate([np.tile(want_d[:, :5], (5, 1)), want_d[:1, :5]])))
    assert _same(prm.nearest_states(queries[3:8], 11), (want_idx[3:8, :11], want_d[3:8, :11]))
    assert _same(prm.nearest_states(queries[7], 64), (want_idx[7:8], want_d[7:8]))
    import torch
    n = len(queries)
    d_q = torch.from_numpy(queries).cuda()
    d_idx = torch.empty((n, 11), dtype=torch.int32, device="cuda")
    d_d = torch.empty((n, 11), dtype=torch.float64, device="cuda")
    prm.nearest_states_dev(d_q, n, 11, d_idx, d_d)
    assert _same((d_idx.cpu().numpy(), d_d.cpu().numpy()), (want_idx[:, :11], want_d[:, :11]))
    d_idx.fill_(-7)
    prm.nearest_states_dev(d_q, n, 11, d_idx)                           # (the distances are optional)
    assert np.array_equal(d_idx.cpu().numpy(), want_idx[:, :11])
    return want_idx, want_d


def test_tension_only_equals_the_restatement_bit_for_bit(irt):
    W = irt.workloads
    robot = W.robot_config3()
    rng = np.random.default_rng(41)
    V = 20000
    states = W.random_states(robot, V, seed=3, tau_max=15.0)
    states[::3] = np.round(states[::3])                                 # a third on a 1 N lattice: exact ties
    status = np.where(rng.random(V) > 0.1, 1, 2).astype(np.uint8)
    chk = irt.VoxelBackboneValidityChecker(robot, irt.VoxelEnvironment(), _free_space(irt))
    prm = irt.VoxelCachedLazyPRM(chk, states, np.zeros((0, 2), dtype=np.int32))
    queries = W.random_states(robot, 1000, seed=4, tau_max=15.0)
    queries[:200] = np.round(queries[:200])                             # lattice points: many vertices at exactly the same distance
    queries[200:260] = states[rng.integers(0, V, 60)]                   # equal to a vertex
    with pytest.raises(irt.InvalidArgument):
        prm.nearest_states(queries[:1], 5)                              # no tips set: the states are not on the device
    prm.set_tips(np.zeros((V, 3)), present=rng.random(V) > 0.5)         # (having a tip is not required)
    prm.set_validity(status)
    eng = chk.engine
    want_idx, want_d = _check_all_launch_shapes(irt, prm, eng, states, status == 1, queries, (1, 5, 11, 64))
    assert (want_d[:200] == np.roll(want_d[:200], 1, axis=1))[:, 1:].any()                   # the ties exist
    hit = status[want_idx[200:260, 0]] == 1
    assert (want_d[200:260, 0] == 0.0).sum() >= 40 and hit.all()
    # a distance bound cuts the rows where the restatement cuts them
    bound = float(np.median(want_d[:, 20]))
    got = prm.nearest_states(queries, 64, max_distance=bound)
    want = _nearest(eng, states, status == 1, queries, 64, max_distance=bound)
    assert _same(got, want)
    assert (got[0][:, 20] == -1).any() and (got[0][:, 20] >= 0).any() and (got[0][:, 0] >= 0).all()
    exact = float(want_d[5, 9])                                         # an entry AT the bound stays
    got = prm.nearest_states(queries[5], 64, max_distance=exact)
    assert _same(got, _nearest(eng, states, status == 1, queries[5:6], 64, max_distance=exact)) and got[0][0, 9] >= 0
    # fewer than k valid vertices: padded with -1 / +inf; none: the whole row
    few = np.full(V, 2, dtype=np.uint8)
    few[rng.choice(V, 40, replace=False)] = 1
    prm.set_validity(few)
    got = prm.nearest_states(queries[:50], 64)
    assert _same(got, _nearest(eng, states, few == 1, queries[:50], 64))
    assert (got[0][:, :40] >= 0).all() and (got[0][:, 40:] == -1).all() and np.isinf(got[1][:, 40:]).all()
    prm.set_validity(np.full(V, 2, dtype=np.uint8))
    idx, dist = prm.nearest_states(queries[:50], 5)
    assert (idx == -1).all() and np.isinf(dist).all()
    # errors
    for k in (0, 65):
        with pytest.raises(irt.InvalidArgument):
            prm.nearest_states(queries[:2], k)
    with pytest.raises(irt.InvalidArgument):
        prm.nearest_states(queries[:2], 5, max_distance=-1.0)
    with pytest.raises(irt.InvalidArgument):
        prm._check(prm.lib.tr_roadmap_nearest_states(prm._rm, queries.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), 2, 5, np.inf, None, None))
    assert prm.lib.tr_roadmap_nearest_states(prm._rm, None, 0, 5, np.inf, None, None) == 0   # n = 0


def test_rotation_and_retraction_equal_the_restatement_bit_for_bit(irt):
    W = irt.workloads
    robot = _rot_ret_robot(irt)
    rng = np.random.default_rng(43)
    V = 12000
    states = W.random_states(robot, V, seed=5, tau_max=4.0)
    queries = W.random_states(robot, 600, seed=6, tau_max=4.0)
    # rotations within 1e-3 of +pi and -pi on both sides: the shortest arc between them is tiny, the plain difference almost 2 pi
    near = lambda n: np.where(rng.random(n) > 0.5, 1.0, -1.0) * (np.pi - rng.uniform(0.0, 1e-3, n))
    states[::2, 4] = near(len(states[::2]))
    queries[:400, 4] = near(400)
    queries[400:440] = states[rng.integers(0, V, 40)]
    status = np.where(rng.random(V) > 0.1, 1, 2).astype(np.uint8)
    chk, prm = _roadmap(irt, robot, states, status)
    eng = chk.engine
    assert eng.state_layout() == (4, True, True)
    want_idx, want_d = _check_all_launch_shapes(irt, prm, eng, states, status == 1, queries, (1, 5, 11, 64))
    # the branch decides neighbours: a nearest vertex on the OTHER side of the cut
    other = np.sign(states[want_idx[:400, 0], 4]) != np.sign(queries[:400, 4])
    assert other.sum() > 50


@pytest.mark.parametrize("V", [1, 63, 64, 65, 200])
def test_small_roadmaps(irt, V):
    W = irt.workloads
    robot = W.robot_config3()
    states = W.random_states(robot, V, seed=7, tau_max=15.0)
    queries = W.random_states(robot, 37, seed=8, tau_max=15.0)
    chk, prm = _roadmap(irt, robot, states)
    ok = np.ones(V, dtype=bool)
    for k in (1, 5, 64):
        assert _same(prm.nearest_states(queries, k), _nearest(chk.engine, states, ok, queries, k)), k
    assert _same(prm.nearest_states(queries[:1], 64), _nearest(chk.engine, states, ok, queries[:1], 64))


@pytest.mark.parametrize("which", ["tensions", "rotation_retraction"])
def test_vertex_rows_equal_tr_knn(irt, which):
    """the query states[v] gets row v of Engine.knn's table: the new kernel and the existing one agree on indices and distance bits"""
    W = irt.workloads
    robot = W.robot_config3() if which == "tensions" else _rot_ret_robot(irt)
    states = W.random_states(robot, 3000, seed=9, tau_max=10.0)
    assert len(np.unique(states, axis=0)) == len(states)
    chk, prm = _roadmap(irt, robot, states)
    for k in (1, 11):
        idx, dist = chk.engine.knn(states, k)
        assert _same(prm.nearest_states(states, k), (idx, dist)), k
