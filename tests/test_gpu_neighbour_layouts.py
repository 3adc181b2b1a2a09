"""The three neighbour-search kernels at EVERY state layout -- 1 .. 8 tendons, rotation on / off, retraction on / off: 32 instantiations
each of knn_wave_query (tr_knn*, k <= 64), knn_bruteforce (k > 64 or TENDON_HIP_KNN=lanes) and state_knn (tr_roadmap_nearest_states)
-- bit for bit against the numpy restatement of the metric in tests/state_metric_reference.py: indices with array_equal, distances
as uint64.  The robots have unequal tension caps; the states carry exact ties, a cluster of coincident states, rotations either side
of the +-pi cut and at exactly pi apart, retractions at 0 and L, first tensions at the ends of their range (their adequacy is
asserted on the CPU by tests/test_state_metric_reference.py).  One engine, one reference table and one roadmap per layout, shared by
the layout's tests."""
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import state_metric_reference as R          # noqa: E402

pytestmark = pytest.mark.gpu

K = R.K_TABLE


# stateq_kernel.hpp: queries per wave and tiles in flight of state_knn by state size
def stateq_q(ss): return 4 if ss <= 6 else 2
def stateq_g(ss): return 4 if ss <= 4 else 2


def _view(d):
    return np.ascontiguousarray(d).view(np.uint64)


def _assert_same(got, want, what):
    bad = np.flatnonzero((got[0] != want[0]).any(axis=1))
    assert len(bad) == 0, (what, "indices differ in %d rows, first" % len(bad), bad[:5], got[0][bad[:2]], want[0][bad[:2]])
    bad = np.flatnonzero((_view(got[1]) != _view(want[1])).any(axis=1))
    assert len(bad) == 0, (what, "distance bits differ in %d rows, first" % len(bad), bad[:5], got[1][bad[:2]], want[1][bad[:2]])


def _cut(table, m):
    """nearest(..., K, max_distance = m) from the unbounded table: the rows are ordered, so what the bound drops is a suffix (that
    this IS what the reference gives: test_state_metric_reference.py, and the roadmap's bound test below on 300 rows)"""
    idx, dist = table[0][:, :K], table[1][:, :K]
    return np.where(dist <= m, idx, -1).astype(np.int32), np.where(dist <= m, dist, np.inf)


def _same_tables(cut, ref, rows):
    return R.same((cut[0][:rows], cut[1][:rows]), ref)


def _free_space(irt):
    vox = irt.VoxelOctree(256)
    vox.set_xlim(-0.25, 0.25); vox.set_ylim(-0.25, 0.25); vox.set_zlim(-0.25, 0.25)
    return vox


def _roadmap(irt, chk, states, status=None):
    prm = irt.VoxelCachedLazyPRM(chk, states, np.zeros((0, 2), dtype=np.int32))
    prm.set_tips(np.zeros((len(states), 3)))                            # (the tips play no part; this uploads the states)
    prm.set_validity(np.ones(len(states), dtype=np.uint8) if status is None else status)
    return prm


PARAMS = list(R.LAYOUTS)     # what every test below that takes `lay` is run for


@pytest.fixture(scope="module", params=PARAMS, ids=R.layout_id)
def lay(request, irt):
    """a layout's robot, engine, states and the reference's table of ALL rows at k = 65 (the rows for a smaller k are prefixes)"""
    w = types.SimpleNamespace()
    w.nt, w.rot, w.ret = w.layout = request.param
    w.ss = w.nt + int(w.rot) + int(w.ret)
    w.robot = R.layout_robot(irt, *w.layout)
    w.eng = w.robot.engine()
    assert w.eng.state_layout() == w.layout
    w.metric = w.layout + tuple(w.eng.space_weights())
    w.st = R.knn_inputs(w.robot)
    w.where = R.layout_rows(len(w.st))
    w.want = R.nearest(*w.metric, w.st, None, w.st, 65)
    return w


@pytest.fixture(scope="module")
def rm(lay, irt):
    """the layout's roadmap in free space (about 10 % of its vertices invalid), queries and the reference's table at k = 64"""
    w = types.SimpleNamespace()
    w.states, w.status, w.queries = R.roadmap_inputs(lay.robot)
    w.chk = irt.VoxelBackboneValidityChecker(lay.robot, irt.VoxelEnvironment(), _free_space(irt))
    assert w.chk.engine.state_layout() == lay.layout
    w.metric = lay.layout + tuple(w.chk.engine.space_weights())
    w.prm = _roadmap(irt, w.chk, w.states, w.status)
    w.want = R.nearest(*w.metric, w.states, w.status == 1, w.queries, 64)
    return w


def _knn(lay, monkeypatch, lanes, *args, **kw):
    if lanes:
        monkeypatch.setenv("TENDON_HIP_KNN", "lanes")
    else:
        monkeypatch.delenv("TENDON_HIP_KNN", raising=False)
    return lay.eng.knn(*args, **kw)


# ---- tr_knn: knn_wave_query and knn_bruteforce --------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["wave", "lanes"])
def test_knn_table_equals_the_restatement_on_every_row(lay, monkeypatch, form):
    got = _knn(lay, monkeypatch, form == "lanes", lay.st, K)
    _assert_same(got, (lay.want[0][:, :K], lay.want[1][:, :K]), form)
    cl = lay.where["cluster"]
    assert (got[1][cl] == 0.0).all() and (got[0][cl] == cl[:K]).all()                      # coincident states: index order


def test_knn_at_the_64_65_boundary(lay, monkeypatch):
    """k = 65 takes the lane-per-query kernel on its own; its first 64 columns are the wave form's k = 64 table; both equal the
    restatement on the sample rows (the cluster, the boundary values, a spread of the rest)"""
    monkeypatch.delenv("TENDON_HIP_KNN", raising=False)
    g65 = lay.eng.knn(lay.st, 65)
    g64 = lay.eng.knn(lay.st, 64)
    _assert_same((g65[0][:, :64], g65[1][:, :64]), g64, "65 / 64")
    rows = R.sample_rows(len(lay.st))
    assert len(rows) == 256 and all(np.isin(v, rows).all() for key, v in lay.where.items() if key != "lattice")
    _assert_same((g65[0][rows], g65[1][rows]), (lay.want[0][rows], lay.want[1][rows]), "k = 65")
    _assert_same((g64[0][rows], g64[1][rows]), (lay.want[0][rows, :64], lay.want[1][rows, :64]), "k = 64")


@pytest.mark.parametrize("form", ["wave", "lanes"])
def test_knn_under_a_distance_bound_that_is_an_exact_entry(lay, monkeypatch, form):
    rows = R.sample_rows(len(lay.st))
    free = rows[~np.isin(rows, lay.where["cluster"])]
    m, r = R.exact_bound(lay.want[1][free, :K])
    r = free[r]
    want = _cut(lay.want, m)
    assert _same_tables(want, R.nearest(*lay.metric, lay.st, None, lay.st[:300], K, max_distance=m), 300)
    assert want[1][r, 5] == m and (want[0][:, K - 1] == -1).any() and (want[0][:, K - 1] >= 0).any()
    got = _knn(lay, monkeypatch, form == "lanes", lay.st, K, max_distance=m)
    assert got[0][r, 5] == lay.want[0][r, 5] >= 0 and got[1][r, 5] == m                    # the entry AT the bound stayed
    _assert_same(got, want, form)


@pytest.mark.parametrize("form", ["wave", "lanes"])
def test_knn_query_range_gives_those_rows(lay, monkeypatch, form):
    """1001 queries: the last block of four waves has one query"""
    got = _knn(lay, monkeypatch, form == "lanes", lay.st, K, query_range=(130, 1001))
    assert got[0].shape == (1001, K)
    _assert_same(got, (lay.want[0][130:1131, :K], lay.want[1][130:1131, :K]), form)


@pytest.mark.parametrize("form", ["wave", "lanes"])
def test_knn_whatever_the_cell_width(lay, monkeypatch, form):
    for cell in ("0.25", "4"):
        monkeypatch.setenv("TENDON_HIP_KNN_CELL", cell)
        got = _knn(lay, monkeypatch, form == "lanes", lay.st, K)
        monkeypatch.delenv("TENDON_HIP_KNN_CELL")
        _assert_same(got, (lay.want[0][:, :K], lay.want[1][:, :K]), (form, cell))


def test_knn_edge_list_equals_the_dedup_of_the_table(lay, monkeypatch):
    monkeypatch.delenv("TENDON_HIP_KNN", raising=False)
    n = len(lay.st)
    src = np.repeat(np.arange(n), K)
    dst = lay.want[0][:, :K].reshape(-1).astype(np.int64)
    keep = (dst >= 0) & (dst != src)
    key = np.unique(np.minimum(src[keep], dst[keep]) * n + np.maximum(src[keep], dst[keep]))
    want = np.stack([key // n, key % n], 1)
    assert np.array_equal(lay.eng.knn_edges(lay.st, K), want)


@pytest.mark.parametrize("form", ["wave", "lanes"])
def test_knn_of_fewer_states_than_k_is_padded(lay, monkeypatch, form):
    small = R.layout_states(lay.robot, 40, seed=8400)
    got = _knn(lay, monkeypatch, form == "lanes", small, 64)
    want = R.nearest(*lay.metric, small, None, small, 64)
    assert (want[0][:, :40] >= 0).all() and (want[0][:, 40:] == -1).all() and np.isinf(want[1][:, 40:]).all()
    _assert_same(got, want, form)


def test_kstar_k_is_the_closed_form_at_this_state_size(lay):
    """og::KStarStrategy: k = ceil((e + e / dim) ln n)"""
    for n in (1000, 100000):
        assert lay.eng.kstar_k(n) == int(np.ceil((np.e + np.e / lay.ss) * np.log(n)))


# ---- tr_roadmap_nearest_states: state_knn (+ tip_knn_merge) ---------------------------------------------------------------------

def test_nearest_states_with_the_vertex_array_whole(lay, rm):
    """2049 queries: one slice for every Q, a last wave with a single query"""
    for k in (1, K, 64):
        _assert_same(rm.prm.nearest_states(rm.queries, k), (rm.want[0][:, :k], rm.want[1][:, :k]), k)


def test_nearest_states_of_a_few_queries_cut_the_vertex_array_into_slices(lay, rm):
    """5 queries, 1 query and 2 Q + 1 (two full groups and a wave with one query): slices of the vertex array and tip_knn_merge"""
    q = stateq_q(lay.ss)
    for first, count in ((3, 5), (22, 1), (7, 1), (40, 2 * q + 1)):
        for k in (1, K, 64):
            got = rm.prm.nearest_states(rm.queries[first:first + count], k)
            _assert_same(got, (rm.want[0][first:first + count, :k], rm.want[1][first:first + count, :k]), (first, count, k))


def test_nearest_states_device_form(lay, rm):
    import torch
    n = len(rm.queries)
    d_q = torch.from_numpy(rm.queries).cuda()
    d_idx = torch.full((n, K), -7, dtype=torch.int32, device="cuda")
    d_d = torch.full((n, K), -7.0, dtype=torch.float64, device="cuda")
    rm.prm.nearest_states_dev(d_q, n, K, d_idx, d_d)
    _assert_same((d_idx.cpu().numpy(), d_d.cpu().numpy()), (rm.want[0][:, :K], rm.want[1][:, :K]), "dev")


def test_nearest_states_under_a_distance_bound_that_is_an_exact_entry(lay, rm):
    free = np.setdiff1d(R.sample_rows(len(rm.queries)), [22])
    m, r = R.exact_bound(rm.want[1][free, :K])
    r = free[r]
    want = _cut(rm.want, m)
    assert _same_tables(want, R.nearest(*rm.metric, rm.states, rm.status == 1, rm.queries[:300], K, max_distance=m), 300)
    assert want[1][r, 5] == m and (want[0][:, K - 1] == -1).any() and (want[0][:, K - 1] >= 0).any()
    got = rm.prm.nearest_states(rm.queries, K, max_distance=m)
    assert got[0][r, 5] == rm.want[0][r, 5] >= 0 and got[1][r, 5] == m                     # the entry AT the bound stayed
    _assert_same(got, want, "all queries")
    one = rm.prm.nearest_states(rm.queries[r], K, max_distance=m)                           # ... and through the slices' merge
    _assert_same(one, (want[0][r:r + 1], want[1][r:r + 1]), "one query")


def test_nearest_states_with_fewer_valid_vertices_than_k_and_with_none(lay, rm):
    V = len(rm.states)
    few = np.full(V, 2, dtype=np.uint8)
    few[np.random.default_rng(8500).choice(V, 40, replace=False)] = 1
    try:
        rm.prm.set_validity(few)
        for count in (50, 5):
            got = rm.prm.nearest_states(rm.queries[:count], 64)
            _assert_same(got, R.nearest(*rm.metric, rm.states, few == 1, rm.queries[:count], 64), count)
            assert (got[0][:, :40] >= 0).all() and (got[0][:, 40:] == -1).all() and np.isinf(got[1][:, 40:]).all()
        rm.prm.set_validity(np.full(V, 2, dtype=np.uint8))
        for count in (50, 5):
            idx, dist = rm.prm.nearest_states(rm.queries[:count], 5)
            assert (idx == -1).all() and np.isinf(dist).all()
    finally:
        rm.prm.set_validity(rm.status)


def test_vertex_rows_equal_tr_knn(lay, rm, irt, monkeypatch):
    """all vertices valid: the query states[v] gets row v of Engine.knn's table -- distinct states, and the layout's own vertices
    (ties and coincident states: both searches order by (distance, index))"""
    monkeypatch.delenv("TENDON_HIP_KNN", raising=False)
    distinct = irt.workloads.random_states(lay.robot, R.V_ROADMAP, seed=8600)
    assert len(np.unique(distinct, axis=0)) == len(distinct)
    prm = _roadmap(irt, rm.chk, distinct)
    _assert_same(prm.nearest_states(distinct, K), rm.chk.engine.knn(distinct, K), "distinct")
    try:
        rm.prm.set_validity(np.ones(len(rm.states), dtype=np.uint8))
        _assert_same(rm.prm.nearest_states(rm.states, K), rm.chk.engine.knn(rm.states, K), "layout vertices")
    finally:
        rm.prm.set_validity(rm.status)


# ---- what the parametrisation covers --------------------------------------------------------------------------------------------

def test_every_layout_is_run():
    assert len(PARAMS) == 32 and sorted(PARAMS) == sorted((nt, rot, ret) for nt in range(1, 9) for rot in (False, True) for ret in (False, True))
    sizes = {nt + rot + ret for nt, rot, ret in PARAMS}
    assert sizes == set(range(1, 11))
    assert {(stateq_q(ss), stateq_g(ss)) for ss in sizes} == {(4, 4), (4, 2), (2, 2)}
    # CH of knn_bruteforce (knn_kernel.hpp): 8 candidates per chunk up to 4 doubles a state, 4 beyond
    assert {8 if ss <= 4 else 4 for ss in sizes} == {8, 4}
