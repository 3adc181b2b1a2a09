"""Queries between arbitrary states (include/tendon_hip.h: rules A1 - A4, S1 - S4, T1 - T3): attach_states equals validate_batch +
nearest_states + validate_edges bit for bit; solve_seeded equals the numpy / scipy restatement of tests/state_query_reference.py;
solve_states equals attach + that restatement; chained_plan_from_states solves what chained_plan solves, no dearer, and starts
off the roadmap too.  Two small worlds, each a roadmap built among few spheres and queried among more (so that cached items are
invalid, the graph falls into components and validity is learned lazily): config 1's robot on a 64^3 grid, config 3's with
rotation on a 256^3 grid."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import state_query_reference as ref          # noqa: E402
from state_metric_reference import distances          # noqa: E402

pytestmark = pytest.mark.gpu

SOLVED, NO_PATH, INVALID_START, INVALID_GOAL = 0, 1, 2, 3


class World:
    pass


def _world(irt, robot, N, n_vertices, k, build_spheres, query_spheres):
    W = irt.workloads
    w = World()
    w.W = W
    vox, _ = W.reach_environment(seed=7, n_spheres=build_spheres, N=N)
    w.robot = robot
    w.chk = irt.VoxelBackboneValidityChecker(robot, irt.VoxelEnvironment(), vox)
    w.mv = irt.VoxelBackboneMotionValidator(w.chk)
    w.eng = w.chk.engine
    rb = irt.RoadmapBuilder(w.chk, w.mv, seed=21)
    w.states, _ = rb.sample_valid_vertices(n_vertices, batch=8192)
    edges = rb.knn_edges_gpu(w.states, k + 1)
    valid, _ = rb.validate_edges(w.states, edges)
    w.edges = np.ascontiguousarray(edges[valid], dtype=np.int32)
    vc = rb.vertex_caches(w.states)
    ec = rb.edge_caches(w.states, w.edges)
    # (explicit weights: the restatement sums the very numbers the library does)
    w.weights = _distance_rows(w.eng, w.states[w.edges[:, 0]], w.states[w.edges[:, 1]])
    w.prm = irt.VoxelCachedLazyPRM(w.chk, w.states, w.edges, weights=w.weights)
    w.prm.set_caches(vc, ec)
    w.prm.set_tips(vc["tips"])
    w.tips = vc["tips"]
    # the environment changes: the same spheres and more
    w.vox, _ = W.reach_environment(seed=7, n_spheres=query_spheres, N=N)
    w.prm.set_obstacles(w.vox)
    w.wmap, w.eid = {}, {}
    for e, ((a, b), x) in enumerate(zip(w.edges, w.weights)):
        w.wmap[(int(a), int(b))] = w.wmap[(int(b), int(a))] = x
        w.eid[(int(a), int(b))] = w.eid[(int(b), int(a))] = e
    return w


@pytest.fixture(scope="module")
def world1(irt):
    return _world(irt, irt.workloads.robot_config1(), 64, 400, 6, 12, 72)


@pytest.fixture(scope="module")
def world3(irt):
    base = irt.workloads.robot_config3()
    robot = irt.TendonRobot(tendons=base.tendons, specs=base.specs, enable_rotation=True)
    return _world(irt, robot, 256, 400, 6, 12, 72)


def _distance_rows(eng, a, b):
    """CompoundStateSpace::distance row by row as the header states it: the tension differences squared and summed left to right
    (tests/state_metric_reference.py)"""
    return distances(*eng.state_layout(), *eng.space_weights(), a, b)


def _mv_args(mv):
    return mv.min_tension_change, mv.min_rotation_change, mv.min_retraction_change


def _pieces(w, states, direction, k, max_distance=np.inf):
    """rules A1 - A3 from validate_batch, nearest_states and validate_edges"""
    valid = w.eng.validate_batch(states, want_tips=False, want_flags=False)["valid"]
    idx, dist = w.prm.nearest_states(states, k, max_distance)
    idx[~valid] = -1
    dist[~valid] = np.inf
    ok = np.zeros(idx.shape, dtype=bool)
    live = np.argwhere(idx >= 0)
    if len(live):
        x, v = states[live[:, 0]], w.states[idx[live[:, 0], live[:, 1]]]
        a, b = (x, v) if direction == "out" else (v, x)
        ok[live[:, 0], live[:, 1]] = w.eng.validate_edges(a, b, *_mv_args(w.mv))["valid"]
    return dict(valid=valid, vertices=idx, cost=dist, edge_ok=ok)


def _same_attach(got, want, what):
    assert np.array_equal(got["valid"], want["valid"]), what
    assert np.array_equal(got["vertices"], want["vertices"]), what
    assert np.array_equal(got["cost"].view(np.uint64), want["cost"].view(np.uint64)), what
    assert np.array_equal(got["edge_ok"], want["edge_ok"]), (what, np.argwhere(got["edge_ok"] != want["edge_ok"])[:5])


def _query_states(w, n, seed):
    """random states of the space (some collide), a few of them roadmap vertices"""
    st = np.array(w.W.random_states(w.robot, n, seed=seed))
    st[5::17] = w.states[np.arange(len(st[5::17])) * 7 % len(w.states)]
    return np.ascontiguousarray(st)


@pytest.mark.parametrize("direction", ["out", "in"])
@pytest.mark.parametrize("which", ["world1", "world3"])
def test_attach_equals_the_pieces(request, which, direction):
    w = request.getfixturevalue(which)
    st = _query_states(w, 130, seed=5)
    valid = w.eng.validate_batch(st, want_tips=False, want_flags=False)["valid"]
    assert valid.any() and not valid.all()                              # the batch mixes valid and colliding states
    for k in (1, 5, 64):
        want = _pieces(w, st, direction, k)
        for n in (1, 63, 64, 65, 130):
            got = w.prm.attach_states(st[:n], direction, k=k, motion_validator=w.mv)
            _same_attach(got, {key: x[:n] for key, x in want.items()}, (k, n))
        assert got["n_domain_errors"] == 0 and (got["n_fk"][~got["edge_ok"] & (got["vertices"] < 0)] == 0).all()
    # 63 / 64 / 65 live slots exactly: valid states, one neighbour each
    good = st[valid][:65]
    assert len(good) == 65
    want = _pieces(w, good, direction, 1)
    assert (want["vertices"] >= 0).all()
    for n in (63, 64, 65):
        _same_attach(w.prm.attach_states(good[:n], direction, k=1, motion_validator=w.mv), {key: x[:n] for key, x in want.items()}, n)
    # a bound that leaves some rows empty
    bound = float(np.median(_pieces(w, good, direction, 1)["cost"][:, 0]))
    want = _pieces(w, st, direction, 5, bound)
    rows = (want["vertices"] >= 0).any(axis=1)
    assert rows[valid].any() and not rows[valid].all()
    _same_attach(w.prm.attach_states(st, direction, k=5, max_distance=bound, motion_validator=w.mv), want, "bound")
    # every state invalid: no live slot at all
    bad = st[~valid]
    got = w.prm.attach_states(bad, direction, k=5, motion_validator=w.mv)
    assert not got["valid"].any() and (got["vertices"] == -1).all() and np.isinf(got["cost"]).all() and not got["edge_ok"].any()
    # rows do not depend on the order of the batch
    perm = np.random.default_rng(1).permutation(len(st))
    want = _pieces(w, st, direction, 5)
    got = w.prm.attach_states(st[perm], direction, k=5, motion_validator=w.mv)
    _same_attach(got, {key: x[perm] for key, x in want.items()}, "order")


@pytest.mark.parametrize("direction", ["out", "in"])
def test_attach_sample_counts_are_the_indexed_edge_call_s(world3, direction):
    """rule A4: n_fk per live slot is what validate_edges_indexed counts for the slot's pair over [roadmap states | query states]; the
    other slots took no sample"""
    w = world3
    st = _query_states(w, 130, seed=5)
    got = w.prm.attach_states(st, direction, k=5, motion_validator=w.mv)
    live = np.argwhere(got["vertices"] >= 0)                            # (in slot order)
    V = len(w.states)
    q, v = V + live[:, 0], got["vertices"][live[:, 0], live[:, 1]]
    pairs = np.stack([q, v] if direction == "out" else [v, q], axis=1).astype(np.int32)
    want = w.eng.validate_edges_indexed(np.vstack([w.states, st]), pairs, *_mv_args(w.mv))
    n_fk = np.zeros_like(got["n_fk"])
    n_fk[live[:, 0], live[:, 1]] = want["n_fk"]
    assert (want["n_fk"] > 0).any()
    assert np.array_equal(got["n_fk"], n_fk)
    assert np.array_equal(got["edge_ok"][live[:, 0], live[:, 1]], want["valid"]) and got["n_domain_errors"] == want["n_domain_errors"]


def test_attach_with_k_beyond_the_valid_vertices(world1):
    w = world1
    st = _query_states(w, 40, seed=6)
    keep = np.full(len(w.states), 2, dtype=np.uint8)
    w.prm.revalidate()
    vs, _ = w.prm.validity()
    keep[np.flatnonzero(vs == 1)[:20]] = 1
    try:
        w.prm.set_validity(vertex_status=keep)
        for direction in ("out", "in"):
            want = _pieces(w, st, direction, 64)
            assert ((want["vertices"] >= 0).sum(axis=1)[want["valid"]] == 20).all()
            _same_attach(w.prm.attach_states(st, direction, k=64, motion_validator=w.mv), want, direction)
    finally:
        w.prm.clearValidity()


@pytest.mark.parametrize("direction", ["out", "in"])
def test_attach_dev_gives_the_same_bits(world3, direction):
    import torch
    w = world3
    st = _query_states(w, 130, seed=7)
    n, k, dev = len(st), 5, "cuda:%d" % w.eng.device
    want = w.prm.attach_states(st, direction, k=k, motion_validator=w.mv)
    d_st = torch.from_numpy(st).to(dev)
    d_valid, d_ok = torch.zeros(n, dtype=torch.uint8, device=dev), torch.zeros((n, k), dtype=torch.uint8, device=dev)
    d_idx, d_cost = torch.zeros((n, k), dtype=torch.int32, device=dev), torch.zeros((n, k), dtype=torch.float64, device=dev)
    d_nfk = torch.zeros((n, k), dtype=torch.int32, device=dev)
    w.prm.attach_states_dev(d_st, n, d_valid, d_idx, d_cost, d_ok, d_nfk, direction=direction, k=k, motion_validator=w.mv)
    got = dict(valid=d_valid.cpu().numpy().astype(bool), vertices=d_idx.cpu().numpy(), cost=d_cost.cpu().numpy(),
               edge_ok=d_ok.cpu().numpy().astype(bool))
    _same_attach(got, want, "dev")
    assert np.array_equal(d_nfk.cpu().numpy(), want["n_fk"])


# ---- the seeded search ------------------------------------------------------------------------------------------------------------
def _seed_lists(w, n_queries, seed):
    rng = np.random.default_rng(seed)
    V = len(w.states)
    src, dst = [], []
    for _ in range(n_queries):
        for lists in (src, dst):
            m = int(rng.integers(0, 9))
            lists.append((rng.integers(0, V, m).astype(np.int32), rng.uniform(0.0, 2.0, m)))
    direct = np.where(np.arange(n_queries) % 3 == 0, rng.uniform(0.0, 8.0, n_queries), np.inf)
    return src, dst, direct


def _search_stats0(prm):
    ss = (ctypes.c_int64 * 8)()
    prm._check(prm.lib.tr_roadmap_search_stats(prm._rm, ss))
    return int(ss[0])


def _check_seeded(w, got, want, src, dst, direct):
    assert np.array_equal(got["status"], want["status"])
    assert np.array_equal(got["src_pick"], want["src_pick"]) and np.array_equal(got["dst_pick"], want["dst_pick"])
    assert np.array_equal(got["direct"], want["direct"])
    solved = want["status"] == SOLVED
    assert np.isinf(got["cost"][~solved]).all()
    # two summation orders over at most V additions differ by at most V 2^-53 ~ 4e-14 relative
    np.testing.assert_allclose(got["cost"][solved], want["cost"][solved], rtol=1e-12, atol=0)
    vs, es = w.prm.validity()
    for q in np.flatnonzero(solved):
        p = got["paths"][q]
        if want["direct"][q]:
            assert len(p) == 0 and got["cost"][q] == direct[q]
            continue
        i, j = got["src_pick"][q], got["dst_pick"][q]
        assert p[0] == src[q][0][i] and p[-1] == dst[q][0][j]
        assert got["cost"][q] == ref.path_cost(lambda a, b: w.wmap[(a, b)], src[q][1][i], p, dst[q][1][j])       # bit for bit
        assert (vs[p] == 1).all()
        assert all(es[w.eid[(int(a), int(b))]] == 1 for a, b in zip(p[:-1], p[1:]))


def _same_answers(a, b):
    for key in ("status", "src_pick", "dst_pick", "direct", "path_offsets", "path_vertices"):
        assert np.array_equal(a[key], b[key]), key
    assert np.array_equal(a["cost"].view(np.uint64), b["cost"].view(np.uint64))


def test_seeded_search_equals_the_restatement(world1, monkeypatch):
    w = world1
    src, dst, direct = _seed_lists(w, 64, seed=11)
    w.prm.revalidate()
    vs, es = w.prm.validity()
    assert (vs == 2).any() and (es == 2).any()                          # the changed environment took items out of the graph
    want = ref.solve_seeded(len(w.states), w.edges, w.weights, vs == 1, es == 1, src, dst, direct)
    assert want["direct"].any() and (want["status"] == NO_PATH).any() and ((want["status"] == SOLVED) & ~want["direct"]).any()
    known = w.prm.solve_seeded(src, dst, direct)
    _check_seeded(w, known, want, src, dst, direct)
    assert _search_stats0(w.prm) == 0                                   # no search of this call ran in roadmap_astar
    # from unknown validity, lazily and with the eager rules forbidden
    w.prm.clearValidity()
    lazy = w.prm.solve_seeded(src, dst, direct)
    assert w.prm.stats["items_checked"] > 0
    _same_answers(lazy, known)
    _check_seeded(w, lazy, want, src, dst, direct)
    w.prm.clearValidity()
    monkeypatch.setenv("TENDON_HIP_LAZY_ONLY", "1")
    _same_answers(w.prm.solve_seeded(src, dst, direct), known)
    monkeypatch.delenv("TENDON_HIP_LAZY_ONLY")
    # with and without landmark tables
    for n_landmarks in (0, 16):
        w.prm.prepare(n_landmarks)
        w.prm.clearValidity()
        _same_answers(w.prm.solve_seeded(src, dst, direct), known)
    # query by query
    w.prm.clearValidity()
    for q in range(len(src)):
        one = w.prm.solve_seeded(src[q:q + 1], dst[q:q + 1], direct[q:q + 1])
        for key in ("status", "src_pick", "dst_pick", "direct"):
            assert one[key][0] == known[key][q], (key, q)
        assert one["cost"].view(np.uint64)[0] == known["cost"].view(np.uint64)[q]
        assert np.array_equal(one["paths"][0], known["paths"][q])
    # CSR triples are the same call
    off = np.concatenate([[0], np.cumsum([len(v) for v, _ in src])])
    csr = (off, np.concatenate([v for v, _ in src]), np.concatenate([c for _, c in src]))
    _same_answers(w.prm.solve_seeded(csr, dst, direct), known)


def test_seeded_search_under_the_expansion_report(world1, monkeypatch, tmp_path, capfd):
    """TENDON_HIP_SEARCH_HIST with a path: a seeded query has seed lists and no start / goal vertex, so the per-search file lines (whose
    columns describe a vertex pair) are not written; the summary on stderr counts the seeded searches' expansions."""
    import re
    w = world1
    src, dst, direct = _seed_lists(w, 64, seed=11)
    w.prm.clearValidity()
    known = w.prm.solve_seeded(src, dst, direct)
    path = tmp_path / "hist.txt"
    monkeypatch.setenv("TENDON_HIP_SEARCH_HIST", str(path))
    capfd.readouterr()
    w.prm.clearValidity()
    _same_answers(w.prm.solve_seeded(src, dst, direct), known)
    err = capfd.readouterr().err
    found = [(int(a), int(b)) for a, b in re.findall(r"  found: (\d+) searches, (\d+) expansions", err)]
    assert found and found[0][0] > 0 and found[0][1] > 0, err            # (the first round: every query with a target is searched)
    assert not path.exists() or path.read_text() == ""
    s, g = _state_queries(w, 16, 31)
    w.prm.clearValidity()
    want = w.prm.solve_states(s, g, k=5, motion_validator=w.mv)
    monkeypatch.delenv("TENDON_HIP_SEARCH_HIST")
    w.prm.clearValidity()
    got = w.prm.solve_states(s, g, k=5, motion_validator=w.mv)
    for key in ("status", "direct", "src_pick", "dst_pick", "path_vertices"):
        assert np.array_equal(got[key], want[key]), key


# ---- state-to-state queries --------------------------------------------------------------------------------------------------------
def _state_queries(w, n, seed):
    """starts and goals: random states (some collide), some of them roadmap vertices, and some goals so close to their start that the
    direct rule applies"""
    rng = np.random.default_rng(seed)
    s, g = _query_states(w, n, seed), _query_states(w, n, seed + 1000)
    near = np.arange(3, n, 4)
    g[near] = s[near]
    nt = w.eng.state_layout()[0]
    g[near, :nt] = np.clip(s[near, :nt] + rng.normal(size=(len(near), nt)) * 0.15, 0.0, None)
    return s, np.ascontiguousarray(g)


def _restate_solve_states(w, s, g, k, max_distance):
    """rules T1 - T3 from attach_states, validate_edges and the restatement of the seeded search"""
    n = len(s)
    out_, in_ = w.prm.attach_states(s, "out", k=k, max_distance=max_distance, motion_validator=w.mv), \
        w.prm.attach_states(g, "in", k=k, max_distance=max_distance, motion_validator=w.mv)
    d = _distance_rows(w.eng, s, g)
    both = out_["valid"] & in_["valid"]
    tried = both & (d <= np.maximum(out_["cost"][:, k - 1], in_["cost"][:, k - 1])) & (d <= max_distance)
    direct = np.full(n, np.inf)
    if tried.any():
        ok = w.eng.validate_edges(s[tried], g[tried], *_mv_args(w.mv))["valid"]
        direct[np.flatnonzero(tried)[ok]] = d[np.flatnonzero(tried)[ok]]
    slots = [[np.flatnonzero(a["edge_ok"][q]) for q in range(n)] for a in (out_, in_)]
    src = [(out_["vertices"][q][slots[0][q]], out_["cost"][q][slots[0][q]]) for q in range(n)]
    dst = [(in_["vertices"][q][slots[1][q]], in_["cost"][q][slots[1][q]]) for q in range(n)]
    w.prm.revalidate()
    vs, es = w.prm.validity()
    want = ref.solve_seeded(len(w.states), w.edges, w.weights, vs == 1, es == 1, src, dst, direct)
    want["status"] = np.where(~out_["valid"], INVALID_START, np.where(~in_["valid"], INVALID_GOAL, want["status"])).astype(np.int32)
    solved = want["status"] == SOLVED
    want["cost"] = np.where(solved, want["cost"], np.inf)
    for key, side in (("src_pick", 0), ("dst_pick", 1)):
        want[key] = np.array([slots[side][q][want[key][q]] if solved[q] and want[key][q] >= 0 else -1 for q in range(n)], dtype=np.int32)
    want["start_vertex"] = np.array([out_["vertices"][q][want["src_pick"][q]] if want["src_pick"][q] >= 0 else -1 for q in range(n)], dtype=np.int32)
    want["goal_vertex"] = np.array([in_["vertices"][q][want["dst_pick"][q]] if want["dst_pick"][q] >= 0 else -1 for q in range(n)], dtype=np.int32)
    want["direct"] = want["direct"] & solved
    return want


# world, batch seed, k, max_distance: chosen on the device so that every class below is met on both worlds (counts in CHANGELOG.md)
STATE_CASES = [("world1", 31, 5, 3.0), ("world3", 32, 5, 6.0), ("world3", 32, 5, np.inf)]


@pytest.mark.parametrize("which,seed,k,max_distance", STATE_CASES)
def test_solve_states_equals_attach_plus_restatement(request, which, seed, k, max_distance):
    w = request.getfixturevalue(which)
    s, g = _state_queries(w, 96, seed)
    want = _restate_solve_states(w, s, g, k, max_distance)
    # the inputs exercise the rule: a seed other than the nearest at either end, the direct edge, no path, the invalid ends
    off_nearest = (want["status"] == SOLVED) & ~want["direct"] & ((want["src_pick"] > 0) | (want["dst_pick"] > 0))
    counts = dict(other_seed=int(off_nearest.sum()), direct=int(want["direct"].sum()), no_path=int((want["status"] == NO_PATH).sum()),
                  invalid_start=int((want["status"] == INVALID_START).sum()), invalid_goal=int((want["status"] == INVALID_GOAL).sum()))
    print(which, counts)
    assert all(c > 0 for c in counts.values()), counts
    w.prm.clearValidity()
    got = w.prm.solve_states(s, g, k=k, max_distance=max_distance, motion_validator=w.mv)
    for key in ("status", "direct", "src_pick", "dst_pick", "start_vertex", "goal_vertex"):
        assert np.array_equal(got[key], want[key]), (key, np.flatnonzero(got[key] != want[key])[:5])
    solved = want["status"] == SOLVED
    assert np.isinf(got["cost"][~solved]).all()
    np.testing.assert_allclose(got["cost"][solved], want["cost"][solved], rtol=1e-12, atol=0)
    for q in np.flatnonzero(solved):
        p = got["paths"][q]
        if want["direct"][q]:
            assert len(p) == 0
        else:
            assert p[0] == got["start_vertex"][q] and p[-1] == got["goal_vertex"][q]
    prof = w.prm.state_query_profile()
    assert all(v >= 0 for v in prof.values()) and prof["nearest_ms"] > 0


# ---- chains from states ------------------------------------------------------------------------------------------------------------
def _waypoints(w, chains, hops, seed):
    rng = np.random.default_rng(seed)
    vs, _ = w.prm.validity()
    ok = np.flatnonzero(vs == 1)
    return w.tips[rng.choice(ok, (chains, hops))] + rng.normal(size=(chains, hops, 3)) * 0.002


def test_chains_from_a_roadmap_vertex_solve_what_chained_plan_solves(irt, world3):
    w = world3
    w.prm.revalidate()
    vs, _ = w.prm.validity()
    start = np.flatnonzero(vs == 1)[:8].astype(np.int32)
    wp = _waypoints(w, len(start), 2, seed=41)
    old = irt.chained_plan(w.prm, start, wp, motion_validator=w.mv)
    new = irt.chained_plan_from_states(w.prm, w.states[start], wp, motion_validator=w.mv)
    assert old["solved"].any()
    assert new["solved"][old["solved"]].all()
    for ho, hn in zip(old["hops"], new["hops"]):
        both = np.isfinite(ho["total_cost"]) & np.isfinite(hn["total_cost"]) & np.all(ho["start_state"] == hn["start_state"], axis=1)
        # (the same path summed in two orders: a few ulp)
        assert (hn["total_cost"][both] <= ho["total_cost"][both] * (1 + 1e-12)).all()


def test_chains_from_off_roadmap_states(irt, world3):
    w = world3
    st = _query_states(w, 64, seed=43)
    st = st[w.eng.validate_batch(st, want_tips=False, want_flags=False)["valid"]][:8]
    wp = _waypoints(w, len(st), 2, seed=44)
    res = irt.chained_plan_from_states(w.prm, st, wp, motion_validator=w.mv)
    assert res["hops"][0]["total_cost"][np.isfinite(res["hops"][0]["total_cost"])].size > 0
    vs, es = w.prm.validity()
    for hop in res["hops"]:
        for j, c in enumerate(hop["chains"]):
            if hop["status"][j] != SOLVED:
                continue
            p = hop["paths"][j]
            assert p[0] == hop["start_vertex"][c] and p[-1] == hop["neighbor_vertex"][j]
            ends = w.eng.validate_edges(np.stack([hop["start_state"][c], w.states[p[-1]]]), np.stack([w.states[p[0]], hop["controls"][j]]),
                                        *_mv_args(w.mv))["valid"]
            assert ends.all()
            assert (vs[p] == 1).all() and all(es[w.eid[(int(a), int(b))]] == 1 for a, b in zip(p[:-1], p[1:]))


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals(irt, world1):
    w = world1
    L = irt._lib
    st = _query_states(w, 4, seed=3)
    one = [(np.array([0], np.int32), np.array([0.0]))]
    with pytest.raises(L.OutOfRange):
        w.prm.solve_seeded([(np.array([len(w.states)], np.int32), np.array([0.0]))], one)
    with pytest.raises(L.OutOfRange):
        w.prm.solve_seeded(one, [(np.array([-1], np.int32), np.array([0.0]))])
    for bad in (-0.5, np.inf, np.nan):
        with pytest.raises(L.InvalidArgument):
            w.prm.solve_seeded([(np.array([0], np.int32), np.array([bad]))], one)
    with pytest.raises(L.InvalidArgument):
        w.prm.solve_seeded(one, one, direct_cost=np.array([-1.0]))
    with pytest.raises(L.InvalidArgument):
        w.prm.attach_states(st, "out", k=65)
    with pytest.raises(L.InvalidArgument):
        w.prm.attach_states(st, "sideways")
    # no tips: the states have not been uploaded
    bare = irt.VoxelCachedLazyPRM(w.chk, w.states, w.edges)
    for call in (lambda: bare.attach_states(st), lambda: bare.solve_states(st, st)):
        with pytest.raises(L.InvalidArgument):
            call()
    # an empty batch is fine
    assert w.prm.attach_states(np.zeros((0, st.shape[1])))["vertices"].shape == (0, 10)
    assert len(w.prm.solve_states(np.zeros((0, st.shape[1])), np.zeros((0, st.shape[1])))["status"]) == 0
    assert len(w.prm.solve_seeded([], [])["status"]) == 0
    # a checker with loads
    w.chk.set_loads(wrench=np.array([0.0, 0.0, -0.05, 0.0, 0.0, 0.0]))
    try:
        for call in (lambda: w.prm.attach_states(st), lambda: w.prm.solve_seeded(one, one), lambda: w.prm.solve_states(st, st),
                     lambda: irt.chained_plan_from_states(w.prm, st[:1], np.zeros((1, 1, 3)))):
            with pytest.raises(L.Unsupported):
                call()
    finally:
        w.chk.clear_loads()
