"""The accurate connection rule of the tip queries (RMAP_IK_ACCURATE: tr_roadmap_ik_batch_connect / _solve_tips_connect; connect_k on
roadmap_ik_batch, solve_to_tips, chained_plan): connect_k = 0 is the one-edge rule bit for bit; connect_k > 0 equals a restatement of
rules 1 - 5' of include/tendon_hip.h over the single pieces, reaches whatever the one-edge rule reaches and more, does not depend on
the batch, holds up against the oracle, and feeds the roadmap query and the chains."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REACHED, CLOSEST, NO_NEIGHBOR = 0, 1, 2
KEYS = ("controls", "tip", "error", "neighbor_vertex", "outcome", "last_valid_t")


def _free_space(irt):
    vox = irt.VoxelOctree(256)
    vox.set_xlim(-0.25, 0.25); vox.set_ylim(-0.25, 0.25); vox.set_zlim(-0.25, 0.25)
    return vox


def _d2(tips, r):
    d = tips - r
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def _nearest(tips, ok, requests, k):
    """numpy's (d2, index) order over the vertices `ok` marks: (n, k) indices padded with -1"""
    cand = np.flatnonzero(ok)
    idx = np.full((len(requests), k), -1, dtype=np.int32)
    for q, r in enumerate(requests):
        order = np.argsort(_d2(tips[cand], r), kind="stable")[:k]
        idx[q, :len(order)] = cand[order]
    return idx


def _obstacle_roadmap(irt, n_vertices=2500, k=6, seed=21, n_spheres=256):
    """The roadmap of tests/test_gpu_tip_queries.py among 256 spheres instead of 64.  Requests that only the accurate rule reaches are
    rare here -- IK ends close to the vertex it started from, so the one edge is short and seldom the one that collides: of 2 048
    requests at k = 1 none with 64 spheres, 4 with 256 (2 with 384, 1 with 640 and with 896)."""
    W = irt.workloads
    robot = W.robot_config3()
    vox, _ = W.reach_environment(seed=7, n_spheres=n_spheres)
    chk = irt.VoxelBackboneValidityChecker(robot, irt.VoxelEnvironment(), vox)
    mv = irt.VoxelBackboneMotionValidator(chk)
    rb = irt.RoadmapBuilder(chk, mv, seed=seed)
    states, _ = rb.sample_valid_vertices(n_vertices, batch=8192)
    edges = rb.knn_edges(states, k)
    valid, _ = rb.validate_edges(states, edges)
    edges = edges[valid]
    vc = rb.vertex_caches(states)
    ec = rb.edge_caches(states, edges)
    prm = irt.VoxelCachedLazyPRM(chk, states, edges)
    prm.set_caches(vc, ec)
    prm.set_tips(vc["tips"])
    return robot, vox, chk, mv, states, edges, vc, ec, prm


def _requests(tips, n, seed):
    rng = np.random.default_rng(seed)
    req = tips[rng.integers(0, len(tips), n)] + rng.normal(size=(n, 3)) * 0.003
    req[n // 2:] = rng.uniform(-0.12, 0.12, (n - n // 2, 3)) + np.array([0.0, 0.0, 0.1])      # anywhere in the workspace: many out of reach or walled in
    return req


@pytest.fixture(scope="module")
def world(irt):
    return _obstacle_roadmap(irt)


def _restate(irt, prm, tips, requests, k, tolerance, kc, max_distance=np.inf):
    """Rules 1 - 5' over the single pieces -> (result, stats)"""
    eng = prm.engine
    vstat, _ = prm.validity()
    N = _nearest(tips, vstat == 1, requests, k)
    n, S = len(requests), prm.states.shape[1]
    out = dict(controls=np.full((n, S), np.nan), tip=np.full((n, 3), np.nan), error=np.full(n, np.nan), neighbor_vertex=np.full(n, -1, np.int32),
               ik_vertex=np.full(n, -1, np.int32), outcome=np.full(n, NO_NEIGHBOR, np.int32), last_valid_t=np.full(n, np.nan))
    stats = dict(pairs_checked=0, reached=0, moved=0, gained=0)
    slots = np.argwhere(N >= 0)
    if len(slots) == 0:
        return out, stats
    nv = N[slots[:, 0], slots[:, 1]]
    ik = eng.ik_batch(prm.states[nv], requests[slots[:, 0]], stop_threshold_err=tolerance)
    C, _ = prm.nearest_states(ik["state"], kc, max_distance)
    pair_slot, pair_src = [], []
    for s in range(len(slots)):
        srcs = [int(c) for c in C[s] if c >= 0]
        if int(nv[s]) not in srcs:
            srcs.append(int(nv[s]))                                    # the IK vertex last, when its state-space neighbours do not hold it
        pair_slot += [s] * len(srcs)
        pair_src += srcs
    pair_slot, pair_src = np.array(pair_slot), np.array(pair_src)
    a, b = prm.states[pair_src], ik["state"][pair_slot]
    ev = eng.validate_edges_last_valid(a, b)
    g = irt.roadmap.interpolate_states(eng, a, b, ev["last_valid_t"])
    gtip, _ = eng.fk_tips(g)
    stats["pairs_checked"] = len(pair_src)
    reaches = (ik["error"][pair_slot] < tolerance) & np.asarray(ev["valid"], dtype=bool)
    for q in range(n):
        mine = np.flatnonzero(slots[pair_slot, 0] == q)                # in (slot, source) order
        if len(mine) == 0:
            continue
        hit = mine[reaches[mine]]
        if len(hit):
            p = hit[0]
            s = pair_slot[p]
            out["controls"][q], out["tip"][q], out["error"][q], out["last_valid_t"][q] = ik["state"][s], ik["tip"][s], ik["error"][s], 1.0
            out["outcome"][q] = REACHED
            stats["reached"] += 1
            stats["gained"] += not (reaches[mine] & (pair_src[mine] == nv[pair_slot[mine]])).any()
        else:
            d = gtip[mine] - requests[q]
            e = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
            p = mine[int(np.argmin(e))]                                 # (argmin: the first of equal values)
            out["controls"][q], out["tip"][q], out["error"][q], out["last_valid_t"][q] = g[p], gtip[p], e.min(), ev["last_valid_t"][p]
            out["outcome"][q] = CLOSEST
        out["neighbor_vertex"][q], out["ik_vertex"][q] = pair_src[p], nv[pair_slot[p]]
        stats["moved"] += pair_src[p] != nv[pair_slot[p]]
    return out, stats


def _same_bits(a, b, keys=KEYS):
    for key in keys:
        x, y = np.ascontiguousarray(a[key]), np.ascontiguousarray(b[key])
        assert x.dtype == y.dtype and x.shape == y.shape, key
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), (key, np.flatnonzero((x != y).reshape(len(x), -1).any(1))[:5])


def _connect_entry(prm, requests, tolerance, k, mv, k_connect):
    """tr_roadmap_ik_batch_connect itself (the package calls the plain entry point when connect_k is 0)"""
    C, L = ctypes, prm._L
    prm_, sp = prm._tip_params(k, tolerance, None, mv)
    r = np.ascontiguousarray(requests, dtype=np.float64)
    o = prm._tip_outputs(len(r))
    o["ik_vertex"] = np.empty(len(r), dtype=np.int32)
    cp = L.TrTipConnectParams(k_connect, np.inf)
    dp, i32 = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    prm._check(prm.lib.tr_roadmap_ik_batch_connect(
        prm._rm, C.byref(sp), C.byref(prm_), C.byref(cp), r.ctypes.data_as(dp), len(r), o["controls"].ctypes.data_as(dp), o["tip"].ctypes.data_as(dp),
        o["error"].ctypes.data_as(dp), o["neighbor_vertex"].ctypes.data_as(i32), o["ik_vertex"].ctypes.data_as(i32), o["outcome"].ctypes.data_as(i32),
        o["last_valid_t"].ctypes.data_as(dp)))
    o["connect_stats"] = prm._connect_stats()
    return o


def test_connect_k_zero_is_the_plain_rule_bit_for_bit(irt, world):
    robot, vox, chk, mv, states, edges, vc, ec, prm = world
    requests = _requests(vc["tips"], 256, seed=5)
    plain = prm.roadmap_ik_batch(requests, motion_validator=mv)
    same = prm.roadmap_ik_batch(requests, motion_validator=mv, connect_k=0)
    assert set(same) == set(plain)
    _same_bits(same, plain)
    entry = _connect_entry(prm, requests, 1e-4, 5, mv, 0)
    _same_bits(entry, plain)
    assert np.array_equal(entry["ik_vertex"], plain["neighbor_vertex"])
    st = entry["connect_stats"]
    assert st["reached"] == (plain["outcome"] == REACHED).sum() and st["moved"] == 0 and st["gained"] == 0 and st["pairs_checked"] == 256 * 5


def test_batch_equals_composition_of_the_single_pieces(irt, world):
    robot, vox, chk, mv, states, edges, vc, ec, prm = world
    requests = _requests(vc["tips"], 512, seed=5)
    for k, tol in ((5, 1e-4), (3, 1e-5)):
        got = prm.roadmap_ik_batch(requests, tolerance=tol, k=k, motion_validator=mv, connect_k=6)
        want, stats = _restate(irt, prm, vc["tips"], requests, k, tol, 6)
        _same_bits(got, want, KEYS + ("ik_vertex",))
        assert got["connect_stats"] == stats
        print("k", k, "tolerance", tol, "outcomes", np.bincount(got["outcome"], minlength=3), "stats", stats)
        assert (got["outcome"] == REACHED).any() and (got["outcome"] == CLOSEST).any()        # both branches of the rule
        assert stats["moved"] > 0
    # a bound on the source search: the sources beyond it are dropped, the IK vertex stays
    d_med = float(np.median(prm.nearest_states(states[:200], 4)[1][:, 3]))
    got = prm.roadmap_ik_batch(requests[:128], motion_validator=mv, connect_k=6, connect_max_distance=d_med)
    want, stats = _restate(irt, prm, vc["tips"], requests[:128], 5, 1e-4, 6, max_distance=d_med)
    _same_bits(got, want, KEYS + ("ik_vertex",))
    assert got["connect_stats"] == stats and stats["pairs_checked"] < 128 * 5 * 6
    # a request's answer does not depend on the batch it is in
    got = prm.roadmap_ik_batch(requests, motion_validator=mv, connect_k=6)
    for q in (0, 17, 255, 300, 511):
        alone = prm.roadmap_ik_batch(requests[q], motion_validator=mv, connect_k=6)
        _same_bits(alone, {key: got[key][q:q + 1] for key in KEYS + ("ik_vertex",)}, KEYS + ("ik_vertex",))
    prof = prm.tip_query_profile()
    assert prof["ik_rounds"] > 0 and prof["nearest_ms"] > 0 and prof["solve_ms"] == 0


def test_accurate_rule_reaches_what_the_plain_rule_reaches_and_more(irt, world):
    robot, vox, chk, mv, states, edges, vc, ec, prm = world
    requests = _requests(vc["tips"], 2048, seed=5)
    gained = {}
    for k in (1, 5):
        plain = prm.roadmap_ik_batch(requests, k=k, motion_validator=mv)
        acc = prm.roadmap_ik_batch(requests, k=k, motion_validator=mv, connect_k=6)
        pr, ar = plain["outcome"] == REACHED, acc["outcome"] == REACHED
        assert (ar | ~pr).all()                                         # REACHED stays REACHED
        both = (plain["outcome"] == CLOSEST) & (acc["outcome"] == CLOSEST)
        assert both.any() and (acc["error"][both] <= plain["error"][both]).all()
        st = acc["connect_stats"]
        assert st["gained"] == (ar & ~pr).sum() and st["reached"] == ar.sum()
        assert st["moved"] == (acc["neighbor_vertex"] != acc["ik_vertex"]).sum()
        gained[k] = st["gained"]
        print("k", k, "plain REACHED", int(pr.sum()), "accurate REACHED", int(ar.sum()), "stats", st)
    assert gained[1] > 0                                                # requests only the accurate rule reaches


def _wall_in(irt, og, req, h=0.006):
    """the block of cells around a request that tests/cpp/shim_ik_test.cpp builds -> the package's octree (and the oracle's grid)"""
    dx = 0.5 / 256
    lo = [int(np.floor((req[a] - h + 0.25) / dx)) for a in range(3)]
    hi = [int(np.floor((req[a] + h + 0.25) / dx)) for a in range(3)]
    vox = _free_space(irt)
    for ix in range(lo[0], hi[0] + 1):
        for iy in range(lo[1], hi[1] + 1):
            for iz in range(lo[2], hi[2] + 1):
                vox.set_cell(ix, iy, iz)
                og.set_cell(ix, iy, iz)
    return vox


def test_answers_hold_up_against_the_oracle(irt, orc, helpers):
    W = irt.workloads
    robot = W.robot_config3()
    vox = _free_space(irt)
    chk = irt.VoxelBackboneValidityChecker(robot, irt.VoxelEnvironment(), vox)
    mv = irt.VoxelBackboneMotionValidator(chk)
    rb = irt.RoadmapBuilder(chk, mv, seed=5)
    states = W.random_states(robot, 2000, seed=21, tau_max=15.0)       # (the roadmap of tests/test_gpu_ik.py)
    edges = rb.knn_edges_gpu(states, 6)
    vc = rb.vertex_caches(states)
    ec = rb.edge_caches(states, edges)
    tips = vc["tips"]
    prm = irt.VoxelCachedLazyPRM(chk, states, edges)
    prm.set_caches(vc, dict(ec, present=ec["fully_valid"]))             # (a random state need not have a valid shape: no cache, never a neighbour)
    prm.set_tips(tips, present=vc["shape_valid"])
    orb, og = helpers.oracle_robot(orc, robot), helpers.oracle_grid(orc, vox)
    tol, k = 1e-4, 5
    js = np.concatenate([[123], np.random.default_rng(2).choice(2000, 63, replace=False)])
    requests = tips[js] + np.array([0.002, -0.001, 0.0015])

    def check(res, requests, og):
        vstat, _ = prm.validity()
        N = _nearest(tips, (vstat == 1) & vc["shape_valid"], requests, k)
        for q in range(len(requests)):
            assert res["outcome"][q] in (REACHED, CLOSEST)
            ctl, nv, iv = res["controls"][q], res["neighbor_vertex"][q], res["ik_vertex"][q]
            ok, tip, _ = orc.is_valid_state(orb, og, ctl)
            assert ok, q
            assert np.abs(tip - res["tip"][q]).max() <= 1e-9
            assert abs(res["error"][q] - np.linalg.norm(tip - requests[q])) <= 1e-9
            assert iv in N[q] and vstat[nv] == 1
            # x = the IK solution from the IK vertex (its bits: test_batch_equals_composition_of_the_single_pieces)
            x = chk.engine.ik_batch(states[iv], requests[q], stop_threshold_err=tol)
            w = orc.check_motion_until_invalid(orb, og, states[nv], x["state"][0])
            if res["outcome"][q] == REACHED:
                assert res["error"][q] < tol and w["is_fully_valid"] and res["last_valid_t"][q] == 1.0
                assert np.array_equal(ctl, x["state"][0])
            else:
                assert res["last_valid_t"][q] == w["last_valid_t"]
                assert not (w["is_fully_valid"] and x["error"][0] < tol)

    free = prm.roadmap_ik_batch(requests, tolerance=tol, k=k, motion_validator=mv, connect_k=6)
    print("free space outcomes", np.bincount(free["outcome"], minlength=3), free["connect_stats"])
    assert free["outcome"][0] == REACHED
    check(free, requests, og)
    # the request walled in: every IK solution collides, the answer is a valid state short of it
    blocked = _wall_in(irt, og, requests[0])
    prm.set_obstacles(blocked)
    walled = prm.roadmap_ik_batch(requests[:8], tolerance=tol, k=k, motion_validator=mv, connect_k=6)
    assert walled["outcome"][0] == CLOSEST and walled["error"][0] > tol and walled["last_valid_t"][0] < 1.0
    check(walled, requests[:8], og)


@pytest.mark.parametrize("search", ["host", "device"])
def test_solve_to_tips_is_the_roadmap_query_plus_one_edge(irt, monkeypatch, search):
    monkeypatch.setenv("TENDON_HIP_SEARCH", search)
    W = irt.workloads
    robot, vox, chk, mv, states, edges, vc, ec, prm = _obstacle_roadmap(irt, n_spheres=64)
    new_vox, _ = W.reach_environment(seed=7, n_spheres=76)
    prm.set_obstacles(new_vox)
    n = 300
    requests = _requests(vc["tips"], n, seed=9)
    starts = np.random.default_rng(10).integers(0, len(states), n).astype(np.int32)
    res = prm.solve_to_tips(starts, requests, motion_validator=mv, connect_k=6)
    prof = prm.tip_query_profile()                                     # (of the last tip call: read before the next one)
    assert prof["solve_ms"] > 0 and prof["ik_rounds"] > 0
    ik = prm.roadmap_ik_batch(requests, motion_validator=mv, connect_k=6)
    _same_bits(res, ik, KEYS + ("ik_vertex",))
    assert res["connect_stats"] == ik["connect_stats"] and ik["connect_stats"]["moved"] > 0
    assert (res["outcome"] != NO_NEIGHBOR).all()
    conn = res["neighbor_vertex"]
    plain = prm.solveWithRoadmap(starts, conn)
    assert np.array_equal(res["status"], plain["status"])
    assert np.array_equal(res["path_vertices"], plain["path_vertices"]) and np.array_equal(res["path_offsets"], plain["path_offsets"])
    solved = res["status"] == 0
    assert solved.any() and np.isinf(res["cost"][~solved]).all()
    last = chk.engine.state_distance(states[conn], res["controls"])
    assert (np.abs(res["cost"][solved] - (plain["cost"][solved] + last[solved])) <= 1e-12).all()
    for q in np.flatnonzero(solved):
        assert res["paths"][q][0] == starts[q] and res["paths"][q][-1] == conn[q]


def test_chained_plan_connects_through_the_connection_vertex(irt, world):
    robot, vox, chk, mv, states, edges, vc, ec, prm = world
    rng = np.random.default_rng(8)
    C_, H = 24, 4
    way = vc["tips"][rng.integers(0, len(states), (C_, H))] + rng.normal(size=(C_, H, 3)) * 0.002
    start = rng.integers(0, len(states), C_)
    plan = irt.chained_plan(prm, start, way, motion_validator=mv, connect_k=6)
    assert len(plan["hops"]) == H and plan["solved"].any()
    eng = chk.engine
    alive = np.ones(C_, dtype=bool)
    prev_state, prev_vertex, on_roadmap = states[start].copy(), start.copy(), True
    moved = 0
    for hop in plan["hops"]:
        idx = np.flatnonzero(alive)
        assert np.array_equal(hop["chains"], idx) and np.array_equal(hop["start_state"][idx], prev_state[idx])
        ok = hop["status"] == 0
        # the hop starts with the reversed connecting edge: the previous goal state back to ITS connection vertex
        pre = np.zeros(len(idx)) if on_roadmap else eng.state_distance(prev_state[idx], states[prev_vertex[idx]])
        assert np.array_equal(hop["prefix_cost"][idx], pre)
        moved += int((hop["neighbor_vertex"] != hop["ik_vertex"]).sum())
        for j, c in enumerate(idx):
            if not ok[j]:
                continue
            p = hop["paths"][j]
            assert p[0] == prev_vertex[c] and p[-1] == hop["neighbor_vertex"][j]
            assert hop["total_cost"][c] == pre[j] + hop["cost"][j]
            prev_state[c], prev_vertex[c] = hop["controls"][j], hop["neighbor_vertex"][j]
        alive[idx[~ok]] = False
        on_roadmap = False
    assert np.array_equal(plan["solved"], alive) and np.array_equal(plan["final_vertex"][alive], prev_vertex[alive])
    assert moved > 0


def test_errors(irt, world):
    robot, vox, chk, mv, states, edges, vc, ec, prm = world
    requests = _requests(vc["tips"], 4, seed=1)
    for bad in (-1, 65):
        with pytest.raises(irt.InvalidArgument):
            prm.roadmap_ik_batch(requests, motion_validator=mv, connect_k=bad)
        with pytest.raises(irt.InvalidArgument):
            prm.solve_to_tips([0, 1, 2, 3], requests, motion_validator=mv, connect_k=bad)
    with pytest.raises(irt.InvalidArgument):
        prm.roadmap_ik_batch(requests, motion_validator=mv, connect_k=6, connect_max_distance=-1.0)
    with pytest.raises(irt.InvalidArgument):
        prm.roadmap_ik_batch(requests, motion_validator=mv, connect_k=6, connect_max_distance=np.nan)
    chk.set_loads(wrench=np.array([0.0, 0.0, -0.05, 0.0, 0.0, 0.0]))
    try:
        for call in (lambda: prm.roadmap_ik_batch(requests, connect_k=6), lambda: prm.solve_to_tips([0, 1, 2, 3], requests, connect_k=6),
                     lambda: irt.chained_plan(prm, [0], requests[None, :2], connect_k=6)):
            with pytest.raises(irt.Unsupported):
                call()
    finally:
        chk.clear_loads()
    assert len(prm.roadmap_ik_batch(requests, motion_validator=mv, connect_k=6)["outcome"]) == 4
