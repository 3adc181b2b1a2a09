"""Batched tip-goal queries (tr_roadmap_set_tips / _nearest_tips / _ik_batch / _solve_tips; VoxelCachedLazyPRM.set_tips,
.nearest_tips, .roadmap_ik_batch, .solve_to_tips, chained_plan): the k nearest tips against numpy bit for bit, the batch against
a restatement of its rule over the single pieces (Engine.ik_batch, the last-valid edge check, fk_tips), every answer against the
oracle, the roadmap query against solveWithRoadmap and the oracle's query loop, and the chains of chained_plan."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REACHED, CLOSEST, NO_NEIGHBOR = 0, 1, 2


def _free_space(irt):
    vox = irt.VoxelOctree(256)
    vox.set_xlim(-0.25, 0.25); vox.set_ylim(-0.25, 0.25); vox.set_zlim(-0.25, 0.25)
    return vox


def _d2(tips, r):
    d = tips - r
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def _nearest(tips, ok, requests, k):
    """numpy's (d2, index) order over the vertices `ok` marks: (n, k) indices padded with -1, d2 padded with +inf"""
    cand = np.flatnonzero(ok)
    idx = np.full((len(requests), k), -1, dtype=np.int32)
    d2 = np.full((len(requests), k), np.inf)
    for q, r in enumerate(requests):
        d = _d2(tips[cand], r)
        order = np.argsort(d, kind="stable")[:k]                  # (cand ascends: a stable sort by d2 is the order (d2, index))
        idx[q, :len(order)] = cand[order]
        d2[q, :len(order)] = d[order]
    return idx, d2


def test_nearest_tips_equal_numpy_bit_for_bit(irt):
    W = irt.workloads
    robot = W.robot_config3()
    chk = irt.VoxelBackboneValidityChecker(robot, irt.VoxelEnvironment(), _free_space(irt))
    rng = np.random.default_rng(31)
    V = 20000
    states = W.random_states(robot, V, seed=3, tau_max=15.0)
    tips = rng.uniform(-0.1, 0.1, (V, 3))
    tips[::3] = np.round(tips[::3] * 1000.0) / 1000.0                 # a third on a 1 mm lattice: exact ties
    present = rng.random(V) > 0.05
    status = np.where(rng.random(V) > 0.1, 1, 2).astype(np.uint8)
    prm = irt.VoxelCachedLazyPRM(chk, states, np.zeros((0, 2), dtype=np.int32))
    with pytest.raises(irt.InvalidArgument):
        prm.nearest_tips(np.zeros((1, 3)), 5)                         # no tips yet
    prm.set_tips(tips, present=present)
    prm.set_validity(status)
    requests = rng.uniform(-0.1, 0.1, (1000, 3))
    requests[:200] = np.round(requests[:200] * 1000.0) / 1000.0       # lattice points: many tips at exactly the same distance
    requests[200:260] = tips[rng.integers(0, V, 60)]                  # equal to a tip
    ok = present & (status == 1)
    for k in (1, 5, 11, 64):
        idx, d2 = prm.nearest_tips(requests, k)
        want_idx, want_d2 = _nearest(tips, ok, requests, k)
        assert np.array_equal(idx, want_idx), (k, np.flatnonzero((idx != want_idx).any(1))[:5])
        assert np.array_equal(d2.view(np.uint64), want_d2.view(np.uint64)), k
    assert (want_d2[:200, :64] == np.roll(want_d2[:200, :64], 1, axis=1))[:, 1:].any()     # the ties exist
    # the tip array whole (a large batch) and cut into slices (a few requests): the same rows
    big = np.tile(requests, (5, 1))
    idx_b, d2_b = prm.nearest_tips(big, 5)
    want_idx, want_d2 = _nearest(tips, ok, requests, 5)
    assert np.array_equal(idx_b, np.tile(want_idx, (5, 1))) and np.array_equal(d2_b, np.tile(want_d2, (5, 1)))
    idx_1, d2_1 = prm.nearest_tips(requests[7], 5)
    assert np.array_equal(idx_1[0], want_idx[7]) and np.array_equal(d2_1[0], want_d2[7])
    # device tensors
    import torch
    d_req = torch.from_numpy(requests).cuda()
    d_idx = torch.empty((len(requests), 5), dtype=torch.int32, device="cuda")
    d_d2 = torch.empty((len(requests), 5), dtype=torch.float64, device="cuda")
    prm.nearest_tips_dev(d_req, len(requests), 5, d_idx, d_d2)
    assert np.array_equal(d_idx.cpu().numpy(), want_idx) and np.array_equal(d_d2.cpu().numpy(), want_d2)
    # fewer than k qualify: padded with -1; none: the whole row
    few = np.full(V, 2, dtype=np.uint8)
    few[rng.choice(np.flatnonzero(present), 40, replace=False)] = 1
    prm.set_validity(few)
    idx, d2 = prm.nearest_tips(requests[:50], 64)
    want_idx, want_d2 = _nearest(tips, present & (few == 1), requests[:50], 64)
    assert np.array_equal(idx, want_idx) and np.array_equal(d2, want_d2)
    assert (idx[:, :40] >= 0).all() and (idx[:, 40:] == -1).all() and np.isinf(d2[:, 40:]).all()
    prm.set_validity(np.full(V, 2, dtype=np.uint8))
    idx, _ = prm.nearest_tips(requests[:50], 5)
    assert (idx == -1).all()
    r = prm.roadmap_ik_batch(requests[:3])
    assert (r["outcome"] == NO_NEIGHBOR).all() and (r["neighbor_vertex"] == -1).all() and np.isnan(r["controls"]).all()
    with pytest.raises(irt.InvalidArgument):
        prm.nearest_tips(requests[:2], 65)
    # tips computed on the device from the roadmap's states: the tips tr_fk_tips gives
    prm.set_tips()
    prm.set_validity(np.ones(V, dtype=np.uint8))
    own, _ = chk.engine.fk_tips(states[:300])
    idx, d2 = prm.nearest_tips(own, 1)
    assert (d2[:, 0] == 0.0).all() and np.array_equal(_d2(own, own[idx[:, 0]]), np.zeros(300))


def _obstacle_roadmap(irt, n_vertices=2500, k=6, seed=21):
    W = irt.workloads
    robot = W.robot_config3()
    vox, _ = W.reach_environment(seed=7, n_spheres=64)
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


def _restate(irt, prm, tips, requests, k, tolerance):
    """Rules 1 - 5 of include/tendon_hip.h over the single pieces."""
    eng = prm.engine
    vstat, _ = prm.validity()
    N, _ = _nearest(tips, vstat == 1, requests, k)
    n, S = len(requests), prm.states.shape[1]
    out = dict(controls=np.full((n, S), np.nan), tip=np.full((n, 3), np.nan), error=np.full(n, np.nan), neighbor_vertex=np.full(n, -1, np.int32),
               outcome=np.full(n, NO_NEIGHBOR, np.int32), last_valid_t=np.full(n, np.nan))
    slots = np.argwhere(N >= 0)
    if len(slots) == 0:
        return out, N
    a = prm.states[N[slots[:, 0], slots[:, 1]]]
    ik = eng.ik_batch(a, requests[slots[:, 0]], stop_threshold_err=tolerance)
    ev = eng.validate_edges_last_valid(a, ik["state"])
    g = irt.roadmap.interpolate_states(eng, a, ik["state"], ev["last_valid_t"])
    gtip, _ = eng.fk_tips(g)
    for q in range(n):
        mine = np.flatnonzero(slots[:, 0] == q)                        # in neighbour order
        if len(mine) == 0:
            continue
        hit = [s for s in mine if ik["error"][s] < tolerance and ev["valid"][s]]
        if hit:
            s = hit[0]
            out["controls"][q], out["tip"][q], out["error"][q], out["last_valid_t"][q] = ik["state"][s], ik["tip"][s], ik["error"][s], 1.0
            out["outcome"][q] = REACHED
        else:
            d = gtip[mine] - requests[q]
            e = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
            s = mine[int(np.argmin(e))]                                 # (argmin: the first of equal values)
            out["controls"][q], out["tip"][q], out["error"][q], out["last_valid_t"][q] = g[s], gtip[s], e.min(), ev["last_valid_t"][s]
            out["outcome"][q] = CLOSEST
        out["neighbor_vertex"][q] = N[q, slots[s, 1]]
    return out, N


def _same_bits(a, b, keys=("controls", "tip", "error", "neighbor_vertex", "outcome", "last_valid_t")):
    for key in keys:
        x, y = np.ascontiguousarray(a[key]), np.ascontiguousarray(b[key])
        assert x.dtype == y.dtype and x.shape == y.shape, key
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), (key, np.flatnonzero((x != y).reshape(len(x), -1).any(1))[:5])


def _requests(tips, n, seed):
    rng = np.random.default_rng(seed)
    req = tips[rng.integers(0, len(tips), n)] + rng.normal(size=(n, 3)) * 0.003
    req[n // 2:] = rng.uniform(-0.12, 0.12, (n - n // 2, 3)) + np.array([0.0, 0.0, 0.1])      # anywhere in the workspace: many out of reach or walled in
    return req


def test_batch_equals_composition_of_the_single_pieces(irt):
    robot, vox, chk, mv, states, edges, vc, ec, prm = _obstacle_roadmap(irt)
    requests = _requests(vc["tips"], 512, seed=5)
    for k, tol in ((5, 1e-4), (3, 1e-5)):
        got = prm.roadmap_ik_batch(requests, tolerance=tol, k=k, motion_validator=mv)
        want, N = _restate(irt, prm, vc["tips"], requests, k, tol)
        _same_bits(got, want)
        print("k", k, "tolerance", tol, "outcomes", np.bincount(got["outcome"], minlength=3), "stepped back",
              int((got["last_valid_t"][got["outcome"] == CLOSEST] < 1.0).sum()))
        assert (got["outcome"] == REACHED).any() and (got["outcome"] == CLOSEST).any()        # both branches of the rule are exercised
    # a request's answer does not depend on the batch it is in
    got = prm.roadmap_ik_batch(requests, motion_validator=mv)
    for q in (0, 17, 255, 300, 511):
        alone = prm.roadmap_ik_batch(requests[q], motion_validator=mv)
        _same_bits(alone, {key: val[q:q + 1] for key, val in got.items()})
    prof = prm.tip_query_profile()
    assert prof["ik_rounds"] > 0 and prof["ik_ms"] > 0 and prof["solve_ms"] == 0


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
        N, _ = _nearest(tips, vstat == 1, requests, k)
        for q in range(len(requests)):
            assert res["outcome"][q] in (REACHED, CLOSEST)
            ctl, nv = res["controls"][q], res["neighbor_vertex"][q]
            ok, tip, _ = orc.is_valid_state(orb, og, ctl)
            assert ok, q
            assert np.abs(tip - res["tip"][q]).max() <= 1e-9
            assert abs(res["error"][q] - np.linalg.norm(tip - requests[q])) <= 1e-9
            assert nv in N[q]
            # x = the IK solution from that neighbour (its bits: test_batch_equals_composition_of_the_single_pieces)
            x = chk.engine.ik_batch(states[nv], requests[q], stop_threshold_err=tol)
            w = orc.check_motion_until_invalid(orb, og, states[nv], x["state"][0])
            if res["outcome"][q] == REACHED:
                assert res["error"][q] < tol and w["is_fully_valid"] and res["last_valid_t"][q] == 1.0
                assert np.array_equal(ctl, x["state"][0])
            else:
                assert res["last_valid_t"][q] == w["last_valid_t"]
                assert not (w["is_fully_valid"] and x["error"][0] < tol)

    free = prm.roadmap_ik_batch(requests, tolerance=tol, k=k, motion_validator=mv)
    print("free space outcomes", np.bincount(free["outcome"], minlength=3))
    assert free["outcome"][0] == REACHED
    check(free, requests, og)
    # the request walled in: every IK solution collides, the answer is a valid state short of it
    blocked = _wall_in(irt, og, requests[0])
    prm.set_obstacles(blocked)
    walled = prm.roadmap_ik_batch(requests[:8], tolerance=tol, k=k, motion_validator=mv)
    assert walled["outcome"][0] == CLOSEST and walled["error"][0] > tol and walled["last_valid_t"][0] < 1.0
    check(walled, requests[:8], og)


@pytest.mark.parametrize("search", ["host", "device"])
def test_solve_to_tips_is_the_roadmap_query_plus_one_edge(irt, orc, helpers, monkeypatch, search):
    monkeypatch.setenv("TENDON_HIP_SEARCH", search)
    W = irt.workloads
    robot, vox, chk, mv, states, edges, vc, ec, prm = _obstacle_roadmap(irt)
    new_vox, _ = W.reach_environment(seed=7, n_spheres=76)
    prm.set_obstacles(new_vox)
    n = 300
    requests = _requests(vc["tips"], n, seed=9)
    starts = np.random.default_rng(10).integers(0, len(states), n).astype(np.int32)
    res = prm.solve_to_tips(starts, requests, motion_validator=mv)
    prof = prm.tip_query_profile()                                     # (of the last tip call: read before the next one)
    assert prof["solve_ms"] > 0 and prof["ik_rounds"] > 0
    ik = prm.roadmap_ik_batch(requests, motion_validator=mv)
    _same_bits(res, ik)
    assert (res["outcome"] != NO_NEIGHBOR).all()
    conn = res["neighbor_vertex"]
    plain = prm.solveWithRoadmap(starts, conn)
    assert np.array_equal(res["status"], plain["status"])
    assert np.array_equal(res["path_vertices"], plain["path_vertices"]) and np.array_equal(res["path_offsets"], plain["path_offsets"])
    orb, og = helpers.oracle_robot(orc, robot), helpers.oracle_grid(orc, new_vox)
    orm = orc.Roadmap(orb, states, edges, None, vc, ec)
    code = {-2: 2, -3: 3, 0: 1}
    dp = lambda a: np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    solved = 0
    for q in range(n):
        w = orm.query(og, starts[q], conn[q])
        assert res["status"][q] == (0 if w["n"] > 0 else code[w["n"]]), (q, w)
        if w["n"] <= 0:
            assert len(res["paths"][q]) == 0 and np.isinf(res["cost"][q])
            continue
        solved += 1
        assert np.array_equal(res["paths"][q], w["path"]) and plain["cost"][q] == w["cost"]
        last = float(orb.lib.orc_state_distance(ctypes.byref(orb.c), dp(states[conn[q]]), dp(res["controls"][q])))
        assert abs(res["cost"][q] - (w["cost"] + last)) <= 1e-12
        assert res["paths"][q][0] == starts[q] and res["paths"][q][-1] == conn[q]
    print("solved", solved, "of", n, "statuses", np.bincount(res["status"], minlength=4))
    assert solved > 0


def test_changed_environment_keeps_validity_consistent_with_revalidate(irt):
    W = irt.workloads
    robot, vox, chk, mv, states, edges, vc, ec, prm = _obstacle_roadmap(irt)
    res0 = prm.solve_to_tips(np.zeros(64, dtype=np.int32), _requests(vc["tips"], 64, seed=1), motion_validator=mv)
    new_vox, _ = W.reach_environment(seed=7, n_spheres=80)
    assert new_vox != vox
    prm.set_obstacles(new_vox)
    requests = _requests(vc["tips"], 256, seed=2)
    starts = np.random.default_rng(3).integers(0, len(states), 256).astype(np.int32)
    res = prm.solve_to_tips(starts, requests, motion_validator=mv)
    v_left, e_left = prm.validity()
    nv, ne = prm.revalidate()
    v_all, e_all = prm.validity()
    assert nv > 0 and (v_all > 0).all()
    conn = res["neighbor_vertex"][res["outcome"] != NO_NEIGHBOR]
    assert len(conn) == 256 and (v_all[conn] == 1).all()
    assert np.array_equal(v_left[v_left > 0], v_all[v_left > 0]) and np.array_equal(e_left[e_left > 0], e_all[e_left > 0])
    # vertices the old environment accepted and the new one does not are no neighbours any more
    assert (res0["outcome"] != NO_NEIGHBOR).all() and (v_all == 2).any()


def test_chained_plan_hops_start_where_the_last_one_ended(irt):
    robot, vox, chk, mv, states, edges, vc, ec, prm = _obstacle_roadmap(irt)
    rng = np.random.default_rng(8)
    C_, H = 24, 4
    way = vc["tips"][rng.integers(0, len(states), (C_, H))] + rng.normal(size=(C_, H, 3)) * 0.002
    start = rng.integers(0, len(states), C_)
    plan = irt.chained_plan(prm, start, way, motion_validator=mv)
    assert len(plan["hops"]) == H and plan["solved"].any()
    eng = chk.engine
    total = np.zeros(C_)
    alive = np.ones(C_, dtype=bool)
    prev_state, prev_vertex, on_roadmap = states[start].copy(), start.copy(), True
    for h, hop in enumerate(plan["hops"]):
        assert np.array_equal(hop["active"], alive)
        idx = np.flatnonzero(alive)
        assert np.array_equal(hop["chains"], idx)
        assert np.array_equal(hop["start_state"][idx], prev_state[idx])        # every hop starts at the previous hop's goal state
        ok = hop["status"] == 0
        pre = np.zeros(len(idx)) if on_roadmap else eng.state_distance(prev_state[idx], states[prev_vertex[idx]])
        assert np.array_equal(hop["prefix_cost"][idx], pre)
        for j, c in enumerate(idx):
            if not ok[j]:
                continue
            p = hop["paths"][j]
            assert p[0] == prev_vertex[c] and p[-1] == hop["neighbor_vertex"][j]
            assert hop["total_cost"][c] == pre[j] + hop["cost"][j]
            total[c] += hop["total_cost"][c]
            prev_state[c], prev_vertex[c] = hop["controls"][j], hop["neighbor_vertex"][j]
        alive[idx[~ok]] = False
        on_roadmap = False
    assert np.array_equal(plan["solved"], alive)
    assert np.array_equal(plan["cost"][alive], total[alive]) and np.isinf(plan["cost"][~alive]).all()
    assert np.array_equal(plan["final_state"][alive], prev_state[alive])
