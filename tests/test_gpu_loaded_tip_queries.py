"""Tip-goal queries on LOADED shapes (tr_roadmap_ik_batch_loaded / _solve_tips_loaded / _set_tips_loaded, tr_fk_loaded_tips*;
VoxelCachedLazyPRM.roadmap_ik_loaded_batch, .solve_to_tips_loaded, .set_tips_loaded, chained_plan_loaded, Engine.fk_loaded_tips).

Worlds, loads and grids: tests/loaded_edges_common.py -- config1 (3 tendons, P = 41, frame base) and config3_rot (rotation, frame
world).  The roadmap is RoadmapBuilder.create_roadmap(64, k=4) under those loads; 12 requests made as
tests/test_gpu_tip_queries.py::_requests makes them; k = 3, connect_k 0 and 3.

 1 the call is its rules (2L - 5'L of include/tendon_hip.h) over the single pieces, byte for byte, vu0 and counts included
 2 the answers are physical: numpy's cold shooting (tests/loaded_fk_reference.py) at `controls`, the oracle's judge on the joining edge
 3 the load matters         4 zero load is the unloaded call         5 batch independence (alone, of 12, TENDON_HIP_SHOOT_CHUNK=7)
 6 no equilibrium, no goal  7 solve_to_tips_loaded, chained_plan_loaded   8 set_tips_loaded, fk_loaded_tips   9 errors

Bounds are tests/test_gpu_loaded_ik.py's: bound_i = 1e-9 m + 1.5 C_i (residual_threshold + |e_i|) from the numpy shooting at the
returned state; an IK answer's cold numpy tip lies within tolerance + bound_i of its goal, the device's loaded tip within bound_i of
the cold numpy tip; at zero load the states of the two IK schemes agree to 1e-6 (1 + |x|) on at least 0.9 of the reached rows."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.join(HERE, "golden")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import fk_truth_common as ftc                                          # noqa: E402
import loaded_edges_reference as ler                                  # noqa: E402
import loaded_fk_reference as ref                                     # noqa: E402
import test_gpu_loaded_roadmap as tlr                                 # noqa: E402  (World: robot, grid, oracle robot and judge of a fixture)
from loaded_edges_common import DIST, WRENCH                          # noqa: E402

pytestmark = pytest.mark.gpu

REACHED, CLOSEST, NO_NEIGHBOR = 0, 1, 2
NAMES = ("config1", "config3_rot")
SEED = {"config1": 7, "config3_rot": 7}                                # of the requests: >= 3 REACHED and >= 2 CLOSEST at connect_k = 0
K, TOL, NREQ = 3, 1e-4, 12
KEYS = ("controls", "tip", "error", "neighbor_vertex", "outcome", "last_valid_t", "vu0")
HOPELESS = [1e6, 0.0, 0.0, 0.0, 0.0, 0.0]                              # test_gpu_loaded_ik.py's isolation load


def _requests(tips, n, seed):
    rng = np.random.default_rng(seed)
    req = tips[rng.integers(0, len(tips), n)] + rng.normal(size=(n, 3)) * 0.003
    req[n // 2:] = rng.uniform(-0.12, 0.12, (n - n // 2, 3)) + np.array([0.0, 0.0, 0.1])
    return np.ascontiguousarray(req)


class Setup:
    """One world: the checker under loads, its roadmap, the requests, and the loaded call's results (computed once per connect_k)."""

    def __init__(self, irt, w):
        self.irt, self.w, self.frame = irt, w, w.frame
        self.loads = dict(wrench=WRENCH, dist=DIST, frame=w.frame)
        self.chk = irt.VoxelBackboneValidityChecker(w.robot, irt.VoxelEnvironment(), w.vox)
        self.mv = irt.VoxelBackboneMotionValidator(self.chk)
        self.chk.set_loads(WRENCH, DIST, frame=w.frame)
        self.prm, self.road = irt.RoadmapBuilder(self.chk, self.mv, seed=0).create_roadmap(64, k=4, device=False)
        self.eng = self.chk.engine
        self.requests = _requests(self.road["tips"], NREQ, SEED[w.name])
        self._got = {}

    def call(self, prm, requests, kc, **kw):
        return prm.roadmap_ik_loaded_batch(requests, tolerance=TOL, k=K, motion_validator=self.mv, connect_k=kc, **{**self.loads, **kw})

    def got(self, kc):
        if kc not in self._got:
            self._got[kc] = self.call(self.prm, self.requests, kc)
        return self._got[kc]

    def clone(self, chk, tips):
        """a roadmap with the same states, edges and caches on another checker; tips: an array, None (computed unloaded), or 'loaded'"""
        prm = self.irt.VoxelCachedLazyPRM(chk, self.road["states"], self.road["edges"])
        prm.set_caches(self.road["vertex_caches"], self.road["edge_caches"])
        if isinstance(tips, str):
            prm.set_tips_loaded(**self.loads)
        else:
            prm.set_tips(tips)
        return prm


_setups = {}


@pytest.fixture(scope="module")
def setup(irt, orc, helpers):
    def get(name):
        if name not in _setups:
            if name not in tlr._worlds:
                tlr._worlds[name] = tlr.World(irt, orc, helpers, name)
            _setups[name] = Setup(irt, tlr._worlds[name])
        return _setups[name]
    return get


def _same_bits(a, b, keys=KEYS, rows=slice(None)):
    for key in keys:
        x, y = np.ascontiguousarray(a[key][rows]), np.ascontiguousarray(b[key])
        assert x.dtype == y.dtype and x.shape == y.shape, key
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), (key, x, y)


def _restate(s, prm, requests, kc, wrench=WRENCH, dist=DIST):
    """Rules 1, 2L - 5L / 5'L of include/tendon_hip.h over the single pieces."""
    irt, eng, states = s.irt, prm.engine, prm.states
    n, S = len(requests), states.shape[1]
    res = dict(min_tension_change=s.mv.min_tension_change, min_rotation_change=s.mv.min_rotation_change,
               min_retraction_change=s.mv.min_retraction_change)
    N, _ = prm.nearest_tips(requests, K)
    out = dict(controls=np.full((n, S), np.nan), tip=np.full((n, 3), np.nan), error=np.full(n, np.nan), neighbor_vertex=np.full(n, -1, np.int32),
               ik_vertex=np.full(n, -1, np.int32), outcome=np.full(n, NO_NEIGHBOR, np.int32), last_valid_t=np.full(n, np.nan),
               vu0=np.full((n, 6), np.nan), counts=np.zeros(4, dtype=np.int64))
    slots = np.argwhere(N >= 0)
    if len(slots) == 0:
        return out
    iv = N[slots[:, 0], slots[:, 1]]                                     # the slots' IK vertices
    ik = eng.ik_loaded_batch(states[iv], requests[slots[:, 0]], wrench=wrench, dist=dist, frame=s.frame, stop_threshold_err=TOL)
    # the pairs (slot, source) in (slot, source) order
    if kc > 0:
        Cn, _ = prm.nearest_states(ik["state"], kc)
        pairs = []
        for i in range(len(slots)):
            src = [int(v) for v in Cn[i] if v >= 0]
            if iv[i] not in src:
                src.append(int(iv[i]))
            pairs += [(i, v) for v in src]
    else:
        pairs = [(i, int(iv[i])) for i in range(len(slots))]
    ps, pv = np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])
    a, b = states[pv], ik["state"][ps]
    ev = eng.validate_edges_loaded(a, b, wrench=wrench, dist=dist, frame=s.frame, warm_start=False, last_valid=True, **res)
    g = irt.roadmap.interpolate_states(eng, a, b, ev["last_valid_t"])
    gt = eng.fk_loaded_tips(g, wrench=wrench, dist=dist, frame=s.frame)
    out["counts"][:] = [len(pairs), int((~ik["equilibrium"]).sum()), int((~gt["converged"]).sum()),
                        int(ik["num_fk_calls"].sum()) + ev["n_integrations"] + gt["n_integrations"]]
    for q in range(n):
        mine = [j for j in range(len(pairs)) if slots[ps[j], 0] == q]   # in (slot, source) order
        hit = [j for j in mine if ik["error"][ps[j]] < TOL and ik["equilibrium"][ps[j]] and ev["valid"][j]]
        if hit:
            j = hit[0]
            i = ps[j]
            out["controls"][q], out["tip"][q], out["error"][q], out["last_valid_t"][q] = ik["state"][i], ik["tip"][i], ik["error"][i], 1.0
            out["vu0"][q], out["outcome"][q] = ik["vu0"][i], REACHED
        else:
            cand = [j for j in mine if gt["converged"][j]]
            if not cand:
                continue
            d = gt["tips"][cand] - requests[q]
            e = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
            j = cand[int(np.argmin(e))]                                  # (argmin: the first of equal values)
            out["controls"][q], out["tip"][q], out["error"][q], out["last_valid_t"][q] = g[j], gt["tips"][j], e.min(), ev["last_valid_t"][j]
            out["vu0"][q], out["outcome"][q] = gt["vu0"][j], CLOSEST
        out["neighbor_vertex"][q], out["ik_vertex"][q] = pv[j], iv[ps[j]]
    return out


# ---- 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kc", [0, 3])
@pytest.mark.parametrize("name", NAMES)
def test_the_call_is_its_rules(setup, name, kc):
    s = setup(name)
    got = s.got(kc)
    want = _restate(s, s.prm, s.requests, kc)
    print(name, "connect_k", kc, "outcomes", np.bincount(got["outcome"], minlength=3), "counts", got["counts"], "want", want["counts"],
          "stepped back", int((got["last_valid_t"][got["outcome"] == CLOSEST] < 1.0).sum()))
    if kc == 0:                                                          # the condition on the inputs
        assert (got["outcome"] == REACHED).sum() >= 3 and (got["outcome"] == CLOSEST).sum() >= 2
        assert "ik_vertex" not in got and "connect_stats" not in got
    else:
        _same_bits(got, want, keys=("ik_vertex",))
        cs = got["connect_stats"]
        assert cs["pairs_checked"] == got["counts"][0] and cs["reached"] == (got["outcome"] == REACHED).sum()
        assert cs["moved"] == (got["neighbor_vertex"] != got["ik_vertex"]).sum()
    _same_bits(got, want)
    assert np.array_equal(got["counts"], want["counts"])
    prof = s.prm.tip_query_profile()
    assert prof["ik_rounds"] > 0 and prof["ik_ms"] > 0 and prof["solve_ms"] == 0


# ---- 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kc", [0, 3])
@pytest.mark.parametrize("name", NAMES)
def test_the_answers_are_physical(setup, name, kc):
    s = setup(name)
    w, got = s.w, s.got(kc)
    live = np.flatnonzero(got["outcome"] != NO_NEIGHBOR)
    ctl = got["controls"][live]
    lw, ldd = s.eng.sample_loads(ctl, WRENCH, DIST, s.frame)
    with np.errstate(all="ignore"):
        cold = ref.shoot(w.orb, ctl, F_e=lw[:, :3], L_e=lw[:, 3:], f_e=ldd[:, :3], l_e=ldd[:, 3:])
    bound = 1e-9 + 1.5 * cold["C"] * (w.robot.residual_threshold + cold["e"])
    tip_cold = cold["p"][:, -1]
    miss = np.linalg.norm(tip_cold - s.requests[live], axis=1)
    off = np.linalg.norm(tip_cold - got["tip"][live], axis=1)
    print(name, "connect_k", kc, "cold numpy tip off the request by", miss, "off the returned tip by", off, "bound", bound)
    assert cold["converged"].all()
    for j, q in enumerate(live):
        if got["outcome"][q] == REACHED:
            assert miss[j] <= TOL + bound[j], q
            assert got["last_valid_t"][q] == 1.0
        else:
            assert off[j] <= bound[j], q
            assert abs(got["error"][q] - np.linalg.norm(got["tip"][q] - s.requests[q])) <= 1e-12, q
            # the joining edge, judged by the oracle's predicates on cold device shapes of its own bisection
            fk = lambda cfg, sa: w.samples(np.asarray(cfg, float).reshape(1, -1))[0]
            r = ler.check_motion(w.space, w.judge, s.road["states"][got["neighbor_vertex"][q]], got["controls"][q], fk, until_invalid=True)
            print("  request", q, "last_valid_t", got["last_valid_t"][q], "edge to controls: fully valid", r["is_fully_valid"], "samples", r["n_fk"])
            assert r["is_fully_valid"] and not r["domain_error"], q


# ---- 3 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_the_load_matters(setup, irt, name):
    s = setup(name)
    plain_chk = irt.VoxelBackboneValidityChecker(s.w.robot, irt.VoxelEnvironment(), s.w.vox)
    plain = s.clone(plain_chk, None)
    un = plain.roadmap_ik_batch(s.requests, tolerance=TOL, k=K, motion_validator=s.mv)
    have = np.flatnonzero(un["outcome"] != NO_NEIGHBOR)
    lw, ldd = s.eng.sample_loads(un["controls"][have], WRENCH, DIST, s.frame)
    fk = s.eng.fk_loaded_batch(un["controls"][have], wrench=lw, dist=ldd)
    miss = np.full(NREQ, np.nan)
    miss[have] = np.linalg.norm(fk["p"][:, -1] - s.requests[have], axis=1)
    reached = s.got(0)["outcome"] == REACHED
    print("%s: the unloaded call's controls under the load miss their requests by %s m; the loaded call reaches %s within %g m"
          % (name, np.array2string(miss, precision=4), np.flatnonzero(reached), TOL))
    assert (miss[reached] > TOL).any()


# ---- 4 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kc", [0, 3])
def test_zero_load_is_the_unloaded_call(setup, irt, kc):
    """On config1 only: the bound of tests/test_gpu_loaded_ik.py's zero-load test is one for a robot whose IK has ONE solution (S = 3
    states for 3 tip coordinates).  config3_rot has S = 4: the solutions of a reachable request form a curve, and the two IK schemes --
    different Jacobians, different steps -- legitimately stop at different points of it (measured: 0 - 2 of 5 - 8 reached rows within
    that bound on 24 seeds).  What else is seed-dependent: under the accurate rule a CLOSEST request whose IK answer is joined by
    several fully valid edges has several pairs that end in the same state, tied up to the last bits of interpolate(); the two
    schemes' answers lie 1e-6 apart, so which source wins is not common to them on every seed (on 17 of 24 it is; SEED is one of those)."""
    name = "config1"
    s = setup(name)
    chk = irt.VoxelBackboneValidityChecker(s.w.robot, irt.VoxelEnvironment(), s.w.vox)
    prm = s.clone(chk, chk.engine.fk_tips(s.road["states"])[0])
    a = prm.roadmap_ik_batch(s.requests, tolerance=TOL, k=K, motion_validator=s.mv, connect_k=kc)
    b = prm.roadmap_ik_loaded_batch(s.requests, np.zeros(6), np.zeros(6), s.frame, tolerance=TOL, k=K, motion_validator=s.mv, connect_k=kc)
    print(name, kc, "outcomes", a["outcome"], b["outcome"], "largest control difference", np.nanmax(np.abs(a["controls"] - b["controls"])))
    assert np.array_equal(a["outcome"], b["outcome"]) and np.array_equal(a["neighbor_vertex"], b["neighbor_vertex"])
    if kc:
        assert np.array_equal(a["ik_vertex"], b["ik_vertex"])
    ra = a["outcome"] == REACHED
    close = (np.abs(a["controls"] - b["controls"]) <= 1e-6 * (1 + np.abs(a["controls"]))).all(axis=1)
    assert (close & ra).sum() >= 0.9 * ra.sum()
    assert b["counts"][1] == 0 and b["counts"][2] == 0


# ---- 5 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["alone", "chunk7"])
@pytest.mark.parametrize("kc", [0, 3])
@pytest.mark.parametrize("name", NAMES)
def test_batch_independence(setup, irt, name, kc, how):
    """(30 outer IK iterations instead of 100 keep the calls of a case short: the out-of-reach requests run to the limit in every
    call; the three runs share the setting)"""
    s = setup(name)
    ik = dict(max_iters=30)
    key = ("independence", kc)
    if key not in s._got:
        s._got[key] = s.call(s.prm, s.requests, kc, ik=ik)
    got = s._got[key]
    assert (got["outcome"] == REACHED).sum() >= 3 and (got["outcome"] == CLOSEST).sum() >= 2
    keys = KEYS + (("ik_vertex",) if kc else ())
    if how == "chunk7":
        with ftc.with_env(TENDON_HIP_SHOOT_CHUNK=7):
            chk7 = irt.VoxelBackboneValidityChecker(s.w.robot, irt.VoxelEnvironment(), s.w.vox)
        _same_bits(s.call(s.clone(chk7, s.road["tips"]), s.requests, kc, ik=ik), got, keys=keys)
    else:
        for q in range(NREQ):
            _same_bits(got, s.call(s.prm, s.requests[q], kc, ik=ik), keys=keys, rows=slice(q, q + 1))


# ---- 6 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_no_equilibrium_no_goal(setup, name):
    s = setup(name)
    before = s.got(0)
    lost = s.call(s.prm, s.requests, 0, wrench=HOPELESS)
    print(name, "hopeless wrench: outcomes", lost["outcome"], "counts", lost["counts"])
    assert not (lost["outcome"] == REACHED).any()
    for q in range(NREQ):
        if lost["outcome"][q] == CLOSEST:
            assert np.isfinite(lost["controls"][q]).all() and np.isfinite(lost["tip"][q]).all() and np.isfinite(lost["vu0"][q]).all()
            assert np.isfinite(lost["error"][q]) and lost["neighbor_vertex"][q] >= 0
        else:
            assert np.isnan(lost["controls"][q]).all() and np.isnan(lost["tip"][q]).all() and np.isnan(lost["vu0"][q]).all()
            assert np.isnan(lost["error"][q]) and np.isnan(lost["last_valid_t"][q]) and lost["neighbor_vertex"][q] == -1
    assert lost["counts"][1] + lost["counts"][2] > 0
    _same_bits(s.call(s.prm, s.requests, 0), before)


# ---- 7 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kc", [0, 3])
def test_solve_to_tips_loaded_and_chained_plan_loaded(setup, irt, kc):
    s = setup("config3_rot")
    prm, eng, states = s.prm, s.eng, s.road["states"]
    rng = np.random.default_rng(11)
    starts = rng.integers(0, len(states), NREQ).astype(np.int32)
    kw = dict(tolerance=TOL, k=K, motion_validator=s.mv, connect_k=kc, **s.loads)
    res = prm.solve_to_tips_loaded(starts, s.requests, **kw)
    keys = KEYS + (("ik_vertex",) if kc else ())
    _same_bits(res, s.got(kc), keys=keys)
    assert np.array_equal(res["counts"], s.got(kc)["counts"])
    live = np.flatnonzero(res["outcome"] != NO_NEIGHBOR)
    sw = prm.solveWithRoadmap(starts[live], res["neighbor_vertex"][live])
    want_status = np.full(NREQ, 3, dtype=np.int32)                      # TR_QUERY_INVALID_GOAL: no goal state
    want_status[live] = sw["status"]
    assert np.array_equal(res["status"], want_status)
    for j, q in enumerate(live):
        assert np.array_equal(res["paths"][q], sw["paths"][j]), q
        if sw["status"][j] == 0:
            last = eng.state_distance(states[res["neighbor_vertex"][q]][None], res["controls"][q][None])[0]
            assert abs(res["cost"][q] - (sw["cost"][j] + last)) <= 1e-12, q
        else:
            assert np.isinf(res["cost"][q])
    assert np.isinf(res["cost"][res["outcome"] == NO_NEIGHBOR]).all()
    print("connect_k", kc, "statuses", np.bincount(res["status"], minlength=4))
    assert (res["status"] == 0).any()
    # two hops = two such calls, the second from the first's connection vertices
    way = np.stack([s.requests, s.requests[::-1]], 1)
    plan = irt.chained_plan_loaded(prm, starts, way, **kw)
    h0, h1 = plan["hops"]
    _same_bits(h0, res, keys=keys + ("status", "cost"))
    ok = res["status"] == 0
    idx = np.flatnonzero(ok)
    assert np.array_equal(h1["chains"], idx) and np.array_equal(plan["solved"][~ok], np.zeros((~ok).sum(), dtype=bool))
    second = prm.solve_to_tips_loaded(res["neighbor_vertex"][idx], way[idx, 1], **kw)
    _same_bits(h1, second, keys=keys + ("status", "cost"))
    assert np.array_equal(h1["start_state"][idx], res["controls"][idx])
    assert np.array_equal(h1["prefix_cost"][idx], eng.state_distance(res["controls"][idx], states[res["neighbor_vertex"][idx]]))


# ---- 8 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_set_tips_loaded_and_fk_loaded_tips(setup, irt, name):
    import torch
    s = setup(name)
    eng, states = s.eng, s.road["states"]
    lw, ldd = eng.sample_loads(states, WRENCH, DIST, s.frame)
    fk = eng.fk_loaded_batch(states, wrench=lw, dist=ldd)
    tips = eng.fk_loaded_tips(states, **s.loads)
    assert np.array_equal(tips["tips"], fk["p"][:, -1]) and np.array_equal(tips["tips"], s.road["tips"])
    assert np.array_equal(tips["vu0"], fk["vu0"]) and np.array_equal(tips["converged"], fk["converged"]) and tips["converged"].all()
    assert tips["n_integrations"] == fk["num_fk_calls"].sum()
    rows = eng.fk_loaded_tips(states, wrench=lw, dist=ldd)               # the rows given, frame base
    assert np.array_equal(rows["tips"], tips["tips"])
    # the device form
    dev = "cuda:%d" % eng.device
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    n = len(states)
    d_tips = torch.empty((n, 3), dtype=torch.float64, device=dev)
    d_vu = torch.empty((n, 6), dtype=torch.float64, device=dev)
    d_conv = torch.empty(n, dtype=torch.uint8, device=dev)
    eng.fk_loaded_tips_dev(up(states), n, d_tips, d_wrench=up(lw), d_dist=up(ldd), d_conv=d_conv, d_vu0=d_vu)
    assert np.array_equal(d_tips.cpu().numpy(), tips["tips"]) and np.array_equal(d_vu.cpu().numpy(), tips["vu0"])
    assert d_conv.cpu().numpy().all()
    # set_tips_loaded: the roadmap answers as the builder's does
    own = s.clone(irt.VoxelBackboneValidityChecker(s.w.robot, irt.VoxelEnvironment(), s.w.vox), "loaded")
    idx, d2 = own.nearest_tips(s.road["tips"], 1)
    assert (d2[:, 0] == 0.0).all()
    _same_bits(s.call(own, s.requests, 0), s.got(0))


# ---- 9 ------------------------------------------------------------------------------------------------------------------------
def test_errors(setup, irt):
    s = setup("config1")
    prm = s.prm
    ret = irt.workloads.robot_config1()
    ret.enable_retraction = True
    with pytest.raises(irt.Unsupported) as e0:
        irt.Engine(ret, 0).fk_loaded_batch(np.zeros((2, 4)))               # shoot_check's wording
    rchk = irt.VoxelBackboneValidityChecker(ret, irt.VoxelEnvironment(), s.w.vox)
    rprm = irt.VoxelCachedLazyPRM(rchk, np.zeros((2, 4)), np.zeros((0, 2), dtype=np.int32))
    for call in (lambda: rprm.roadmap_ik_loaded_batch(s.requests[:2], **s.loads), lambda: rprm.solve_to_tips_loaded([0, 1], s.requests[:2], **s.loads),
                 lambda: rprm.set_tips_loaded(**s.loads), lambda: rchk.engine.fk_loaded_tips(np.zeros((2, 4)))):
        with pytest.raises(irt.Unsupported) as e1:
            call()
        assert str(e1.value) == str(e0.value)
    with pytest.raises(irt.InvalidArgument):
        prm.roadmap_ik_loaded_batch(s.requests, WRENCH, DIST, "tool")
    with pytest.raises(irt.InvalidArgument):
        prm.roadmap_ik_loaded_batch(s.requests, shoot=dict(max_iters=-1), **s.loads)
    with pytest.raises(irt.InvalidArgument):
        prm.set_tips_loaded(max_iters=-1, **s.loads)
    plain = s.clone(irt.VoxelBackboneValidityChecker(s.w.robot, irt.VoxelEnvironment(), s.w.vox), None)
    with pytest.raises(irt.InvalidArgument) as e2:
        plain.roadmap_ik_loaded_batch(s.requests, **s.loads)
    assert "UNLOADED" in str(e2.value)
    with pytest.raises(irt.InvalidArgument):
        prm.solve_to_tips_loaded([0, 1, 2], s.requests, **s.loads)           # starts of another length
    # n = 0: empty results, also before set_tips
    bare = irt.VoxelCachedLazyPRM(s.chk, s.road["states"], s.road["edges"])
    for p in (prm, bare):
        r = p.roadmap_ik_loaded_batch(np.zeros((0, 3)), **s.loads)
        assert r["controls"].shape == (0, s.road["states"].shape[1]) and r["vu0"].shape == (0, 6) and not r["counts"].any()
        r = p.solve_to_tips_loaded([], np.zeros((0, 3)), **s.loads)
        assert len(r["status"]) == 0 and len(r["paths"]) == 0
    # the checker-routed calls keep refusing a checker with loads
    with pytest.raises(irt.Unsupported):
        prm.roadmap_ik_batch(s.requests[:2])
