"""Load profiles on the device (tr_set_load_profile; csrc/fk_loaded_kernel.hpp: fk_loaded_profile; csrc/fk_loaded_lin_kernel.hpp:
fk_loaded_lin_profile): every loaded call integrates under w(s) f_e, w(s) l_e.

The references are the numpy ones of the loaded tests, run under tests/load_profile_reference.under.  Tolerances are those of
tests/test_gpu_loaded_fk.py: 1e-9 m between the device's points and a CPU integration from the SAME base strains; 1 % of
residual_threshold between the two arithmetics' residuals; bound_i = 1e-9 + 1.5 C_i (threshold + e_i) between two solutions
(make_loaded_fk.solve_case's bound, C and e from the numpy shooting under the profile).  Profiles: `tip` (0, 0.75 L, L) -> (1, 1, 3),
`zig` (0, 0.25 L, 0.5 L, 0.8 L, L) -> (0, 0, 2, 0.5, 2.5); load cases B (gravity) and D (all twelve load numbers) of the fixtures.

Identities (bit for bit): weights of one are no profile; a constant weight c on the row d is no profile on the row c * d of the host
(c = 0.3 on base-frame rows: the product is rounded once, before the rotation; c = 0.5 under frame='world', where only an exact
scaling commutes with the turn); two knot sets of one function are one table.

Linearisation: the gap of the device's J to loaded_jacobian_reference.sensitivities under the profile must stay within 4 x the same
gap measured here with no profile on the same states (the existing kernel against the same reference); the profile adds one rounded
product per load component and stage and no new difference."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.join(HERE, "golden")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import load_profile_reference as lpr                                 # noqa: E402
import loaded_fk_reference as ref                                    # noqa: E402
import loaded_ik_reference as ikr                                    # noqa: E402
import loaded_jacobian_reference as ljr                              # noqa: E402
from loaded_edges_common import DIST_FULL, FIXTURES, WRENCH, make_edges, make_grid      # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = ("config1", "config3_rot", "n5", "n8", "n1")
KEYS = ("p", "L", "L_i", "vu0", "vuL", "residual", "iters", "num_fk_calls", "converged")
TIPQ_KEYS = ("controls", "tip", "error", "neighbor_vertex", "outcome", "last_valid_t", "vu0")


@pytest.fixture(scope="module")
def gen(orc):
    import make_loaded_fk
    return make_loaded_fk


@pytest.fixture(scope="module")
def world(gen, irt):
    """name -> (robot, oracle robot, fixture arrays, engine): a robot and an engine of this module's own"""
    cache = {}

    def get(name):
        if name not in cache:
            robot, rob, st = gen.fixture(name)
            fx = dict(np.load(gen.path(name)))
            assert np.array_equal(st, fx["states"])
            cache[name] = (robot, rob, fx, robot.engine(0))
        return cache[name]
    return get


@pytest.fixture(scope="module")
def solved(world):
    """(name, profile, case) -> (the device's result under the profile, the numpy shooting's under the helper), computed once"""
    cache = {}

    def get(name, prof, case):
        if (name, prof, case) not in cache:
            robot, rob, fx, eng = world(name)
            knots, weights = lpr.profile(prof, robot.specs.L)
            w, d = fx["wrench_" + case], fx["dist_" + case]
            with eng.load_profile_scope((knots, weights)):
                dev = eng.fk_loaded_batch(fx["states"], wrench=w, dist=d)
            with lpr.under(knots, weights):
                cpu = ref.shoot(rob, fx["states"], F_e=w[:, :3], L_e=w[:, 3:], f_e=d[:, :3], l_e=d[:, 3:])
            cache[name, prof, case] = (dev, cpu)
        return cache[name, prof, case]
    return get


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_same(a, b, keys, what=""):
    for k in keys:
        if isinstance(a[k], dict):
            assert_same(a[k], b[k], sorted(a[k]), what + " " + k)
        elif a[k] is None or np.isscalar(a[k]):
            assert a[k] == b[k], (what, k)
        else:
            assert same_bits(a[k], b[k]), (what, k)


# ---- 1. the table -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["config1", "config3_rot", "n1"])
def test_the_installed_table_is_the_numpy_table(world, irt, name):
    robot, _, _, eng = world(name)
    L = robot.specs.L
    assert eng.load_profile_table().size == 0 and eng.load_profile() is None
    try:
        for knots, weights in (lpr.profile("tip", L), lpr.profile("zig", L), ([0.4 * L], [1.7]), ([-1.0, 0.13, 2.0], [0.5, -2.0, 4.0])):
            eng.set_load_profile(knots, weights)
            assert same_bits(eng.load_profile_table(), irt.load_profile_table(robot, knots, weights))
        assert eng.load_profile_table().size == 1 + 3 * len(ref.step_list(world(name)[1])[1])
    finally:
        eng.clear_load_profile()
    assert eng.load_profile_table().size == 0 and eng.load_profile() is None


def test_table_errors(world, irt):
    robot, _, _, eng = world("config1")
    ret = irt.workloads.robot_config1()
    ret.enable_retraction = True
    reng = irt.Engine(ret, 0)
    with pytest.raises(irt.Unsupported, match="retraction"):
        reng.set_load_profile([0.0, 0.1], [1.0, 2.0])
    assert reng.load_profile_table().size == 0
    reng.close()
    import ctypes as C
    dp = lambda a: np.asarray(a, float).ctypes.data_as(C.POINTER(C.c_double))
    for s, w in (([0.0, 0.0], [1.0, 2.0]), ([0.1, 0.0], [1.0, 2.0]), ([0.0, np.nan], [1.0, 2.0]), ([0.0, 0.1], [np.inf, 2.0])):
        s, w = np.array(s), np.array(w)
        assert eng.lib.tr_set_load_profile(eng._ctx, 2, dp(s), dp(w)) == irt._lib.TR_ERR_INVALID_ARG
        with pytest.raises(irt.InvalidArgument):
            eng.set_load_profile(s, w)
    one = np.array([1.0])
    assert eng.lib.tr_set_load_profile(eng._ctx, 0, dp(one), dp(one)) == irt._lib.TR_ERR_INVALID_ARG
    assert eng.lib.tr_set_load_profile(eng._ctx, 1, None, dp(one)) == irt._lib.TR_ERR_INVALID_ARG
    assert eng.load_profile_table().size == 0                         # a refused call installs nothing


# ---- 2., 3. the integration and the solution ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["B", "D"])
@pytest.mark.parametrize("prof", ["tip", "zig"])
@pytest.mark.parametrize("name", NAMES)
def test_it_is_a_solution_under_the_profile(world, solved, name, prof, case):
    robot, rob, fx, _ = world(name)
    out, _ = solved(name, prof, case)
    thr = robot.residual_threshold
    assert out["converged"].all(), np.nonzero(~out["converged"])[0]
    w, d = fx["wrench_" + case], fx["dist_" + case]
    with lpr.under(*lpr.profile(prof, robot.specs.L)):
        cpu = ref.evaluate(rob, fx["states"], out["vu0"], F_e=w[:, :3], L_e=w[:, 3:], f_e=d[:, :3], l_e=d[:, 3:])
    e = np.linalg.norm(cpu["e"], axis=1)
    figures = (np.abs(out["p"] - cpu["p"]).max(), np.abs(out["L"] - cpu["L"]).max(), np.abs(out["L_i"] - cpu["L_i"]).max(), e.max() / thr,
               np.abs(out["residual"] - e).max() / thr)
    print("%s %s %s: points %.3g m, L %.3g m, L_i %.3g m, |e| %.4f thr, residual_out off by %.3g thr; iters <= %d"
          % ((name, prof, case) + figures + (out["iters"].max(),)))
    assert figures[0] <= 1e-9 and figures[1] <= 1e-9 and figures[2] <= 1e-9
    assert (e <= 1.01 * thr).all()
    assert (np.abs(out["residual"] - e) <= 0.01 * thr).all()


@pytest.mark.parametrize("case", ["B", "D"])
@pytest.mark.parametrize("prof", ["tip", "zig"])
@pytest.mark.parametrize("name", NAMES)
def test_it_is_the_solution_under_the_profile(world, solved, name, prof, case):
    robot, _, fx, _ = world(name)
    out, cpu = solved(name, prof, case)
    assert cpu["converged"].all()
    bound = 1e-9 + 1.5 * cpu["C"] * (robot.residual_threshold + cpu["e"])
    err = np.linalg.norm(out["p"] - cpu["p"], axis=2).max(axis=1)
    moved = np.linalg.norm(cpu["p"][:, -1] - fx["p_" + case][:, -1], axis=1)
    print("%s %s %s: points %.3g of bound (bound <= %.3g m); the profile moves the tips by %.3g .. %.3g m"
          % (name, prof, case, (err / bound).max(), bound.max(), moved.min(), moved.max()))
    assert (err <= bound).all()
    assert moved.min() > 100 * bound.max()                            # a call that ignored the profile would miss by two orders


# ---- 4. identities, bit for bit ---------------------------------------------------------------------------------------------------
class Small:
    """The small world of tests/loaded_edges_common.py on a checker (and an engine) of its own: 8 of its edges, its grid."""

    def __init__(self, irt, name):
        import make_fk_truth as mft
        _, eseed, cap, gseed, count, radius = FIXTURES[name]
        self.irt = irt
        self.robot, self.states = mft.fixture_states(irt, name)
        self.rob = mft.oracle_robot(self.robot)
        self.a, self.b = make_edges(self.robot, 8, eseed, cap)
        self.vox = make_grid(irt, self.robot.specs.dL, gseed, count, radius)
        self.L = self.robot.specs.L

    def checker(self):
        chk = self.irt.VoxelBackboneValidityChecker(self.robot, self.irt.VoxelEnvironment(), self.vox)
        return chk, self.irt.VoxelBackboneMotionValidator(chk)


@pytest.fixture(scope="module")
def small(irt, orc):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Small(irt, name)
        return cache[name]
    return get


def engine_calls(eng, s, dist, frame):
    """Every loaded call of the engine on the small world under one distributed row, whatever profile is installed."""
    st = s.states
    w_rows, d_rows = eng.sample_loads(st, WRENCH, dist, frame)
    out = dict(fk=eng.fk_loaded_batch(st, wrench=w_rows, dist=d_rows))
    out["tips"] = eng.fk_loaded_tips(st, wrench=WRENCH, dist=dist, frame=frame)
    out["valid"] = eng.validate_loaded(st, wrench=w_rows, dist=d_rows)
    out["jac"] = eng.tip_jacobian_loaded(st, wrench=WRENCH, dist=dist, frame=frame, want=("compliance", "W", "blocks"))
    starts = ikr.offset_starts(s.rob, st, 1.0, 0.05)
    out["ik"] = eng.ik_loaded_batch(starts, out["tips"]["tips"], wrench=WRENCH, dist=dist, frame=frame, max_iters=6)
    out["edges"] = eng.validate_edges_loaded(s.a, s.b, wrench=WRENCH, dist=dist, frame=frame)
    n = len(s.a)
    out["indexed"] = eng.validate_edges_loaded_indexed(np.vstack([s.a, s.b]), np.stack([np.arange(n), n + np.arange(n)], axis=1),
                                                       wrench=WRENCH, dist=dist, frame=frame)
    return out


CALL_KEYS = dict(fk=KEYS, tips=("tips", "converged", "vu0", "n_integrations"), valid=("valid", "bits", "flags"),
                 jac=("J", "compliance", "W", "blocks", "tips", "vu0", "equilibrium"), ik=("state", "error", "iters", "tip", "vu0"),
                 edges=("valid", "bits", "n_fk", "n_unconverged", "n_integrations"), indexed=("valid", "bits", "n_fk", "n_unconverged", "n_integrations"))


def assert_calls_same(a, b, what):
    for call, keys in CALL_KEYS.items():
        assert_same(a[call], b[call], keys, what + " " + call)


@pytest.mark.parametrize("name,frame,c", [("config1", "base", 0.3), ("config3_rot", "base", 0.3), ("config3_rot", "world", 0.5)])
def test_identities_of_the_engine_calls(small, name, frame, c):
    s = small(name)
    chk, _ = s.checker()
    eng = chk.engine
    plain = engine_calls(eng, s, DIST_FULL, frame)
    assert plain["fk"]["converged"].all() and plain["jac"]["equilibrium"].all() and plain["ik"]["iters"].max() > 0
    scaled = engine_calls(eng, s, c * DIST_FULL, frame)
    assert not same_bits(scaled["fk"]["p"], plain["fk"]["p"])
    try:
        eng.set_load_profile([0.0, 0.6 * s.L, s.L], [1.0, 1.0, 1.0])     # (a) weights of one
        assert_calls_same(engine_calls(eng, s, DIST_FULL, frame), plain, "ones")
        eng.set_load_profile([0.3 * s.L, 0.7 * s.L], [c, c])            # (b) a constant weight
        assert_calls_same(engine_calls(eng, s, DIST_FULL, frame), scaled, "constant")
        eng.set_load_profile([0.1 * s.L], [c])                          # ... from one knot
        assert_calls_same(engine_calls(eng, s, DIST_FULL, frame), scaled, "one knot")
    finally:
        eng.clear_load_profile()
    assert_calls_same(engine_calls(eng, s, DIST_FULL, frame), plain, "cleared")


@pytest.mark.parametrize("name,frame", [("config1", "base"), ("config3_rot", "base"), ("config3_rot", "world")])
def test_two_knot_sets_of_one_function_are_one_table(small, name, frame):
    """(c): the `tip` profile, and the same function with knots added where it is flat and outside the backbone -- one table, and every
    engine call of the small world (both integrators, both frames on the rotation fixture) returns the same bits under either"""
    s = small(name)
    chk, _ = s.checker()
    eng = chk.engine
    try:
        eng.set_load_profile(*lpr.profile("tip", s.L))
        tab = eng.load_profile_table()
        a = engine_calls(eng, s, DIST_FULL, frame)
        eng.set_load_profile([-0.1, 0.0, 0.5 * s.L, 0.75 * s.L, s.L, 2 * s.L], [1.0, 1.0, 1.0, 1.0, 3.0, 3.0])
        assert same_bits(eng.load_profile_table(), tab)
        b = engine_calls(eng, s, DIST_FULL, frame)
    finally:
        eng.clear_load_profile()
    assert a["fk"]["converged"].all() and a["jac"]["equilibrium"].all()
    assert_calls_same(a, b, "two knot sets")
    assert not same_bits(a["fk"]["p"], engine_calls(eng, s, DIST_FULL, frame)["fk"]["p"])     # (and the profile is seen)


@pytest.mark.parametrize("name,frame,c", [("config1", "base", 0.3), ("config3_rot", "world", 0.5)])
def test_identities_of_the_roadmap_calls(small, irt, name, frame, c):
    """create_roadmap of 64 vertices under set_loads(..., profile=...) and roadmap_ik_loaded_batch on eight requests"""
    s = small(name)

    def build(dist, profile):
        chk, mv = s.checker()
        chk.set_loads(WRENCH, dist, frame=frame, profile=profile)
        assert (chk.load_profile() is None) == (profile is None) and "profile" not in chk.loads()
        prm, road = irt.RoadmapBuilder(chk, mv, seed=0).create_roadmap(64, k=4, device=False)
        rng = np.random.default_rng(11)
        req = np.ascontiguousarray(road["tips"][rng.integers(0, len(road["tips"]), 8)] + rng.normal(size=(8, 3)) * 0.003)
        got = prm.roadmap_ik_loaded_batch(req, WRENCH, dist, frame, tolerance=1e-4, k=3, motion_validator=mv)
        chk.clear_loads()
        assert chk.load_profile() is None and chk.engine.load_profile_table().size == 0
        return road, got

    def same(x, y, what):
        assert_same(x[0], y[0], ("states", "tips", "edges"), what)
        assert_same(x[1], y[1], TIPQ_KEYS, what)

    plain = build(DIST_FULL, None)
    scaled = build(c * DIST_FULL, None)
    assert not same_bits(plain[0]["tips"], scaled[0]["tips"])
    same(build(DIST_FULL, ([0.0, s.L], [1.0, 1.0])), plain, "ones")
    same(build(DIST_FULL, ([0.5 * s.L], [c])), scaled, "constant")


# ---- 5. the linearisation -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,frame", [("config1", "base"), ("config3_rot", "world")])
def test_linearisation_under_the_profiles(world, name, frame):
    robot, rob, fx, eng = world(name)
    st, thr = fx["states"], robot.residual_threshold
    row = lpr.GRAVITY_ROW

    def gap(profile):
        knots, weights = profile if profile is not None else (None, None)
        with eng.load_profile_scope(profile):
            out = eng.tip_jacobian_loaded(st, dist=row, frame=frame, want=("blocks",))
        assert out["equilibrium"].all()
        b = out["blocks"]
        _, d = ikr.load_rows(rob, st, None, row, frame)
        with lpr.under(knots, weights):
            cpu = ref.evaluate(rob, st, b["y"], f_e=d[:, :3], l_e=d[:, 3:])
            sens = ljr.sensitivities(rob, st, b["y"], dist=row, frame=frame)
        tip, res = np.abs(b["x"] - cpu["p"][:, -1]).max(), np.linalg.norm(b["e"] - cpu["e"], axis=1).max()
        assert tip <= 1e-9 and res <= 0.01 * thr, (tip, res)
        return ljr.relative_gap(out["J"], sens["J"]).max(), out["J"]

    base, J0 = gap(None)
    for prof in ("tip", "zig"):
        g, J = gap(lpr.profile(prof, robot.specs.L))
        print("%s %s %s: J against the numpy sensitivities %.3g; with no profile %.3g" % (name, frame, prof, g, base))
        assert g <= 4 * base
        assert ljr.relative_gap(J, J0).max() > 1e-3                     # (the profile is seen by the linearisation)


# ---- 6. IK under `tip` -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(lpr.IK_SETS))
def test_ik_under_the_tip_profile(world, name):
    robot, rob, fx, eng = world(name)
    thr = robot.residual_threshold
    starts, goals, row, frame = lpr.ik_problem(name, rob, fx["states"])
    prof = lpr.profile("tip", robot.specs.L)
    with eng.load_profile_scope(prof):
        out = eng.ik_loaded_batch(starts, goals, dist=row, frame=frame, max_iters=lpr.IK_MAX_ITERS)
    reached = out["equilibrium"] & (out["error"] <= 1e-4)
    print("%s: reached %d of 24 (not: %s), outer iterations <= %d" % (name, reached.sum(), np.flatnonzero(~reached).tolist(), out["iters"].max()))
    assert reached[list(lpr.IK_REACHED[name])].all(), sorted(set(lpr.IK_REACHED[name]) - set(np.flatnonzero(reached)))
    k = np.flatnonzero(reached)
    _, d = ikr.load_rows(rob, out["state"][k], None, row, frame)
    with lpr.under(*prof):
        cpu = ref.evaluate(rob, out["state"][k], out["vu0"][k], f_e=d[:, :3], l_e=d[:, 3:])
    e, off = np.linalg.norm(cpu["e"], axis=1), np.linalg.norm(cpu["p"][:, -1] - goals[k], axis=1)
    print("%s: |e| <= %.4f thr, |tip - goal| <= %.3g m" % (name, e.max() / thr, off.max()))
    assert (e <= 1.01 * thr).all()
    assert (off <= 1e-4 + 1e-9).all()
    plain = eng.ik_loaded_batch(starts, goals, dist=row, frame=frame, max_iters=lpr.IK_MAX_ITERS)
    apart = np.abs(plain["state"] - out["state"]).max(axis=1)
    print("%s: without the profile %d of 24 reached; states apart by >= %.3g" % (name, (plain["error"] <= 1e-4).sum(), apart.min()))
    assert apart.min() >= lpr.IK_APART[name]                          # (what the numpy scheme shows: tests/test_load_profile.py)


# ---- 7. lifetime -----------------------------------------------------------------------------------------------------------
def test_set_call_clear_call(world):
    robot, _, fx, eng = world("config3_rot")
    st, d = fx["states"], fx["dist_B"]
    plain = eng.fk_loaded_batch(st, dist=d)
    eng.set_load_profile(*lpr.profile("zig", robot.specs.L))
    try:
        under = eng.fk_loaded_batch(st, dist=d)
    finally:
        eng.clear_load_profile()
    assert np.abs(under["p"] - plain["p"]).max() > 1e-3
    assert_same(eng.fk_loaded_batch(st, dist=d), plain, KEYS)


def test_a_queued_call_keeps_the_profile_it_was_issued_under(world):
    import torch
    robot, _, fx, eng = world("config1")
    st, d = fx["states"], fx["dist_B"]
    prof = lpr.profile("tip", robot.specs.L)
    n, P, ld, dev = len(st), eng.num_points, 64, "cuda:0"
    plain = eng.fk_loaded_batch(st, dist=d)
    with eng.load_profile_scope(prof):
        under = eng.fk_loaded_batch(st, dist=d)
    d_st, d_d = torch.from_numpy(st).to(dev), torch.from_numpy(d).to(dev)
    stream = torch.cuda.Stream()

    def queued(install):
        planes = torch.zeros((3, P, ld), dtype=torch.float64, device=dev)
        vu0 = torch.zeros((n, 6), dtype=torch.float64, device=dev)
        stream.wait_stream(torch.cuda.current_stream())
        eng.fk_loaded_batch_dev(d_st, n, ld, planes[0], planes[1], planes[2], d_dist=d_d, d_vu0=vu0, stream=stream)
        install()                                                     # while the call's last launches may still be queued
        stream.synchronize()
        return planes[:, :, :n].cpu().numpy().transpose(2, 1, 0), vu0.cpu().numpy()

    try:
        p, y = queued(lambda: eng.set_load_profile(*prof))
        assert same_bits(p, plain["p"]) and same_bits(y, plain["vu0"])
        p, y = queued(eng.clear_load_profile)
        assert same_bits(p, under["p"]) and same_bits(y, under["vu0"])
    finally:
        eng.clear_load_profile()


def test_the_per_call_profile_is_restored(world, irt):
    robot, _, fx, eng = world("config1")
    L = robot.specs.L
    st, d = fx["states"][:5], fx["dist_B"][:5]
    zig, tip = lpr.profile("zig", L), lpr.profile("tip", L)
    with eng.load_profile_scope(tip):
        want = eng.fk_loaded_batch(st, dist=d)
    plain = eng.fk_loaded_batch(st, dist=d)
    got = robot.general_shape_batch(st, f_e=d[:, :3], l_e=d[:, 3:], load_profile=tip)
    assert_same(got, want, KEYS)
    assert eng.load_profile() is None and eng.load_profile_table().size == 0
    one = robot.general_shape(st[2], f_e=d[2, :3], l_e=d[2, 3:], load_profile=tip)
    assert same_bits(one.p, want["p"][2])
    jac = robot.tip_jacobian_loaded_batch(st, f_e=d[0, :3], l_e=d[0, 3:], load_profile=tip)
    with eng.load_profile_scope(tip):
        assert same_bits(jac["J"], eng.tip_jacobian_loaded(st, dist=d[0])["J"])
    eng.set_load_profile(*zig)
    try:
        tab = eng.load_profile_table()
        with pytest.raises(irt.InvalidArgument):
            robot.general_shape_batch(np.zeros((2, robot.state_size() + 1)), f_e=d[0, :3], load_profile=tip)     # raises under `tip`
        assert same_bits(eng.load_profile_table(), tab)
        with pytest.raises(irt.InvalidArgument):
            robot.general_shape_batch(st, f_e=d[:, :3], load_profile=([0.0, 0.0], [1.0, 2.0]))                    # refused knots
        assert same_bits(eng.load_profile_table(), tab)
        assert_same(robot.general_shape_batch(st, f_e=d[:, :3], l_e=d[:, 3:], load_profile=tip), want, KEYS)
        assert same_bits(eng.load_profile_table(), tab)
    finally:
        eng.clear_load_profile()
    assert_same(eng.fk_loaded_batch(st, dist=d), plain, KEYS)
