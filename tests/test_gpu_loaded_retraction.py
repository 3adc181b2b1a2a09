"""The loaded FK of robots WITH retraction on the device (fk_loaded_retract<N>, shoot_start_retract<N>: csrc/fk_loaded_retract_kernel.hpp)
through tr_fk_loaded_batch*, tr_fk_loaded_tips*, tr_fk_loaded_batch_retraction_dev and Engine.validate_loaded.

Fixtures: tests/golden/loaded_ret_truth_<name>.npz (make_loaded_ret_truth.py: five robots, 24 states each on its own grid
t_range(s_start, L, dL), load cases A -- one wrench, NO distributed load, passed as dist = None -- and D -- all twelve load numbers
non-zero) and the unloaded fk_truth_<name>.npz.  Only .npz files and the oracle are read.

  (a) ONE integration from the fixture's strains (guess = vu0, max_iters = 0) against the 40-digit truth within
      fk_truth_common.loaded_bounds: points, tip frame, L, L_i, tip strains, and |e| within `enorm`, the sum of the six component
      bounds (the call returns the residual's norm, not its components); the point counts, zero iterations, one integration, the guess
      echoed bit for bit; `converged` agrees with the truth wherever | |e| - threshold | exceeds the bound.  Rows 12 and 13 of the
      dL = L / 40 fixtures (s_start >= L) integrate nothing and are asserted exactly; a negative s_start reports unconverged.
  (b) zero load from the unloaded start against the UNLOADED truth (fk_truth_common.compare) on every retraction fixture.
  (c) the shooting: cold start, default parameters, converges on every row the reference converged on (all), every stored point
      within the fixture's bound_i of the reference's shape; from guess = vu0 at most one LM iteration.
  (d) launch shapes, bit for bit: without frames, 72 problems, the device form, the tips alone, a permuted batch.
  (e) validity of loaded shapes against the oracle's predicate on the device's own points; the per-configuration home lengths.
  (f) robot.general_shape and tip_forces.
  (g) what stays refused on a retraction robot, each call under its own name.
  (h) an engine that was never opened (Engine.set_loaded_retraction) refuses every loaded call with the one message it always had.
Every call of (a) - (f) raised Unsupported before the loaded FK took retraction robots; the engines of (a) - (g) are opened."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.join(HERE, "golden")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import fk_truth_common as ftc                                        # noqa: E402
import loaded_ret_common as lrc                                      # noqa: E402

pytestmark = pytest.mark.gpu

KEYS = ("p", "L", "L_i", "converged", "n_points", "vu0", "vuL", "residual", "iters", "num_fk_calls")
_cache = {}


def _world(irt, name):
    """(fixture, robot, engine) of a loaded-retraction fixture"""
    if name not in _cache:
        fx = lrc.load(name)
        robot = ftc.robot_from_fixture(irt, fx)
        robot.engine(0).set_loaded_retraction()                      # every test below runs on an engine opened to retraction robots
        _cache[name] = (fx, robot, robot.engine(0))
    return _cache[name]


def _args(fx, case, rows=slice(None)):
    d = lrc.dist_of(fx, case)
    return dict(wrench=fx["wrench_" + case][rows], dist=None if d is None else d[rows])


def _once(irt, name, case, kind):
    """kind 'truth': one integration from vu0; 'cold': the full shooting from the unloaded start"""
    if (name, case, kind) not in _cache:
        fx, _, eng = _world(irt, name)
        extra = dict(guess=fx["vu0_" + case], max_iters=0) if kind == "truth" else {}
        _cache[name, case, kind] = eng.fk_loaded_batch(fx["states"], want_R=True, **extra, **_args(fx, case))
    return _cache[name, case, kind]


def _same(a, b, rows_a=slice(None), rows_b=slice(None), keys=KEYS):
    for k in keys:
        assert np.array_equal(a[k][rows_a], b[k][rows_b], equal_nan=True), k


def _host_layout(out):
    """every state's points from row 0, NaN behind them"""
    P = out["p"].shape[1]
    for i, k in enumerate(out["n_points"]):
        assert 1 <= k <= P and np.isfinite(out["p"][i, :k]).all() and np.isnan(out["p"][i, k:]).all(), i
        if out["R"] is not None:
            assert np.isfinite(out["R"][i, :k]).all() and np.isnan(out["R"][i, k:]).all(), i


# ---- (a) ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", lrc.CASES)
@pytest.mark.parametrize("name", lrc.NAMES)
def test_loaded_integration_against_truth(irt, name, case):
    fx, _, _ = _world(irt, name)
    out = _once(irt, name, case, "truth")
    thr = float(fx["consts"][7])
    keep = lrc.truth_rows(fx)
    assert (out["iters"] == 0).all() and (out["num_fk_calls"] == 1).all() and out["rounds"] == 1
    assert np.array_equal(out["vu0"], fx["vu0_" + case])                                # bit for bit the guess
    assert np.array_equal(out["n_points"], fx["n_points"])
    _host_layout(out)
    errs = lrc.errors(fx, case, out["p"], lrc.tip_frames(out["R"], out["n_points"]), out["L"], out["L_i"], out["vuL"], np.zeros((lrc.N, 6)))
    ratio = lrc.ratios(fx, case, errs)[:, :5]                                           # p, R, L, L_i, vu
    b = ftc.loaded_bounds(fx, case)
    en = ftc.loaded_e_norm(fx, case)
    r_e = np.where(keep, np.abs(out["residual"] - en) / b["enorm"], 0.0)
    print("%s %s: error / bound: p %.3f R %.3f L %.3f L_i %.3f vu %.3f |e| %.3f; bound p <= %.2g m, |e| <= %.2g N; |e_truth| <= %.2g N"
          % ((name, case) + tuple(ratio.max(axis=0)) + (r_e.max(), b["p"][keep].max(), b["enorm"][keep].max(), en[keep].max())))
    assert (ratio <= 1.0).all(), np.argwhere(ratio > 1.0)
    assert (r_e <= 1.0).all(), np.flatnonzero(r_e > 1.0)
    clear = keep & (np.abs(en - thr) > b["enorm"])                   # the truth decides the flag with the bound to spare
    assert np.array_equal(out["converged"][clear], (en <= thr)[clear])
    # s_start >= L: the reference's early return, exactly
    for i in fx["no_truth"]:
        assert out["n_points"][i] == 1 and not out["p"][i, 0].any() and out["L"][i] == 0.0 and not out["L_i"][i].any()
        assert out["converged"][i] and out["iters"][i] == 0 and out["residual"][i] == 0.0


def test_a_negative_s_start_is_reported_unconverged(irt):
    fx, _, eng = _world(irt, "config3_ret_edges")
    st = fx["states"][:5].copy()
    st[1::2, -1] = -0.01
    out = eng.fk_loaded_batch(st, **_args(fx, "D", slice(0, 5)))
    assert not out["converged"][1::2].any() and (out["n_points"][1::2] == 1).all() and (out["iters"][1::2] == 0).all()
    assert not out["p"][1::2, 0].any() and not out["L"][1::2].any()
    _same(out, _once(irt, "config3_ret_edges", "D", "cold"), slice(0, 5, 2), slice(0, 5, 2))


# ---- (b) ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ftc.RETRACTION)
def test_zero_load_against_the_unloaded_truth(irt, name):
    un = ftc.load(name)
    eng = _world(irt, name)[2]
    out = eng.fk_loaded_batch(un["states"], guess=np.hstack([un["v0"], un["u0"]]), max_iters=0, want_R=True)
    assert np.array_equal(out["n_points"], un["n_points"])
    worst, ok = ftc.compare(un, out["p"], lrc.tip_frames(out["R"], out["n_points"]), out["L"], out["L_i"])
    print("%s: worst error / bound %.3f" % (name, worst))
    assert ok.all(), np.flatnonzero(~ok)


# ---- (c) ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", lrc.CASES)
@pytest.mark.parametrize("name", lrc.NAMES)
def test_the_shooting_reaches_the_reference_shape(irt, name, case):
    fx, _, eng = _world(irt, name)
    out = _once(irt, name, case, "cold")
    assert out["converged"].all(), np.flatnonzero(~out["converged"])                    # the reference converged on every row
    assert np.array_equal(out["n_points"], fx["n_points"])
    _host_layout(out)
    err = np.linalg.norm(lrc.stored(fx, out["p"]) - fx["shoot_p_" + case], axis=2).max(axis=1)
    bound = fx["bound_" + case]
    print("%s %s: points %.3g of bound (bound <= %.3g m), iters <= %d, rounds %d" % (name, case, (err / bound).max(), bound.max(), out["iters"].max(), out["rounds"]))
    assert (err <= bound).all(), np.flatnonzero(err > bound)
    warm = eng.fk_loaded_batch(fx["states"], guess=fx["vu0_" + case], **_args(fx, case))
    assert warm["converged"].all() and (warm["iters"] <= 1).all(), warm["iters"]


# ---- (d) ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("config3_ret_edges", "n8_ret"))       # two waves per SIMD with every special row; one wave
def test_shapes_of_the_launch_do_not_change_a_bit(irt, name):
    import torch
    fx, _, eng = _world(irt, name)
    st, kw = fx["states"], _args(fx, "D")
    full = _once(irt, name, "D", "cold")
    _same(eng.fk_loaded_batch(st, **kw), full)                                          # without the frames (WRITE_R = false)
    # 72 problems: two waves and a masked tail in the start launch, each problem's 13 lanes straddling waves of mixed s_start
    idx = np.arange(72) % 24
    _same(eng.fk_loaded_batch(st[idx], **_args(fx, "D", idx)), full, rows_b=idx)
    perm = np.random.default_rng(5).permutation(24)
    _same(eng.fk_loaded_batch(st[perm], **_args(fx, "D", perm)), full, rows_b=perm)
    tips = eng.fk_loaded_tips(st, **kw)
    assert np.array_equal(tips["tips"], full["p"][np.arange(24), full["n_points"] - 1])
    assert np.array_equal(tips["converged"], full["converged"]) and np.array_equal(tips["vu0"], full["vu0"])
    # the device form: rows aligned at the tip, state i's point j in row j + P - n_points[i]
    n, P, ld, dev = 24, eng.num_points, 64, "cuda:0"
    planes = torch.full((3, P, ld), float("nan"), dtype=torch.float64, device=dev)
    npts = torch.zeros(n, dtype=torch.int32, device=dev)
    vu0 = torch.empty((n, 6), dtype=torch.float64, device=dev)
    conv = torch.empty(n, dtype=torch.uint8, device=dev)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    eng.fk_loaded_batch_dev(up(st), n, ld, planes[0], planes[1], planes[2], d_wrench=up(kw["wrench"]), d_dist=up(kw["dist"]), d_npts=npts,
                            d_vu0=vu0, d_conv=conv)
    torch.cuda.synchronize()
    assert np.array_equal(npts.cpu().numpy(), full["n_points"]) and np.array_equal(vu0.cpu().numpy(), full["vu0"])
    assert np.array_equal(conv.cpu().numpy().astype(bool), full["converged"])
    got = planes[:, :, :n].cpu().numpy().transpose(2, 1, 0)                             # (n, P, 3)
    for i, k in enumerate(full["n_points"]):
        assert np.array_equal(got[i, P - k:], full["p"][i, :k]) and np.isnan(got[i, :P - k]).all(), i


# ---- (e) ----------------------------------------------------------------------------------------------------------------------
def test_validity_of_loaded_shapes(irt, orc):
    """config3_rot_ret under case D on a grid with spheres on three loaded tips (make_loaded_fk.verdict_obstacles' grid and sphere
    size): Engine.validate_loaded equals the oracle's predicate applied to the DEVICE's host-form points -- converged,
    is_within_length_limits(home_shape(s_start).L_i, L_i), collides_self, the voxel test."""
    import torch
    import make_fk_truth as mft
    import make_loaded_fk as mlf
    fx, robot, eng = _world(irt, "config3_rot_ret")
    orb = mft.oracle_robot(robot)
    st, kw = fx["states"], _args(fx, "D")
    out = _once(irt, "config3_rot_ret", "D", "cold")
    pts = [out["p"][i, :k] for i, k in enumerate(out["n_points"])]
    N, half = mlf.GRID_N, mlf.GRID_HALF
    lim = (-half, half) * 3
    radius = mlf.SPHERE_VOXELS * 2 * half / N
    g = orc.Grid(N, lim)
    for i in (2, 9, 17):
        g.add_sphere(pts[i][-1], radius)
    eng.set_grid(N, lim, g.blocks())
    got = eng.validate_loaded(st, **kw)

    def predicate(i):
        if not out["converged"][i] or not orb.is_within_length_limits(orb.home_shape(st[i, -1])["L_i"], out["L_i"][i]) or orb.collides_self(pts[i]):
            return False
        line = g.empty_copy()
        line.add_piecewise_line(pts[i])
        return not g.collides(line)
    want = np.array([predicate(i) for i in range(24)])
    assert not want[[2, 9, 17]].any() and want.any()
    assert np.array_equal(got["valid"], want), np.flatnonzero(got["valid"] != want)
    # the per-configuration home lengths of the loaded call against the unloaded truth's
    un = ftc.load("config3_rot_ret")
    n, P, Nt, ld, dev = 24, eng.num_points, eng.n_tendons, 64, "cuda:0"
    planes = torch.empty((3, P, ld), dtype=torch.float64, device=dev)
    Li, home = (torch.empty((Nt, ld), dtype=torch.float64, device=dev) for _ in range(2))
    npts, conv = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    eng.fk_loaded_batch_retraction_dev(up(st), n, ld, planes[0], planes[1], planes[2], Li, conv, npts, home, d_wrench=up(kw["wrench"]),
                                       d_dist=up(kw["dist"]))
    torch.cuda.synchronize()
    h = home[:, :n].cpu().numpy().T
    bound = 4.0 * (un["Eref_home"] + 4.0 * np.spacing(np.abs(un["home_hi"])))
    err = ftc.err_vs_truth(h, un["home_hi"], un["home_lo"])
    print("home lengths: %.3f of bound" % (err / bound).max())
    assert (err <= bound).all()
    assert np.array_equal(Li[:, :n].cpu().numpy().T, out["L_i"]) and np.array_equal(npts.cpu().numpy(), out["n_points"])
    # zero load: the unloaded checker's verdicts
    zero, plain = eng.validate_loaded(st), eng.validate_batch(st)
    assert np.array_equal(zero["valid"], plain["valid"]) and np.array_equal(zero["flags"], plain["flags"])


# ---- (f) ----------------------------------------------------------------------------------------------------------------------
def test_general_shape_of_a_retraction_robot(irt):
    fx, robot, _ = _world(irt, "config3_ret_edges")
    full = _once(irt, "config3_ret_edges", "D", "cold")
    w, d = fx["wrench_D"], fx["dist_D"]
    thr = robot.residual_threshold
    for i in (1, 3, 10):                                             # three of the special rows; row 10 is a two-point backbone
        st = fx["states"][i]
        res = robot.general_shape(st, f_e=d[i, :3], l_e=d[i, 3:], F_e=w[i, :3], L_e=w[i, 3:])
        k = int(full["n_points"][i])
        assert len(res.t) == k and res.p.shape == (k, 3) and res.R.shape == (k, 3, 3)
        assert np.array_equal(res.p, full["p"][i, :k]) and res.L == full["L"][i] and np.array_equal(res.L_i, full["L_i"][i])
        assert np.array_equal(np.r_[res.v_i, res.u_i], full["vu0"][i]) and np.array_equal(np.r_[res.v_f, res.u_f], full["vuL"][i])
        assert res.t[0] == pytest.approx(st[-1], abs=1e-15) and res.t[-1] == robot.specs.L and res.converged
        # config3_ret_edges has no rotation: result.R is the base frame, and the tip balance returns the wrench within the residual
        tip = robot.tip_forces(st, res)
        assert np.linalg.norm(np.r_[tip.F_e - w[i, :3], tip.L_e - w[i, 3:]]) <= 1.01 * thr
        robot.base_forces(st, res)
    batch = robot.general_shape_batch(fx["states"][:3], f_e=d[:3, :3], l_e=d[:3, 3:], F_e=w[:3, :3], L_e=w[:3, 3:])
    _same(batch, full, rows_b=slice(0, 3))


# ---- (g) ----------------------------------------------------------------------------------------------------------------------
def test_what_stays_refused_on_a_retraction_robot(irt):
    fx, robot, eng = _world(irt, "config3_rot_ret")
    st = fx["states"][:2]
    vox, _ = irt.workloads.reach_environment(seed=7, n_spheres=4)
    eng.set_grid(vox.Nx(), vox.limits(), vox.blocks)
    loads = dict(wrench=fx["wrench_A"][0])
    calls = dict(set_load_profile=lambda: eng.set_load_profile([0.0, 0.1], [1.0, 2.0]),
                 validate_edges_loaded=lambda: eng.validate_edges_loaded(st, st[::-1], **loads),
                 ik_loaded_batch=lambda: eng.ik_loaded_batch(st, np.zeros(3), **loads),
                 tip_jacobian_loaded=lambda: eng.tip_jacobian_loaded(st, **loads),
                 sample_valid_vertices_loaded=lambda: eng.sample_valid_vertices_loaded(4, **loads),
                 set_loads=lambda: irt.VoxelBackboneValidityChecker(robot, irt.VoxelEnvironment(), vox).set_loads(**loads))
    messages = {}
    for name, call in calls.items():
        with pytest.raises(irt.Unsupported, match="retraction") as e:
            call()
        messages[name] = str(e.value)
    assert len(set(messages.values())) == len(messages), messages                       # each under its own name
    with pytest.raises(irt.Unsupported, match="retraction"):
        irt.load_profile_table(robot, [0.0, 0.1], [1.0, 2.0])


# ---- (h) ----------------------------------------------------------------------------------------------------------------------
def test_an_engine_that_was_never_opened_refuses_as_before(irt):
    fx, robot, opened = _world(irt, "config3_ret_edges")
    st = fx["states"][:2]
    eng = irt.Engine(robot, 0)
    calls = (lambda: eng.fk_loaded_batch(st), lambda: eng.fk_loaded_tips(st), lambda: eng.ik_loaded_batch(st, np.zeros(3)),
             lambda: eng.tip_jacobian_loaded(st), lambda: eng.set_load_profile([0.0, 0.1], [1.0, 2.0]))
    messages = set()
    for call in calls:
        with pytest.raises(irt.Unsupported, match="loaded FK \\(general_shape\\) is not built for robots with retraction") as e:
            call()
        messages.add(str(e.value))
    assert len(messages) == 1
    eng.set_loaded_retraction()
    _same(eng.fk_loaded_batch(st), opened.fk_loaded_batch(st))
    eng.set_loaded_retraction(False)
    with pytest.raises(irt.Unsupported):
        eng.fk_loaded_batch(st)
    eng.close()
