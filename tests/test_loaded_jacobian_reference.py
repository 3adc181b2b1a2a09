"""The specification of the loaded tip Jacobian and compliance (tests/loaded_jacobian_reference.py) against the 40-digit truth of
its lanes (tests/golden/loaded_lin_truth_<name>.npz, make_loaded_lin_truth.py) and against what J and C mean (central differences
of shooting solves taken to 1e-12 N).  No GPU.

The tolerances of tests/test_gpu_loaded_jacobian.py are MEASURED here, on the reference alone; the device tests use 4 x the figure,
the project's factor.  Every figure is re-measured by the test named beside it, which holds the table to within a factor 2.

  END_TO_END   max |helper - differenced solves| / max |differenced solves| over the first 6 states of case C, per robot and block
               (test_helper_has_the_meaning_of_differenced_solves).  The helper is evaluated where a shooting may stop: at the
               twelve points around the equilibrium whose residual is residual_threshold along -+ each residual axis
               (loaded_jacobian_reference.stop_points) -- at the equilibrium itself J misses by ~2e-6 of FD truncation only, at the
               threshold by ten times that, and a device solve stops anywhere in between.  The residual ball's worst direction is at
               most sqrt(6) times the worst axis, to first order; the factor 4 covers it.
  REDUCTION    max |np.linalg.solve - mpmath| / (kappa_inf(J_y) eps |result|_inf) of W, J, C, y_c, x_c reduced from the helper's own
               fp64 blocks, over the four truth fixtures (test_reduction_arithmetic)
  ZERO_LOAD    max |helper's J at zero load - central differences of the oracle's unloaded tip| / max |the latter|, first 6
               states, the helper at the unloaded start strains and at the twelve stop points around the zero-load equilibrium, the
               worst of the thirteen (test_zero_load_is_the_unloaded_jacobian): at the start alone 1.2e-6 / 1.3e-6

                 END_TO_END   J         C            REDUCTION   1.3e-4        ZERO_LOAD
                 config1      4.7e-5    5.2e-5                                 config1      4.5e-5
                 config3_rot  6.9e-5    4.9e-5                                 config3_rot  7.0e-5
                 n8           4.9e-4    4.1e-5
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.join(HERE, "golden")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import fk_truth_common as ftc                                        # noqa: E402
import loaded_fk_reference as ref                                    # noqa: E402
import loaded_ik_reference as ikr                                    # noqa: E402
import loaded_jacobian_reference as ljr                              # noqa: E402
import make_loaded_lin_truth as mlt                                  # noqa: E402

END_TO_END = {"config1": dict(J=4.7e-5, C=5.2e-5), "config3_rot": dict(J=6.9e-5, C=4.9e-5), "n8": dict(J=4.9e-4, C=4.1e-5)}
REDUCTION = 1.3e-4
ZERO_LOAD = {"config1": 4.5e-5, "config3_rot": 7.0e-5}
FACTOR = 4.0

BLOCKS = ("J_y", "J_p", "X_y", "X_p")


def held(measured, table):
    """the table holds the measurement, and is not more than twice as wide"""
    return table / 2 <= measured <= table


@pytest.fixture(scope="module")
def gen(orc):
    import make_loaded_fk
    return make_loaded_fk


@pytest.fixture(scope="module")
def truth(gen):
    """name -> (oracle robot, truth fixture, frame)"""
    cache = {}

    def get(name):
        if name not in cache:
            _, rob, st = gen.fixture(name)
            fx = mlt.load(name)
            assert np.array_equal(st[:mlt.N_STATES], fx["states"])
            cache[name] = (rob, fx, mlt.NAMES[name])
        return cache[name]
    return get


def lanes_of(rob, fx, frame, **kw):
    """the reference's lanes of every state of a truth fixture, one call per state (one load set per call)"""
    out = [ljr.lanes(rob, fx["states"][i:i + 1], fx["vu0"][i:i + 1], fx["wrench"][i], fx["dist"][i], frame, mlt.DELTA, mlt.DELTA_Y, **kw)
           for i in range(len(fx["states"]))]
    return tuple(np.concatenate([o[k] for o in out]) for k in range(3))


def states_outside(fx, blocks):
    """(n,) bool: some entry of the four blocks leaves the bound of the truth's quotient"""
    tb = mlt.truth_blocks(fx)
    out = np.zeros(len(fx["states"]), bool)
    for key, got in zip(BLOCKS, blocks):
        want, bound = tb[key]
        out |= (np.abs(got - want) > bound).any(axis=(1, 2))
    return out


@pytest.mark.parametrize("name", list(mlt.NAMES))
def test_reference_reproduces_the_stored_reference_errors(truth, name):
    rob, fx, frame = truth(name)
    x, e, d = lanes_of(rob, fx, frame)
    assert np.array_equal(d, fx["lane_d"])
    assert np.array_equal(ftc.err_vs_truth(x, fx["x_hi"], fx["x_lo"]), fx["Eref_x"])
    assert np.array_equal(ftc.err_vs_truth(e, fx["e_hi"], fx["e_lo"]), fx["Eref_e"])


@pytest.mark.parametrize("name", list(mlt.NAMES))
def test_two_lanes_rerun_in_mpmath_agree_with_the_fixture(truth, name):
    import make_fk_truth as mft
    _, _, model, _ = mlt.fixture_inputs(name, [1])
    consts, C, D, steps = model
    _, fx, _ = truth(name)
    Q = fx["lane_d"].shape[1]
    for q in (2, Q - 2):                                                # a strain lane and the last state entry's -d lane (theta)
        tip, e, _ = mlt.lane_model(consts, C, D, fx["lane_states"][1, q], fx["lane_vu"][1, q], steps, fx["wrench"][1], fx["dist"][1],
                                   bool(fx["world"]))
        for vals, key in ((tip, "x"), (e, "e")):
            for k, v in enumerate(vals):
                stored = mft.mp.mpf(float(fx[key + "_hi"][1, q, k])) + mft.mp.mpf(float(fx[key + "_lo"][1, q, k]))
                assert abs(v - stored) <= 1e-30 + abs(v) * 2.0 ** -76, (name, q, key, k)


@pytest.mark.parametrize("name", list(mlt.NAMES))
def test_reference_blocks_lie_within_the_difference_bound(truth, name):
    rob, fx, frame = truth(name)
    x, e, d = lanes_of(rob, fx, frame)
    blocks = ljr.blocks_from_lanes(x, e, d)
    tb = mlt.truth_blocks(fx)
    worst = max(float((np.abs(got - tb[key][0]) / tb[key][1]).max()) for key, got in zip(BLOCKS, blocks))
    print("%s: worst error / bound of the reference's blocks %.3f" % (name, worst))
    assert not states_outside(fx, blocks).any()
    for i in range(len(fx["states"])):                                  # linearise forms the same blocks from the same lanes
        lin = ikr.linearise(rob, fx["states"][i:i + 1], fx["vu0"][i:i + 1], fx["wrench"][i], fx["dist"][i], frame, mlt.DELTA, mlt.DELTA_Y)
        for key, got in zip(BLOCKS, blocks):
            assert np.array_equal(lin[key][0], got[i])


def test_mutations_leave_the_bound(truth):
    """Each mutation leaves the bound on every state of at least one fixture; the reference itself leaves it on none
    (test_reference_blocks_lie_within_the_difference_bound)."""
    counts = {}
    for name in mlt.NAMES:
        rob, fx, frame = truth(name)
        x, e, d = lanes_of(rob, fx, frame)
        # a forward difference in place of the central one: (f(+d) - f(0)) / d
        fwd = lambda a, first, cnt: np.transpose((a[:, first + 1:first + 2 * cnt:2] - a[:, :1]) / d[:, first + 1:first + 2 * cnt:2, None], (0, 2, 1))
        S = fx["states"].shape[1]
        counts.setdefault("forward", {})[name] = int(states_outside(fx, (fwd(e, 1, 6), fwd(e, 13, S), fwd(x, 1, 6), fwd(x, 13, S))).sum())
        # levmar's relative step on the strains
        counts.setdefault("levmar", {})[name] = int(states_outside(fx, ljr.blocks_from_lanes(*lanes_of(rob, fx, frame, strain_steps="levmar"))).sum())
        # a theta-perturbed lane that keeps the unperturbed load rows (frame WORLD only)
        if frame == "world":
            counts.setdefault("rows", {})[name] = int(states_outside(fx, ljr.blocks_from_lanes(*lanes_of(rob, fx, frame, turn_with="state"))).sum())
    print("states outside the bound, of %d: %s" % (mlt.N_STATES, counts))
    for kind, per in counts.items():
        assert max(per.values()) == mlt.N_STATES, (kind, per)


def call_sets(gen, name, case, rows):
    """(oracle robot, states, wrench rows, dist rows, frame): the call's load set of every state, as the truth fixtures have it"""
    _, rob, st = gen.fixture(name)
    lf = dict(np.load(gen.path(name)))
    frame = mlt.NAMES[name]
    w, d = lf["wrench_" + case][rows], lf["dist_" + case][rows]
    st = np.ascontiguousarray(st[rows])
    if frame == "world":
        w, d = mlt.world_set(w, st[:, rob.n_tendons]), mlt.world_set(d, st[:, rob.n_tendons])
    return rob, st, w, d, frame


def helper_at(rob, st, y, w, d, frame):
    out = [ljr.sensitivities(rob, st[i:i + 1], y[i:i + 1], w[i], d[i], frame) for i in range(len(st))]
    return {k: np.concatenate([o[k] for o in out]) for k in ("J", "C", "W", "x_c", "y_c", "T", "X_y", "J_y")}


@pytest.mark.parametrize("name", list(END_TO_END))
def test_helper_has_the_meaning_of_differenced_solves(gen, name):
    rob, st, w, d, frame = call_sets(gen, name, "C", np.arange(6))
    fd = ljr.differenced_solves(rob, st, w, d, frame)
    assert fd["converged"].all()
    at_eq = helper_at(rob, st, fd["y"], w, d, frame)
    assert np.abs(at_eq["x_c"] - fd["tip"]).max() <= 1e-11
    pts = ljr.stop_points(rob, st, fd["y"], w, d, frame)
    worst = dict(J=0.0, C=0.0, tip=0.0)
    no_T = np.ones(len(st), bool)
    for k in range(12):
        h = helper_at(rob, st, pts[:, k], w, d, frame)
        worst["J"] = max(worst["J"], float(ljr.relative_gap(h["J"], fd["J"]).max()))
        worst["C"] = max(worst["C"], float(ljr.relative_gap(h["C"], fd["C"]).max()))
        worst["tip"] = max(worst["tip"], float(np.abs(h["x_c"] - fd["tip"]).max()))
        # the mutation `compliance without T`: X_y J_y^-1 alone
        bare = h["X_y"] @ np.linalg.inv(h["J_y"])
        no_T &= ljr.relative_gap(bare, fd["C"]) > FACTOR * END_TO_END[name]["C"]
    print("%s: at the equilibrium J %.3g C %.3g; at the threshold J %.3g C %.3g, x_c within %.3g m; without T %d of %d states outside"
          % (name, ljr.relative_gap(at_eq["J"], fd["J"]).max(), ljr.relative_gap(at_eq["C"], fd["C"]).max(), worst["J"], worst["C"],
             worst["tip"], no_T.sum(), len(st)))
    assert held(worst["J"], END_TO_END[name]["J"]) and held(worst["C"], END_TO_END[name]["C"]), worst
    assert worst["tip"] <= 1e-9
    if frame == "world":
        assert no_T.all()


def mp_reduce(y, x, e, J_y, J_p, X_y, X_p, T):
    """reduce_blocks for one point in mpmath (40 digits), from the same fp64 blocks"""
    import make_fk_truth as mft
    mp = mft.mp
    M = lambda a: mp.matrix(np.asarray(a, float).tolist())
    Jy, Jp, Xy, Xp = M(J_y), M(J_p), M(X_y), M(X_p)
    def solve(B):                                                       # column by column: lu_solve takes vectors
        out = mp.matrix(6, B.cols)
        for j in range(B.cols):
            col = mp.lu_solve(Jy, B[:, j])
            for i in range(6):
                out[i, j] = col[i]
        return out

    W, c, G = solve(Jp), solve(M(np.asarray(e)[:, None])), solve(M(T))
    f = lambda m: np.array([[float(m[i, j]) for j in range(m.cols)] for i in range(m.rows)])
    return dict(W=f(W), J=f(Xp - Xy * W), C=f(Xy * G), y_c=f(M(np.asarray(y)[:, None]) - c)[:, 0], x_c=f(M(np.asarray(x)[:, None]) - Xy * c)[:, 0])


def reduction_ratio(fp, mpv, J_y):
    """max over the results of |fp64 - mpmath| / (kappa_inf(J_y) eps |result|_inf)"""
    kappa = np.linalg.cond(J_y, np.inf)
    eps = np.finfo(float).eps
    return max(float(np.abs(fp[k] - mpv[k]).max() / (kappa * eps * np.abs(mpv[k]).max())) for k in mpv)


def test_reduction_arithmetic(truth):
    worst = 0.0
    for name in mlt.NAMES:
        rob, fx, frame = truth(name)
        for i in range(len(fx["states"])):
            s = ljr.sensitivities(rob, fx["states"][i:i + 1], fx["vu0"][i:i + 1], fx["wrench"][i], fx["dist"][i], frame)
            y, x, e = s["point"]
            mpv = mp_reduce(y[0], x[0], e[0], s["J_y"][0], s["J_p"][0], s["X_y"][0], s["X_p"][0], s["T"][0])
            worst = max(worst, reduction_ratio({k: s[k][0] for k in mpv}, mpv, s["J_y"][0]))
    print("reduction: worst |np.linalg.solve - mpmath| / (kappa eps |result|) = %.3g" % worst)
    assert held(worst, REDUCTION)


@pytest.mark.parametrize("name", list(ZERO_LOAD))
def test_zero_load_is_the_unloaded_jacobian(gen, name):
    _, rob, st = gen.fixture(name)
    st = np.ascontiguousarray(st[:6])
    y = ref.unloaded_start(rob, st[:, :rob.n_tendons])
    h = ljr.sensitivities(rob, st, y)
    Jo = ljr.unloaded_differences(rob, st)
    at_start = float(ljr.relative_gap(h["J"], Jo).max())
    assert np.isfinite(h["C"]).all()
    # the unloaded start is not the rod's discrete equilibrium (the tip balance of the RK4 solution misses by up to the threshold
    # itself), and a cold solve stops anywhere within the threshold of it: the twelve stop points around the tight solve
    eq = ref.shoot(rob, st, tol=ljr.SOLVE_TOL, max_iters=20)
    assert eq["converged"].all()
    pts = ljr.stop_points(rob, st, eq["vu0"])
    gap = max([at_start] + [float(ljr.relative_gap(ljr.sensitivities(rob, st, pts[:, k])["J"], Jo).max()) for k in range(12)])
    print("%s: helper at zero load against the oracle's differences: %.3g at the unloaded start (|e| <= %.3g N), %.3g at the threshold"
          % (name, at_start, np.linalg.norm(h["point"][2], axis=1).max(), gap))
    assert held(gap, ZERO_LOAD[name])
