"""The integrator of the FK kernels against an extended-precision evaluation of the scheme they restate.

The fixtures tests/golden/fk_truth_*.npz (tests/golden/make_fk_truth.py) hold, for 24 states of nineteen small robots, the
40-digit result of the discrete scheme (dense 6x6 right-hand side, classical RK4 over the oracle's step sequence, exact
start values) and two CPU-side error figures per state: E_ref, how far the fp64 oracle is from that truth, and E_design,
how far one Newton step's 2e-14 in the kernels' reciprocals moves it.  Every output of every state must lie within
4 (E_ref + E_design) of the truth (floor: 4 ulp) -- 1e-16 to 1e-12 where the parity tests ask for 1e-9 m, so a dropped
Newton step, a routing term from the wrong stage row or a lost factor in a small term shows.  Nothing here reads anything
but the .npz files: no mpmath, no oracle, no reference.

  (a) the stored-point kernels (fk_rk4_batch_uniform<N>, fk_rk4_batch_retract<N>; rotation epilogue, R output), at batch
      sizes that put the fixture's states into other lanes and waves, bit for bit the same;
  (b) the tips-only form (tr_fk_tips, tr_fk_tips_dev);
  (c) fk_verdict<N>, which stores no point: its length test `home_Li[j] - Li[j]` against min_length / max_length serves as
      a comparator on its own L_i -- a limit placed one bound beyond a state's true length change must pass it, one bound
      short of it must reject it;
  (d) the retraction integrator where a lane's own first interval takes every path it has (fixtures *_ret_edges, n1_ret, n8_ret:
      aligned grids, two RK4 steps, two- and one-point backbones, s_start = L and beyond, N = 1, 3, 4, 8, rotation on and
      off), through tr_fk_batch_retraction_dev, which also returns the lane's home lengths -- Simpson's rule over its own
      points, the closed forms -- against a truth of their own, in arrival order and in the order of the backbone lengths;
  (e) fk_verdict_retract (prologue launch -> hand-over planes -> tip-aligned launch) through the same comparator, with the
      length change home - L_i taken per state from the two truths, and the tips all verdict kernels report;
  (f) fk_edge_queue, alone: edges that turn a state about the z axis, whose interior samples only the queue integrates and
      which all have the state's L_i, with the vertices' signature rows given so that no other kernel sees them;
  (g) the fused stored-point kernel fk_sweep_fused<N> (voxel caches, tr_connect_edges_indexed, TENDON_HIP_FUSED=1) and the
      separate K1 + K2 launches beside it, on every fixture without retraction, in both routing forms where the robot is a
      uniform helix;
  (h) fk_sweep_fused_list, the fallback pass of the verdict path, on tightly curled states of the 5- and 6-tendon robots -- the
      one test here that asks the oracle: its pairwise self-collision sweep on the device's own points."""
import numpy as np
import pytest

import fk_truth_common as ftc

pytestmark = pytest.mark.gpu
_cache = {}


def _fk(irt, name):
    """fixture, its robot and the stored-point result of its 24 states (computed once)."""
    if name not in _cache:
        fx = ftc.load(name)
        robot = ftc.robot_from_fixture(irt, fx)
        _cache[name] = (fx, robot, robot.shape_batch(fx["states"], want_R=True))
    return _cache[name]


def _tip_R(out):
    n = out["n_points"]
    return out["R"][np.arange(len(n)), n - 1]


def _same(a, b, rows_a, rows_b, what, keys=("p", "R", "L", "L_i", "converged", "n_points")):
    for k in keys:
        assert np.array_equal(a[k][rows_a], b[k][rows_b], equal_nan=k in ("p", "R")), (what, k)


@pytest.mark.parametrize("name", ftc.FIXTURES)
def test_stored_point_kernels_against_truth(irt, name):
    fx, robot, out = _fk(irt, name)
    st = fx["states"]
    assert out["converged"].all() and np.array_equal(out["n_points"], fx["n_points"])
    ratio, ok = ftc.compare(fx, out["p"], _tip_R(out), out["L"], out["L_i"])
    e, b = ftc.errors(fx, out["p"], _tip_R(out), out["L"], out["L_i"]), ftc.bounds(fx)
    print("%s: max error / bound %.3f (points %.3f, R %.3f, L %.3f, L_i %.3f); point error %.2g .. %.2g m, bound %.2g .. %.2g m"
          % (name, ratio, (e["p"] / b["p"]).max(), (e["R"] / b["R"]).max(), (e["L"] / b["L"]).max(), (e["L_i"] / b["L_i"]).max(),
             e["p"].min(), e["p"].max(), b["p"].min(), b["p"].max()))
    assert ok.all(), (np.flatnonzero(~ok), ratio)
    # the same states in other lanes and waves: 24 -> 65 and 130 columns, the rest copies of state 0
    rng = np.random.default_rng(5)
    every = np.arange(ftc.N_STATES)
    for n in (65, 130):
        pos = rng.permutation(n)[:ftc.N_STATES]
        big = np.tile(st[0], (n, 1))
        big[pos] = st
        _same(robot.shape_batch(big, want_R=True), out, pos, every, n)
    if fx["consts"][9]:                                  # retraction: the same 24 in another order
        perm = rng.permutation(ftc.N_STATES)
        _same(robot.shape_batch(st[perm], want_R=True), out, every, perm, "permuted")


@pytest.mark.parametrize("name", ftc.FIXTURES)
def test_tips_only_kernel_against_truth(irt, name):
    import torch
    fx, robot, out = _fk(irt, name)
    st, eng = fx["states"], robot.engine()
    rows, q = np.arange(ftc.N_STATES), ftc.tip_rows(fx)
    bound = ftc.bounds(fx)["p"]
    last = out["p"][rows, fx["n_points"] - 1]
    tips, conv = eng.fk_tips(st)
    d_tips = torch.zeros(3 * ftc.N_STATES, dtype=torch.float64, device="cuda")
    d_conv = torch.zeros(ftc.N_STATES, dtype=torch.uint8, device="cuda")
    eng.fk_tips_dev(torch.from_numpy(st).cuda(), ftc.N_STATES, d_tips, d_conv)
    torch.cuda.synchronize()
    for got, c in ((tips, conv), (d_tips.cpu().numpy().reshape(-1, 3), d_conv.cpu().numpy().astype(bool))):
        err = ftc.err_vs_truth(got, fx["p_hi"][rows, q], fx["p_lo"][rows, q]).max(axis=1)
        print("%s: tips max error / bound %.3f" % (name, (err / bound).max()))
        assert c.all() and (err <= bound).all(), np.flatnonzero(err > bound)
        assert np.array_equal(got, last)                 # what test_fk_tips_are_fk_batch_last_point claims


def _flags(irt, fx, vox, spheres, lo, hi, **env):
    robot = ftc.robot_from_fixture(irt, fx, min_length=lo, max_length=hi)
    cls = irt.VoxelValidityChecker if spheres else irt.VoxelBackboneValidityChecker
    with ftc.with_env(**env):
        chk = cls(robot, irt.VoxelEnvironment(), vox)
    fl = chk.is_valid_detail(fx["states"])["flags"]
    chk.engine.close()
    assert (fl & 1).all()
    return (fl & 2) != 0


def _grid(irt, n):
    vox = irt.VoxelOctree(n)
    vox.set_xlim(-0.3, 0.3); vox.set_ylim(-0.3, 0.3); vox.set_zlim(-0.3, 0.3)
    return vox


def _probe_limit(fx, dl, b, i, j, which, limit, passes, got, what):
    """One launch of a comparator probe: state i's own flag, and every other state's against what its truth says -- but a
    state (at most one, never the probed one) whose truth is within its own bound of the limit.  One-point backbones whose home
    length is 0 have no such allowance: their home - L_i is 0 - 0 (fk_truth_common.exact_zero)."""
    want = ~(dl[:, j] > limit) if which == "max" else ~(dl[:, j] < limit)
    want[i] = passes
    near = (np.abs(dl[:, j] - limit) <= b[:, j]) & ~ftc.exact_zero(fx)[:, j]
    near[i] = False
    assert near.sum() <= 1, (what, i, j, which, np.flatnonzero(near))
    bad = np.flatnonzero((got != want) & ~near)
    assert bad.size == 0, (what, "state %d tendon %d %s_length %s" % (i, j, which, "passes" if passes else "fails"), bad,
                           (dl[bad, j] - limit), b[bad, j])


@pytest.mark.parametrize("name,spheres", [("config2", False), ("config3", False), ("n1", False), ("n8", False), ("config2", True), ("n5", False),
                                          ("n6", False), ("n7", False), ("helix5", False), ("helix6", False), ("n5", True)])
def test_verdict_kernel_length_test_as_comparator(irt, name, spheres):
    """fk_verdict<3>, <4>, <1>, <8> and the sphere-checker form of <3>; fk_verdict<5> (the first width at one wave), <6>, <7>, the
    UniformHelix form of <5> and <6>, and the sphere-checker form of <5>.  Probes: the four states with the largest bound and the
    four with the smallest, each on its tendon with the largest |home - L_i|; per probe four robots that differ in one limit
    of that tendon (all other limits wide open), an empty voxel grid, all 24 states per launch.
    A state that passes the kernel's length test and then needs the exact self-collision sweep has its flags written again
    by the fallback pass from that pass's own stored-point integration, so a clear flag may come from either kernel; a set
    flag needs fk_verdict's own yes, and the two `set` robots of a probe bound fk_verdict's L_i from both sides."""
    fx = ftc.load(name)
    N = fx["C"].shape[0]
    home = ftc.robot_from_fixture(irt, fx).engine().home_lengths()
    dl, b = ftc.length_change(fx, home)                                          # what the truth says about home - L_i
    jj = np.abs(dl).argmax(axis=1)
    order = np.argsort(b[np.arange(ftc.N_STATES), jj], kind="stable")
    vox = irt.VoxelOctree(64)
    vox.set_xlim(-0.3, 0.3); vox.set_ylim(-0.3, 0.3); vox.set_zlim(-0.3, 0.3)
    wide = 1e3
    for i in list(order[:4]) + list(order[-4:]):
        j = jj[i]
        # (which limit, its value, does state i pass)
        for which, limit, passes in (("max", dl[i, j] + b[i, j], True), ("max", dl[i, j] - b[i, j], False),
                                     ("min", dl[i, j] - b[i, j], True), ("min", dl[i, j] + b[i, j], False)):
            lo, hi = np.full(N, -wide), np.full(N, wide)
            (hi if which == "max" else lo)[j] = limit
            got = _flags(irt, fx, vox, spheres, lo, hi)
            want = ~(dl[:, j] > limit) if which == "max" else ~(dl[:, j] < limit)
            want[i] = passes
            near = np.abs(dl[:, j] - limit) <= b[:, j]                           # its own truth is within its own bound of the limit
            near[i] = False
            assert near.sum() <= 1, (i, j, which, np.flatnonzero(near))
            bad = np.flatnonzero((got != want) & ~near)
            assert bad.size == 0, (name, "state %d tendon %d %s_length %s" % (i, j, which, "passes" if passes else "fails"), bad,
                                   (dl[bad, j] - limit), b[bad, j])


# ---- the fused stored-point kernels ------------------------------------------------------------------------------------------
NO_RETRACTION = [n for n in ftc.FIXTURES if n not in ftc.RETRACTION]
UNIFORM_HELIX = ("config1", "config2", "config2_dl35") + ftc.NEW_HELIX       # one pitch, one radius: routing_form.hpp picks UniformHelix


@pytest.mark.parametrize("name", NO_RETRACTION)
def test_fused_stored_point_kernels_against_truth(irt, name):
    """Which kernel an entry launches (launch_host.inc: launch_fk_sweep and launch_fused; tendon_hip.hip: validate_batch_dev_impl, tr_voxelize_batch),
    backbone checker, no retraction, empty 64^3 grid:
      TENDON_HIP_FUSED=1  is_valid_detail -> launch_fk_sweep -> launch_fused: fk_sweep_fused<N>, K1 + K2 over stored points in one
                          launch, tips from its own integration; voxelize_batch -> the same kernel with voxel_test = 0 (then
                          the block-list kernels, which do not touch the tips);
      TENDON_HIP_FUSED=0  is_valid_detail -> launch_fk (fk_rk4_batch_uniform<N>) + launch_sweep (the K2 sweep) as separate
                          launches; voxelize_batch likewise;
      TENDON_HIP_FUSED=2  is_valid_detail -> launch_verdict: fk_verdict<N>, then fk_sweep_fused_list<N> over the pending states
                          (test_verdict_kernels_tips_against_truth has its tips).
    (i) FUSED=1 and (ii) FUSED=0: both entries' tips within the point bound of the truth's last point, every state converged;
    robots that are uniform helices run (i) in the helix and in the table form.  (iii) verdicts and flags of FUSED = 0, 1, 2 equal
    on the 24 states."""
    fx = ftc.load(name)
    rows, q = np.arange(ftc.N_STATES), ftc.tip_rows(fx)
    bound = ftc.bounds(fx)["p"]
    det = {}
    for fuse, form in [(1, "helix"), (1, "table"), (0, "helix"), (2, "helix")]:
        if form == "table" and name not in UNIFORM_HELIX:
            continue
        env = dict(TENDON_HIP_FUSED=fuse, **({"TENDON_HIP_ROUTING": "table"} if form == "table" else {}))
        with ftc.with_env(**env):
            chk = irt.VoxelBackboneValidityChecker(ftc.robot_from_fixture(irt, fx), irt.VoxelEnvironment(), _grid(irt, 64))
        d = det[fuse, form] = chk.is_valid_detail(fx["states"])
        vox = chk.engine.voxelize_batch(fx["states"]) if fuse < 2 else None
        chk.engine.close()
        assert (d["flags"] & 1).all()
        if fuse == 2:
            continue
        assert np.array_equal(vox["shape_valid"], np.asarray(d["valid"], bool))      # an empty grid: the shape test is the verdict
        for what, tips in (("is_valid_detail", d["tips"]), ("voxelize_batch", vox["tips"])):
            err = ftc.err_vs_truth(tips, fx["p_hi"][rows, q], fx["p_lo"][rows, q]).max(axis=1)
            print("%s: FUSED=%d%s %s tips, max error / bound %.3f" % (name, fuse, " (table form)" if form == "table" else "", what,
                                                                       (err / bound).max()))
            assert (err <= bound).all(), (fuse, form, what, np.flatnonzero(err > bound), (err / bound).max())
    for key in ((0, "helix"), (2, "helix")):
        assert np.array_equal(det[key]["flags"], det[1, "helix"]["flags"]), key
        assert np.array_equal(det[key]["valid"], det[1, "helix"]["valid"]), key


@pytest.mark.parametrize("name", ["n5", "n6", "helix5", "helix6"])
def test_fallback_pass_on_curled_states(irt, orc, helpers, name):
    """fk_sweep_fused_list<5>, <6> in both routing forms: 64 tightly curled states (fk_truth_common.curled_states) through
    fk_verdict and, for every state whose milestones do not settle the self-collision test, the fallback pass, whose workspace
    TENDON_HIP_FB_CAP=64 makes exactly one wave wide.  Flags and verdicts equal the oracle's tests (collides_self,
    is_within_length_limits) on the device's own stored points.  No fallback counter leaves the library; but fk_verdict never
    clears the self-collision bit of a converged state within its limits itself (verdict_kernel.hpp: verdict_decide sets it where the
    milestones resolve, and hands every other state over), so a state with bits 1 and 2 set and bit 4 clear was decided by the
    fallback pass: at least 8 of them (tests/test_fk_truth.py counts them with the oracle alone)."""
    fx = ftc.load(name)
    st = ftc.curled_states(fx)
    robot = ftc.curled_robot(irt, fx)
    with ftc.with_env(TENDON_HIP_FB_CAP=64):
        chk = irt.VoxelBackboneValidityChecker(robot, irt.VoxelEnvironment(), _grid(irt, 128))
    got = chk.is_valid_detail(st)
    fk = chk.engine.fk_batch(st)
    home = chk.engine.home_lengths()
    chk.engine.close()
    orb = helpers.oracle_robot(orc, robot)
    conv = fk["converged"].astype(bool)
    within = np.array([bool(conv[i]) and orb.is_within_length_limits(home, fk["L_i"][i]) for i in range(len(st))])
    hits = np.array([bool(conv[i]) and orb.collides_self(fk["p"][i]) for i in range(len(st))])
    want = conv.astype(np.uint8) | ((conv & within).astype(np.uint8) << 1) | ((conv & within & ~hits).astype(np.uint8) << 2)
    fallback = ((got["flags"] & 7) == 3) & ((got["flags"] & 16) == 0)
    print("%s: %d converged, %d decided as self-colliding by the fallback pass, %d free" % (name, conv.sum(), fallback.sum(), ((got["flags"] & 4) != 0).sum()))
    assert np.array_equal(got["flags"] & 7, want), np.flatnonzero((got["flags"] & 7) != want)
    assert not (got["flags"] & 16).any()                                 # every point inside the grid: nothing else decides
    assert np.array_equal(np.asarray(got["valid"], bool), conv & within & ~hits)
    assert fallback.sum() >= 8 and ((got["flags"] & 4) != 0).sum() >= 8


# ---- retraction: the stored-point kernel with its home lengths, the verdict form, the verdict kernels' tips ---------------------
def _retraction_dev(irt, fx, states, ld, **env):
    """tr_fk_batch_retraction_dev on a context of its own: dict(p (n, P, 3) with every state's points moved from their tip-aligned
    rows to rows 0 .. n_points - 1 (NaN beyond), unwritten (n,) whether every row before a state's first point was left alone,
    L, L_i, home (n, N), converged, n_points)."""
    import torch
    with ftc.with_env(**env):
        eng = irt.engine.Engine(ftc.robot_from_fixture(irt, fx))
    n, P, N = len(states), eng.num_points, eng.n_tendons
    f64 = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device="cuda")
    px, py, pz, Li, home, Lb = f64(P * ld), f64(P * ld), f64(P * ld), f64(N * ld), f64(N * ld), f64(n)
    conv = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    npts = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    eng.fk_batch_retraction_dev(torch.from_numpy(np.ascontiguousarray(states)).cuda(), n, ld, px, py, pz, Li, conv, npts, home, d_L=Lb)
    torch.cuda.synchronize()
    planes = np.stack([a.cpu().numpy().reshape(P, ld)[:, :n] for a in (px, py, pz)], axis=2)         # (P, n, 3), rows aligned at the tip
    npt = npts.cpu().numpy()
    eng.close()
    assert ((npt >= 1) & (npt <= P)).all()
    p = np.full((n, P, 3), np.nan)
    unwritten = np.ones(n, bool)
    for i in range(n):
        p[i, :npt[i]] = planes[P - npt[i]:, i]
        unwritten[i] = np.isnan(planes[:P - npt[i], i]).all()
    return dict(p=p, unwritten=unwritten, L=Lb.cpu().numpy(), L_i=Li.cpu().numpy().reshape(N, ld)[:, :n].T.copy(),
                home=home.cpu().numpy().reshape(N, ld)[:, :n].T.copy(), converged=conv.cpu().numpy(), n_points=npt)


_DEV_KEYS = ("p", "L", "L_i", "home", "converged", "n_points", "unwritten")


@pytest.mark.parametrize("name", ftc.RETRACTION)
def test_retraction_kernel_and_its_home_lengths_against_truth(irt, name):
    """fk_rk4_batch_retract through tr_fk_batch_retraction_dev: every stored point (the lane's point j is in row j + P - n_points),
    L, every L_i and every home length within its bound; point counts and `converged` the fixture's; nothing written before a
    lane's first row; bit for bit the same in the order of the backbone lengths (TENDON_HIP_RETRACT_SORT=1: from one
    configuration on, with the per-wave start of the tip-aligned loop) and scattered over 65 and 130 columns."""
    fx = ftc.load(name)
    st = fx["states"]
    out = _retraction_dev(irt, fx, st, 64, TENDON_HIP_RETRACT_SORT=0)
    assert (out["converged"] == 1).all() and np.array_equal(out["n_points"], fx["n_points"]) and out["unwritten"].all()
    b = ftc.bounds(fx)
    ep = np.where(fx["pt_idx"][:, :, None] >= 0, ftc.err_vs_truth(ftc.stored_points(fx, out["p"]), fx["p_hi"], fx["p_lo"]), 0.0)
    assert not np.isnan(ep).any()
    e = dict(p=ep.max(axis=(1, 2)), L=ftc.err_vs_truth(out["L"], fx["L_hi"], fx["L_lo"]), L_i=ftc.err_vs_truth(out["L_i"], fx["Li_hi"], fx["Li_lo"]),
             home=ftc.err_vs_truth(out["home"], fx["home_hi"], fx["home_lo"]))
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = {k: np.where(e[k] == 0, 0.0, e[k] / b[k]) for k in e}
    print("%s: error / bound of fk_rk4_batch_retract: points %.3f, L %.3f, L_i %.3f, home %.3f; home error %.2g .. %.2g, bound %.2g .. %.2g"
          % (name, ratio["p"].max(), ratio["L"].max(), ratio["L_i"].max(), ratio["home"].max(), e["home"].min(), e["home"].max(),
             b["home"].min(), b["home"].max()))
    for k in e:
        assert (e[k] <= b[k]).all(), (k, np.argwhere(e[k] > b[k]), ratio[k].max())
    every = np.arange(ftc.N_STATES)
    _same(_retraction_dev(irt, fx, st, 64, TENDON_HIP_RETRACT_SORT=1), out, every, every, "length order", _DEV_KEYS)
    rng = np.random.default_rng(6)
    for n, sort in ((65, 0), (130, 1)):
        pos = rng.permutation(n)[:ftc.N_STATES]
        big = np.tile(st[0], (n, 1))
        big[pos] = st
        _same(_retraction_dev(irt, fx, big, 192, TENDON_HIP_RETRACT_SORT=sort), out, pos, every, (n, sort), _DEV_KEYS)
    if name in ftc.NEW_RETRACTION:
        # the sixteenth special value, a negative s_start: no truth, reported unconverged with a one-point backbone
        neg = st[:3].copy()
        neg[1, -1] = ftc.special_s_start(fx["consts"][0], fx["consts"][1])[15]
        for sort in (0, 1):
            got = _retraction_dev(irt, fx, neg, 64, TENDON_HIP_RETRACT_SORT=sort)
            assert got["converged"].tolist() == [1, 0, 1] and got["n_points"][1] == 1
            _same(got, out, [0, 2], [0, 2], "beside a negative s_start", _DEV_KEYS)


@pytest.mark.parametrize("spheres", [False, True])
@pytest.mark.parametrize("name", ftc.RETRACTION)
def test_retraction_verdict_kernel_length_test_as_comparator(irt, name, spheres):
    """fk_verdict_retract: fk_retract_prologue -> hand-over planes -> the tip-aligned launch, whose state (tensions, angle, s_start,
    L_i, point 1 and its frame) comes from the planes and whose home lengths are its own quadrature.  The comparator of
    test_verdict_kernel_length_test_as_comparator with the length change home - L_i per state from the two truths and
    b = bound(L_i) + bound(home) + 2 ulp(home) (fk_truth_common.length_change; one- and two-point backbones: the floor).  Probes:
    the four states with the largest b, the four with the smallest, one state of every first-interval class; both checkers; in
    arrival order and in the order of the backbone lengths; through a 64-column fallback workspace."""
    fx = ftc.load(name)
    N = fx["C"].shape[0]
    dl, b = ftc.length_change(fx)
    jj = np.abs(dl).argmax(axis=1)
    order = np.argsort(b[np.arange(ftc.N_STATES), jj], kind="stable")
    cls = ftc.first_interval_class(fx)
    probes = list(order[:4]) + list(order[-4:])
    probes += [int(np.flatnonzero(cls == c)[-1]) for c in range(5) if (cls == c).any() and not (cls[probes] == c).any()]
    assert set(cls[probes]) == set(cls) and (name != "config3_ret_edges" or len(set(cls)) == 5)
    vox = _grid(irt, 64)
    wide = 1e3
    for sort in (0, 1):
        for i in probes:
            j = jj[i]
            for which, limit, passes in (("max", dl[i, j] + b[i, j], True), ("max", dl[i, j] - b[i, j], False),
                                         ("min", dl[i, j] - b[i, j], True), ("min", dl[i, j] + b[i, j], False)):
                lo, hi = np.full(N, -wide), np.full(N, wide)
                (hi if which == "max" else lo)[j] = limit
                got = _flags(irt, fx, vox, spheres, lo, hi, TENDON_HIP_RETRACT_SORT=sort, TENDON_HIP_FB_CAP=64)
                _probe_limit(fx, dl, b, i, j, which, limit, passes, got, (name, spheres, sort))


@pytest.mark.parametrize("name", ftc.FIXTURES)
def test_verdict_kernels_tips_against_truth(irt, name):
    """The tips fk_verdict<1 .. 8> (both routing forms' instantiations at 2, 5, 6) and fk_verdict_retract report (is_valid_detail: no stored point behind them) lie within the
    point bound of the truth's last point, for every state the kernel reports converged -- all of them."""
    fx = ftc.load(name)
    rows, q = np.arange(ftc.N_STATES), ftc.tip_rows(fx)
    bound = ftc.bounds(fx)["p"]
    for sort in ((0, 1) if fx["consts"][9] else (0,)):
        with ftc.with_env(TENDON_HIP_RETRACT_SORT=sort):
            chk = irt.VoxelBackboneValidityChecker(ftc.robot_from_fixture(irt, fx), irt.VoxelEnvironment(), _grid(irt, 64))
        det = chk.is_valid_detail(fx["states"])
        chk.engine.close()
        err = ftc.err_vs_truth(det["tips"], fx["p_hi"][rows, q], fx["p_lo"][rows, q]).max(axis=1)
        with np.errstate(invalid="ignore", divide="ignore"):
            print("%s: verdict kernel tips, max error / bound %.3f" % (name, np.where(err == 0, 0.0, err / bound).max()))
        assert (det["flags"] & 1).all() and (err <= bound).all(), np.flatnonzero(err > bound)


# ---- fk_edge_queue ---------------------------------------------------------------------------------------------------------
def _signature_rows(vox, pts, width):
    """The vertices' signature rows from stored points, as test_signature_rows_equal_the_cells_of_the_stored_points lays the
    words out (collision/VoxelOctree.cpp:309-317: closed domain check, truncated quotient); zero beyond the P points."""
    M, P = pts.shape[:2]
    inside = np.ones((M, P), dtype=bool)
    word = np.zeros((M, P), dtype=np.int64)
    for a, ((lo, hi), d) in enumerate(zip((vox.xlim(), vox.ylim(), vox.zlim()), (vox.dx(), vox.dy(), vox.dz()))):
        x = pts[:, :, a]
        inside &= ~((x < lo) | (hi < x)) & (np.abs(x) < 1e300)
        word |= (((x - lo) / d).astype(np.int64) & 1023) << (10 * a)
    word[~inside] = 1 << 30
    out = np.zeros((M, width), dtype=np.uint32)
    out[:, :P] = word
    return out.view(np.int32)


@pytest.mark.parametrize("name", ["config3_rot", "n1", "n8", "config2", "n5", "n6", "helix5", "helix6"])
def test_edge_queue_length_test_as_comparator(irt, name):
    """fk_edge_queue integrates every interior sample of an edge and nothing else does when the vertices come with their signature
    rows (tr_validate_edges_indexed_sig_dev takes every vertex as valid).  Edge i turns state i about the z axis, from theta - 0.125
    to theta + 0.125: every sample has state i's tensions, so state i's L_i, whatever its angle, and the truth of L_i does not
    depend on the angle.  An edge nothing subdivides (n_fk == 2: a straight backbone does not move) is valid whatever the limit;
    an edge with interior samples is valid exactly when its state's truth passes the limit.  Probes as in
    test_verdict_kernel_length_test_as_comparator, among the states whose edge has interior samples.  Empty 256^3 grid on
    +- 0.3 m; 128^3 for n1, n8, n5, n6, helix5 and helix6, whose dL = 4 mm the backbone checker refuses on 2.3 mm voxels (VoxelBackboneValidityChecker.h:
    37-45) while the sphere checker, which has no such check, hands no signature rows over.  config2: the fixture's states with
    rotation switched on."""
    import torch
    fx = ftc.load(name)
    N, n = fx["C"].shape[0], ftc.N_STATES
    theta = fx["states"][:, N] if fx["consts"][8] else np.random.default_rng(12).uniform(-np.pi, np.pi, n)
    verts = np.vstack([np.column_stack([fx["states"][:, :N], theta - 0.125]), np.column_stack([fx["states"][:, :N], theta + 0.125])])
    edges = np.ascontiguousarray(np.stack([np.arange(n), n + np.arange(n)], 1), dtype=np.int32)
    base = ftc.robot_from_fixture(irt, fx, enable_rotation=True)
    home = base.engine().home_lengths()
    dl, b = ftc.length_change(fx, home)
    vox = _grid(irt, 256 if fx["consts"][1] <= 0.6 / 256 else 128)
    d_states, d_edges = torch.from_numpy(verts).cuda(), torch.from_numpy(edges).cuda()
    pts = base.shape_batch(verts)["p"]

    def run(lo, hi):
        robot = ftc.robot_from_fixture(irt, fx, enable_rotation=True, min_length=lo, max_length=hi)
        eng = irt.VoxelBackboneValidityChecker(robot, irt.VoxelEnvironment(), vox).engine
        d_sig = torch.from_numpy(_signature_rows(vox, pts, eng.signature_words())).cuda()
        d_bits = torch.zeros(1, dtype=torch.int64, device="cuda")
        d_nfk = torch.zeros(n, dtype=torch.int32, device="cuda")
        nd = eng.validate_edges_indexed_dev(d_states, 2 * n, d_edges, n, d_bits, d_nfk, d_vertex_sig=d_sig)
        valid, nfk, sch = irt.unpack_bits(d_bits.cpu().numpy().view(np.uint64), n), d_nfk.cpu().numpy(), eng.edge_schedule_last()
        eng.close()
        assert nd == 0 and sch["flags"] == 0 and sch["samples"] == int(nfk.sum()) - 2 * n and sch["samples"] > 0, sch   # the queue took the call
        return valid, nfk

    wide = 1e3
    valid, nfk = run(np.full(N, -wide), np.full(N, wide))
    assert valid.all()
    split = nfk >= 3
    assert (nfk[~split] == 2).all() and split.sum() >= 8
    print("%s: %d edges with interior samples (%d samples), %d that nothing subdivides" % (name, split.sum(), nfk.sum() - 2 * n, (~split).sum()))
    jj = np.abs(dl).argmax(axis=1)
    among = np.flatnonzero(split)
    order = among[np.argsort(b[among, jj[among]], kind="stable")]
    for i in list(order[:4]) + list(order[-4:]):
        j = jj[i]
        assert nfk[i] >= 3
        for which, limit, passes in (("max", dl[i, j] + b[i, j], True), ("max", dl[i, j] - b[i, j], False),
                                     ("min", dl[i, j] - b[i, j], True), ("min", dl[i, j] + b[i, j], False)):
            lo, hi = np.full(N, -wide), np.full(N, wide)
            (hi if which == "max" else lo)[j] = limit
            got, nfk_now = run(lo, hi)
            assert nfk_now[i] >= 3 and np.array_equal(nfk_now >= 3, split)
            want = ~(dl[:, j] > limit) if which == "max" else ~(dl[:, j] < limit)
            want[i] = passes
            want[~split] = True
            near = (np.abs(dl[:, j] - limit) <= b[:, j]) & split
            near[i] = False
            assert near.sum() <= 1, (i, j, which, np.flatnonzero(near))
            bad = np.flatnonzero((got != want) & ~near)
            assert bad.size == 0, (name, "state %d tendon %d %s_length %s" % (i, j, which, "passes" if passes else "fails"), bad,
                                   (dl[bad, j] - limit), b[bad, j])
