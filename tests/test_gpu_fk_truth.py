"""The integrator of the FK kernels against an extended-precision evaluation of the scheme they restate.

The fixtures tests/golden/fk_truth_*.npz (tests/golden/make_fk_truth.py) hold, for 24 states of eight small robots, the
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
      short of it must reject it.

Still unobserved after this module: fk_verdict_retract (its home length is a quadrature of its own) and fk_edge_queue."""
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


def _same(a, b, rows_a, rows_b, what):
    for k in ("p", "R", "L", "L_i", "converged", "n_points"):
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


def _flags(irt, fx, vox, spheres, lo, hi):
    robot = ftc.robot_from_fixture(irt, fx, min_length=lo, max_length=hi)
    cls = irt.VoxelValidityChecker if spheres else irt.VoxelBackboneValidityChecker
    chk = cls(robot, irt.VoxelEnvironment(), vox)
    fl = chk.is_valid_detail(fx["states"])["flags"]
    chk.engine.close()
    assert (fl & 1).all()
    return (fl & 2) != 0


@pytest.mark.parametrize("name,spheres", [("config2", False), ("config3", False), ("n1", False), ("n8", False), ("config2", True)])
def test_verdict_kernel_length_test_as_comparator(irt, name, spheres):
    """fk_verdict<3>, <4>, <1>, <8> and the sphere-checker form of <3>.  Probes: the four states with the largest bound and the
    four with the smallest, each on its tendon with the largest |home - L_i|; per probe four robots that differ in one limit
    of that tendon (all other limits wide open), an empty voxel grid, all 24 states per launch.
    A state that passes the kernel's length test and then needs the exact self-collision sweep has its flags written again
    by the fallback pass from that pass's own stored-point integration, so a clear flag may come from either kernel; a set
    flag needs fk_verdict's own yes, and the two `set` robots of a probe bound fk_verdict's L_i from both sides."""
    fx = ftc.load(name)
    N = fx["C"].shape[0]
    home = ftc.robot_from_fixture(irt, fx).engine().home_lengths()
    b = ftc.bounds(fx)["L_i"] + 2 * np.spacing(home)[None, :]
    dl = (home[None, :] - fx["Li_hi"]) - fx["Li_lo"].astype(np.float64)          # what the truth says about home - L_i
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
