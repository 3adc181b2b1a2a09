"""CPU side of the extended-precision truth of the LOADED rod integration (tests/golden/loaded_fk_truth_<name>.npz,
tests/golden/make_loaded_fk_truth.py): the fixtures still describe the numpy reference and the loaded-FK fixtures they start from,
the generator still reproduces them, and the bounds of tests/test_gpu_loaded_fk_truth.py see what the 1e-9 m of
tests/test_gpu_loaded_fk.py lets through -- a distributed force or moment that is off by a factor, load terms taken with the frame
of the step's first stage, and load terms taken with R in the place of R^T.  No kernel, no GPU."""
import importlib.util
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

NAMES = ("config1", "n1", "n8", "config3_rot", "n5", "n6")
SHOOT_TOL = 1e-11                                                     # loaded_fk_reference.shoot's: what make_loaded_fk.py converged to


@pytest.fixture(scope="module")
def world(orc):
    """name -> (truth fixture, loaded-FK fixture, oracle robot)"""
    import make_loaded_fk as mlf
    cache = {}

    def get(name):
        if name not in cache:
            _, rob, st = mlf.fixture(name)
            fx = ftc.load_loaded(name)
            assert np.array_equal(st, fx["states"])
            cache[name] = (fx, dict(np.load(mlf.path(name))), rob)
        return cache[name]
    return get


def _evaluate(rob, fx, case, f_scale=1.0, l_scale=1.0):
    """loaded_fk_reference.evaluate from the fixture's vu0 and loads, the distributed rows scaled."""
    w, d = fx["wrench_" + case], fx["dist_" + case]
    return ref.evaluate(rob, fx["states"], fx["vu0_" + case], F_e=w[:, :3], L_e=w[:, 3:], f_e=d[:, :3] * f_scale, l_e=d[:, 3:] * l_scale)


def _errors(fx, case, out):
    Rtip = np.swapaxes(out["R"][:, -1], 1, 2).reshape(ftc.N_STATES, 9)              # column-major
    return ftc.loaded_errors(fx, case, out["p"], Rtip, out["L"], out["L_i"], out["vuL"], out["e"])


def _outside(fx, case, out):
    """(24,) bool: the result's points leave the point bound"""
    return _errors(fx, case, out)["p"] > ftc.loaded_bounds(fx, case)["p"]


@pytest.mark.parametrize("case", ftc.LOADED_CASES)
@pytest.mark.parametrize("name", NAMES)
def test_reference_error_is_the_recorded_e_ref(world, name, case):
    """A change to the reference's arithmetic shows here: its distance from the truth is the stored E_ref, bit for bit, for every
    output.  The loads and start strains are those of loaded_fk_<name>.npz, and from them the reference still meets its own
    stopping test -- the shooting would return them with zero iterations."""
    fx, lf, rob = world(name)
    assert os.path.getsize(ftc.loaded_path(name)) <= 393 * 1024
    for k in ("wrench", "dist", "vu0"):
        assert np.array_equal(fx["%s_%s" % (k, case)], lf["%s_%s" % (k, case)]), k
    out = _evaluate(rob, fx, case)
    e = _errors(fx, case, out)
    for k, key in (("p", "p"), ("R", "R"), ("L", "L"), ("L_i", "Li"), ("vu", "vu"), ("e", "e")):
        assert np.array_equal(e[k], fx["Eref_%s_%s" % (key, case)]), (name, case, k)
    en = np.linalg.norm(out["e"], axis=1)
    assert (en <= SHOOT_TOL).all() and np.array_equal(en, lf["e_ref_" + case])
    assert (np.abs(en - ftc.loaded_e_norm(fx, case)) <= 0.25 * ftc.loaded_bounds(fx, case)["enorm"] * (1 + 1e-12)).all()
    ratios = ftc.loaded_ratios(fx, case, e)
    assert all((v <= 0.25 + 1e-12).all() for v in ratios.values())                      # every bound is at least 4 E_ref
    d = fx["dist_" + case]
    if case == "D":                                                                     # all twelve numbers, and a moment to see
        assert (fx["wrench_D"] != 0).all() and (d != 0).all() and (np.linalg.norm(d[:, 3:], axis=1) >= 0.003).all()
    else:
        assert not d[:, 2].any() and not d[:, 3:].any()


def test_the_zero_load_fixtures_cover_every_width():
    """test_zero_load_against_the_unloaded_truth (tests/test_gpu_loaded_fk_truth.py) runs fk_loaded_uniform<N> for N = 1 .. 8."""
    names = [n for n in ftc.FIXTURES if n not in ftc.RETRACTION]
    assert len(names) == 14 and {ftc.load(n)["C"].shape[0] for n in names} == set(range(1, 9))


@pytest.mark.parametrize("name", NAMES)
def test_generator_reproduces_the_stored_truth(name):
    """One state of case D and one of case A per fixture through the mpmath model again: the stored hi + lo to 1e-30."""
    mp = pytest.importorskip("mpmath")
    spec = importlib.util.spec_from_file_location("make_loaded_fk_truth", os.path.join(ftc.GOLD, "make_loaded_fk_truth.py"))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    fx = ftc.load_loaded(name)
    steps = [(float(t), float(h), int(r)) for (t, h), r in zip(fx["steps"], fx["step_row"])]
    idx = [int(q) for q in fx["pt_idx"]]
    for case, i in (("D", 5), ("A", 14)):
        vu0, w, d = fx["vu0_" + case][i], fx["wrench_" + case][i], fx["dist_" + case][i]
        m = g.mft.model(fx["consts"], fx["C"], fx["D"], fx["states"][i], vu0[:3], vu0[3:], steps, f_e=d[:3], l_e=d[3:], wrench=w)
        for key, vals in g.outputs(m, idx).items():
            hi, lo = (np.asarray(fx["%s_%s_%s" % (key, part, case)][i]).reshape(-1) for part in ("hi", "lo"))
            assert len(vals) == len(hi)
            for x, h, l in zip(vals, hi, lo):
                assert abs(x - (mp.mpf(float(h)) + mp.mpf(float(l)))) <= abs(x) * mp.mpf(2) ** -76 + mp.mpf("1e-30"), (case, key)
        assert np.array_equal(np.array([float(x) for x in m["e_terms"]]), fx["e_terms_" + case][i])


# ---- the bounds have teeth ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,case,f_scale,l_scale", [("config1", "C", 1 + 1e-8, 1.0), ("n8", "C", 1 + 1e-8, 1.0),
                                                       ("config1", "D", 1.0, 1 + 1e-5), ("config3_rot", "D", 1.0, 1 + 1e-5)])
def test_bounds_see_a_scaled_distributed_load(world, name, case, f_scale, l_scale):
    """f_e (1 + 1e-8), an order below the factor that moved every state by 3.9e-10 m or more and that the 1e-9 m check lets pass,
    and l_e (1 + 1e-5) on case D, whose weakest moment (0.003 N) then moves a state by more than 1e-11 m: at least 20 of the 24
    states leave the point bound, and the reference itself leaves it on none.  Measured when the fixtures were written: 24, 24, 24
    and 24 of 24 (CHANGELOG, round 20)."""
    fx, _, rob = world(name)
    plain, bent = _evaluate(rob, fx, case), _evaluate(rob, fx, case, f_scale, l_scale)
    shift = np.abs(bent["p"] - plain["p"]).max(axis=(1, 2))
    out = _outside(fx, case, bent)
    print("%s %s, f_e x %.9g, l_e x %.6g: %d of 24 states outside the point bound; point shift %.2g .. %.2g m, bound %.2g .. %.2g m"
          % (name, case, f_scale, l_scale, out.sum(), shift.min(), shift.max(), ftc.loaded_bounds(fx, case)["p"].min(),
             ftc.loaded_bounds(fx, case)["p"].max()))
    assert not _outside(fx, case, plain).any()
    assert out.sum() >= 20
    if l_scale == 1.0:
        assert shift.max() <= 1e-10                                                     # ... an order under the interface tolerance


def _with_load_frame(monkeypatch, mode):
    """loaded_fk_reference.rhs with its two load terms taken through another matrix than R^T: `frozen`, the transpose of the frame
    the step's FIRST stage had (integrate() calls rhs four times a step, in stage order), or `transposed`, R itself.  The
    wrapper hands rhs the vectors f', l' with R^T f' = M f, so nothing else of the right-hand side changes."""
    plain, calls, first = ref.rhs, [0], [None]

    def rhs(Kse, Kbt, route, tau, R, v, u, f_e, l_e):
        if calls[0] % 4 == 0:
            first[0] = R
        calls[0] += 1
        M = np.swapaxes(first[0], -1, -2) if mode == "frozen" else R
        through = lambda x: np.linalg.solve(np.swapaxes(R, -1, -2), (M @ x[..., None]))[..., 0]
        return plain(Kse, Kbt, route, tau, R, v, u, through(f_e), through(l_e))
    monkeypatch.setattr(ref, "rhs", rhs)


@pytest.mark.parametrize("mode", ["frozen", "transposed"])
def test_bounds_see_a_wrong_frame_in_the_load_terms(world, monkeypatch, mode):
    """config1, case D: both load terms with the frame of the step's first stage in all four stages, and with R in the place of
    R^T.  Either leaves the point bound on all 24 states."""
    fx, _, rob = world("config1")
    plain = _evaluate(rob, fx, "D")
    _with_load_frame(monkeypatch, mode)
    bent = _evaluate(rob, fx, "D")
    shift = np.abs(bent["p"] - plain["p"]).max(axis=(1, 2))
    out = _outside(fx, "D", bent)
    print("config1 D, %s frame in the load terms: %d of 24 states outside the point bound; point shift %.2g .. %.2g m" % (mode, out.sum(), shift.min(), shift.max()))
    assert out.all()
