"""CPU side of the extended-precision FK truth (tests/golden/fk_truth_*.npz, tests/golden/make_fk_truth.py): the fixtures
still describe this oracle, the generator still reproduces them, the mpmath model agrees with an integrator and a
right-hand side that share nothing with it, and the bounds of tests/test_gpu_fk_truth.py see an error that the 1e-9 m
parity bar lets through."""
import importlib.util
import os

import numpy as np
import pytest

import fk_truth_common as ftc

GEN = os.path.join(ftc.GOLD, "make_fk_truth.py")


def _generator():
    """tests/golden/make_fk_truth.py by file path (mpmath comes with torch's sympy)."""
    spec = importlib.util.spec_from_file_location("make_fk_truth", GEN)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _oracle_robot(orc, fx):
    L, dL, ro, ri, E, nu, r, res, rot, ret = (float(x) for x in fx["consts"])
    return orc.Robot(fx["C"].tolist(), fx["D"].tolist(), r=r, L=L, dL=dL, ro=ro, ri=ri, E=E, nu=nu, max_tension=fx["max_tension"].tolist(),
                     enable_rotation=bool(rot), enable_retraction=bool(ret), residual_threshold=res)


def _oracle_result(orc, fx):
    """The oracle's shapes of the fixture's states in the form fk_truth_common.compare takes: p (24, P, 3) NaN-padded,
    R at the tip (24, 9), L (24,), L_i (24, N)."""
    orb = _oracle_robot(orc, fx)
    shapes = [orb.shape(s) for s in fx["states"]]
    p = np.full((ftc.N_STATES, int(fx["n_points"].max()), 3), np.nan)
    for i, s in enumerate(shapes):
        p[i, :len(s["p"])] = s["p"]
    return shapes, (p, np.array([s["R"][-1] for s in shapes]), np.array([s["L"] for s in shapes]), np.array([s["L_i"] for s in shapes]))


@pytest.mark.parametrize("name", ftc.FIXTURES)
def test_oracle_error_is_the_recorded_e_ref(orc, name):
    """A change to the oracle's arithmetic shows here: its distance from the truth is E_ref to the last bit (allowed: 1 ulp),
    its start values and step sequence are the ones the truth was integrated with, and every state converges."""
    fx = ftc.load(name)
    assert fx["states"].shape[0] == ftc.N_STATES and os.path.getsize(ftc.path(name)) < 250 * 1024
    shapes, res = _oracle_result(orc, fx)
    e = ftc.errors(fx, *res)
    for k, key in (("p", "Eref_p"), ("R", "Eref_R"), ("L", "Eref_L"), ("L_i", "Eref_Li")):
        assert (np.abs(e[k] - fx[key]) <= np.spacing(fx[key])).all(), (name, k)
    for i, s in enumerate(shapes):
        assert s["converged"] and len(s["t"]) == fx["n_points"][i]
        assert np.array_equal(s["v_i"], fx["v0"][i]) and np.array_equal(s["u_i"], fx["u0"][i])
        k = fx["n_steps"][i]
        assert np.isnan(fx["steps"][i, k:]).all() and not np.isnan(fx["steps"][i, :k]).any()
        ends = fx["step_row"][i, :k]
        assert np.array_equal(ends[ends >= 0], np.arange(1, len(s["t"])))             # every interval ends in the next point
        assert np.array_equal(fx["steps"][i, :k, 0][np.r_[True, ends[:-1] >= 0]], s["t"][:-1])   # and restarts at exactly t[j]
    if name == "config2_dl35":
        assert (fx["step_row"][:, 0] == -1).all() and fx["n_steps"][0] == fx["n_points"][0]      # two steps in the first interval
    ratio, ok = ftc.compare(fx, *res)
    assert ok.all() and ratio <= 0.25 + 1e-12                                           # the bound is at least 4 E_ref


@pytest.mark.parametrize("name", ftc.FIXTURES)
def test_generator_reproduces_the_stored_truth(name):
    """Two states per fixture through the mpmath model again: the stored hi + lo to 1e-30."""
    mp = pytest.importorskip("mpmath")
    g = _generator()
    fx = ftc.load(name)
    for i in (5, 14):
        k = int(fx["n_steps"][i])
        steps = [(float(t), float(h), int(r)) for (t, h), r in zip(fx["steps"][i, :k], fx["step_row"][i, :k])]
        m = g.model(fx["consts"], fx["C"], fx["D"], fx["states"][i], fx["v0"][i], fx["u0"][i], steps)
        idx = fx["pt_idx"][i][fx["pt_idx"][i] >= 0]
        got = [m["p"][q][c] for q in idx for c in range(3)] + list(m["R"]) + [m["L"]] + list(m["Li"])
        hi = np.concatenate([fx["p_hi"][i, :len(idx)].reshape(-1), fx["R_hi"][i], [fx["L_hi"][i]], fx["Li_hi"][i]])
        lo = np.concatenate([fx["p_lo"][i, :len(idx)].reshape(-1), fx["R_lo"][i], [fx["L_lo"][i]], fx["Li_lo"][i]])
        assert len(got) == len(hi)
        for x, h, l in zip(got, hi, lo):
            xh, xl = g.split(x)
            assert abs((mp.mpf(float(h)) + mp.mpf(float(l))) - (mp.mpf(xh) + mp.mpf(float(xl)))) <= mp.mpf("1e-30")
            assert abs(x - (mp.mpf(float(h)) + mp.mpf(float(l)))) <= abs(x) * mp.mpf(2) ** -76 + mp.mpf("1e-60")   # hi + lo holds the truth


def test_model_against_high_order_integrator(orc):
    """DOP853 (rtol 1e-13) on the numpy right-hand side of tests/test_oracle.py -- another integrator, another linear
    solver, fp64 -- against the mpmath RK4 tip: the difference is RK4's truncation error, 4th order in dL."""
    from scipy.integrate import solve_ivp
    from test_oracle import HELIX_C, HELIX_D, helix_robot, np_deriv
    g = _generator()
    tau = np.array([9.0, 1.5, 4.0])
    errs = []
    for dL in (0.01, 0.005, 0.0025):
        rb = helix_robot(orc, dL=dL)
        s = rb.shape(tau)
        consts = np.array([0.2, dL, 0.01, 0.0, 2.1e6, 0.3, 0.015, 5e-6, 0.0, 0.0])
        m = g.model(consts, np.array(HELIX_C), np.array(HELIX_D), tau, s["v_i"], s["u_i"], g.step_list(s["t"], dL))
        tip = np.array([float(x) for x in m["p"][-1]])
        assert len(m["p"]) == len(s["t"]) and np.abs(tip - s["p"][-1]).max() < 1e-13          # the scheme the oracle restates
        x0 = np.zeros(22)
        x0[3] = x0[7] = x0[11] = 1
        x0[12:15], x0[15:18] = s["v_i"], s["u_i"]
        ref = solve_ivp(lambda t, x: np_deriv(HELIX_C, HELIX_D, tau, x, t), (0, 0.2), x0, method="DOP853", rtol=1e-13, atol=1e-15)
        errs.append(np.abs(ref.y[0:3, -1] - tip).max())
    assert errs[-1] < 2e-9
    assert 10 < errs[0] / errs[1] < 24 and 10 < errs[1] / errs[2] < 24


def test_bounds_see_what_the_parity_bar_lets_through(orc, monkeypatch):
    """One routing second derivative (tendon 0's r'') scaled by 1 + 1e-9: the shift this makes in a numpy RK4 over the
    fixture's step sequence, added to the oracle's result, fails the truth bound for most states and passes the 1e-9 m /
    1e-10 bar of the parity tests for all of them.  No kernel, no GPU: this checks that the bounds bite."""
    import test_oracle as to
    fx = ftc.load("config2_dl35")
    N = fx["C"].shape[0]
    _, (p, R, L, Li) = _oracle_result(orc, fx)
    assert ftc.compare(fx, p, R, L, Li)[1].all()
    plain = to.np_rinfo

    def rk4(state, v0, u0, steps):
        x = np.zeros(19 + N)
        x[3] = x[7] = x[11] = 1
        x[12:15], x[15:18] = v0, u0
        f = lambda xx, tt: to.np_deriv(fx["C"], fx["D"], state[:N], xx, tt)
        pts = [x[:3].copy()]
        for (t, h), row in steps:
            k1 = f(x, t); k2 = f(x + h / 2 * k1, t + h / 2); k3 = f(x + h / 2 * k2, t + h / 2); k4 = f(x + h * k3, t + h)
            x = x + h / 6 * k1 + h / 3 * k2 + h / 3 * k3 + h / 6 * k4
            if row >= 0:
                pts.append(x[:3].copy())
        return np.array(pts), x[3:12].copy(), x[18], x[19:].copy()

    def run():
        out = []
        for i in range(ftc.N_STATES):
            k = int(fx["n_steps"][i])
            out.append(rk4(fx["states"][i], fx["v0"][i], fx["u0"][i], list(zip(fx["steps"][i, :k], fx["step_row"][i, :k]))))
        return [np.array([o[c] for o in out]) for c in range(4)]

    base = run()
    monkeypatch.setattr(to, "np_rinfo", lambda C, D, t: [(r, rd, rdd * (1 + 1e-9) if j == 0 else rdd) for j, (r, rd, rdd) in enumerate(plain(C, D, t))])
    bent = run()
    d = [b - a for a, b in zip(base, bent)]
    ratio, ok = ftc.compare(fx, p + d[0], R + d[1], L + d[2], Li + d[3])
    print("r'' of tendon 0 scaled by 1 + 1e-9: %d of 24 states outside their bound, worst error / bound %.3g, largest point shift %.3g m"
          % ((~ok).sum(), ratio, np.abs(d[0]).max()))
    assert (~ok).sum() > ftc.N_STATES // 2
    assert np.abs(d[0]).max() <= 1e-9 and np.abs(d[2]).max() <= 1e-10 and np.abs(d[3]).max() <= 1e-10
