"""CPU side of the extended-precision FK truth (tests/golden/fk_truth_*.npz, tests/golden/make_fk_truth.py): the fixtures
still describe this oracle, the generator still reproduces them, the mpmath model agrees with an integrator and a
right-hand side that share nothing with it, and the bounds of tests/test_gpu_fk_truth.py see an error that the 1e-9 m
parity bar lets through -- in the integrator, in the stepping of a retracted lane's own first interval and in the home-length
quadrature."""
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
        assert np.array_equal(fx["steps"][i, :k, 0][np.r_[True, ends[:-1] >= 0][:k]], s["t"][:-1])   # and restarts at exactly t[j]
    if name == "config2_dl35":
        assert (fx["step_row"][:, 0] == -1).all() and fx["n_steps"][0] == fx["n_points"][0]      # two steps in the first interval
    ratio, ok = ftc.compare(fx, *res)
    assert ok.all() and ratio <= 0.25 + 1e-12                                           # the bound is at least 4 E_ref
    assert (name in ftc.RETRACTION) == bool(fx["consts"][9]) == ("home_hi" in fx)
    if name in ftc.RETRACTION:
        orb = _oracle_robot(orc, fx)
        e_home = ftc.err_vs_truth(np.array([orb.home_shape(s[-1])["L_i"] for s in fx["states"]]), fx["home_hi"], fx["home_lo"])
        assert (np.abs(e_home - fx["Eref_home"]) <= np.spacing(fx["Eref_home"])).all()
        assert (e_home <= 0.25 * ftc.bounds(fx)["home"]).all()
        assert ftc.separated(fx) is None
    if name in ftc.NEW_RETRACTION:
        L, dL = fx["consts"][:2]
        assert dL == L / 40 and np.array_equal(fx["states"][:15, -1], ftc.special_s_start(L, dL)[:15])
        assert ((fx["states"][15:, -1] >= 0) & (fx["states"][15:, -1] <= 0.6 * L)).all()
        one = fx["n_points"] == 1                        # one-point backbones: the truth is p = 0, L_i = 0 ...
        assert one.tolist() == [False] * 11 + [True] * 3 + [False] * 10 and not fx["p_hi"][one].any() and not fx["Li_hi"][one].any()
        # ... and home = 0: s_start >= L, and the quadrature over one point; the helix form is (L - s_start) helix_scale even then
        assert not fx["home_hi"][12:14].any() and (fx["home_hi"][11] == 0).all() == (name != "config2_ret_edges")
        assert ftc.exact_zero(fx).sum() == (2 if name == "config2_ret_edges" else 3) * fx["C"].shape[0]
        cls = ftc.first_interval_class(fx)
        print("%s: first-interval classes %s" % (name, {ftc.CLASS_NAMES[c]: np.flatnonzero(cls == c).tolist() for c in range(5)}))
        if name == "config3_ret_edges":
            assert all((cls == c).any() for c in range(5))
        # the row that is not in the fixture: the oracle integrates a backbone longer than L for a negative s_start
        neg = fx["states"][0].copy()
        neg[-1] = ftc.special_s_start(L, dL)[15]
        assert neg[-1] < 0 and len(orb.shape(neg)["t"]) > int(fx["n_points"].max())


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
        if name in ftc.RETRACTION:
            t_pts = ftc.abscissae(fx, i)
            assert len(t_pts) == fx["n_points"][i]
            got += g.home_truth(fx["consts"], fx["C"], fx["D"], fx["states"][i, -1], t_pts)
            hi, lo = np.concatenate([hi, fx["home_hi"][i]]), np.concatenate([lo, fx["home_lo"][i]])
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


def _steps(fx, i):
    k = int(fx["n_steps"][i])
    return list(zip(fx["steps"][i, :k], fx["step_row"][i, :k]))


def _np_rk4(fx, i, steps):
    """Classical RK4 of state i over [((t, h), row)] on the numpy right-hand side of tests/test_oracle.py: (points, R at the tip,
    L, L_i), not rotated."""
    import test_oracle as to
    N = fx["C"].shape[0]
    x = np.zeros(19 + N)
    x[3] = x[7] = x[11] = 1
    x[12:15], x[15:18] = fx["v0"][i], fx["u0"][i]
    f = lambda xx, tt: to.np_deriv(fx["C"], fx["D"], fx["states"][i, :N], xx, tt)
    pts = [x[:3].copy()]
    for (t, h), row in steps:
        k1 = f(x, t); k2 = f(x + h / 2 * k1, t + h / 2); k3 = f(x + h / 2 * k2, t + h / 2); k4 = f(x + h * k3, t + h)
        x = x + h / 6 * k1 + h / 3 * k2 + h / 3 * k3 + h / 6 * k4
        if row >= 0:
            pts.append(x[:3].copy())
    return np.array(pts), x[3:12].copy(), x[18], x[19:].copy()


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

    def run():
        out = [_np_rk4(fx, i, _steps(fx, i)) for i in range(ftc.N_STATES)]
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


@pytest.mark.parametrize("name", ["n5", "helix5"])
def test_bounds_of_the_five_tendon_fixtures_see_tendon_4(orc, monkeypatch, name):
    """test_bounds_see_what_the_parity_bar_lets_through on the widths of round 19, at the LAST tendon of five -- the one a
    kernel of another width would drop or misplace: its r'' scaled by 1 + 1e-9 leaves the bound on most states and stays under
    1e-9 m / 1e-10."""
    import test_oracle as to
    fx = ftc.load(name)
    assert fx["C"].shape[0] == 5
    _, (p, R, L, Li) = _oracle_result(orc, fx)
    plain = to.np_rinfo

    def run():
        out = [_np_rk4(fx, i, _steps(fx, i)) for i in range(ftc.N_STATES)]
        pts = np.array([o[0] for o in out])
        th = fx["states"][:, 5]                                          # rotate_z of the points; the frame, L and L_i shifts stay unrotated
        c, s = np.cos(th)[:, None], np.sin(th)[:, None]
        rot = np.stack([c * pts[:, :, 0] - s * pts[:, :, 1], s * pts[:, :, 0] + c * pts[:, :, 1], pts[:, :, 2]], axis=2)
        return [rot] + [np.array([o[k] for o in out]) for k in (2, 3)]

    base = run()
    monkeypatch.setattr(to, "np_rinfo", lambda C, D, t: [(r, rd, rdd * (1 + 1e-9) if j == 4 else rdd) for j, (r, rd, rdd) in enumerate(plain(C, D, t))])
    bent = run()
    d = [b - a for a, b in zip(base, bent)]
    ratio, ok = ftc.compare(fx, p + d[0], R, L + d[1], Li + d[2])
    print("%s, r'' of tendon 4 scaled by 1 + 1e-9: %d of 24 states outside their bound, worst error / bound %.3g, largest point shift %.3g m"
          % (name, (~ok).sum(), ratio, np.abs(d[0]).max()))
    assert (~ok).sum() > ftc.N_STATES // 2
    assert np.abs(d[0]).max() <= 1e-9 and np.abs(d[1]).max() <= 1e-10 and np.abs(d[2]).max() <= 1e-10


@pytest.mark.parametrize("name", ["n5", "n6", "helix5", "helix6"])
def test_curled_states_collide_by_the_oracle_alone(orc, name):
    """The states of test_fallback_pass_on_curled_states (tests/test_gpu_fk_truth.py), here with the oracle's own shapes: at
    least 8 converge and collide with themselves, at least 8 converge and do not, all of those within the +- 1 m length limits."""
    fx = ftc.load(name)
    N = fx["C"].shape[0]
    L, dL, ro, ri, E, nu, r, res, rot, ret = (float(x) for x in fx["consts"])
    rob = orc.Robot(fx["C"].tolist(), fx["D"].tolist(), r=ftc.CURL_RADIUS, L=L, dL=dL, ro=ro, ri=ri, E=E, nu=nu, max_tension=[ftc.CURL_TENSION] * N,
                    min_length=[-1.0] * N, max_length=[1.0] * N, enable_rotation=True, enable_retraction=False, residual_threshold=res)
    st = ftc.curled_states(fx)
    assert st.shape == (ftc.N_CURLS, N + 1) and (st[:, :N] <= ftc.CURL_TENSION).all()
    shapes = [rob.shape(s) for s in st]
    home = rob.home_shape()["L_i"]
    conv = np.array([bool(s["converged"]) for s in shapes])
    hits = np.array([rob.collides_self(s["p"]) for s in shapes])
    assert all(rob.is_within_length_limits(home, s["L_i"]) for s, c in zip(shapes, conv) if c)
    print("%s: %d converged and self-colliding, %d converged and free, %d unconverged" % (name, (conv & hits).sum(), (conv & ~hits).sum(), (~conv).sum()))
    assert (conv & hits).sum() >= 8 and (conv & ~hits).sum() >= 8


def test_point_bound_sees_one_long_step_in_the_first_interval(orc):
    """A retracted lane whose own first interval is longer than dL takes two RK4 steps there (dL, then the rest), as
    integrate_times does.  One step over the whole interval instead -- 1.25 dL for dL + 0.25 dL -- is a fourth-order difference
    at or below the 1e-9 m of the parity tests; added to the oracle's result it leaves the point bound for every two-step state of config3_ret_edges."""
    fx = ftc.load("config3_ret_edges")
    _, (p, R, L, Li) = _oracle_result(orc, fx)
    two = np.flatnonzero(ftc.first_interval_class(fx) == ftc.TWO_STEPS)
    assert len(two) >= 5 and 8 in two                    # (row 8: s_start = L - 1.25 dL, a two-point backbone)
    bound = ftc.bounds(fx)["p"]
    factors, shifts = [], []
    for i in two:
        steps = _steps(fx, i)
        ((t0, h0), r0), ((t1, h1), r1) = steps[:2]
        assert r0 < 0 and r1 == 1 and h0 == fx["consts"][1] and t1 == t0 + h0
        merged = [((t0, (t1 + h1) - t0), 1)] + steps[2:]
        d = _np_rk4(fx, i, merged)[0] - _np_rk4(fx, i, steps)[0]
        q = p[i].copy()
        q[:len(d)] += d
        err = ftc.errors(fx, np.where(np.arange(ftc.N_STATES)[:, None, None] == i, q[None], p), R, L, Li)["p"][i]
        factors.append(err / bound[i])
        shifts.append(np.abs(d).max())
    print("one RK4 step over a first interval of more than dL: point shift %.2g .. %.2g m, error / point bound %s"
          % (min(shifts), max(shifts), ", ".join("%d: %.3g" % x for x in zip(two, factors))))
    assert min(factors) > 1.0


def _np_home(fx, i, rule="tip", scale=1.0):
    """home_shape(s_start).L_i of state i in fp64 numpy: orc_home_shape's rule (rule = "tip"), Simpson with the trailing odd
    interval dropped ("none") or with the trapezoid at the base instead of the tip ("base"); scale multiplies the helix factor."""
    L, dL = fx["consts"][:2]
    s = min(max(fx["states"][i, -1], 0.0), L)
    N = fx["C"].shape[0]
    if s == L:
        return np.zeros(N)
    t = ftc.abscissae(fx, i)
    out = np.empty(N)
    for j in range(N):
        C, D = np.polynomial.Polynomial(fx["C"][j]), np.polynomial.Polynomial(fx["D"][j])
        if D.degree() == 0 and C.degree() == 0:
            out[j] = L - s
        elif D.degree() == 0 and C.degree() == 1:
            out[j] = (L - s) * (np.sqrt(1 + D.coef[0] ** 2 * C.coef[1] ** 2) * scale)
        else:
            v = np.sqrt(D.deriv()(t) ** 2 + D(t) ** 2 * C.deriv()(t) ** 2 + 1)
            n = len(v)
            lo, hi, odd = 0, n - 1, 0.0
            if (n - 1) % 2:
                if rule == "tip":
                    odd, hi = 0.5 * dL * (v[n - 2] + v[n - 1]), n - 2
                elif rule == "base":
                    odd, lo = 0.5 * dL * (v[0] + v[1]), 1
                else:
                    hi = n - 2
            w = v[lo:hi + 1]
            simpson = 0.0 if len(w) < 3 else (w[0] + w[-1] + (np.where(np.arange(1, len(w) - 1) % 2 == 1, 4.0, 2.0) * w[1:-1]).sum()) * dL / 3.0
            out[j] = odd + simpson
    return out


def test_home_bound_sees_a_wrong_simpson_tail_and_a_wrong_helix_scale():
    """The home-length truth and its bound: a numpy restatement of the rule is within it, and is outside it for every state it can
    be -- Simpson without the trapezoid of a trailing odd interval (every odd-interval state of config3_ret_edges), the trapezoid
    at the base instead of the tip (the same states but the one-interval backbones, where both are the same trapezoid), and the
    helix factor of config2_ret_edges scaled by 1 + 1e-9 (every state with a backbone to measure)."""
    fx = ftc.load("config3_ret_edges")
    b = ftc.bounds(fx)["home"]
    err = lambda f, i, **kw: ftc.err_vs_truth(_np_home(f, i, **kw), f["home_hi"][i], f["home_lo"][i])
    nint = fx["n_points"] - 1
    odd = np.flatnonzero(nint % 2 == 1)
    assert len(odd) >= 6 and (nint[odd] == 1).any() and (nint[odd] >= 3).any() and (nint % 2 == 0).sum() >= 6
    for i in range(ftc.N_STATES):
        assert (err(fx, i) <= b[i]).all(), i
    none = np.array([(err(fx, i, rule="none") / b[i]).min() for i in odd])
    base = np.array([(err(fx, i, rule="base") / b[i]).min() for i in odd if nint[i] >= 3])
    print("home length of config3_ret_edges, smallest error / bound over the tendons: no trapezoid %.3g .. %.3g, trapezoid at the base %.3g .. %.3g"
          % (none.min(), none.max(), base.min(), base.max()))
    assert none.min() > 1.0 and base.min() > 1.0
    hx = ftc.load("config2_ret_edges")
    hb = ftc.bounds(hx)["home"]
    some = np.flatnonzero(hx["n_points"] > 1)
    for i in range(ftc.N_STATES):
        assert (err(hx, i) <= hb[i]).all(), i
    scaled = np.array([(err(hx, i, scale=1 + 1e-9) / hb[i]).min() for i in some])
    print("home length of config2_ret_edges with helix_scale (1 + 1e-9): error / bound %.3g .. %.3g" % (scaled.min(), scaled.max()))
    assert len(some) == 21 and scaled.min() > 1.0
