"""Tip inverse kinematics on loaded shapes in plain numpy: the specification of tr_ik_loaded_batch (csrc/loaded_ik_host.inc), as
tip_control.py is of the unloaded tr_ik_batch.

For a state p (S entries) and base strains y = (v0, u0), e_w(y, p) is the tip-balance residual of the loaded rod and x(y, p) its tip
after rotate_z (tests/loaded_fk_reference.py).  At an equilibrium, |e_w| <= residual_threshold, the tip of the loaded shape moves
with the state as

    dx/dp = X_p - X_y J_y^-1 J_p,        J_y = de_w/dy, J_p = de_w/dp, X_y = dx/dy, X_p = dx/dp

(the implicit-function theorem on e_w(y(p), p) = 0).  The four blocks are central differences, 13 + 2 S integrations from the
same point, none of them a solve.  The state's steps are levmar's, d = max(|1e-4 p_k|, delta).  The strains' steps are the
shooting's delta itself: levmar's rule gives 1e-4 for v_3 ~ 1, and the moment balance is curved enough in v_3 to put 2e-4 of
truncation error into J_y and 2e-3 into the reduced Jacobian (config1 under gravity; 1e-6 with the absolute step).  The outer iteration is
tip_control.inverse_kinematics_batch's projected Levenberg-Marquardt on p with that Jacobian.  One round of a problem:

  predict      y_trial = y - W (p_trial - p), W = J_y^-1 J_p
  equilibrate  shooting on y at p_trial from y_trial under the problem's load rows (here: Newton, loaded_fk_reference.shoot;
               on the device: shoot_lm_step's rounds).  A trial that does not reach the threshold is a rejected step
               (mu *= nu, nu *= 2); a start that does not ends its problem with equilibrium = 0 and error = inf
  linearise    the 13 + 2 S lanes: lane 0 the equilibrated trial, lanes 1 .. 12 y -+ d_j, lanes 13 .. p -+ delta_k at fixed y
  step         one Newton step on the trial's strains with the new J_y, dy = -J_y^-1 e_w, which moves its tip by X_y dy (the
               shooting stops at the threshold, which leaves the tip up to ~1e-5 m from the equilibrium's); accept / reject on
               |des - x|^2, the new reduced Jacobian and W, the stop tests, the next trial point

Loads are one set per call, tr_edge_loads' meaning (or, here only, one row per problem): frame 'base' rows are fixed before the state's rotation, frame 'world' rows
are turned by Rz(-theta) of the state they act on -- every lane turns them with its own theta, so a lane whose rotation is perturbed
sees the load it would see there.
"""
import numpy as np

import loaded_fk_reference as ref


# The wider state sizes (S = 6, 7, 9: tests/test_gpu_loaded_ik.py, n5_world, n6_world, n8_world): goals are case B's loaded tips of
# loaded_fk_<name>.npz, gravity in the world frame, starts offset by sigma = 0.3 N and 0.05 rad, max_iters = 25.  This scheme then
# reaches 24, 22 and 21 of the 24 goals at 1e-4 m (the laggards: rows 20 - 22, whose tensions sit on the box), and ends these rows at
# 0.5e-4 m or less.  tests/test_loaded_ik_reference.py re-runs it and holds the rows to this table; the device test reads the table
# instead of running 10 - 16 s of numpy per robot.
WIDE_SIGMA, WIDE_MAX_ITERS = (0.3, 0.05), 25
WIDE_HALF_TOL_ROWS = {"n5": (6, 10, 11, 14, 18), "n6": (2, 5, 6, 12, 16), "n8": (6, 10, 11, 16, 17)}


def bounds(rob):
    """Bounds::from_robot for a robot without retraction: (lower, upper)."""
    N, S = rob.n_tendons, rob.n_tendons + int(bool(rob.c.enable_rotation))
    lo, hi = np.zeros(S), np.zeros(S)
    hi[:N] = [rob.c.max_tension[k] for k in range(N)]
    if S > N:
        lo[N], hi[N] = np.finfo(float).min, np.finfo(float).max
    return lo, hi


def offset_starts(rob, states, sigma_tension, sigma_rotation=0.0, seed=5):
    """The starts of the tests: the states plus seeded normal offsets, clipped to the bounds."""
    rng = np.random.default_rng(seed)
    st = np.array(states, float)
    N = rob.n_tendons
    off = rng.normal(size=st.shape)
    off[:, :N] *= sigma_tension
    off[:, N:] *= sigma_rotation
    lo, hi = bounds(rob)
    return np.clip(st + off, lo, hi)


# One distributed row with all six numbers non-zero (tests/loaded_edges_common.py: DIST_FULL, gravity plus a force of case D's size
# with a z component, and a distributed moment) on config1, sigma = 3 N: the set `config1_full` of tests/test_gpu_loaded_ik.py -- the
# one that runs fk_loaded_lin's load.l.  No fixture holds shapes under that row, so the goals are the numpy shooting's tips under it
# (loaded_tips), as the other sets' goals are the fixtures' tips under their loads.  This scheme reaches 24 of 24 in at most 6 outer
# iterations (measured when the set was added; tests/test_loaded_ik_reference.py holds it to that).
FULL_REACHED = 24


def loaded_tips(rob, states, wrench=None, dist=None):
    """(n, 3) tips of the loaded shapes of `states` under one BASE-frame load set, by the numpy shooting from the unloaded start."""
    w, d = (np.zeros(6) if a is None else np.asarray(a, float) for a in (wrench, dist))
    sol = ref.shoot(rob, states, F_e=w[:3], L_e=w[3:], f_e=d[:3], l_e=d[3:])
    assert sol["converged"].all()
    return np.ascontiguousarray(sol["p"][:, -1])


def load_rows(rob, states, wrench=None, dist=None, frame="base"):
    """(n, 6) wrench and distributed-load rows of the states, in the frame before the state's rotation."""
    st = np.atleast_2d(np.asarray(states, float))
    n, N = st.shape[0], rob.n_tendons
    out = []
    for v in (wrench, dist):
        v = np.zeros(6) if v is None else np.asarray(v, float)
        v = np.broadcast_to(v, (n, 6))                                  # one set for all (the C ABI), or one row per state
        r = v.copy()
        if frame == "world" and rob.c.enable_rotation:
            c, s = np.cos(st[:, N]), np.sin(st[:, N])
            for h in (0, 3):                                            # Rz(-theta) (x, y, z) = (c x + s y, c y - s x, z)
                r[:, h + 0] = c * v[:, h + 0] + s * v[:, h + 1]
                r[:, h + 1] = c * v[:, h + 1] - s * v[:, h + 0]
        out.append(r)
    return out[0], out[1]


def tips_and_residuals(rob, states, y, wrench=None, dist=None, frame="base", routing=None):
    """One integration per row: (x (n, 3) after rotate_z, e_w (n, 6))."""
    st = np.atleast_2d(np.asarray(states, float))
    n, N = st.shape[0], rob.n_tendons
    w, d = load_rows(rob, st, wrench, dist, frame)
    routing = routing or ref.Routing(rob)
    tau = np.ascontiguousarray(st[:, :N])
    sh = ref.integrate(rob, tau, np.asarray(y, float).reshape(n, 6), d[:, :3].copy(), d[:, 3:].copy(), routing)
    e = ref.tip_residual(rob, tau, sh, w[:, :3], w[:, 3:], routing)
    theta = st[:, N] if rob.c.enable_rotation else np.zeros(n)
    c, s = np.cos(theta), np.sin(theta)
    p = sh["p"][:, -1]
    x = np.stack([c * p[:, 0] - s * p[:, 1], s * p[:, 0] + c * p[:, 1], p[:, 2]], axis=1)
    return x, e


def linearise(rob, states, y, wrench=None, dist=None, frame="base", delta=1e-6, delta_y=1e-6, routing=None):
    """The 13 + 2 S lanes of every row.  dict(x (n, 3), e (n, 6), J_y (n, 6, 6), J_p (n, 6, S), X_y (n, 3, 6), X_p (n, 3, S),
    W (n, 6, S) = J_y^-1 J_p, J_r (n, 3, S) = X_p - X_y W, y_c (n, 6) = y - J_y^-1 e, x_c (n, 3) = x - X_y J_y^-1 e)."""
    st = np.atleast_2d(np.asarray(states, float))
    y = np.asarray(y, float).reshape(-1, 6)
    n, S = st.shape
    Q = 13 + 2 * S
    dy, dp = np.full_like(y, delta_y), ref.fd_steps(st, delta)
    sl, yl = np.repeat(st[:, None, :], Q, axis=1), np.repeat(y[:, None, :], Q, axis=1)
    j, k = np.arange(6), np.arange(S)
    yl[:, 1 + 2 * j, j] -= dy
    yl[:, 2 + 2 * j, j] += dy
    sl[:, 13 + 2 * k, k] -= dp
    sl[:, 14 + 2 * k, k] += dp
    lane_rows = lambda a: a if a is None or np.ndim(a) == 1 else np.repeat(np.asarray(a, float), Q, axis=0)
    x, e = tips_and_residuals(rob, sl.reshape(-1, S), yl.reshape(-1, 6), lane_rows(wrench), lane_rows(dist), frame, routing)
    x, e = x.reshape(n, Q, 3), e.reshape(n, Q, 6)
    diff = lambda a, first, cnt, d: np.transpose((a[:, first + 1:first + 2 * cnt:2] - a[:, first:first + 2 * cnt:2]) * (0.5 / d)[:, :, None],
                                                 (0, 2, 1))
    J_y, X_y = diff(e, 1, 6, dy), diff(x, 1, 6, dy)
    J_p, X_p = diff(e, 13, S, dp), diff(x, 13, S, dp)
    with np.errstate(all="ignore"):
        W, c = np.full((n, 6, S), np.nan), np.full((n, 6), np.nan)
        for i in range(n):
            if np.isfinite(J_y[i]).all() and np.isfinite(J_p[i]).all() and np.isfinite(e[i, 0]).all():
                try:
                    sol = np.linalg.solve(J_y[i], np.concatenate([J_p[i], e[i, 0][:, None]], axis=1))
                    W[i], c[i] = sol[:, :S], sol[:, S]
                except np.linalg.LinAlgError:
                    pass
        J_r = X_p - X_y @ W
        x_c = x[:, 0] - np.einsum("nij,nj->ni", X_y, c)
    return dict(x=x[:, 0], e=e[:, 0], J_y=J_y, J_p=J_p, X_y=X_y, X_p=X_p, W=W, J_r=J_r, y_c=y - c, x_c=x_c)


def equilibrate(rob, states, guess, wrench=None, dist=None, frame="base", tol=None, max_iters=10):
    """Shooting on the base strains of every row from `guess` (None: the unloaded start): (y (n, 6), reached (n,) bool,
    integrations (n,))."""
    st = np.atleast_2d(np.asarray(states, float))
    w, d = load_rows(rob, st, wrench, dist, frame)
    tol = rob.c.residual_threshold if tol is None else tol
    with np.errstate(all="ignore"):
        out = ref.shoot(rob, st, F_e=w[:, :3], L_e=w[:, 3:], f_e=d[:, :3], l_e=d[:, 3:], guess=guess, tol=tol, max_iters=max_iters)
    return out["vu0"], out["e"] <= tol, 13 * (out["iters"] + 1)


def canonical_angle(theta):
    two_pi = 2 * np.pi
    return np.fmod(np.fmod(theta + np.pi, two_pi) + two_pi, two_pi) - np.pi


def inverse_kinematics_loaded_batch(rob, initial_states, des, wrench=None, dist=None, frame="base", guess=None, lower=None, upper=None,
                                    max_iters=100, mu_init=0.1, stop_threshold_JT_err_inf=1e-9, stop_threshold_Dp=1e-4,
                                    stop_threshold_err=1e-4, finite_difference_delta=1e-6, shoot_delta=1e-6, shoot_tol=None):
    """Solve tip(state under the load) = des from every row of initial_states (des: (3,) or one row per start).
    dict(state, tip, error, iters, integrations, vu0, equilibrium, rounds)."""
    assert not rob.c.enable_retraction
    p = np.array(np.atleast_2d(np.asarray(initial_states, float)))
    n, S = p.shape
    N = rob.n_tendons
    des = np.broadcast_to(np.asarray(des, float), (n, 3)).copy()
    lo, hi = bounds(rob)
    lo = lo if lower is None else np.asarray(lower, float)
    hi = hi if upper is None else np.asarray(upper, float)
    def ld(idx):                                                      # the loads of the problems idx (one set for all, or rows)
        row = lambda a: a if a is None or np.ndim(a) == 1 else np.asarray(a, float)[idx]
        return dict(wrench=row(wrench), dist=row(dist), frame=frame)
    Q = 13 + 2 * S
    eps1, eps2_sq, eps3_sq = stop_threshold_JT_err_inf, stop_threshold_Dp ** 2, stop_threshold_err ** 2
    routing = ref.Routing(rob)
    p = np.clip(p, lo, hi)
    y, eq, calls = equilibrate(rob, p, guess, tol=shoot_tol, **ld(slice(None)))
    calls = calls.astype(np.int64)
    f, J, W = np.full((n, 3), np.nan), np.zeros((n, 3, S)), np.zeros((n, 6, S))
    err2 = np.full(n, np.inf)
    mu, nu = np.full(n, mu_init), np.full(n, 2.0)
    iters = np.zeros(n, dtype=int)
    active = np.zeros(n, dtype=bool)
    rounds = 0

    def free_gradient(pp, gg):
        blocked = ((pp <= lo) & (gg < 0)) | ((pp >= hi) & (gg > 0))
        return np.where(blocked, 0.0, gg)

    k0 = np.flatnonzero(eq)
    if k0.size:
        lin = linearise(rob, p[k0], y[k0], delta=finite_difference_delta, delta_y=shoot_delta, routing=routing, **ld(k0))
        rounds += 1
        calls[k0] += Q
        f[k0], J[k0], W[k0], y[k0] = lin["x_c"], lin["J_r"], lin["W"], lin["y_c"]
        e = des[k0] - f[k0]
        err2[k0] = (e * e).sum(1)
        A = np.einsum("nki,nkj->nij", J[k0], J[k0])
        m0 = mu_init * np.max(np.diagonal(A, axis1=1, axis2=2), axis=1)
        mu[k0] = np.where(m0 > 0, m0, mu_init)
        g = np.einsum("nki,nk->ni", J[k0], e)
        active[k0] = (err2[k0] > eps3_sq) & (np.abs(free_gradient(p[k0], g)).max(1) > eps1)
    eye = np.eye(S)
    while True:
        idx = np.flatnonzero(active & (iters < max_iters))
        if idx.size == 0:
            break
        active[:] = False
        e = des[idx] - f[idx]
        A = np.einsum("nki,nkj->nij", J[idx], J[idx])
        g = np.einsum("nki,nk->ni", J[idx], e)
        with np.errstate(all="ignore"):
            try:
                dp = np.linalg.solve(A + mu[idx, None, None] * eye, g[..., None])[..., 0]
            except np.linalg.LinAlgError:
                dp = np.full_like(g, np.nan)
        pn = np.clip(p[idx] + dp, lo, hi)
        dpe = pn - p[idx]
        small = ~((dpe * dpe).sum(1) > eps2_sq * (p[idx] * p[idx]).sum(1))
        iters[idx] += 1
        go = ~small
        if not go.any():
            continue
        k, pn, dpe, g = idx[go], pn[go], dpe[go], g[go]
        y_trial = y[k] - np.einsum("nij,nj->ni", W[k], dpe)                  # predict
        yn, reached, c = equilibrate(rob, pn, y_trial, tol=shoot_tol, **ld(k))  # equilibrate
        lin = linearise(rob, pn, yn, delta=finite_difference_delta, delta_y=shoot_delta, routing=routing, **ld(k))
        rounds += 1
        calls[k] += c + Q
        en = des[k] - lin["x_c"]
        err2n = (en * en).sum(1)
        pred = (dpe * (mu[k, None] * dpe + g)).sum(1)
        with np.errstate(all="ignore"):
            rho = np.where(pred > 0, (err2[k] - err2n) / np.where(pred > 0, pred, 1.0), -1.0)
        acc = reached & (rho > 0)
        ka = k[acc]
        p[ka], y[ka], f[ka], J[ka], W[ka], err2[ka] = pn[acc], lin["y_c"][acc], lin["x_c"][acc], lin["J_r"][acc], lin["W"][acc], err2n[acc]
        mu[ka] *= np.maximum(1.0 / 3.0, 1.0 - (2.0 * rho[acc] - 1.0) ** 3)
        nu[ka] = 2.0
        ga = np.einsum("nki,nk->ni", J[ka], en[acc])
        active[ka] = (err2[ka] > eps3_sq) & (np.abs(free_gradient(p[ka], ga)).max(1) > eps1)
        kr = k[~acc]
        mu[kr] *= nu[kr]
        nu[kr] *= 2.0
        active[kr] = np.isfinite(mu[kr]) & (mu[kr] < 1e300)
    state = p.copy()
    if rob.c.enable_rotation:
        state[:, N] = canonical_angle(state[:, N])
    return dict(state=state, tip=f, error=np.sqrt(err2), iters=iters, integrations=calls, vu0=y, equilibrium=eq, rounds=rounds)
