"""The loaded forward kinematics of robots WITH retraction in plain numpy: the reference of the loaded-retraction tests and fixtures.

TendonRobot::general_tension_shape(tau, s_start, ...) (tendon/TendonRobot.cpp:689-952): s_start is truncated to L; at s_start == L
the result is one point at the origin; otherwise the rod of loaded_fk_reference.py is integrated over t_range(s_start, L, dL) -- every
state on its OWN grid, with its own step list (two RK4 steps where its first interval exceeds dL) and its own number of points --
and shot on (v0, u0) from the unloaded solution AT the state's s_start.  The tip residual takes the routing at s = L, which does not
depend on the retraction; a state whose grid is the single point s_start < L evaluates it at R = I with its start strains.

The right-hand side, the tip residual, the difference steps and rotate_z are loaded_fk_reference's; the routing, the grids and the
unloaded start come from the CPU oracle (oracle/oracle.py: r_info, t_range, solve_initial_bending).  A state's 13 integrations run as
one array program; the states are a Python loop, since no two share a grid.

`fault` plants one of three mistakes (tests/test_loaded_ret_truth.py shows that the fixtures' bounds see each of them):
  "scale"       the distributed load off by 1 + 1e-8
  "prev_frame"  the load rotated with the PREVIOUS stage's frame (the step's start frame in its first stage)
  "table"       the first interval integrated with the routing of the SHARED grid's abscissae, t_range(0)[shift] onwards, instead
                of the state's own
"""
import numpy as np

from loaded_fk_reference import DBL_EPS, Routing, fd_steps, rhs, rotate_z, stiffness, tip_residual

FAULTS = ("scale", "prev_frame", "table")


def step_list(t_pts, dL):
    """integrate_times' steps over the abscissae t_pts, [(t, h, row)]: steps of min(dL, remaining) while remaining > eps; row = the
    backbone point the step ends in, -1 inside an interval (tests/golden/make_fk_truth.py: step_list, the same rule)."""
    out = []
    for j in range(len(t_pts) - 1):
        cur, tn = float(t_pts[j]), float(t_pts[j + 1])
        while tn - cur > DBL_EPS:
            h = dL if dL < tn - cur else tn - cur
            nxt = cur + h
            out.append((cur, h, j + 1 if not (tn - nxt > DBL_EPS) else -1))
            cur = nxt
    return out


def state_grid(rob, s_start):
    """(abscissae, steps, single) of one state: `single` is general_tension_shape's early return (s_start >= L)."""
    L = rob.c.L
    s = min(float(s_start), L)
    if s == L:
        return np.array([L]), [], True
    t = np.asarray(rob.t_range(s), float)
    return t, step_list(t, rob.c.dL), False


def unloaded_start(rob, tau, s_start):
    v, u, _ = rob.solve_initial_bending(tau, min(float(s_start), rob.c.L))
    return np.concatenate([v, u])


def integrate(rob, tau, vu0, f_e, l_e, steps, n_points, routing=None, fault=None):
    """RK4 over ONE state's steps for a batch of base strains: tau (N,), vu0 (B, 6), f_e, l_e (3,).  dict(p (B, n_points, 3),
    R (B, n_points, 3, 3), v, u (B, 3) at the tip, L (B,), L_i (B, N))."""
    routing = routing or Routing(rob)
    Kse, Kbt = stiffness(rob)
    B, N = len(vu0), len(tau)
    tauB = np.tile(np.asarray(tau, float), (B, 1))
    scale = 1.0 + 1e-8 if fault == "scale" else 1.0
    fB, lB = np.tile(np.asarray(f_e, float) * scale, (B, 1)), np.tile(np.asarray(l_e, float) * scale, (B, 1))
    st = [np.zeros((B, 3)), np.tile(np.eye(3), (B, 1, 1)), vu0[:, :3].copy(), vu0[:, 3:].copy(), np.zeros(B), np.zeros((B, N))]
    pts, Rs = np.zeros((B, n_points, 3)), np.zeros((B, n_points, 3, 3))
    pts[:, 0], Rs[:, 0] = st[0], st[1]
    shared = np.asarray(rob.t_range(0.0), float)
    shift = len(shared) - n_points
    own = True                                                        # inside the state's own first interval

    def axpy(x, a, k):
        return [xi + a * ki for xi, ki in zip(x, k)]

    for cur, h, obs in steps:
        where = cur
        if fault == "table" and own:
            where = shared[shift] + (cur - steps[0][0])               # the shared table's abscissae for the same steps
        prev = [st[1]]                                                # the frame of the stage before (fault "prev_frame")

        def f(x, tt):
            if fault == "prev_frame":
                out = rhs_with_frame(Kse, Kbt, routing(tt), tauB, x[1], x[2], x[3], fB, lB, prev[0])
            else:
                out = rhs(Kse, Kbt, routing(tt), tauB, x[1], x[2], x[3], fB, lB)
            prev[0] = x[1]
            return out

        k1 = f(st, where)
        k2 = f(axpy(st, h * 0.5, k1), where + h * 0.5)
        k3 = f(axpy(st, h * 0.5, k2), where + h * 0.5)
        k4 = f(axpy(st, h, k3), where + h)
        b1, b2 = h * (1.0 / 6.0), h * (1.0 / 3.0)
        st = [x + b1 * a + b2 * b + b2 * c + b1 * d for x, a, b, c, d in zip(st, k1, k2, k3, k4)]
        if obs >= 0:
            pts[:, obs], Rs[:, obs] = st[0], st[1]
            own = False
    return dict(p=pts, R=Rs, v=st[2], u=st[3], L=st[4], L_i=st[5])


def rhs_with_frame(Kse, Kbt, route, tau, R, v, u, f_e, l_e, R_load):
    """rhs() with the load turned by R_load instead of R: R^T_load f = R^T (R R^T_load f), so the load is re-expressed for rhs()."""
    back = R @ np.swapaxes(R_load, -1, -2)
    return rhs(Kse, Kbt, route, tau, R, v, u, (back @ f_e[..., None])[..., 0], (back @ l_e[..., None])[..., 0])


def _loads(n, F_e, L_e, f_e, l_e):
    rows = lambda a: np.zeros((n, 3)) if a is None else np.broadcast_to(np.asarray(a, float), (n, 3)).copy()
    return rows(F_e), rows(L_e), rows(f_e), rows(l_e)


def _split(rob, states):
    st = np.atleast_2d(np.asarray(states, float))
    N = rob.n_tendons
    assert rob.c.enable_retraction
    theta = st[:, N].copy() if rob.c.enable_rotation else np.zeros(len(st))
    return st, np.ascontiguousarray(st[:, :N]), theta, st[:, -1]


def evaluate(rob, states, vu0, F_e=None, L_e=None, f_e=None, l_e=None, fault=None):
    """One integration per state from given base strains.  dict(p (n, P, 3) and R (n, P, 3, 3) after rotate_z, from row 0, NaN past
    n_points; n_points (n,); L, L_i, e (n, 6), vuL (n, 6) the tip strains).  A single state (s_start >= L): one point at the
    origin, zeros, e = 0."""
    st, tau, theta, s0 = _split(rob, states)
    n, P = len(st), rob.max_points()
    F_e, L_e, f_e, l_e = _loads(n, F_e, L_e, f_e, l_e)
    vu0 = np.asarray(vu0, float).reshape(n, 6)
    routing = Routing(rob)
    out = dict(p=np.full((n, P, 3), np.nan), R=np.full((n, P, 3, 3), np.nan), n_points=np.zeros(n, np.int32), L=np.zeros(n),
               L_i=np.zeros((n, rob.n_tendons)), e=np.zeros((n, 6)), vuL=vu0.copy())
    for i in range(n):
        t, steps, single = state_grid(rob, s0[i])
        k = len(t)
        out["n_points"][i] = k
        if single:
            out["p"][i, 0], out["R"][i, 0] = 0.0, rotate_z(np.zeros((1, 1, 3)), np.eye(3)[None, None], theta[i:i + 1])[1][0, 0]
            continue
        sh = integrate(rob, tau[i], vu0[i:i + 1], f_e[i], l_e[i], steps, k, routing, fault)
        out["e"][i] = tip_residual(rob, tau[i:i + 1], sh, F_e[i:i + 1], L_e[i:i + 1], routing)[0]
        p, R = rotate_z(sh["p"], sh["R"], theta[i:i + 1])
        out["p"][i, :k], out["R"][i, :k] = p[0], R[0]
        out["L"][i], out["L_i"][i] = sh["L"][0], sh["L_i"][0]
        out["vuL"][i] = np.concatenate([sh["v"][0], sh["u"][0]])
    return out


def shoot(rob, states, F_e=None, L_e=None, f_e=None, l_e=None, guess=None, tol=1e-11, max_iters=10, delta=1e-6):
    """Newton shooting per state, as loaded_fk_reference.shoot: start `guess` (n, 6) or the unloaded solution at the state's s_start;
    stops a state at |e| <= tol or after max_iters steps.  dict(vu0, p, R (rotate_z applied, NaN past n_points), n_points, L, L_i,
    e (n,) = |e|, iters, converged, C (n,) = max over the backbone points of |dp/d(v0, u0) J^-1|_2 in m/N).  Single states:
    converged with zero iterations, C = 0."""
    st, tau, theta, s0 = _split(rob, states)
    n, P = len(st), rob.max_points()
    F_e, L_e, f_e, l_e = _loads(n, F_e, L_e, f_e, l_e)
    routing = Routing(rob)
    out = dict(vu0=np.zeros((n, 6)), p=np.full((n, P, 3), np.nan), R=np.full((n, P, 3, 3), np.nan), n_points=np.zeros(n, np.int32),
               L=np.zeros(n), L_i=np.zeros((n, rob.n_tendons)), e=np.zeros(n), iters=np.zeros(n, np.int32), converged=np.zeros(n, bool),
               C=np.zeros(n))
    j = np.arange(6)
    for i in range(n):
        t, steps, single = state_grid(rob, s0[i])
        k = len(t)
        out["n_points"][i] = k
        x = unloaded_start(rob, tau[i], s0[i]) if guess is None else np.array(guess, float).reshape(n, 6)[i].copy()
        out["vu0"][i] = x
        if single:
            out["p"][i, 0], out["R"][i, 0] = 0.0, rotate_z(np.zeros((1, 1, 3)), np.eye(3)[None, None], theta[i:i + 1])[1][0, 0]
            out["converged"][i] = True
            continue
        iters = 0
        while True:
            d = fd_steps(x, delta)
            lanes = np.repeat(x[None, :], 13, axis=0)
            lanes[1 + 2 * j, j] -= d
            lanes[2 + 2 * j, j] += d
            sh = integrate(rob, tau[i], lanes, f_e[i], l_e[i], steps, k, routing)
            e13 = tip_residual(rob, np.tile(tau[i], (13, 1)), sh, F_e[i:i + 1], L_e[i:i + 1], routing)
            e = e13[0]
            enorm = np.linalg.norm(e)
            J = ((e13[2::2] - e13[1::2]) * (0.5 / d)[:, None]).T                       # (6 residuals, 6 strains)
            if not (enorm > tol) or iters >= max_iters or not np.isfinite(enorm):
                break
            x = x - np.linalg.solve(J, e)
            iters += 1
        dp = np.transpose((sh["p"][2::2] - sh["p"][1::2]) * (0.5 / d)[:, None, None], (1, 2, 0))   # (k, 3, 6)
        if np.isfinite(J).all() and np.isfinite(dp).all():
            Ji = np.linalg.inv(J)
            out["C"][i] = max(np.linalg.norm(dp[q] @ Ji, 2) for q in range(k))
        else:
            out["C"][i] = np.inf
        p, R = rotate_z(sh["p"][:1], sh["R"][:1], theta[i:i + 1])
        out["vu0"][i], out["p"][i, :k], out["R"][i, :k] = x, p[0], R[0]
        out["L"][i], out["L_i"][i], out["e"][i], out["iters"][i], out["converged"][i] = sh["L"][0], sh["L_i"][0], enorm, iters, enorm <= tol
    return out
