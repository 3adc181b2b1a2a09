"""The loaded forward kinematics in plain numpy: the reference of the loaded-FK tests and fixtures.

The rod of TendonRobot::general_tension_shape: state x = (p, R, v, u, L, L_i); right-hand side tendon_deriv with the two load
terms c -= R^T l_e, d -= R^T f_e (f_e, l_e constant per problem, per unit length, in the robot's base frame); classical RK4 over
t_range(0, L, dL) from p = 0, R = I, (v, u) = (v0, u0); tip residual e = (F_e_est - F_e, L_e_est - L_e) from the force and moment
balance at s = L; Newton shooting on (v0, u0) with the central-difference Jacobian d_j = max(|1e-4 p_j|, delta).

Written from those equations; the routing r(s), r'(s), r''(s), the arc-length grid and the unloaded start come from the CPU oracle
(oracle/oracle.py: r_info, t_range, solve_initial_bending).  Everything is batched over a leading axis so a fixture's 24 states and
their 13 integrations each run as one array program.
"""
import numpy as np

E3 = np.array([0.0, 0.0, 1.0])
DBL_EPS = np.finfo(float).eps


def stiffness(rob):
    """(K_se diagonal, K_bt diagonal) of the oracle robot `rob` (get_stiffness_matrices)."""
    c = rob.c
    ro2, ri2 = c.ro * c.ro, c.ri * c.ri
    I = 0.25 * np.pi * (ro2 * ro2 - ri2 * ri2)
    Ar = np.pi * (ro2 - ri2)
    G = c.E / (2 * (1 + c.nu))
    return np.array([G * Ar, G * Ar, c.E * Ar]), np.array([c.E * I, c.E * I, 2 * I * G])


def step_list(rob):
    """[(t, h, observed point index or -1)]: integrate_times' steps of min(dL, t[j+1] - cur) while t[j+1] - cur > eps."""
    t = rob.t_range(0.0)
    dL = rob.c.dL
    steps = []
    for j in range(len(t) - 1):
        cur, tn = t[j], t[j + 1]
        first = len(steps)
        while tn - cur > DBL_EPS:
            h = min(dL, tn - cur)
            steps.append([cur, h, -1])
            cur += h
        if len(steps) == first:
            steps.append([cur, 0.0, -1])
        steps[-1][2] = j + 1
    return t, steps


class Routing:
    """r, r', r'' of every tendon at an abscissa, from the oracle, remembered per abscissa."""

    def __init__(self, rob):
        self.rob, self.memo = rob, {}

    def __call__(self, t):
        t = float(t)
        if t not in self.memo:
            self.memo[t] = self.rob.r_info(t)
        return self.memo[t]


def hat(w):
    o = np.zeros(w.shape[:-1] + (3, 3))
    o[..., 0, 1], o[..., 0, 2] = -w[..., 2], w[..., 1]
    o[..., 1, 0], o[..., 1, 2] = w[..., 2], -w[..., 0]
    o[..., 2, 0], o[..., 2, 1] = -w[..., 1], w[..., 0]
    return o


def rhs(Kse, Kbt, route, tau, R, v, u, f_e, l_e):
    """The loaded tendon_deriv for a batch: tau (B, N), R (B, 3, 3), v, u, f_e, l_e (B, 3); route = (r, r', r'') each (N, 3).
    Returns (p', R', v', u', L', L_i')."""
    r, rd, rdd = route
    uh, rh = hat(u), hat(r)
    pd = np.cross(u[:, None, :], r[None]) + rd[None] + v[:, None, :]                 # (B, N, 3)
    s = np.linalg.norm(pd, axis=-1)
    pdh = hat(pd)
    Ai = -(tau / s ** 3)[..., None, None] * (pdh @ pdh)
    Bi = rh[None] @ Ai
    Gi = -Ai @ rh[None]
    Hi = -Bi @ rh[None]
    w = np.cross(u[:, None, :], pd) + np.cross(u[:, None, :], rd[None]) + rdd[None]
    ai = (Ai @ w[..., None])[..., 0]
    bi = np.cross(r[None], ai)
    A, Bm, G, H = Ai.sum(1), Bi.sum(1), Gi.sum(1), Hi.sum(1)
    a, b = ai.sum(1), bi.sum(1)
    nb = Kse * (v - E3)                                                              # K_se (v - e3)
    Rt = np.swapaxes(R, -1, -2)
    c = -np.cross(u, Kbt * u) - np.cross(v, nb) - b - (Rt @ l_e[..., None])[..., 0]
    d = -np.cross(u, nb) - a - (Rt @ f_e[..., None])[..., 0]
    M = np.zeros((tau.shape[0], 6, 6))
    M[:, :3, :3] = np.diag(Kse) + A
    M[:, :3, 3:] = G
    M[:, 3:, :3] = Bm
    M[:, 3:, 3:] = np.diag(Kbt) + H
    xi = np.linalg.solve(M, np.concatenate([d, c], axis=1)[..., None])[..., 0]
    return (R @ v[..., None])[..., 0], R @ uh, xi[:, :3], xi[:, 3:], np.linalg.norm(v, axis=-1), s


def deriv_flat(rob, tau, x, t, f_e=None, l_e=None):
    """The right-hand side on tendon_deriv's flat state (p[0:3], R[3:12] column-major, v, u, L, L_i): what Robot.deriv computes
    at zero load."""
    x = np.asarray(x, float)
    Kse, Kbt = stiffness(rob)
    z = np.zeros((1, 3))
    R = x[3:12].reshape(3, 3).T[None]
    out = rhs(Kse, Kbt, rob.r_info(t), np.asarray(tau, float)[None], R, x[None, 12:15], x[None, 15:18],
              z if f_e is None else np.asarray(f_e, float)[None], z if l_e is None else np.asarray(l_e, float)[None])
    return np.concatenate([out[0][0], out[1][0].T.reshape(9), out[2][0], out[3][0], [out[4][0]], out[5][0]])


def integrate(rob, tau, vu0, f_e, l_e, routing=None):
    """RK4 over the grid for a batch: tau (B, N), vu0 (B, 6), f_e, l_e (B, 3).  dict(p (B, P, 3), R (B, P, 3, 3), v, u (B, 3) at
    the tip, L (B,), L_i (B, N))."""
    routing = routing or Routing(rob)
    Kse, Kbt = stiffness(rob)
    t, steps = step_list(rob)
    B, N = tau.shape
    st = [np.zeros((B, 3)), np.tile(np.eye(3), (B, 1, 1)), vu0[:, :3].copy(), vu0[:, 3:].copy(), np.zeros(B), np.zeros((B, N))]
    P = len(t)
    pts, Rs = np.zeros((B, P, 3)), np.zeros((B, P, 3, 3))
    pts[:, 0], Rs[:, 0] = st[0], st[1]

    def f(x, tt):
        return rhs(Kse, Kbt, routing(tt), tau, x[1], x[2], x[3], f_e, l_e)

    def axpy(x, a, k):
        return [xi + a * ki for xi, ki in zip(x, k)]

    for cur, h, obs in steps:
        k1 = f(st, cur)
        k2 = f(axpy(st, h * 0.5, k1), cur + h * 0.5)
        k3 = f(axpy(st, h * 0.5, k2), cur + h * 0.5)
        k4 = f(axpy(st, h, k3), cur + h)
        b1, b2 = h * (1.0 / 6.0), h * (1.0 / 3.0)
        st = [x + b1 * a + b2 * b + b2 * c + b1 * d for x, a, b, c, d in zip(st, k1, k2, k3, k4)]
        if obs >= 0:
            pts[:, obs], Rs[:, obs] = st[0], st[1]
    return dict(p=pts, R=Rs, v=st[2], u=st[3], L=st[4], L_i=st[5])


def tip_residual(rob, tau, sh, F_e, L_e, routing=None):
    """e = (F_e_est - F_e, L_e_est - L_e) (B, 6) of integrate()'s result: PointForces::calc_point_forces at s = L, base frame."""
    routing = routing or Routing(rob)
    Kse, Kbt = stiffness(rob)
    r, rd, _ = routing(rob.c.L)
    R, v, u = sh["R"][:, -1], sh["v"], sh["u"]
    n = (R @ (Kse * (v - E3))[..., None])[..., 0]
    m = (R @ (Kbt * u)[..., None])[..., 0]
    pd = np.cross(u[:, None, :], r[None]) + rd[None] + v[:, None, :]                 # (B, N, 3)
    pdw = np.einsum("bij,bnj->bni", R, pd)
    unit = pdw / np.linalg.norm(pdw, axis=-1, keepdims=True)
    Fti = -tau[..., None] * unit
    Lti = np.cross(np.einsum("bij,nj->bni", R, r), Fti)
    return np.concatenate([n - Fti.sum(1) - F_e, m - Lti.sum(1) - L_e], axis=1)


def fd_steps(x, delta=1e-6):
    return np.maximum(np.abs(1e-4 * x), delta)


def unloaded_start(rob, tau):
    out = np.zeros((len(tau), 6))
    for i, tq in enumerate(tau):
        v, u, _ = rob.solve_initial_bending(tq)
        out[i, :3], out[i, 3:] = v, u
    return out


def rotate_z(p, R, theta):
    """TendonResult::rotate_z for a batch: p (B, P, 3), R (B, P, 3, 3), theta (B,)."""
    c, s = np.cos(theta), np.sin(theta)
    Rz = np.zeros((len(theta), 3, 3))
    Rz[:, 0, 0], Rz[:, 0, 1], Rz[:, 1, 0], Rz[:, 1, 1], Rz[:, 2, 2] = c, -s, s, c, 1.0
    return np.einsum("bij,bpj->bpi", Rz, p), np.einsum("bij,bpjk->bpik", Rz, R)


def shoot(rob, states, F_e=None, L_e=None, f_e=None, l_e=None, guess=None, tol=1e-11, max_iters=10, delta=1e-6):
    """Newton shooting for a batch of states (n, S) of a robot without retraction; loads (n, 3) or (3,) or None (zero), in the
    frame before the state's rotation.  Start: `guess` (n, 6) rows (v, u), or the unloaded solution of the tensions.
    Stops a problem at |e| <= tol or after max_iters Newton steps.
    dict(vu0 (n, 6), p (n, P, 3) and R (n, P, 3, 3) after rotate_z, L, L_i, e (n,) = |e|, iters, converged,
         C (n,) = max over the backbone points of |dp/d(v0, u0) J^-1|_2 in m/N, from the last Jacobian's integrations)."""
    st = np.atleast_2d(np.asarray(states, float))
    n, N = st.shape[0], rob.n_tendons
    assert not rob.c.enable_retraction
    tau = np.ascontiguousarray(st[:, :N])
    theta = st[:, N].copy() if rob.c.enable_rotation else np.zeros(n)

    def rows(a):
        return np.zeros((n, 3)) if a is None else np.broadcast_to(np.asarray(a, float), (n, 3)).copy()

    F_e, L_e, f_e, l_e = rows(F_e), rows(L_e), rows(f_e), rows(l_e)
    routing = Routing(rob)
    x = unloaded_start(rob, tau) if guess is None else np.array(guess, float).reshape(n, 6)
    iters = np.zeros(n, dtype=np.int32)
    done = np.zeros(n, dtype=bool)
    rep = lambda a: np.repeat(a, 13, axis=0)
    while True:
        d = fd_steps(x, delta)                                       # (n, 6)
        lanes = np.repeat(x[:, None, :], 13, axis=1)                 # trial, then -d_j, +d_j
        j = np.arange(6)
        lanes[:, 1 + 2 * j, j] -= d
        lanes[:, 2 + 2 * j, j] += d
        sh = integrate(rob, rep(tau), lanes.reshape(-1, 6), rep(f_e), rep(l_e), routing)
        e13 = tip_residual(rob, rep(tau), sh, rep(F_e), rep(L_e), routing).reshape(n, 13, 6)
        e = e13[:, 0]
        enorm = np.linalg.norm(e, axis=1)
        J = np.transpose((e13[:, 2::2] - e13[:, 1::2]) * (0.5 / d)[:, :, None], (0, 2, 1))    # (n, 6 residuals, 6 strains)
        done |= ~(enorm > tol) | (iters >= max_iters) | ~np.isfinite(enorm)
        if done.all():
            break
        step = np.linalg.solve(J[~done], e[~done][..., None])[..., 0]
        x[~done] -= step
        iters[~done] += 1
    P = sh["p"].shape[1]
    p13 = sh["p"].reshape(n, 13, P, 3)
    dp = np.transpose((p13[:, 2::2] - p13[:, 1::2]) * (0.5 / d)[:, :, None, None], (0, 2, 3, 1))   # (n, P, 3, 6)
    C = np.zeros(n)
    for i in range(n):
        if np.isfinite(J[i]).all() and np.isfinite(dp[i]).all():
            C[i] = max(np.linalg.norm(dp[i, q] @ np.linalg.inv(J[i]), 2) for q in range(P))
        else:
            C[i] = np.inf
    sel = lambda a: a.reshape((n, 13) + a.shape[1:])[:, 0]
    p, R = rotate_z(sel(sh["p"]), sel(sh["R"]), theta)
    return dict(vu0=x, p=p, R=R, L=sel(sh["L"]), L_i=sel(sh["L_i"]), e=enorm, iters=iters, converged=enorm <= tol, C=C)


def evaluate(rob, states, vu0, F_e=None, L_e=None, f_e=None, l_e=None):
    """One integration per state from given base strains: dict(p, R after rotate_z, L, L_i, e (n, 6), vuL (n, 6) the tip strains)."""
    st = np.atleast_2d(np.asarray(states, float))
    n, N = st.shape[0], rob.n_tendons
    tau = np.ascontiguousarray(st[:, :N])
    theta = st[:, N].copy() if rob.c.enable_rotation else np.zeros(n)
    rows = lambda a: np.zeros((n, 3)) if a is None else np.broadcast_to(np.asarray(a, float), (n, 3)).copy()
    routing = Routing(rob)
    sh = integrate(rob, tau, np.asarray(vu0, float).reshape(n, 6), rows(f_e), rows(l_e), routing)
    e = tip_residual(rob, tau, sh, rows(F_e), rows(L_e), routing)
    p, R = rotate_z(sh["p"], sh["R"], theta)
    return dict(p=p, R=R, L=sh["L"], L_i=sh["L_i"], e=e, vuL=np.concatenate([sh["v"], sh["u"]], axis=1))
