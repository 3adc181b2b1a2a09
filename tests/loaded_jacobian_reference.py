"""The loaded tip Jacobian and tip compliance in plain numpy: the specification of tr_tip_jacobian_loaded
(csrc/loaded_jacobian_host.inc, csrc/loaded_sens_kernel.hpp), built on loaded_ik_reference.linearise.

At base strains y with e_w(y, p) = balance(y, p) - w = 0 the tip x(y, p) of the loaded rod moves

    with the state   as dx/dp = J = X_p - X_y W,   W = J_y^-1 J_p
    with the wrench  as dx/dw = C = X_y J_y^-1 T   (de_w/dw = -T, so dy/dw = J_y^-1 T)

J_y = de_w/dy, J_p = de_w/dp, X_y = dx/dy, X_p = dx/dp are central differences of the 13 + 2 S lanes of one point: the strains'
steps are delta_y itself, the state's max(|1e-4 p_k|, delta) -- the loaded IK's.  T is the identity for a wrench in the frame before
the state's rotation (frame 'base'); a wrench fixed in the world frame enters the residual turned by Rz(-theta), so T =
blockdiag(Rz(-theta), Rz(-theta)) and C is the derivative with respect to the wrench as the caller gave it.  The shooting stops at
the threshold, not at the equilibrium: y_c = y - J_y^-1 e and x_c = x - X_y J_y^-1 e are one Newton step further.
"""
import numpy as np

import loaded_ik_reference as ikr

BLOCK_KEYS = ("J_y", "J_p", "X_y", "X_p")


def wrench_turn(rob, states, frame):
    """(n, 6, 6) T: d(wrench row the residual subtracts) / d(wrench as given)."""
    st = np.atleast_2d(np.asarray(states, float))
    n, N = st.shape[0], rob.n_tendons
    T = np.tile(np.eye(6), (n, 1, 1))
    if frame == "world" and rob.c.enable_rotation:
        c, s = np.cos(st[:, N]), np.sin(st[:, N])
        for h in (0, 3):                                                # Rz(-theta) = [c s 0; -s c 0; 0 0 1]
            T[:, h + 0, h + 0], T[:, h + 0, h + 1] = c, s
            T[:, h + 1, h + 0], T[:, h + 1, h + 1] = -s, c
    return T


def reduce_blocks(y, x, e, J_y, J_p, X_y, X_p, T):
    """dict(W, J, y_c, x_c, C) of the blocks of n points (np.linalg.solve; a singular J_y leaves NaN in its row)."""
    n, S = J_p.shape[0], J_p.shape[2]
    W, c, G = np.full((n, 6, S), np.nan), np.full((n, 6), np.nan), np.full((n, 6, 6), np.nan)
    with np.errstate(all="ignore"):
        for i in range(n):
            if np.isfinite(J_y[i]).all() and np.isfinite(J_p[i]).all() and np.isfinite(e[i]).all():
                try:
                    sol = np.linalg.solve(J_y[i], np.concatenate([J_p[i], e[i][:, None], T[i]], axis=1))
                    W[i], c[i], G[i] = sol[:, :S], sol[:, S], sol[:, S + 1:]
                except np.linalg.LinAlgError:
                    pass
        return dict(W=W, J=X_p - X_y @ W, y_c=y - c, x_c=x - np.einsum("nij,nj->ni", X_y, c), C=X_y @ G)


def sensitivities(rob, states, y, wrench=None, dist=None, frame="base", delta=1e-6, delta_y=1e-6, routing=None):
    """The linearisation of every row (states (n, S), strains y (n, 6)) under one load set: dict(point = (y, x, e) of lane 0, the
    blocks J_y (n, 6, 6), J_p (n, 6, S), X_y (n, 3, 6), X_p (n, 3, S), W, J (n, 3, S), y_c, x_c, C (n, 3, 6), T)."""
    st = np.atleast_2d(np.asarray(states, float))
    y = np.asarray(y, float).reshape(-1, 6)
    lin = ikr.linearise(rob, st, y, wrench=wrench, dist=dist, frame=frame, delta=delta, delta_y=delta_y, routing=routing)
    T = wrench_turn(rob, st, frame)
    out = dict(point=(y, lin["x"], lin["e"]), T=T, **{k: lin[k] for k in BLOCK_KEYS})
    out.update(reduce_blocks(y, lin["x"], lin["e"], lin["J_y"], lin["J_p"], lin["X_y"], lin["X_p"], T))
    return out


def lanes(rob, states, y, wrench=None, dist=None, frame="base", delta=1e-6, delta_y=1e-6, routing=None, strain_steps="absolute",
          turn_with="lane"):
    """(x (n, Q, 3), e (n, Q, 6), d (n, Q)) of the 13 + 2 S lanes of every row in fk_loaded_lin's order (lane 0 the point, 1 + 2j /
    2 + 2j strain j moved by -+ delta_y, 13 + 2k / 14 + 2k state entry k moved by -+ its step), with the lanes' steps d.
    Two switches state what the scheme is NOT, for the mutation tests: strain_steps='levmar' moves the strains by max(|1e-4 y_j|,
    delta_y); turn_with='state' turns a world-frame load set by the unperturbed state's rotation in every lane."""
    import loaded_fk_reference as ref
    st = np.atleast_2d(np.asarray(states, float))
    y = np.asarray(y, float).reshape(-1, 6)
    n, S = st.shape
    Q = 13 + 2 * S
    dy = np.full_like(y, delta_y) if strain_steps == "absolute" else ref.fd_steps(y, delta_y)
    dp = ref.fd_steps(st, delta)
    sl, yl = np.repeat(st[:, None, :], Q, axis=1), np.repeat(y[:, None, :], Q, axis=1)
    j, k = np.arange(6), np.arange(S)
    yl[:, 1 + 2 * j, j] -= dy
    yl[:, 2 + 2 * j, j] += dy
    sl[:, 13 + 2 * k, k] -= dp
    sl[:, 14 + 2 * k, k] += dp
    if turn_with == "state":
        w, dd = ikr.load_rows(rob, st, wrench, dist, frame)
        wrench, dist, frame = np.repeat(w, Q, axis=0), np.repeat(dd, Q, axis=0), "base"
    x, e = ikr.tips_and_residuals(rob, sl.reshape(-1, S), yl.reshape(-1, 6), wrench, dist, frame, routing)
    d = np.zeros((n, Q))
    d[:, 1:13] = np.repeat(dy, 2, axis=1)
    d[:, 13:] = np.repeat(dp, 2, axis=1)
    return x.reshape(n, Q, 3), e.reshape(n, Q, 6), d


D_FORCE, D_MOMENT, SOLVE_TOL = 1e-4, 1e-5, 1e-12      # steps of the differenced solves in N and N m; their residual in N


def differenced_solves(rob, states, wrench=None, dist=None, frame="base", delta=1e-6, tol=SOLVE_TOL):
    """What J and C mean, without the implicit-function theorem: central differences of the tips of shooting solves taken to
    |e| <= tol.  Per state the solve at the state, 2 S solves at p_k -+ max(|1e-4 p_k|, delta) and 12 at F_e -+ D_FORCE, L_e -+
    D_MOMENT (the wrench as given: in the world frame under frame='world'), each from the state's own strains.
    dict(y (n, 6) the state's strains, tip (n, 3), J (n, 3, S), C (n, 3, 6), converged (n,) all of a state's solves)."""
    import loaded_fk_reference as ref
    st = np.atleast_2d(np.asarray(states, float))
    n, S = st.shape
    w = np.broadcast_to(np.zeros(6) if wrench is None else np.asarray(wrench, float), (n, 6))
    d = np.broadcast_to(np.zeros(6) if dist is None else np.asarray(dist, float), (n, 6))

    def solve(s_rows, w_rows, d_rows, guess):
        wr, dr = ikr.load_rows(rob, s_rows, w_rows, d_rows, frame)
        with np.errstate(all="ignore"):
            out = ref.shoot(rob, s_rows, F_e=wr[:, :3], L_e=wr[:, 3:], f_e=dr[:, :3], l_e=dr[:, 3:], guess=guess, tol=tol, max_iters=20)
        return out["vu0"], np.ascontiguousarray(out["p"][:, -1]), out["converged"]

    y, tip, ok = solve(st, w, d, None)
    M = 2 * S + 12
    dp = ref.fd_steps(st, delta)
    dw = np.array([D_FORCE] * 3 + [D_MOMENT] * 3)
    sl, wl = np.repeat(st[:, None, :], M, axis=1), np.repeat(w[:, None, :], M, axis=1)
    k, j = np.arange(S), np.arange(6)
    sl[:, 2 * k, k] -= dp
    sl[:, 2 * k + 1, k] += dp
    wl[:, 2 * S + 2 * j, j] -= dw
    wl[:, 2 * S + 2 * j + 1, j] += dw
    rep = lambda a: np.repeat(a, M, axis=0)
    _, t, okl = solve(sl.reshape(-1, S), wl.reshape(-1, 6), rep(d), rep(y))
    t = t.reshape(n, M, 3)
    J = np.transpose((t[:, 1:2 * S:2] - t[:, 0:2 * S:2]) * (0.5 / dp)[:, :, None], (0, 2, 1))
    Cm = np.transpose((t[:, 2 * S + 1::2] - t[:, 2 * S::2]) * (0.5 / dw)[None, :, None], (0, 2, 1))
    return dict(y=y, tip=tip, J=J, C=Cm, converged=ok & okl.reshape(n, M).all(axis=1))


def stop_points(rob, states, y, wrench=None, dist=None, frame="base", threshold=None):
    """(n, 12, 6) strains around the equilibria y whose residual is `threshold` (default: the robot's residual_threshold) along -+
    each residual axis, to first order: y + J_y^-1 (-+ threshold e_k).  A shooting may stop anywhere with |e_w| <= threshold;
    these are the twelve axis points of that ball's surface."""
    st = np.atleast_2d(np.asarray(states, float))
    thr = rob.c.residual_threshold if threshold is None else threshold
    out = np.empty((len(st), 12, 6))
    for i in range(len(st)):
        row = lambda a: a if a is None or np.ndim(a) == 1 else np.asarray(a, float)[i]
        lin = ikr.linearise(rob, st[i:i + 1], np.asarray(y, float)[i:i + 1], wrench=row(wrench), dist=row(dist), frame=frame)
        G = np.linalg.inv(lin["J_y"][0])
        for k in range(6):
            out[i, 2 * k], out[i, 2 * k + 1] = y[i] - thr * G[:, k], y[i] + thr * G[:, k]
    return out


def unloaded_differences(rob, states, delta=1e-6):
    """(n, 3, S) central differences of the oracle's unloaded tip with levmar's steps: what Engine.tip_jacobian returns."""
    import loaded_fk_reference as ref
    st = np.atleast_2d(np.asarray(states, float))
    n, S = st.shape
    d = ref.fd_steps(st, delta)
    J = np.empty((n, 3, S))
    for i in range(n):
        for k in range(S):
            a, b = st[i].copy(), st[i].copy()
            a[k] -= d[i, k]
            b[k] += d[i, k]
            J[i, :, k] = (np.asarray(rob.shape(b)["p"][-1]) - np.asarray(rob.shape(a)["p"][-1])) * (0.5 / d[i, k])
    return J


def relative_gap(a, b):
    """(n,) max |a - b| / max |b| per leading row: the measure of every tolerance on J and C."""
    a, b = np.asarray(a), np.asarray(b)
    ax = tuple(range(1, a.ndim))
    return np.abs(a - b).max(axis=ax) / np.abs(b).max(axis=ax)


def blocks_from_lanes(x, e, d):
    """(J_y, J_p, X_y, X_p) by central differences of lanes()' arrays, with linearise's expression."""
    S = (x.shape[1] - 13) // 2
    diff = lambda a, first, cnt: np.transpose((a[:, first + 1:first + 2 * cnt:2] - a[:, first:first + 2 * cnt:2])
                                              * (0.5 / d[:, first:first + 2 * cnt:2])[:, :, None], (0, 2, 1))
    return diff(e, 1, 6), diff(e, 13, S), diff(x, 1, 6), diff(x, 13, S)
