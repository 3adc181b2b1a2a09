"""An extended-precision reference for ONE Levenberg-Marquardt iteration of the device tip IK (ik_lm_step<S>, csrc/ik_kernel.hpp,
with csrc/lm_dense.hpp), and the harness that holds every iteration of a run to it.  CPU only: numpy and mpmath at 40 digits.

What makes the iteration observable.  `max_iters = k` ends a problem after its k-th trial point has been evaluated and accepted or
rejected, and a problem's iterates do not depend on the batch, so the calls with max_iters = 0 .. K return the whole sequence p_k,
f(p_k), sqrt(err2_k), iters, num_fk_calls.  From call k to call k + 1:
    iters equal                                          stopped at or before k
    iters + 1, num_fk_calls equal                        stop on the small step (or on a matrix that is not positive definite)
    iters + 1, num_fk_calls + (2 S + 1), state changed   trial accepted
    iters + 1, num_fk_calls + (2 S + 1), state equal     trial rejected
Only mu and nu are hidden; they follow from mu_0 = mu_init max diag(J^T J) and the observed decisions (replay).

    truth_step      the step from float64 inputs taken as exact, at 40 digits, with its stop tests, kappa_2 and the bound below
    replay          walks K + 1 results, carries mu and nu, returns one record per (problem, step)
    float64_scheme  ik_lm_step's operations in its order in Python floats (no contraction), with an FK function like
                    inverse_kinematics_batch(fk=...); `variant` switches on exactly one deliberate error

The bound on an accepted trial x = clip(p + y), (J^T J + mu I) y = g, g = J^T (des - f).  u = 2^-53, gamma_k = k u to first order.
  1. Cholesky solve.  The computed y solves (A^ + dA) y = g^ with |dA| <= gamma_{3S+1} |R^T| |R| (Higham, Accuracy and Stability of
     Numerical Algorithms, 2nd ed., Theorem 10.4) and || |R^T| |R| ||_2 <= S ||A||_2 (ibid. eq. 10.7): ||dA||_2 <= S (3S+1) u ||A||_2.
  2. Forming A.  An entry is three products and three sums, mu (or 0.0, exactly) added last: |A^ - A| <= gamma_4 (|J|^T |J| + mu I),
     and || |J|^T |J| ||_2 <= ||J||_F^2 <= 3 ||J||_2^2 because J has three rows: at most 3 gamma_4 ||A||_2 = 12 u ||A||_2.
  3. Forming g.  e = des - f is one rounding, a component of g three products and two sums: |g^ - g| <= gamma_4 |J|^T |e|.  With
     chi = || |J|^T |e| ||_2 / ||g||_2 >= 1 (the cancellation in J^T e, large where the residual is nearly orthogonal to the range of
     J) and ||g||_2 <= ||A||_2 ||y||_2 this is ||A^-1 dg||_2 <= 4 chi u kappa_2 ||y||_2.
  First order: ||y^ - y||_2 <= (c_S + 4 chi) u kappa_2(A) ||y||_2 with c_S = S (3S + 1) + 12, i.e. 16, 42, 64, 92, 126, 166, 212, 264,
  322 for S = 1, 3, 4 .. 10 (26 at S = 2).
  Scaled form.  Both perturbations are componentwise small against d d^T, d_j = A_jj^1/2: |R^T| |R| <= d d^T (Cauchy-Schwarz on the
  rows of R; Higham, section 10.1), (|J|^T |J|)_ab <= d_a d_b, mu <= d_a^2.  With D = diag(d) and H = D^-1 A D^-1 (unit diagonal):
  ||D^-1 dA D^-1||_2 <= (S (3S+1) + 4 S) u, so ||D (y^ - y)||_2 <= ||H^-1||_2 ((S (3S+1) + 4 S) ||D y||_2 + 4 || D^-1 |J|^T |e| ||_2) u
  and |y^_j - y_j| <= ||D (y^ - y)||_2 / d_j.  This is the same analysis in other units, it holds whenever the first form does, and
  the smaller of the two is the bound.  It matters where one column of J is out of scale: on the device the retraction column at
  the face s_start = 0 is about L / 2e-6, because the central difference there asks the FK for s_start = -1e-6, which it returns as a
  one-point backbone; kappa_2(A) is then 3e11 and kappa_2(H) what it was.
  4. mu.  The kernel's mu differs from the replayed one by the roundings of its own recurrence.  mu ||A^-1||_2 <= 1, so a relative
     error r in mu moves y by at most r ||y||_2.  r is carried by replay: 4 u for mu_0 (gamma_3 in a diagonal entry, one product), 2 u
     per accept on the 1/3 floor, and where 1 - cube is the factor the roundings of pred (its own, gamma_{3S+4} on the sum of its
     terms' magnitudes, and those of g, 4 u |dp| . |J|^T |e|), rho, t, the cube and the difference through the derivative
     6 t^2 rho / (1 - cube); a reject scales by a power of two and adds nothing.  The recurrence feeds on itself there: pred holds
     mu |dp|^2, so the r already carried is multiplied by 1 + (6 t^2 rho / (1 - cube)) (mu |dp|^2 / pred), up to about 8 near
     rho = 0.9.  A run of accepts with rho between 0.5 and 0.94 therefore ends gated; on the 1/3 floor r only adds.
  5. p + y is one rounding (half an ulp), the clip none.  The state comes back with its rotation canonical (lm_write_result), whose
     two additions round at magnitudes up to 4 pi; replay reconstructs the kernel's own rotation entry (below) wherever it can, and
     where it cannot the comparison is modulo 2 pi and that rounding, at most 2 ulp(2 pi), is inside this term.  Two ulps of x per
     component (ulp(2 pi) for a rotation compared modulo 2 pi).
None of this is fitted to the implementation.  For orientation only: LAPACK's solve lies at 0.2 to 1.5 u kappa_2 relative.

The rotation entry.  Its box is +-DBL_MAX and the result holds canonical_angle(p_rot), which rounds to a grid of 2^-49: the returned
state is not the point the kernel differentiates at, and the tips of Engine.tip_jacobian(returned state) are not the IK's.  The
kernel's own entry is fl(p_rot + y_rot).  replay forms y_rot with the float64 restatement (f64_step) from the same J, f and a float64
mu carried beside the mpmath one, and takes the double nearest to that candidate whose canonical angle is the returned entry bit
for bit AND whose tip is the IK's bit for bit (_recover_rotation: the candidate itself where it qualifies, else a search of the
grid cell through the FK; the device's pow(t, 3.0) is not glibc's to the last bit, and the recurrence of mu amplifies one ulp, so
the candidate alone does not always hold).  The next step's tips, which must again equal the IK's bit for bit, confirm it.  The
starts' rotation lies in (-pi, pi), so the first point is exact.  Because the entry is known through the grid, the rotation's share
of the two-ulp term is always 2 ulp(2 pi).  Where the search finds several members of the cell with the IK's tip (a small angle:
one ulp of it moves the tip by less than an ulp), the point is not pinned: the perturbed tips, and so J's rotation column, differ
between the members at 1e-17 m / 2e-6, four orders above c_S u.  For the steps from such a point the bound carries that
uncertainty of J: two ulps in each perturbed tip, dJ_kj = 2 ulp(|f_k| + |J_kj| d_j) / d_j, through dA = dJ^T J + J^T dJ and dg = dJ^T e.

Gating.  A step whose bound exceeds 1e-3 ||y|| cannot tell a 0.1 % error in the step: it is counted, not judged.  A decision is gated
when |err2 - err2n| lies within 2 bound ||J||_2 (||e|| + ||e_n||), the change of err2n that an error of `bound` in x implies; the
small-step test when | |dp| - eps2 |p| | <= bound; the gradient test when its margin is within gamma_4 || |J|^T |e| ||_inf.  No case
may have more than 10 % of its steps gated.  A step that ends on the small-step test evaluates no trial, so there is no error to
judge and only its decision can be gated (after a run of rejections mu is huge, |y| about 1e-12, and two ulps exceed 1e-3 |y|).

Stops no finite input reaches here: mu overflow needs about 1000 consecutive rejections of nu = 2^k (mu >= 1e300), and a matrix
that is not positive definite needs mu = inf or a NaN in J.  Neither is constructed.
"""
import math

import mpmath as mp
import numpy as np

DPS = 40
U = 2.0 ** -53
VARIANTS = ("no_floor", "nu_not_reset", "reject_times_2", "pred_without_mu", "undamped_entry", "unclipped", "J_refreshed_on_reject",
            "small_on_y")
KEYS = ("state", "tip", "error", "iters", "num_fk_calls")


def c_S(S):
    return S * (3 * S + 1) + 12


def c_S_scaled(S):
    return S * (3 * S + 1) + 4 * S


def canonical_angle(v):
    """lm_dense.hpp's, in its operation order"""
    pi = 3.141592653589793
    two_pi = 2.0 * pi
    return math.fmod(math.fmod(v + pi, two_pi) + two_pi, two_pi) - pi


def eval_fk(fk, P, delta):
    """f(p) (n, 3) and the central-difference J(p) (n, 3, S) of the rows of P in ik_expand's / ik_f_and_J's operations.
    fk: states (m, S) -> tips (m, 3) through tip_control's FK wrapper."""
    P = np.asarray(P, float)
    n, S = P.shape
    d = np.maximum(np.abs(1e-4 * P), delta)
    batch = np.repeat(P[:, None, :], 2 * S + 1, axis=1)
    j = np.arange(S)
    batch[:, 1 + 2 * j, j] -= d
    batch[:, 2 + 2 * j, j] += d
    tips = np.asarray(fk(batch.reshape(-1, S)), float).reshape(n, 2 * S + 1, 3)
    J = (tips[:, 2::2, :] - tips[:, 1::2, :]) * (0.5 / d)[:, :, None]
    return tips[:, 0, :].copy(), np.ascontiguousarray(np.transpose(J, (0, 2, 1)))


# ---- the float64 restatement: Python floats, one rounding per operation, the kernel's order ---------------------------------------
def f64_err(des, f):
    e = [float(des[k]) - float(f[k]) for k in range(3)]
    return e, e[0] * e[0] + e[1] * e[1] + e[2] * e[2]


def f64_grad(J, e):
    S = len(J[0])
    return [J[0][j] * e[0] + J[1][j] * e[1] + J[2][j] * e[2] for j in range(S)]


def f64_mu0(J, mu_init):
    S = len(J[0])
    dmax = 0.0
    for j in range(S):
        a = J[0][j] * J[0][j] + J[1][j] * J[1][j] + J[2][j] * J[2][j]
        if not a <= dmax:
            dmax = a
    mu = mu_init * dmax
    return mu if mu > 0.0 else mu_init


def f64_moving(p, g, lo, hi, eps1):
    mx = 0.0
    for j in range(len(p)):
        blocked = (p[j] <= lo[j] and g[j] < 0.0) or (p[j] >= hi[j] and g[j] > 0.0)
        a = 0.0 if blocked else abs(g[j])
        if not a <= mx:
            mx = a
    return mx > eps1


def f64_chol_solve(A, g):
    """chol_solve_packed"""
    S = len(g)
    A = list(A)
    T = lambda a, b: a * (a + 1) // 2 + b
    spd = True
    for a in range(S):
        for b in range(a + 1):
            s = A[T(a, b)]
            for k in range(b):
                s -= A[T(a, k)] * A[T(b, k)]
            if a == b:
                spd = spd and s > 0.0
                A[T(a, a)] = math.sqrt(s if s > 0.0 else 1.0)
            else:
                A[T(a, b)] = s / A[T(b, b)]
    y = [0.0] * S
    for a in range(S):
        s = g[a]
        for k in range(a):
            s -= A[T(a, k)] * y[k]
        y[a] = s / A[T(a, a)]
    for a in range(S - 1, -1, -1):
        s = y[a]
        for k in range(a + 1, S):
            s -= A[T(k, a)] * y[k]
        y[a] = s / A[T(a, a)]
    return spd, y


def _clip(x, lo, hi):
    v = lo if x < lo else x
    return hi if v > hi else v


def f64_step(p, J, g, mu, lo, hi, variant=None):
    """the damped step of ik_lm_step from p: (x, y, spd, dd, pp)"""
    S = len(p)
    A = []
    for a in range(S):
        for b in range(a + 1):
            damp = mu if a == b else 0.0
            if variant == "undamped_entry" and a == b == S - 1:
                damp = 0.0
            A.append(J[0][a] * J[0][b] + J[1][a] * J[1][b] + J[2][a] * J[2][b] + damp)
    spd, y = f64_chol_solve(A, g)
    x, dd, pp = [], 0.0, 0.0
    for j in range(S):
        pn = p[j] + y[j] if variant == "unclipped" else _clip(p[j] + y[j], lo[j], hi[j])
        dpe = y[j] if variant == "small_on_y" else pn - p[j]
        dd += dpe * dpe
        pp += p[j] * p[j]
        x.append(pn)
    return x, y, spd, dd, pp


def f64_gain_ratio(x, p, g, mu, err2, err2n, variant=None):
    pred = 0.0
    for j in range(len(p)):
        dp = x[j] - p[j]
        pred += dp * g[j] if variant == "pred_without_mu" else dp * (mu * dp + g[j])
    return (err2 - err2n) / pred if pred > 0.0 else -1.0


def f64_shrink(rho, variant=None):
    t = 2.0 * rho - 1.0
    sh = 1.0 - math.pow(t, 3.0)
    if variant == "no_floor":
        return sh
    return (1.0 / 3.0) if (1.0 / 3.0) > sh else sh


def float64_scheme(fk, start, des, lo, hi, max_iters, mu_init=0.1, eps1=1e-9, eps2=1e-4, eps3=1e-4, delta=1e-6, rot_index=-1,
                   variant=None):
    """tr_ik_batch in Python floats.  Returns the results of the calls max_iters = 0 .. max_iters (a list of dicts of KEYS, plus
    p_internal: the state before the rotation is made canonical), taken from ONE run: the state after round k is what the call
    with max_iters = k returns."""
    start = np.asarray(start, float)
    n, S = start.shape
    Q = 2 * S + 1
    des = np.broadcast_to(np.asarray(des, float), (n, 3))
    lo, hi = [float(v) for v in lo], [float(v) for v in hi]
    eps2_sq, eps3_sq = eps2 * eps2, eps3 * eps3
    pn = [[_clip(float(start[i, j]), lo[j], hi[j]) for j in range(S)] for i in range(n)]
    P, F, JJ, G = [None] * n, [None] * n, [None] * n, [None] * n
    err2, mu, nu = [0.0] * n, [0.0] * n, [2.0] * n
    iters, calls = [0] * n, [0] * n
    active = list(range(n))
    out = []
    for rnd in range(max_iters + 1):
        if active:
            fn_all, Jn_all = eval_fk(fk, np.array([pn[i] for i in active]), delta)
        nxt = []
        for r, i in enumerate(active):
            fn, Jn = [float(v) for v in fn_all[r]], [[float(v) for v in row] for row in Jn_all[r]]
            en, err2n = f64_err(des[i], fn)
            calls[i] += Q
            if rnd == 0:
                accepted = True
                P[i], F[i], JJ[i], err2[i] = pn[i], fn, Jn, err2n
                G[i] = f64_grad(Jn, en)
                mu[i] = f64_mu0(Jn, mu_init)
                alive = err2n > eps3_sq and f64_moving(P[i], G[i], lo, hi, eps1)
            else:
                rho = f64_gain_ratio(pn[i], P[i], G[i], mu[i], err2[i], err2n, variant)
                accepted = rho > 0.0
                if accepted:
                    P[i], F[i], JJ[i], err2[i] = pn[i], fn, Jn, err2n
                    G[i] = f64_grad(Jn, en)
                    mu[i] *= f64_shrink(rho, variant)
                    if variant != "nu_not_reset":
                        nu[i] = 2.0
                    alive = err2n > eps3_sq and f64_moving(P[i], G[i], lo, hi, eps1)
                else:
                    if variant == "J_refreshed_on_reject":
                        JJ[i] = Jn
                        G[i] = f64_grad(Jn, f64_err(des[i], F[i])[0])
                    mu[i] *= 2.0 if variant == "reject_times_2" else nu[i]
                    nu[i] *= 2.0
                    alive = math.isfinite(mu[i]) and mu[i] < 1e300
            if alive:
                nxt.append(i)
        out.append(_snapshot(P, F, err2, iters, calls, rot_index))
        active = []
        if rnd == max_iters:
            break
        for i in nxt:
            x, y, spd, dd, pp = f64_step(P[i], JJ[i], G[i], mu[i], lo, hi, variant)
            iters[i] += 1
            if spd and not dd <= eps2_sq * pp:
                pn[i] = x
                active.append(i)
    return out


def _snapshot(P, F, err2, iters, calls, rot_index):
    p = np.array(P, float)
    state = p.copy()
    if rot_index >= 0:
        state[:, rot_index] = [canonical_angle(v) for v in p[:, rot_index]]
    return dict(state=state, tip=np.array(F, float), error=np.sqrt(np.array(err2)), iters=np.array(iters, dtype=np.int32),
                num_fk_calls=np.array(calls, dtype=np.int32), p_internal=p)


# ---- the truth ---------------------------------------------------------------------------------------------------------------------
def _mp_solve(A, b):
    """Gaussian elimination on a symmetric positive definite matrix of mpf (no pivoting needed)"""
    S = len(b)
    A = [row[:] for row in A]
    b = b[:]
    for c in range(S):
        for a in range(c + 1, S):
            l = A[a][c] / A[c][c]
            if l:
                for k in range(c, S):
                    A[a][k] -= l * A[c][k]
                b[a] -= l * b[c]
    for a in range(S - 1, -1, -1):
        s = b[a]
        for k in range(a + 1, S):
            s -= A[a][k] * b[k]
        b[a] = s / A[a][a]
    return b


def truth_step(p, f, J, des, mu, lo, hi, eps1=1e-9, eps2_sq=1e-8, eps3_sq=1e-8, mu_rel=0.0, mod_2pi_index=-1, dJ=None):
    """The iteration from p at 40 digits; p, f, J, des, lo, hi: float64 taken as exact, mu: mpf.  dict(g, y, x, dd, pp, err2,
    stop_err, stop_grad, grad_margin, small, small_margin, clipped, kappa, chi, ynorm, normJ, bound)."""
    with mp.workdps(DPS):
        S = len(p)
        M = mp.mpf
        Jm = [[M(float(J[k][j])) for j in range(S)] for k in range(3)]
        pm = [M(float(v)) for v in p]
        e = [M(float(des[k])) - M(float(f[k])) for k in range(3)]
        err2 = e[0] * e[0] + e[1] * e[1] + e[2] * e[2]
        g = [Jm[0][j] * e[0] + Jm[1][j] * e[1] + Jm[2][j] * e[2] for j in range(S)]
        A = [[Jm[0][a] * Jm[0][b] + Jm[1][a] * Jm[1][b] + Jm[2][a] * Jm[2][b] + (mu if a == b else 0) for b in range(S)] for a in range(S)]
        y = _mp_solve(A, g)
        x, clipped = [], []
        for j in range(S):
            v = pm[j] + y[j]
            l, h = M(float(lo[j])), M(float(hi[j]))
            c = l if v < l else (h if v > h else v)
            clipped.append(c != v)
            x.append(c)
        dd = sum(((x[j] - pm[j]) ** 2 for j in range(S)), M(0))
        pp = sum((pm[j] ** 2 for j in range(S)), M(0))
        free = M(0)
        for j in range(S):
            blocked = (pm[j] <= M(float(lo[j])) and g[j] < 0) or (pm[j] >= M(float(hi[j])) and g[j] > 0)
            if not blocked and abs(g[j]) > free:
                free = abs(g[j])
        Jf = np.asarray(J, float)
        Af = Jf.T @ Jf + float(mu) * np.eye(S)
        sv = np.linalg.svd(Af, compute_uv=False)
        kappa = float(sv[0] / sv[-1]) if sv[-1] > 0 else math.inf
        ynorm = float(mp.sqrt(sum((v * v for v in y), M(0))))
        gnorm = float(mp.sqrt(sum((v * v for v in g), M(0))))
        ef = np.array([float(v) for v in e])
        absg = np.abs(Jf).T @ np.abs(ef)
        chi = float(np.linalg.norm(absg) / gnorm) if gnorm > 0 else math.inf
        xf = np.array([float(v) for v in x])
        ulps = np.spacing(np.abs(xf))
        if mod_2pi_index >= 0:
            ulps[mod_2pi_index] = np.spacing(2 * np.pi)
        solve = (c_S(S) + 4 * chi) * U * kappa * ynorm
        # the same analysis on H = D^-1 A D^-1, D = diag(A)^1/2 (see the docstring): never weaker, taken where it is the smaller
        dg = np.sqrt(np.diag(Af))
        yf = np.array([float(v) for v in y])
        if (dg > 0).all() and np.isfinite(dg).all():
            H = Af / np.outer(dg, dg)
            svH = np.linalg.svd(H, compute_uv=False)
            if svH[-1] > 0:
                Dd = (c_S_scaled(S) * float(np.linalg.norm(dg * yf)) + 4 * float(np.linalg.norm(absg / dg))) * U / float(svH[-1])
                solve = min(solve, Dd * float(np.linalg.norm(1.0 / dg)))
        if dJ is not None:        # J known only to dJ (an unpinned rotation entry): dA = dJ^T J + J^T dJ, dg = dJ^T e, first order
            nJ, ndJ = float(np.linalg.norm(Jf, 2)), float(np.linalg.norm(dJ))
            solve += (ndJ * float(np.linalg.norm(ef)) + 2 * nJ * ndJ * ynorm) / float(sv[-1])
        bound = solve + mu_rel * ynorm + 2 * float(np.linalg.norm(ulps))
        return dict(g=g, y=y, x=x, dd=dd, pp=pp, err2=err2, stop_err=not err2 > M(eps3_sq), stop_grad=not free > M(eps1),
                    grad_margin=abs(float(free) - eps1), grad_tol=4 * U * float(np.abs(absg).max()),
                    small=dd <= M(eps2_sq) * pp, small_margin=abs(float(mp.sqrt(dd)) - math.sqrt(eps2_sq) * float(mp.sqrt(pp))),
                    clipped=any(clipped), kappa=kappa, chi=chi, absg=absg, ynorm=ynorm, normJ=float(np.linalg.norm(Jf, 2)), bound=bound)


def _pred(x, p, g, mu):
    """dp . (mu dp + g) at 40 digits, and the sum of the terms' magnitudes"""
    s, a = mp.mpf(0), mp.mpf(0)
    for j in range(len(p)):
        dp = x[j] - mp.mpf(float(p[j]))
        t = dp * (mu * dp + g[j])
        s += t
        a += abs(t)
    return s, a


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float64).view(np.uint64), np.ascontiguousarray(b, dtype=np.float64).view(np.uint64))


def _rotation_entry(cand, out):
    """the double nearest to cand whose canonical angle is `out` bit for bit, or None"""
    for j in range(17):
        for w in ((cand,) if j == 0 else (cand + j * math.ulp(cand), cand - j * math.ulp(cand))):
            if _same_bits([canonical_angle(w)], [out]):
                return w
    return None


def _np_canonical(v):
    pi = 3.141592653589793
    two_pi = 2.0 * pi
    return np.fmod(np.fmod(v + pi, two_pi) + two_pi, two_pi) - pi


def _cell(base, out, cap=1 << 16):
    """every double near `base` whose canonical angle is `out` bit for bit (at most 2 cap of them)"""
    for n in (64, 1024, cap):
        w = (np.array([base]).view(np.int64) + np.arange(-n, n + 1)).view(np.float64)
        ok = _np_canonical(w).view(np.uint64) == np.array([out]).view(np.uint64)
        if ok.any() and not ok[0] and not ok[-1]:
            break
    return w[ok]


def _recover_rotation(x_out, cand, tip, fk, rot, always=False):
    """The kernel's own rotation entry of an accepted point: x_out is the returned state (rotation canonical), cand the float64
    restatement's entry, tip the IK's tip there.  The doubles whose canonical angle is the returned entry form a cell of the
    2^-49 grid; the FK tells them apart: the entry is the member nearest to cand whose tip is the IK's bit for bit.  Without an FK
    the nearest member is taken.  Returns (entry, pinned by the tips)."""
    out = float(x_out[rot])
    base = out + 2 * math.pi * round((cand - out) / (2 * math.pi))
    w = _rotation_entry(cand, out)
    if fk is None:
        return (w, False) if w is not None else (base, False)
    if w is not None:
        x = np.array(x_out, float)
        x[rot] = w
        if not always and _same_bits(np.asarray(fk(x[None]))[0], tip):
            return w, True
    cell = _cell(base, out)
    if cell.size == 0:
        return base, False
    X = np.repeat(np.array(x_out, float)[None], cell.size, axis=0)
    X[:, rot] = cell
    tips = np.ascontiguousarray(np.asarray(fk(X), float))
    hit = (tips.view(np.uint64) == _bits3(tip)).all(1)
    if not hit.any():
        return (w if w is not None else base), False
    cell = cell[hit]
    return float(cell[np.argmin(np.abs(cell - cand))]), (True if cell.size == 1 else "ambiguous")


def _bits3(t):
    return np.ascontiguousarray(t, dtype=np.float64).view(np.uint64)


def replay(calls, jac, start, des, lo, hi, mu_init=0.1, eps1=1e-9, eps2=1e-4, eps3=1e-4, rot_index=-1, fk=None, search_cell=False,
           delta=1e-6):
    """Walk the results `calls` of max_iters = 0 .. K.  jac: states (n, S) -> (J (n, 3, S), f (n, 3)), the kernel's own at those
    states; fk: states -> tips through the wrapper, for the truth's trial of a rejected step (None: that decision is not judged).
    search_cell: always search the rotation's grid cell through fk (cheap on the device), so that a point counts as pinned only
    if no other member of the cell has the IK's tip.
    Returns (records, p_internal): one dict per (problem, step) with problem, step, kind ('accepted', 'rejected', 'small',
    'stopped'), stop (the truth's: 'err', 'grad', 'mu', 'small' or None), err, bound, ratio, ynorm, rho, nu, clipped, kappa, gated
    (the step's error is not judged), decision_gated, ok (the observed kind is the truth's, or gated), tips_equal (jac's f at the
    reconstructed point equals the call's tip bit for bit), exact_point (the rotation entry was reconstructed); p_internal
    (K + 1, n, S) the reconstructed points."""
    K = len(calls) - 1
    start = np.asarray(start, float)
    n, S = start.shape
    Q = 2 * S + 1
    des = np.broadcast_to(np.asarray(des, float), (n, 3))
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    eps2_sq, eps3_sq = eps2 * eps2, eps3 * eps3
    p_int = np.clip(start, lo, hi)
    track = [p_int.copy()]
    mu, mu64, nu, mu_rel = [None] * n, [0.0] * n, [2.0] * n, [4 * U] * n
    last = ["accept"] * n                    # what the truth's stop tests follow: an accept (or the start), or a reject
    done = [False] * n
    exact = [True] * n
    ambiguous = [False] * n                  # several members of the rotation's grid cell have the IK's tip: J is not known to be the kernel's
    records = []
    with mp.workdps(DPS):
        for k in range(K):
            a, b = calls[k], calls[k + 1]
            J_all, f_all = jac(p_int)
            pending = []                     # rejected steps whose truth's trial still needs its FK
            nxt = p_int.copy()
            for i in range(n):
                J, f = J_all[i], a["tip"][i]
                tips_equal = _same_bits(f_all[i], f)
                di, dc = int(b["iters"][i]) - int(a["iters"][i]), int(b["num_fk_calls"][i]) - int(a["num_fk_calls"][i])
                changed = not _same_bits(a["state"][i], b["state"][i])
                if di == 0 and dc == 0:
                    kind = "stopped"
                elif di == 1 and dc == 0:
                    kind = "small"
                elif di == 1 and dc == Q:
                    kind = "accepted" if changed else "rejected"
                else:
                    kind = "invalid"
                if done[i]:
                    assert kind == "stopped" and not changed, ("a stopped problem went on", i, k, kind)
                    continue
                Jl = [[float(v) for v in row] for row in J]
                e64, err2_64 = f64_err(des[i], f)
                g64 = f64_grad(Jl, e64)
                if k == 0:
                    mu64[i] = f64_mu0(Jl, mu_init)
                    d = max(sum(mp.mpf(Jl[r][j]) ** 2 for r in range(3)) for j in range(S))
                    mu[i] = mp.mpf(mu_init) * d if d > 0 else mp.mpf(mu_init)
                mod = rot_index                # the rotation entry is known through its canonical angle: ulp(2 pi) in the two-ulp term
                dJ = None
                if ambiguous[i]:              # each perturbed tip known to two ulps: an entry of J to 2 * 2 ulp * 0.5 / d
                    dstep = np.maximum(np.abs(1e-4 * p_int[i]), delta)
                    dJ = 2 * np.spacing(np.abs(np.asarray(f, float))[:, None] + np.abs(np.asarray(J, float)) * dstep[None, :]) / dstep[None, :]
                t = truth_step(p_int[i], f, J, des[i], mu[i], lo, hi, eps1, eps2_sq, eps3_sq, mu_rel[i], mod, dJ)
                rec = dict(problem=i, step=k, kind=kind, stop=None, err=None, bound=t["bound"], ratio=None, ynorm=t["ynorm"], rho=None,
                           nu=nu[i], clipped=t["clipped"], kappa=t["kappa"], gated=t["bound"] > 1e-3 * t["ynorm"], decision_gated=False,
                           ok=True, tips_equal=tips_equal, exact_point=exact[i], mu_rel=mu_rel[i], chi=t["chi"])
                records.append(rec)
                # the stop the truth predicts before a step is taken; the error test is the kernel's own comparison of float64 values
                stop = None
                if last[i] == "accept":
                    if not err2_64 > eps3_sq:
                        stop = "err"
                    elif t["stop_grad"]:
                        stop = "grad"
                elif not mu[i] < mp.mpf(1e300):
                    stop = "mu"
                grad_gated = last[i] == "accept" and err2_64 > eps3_sq and t["grad_margin"] <= t["grad_tol"]
                if stop is None and t["small"]:
                    stop = "small"
                small_gated = t["small_margin"] <= t["bound"]
                if kind in ("stopped", "small"):
                    rec["stop"] = stop
                    want = kind == "small"
                    if (stop == "small") != want or stop is None:
                        rec["decision_gated"] = grad_gated or small_gated
                        rec["ok"] = rec["decision_gated"]
                    done[i] = True
                    continue
                if kind == "invalid":
                    rec["ok"] = False
                    done[i] = True
                    continue
                if stop is not None:          # the device went on where the truth stops
                    rec["stop"] = stop
                    rec["decision_gated"] = grad_gated if stop == "grad" else (small_gated if stop == "small" else False)
                    rec["ok"] = rec["decision_gated"]
                if kind == "accepted":
                    x_dev = np.array(b["state"][i], float)
                    if rot_index >= 0:
                        x64 = f64_step([float(v) for v in p_int[i]], Jl, g64, mu64[i], lo, hi)[0]
                        w, pinned = _recover_rotation(x_dev, x64[rot_index], b["tip"][i], fk, rot_index, search_cell)
                        if not pinned:        # compare modulo 2 pi; the point is no longer known to be the kernel's own
                            exact[i] = False
                        ambiguous[i] = pinned == "ambiguous"
                        x_dev[rot_index] = w
                    xm = [mp.mpf(float(v)) for v in x_dev]
                    diff = [xm[j] - t["x"][j] for j in range(S)]
                    if rot_index >= 0 and not exact[i]:
                        diff[rot_index] -= 2 * mp.pi * mp.nint(diff[rot_index] / (2 * mp.pi))
                    rec["exact_point"] = exact[i]
                    rec["err"] = float(mp.sqrt(sum((v * v for v in diff), mp.mpf(0))))
                    rec["ratio"] = rec["err"] / rec["bound"]
                    _, err2n_64 = f64_err(des[i], b["tip"][i])
                    pred, apred = _pred(xm, p_int[i], t["g"], mu[i])
                    num = mp.mpf(err2_64) - mp.mpf(err2n_64)
                    rho = num / pred if pred > 0 else mp.mpf(-1)
                    rec["rho"] = float(rho)
                    if not rho > 0:
                        rec["ok"] = False
                    tt = 2 * rho - 1
                    sh = 1 - tt ** 3
                    if sh > mp.mpf(1) / 3:
                        dg = sum(abs(float(xm[j]) - float(p_int[i][j])) * 4 * U * t["absg"][j] for j in range(S))     # g's own roundings
                        rho_rel = ((3 * S + 4) * U * float(apred) + dg) / float(pred) + 2 * U
                        slope = float(6 * tt * tt * abs(rho) / sh)
                        own = float(mu[i] * sum(((xm[j] - mp.mpf(float(p_int[i][j]))) ** 2 for j in range(S)), mp.mpf(0)) / pred)   # d ln pred / d ln mu
                        mu_rel[i] = mu_rel[i] * (1 + slope * own) + slope * rho_rel + float(abs(tt ** 3) / sh) * 4 * U + 2 * U
                        mu[i] *= sh
                    else:
                        mu_rel[i] += 2 * U
                        mu[i] /= 3
                    rho64 = f64_gain_ratio([float(v) for v in x_dev], [float(v) for v in p_int[i]], g64, mu64[i], err2_64, err2n_64)
                    mu64[i] *= f64_shrink(rho64)
                    nu[i] = 2.0
                    last[i] = "accept"
                    nxt[i] = x_dev
                else:
                    pending.append((i, rec, t, err2_64, mu[i]))
                    mu[i] *= mp.mpf(nu[i])
                    mu64[i] *= nu[i]
                    nu[i] *= 2.0
                    last[i] = "reject"
            if pending and fk is not None:
                X = np.array([[float(v) for v in t["x"]] for (_, _, t, _, _) in pending])
                tips = np.asarray(fk(X), float)
                for (i, rec, t, err2_64, mu_step), tip in zip(pending, tips):
                    en, err2n = f64_err(des[i], tip)
                    pred, _ = _pred(t["x"], p_int[i], t["g"], mu_step)
                    rho = (mp.mpf(err2_64) - mp.mpf(err2n)) / pred if pred > 0 else mp.mpf(-1)
                    rec["rho"] = float(rho)
                    margin = 2 * rec["bound"] * t["normJ"] * (math.sqrt(err2_64) + math.sqrt(err2n))
                    if rho > 0:
                        rec["decision_gated"] = abs(err2_64 - err2n) <= margin
                        rec["ok"] = rec["ok"] and rec["decision_gated"]
            p_int = nxt
            track.append(p_int.copy())
    return records, np.array(track)


def summary(records):
    """counts and the worst ratio of a case"""
    acc = [r for r in records if r["kind"] == "accepted"]
    judged = [r for r in acc if not r["gated"]]
    steps = [r for r in records if r["kind"] in ("accepted", "rejected", "small")]
    # a small-step stop has no trial point whose error could be judged: only its decision can be gated
    gated = [r for r in steps if (r["gated"] and r["kind"] != "small") or r["decision_gated"]]
    return dict(accepted=len(acc), rejected=sum(r["kind"] == "rejected" for r in records),
                clipped=sum(r["clipped"] for r in steps), gated=len(gated), steps=len(steps),
                gated_share=len(gated) / max(1, len(steps)), worst=max((r["ratio"] for r in judged), default=0.0),
                stops={s: sum(r["stop"] == s and r["kind"] in ("stopped", "small") for r in records) for s in ("err", "grad", "mu", "small")},
                max_nu=max((r["nu"] for r in records), default=2.0),
                low_rho=sum(r["rho"] is not None and 0 < r["rho"] < 0.5 for r in acc),
                bad=[(r["problem"], r["step"], r["kind"], r["stop"], r["ratio"]) for r in records
                     if not r["ok"] or (r["kind"] == "accepted" and not r["gated"] and r["ratio"] > 1.0)])


# ---- the cases, shared by the CPU test (float64_scheme over the oracle) and the GPU test (tr_ik_batch) --------------------------------
#        kind -> state size.  test_gpu_ik_device's seven kinds, and the three sizes of TRK_FOR_STATE_SIZE they leave out
SIZES = {"n1_norot": 1, "n1": 2, "config2": 3, "config3": 4, "rot_ret": 5, "n5": 6, "n6": 7, "n7": 8, "n8": 9, "n8_ret": 10}
N_PROBLEMS = 12
LM = dict(eps3=1e-6, eps2=1e-12, eps1=1e-16, mu_init=0.1)          # test_gpu_ik_device.LM
#        case -> (goal scale from the origin, K, solver arguments, half widths of a tight box about the start or None)
CASES = {"reach": (1.0, 16, LM, None),
         "unreach": (1.5, 40, LM, None),
         "mu6": (1.5, 40, dict(LM, mu_init=1e-6), None),
         "blocked": (1.5, 24, dict(LM, eps1=1e-9), (0.3, 0.03, 0.002))}     # N, rad, m


def case_robot(irt, kind):
    import make_fk_truth
    import test_gpu_ik_device as dev
    if kind in dev.KINDS:
        return dev._robot(irt, kind)
    robot = make_fk_truth.fixture_robot(irt, "n1" if kind == "n1_norot" else kind)[0]
    if kind == "n1_norot":
        robot.enable_rotation = False
    return robot


def build_case(irt, orc, helpers, kind, case):
    """dict(robot, orb, start (12, S), goals (12, 3), lo, hi, K, rot_index, lm): test_gpu_ik_device._ik_case's first 12 problems
    (for the three added kinds the same recipe), the starts' rotation wrapped into (-pi, pi), the goals scaled from the origin."""
    import test_gpu_ik_device as dev
    T = irt.tip_control
    if kind in dev.KINDS:
        robot, orb, goals, start, b = dev._ik_case(irt, orc, helpers, kind)
    else:
        robot = case_robot(irt, kind)
        N = len(robot.tendons)
        goal_states = irt.workloads.random_states(robot, 48, seed=11, tau_max=12.0 / np.sqrt(N))
        orb = helpers.oracle_robot(orc, robot)
        goals = np.array([orb.shape(s)["p"][-1] for s in goal_states])
        rng = np.random.default_rng(12)
        start = goal_states + rng.normal(size=goal_states.shape) * np.array([1.5 / np.sqrt(N)] * N + ([0.3] if robot.enable_rotation else []))
        b = T.Bounds.from_robot(robot)
        start = np.clip(start, np.maximum(b.lower, -10), np.minimum(b.upper, 25))
    scale, K, lm, box = CASES[case]
    start, goals = np.ascontiguousarray(start[:N_PROBLEMS]), np.ascontiguousarray(goals[:N_PROBLEMS] * scale)
    N = len(robot.tendons)
    rot = N if robot.enable_rotation else -1
    if rot >= 0:
        start[:, rot] = [canonical_angle(v) for v in start[:, rot]]
        assert (np.abs(start[:, rot]) < np.pi).all()
    lo, hi = b.lower.copy(), b.upper.copy()
    if box is not None:
        # one box for the whole call, about the mean start: every problem's start is clipped into it
        half = np.array([box[0]] * N + ([box[1]] if robot.enable_rotation else []) + ([box[2]] if robot.enable_retraction else []))
        mid = np.clip(start.mean(0), lo, hi)
        lo, hi = np.maximum(lo, mid - half), np.minimum(hi, mid + half)
    return dict(robot=robot, orb=orb, start=start, goals=goals, lo=lo, hi=hi, K=K, rot_index=rot, lm=lm, S=robot.state_size())


def oracle_fk(robot, orb):
    """states (m, S) -> tips (m, 3) of the oracle through tip_control's FK wrapper"""
    L, ret = robot.specs.L, robot.enable_retraction

    def fk(states):
        out = np.empty((len(states), 3))
        for i, x in enumerate(np.asarray(states, float)):
            out[i] = (0.0, 0.0, L - x[-1]) if ret and x[-1] > L else orb.shape(x)["p"][-1]
        return out
    return fk
