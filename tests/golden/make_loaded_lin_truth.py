#!/usr/bin/env python3
"""Generates tests/golden/loaded_lin_truth_<name>.npz: the extended-precision (mpmath, 40 digits) evaluation of the 13 + 2 S lanes
of the loaded rod's linearisation (csrc/fk_loaded_lin_kernel.hpp; tests/loaded_ik_reference.linearise), for four robots of
make_loaded_fk.NAMES -- config1 (S = 3, frame BASE), n1 (S = 2), config3_rot (S = 5, 129 points) and n8 (S = 9), the last three with
the load fixed in the WORLD frame -- under load case D (the only one with a distributed moment), first 6 states.

    python tests/golden/make_loaded_lin_truth.py [name ...]        (a process pool of at most 16; minutes)

The model is make_fk_truth's loaded integration and tip balance (make_loaded_fk_truth.py), per LANE: the lane's state and base
strains are the fp64 numbers linearise forms (lane 0 the point, 1 + 2j / 2 + 2j strain j moved by -+ delta_y, 13 + 2k / 14 + 2k state
entry k moved by -+ max(|1e-4 p_k|, delta)), converted exactly; nothing is solved.  The point's strains are the fixture's vu0_D
(tests/golden/loaded_fk_<name>.npz).  The call's one load set of a state is
  BASE    the fixture's rows wrench_D[i], dist_D[i] themselves;
  WORLD   those rows turned by Rz(theta_i) in fp64 -- twelve fp64 numbers that DEFINE the set.  Every lane's rows are then
          Rz(-theta_lane) of the set with theta_lane the lane's own, possibly perturbed, rotation, formed in mpmath: a lane whose
          rotation is perturbed sees the load it would see there.
Per state and lane the fixture stores the tip after rotate_z (x) and the six residual components (e) as hi / lo pairs and
  E_ref     |loaded_ik_reference.tips_and_residuals - truth| on the same lane;
  E_design  the largest shift under make_fk_truth's four Newton-step patterns;
  e_terms   per residual component the largest magnitude among the terms summed into it.
Layout (n = 6 states, Q = 13 + 2 S lanes):
  states (n, S), vu0 (n, 6), wrench (n, 6), dist (n, 6) (the call's set of every state), world (), delta (), delta_y ()
  lane_states (n, Q, S), lane_vu (n, Q, 6), lane_d (n, Q)
  x_hi (n, Q, 3) f64, x_lo f32, e_hi (n, Q, 6), e_lo, Eref_x, Edes_x (n, Q, 3), Eref_e, Edes_e, e_terms (n, Q, 6)
The bounds (lane_bounds, below) are fk_truth_common.loaded_bounds' rule per lane and component: max(4 (E_ref + E_design),
4 ulp(magnitude)), the magnitude of a tip component being the lane's largest tip coordinate and of a residual component its e_terms.
The bound of a central difference of two lanes is (B+ + B-) 0.5 / d.  Nothing else is tuned.
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
for _p in (ROOT, TESTS, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import fk_truth_common as ftc                                        # noqa: E402

#        fixture -> frame of the call's load set
NAMES = {"config1": "base", "n1": "world", "config3_rot": "world", "n8": "world"}
CASE, N_STATES = "D", 6
DELTA = DELTA_Y = 1e-6


def path(name):
    return os.path.join(HERE, "loaded_lin_truth_%s.npz" % name)


def load(name):
    with np.load(path(name)) as d:
        return {k: d[k] for k in d.files}


def world_set(rows, theta):
    """The call's load set of every state whose rows before the rotation are `rows` (n, 6): Rz(theta) of them, in fp64."""
    c, s = np.cos(theta), np.sin(theta)
    out = rows.copy()
    for h in (0, 3):
        out[:, h + 0] = c * rows[:, h + 0] - s * rows[:, h + 1]
        out[:, h + 1] = s * rows[:, h + 0] + c * rows[:, h + 1]
    return out


def lane_bounds(fx):
    """(Bx (n, Q, 3), Be (n, Q, 6)): the bound of every lane's tip and residual components."""
    f = lambda e_ref, e_des, mag: np.maximum(4.0 * (e_ref + e_des), 4.0 * np.spacing(np.abs(mag)))
    xmag = np.abs(fx["x_hi"]).max(axis=2, keepdims=True)
    return f(fx["Eref_x"], fx["Edes_x"], np.broadcast_to(xmag, fx["x_hi"].shape)), f(fx["Eref_e"], fx["Edes_e"], fx["e_terms"])


def truth_blocks(fx):
    """The central-difference quotients of the truth and their bounds: dict(J_y (n, 6, 6), J_p (n, 6, S), X_y (n, 3, 6), X_p
    (n, 3, S), x (n, 3), e (n, 6)) of (value, bound) pairs.  The quotient is formed in fp64 from the hi + lo pairs: hi+ - hi- is
    exact (Sterbenz) or rounds at 1e-16 of numbers whose bounds are 4 ulp at least."""
    Bx, Be = lane_bounds(fx)
    d = fx["lane_d"]
    S = fx["states"].shape[1]
    val = lambda k: (fx[k + "_hi"], fx[k + "_lo"].astype(np.float64))

    def quot(key, B, first, cnt):
        hi, lo = val(key)
        m, p = slice(first, first + 2 * cnt, 2), slice(first + 1, first + 2 * cnt, 2)
        sc = (0.5 / d[:, m])[:, :, None]
        q = ((hi[:, p] - hi[:, m]) + (lo[:, p] - lo[:, m])) * sc
        return np.transpose(q, (0, 2, 1)), np.transpose((B[:, p] + B[:, m]) * sc, (0, 2, 1))
    xh, xl = val("x")
    eh, el = val("e")
    return dict(J_y=quot("e", Be, 1, 6), J_p=quot("e", Be, 13, S), X_y=quot("x", Bx, 1, 6), X_p=quot("x", Bx, 13, S),
                x=(xh[:, 0] + xl[:, 0], Bx[:, 0]), e=(eh[:, 0] + el[:, 0], Be[:, 0]))


def lane_model(consts, C, D, state, vu, steps, wrench, dist, world, pattern=None):
    """(x [3], e [6], e_terms [6]) of one lane in mpmath: make_fk_truth.model's integration with the lane's load rows formed in
    mpmath from the call's set."""
    import make_fk_truth as mft
    mp = mft.mp
    Lr, dL, ro, ri, E, nu, r, res, rot, ret = (float(x) for x in consts)
    N = len(C)
    signs = mft.Signs(pattern) if pattern is not None else None
    Kse, Kbt = mft.stiffness(ro, ri, E, nu)
    tau = [mp.mpf(float(s)) for s in state[:N]]
    th = mp.mpf(float(state[N])) if rot else mft.ZERO
    cs, sn = mp.cos(th), mp.sin(th)
    w, d = ([mp.mpf(float(y)) for y in a] for a in (wrench, dist))
    if world and rot:                                                   # Rz(-theta) (x, y, z) = (c x + s y, c y - s x, z)
        turn = lambda v: [cs * v[0] + sn * v[1], cs * v[1] - sn * v[0], v[2]]
        w, d = turn(w[:3]) + turn(w[3:]), turn(d[:3]) + turn(d[3:])
    x = dict(p=[mft.ZERO] * 3, R=[[mft.ONE, mft.ZERO, mft.ZERO], [mft.ZERO, mft.ONE, mft.ZERO], [mft.ZERO, mft.ZERO, mft.ONE]],
             v=[mp.mpf(float(s)) for s in vu[:3]], u=[mp.mpf(float(s)) for s in vu[3:]], L=mft.ZERO, Li=[mft.ZERO] * N)
    rcache = {}

    def rt(t):
        if t not in rcache:
            if len(rcache) > 4:
                rcache.clear()
            rcache[t] = mft.routing(C, D, t)
        return rcache[t]

    for (t, h, row) in steps:
        hm = mp.mpf(h)
        tm, te = t + h * 0.5, t + h
        k1 = mft.deriv(rt(t), Kse, Kbt, tau, x, signs, d[:3], d[3:])
        k2 = mft.deriv(rt(tm), Kse, Kbt, tau, mft._axpy(x, hm / 2, k1), signs, d[:3], d[3:])
        k3 = mft.deriv(rt(tm), Kse, Kbt, tau, mft._axpy(x, hm / 2, k2), signs, d[:3], d[3:])
        k4 = mft.deriv(rt(te), Kse, Kbt, tau, mft._axpy(x, hm, k3), signs, d[:3], d[3:])
        x = mft._axpy(mft._axpy(mft._axpy(mft._axpy(x, hm / 6, k1), hm / 3, k2), hm / 3, k3), hm / 6, k4)
    e, terms = mft.tip_balance(C, D, Lr, Kse, Kbt, tau, x, w[:3], w[3:])
    p = x["p"]
    tip = [cs * p[0] - sn * p[1], sn * p[0] + cs * p[1], p[2]] if rot else list(p)
    return tip, e, terms


def lane_task(args):
    """One lane: the truth, E_ref against the reference's row, E_design over the Newton-step patterns."""
    import make_fk_truth as mft
    consts, C, D, state, vu, steps, wrench, dist, world, ref_x, ref_e = args
    t0 = time.time()
    run = lambda pat: lane_model(consts, C, D, state, vu, steps, wrench, dist, world, pat)
    tip, e, terms = run(None)
    out = {}
    for key, vals, refv in (("x", tip, ref_x), ("e", e, ref_e)):
        hl = [mft.split(v) for v in vals]
        out[key + "_hi"] = np.array([h for h, _ in hl], np.float64)
        out[key + "_lo"] = np.array([l for _, l in hl], np.float32)
        out["Eref_" + key] = ftc.err_vs_truth(refv, out[key + "_hi"], out[key + "_lo"])
    des = dict(x=[mft.ZERO] * 3, e=[mft.ZERO] * 6)
    for pat in mft.PERT_PATTERNS:
        bt, be, _ = run(pat)
        des["x"] = [max(q, abs(a - b)) for q, a, b in zip(des["x"], bt, tip)]
        des["e"] = [max(q, abs(a - b)) for q, a, b in zip(des["e"], be, e)]
    for key in des:
        out["Edes_" + key] = np.array([float(q) for q in des[key]])
    out["e_terms"] = np.array([float(v) for v in terms])
    out["seconds"] = time.time() - t0
    return out


def fixture_inputs(name, rows=None):
    """(rob, fixture arrays that need no mpmath, (consts, C, D, steps)): the states, the call's load set of every state, the
    lanes' states, strains and steps, and the reference's lanes."""
    import loaded_jacobian_reference as ljr
    import make_fk_truth as mft
    import make_loaded_fk as mlf
    robot, rob, st = mlf.fixture(name)
    lf = dict(np.load(mlf.path(name)))
    assert np.array_equal(st, lf["states"]) and not robot.enable_retraction
    rows = np.arange(N_STATES) if rows is None else np.asarray(rows)
    st = np.ascontiguousarray(st[rows])
    frame = NAMES[name]
    N = len(robot.tendons)
    w, d, vu0 = (lf["%s_%s" % (k, CASE)][rows] for k in ("wrench", "dist", "vu0"))
    if frame == "world":
        assert robot.enable_rotation
        w, d = world_set(w, st[:, N]), world_set(d, st[:, N])
    sp = robot.specs
    C = np.array([t.C for t in robot.tendons], np.float64)
    D = np.array([t.D for t in robot.tendons], np.float64)
    consts = np.array([sp.L, sp.dL, sp.ro, sp.ri, sp.E, sp.nu, robot.r, robot.residual_threshold, float(robot.enable_rotation), 0.0])
    t_pts = rob.t_range(0.0)
    steps = mft.step_list(t_pts, sp.dL)
    n, S = st.shape
    Q = 13 + 2 * S
    ls, lv = np.repeat(st[:, None, :], Q, axis=1), np.repeat(vu0[:, None, :], Q, axis=1)
    import loaded_fk_reference as ref
    dp = ref.fd_steps(st, DELTA)
    j, k = np.arange(6), np.arange(S)
    lv[:, 1 + 2 * j, j] -= DELTA_Y
    lv[:, 2 + 2 * j, j] += DELTA_Y
    ls[:, 13 + 2 * k, k] -= dp
    ls[:, 14 + 2 * k, k] += dp
    ref_x, ref_e, ld = np.empty((n, Q, 3)), np.empty((n, Q, 6)), np.empty((n, Q))
    for i in range(n):                                                  # one load set per call: one state at a time
        x, e, dd = ljr.lanes(rob, st[i:i + 1], vu0[i:i + 1], w[i], d[i], frame, DELTA, DELTA_Y)
        ref_x[i], ref_e[i], ld[i] = x[0], e[0], dd[0]
    fx = dict(states=st, vu0=vu0, wrench=w, dist=d, world=np.array(int(frame == "world"), np.int32), delta=np.array(DELTA),
              delta_y=np.array(DELTA_Y), lane_states=ls, lane_vu=lv, lane_d=ld)
    return rob, fx, (consts, C, D, steps), (ref_x, ref_e)


def lane_args(fx, model, refs, i, q):
    consts, C, D, steps = model
    return (consts, C, D, fx["lane_states"][i, q], fx["lane_vu"][i, q], steps, fx["wrench"][i], fx["dist"][i], bool(fx["world"]),
            refs[0][i, q], refs[1][i, q])


def assemble(name, fx, results):
    n, Q = fx["lane_d"].shape
    for key in ("x_hi", "x_lo", "e_hi", "e_lo", "Eref_x", "Eref_e", "Edes_x", "Edes_e", "e_terms"):
        fx[key] = np.stack([np.stack([results[i][q][key] for q in range(Q)]) for i in range(n)])
    import make_fk_truth as mft
    mft.save_npz(path(name), fx)
    size = os.path.getsize(path(name))
    assert size <= 200 * 1024, size
    Bx, Be = lane_bounds(fx)
    rng = lambda a: "%.2g .. %.2g" % (np.min(a), np.max(a))
    secs = sum(r["seconds"] for rs in results for r in rs)
    print("%-12s E_ref x %s  e %s | E_design x %s  e %s | bound x %s  e %s | %.0f s of model runs, %d KB"
          % (name, rng(fx["Eref_x"]), rng(fx["Eref_e"]), rng(fx["Edes_x"]), rng(fx["Edes_e"]), rng(Bx), rng(Be), secs, size // 1024),
          flush=True)


def main(names):
    from concurrent.futures import ProcessPoolExecutor
    t0 = time.time()
    prepared = [(n,) + fixture_inputs(n, np.arange(N_STATES))[1:] for n in names]
    with ProcessPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        futures = [(n, fx, [[pool.submit(lane_task, lane_args(fx, model, refs, i, q)) for q in range(fx["lane_d"].shape[1])]
                            for i in range(fx["lane_d"].shape[0])]) for n, fx, model, refs in prepared]
        for n, fx, fs in futures:
            assemble(n, fx, [[f.result() for f in row] for row in fs])
    print("generated %d fixtures in %.0f s" % (len(names), time.time() - t0))


if __name__ == "__main__":
    main(sys.argv[1:] or list(NAMES))
