#!/usr/bin/env python3
"""Generates tests/golden/loaded_fk_truth_<name>.npz: the extended-precision (mpmath, 40 digits) evaluation of the LOADED rod
integration -- make_fk_truth.model with the two load terms c -= R^T l_e, d -= R^T f_e in the right-hand side and the tip balance
behind it -- for the six robots of make_loaded_fk.NAMES under the load cases A (one wrench), C (gravity and a wrench per state)
and D (C plus a distributed force of any direction and a distributed moment).  Case B is C without the wrench and has no truth of
its own.

    python tests/golden/make_loaded_fk_truth.py [name ...]        (a process pool of at most 16; a few minutes)

What is pinned is ONE integration from given base strains, not the shooting: the start values are the fixture's vu0_<case>
(tests/golden/loaded_fk_<name>.npz, the numpy reference's converged strains), converted exactly, and nothing is solved in mpmath.
The step sequence is make_fk_truth.step_list on the oracle's t_range(0): the same (t, h) pairs for all 24 states; the stored
backbone points are make_fk_truth.stored_idx's (all of them up to P = 64; every fourth and the last two of config3_rot's 129).
The loads are the fixture's rows, converted exactly, in the base frame before the state's rotation.

Per state and case the fixture stores the truth of the points, the tip frame, L, every L_i, the tip strains (v, u) and the six
components of the tip residual e (make_fk_truth.tip_balance) as hi / lo pairs, and for each of them
  E_ref     |loaded_fk_reference.evaluate - truth| from the same vu0 and loads: the fp64 rounding this state amplifies;
  E_design  the largest shift under make_fk_truth's four Newton-step patterns (the sites are the unloaded model's: the load terms
            and the tip balance have no reciprocal of their own -- fk_loaded_uniform forms R^T f_e, R^T l_e with fused multiply-adds
            and the balance with IEEE sqrt and division, contraction off);
  e_terms   per residual component the largest magnitude among the terms summed into it: the floor of its bound.
The bounds of the tests are fk_truth_common.loaded_bounds: 4 (E_ref + E_design), at least 4 ulp of the output's magnitude (of
e_terms for a residual component); the bound on |e| is the sum of the six component bounds, since | |a| - |b| | <= |a - b|_1.
They come from this model alone, change only through a change to it with the reason written here, and are never tuned on what a
kernel returns.  Layout: tests/fk_truth_common.py.
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
import loaded_fk_reference as ref                                    # noqa: E402
import make_fk_truth as mft                                          # noqa: E402
import make_loaded_fk as mlf                                         # noqa: E402

CASES = ftc.LOADED_CASES


def outputs(m, idx):
    """The stored outputs of one model run, in ftc.LOADED_KEYS' order: flat lists of mpf.  idx: the stored backbone points."""
    return dict(p=[x for q in idx for x in m["p"][q]], R=list(m["R"]), L=[m["L"]], Li=list(m["Li"]), vu=list(m["v"]) + list(m["u"]), e=list(m["e"]))


def reference(rob, st, vu0, wrench, dist, idx):
    """loaded_fk_reference.evaluate in the outputs' layout: dict of (24, k) arrays."""
    out = ref.evaluate(rob, st, vu0, F_e=wrench[:, :3], L_e=wrench[:, 3:], f_e=dist[:, :3], l_e=dist[:, 3:])
    n = len(st)
    return dict(p=out["p"][:, idx].reshape(n, -1), R=np.swapaxes(out["R"][:, -1], 1, 2).reshape(n, 9), L=out["L"].reshape(n, 1), Li=out["L_i"],
                vu=out["vuL"], e=out["e"])


def state_task(args):
    """One (state, case): the truth, E_ref against the reference's row, E_design over the Newton-step patterns."""
    consts, C, D, state, vu0, steps, idx, wrench, dist, ref_row = args
    t0 = time.time()
    run = lambda pat: mft.model(consts, C, D, state, vu0[:3], vu0[3:], steps, pat, f_e=dist[:3], l_e=dist[3:], wrench=wrench)
    m = run(None)
    base = outputs(m, idx)
    out = {}
    for key, vals in base.items():
        hl = [mft.split(x) for x in vals]
        out[key + "_hi"] = np.array([h for h, _ in hl], np.float64)
        out[key + "_lo"] = np.array([l for _, l in hl], np.float32)
        out["Eref_" + key] = ftc.err_vs_truth(ref_row[key], out[key + "_hi"], out[key + "_lo"])
    des = {key: [mft.ZERO] * len(vals) for key, vals in base.items()}
    for pat in mft.PERT_PATTERNS:
        bent = outputs(run(pat), idx)
        for key in des:
            des[key] = [max(d, abs(x - y)) for d, x, y in zip(des[key], bent[key], base[key])]
    for key in des:
        out["Edes_" + key] = np.array([float(d) for d in des[key]])
    out["e_terms"] = np.array([float(x) for x in m["e_terms"]])
    out["seconds"] = time.time() - t0
    return out


def fixture_tasks(name):
    """(arrays that need no mpmath, {case: [state_task arguments]})"""
    robot, rob, st = mlf.fixture(name)
    lf = dict(np.load(mlf.path(name)))
    assert np.array_equal(st, lf["states"]) and not robot.enable_retraction
    sp = robot.specs
    C = np.array([t.C for t in robot.tendons], np.float64)
    D = np.array([t.D for t in robot.tendons], np.float64)
    consts = np.array([sp.L, sp.dL, sp.ro, sp.ri, sp.E, sp.nu, robot.r, robot.residual_threshold, float(robot.enable_rotation), 0.0])
    t_pts = rob.t_range(0.0)
    steps = mft.step_list(t_pts, sp.dL)
    assert [r for _, _, r in steps if r >= 0] == list(range(1, len(t_pts)))
    idx = mft.stored_idx(len(t_pts), len(t_pts))
    fx = dict(states=st, C=C, D=D, consts=consts, max_tension=np.array([t.max_tension for t in robot.tendons]),
              steps=np.array([(t, h) for t, h, _ in steps]), step_row=np.array([r for _, _, r in steps], np.int32),
              n_points=np.array(len(t_pts), np.int32), pt_idx=np.array(idx, np.int32))
    tasks = {}
    for case in CASES:
        w, d, vu0 = lf["wrench_" + case], lf["dist_" + case], lf["vu0_" + case]
        fx["wrench_" + case], fx["dist_" + case], fx["vu0_" + case] = w, d, vu0
        rr = reference(rob, st, vu0, w, d, idx)
        tasks[case] = [(consts, C, D, st[i], vu0[i], steps, idx, w[i], d[i], {k: v[i] for k, v in rr.items()}) for i in range(len(st))]
    return fx, tasks


def assemble(name, fx, results):
    P = len(fx["pt_idx"])
    secs = 0.0
    for case, rs in results.items():
        for key in ftc.LOADED_KEYS:
            for pre in ("%s_hi", "%s_lo", "Eref_%s", "Edes_%s"):
                a = np.stack([r[pre % key] for r in rs])
                if key == "p":
                    a = a.reshape(len(rs), P, 3) if pre in ("%s_hi", "%s_lo") else a.max(axis=1)
                elif key in ("R", "L"):
                    a = a[:, 0] if (key == "L" and pre in ("%s_hi", "%s_lo")) else (a if pre in ("%s_hi", "%s_lo") else a.max(axis=1))
                fx["%s_%s" % (pre % key, case)] = a
        fx["e_terms_" + case] = np.stack([r["e_terms"] for r in rs])
        secs += sum(r["seconds"] for r in rs)
    mft.save_npz(ftc.loaded_path(name), fx)
    size = os.path.getsize(ftc.loaded_path(name))
    assert size <= 393 * 1024, size
    rng = lambda a: "%.2g .. %.2g" % (np.min(a), np.max(a))
    for case in results:
        b = ftc.loaded_bounds(fx, case)
        print("%-12s %s E_ref p %s  e %s | E_design p %s  e %s | bound p %s  R %s  L %s  L_i %s  vu %s  |e| %s"
              % (name, case, rng(fx["Eref_p_" + case]), rng(fx["Eref_e_" + case]), rng(fx["Edes_p_" + case]), rng(fx["Edes_e_" + case]),
                 rng(b["p"]), rng(b["R"]), rng(b["L"]), rng(b["L_i"]), rng(b["vu"]), rng(b["enorm"])), flush=True)
    print("%-12s %.0f s of model runs, %d KB" % (name, secs, size // 1024), flush=True)


def main(names):
    from concurrent.futures import ProcessPoolExecutor
    t0 = time.time()
    prepared = [(n,) + fixture_tasks(n) for n in names]
    with ProcessPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        futures = [(n, fx, {case: [pool.submit(state_task, t) for t in ts] for case, ts in tasks.items()}) for n, fx, tasks in prepared]
        for n, fx, fs in futures:
            assemble(n, fx, {case: [f.result() for f in ff] for case, ff in fs.items()})
    print("generated %d fixtures in %.0f s" % (len(names), time.time() - t0))


if __name__ == "__main__":
    main(sys.argv[1:] or list(mlf.NAMES))
