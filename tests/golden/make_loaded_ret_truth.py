#!/usr/bin/env python3
"""Generates tests/golden/loaded_ret_truth_<name>.npz: the loaded rod of robots WITH retraction -- the numpy reference's converged
shooting (tests/loaded_ret_reference.py) and the extended-precision (mpmath, 40 digits) truth of ONE integration from its strains,
every state on its own grid t_range(s_start, L, dL).

    python tests/golden/make_loaded_ret_truth.py [name ...]        (a process pool of at most 16; some minutes)

Robots and states: make_fk_truth.fixture_states of the five retraction fixtures, with the attempt recorded in fk_truth_<name>.npz, so
that the states are the unloaded truth's (asserted) and its v0, u0 serve the zero-load comparison.  config3_rot_ret: N = 4, rotation,
129 points, seeded s_start; n1_ret, n8_ret, config3_ret_edges, config2_ret_edges: dL = L / 40, rows 0 - 14 are
fk_truth_common.special_s_start (aligned grids, two-step first intervals, two- and one-point backbones, s_start = L and beyond).

Load cases, built as make_loaded_fk.loads builds them but seeded by the fixture's position in NAMES below:
  A  one wrench for all (make_loaded_fk.WRENCH_A), NO distributed load: the tests pass dist = None (the kernel's null pointer)
  D  gravity turned by Rz(-theta), plus a seeded distributed force (0.3 .. 1.0 N/m) and moment (0.003 .. 0.01 N), plus a seeded
     wrench (|F| <= 0.1 N, |L| <= 2e-3 N m): all twelve numbers of a row are non-zero

Per state and case:
  vu0       the reference's converged strains (Newton shooting from the unloaded solution at the state's s_start)
  truth     make_fk_truth.model(consts, C, D, state, v0, u0, steps of the state, pattern, f_e, l_e, wrench) from vu0: points (thinned
            by make_fk_truth.stored_idx for config3_rot_ret), tip frame, L, L_i, tip strains, the six residual components, as
            hi / lo pairs
  E_ref     |loaded_ret_reference.evaluate - truth|
  Edes_*    E_design + E_trig: the largest shift under make_fk_truth.PERT_PATTERNS (the Newton-step sites) PLUS the largest shift
            under make_fk_truth.TRIG_PATTERNS (route_tendon's carried rotations of (sin, cos) in the state's own first interval; the
            allowance fixed in make_fk_truth.py).  Stored as one number so that the bound rule is fk_truth_common.loaded_bounds'
            verbatim: 4 (E_ref + E_design), floors of 4 ulp and, for the residual, e_terms.
  shooting  the converged shape at the stored points, C_i and bound_i = 1e-9 m + 1.5 C_i (residual_threshold + |e_ref,i|):
            make_loaded_fk.py's rule, the project's tolerance for a shooting result.
Rows with s_start >= L integrate nothing and have no truth: NO_TRUTH_ROWS = (12, 13) of the four dL = L / 40 fixtures, known in
advance; their truth arrays are zero and the tests assert these rows exactly instead.  They are the only rows left out.
The generator FAILS if any other (state, case) does not converge in the reference; no row is dropped.  (Should that happen after a
change: replace the STATE by the next seeded one and record it here.  So far no state has been replaced.)
Layout: per case the keys of fk_truth_common.LOADED_KEYS as <key>_hi_<case>, <key>_lo_<case>, Eref_<key>_<case>, Edes_<key>_<case>,
e_terms_<case>; points padded with zeros to the widest state, pt_idx (24, Q) padded with -1.  Size: at most 393 KB per file.
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
import loaded_ret_reference as ref                                   # noqa: E402
import make_fk_truth as mft                                          # noqa: E402
import make_loaded_fk as mlf                                         # noqa: E402

NAMES = ("config3_rot_ret", "n1_ret", "n8_ret", "config3_ret_edges", "config2_ret_edges")     # new names go last: case D is seeded by position
CASES = ("A", "D")


def path(name):
    return os.path.join(HERE, "loaded_ret_truth_%s.npz" % name)


def no_truth_rows(name):
    return () if name == "config3_rot_ret" else (12, 13)


def fixture(name):
    """(robot, oracle robot, states (24, S), the unloaded truth fixture)"""
    un = ftc.load(name)
    robot, st = mft.fixture_states(mft._irt(), name, int(un["attempt"]))
    assert np.array_equal(st, un["states"]) and robot.enable_retraction
    return robot, mft.oracle_robot(robot), st, un


def loads(name, robot, st, case):
    """(wrench (n, 6), dist (n, 6)) of a case: make_loaded_fk.loads' cases A and D under this generator's seeds"""
    n, N = st.shape[0], len(robot.tendons)
    theta = st[:, N] if robot.enable_rotation else np.zeros(n)
    wrench, dist = np.zeros((n, 6)), np.zeros((n, 6))
    if case == "A":
        wrench[:] = mlf.WRENCH_A
        return wrench, dist
    c, s = np.cos(-theta), np.sin(-theta)
    dist[:, 0] = c * mlf.GRAVITY[0] - s * mlf.GRAVITY[1]
    dist[:, 1] = s * mlf.GRAVITY[0] + c * mlf.GRAVITY[1]
    rng = np.random.default_rng(9000 + NAMES.index(name))
    for col, cap in ((0, 0.1), (3, 2e-3)):
        d = rng.normal(size=(n, 3))
        wrench[:, col:col + 3] = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.0, cap, (n, 1))
    rng = np.random.default_rng(9500 + NAMES.index(name))
    for col, lo, hi in ((0, 0.3, 1.0), (3, 0.003, 0.01)):
        d = rng.normal(size=(n, 3))
        dist[:, col:col + 3] += d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(lo, hi, (n, 1))
    return wrench, dist


def outputs(m, idx):
    """The stored outputs of one model run, in ftc.LOADED_KEYS' order: flat lists of mpf.  idx: the stored backbone points."""
    return dict(p=[x for q in idx for x in m["p"][q]], R=list(m["R"]), L=[m["L"]], Li=list(m["Li"]), vu=list(m["v"]) + list(m["u"]), e=list(m["e"]))


def reference_row(ev, i, idx):
    k = int(ev["n_points"][i])
    return dict(p=ev["p"][i, idx].reshape(-1), R=ev["R"][i, k - 1].T.reshape(9), L=ev["L"][i:i + 1], Li=ev["L_i"][i], vu=ev["vuL"][i], e=ev["e"][i])


def state_task(args):
    """One (state, case): the truth, E_ref against the reference's row, E_design over the Newton-step patterns plus E_trig over the
    carried-rotation patterns."""
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
    total = {key: [mft.ZERO] * len(vals) for key, vals in base.items()}
    for patterns in (mft.PERT_PATTERNS, mft.TRIG_PATTERNS if steps else ()):
        des = {key: [mft.ZERO] * len(vals) for key, vals in base.items()}
        for pat in patterns:
            bent = outputs(run(pat), idx)
            for key in des:
                des[key] = [max(d, abs(x - y)) for d, x, y in zip(des[key], bent[key], base[key])]
        for key in des:
            total[key] = [a + b for a, b in zip(total[key], des[key])]
    for key in total:
        out["Edes_" + key] = np.array([float(d) for d in total[key]])
    out["e_terms"] = np.array([float(x) for x in m["e_terms"]])
    out["seconds"] = time.time() - t0
    return out


def fixture_tasks(name):
    """(arrays that need no mpmath, {case: {row: state_task arguments}})"""
    robot, rob, st, un = fixture(name)
    sp = robot.specs
    C = np.array([t.C for t in robot.tendons], np.float64)
    D = np.array([t.D for t in robot.tendons], np.float64)
    consts = np.array([sp.L, sp.dL, sp.ro, sp.ri, sp.E, sp.nu, robot.r, robot.residual_threshold, float(robot.enable_rotation), 1.0])
    grids = [ref.state_grid(rob, s) for s in st[:, -1]]
    n_points = np.array([len(t) for t, _, _ in grids], np.int32)
    assert np.array_equal(n_points, un["n_points"])
    skip = no_truth_rows(name)
    assert [i for i, (_, _, single) in enumerate(grids) if single] == list(skip)
    steps = [mft.step_list(t, sp.dL) for t, _, _ in grids]
    assert all(a == b for a, (_, b, _) in zip(steps, grids))
    idxs = [mft.stored_idx(int(k), int(n_points.max())) for k in n_points]
    Q = max(len(i) for i in idxs)
    fx = dict(states=st, C=C, D=D, consts=consts, max_tension=np.array([t.max_tension for t in robot.tendons]), n_points=n_points,
              pt_idx=np.full((ftc.N_STATES, Q), -1, np.int32), no_truth=np.array(skip, np.int32))
    for i, idx in enumerate(idxs):
        fx["pt_idx"][i, :len(idx)] = idx
    tasks = {}
    for case in CASES:
        w, d = loads(name, robot, st, case)
        sol = ref.shoot(rob, st, F_e=w[:, :3], L_e=w[:, 3:], f_e=d[:, :3], l_e=d[:, 3:])
        if not sol["converged"].all():
            raise RuntimeError("%s case %s: states %s did not converge (|e| = %s)" % (name, case, np.nonzero(~sol["converged"])[0], sol["e"][~sol["converged"]]))
        ev = ref.evaluate(rob, st, sol["vu0"], F_e=w[:, :3], L_e=w[:, 3:], f_e=d[:, :3], l_e=d[:, 3:])
        shoot_p = np.zeros((ftc.N_STATES, Q, 3))
        for i, idx in enumerate(idxs):
            shoot_p[i, :len(idx)] = sol["p"][i, idx]
        fx.update({"wrench_" + case: w, "dist_" + case: d, "vu0_" + case: sol["vu0"], "shoot_p_" + case: shoot_p, "e_ref_" + case: sol["e"],
                   "C_" + case: sol["C"], "bound_" + case: 1e-9 + 1.5 * sol["C"] * (robot.residual_threshold + sol["e"]),
                   "iters_" + case: sol["iters"]})
        tasks[case] = {i: (consts, C, D, st[i], sol["vu0"][i], steps[i], idxs[i], w[i], d[i], reference_row(ev, i, idxs[i]))
                       for i in range(ftc.N_STATES) if i not in skip}
    return fx, tasks


def assemble(name, fx, results):
    n, Q, N = ftc.N_STATES, fx["pt_idx"].shape[1], fx["C"].shape[0]
    width = dict(p=3 * Q, R=9, L=1, Li=N, vu=6, e=6)
    secs = 0.0
    for case, rs in results.items():
        for key in ftc.LOADED_KEYS:
            for pre, dt in (("%s_hi", np.float64), ("%s_lo", np.float32), ("Eref_%s", np.float64), ("Edes_%s", np.float64)):
                a = np.zeros((n, width[key]), dt)
                for i, r in rs.items():
                    v = r[pre % key]
                    a[i, :len(v)] = v
                per_value = pre in ("%s_hi", "%s_lo")
                if key == "p":
                    a = a.reshape(n, Q, 3) if per_value else a.max(axis=1)
                elif key in ("R", "L"):
                    a = a[:, 0] if (key == "L" and per_value) else (a if per_value else a.max(axis=1))
                fx["%s_%s" % (pre % key, case)] = a
        et = np.zeros((n, 6))
        for i, r in rs.items():
            et[i] = r["e_terms"]
        fx["e_terms_" + case] = et
        secs += sum(r["seconds"] for r in rs.values())
    mft.save_npz(path(name), fx)
    size = os.path.getsize(path(name))
    assert size <= 393 * 1024, size
    keep = np.setdiff1d(np.arange(n), fx["no_truth"])
    rng = lambda a: "%.2g .. %.2g" % (np.min(a[keep]), np.max(a[keep]))
    for case in results:
        b = ftc.loaded_bounds(fx, case)
        print("%-18s %s E_ref p %s  e %s | E_des+trig p %s  e %s | bound p %s  R %s  L %s  L_i %s  vu %s  |e| %s | shooting bound %s m, Newton steps <= %d"
              % (name, case, rng(fx["Eref_p_" + case]), rng(fx["Eref_e_" + case]), rng(fx["Edes_p_" + case]), rng(fx["Edes_e_" + case]),
                 rng(b["p"]), rng(b["R"]), rng(b["L"]), rng(b["L_i"]), rng(b["vu"]), rng(b["enorm"]), rng(fx["bound_" + case]),
                 fx["iters_" + case].max()), flush=True)
    print("%-18s %.0f s of model runs, %d KB" % (name, secs, size // 1024), flush=True)


def main(names):
    from concurrent.futures import ProcessPoolExecutor
    t0 = time.time()
    prepared = [(n,) + fixture_tasks(n) for n in names]
    with ProcessPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        futures = [(n, fx, {case: {i: pool.submit(state_task, t) for i, t in ts.items()} for case, ts in tasks.items()}) for n, fx, tasks in prepared]
        for n, fx, fs in futures:
            assemble(n, fx, {case: {i: f.result() for i, f in ff.items()} for case, ff in fs.items()})
    print("generated %d fixtures in %.0f s" % (len(names), time.time() - t0))


if __name__ == "__main__":
    main(sys.argv[1:] or list(NAMES))
