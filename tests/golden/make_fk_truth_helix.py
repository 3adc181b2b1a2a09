#!/usr/bin/env python3
"""Generates tests/golden/fk_truth_helix_<robot>.npz: the 40-digit truth of tests/golden/make_fk_truth.py (same model, same
E_ref and E_design, same array layout) for the 256 states per robot of tests/test_gpu_rhs_helix.py -- the robots whose routing is
a uniform helix (one pitch, one radius): BASELINE config 2, three straight tendons, a 4-tendon helix with a common pitch, one
helical tendon, all at dL = L / 128.  States: seeded U[0, max_tension) rows, then the corners -- all tensions 0, all at the
maximum, one tendon at the maximum with the others 0.  The rows are padded to whole groups of 24 (fk_truth_common.N_STATES, the
size its bounds are written for) with copies of the first rows; `n_states` holds 256.

    python tests/golden/make_fk_truth_helix.py [robot ...]        # needs mpmath and the oracle; ~15 min on 8 cores
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import fk_truth_common as ftc          # noqa: E402
import make_fk_truth as mk             # noqa: E402

KINDS = ("config2", "straight3", "helix4", "helix1")
N_STATES = 256
SEED = 211


def path(kind):
    return os.path.join(ftc.GOLD, "fk_truth_helix_%s.npz" % kind)


def robot(irt, kind):
    if kind == "config2":
        return irt.workloads.robot_config2()
    n, omega = {"straight3": (3, None), "helix4": (4, -3.0), "helix1": (1, 7.0)}[kind]
    C = lambda k: [2 * np.pi * k / n] + ([] if omega is None else [omega])
    tendons = [irt.TendonSpecs(C=C(k), D=[0.01]) for k in range(n)]
    return irt.TendonRobot(tendons=tendons, specs=irt.BackboneSpecs(dL=0.2 / 128))


def states(rb, seed=SEED):
    rng = np.random.default_rng(seed)
    tmax = np.array([t.max_tension for t in rb.tendons])
    N = len(tmax)
    corners = [np.zeros(N), tmax.copy()]
    for j in range(N):
        c = np.zeros(N)
        c[j] = tmax[j]
        corners.append(c)
    st = np.vstack([rng.uniform(0.0, 1.0, (N_STATES - len(corners), N)) * tmax, np.array(corners)])
    assert st.shape == (N_STATES, N)
    return np.ascontiguousarray(st)


def prepare(kind):
    irt = mk._irt()
    rb = robot(irt, kind)
    st = states(rb)
    st = np.ascontiguousarray(np.vstack([st, st[:(-len(st)) % ftc.N_STATES]]))
    M = len(st)
    orb = mk.oracle_robot(rb)
    shapes = [orb.shape(s) for s in st]
    sp = rb.specs
    C = np.array([t.C for t in rb.tendons], np.float64)
    D = np.array([t.D for t in rb.tendons], np.float64)
    consts = np.array([sp.L, sp.dL, sp.ro, sp.ri, sp.E, sp.nu, rb.r, rb.residual_threshold, 0.0, 0.0])
    steps = [mk.step_list(s["t"], sp.dL) for s in shapes]
    n_points = np.array([len(s["t"]) for s in shapes], np.int32)
    idxs = [mk.stored_idx(int(n), int(n_points.max())) for n in n_points]
    K, Q = max(len(s) for s in steps), max(len(i) for i in idxs)
    fx = dict(states=st, n_states=np.array(N_STATES), C=C, D=D, consts=consts, max_tension=np.array([t.max_tension for t in rb.tendons]),
              converged=np.array([bool(s["converged"]) for s in shapes]),
              steps=np.full((M, K, 2), np.nan), n_steps=np.array([len(s) for s in steps], np.int32),
              step_row=np.full((M, K), -1, np.int32), n_points=n_points, pt_idx=np.full((M, Q), -1, np.int32),
              v0=np.array([s["v_i"] for s in shapes]), u0=np.array([s["u_i"] for s in shapes]))
    tasks = []
    for i, (s, sl, idx) in enumerate(zip(shapes, steps, idxs)):
        fx["steps"][i, :len(sl)] = np.array([(t, h) for t, h, _ in sl]).reshape(-1, 2)
        fx["step_row"][i, :len(sl)] = [r for _, _, r in sl]
        fx["pt_idx"][i, :len(idx)] = idx
        tasks.append((consts, C, D, st[i], s["v_i"], s["u_i"], sl, idx, s["p"], s["R"][-1], s["L"], s["L_i"], s["t"], None))
    return fx, tasks


def assemble(kind, fx, results):
    M, Q = fx["pt_idx"].shape
    fx["p_hi"] = np.zeros((M, Q, 3)); fx["p_lo"] = np.zeros((M, Q, 3), np.float32)
    for i, r in enumerate(results):
        q = len(r["p_hi"]) // 3
        fx["p_hi"][i, :q] = r["p_hi"].reshape(q, 3)
        fx["p_lo"][i, :q] = r["p_lo"].reshape(q, 3)
    for key in ("R_hi", "R_lo", "Li_hi", "Li_lo", "Eref_Li", "Edes_Li"):
        fx[key] = np.stack([r[key] for r in results])
    for key in ("L_hi", "L_lo"):
        fx[key] = np.array([r[key][0] for r in results])
    for key in ("Eref_p", "Eref_R", "Eref_L", "Edes_p", "Edes_R", "Edes_L"):
        fx[key] = np.array([r[key] for r in results], np.float64)
    mk.save_npz(path(kind), fx)
    print("%-10s %d states (%d converged), E_ref p %.2g .. %.2g, E_design p %.2g .. %.2g, %.0f s of model runs, %d KB" %
          (kind, M, int(fx["converged"].sum()), fx["Eref_p"].min(), fx["Eref_p"].max(), fx["Edes_p"].min(), fx["Edes_p"].max(),
           sum(r["seconds"] for r in results), os.path.getsize(path(kind)) // 1024), flush=True)


def main(kinds):
    from concurrent.futures import ProcessPoolExecutor
    t0 = time.time()
    prepared = [(k,) + prepare(k) for k in kinds]
    with ProcessPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        futures = [(k, fx, [pool.submit(mk.state_task, t) for t in tasks]) for k, fx, tasks in prepared]
        for k, fx, fs in futures:
            assemble(k, fx, [f.result() for f in fs])
    print("generated %d fixtures in %.0f s" % (len(kinds), time.time() - t0))


if __name__ == "__main__":
    main(sys.argv[1:] or list(KINDS))
