#!/usr/bin/env python3
"""Loaded edges on one MI355X (tr_validate_edges_loaded; not part of the driver's bench.py).  Config 2's robot at dL = L / 40, as
bench_loaded_fk.py takes it, under the gravity of a 50 g robot (f_e = 2.4525 N/m downwards in the world frame); 2^11 states that are
valid under that load among spheres on a 64^3 grid over +-0.25 m (7.8 mm voxels: the finest power of two the backbone checker accepts
for this dL), their 10 nearest neighbours' edges.  One process alternates, --reps times: the loaded check cold, the loaded check with
warm start, the unloaded tr_validate_edges on the same edges.  Prints one JSON object and writes it to --out:

  cold / warm     ms_per_call (median), ms_per_call_min_max, edges_per_s, integrations_per_sample (n_integrations over the samples
                  evaluated), samples, levels, rounds (Levenberg-Marquardt rounds = host synchronisations of the shooting), chunks,
                  valid, n_unconverged
  unloaded        ms_per_call, edges_per_s, valid
  verdicts_differ_cold_warm, verdicts_differ_loaded_unloaded

    python bench_loaded_edges.py [--reps 5] [--states 2048] [--out profiles/r15/loaded_edges_v1.json]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

DIST = np.array([0.0, -2.4525, 0.0, 0.0, 0.0, 0.0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--states", type=int, default=1 << 11)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15", "loaded_edges_v1.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_loaded_edges.py needs a GPU: there is no CPU path to time")
    irt = importlib.import_module("interactive-rate-tendons_amd")
    irt.build()
    W = irt.workloads
    robot = W.robot_config2()
    robot.specs.dL = robot.specs.L / 40
    vox, _ = W.reach_environment(seed=7, n_spheres=48, N=64)
    chk = irt.VoxelBackboneValidityChecker(robot, irt.VoxelEnvironment(), vox)
    eng = chk.engine
    cand = W.random_states(robot, 4 * args.states, seed=31, tau_max=15.0)
    ok = eng.validate_loaded(cand, dist=DIST)["valid"]
    states = np.ascontiguousarray(cand[ok][:args.states])
    if len(states) < args.states:
        raise SystemExit("only %d of %d candidates are valid under the load" % (len(states), len(cand)))
    edges = eng.knn_edges(states, 11)                                         # k counts the vertex itself: 10 neighbours
    a, b = np.ascontiguousarray(states[edges[:, 0]]), np.ascontiguousarray(states[edges[:, 1]])
    E = len(edges)

    def loaded(warm):
        t0 = time.perf_counter()
        r = eng.validate_edges_loaded(a, b, dist=DIST, frame="world", warm_start=warm)      # (returns after the last device synchronise)
        return time.perf_counter() - t0, r, eng.edges_loaded_last()

    def unloaded():
        t0 = time.perf_counter()
        r = eng.validate_edges(a, b)
        return time.perf_counter() - t0, r

    loaded(False); loaded(True); unloaded()                                   # warm-up: pools, workspaces, code objects
    t = {"cold": [], "warm": [], "unloaded": []}
    last = {}
    for _ in range(args.reps):                                                # alternated: all three see the same machine
        for key, warm in (("cold", False), ("warm", True)):
            dt, r, how = loaded(warm)
            t[key].append(dt); last[key] = (r, how)
        dt, r = unloaded()
        t["unloaded"].append(dt); last["unloaded"] = (r, None)
    out = {"bench": "loaded_edges", "robot": "config2, dL = L/40", "grid": "64^3 over +-0.25 m, 48 spheres", "states": len(states), "edges": E,
           "reps": args.reps}
    for key in ("cold", "warm"):
        r, how = last[key]
        med = float(np.median(t[key]))
        out[key] = {"ms_per_call": 1e3 * med, "ms_per_call_min_max": [1e3 * min(t[key]), 1e3 * max(t[key])], "edges_per_s": E / med,
                    "integrations_per_sample": r["n_integrations"] / max(1, how["samples"]), "n_integrations": r["n_integrations"],
                    "samples": how["samples"], "levels": how["levels"], "rounds": how["rounds"], "chunks": how["chunks"],
                    "valid": int(r["valid"].sum()), "n_unconverged": r["n_unconverged"], "n_domain_errors": r["n_domain_errors"]}
    med = float(np.median(t["unloaded"]))
    out["unloaded"] = {"ms_per_call": 1e3 * med, "ms_per_call_min_max": [1e3 * min(t["unloaded"]), 1e3 * max(t["unloaded"])], "edges_per_s": E / med,
                       "valid": int(last["unloaded"][0]["valid"].sum())}
    out["verdicts_differ_cold_warm"] = int((last["cold"][0]["valid"] != last["warm"][0]["valid"]).sum())
    out["verdicts_differ_loaded_unloaded"] = int((last["cold"][0]["valid"] != last["unloaded"][0]["valid"]).sum())
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
