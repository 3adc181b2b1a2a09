#!/usr/bin/env python3
"""What a load profile costs on one MI355X (tr_set_load_profile; not part of the driver's bench.py).  Config 2's robot at
dL = L / 40, as bench_loaded_fk.py takes it, under the gravity of a 50 g robot (f_e = 2.4525 N/m downwards, base frame):
fk_loaded_batch on 2^14 states and tip_jacobian_loaded on 2^12 states, each with and without a three-knot profile
(0, 0.75 L, L) -> (1, 1, 3), alternating --reps times in one process.  The profile changes the problem as well as the kernel (the
tip section weighs three times as much), so the integrations per problem are reported beside the times.  Prints one JSON object and
writes it to --out:

  fk_loaded_batch / tip_jacobian_loaded   per form (`none`, `profile`): ms_per_call (median), ms_per_call_min_max,
                                          integrations_per_problem, rounds, converged

    python bench_load_profile.py [--reps 5] [--fk-states 16384] [--jacobian-states 4096] [--out profiles/r26/load_profile_v1.json]
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
    ap.add_argument("--fk-states", type=int, default=1 << 14)
    ap.add_argument("--jacobian-states", type=int, default=1 << 12)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r26", "load_profile_v1.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_load_profile.py needs a GPU: there is no CPU path to time")
    irt = importlib.import_module("interactive-rate-tendons_amd")
    irt.build()
    W = irt.workloads
    robot = W.robot_config2()
    robot.specs.dL = robot.specs.L / 40
    L = robot.specs.L
    profile = ([0.0, 0.75 * L, L], [1.0, 1.0, 3.0])
    eng = robot.engine(0)
    fk_states = W.random_states(robot, args.fk_states, seed=31, tau_max=15.0)
    jac_states = np.ascontiguousarray(fk_states[:args.jacobian_states])

    def fk():
        t0 = time.perf_counter()
        r = eng.fk_loaded_batch(fk_states, dist=DIST)                             # (returns after the last device synchronise)
        return time.perf_counter() - t0, dict(integrations_per_problem=float(r["num_fk_calls"].mean()), rounds=int(r["rounds"]),
                                              converged=int(r["converged"].sum()))

    def jac():
        t0 = time.perf_counter()
        r = eng.tip_jacobian_loaded(jac_states, dist=DIST)
        return time.perf_counter() - t0, dict(integrations_per_problem=float(r["n_integrations"].mean()), rounds=int(r["rounds"]),
                                              converged=int(r["equilibrium"].sum()))

    calls = {"fk_loaded_batch": fk, "tip_jacobian_loaded": jac}
    for call in calls.values():                                                   # warm-up: workspaces, both kernel forms
        call()
        with eng.load_profile_scope(profile):
            call()
    times = {name: {"none": [], "profile": []} for name in calls}
    facts = {name: {} for name in calls}
    for _ in range(args.reps):
        for name, call in calls.items():
            for form in ("none", "profile"):
                with eng.load_profile_scope(profile if form == "profile" else None):
                    t, facts[name][form] = call()
                times[name][form].append(t)
    out = dict(robot="config2, dL = L / 40", dist=DIST.tolist(), profile=dict(knots=profile[0], weights=profile[1]), reps=args.reps,
               states={"fk_loaded_batch": len(fk_states), "tip_jacobian_loaded": len(jac_states)}, source=irt._lib.source_hash())
    for name in calls:
        out[name] = {}
        for form in ("none", "profile"):
            ms = np.array(times[name][form]) * 1e3
            out[name][form] = dict(ms_per_call=float(np.median(ms)), ms_per_call_min_max=[float(ms.min()), float(ms.max())], **facts[name][form])
    text = json.dumps(out, indent=1)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
