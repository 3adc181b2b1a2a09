#!/usr/bin/env python3
"""The loaded tip Jacobian on one MI355X (tr_tip_jacobian_loaded; not part of the driver's bench.py).  Config 2's robot at
dL = L / 40 under the gravity of a 50 g robot (f_e = 2.4525 N/m downwards, fixed in the world frame), 2^12 seeded states.  Three
ways alternate in one process, --reps times each:

  loaded     tr_tip_jacobian_loaded on all states (J and the compliance): one shooting solve and 13 + 2 S integrations per state
  composed   central differences of the tips of 2 S + 1 cold fk_loaded_batch solves per state, differenced on the host (what a
             caller had to do before), on the first --composed of the states
  unloaded   tr_tip_jacobian on the same states at zero load

Writes one JSON object (also to --out): ms per call, integrations per state, rounds, and how far the composed Jacobian lies from
the loaded one.

    python bench_loaded_jacobian.py [--reps 5] [--n 4096] [--composed 64] [--out profiles/r21/loaded_jacobian_v1.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=1 << 12)
    ap.add_argument("--composed", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21", "loaded_jacobian_v1.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_loaded_jacobian.py needs a GPU: there is no CPU path to time")
    irt = importlib.import_module("interactive-rate-tendons_amd")
    irt.build()
    W = irt.workloads
    robot = W.robot_config2()
    robot.specs.dL = robot.specs.L / 40
    eng = robot.engine(0)
    n, S = args.n, eng.state_size
    gravity = np.array([0.0, -2.4525, 0.0, 0.0, 0.0, 0.0])
    st = W.random_states(robot, n, seed=31, tau_max=15.0)
    m = min(args.composed, n)
    d = np.maximum(np.abs(1e-4 * st[:m]), 1e-6)
    pert = np.repeat(st[:m, None, :], 2 * S + 1, axis=1)
    k = np.arange(S)
    pert[:, 1 + 2 * k, k] -= d
    pert[:, 2 + 2 * k, k] += d
    pert = np.ascontiguousarray(pert.reshape(-1, S))

    def composed():
        w, dd = eng.sample_loads(pert, None, gravity, "world")
        out = eng.fk_loaded_batch(pert, w, dd)
        tips = out["p"][:, -1].reshape(m, 2 * S + 1, 3)
        J = np.transpose((tips[:, 2::2] - tips[:, 1::2]) * (0.5 / d)[:, :, None], (0, 2, 1))
        return dict(J=J, integrations=int(out["num_fk_calls"].sum()) + len(pert), rounds=out["rounds"], converged=out["converged"])

    runs = {"loaded": lambda: eng.tip_jacobian_loaded(st, dist=gravity, frame="world", want=("compliance",)),
            "composed": composed,
            "unloaded": lambda: eng.tip_jacobian(st)}
    last, times = {}, {key: [] for key in runs}
    for key, f in runs.items():                                                # warm-up: workspaces, code objects
        last[key] = f()
    for _ in range(args.reps):                                                 # alternated: all see the same machine
        for key, f in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[key] = f()
            torch.cuda.synchronize()
            times[key].append(time.perf_counter() - t0)
    ms = {key: 1e3 * float(np.median(v)) for key, v in times.items()}
    span = lambda key: [1e3 * min(times[key]), 1e3 * max(times[key])]
    lo, co = last["loaded"], last["composed"]
    gap = np.abs(co["J"] - lo["J"][:m]).max(axis=(1, 2)) / np.abs(lo["J"][:m]).max(axis=(1, 2))
    res = {"bench": "loaded_jacobian", "robot": "config2, dL = L/40, 50 g under gravity (world frame)", "states": n, "state_size": S,
           "reps": args.reps,
           "loaded": {"ms_per_call": ms["loaded"], "ms_min_max": span("loaded"), "us_per_state": 1e3 * ms["loaded"] / n,
                      "integrations_per_state": float(lo["n_integrations"].mean()), "shoot_rounds": lo["rounds"],
                      "equilibrium": float(lo["equilibrium"].mean())},
           "composed": {"states": m, "ms_per_call": ms["composed"], "ms_min_max": span("composed"), "us_per_state": 1e3 * ms["composed"] / m,
                        "integrations_per_state": co["integrations"] / m, "shoot_rounds": co["rounds"],
                        "converged": float(co["converged"].mean()), "worst_relative_gap_to_loaded_J": float(gap.max()),
                        "median_relative_gap_to_loaded_J": float(np.median(gap))},
           "unloaded": {"ms_per_call": ms["unloaded"], "ms_min_max": span("unloaded"), "us_per_state": 1e3 * ms["unloaded"] / n,
                        "fk_calls_per_state": 2 * S + 1},
           "loaded_over_unloaded_per_state": ms["loaded"] / ms["unloaded"],
           "composed_over_loaded_per_state": (ms["composed"] / m) / (ms["loaded"] / n),
           "source_hash": irt._lib.source_hash()}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
