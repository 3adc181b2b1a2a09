#!/usr/bin/env python3
"""Tip IK on loaded shapes on one MI355X (tr_ik_loaded_batch; not part of the driver's bench.py).  Config 2's robot at dL = L / 40
under the gravity of a 50 g robot (f_e = 2.4525 N/m downwards, fixed in the world frame), 2^12 goals that are reachable by
construction: the loaded tips of seeded states; the starts are those states plus seeded normal offsets of 2 N (and 0.2 rad, 2 mm where
the robot has such entries), clipped to the bounds.  Three solvers alternate in one process, --reps times each:

  loaded     tr_ik_loaded_batch on all problems
  unloaded   tr_ik_batch on the same starts at zero load (goals: the unloaded tips of the same states)
  composed   tip_control.inverse_kinematics_batch with fk_loaded_batch as its FK (every difference through a shooting solve, the
             reference's way) on the first --composed of the problems

Writes one JSON object (also to --out): ms per call, integrations per problem, outer and shooting rounds, the share reached.

    python bench_loaded_ik.py [--reps 5] [--n 4096] [--composed 64] [--out profiles/r17/loaded_ik_v1.json]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17", "loaded_ik_v1.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_loaded_ik.py needs a GPU: there is no CPU path to time")
    irt = importlib.import_module("interactive-rate-tendons_amd")
    irt.build()
    W, tc = irt.workloads, irt.tip_control
    robot = W.robot_config2()
    robot.specs.dL = robot.specs.L / 40
    eng = robot.engine(0)
    n, N, S = args.n, eng.n_tendons, eng.state_size
    gravity = np.array([0.0, -2.4525, 0.0, 0.0, 0.0, 0.0])
    at = W.random_states(robot, n, seed=31, tau_max=15.0)
    b = tc.Bounds.from_robot(robot)
    rng = np.random.default_rng(32)
    off = rng.normal(size=at.shape) * 2.0
    if robot.enable_rotation:
        off[:, N] *= 0.1
    if robot.enable_retraction:
        off[:, -1] *= 1e-3
    starts = np.clip(at + off, b.lower, b.upper)
    there = eng.fk_loaded_batch(at, *eng.sample_loads(at, None, gravity, "world"))
    keep = there["converged"]
    goals_loaded = np.ascontiguousarray(there["p"][:, -1])
    goals_unloaded, _ = eng.fk_tips(at)
    m = min(args.composed, n)

    def loaded_fk(states):
        w, d = eng.sample_loads(states, None, gravity, "world")
        return eng.fk_loaded_batch(states, w, d)

    fk_lanes = [0]

    def loaded_tips(states):
        out = loaded_fk(states)
        fk_lanes[0] += int(out["num_fk_calls"].sum()) + len(states)
        return out["p"][:, -1]

    runs = {"loaded": lambda: eng.ik_loaded_batch(starts, goals_loaded, dist=gravity, frame="world"),
            "unloaded": lambda: eng.ik_batch(starts, goals_unloaded),
            "composed": lambda: tc.inverse_kinematics_batch(robot, starts[:m], goals_loaded[:m], fk=loaded_tips)}
    last, times = {}, {k: [] for k in runs}
    for k, f in runs.items():                                                  # warm-up: workspaces, code objects
        last[k] = f()
    for _ in range(args.reps):                                                 # alternated: all see the same machine
        for k, f in runs.items():
            fk_lanes[0] = 0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[k] = f()
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t0)
    ms = {k: 1e3 * float(np.median(v)) for k, v in times.items()}
    lo, un, co = last["loaded"], last["unloaded"], last["composed"]
    # the loaded answers, checked by the loaded FK itself (cold)
    back = loaded_fk(lo["state"])
    miss = np.linalg.norm(back["p"][:, -1] - goals_loaded, axis=1)
    res = {"bench": "loaded_ik", "robot": "config2, dL = L/40, 50 g under gravity (world frame)", "problems": n, "state_size": S,
           "reps": args.reps, "goals_from_converged_states": float(keep.mean()),
           "loaded": {"ms_per_call": ms["loaded"], "ms_min_max": [1e3 * min(times["loaded"]), 1e3 * max(times["loaded"])],
                      "us_per_problem": 1e3 * ms["loaded"] / n, "integrations_per_problem": float(lo["num_fk_calls"].mean()),
                      "outer_rounds": lo["rounds"], "shoot_rounds": lo["shoot_rounds"], "mean_iters": float(lo["iters"].mean()),
                      "max_iters": int(lo["iters"].max()), "equilibrium": float(lo["equilibrium"].mean()),
                      "reached": float((lo["error"] <= 1e-4).mean()),
                      "reached_by_cold_loaded_fk_within_2e-4": float(((miss <= 2e-4) & back["converged"]).mean())},
           "unloaded": {"ms_per_call": ms["unloaded"], "us_per_problem": 1e3 * ms["unloaded"] / n,
                        "fk_calls_per_problem": float(un["num_fk_calls"].mean()), "rounds": un["rounds"],
                        "mean_iters": float(un["iters"].mean()), "reached": float((un["error"] <= 1e-4).mean())},
           "composed": {"problems": m, "ms_per_call": ms["composed"], "us_per_problem": 1e3 * ms["composed"] / m,
                        "integrations_per_problem": fk_lanes[0] / m, "fk_batches": co["launches"],
                        "mean_iters": float(co["iters"].mean()), "reached": float((co["error"] <= 1e-4).mean())},
           "loaded_over_unloaded_per_problem": ms["loaded"] / ms["unloaded"],
           "composed_over_loaded_per_problem": (ms["composed"] / m) / (ms["loaded"] / n),
           "source_hash": irt._lib.source_hash()}
    text = json.dumps(res)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
