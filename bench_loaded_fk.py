#!/usr/bin/env python3
"""Loaded FK on one MI355X (tr_fk_loaded_batch_dev; not part of the driver's bench.py).  Config 2's robot at dL = L / 40, 2^14 states,
each under the gravity of a 50 g robot (f_e = 2.4525 N/m downwards in the world frame) plus a seeded tip force of at most 0.1 N.
Prints one JSON object:

  ms_per_call, rounds, loaded_fk_per_s      the whole call on device tensors (median of --reps)
  lane_integrations, ns_per_lane_loaded     integrations of the call (sum of fk_calls_out plus the output launch) and the call's
                                            time over them
  ns_per_lane_tips                          tr_fk_tips_dev on the same number of lanes, alternated with the loaded call in one process
  lane_ratio                                the two per-lane times' ratio: what the load terms, the residual and the rounds' host
                                            synchronisations cost per integration

    python bench_loaded_fk.py [--reps 7] [--n 16384]
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
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--n", type=int, default=1 << 14)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_loaded_fk.py needs a GPU: there is no CPU path to time")
    irt = importlib.import_module("interactive-rate-tendons_amd")
    irt.build()
    W = irt.workloads
    robot = W.robot_config2()
    robot.specs.dL = robot.specs.L / 40
    eng = robot.engine(0)
    n, P, N = args.n, eng.num_points, eng.n_tendons
    st = W.random_states(robot, n, seed=21, tau_max=15.0)
    rng = np.random.default_rng(22)
    d = rng.normal(size=(n, 3))
    wrench = np.zeros((n, 6))
    wrench[:, :3] = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.0, 0.1, (n, 1))
    dist = np.array([0.0, -2.4525, 0.0, 0.0, 0.0, 0.0])
    dev = "cuda:0"
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_st, d_w, d_d = up(st), up(wrench), up(dist)
    ld = (n + 63) // 64 * 64
    planes = torch.empty((3, P, ld), dtype=torch.float64, device=dev)
    Li = torch.empty((N, ld), dtype=torch.float64, device=dev)
    conv = torch.empty(n, dtype=torch.uint8, device=dev)
    calls = torch.empty(n, dtype=torch.int32, device=dev)
    iters = torch.empty(n, dtype=torch.int32, device=dev)
    rounds = [0]

    def loaded():
        rounds[0] = eng.fk_loaded_batch_dev(d_st, n, ld, planes[0], planes[1], planes[2], d_wrench=d_w, wrench_ld=6, d_dist=d_d, dist_ld=0,
                                            d_Li=Li, d_conv=conv, d_iters=iters, d_fk_calls=calls)
        torch.cuda.synchronize()

    loaded()                                                                  # warm-up: workspace, code objects
    lanes = int(calls.sum().item()) + n                                       # + the launch that writes the outputs
    tip_states = up(np.tile(st, (lanes // n + 1, 1))[:lanes])
    tips = torch.empty((lanes, 3), dtype=torch.float64, device=dev)

    def unloaded():
        eng.fk_tips_dev(tip_states, lanes, tips)
        torch.cuda.synchronize()

    unloaded()
    t_l, t_u = [], []
    for _ in range(args.reps):                                                # alternated: both see the same machine
        t0 = time.perf_counter(); loaded(); t_l.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); unloaded(); t_u.append(time.perf_counter() - t0)
    tl, tu = float(np.median(t_l)), float(np.median(t_u))
    print(json.dumps({"bench": "loaded_fk", "robot": "config2, dL = L/40", "problems": n, "ms_per_call": 1e3 * tl,
                      "ms_per_call_min_max": [1e3 * min(t_l), 1e3 * max(t_l)], "rounds": rounds[0], "loaded_fk_per_s": n / tl,
                      "converged": float(conv.float().mean().item()), "mean_iters": float(iters.float().mean().item()),
                      "max_iters": int(iters.max().item()), "lane_integrations": lanes, "ns_per_lane_loaded": 1e9 * tl / lanes,
                      "fk_tips_ms": 1e3 * tu, "ns_per_lane_tips": 1e9 * tu / lanes, "lane_ratio": tl / tu}))


if __name__ == "__main__":
    main()
