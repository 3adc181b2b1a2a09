#!/usr/bin/env python3
"""Loaded FK of a robot WITH retraction on one MI355X (tr_fk_loaded_batch_dev; not part of the driver's bench.py).  bench_loaded_fk.py's
problem: config 2's robot at dL = L / 40, 2^14 states, each under the gravity of a 50 g robot (f_e = 2.4525 N/m) plus a seeded tip
force of at most 0.1 N, device tensors in and out.  Four ways alternate --reps times in one process, so that all see the same machine:

  off       retraction disabled: fk_loaded_uniform (the yardstick -- before the retraction kernel there was nothing else to compare with)
  zero      retraction enabled, s_start = 0 everywhere: fk_loaded_retract on the SAME problems (the cost of the per-lane prologue and
            of the tip-aligned loop)
  uniform   s_start ~ U[0, 0.6 L]
  sorted    the states of `uniform` ordered by s_start by the caller (a wave then holds backbones of one length)

Per way: ms per call, median (min to max); integrations per problem (sum of fk_calls_out plus the output launch, over the problems);
rounds; converged count.  Prints one JSON object and, with --out, writes it to a file.

    python bench_loaded_retraction.py [--reps 5] [--n 16384] [--out profiles/r29/loaded_retraction_v1.json]
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
    ap.add_argument("--n", type=int, default=1 << 14)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_loaded_retraction.py needs a GPU: there is no CPU path to time")
    irt = importlib.import_module("interactive-rate-tendons_amd")
    irt.build()
    W = irt.workloads
    n, dev = args.n, "cuda:0"

    def robot(retraction):
        r = W.robot_config2()
        r.specs.dL = r.specs.L / 40
        r.enable_retraction = retraction
        return r

    plain, ret = robot(False), robot(True)
    st = W.random_states(plain, n, seed=21, tau_max=15.0)
    rng = np.random.default_rng(22)
    d = rng.normal(size=(n, 3))
    wrench = np.zeros((n, 6))
    wrench[:, :3] = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.0, 0.1, (n, 1))
    dist = np.array([0.0, -2.4525, 0.0, 0.0, 0.0, 0.0])
    s_start = np.random.default_rng(23).uniform(0.0, 0.6 * plain.specs.L, n)
    order = np.argsort(s_start, kind="stable")
    with_s = lambda s: np.ascontiguousarray(np.hstack([st, np.asarray(s, float).reshape(n, 1)]))
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    ld = (n + 63) // 64 * 64
    ways = {}
    for name, rob, states, w in (("off", plain, st, wrench), ("zero", ret, with_s(np.zeros(n)), wrench), ("uniform", ret, with_s(s_start), wrench),
                                 ("sorted", ret, with_s(s_start)[order], wrench[order])):
        eng = rob.engine(0)
        eng.set_loaded_retraction()                                           # (no effect on the robot without retraction)
        P, N = eng.num_points, eng.n_tendons
        ways[name] = dict(eng=eng, st=up(states), w=up(w), d=up(dist), planes=torch.empty((3, P, ld), dtype=torch.float64, device=dev),
                          Li=torch.empty((N, ld), dtype=torch.float64, device=dev), conv=torch.empty(n, dtype=torch.uint8, device=dev),
                          calls=torch.empty(n, dtype=torch.int32, device=dev), npts=torch.empty(n, dtype=torch.int32, device=dev), t=[], rounds=0)

    def run(x):
        x["rounds"] = x["eng"].fk_loaded_batch_dev(x["st"], n, ld, x["planes"][0], x["planes"][1], x["planes"][2], d_wrench=x["w"], wrench_ld=6,
                                                   d_dist=x["d"], dist_ld=0, d_Li=x["Li"], d_conv=x["conv"], d_npts=x["npts"], d_fk_calls=x["calls"])
        torch.cuda.synchronize()

    for x in ways.values():
        run(x)                                                                # warm-up: workspaces, code objects
    for _ in range(args.reps):                                                # alternated
        for x in ways.values():
            t0 = time.perf_counter()
            run(x)
            x["t"].append(time.perf_counter() - t0)
    out = {"bench": "loaded_retraction", "robot": "config2, dL = L/40", "problems": n, "reps": args.reps, "note": "one run, one box", "ways": {}}
    for name, x in ways.items():
        t = np.array(x["t"])
        out["ways"][name] = {"ms_per_call": 1e3 * float(np.median(t)), "ms_per_call_min_max": [1e3 * float(t.min()), 1e3 * float(t.max())],
                             "integrations_per_problem": (int(x["calls"].sum().item()) + n) / n, "rounds": x["rounds"],
                             "converged": int(x["conv"].sum().item()), "mean_points": float(x["npts"].float().mean().item())}
    u, s = out["ways"]["uniform"], out["ways"]["sorted"]
    out["sorted_gain_ms"] = u["ms_per_call"] - s["ms_per_call"]
    out["uniform_spread_ms"] = u["ms_per_call_min_max"][1] - u["ms_per_call_min_max"][0]
    text = json.dumps(out)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
