#!/usr/bin/env python3
"""Loaded edges of a robot WITH retraction on one MI355X (tr_validate_edges_loaded on a context opened with
TR_LOADED_RETRACTION_EDGES; not part of the driver's bench.py).  bench_loaded_edges.py's problem with retraction: config 2's robot at
dL = L / 40 under the gravity of a 50 g robot (f_e = 2.4525 N/m downwards in the world frame), 2^11 states with s_start ~ U[0, 0.6 L]
that are valid under that load among spheres on a 64^3 grid over +-0.25 m, their 10 nearest neighbours' edges, cold start.  One
process alternates three ways, --reps times, so that all see the same machine:

  arrival   the shooting solves every level's samples in arrival order (an engine created under TENDON_HIP_LOADED_RETRACT_SORT=0)
  ordered   ... in the order of their backbone lengths (=1: every level, whatever its size)
  off       the robot WITHOUT retraction on the same tensions and the same edges (the yardstick: fk_loaded_uniform, shared grid)

Per way: ms per call, median (min to max); samples, levels, rounds; integrations per sample; valid edges; unconverged samples.

--fk-sizes: the loaded FK alone (tr_fk_loaded_batch_dev, bench_loaded_retraction.py's `uniform` problem) at those problem counts,
arrival order against the ordered solve, alternating: what the default of TENDON_HIP_LOADED_RETRACT_SORT rests on.  Per size and
way: ms per call, median (min to max); `gain_ms` = arrival - ordered medians, `spread_ms` = arrival's max - min.

    python bench_loaded_retraction_edges.py [--reps 5] [--states 2048] [--fk-sizes 1024,4096,16384] [--out profiles/r30/loaded_retraction_edges_v1.json]
"""
import argparse
import contextlib
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

DIST = np.array([0.0, -2.4525, 0.0, 0.0, 0.0, 0.0])


@contextlib.contextmanager
def env(**values):
    """environment variables while an engine is created (the library reads its switches at context creation)"""
    old = {k: os.environ.get(k) for k in values}
    os.environ.update(values)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def stats(t):
    t = np.asarray(t)
    return {"ms_per_call": 1e3 * float(np.median(t)), "ms_per_call_min_max": [1e3 * float(t.min()), 1e3 * float(t.max())]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--states", type=int, default=1 << 11)
    ap.add_argument("--fk-sizes", default="1024,4096,16384")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r30", "loaded_retraction_edges_v1.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_loaded_retraction_edges.py needs a GPU: there is no CPU path to time")
    irt = importlib.import_module("interactive-rate-tendons_amd")
    irt.build()
    W = irt.workloads

    def robot(retraction):
        r = W.robot_config2()
        r.specs.dL = r.specs.L / 40
        r.enable_retraction = retraction
        return r

    plain, ret = robot(False), robot(True)
    vox, _ = W.reach_environment(seed=7, n_spheres=48, N=64)

    def checker(rob, sort=None):
        with env(**({} if sort is None else {"TENDON_HIP_LOADED_RETRACT_SORT": sort})):
            chk = irt.VoxelBackboneValidityChecker(rob, irt.VoxelEnvironment(), vox)
        chk.engine.set_loaded_retraction(edges=True)                              # (no effect on the robot without retraction)
        return chk

    chks = {"arrival": checker(ret, "0"), "ordered": checker(ret, "1"), "off": checker(plain)}
    # states valid under the load WITH their retraction, the edges of their 10 nearest neighbours
    n_cand = 4 * args.states
    tau = W.random_states(plain, n_cand, seed=31, tau_max=15.0)
    s_start = np.random.default_rng(33).uniform(0.0, 0.6 * plain.specs.L, n_cand)
    cand = np.ascontiguousarray(np.hstack([tau, s_start[:, None]]))
    ok = chks["arrival"].engine.validate_loaded(cand, dist=DIST)["valid"]
    states = np.ascontiguousarray(cand[ok][:args.states])
    if len(states) < args.states:
        raise SystemExit("only %d of %d candidates are valid under the load" % (len(states), len(cand)))
    edges = chks["arrival"].engine.knn_edges(states, 11)                          # k counts the vertex itself: 10 neighbours
    E = len(edges)
    ends = {}
    for key in chks:
        st = states if key != "off" else np.ascontiguousarray(states[:, :-1])
        ends[key] = (np.ascontiguousarray(st[edges[:, 0]]), np.ascontiguousarray(st[edges[:, 1]]))

    def run(key):
        eng = chks[key].engine
        a, b = ends[key]
        t0 = time.perf_counter()
        r = eng.validate_edges_loaded(a, b, dist=DIST, frame="world", warm_start=False)     # (returns after the last device synchronise)
        return time.perf_counter() - t0, r, eng.edges_loaded_last()

    for key in chks:
        run(key)                                                                  # warm-up: pools, workspaces, code objects
    t, last = {k: [] for k in chks}, {}
    for _ in range(args.reps):                                                    # alternated
        for key in chks:
            dt, r, how = run(key)
            t[key].append(dt); last[key] = (r, how)
    out = {"bench": "loaded_retraction_edges", "robot": "config2, dL = L/40", "grid": "64^3 over +-0.25 m, 48 spheres", "states": len(states),
           "edges": E, "reps": args.reps, "note": "one run, one box", "ways": {}}
    for key in chks:
        r, how = last[key]
        out["ways"][key] = dict(stats(t[key]), samples=how["samples"], levels=how["levels"], rounds=how["rounds"], chunks=how["chunks"],
                                integrations_per_sample=r["n_integrations"] / max(1, how["samples"]), valid=int(r["valid"].sum()),
                                n_unconverged=int(r["n_unconverged"]))
    out["verdicts_differ_arrival_ordered"] = int((last["arrival"][0]["valid"] != last["ordered"][0]["valid"]).sum())
    out["ordered_gain_ms"] = out["ways"]["arrival"]["ms_per_call"] - out["ways"]["ordered"]["ms_per_call"]
    out["arrival_spread_ms"] = out["ways"]["arrival"]["ms_per_call_min_max"][1] - out["ways"]["arrival"]["ms_per_call_min_max"][0]

    # ---- the loaded FK alone, arrival order against the ordered solve
    sizes = [int(x) for x in args.fk_sizes.split(",") if x]
    out["fk"] = {}
    dev = "cuda:0"
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    engs = {"arrival": chks["arrival"].engine, "ordered": chks["ordered"].engine}
    for n in sizes:
        st = W.random_states(plain, n, seed=21, tau_max=15.0)
        rng = np.random.default_rng(22)
        d = rng.normal(size=(n, 3))
        wrench = np.zeros((n, 6))
        wrench[:, :3] = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.0, 0.1, (n, 1))
        s = np.random.default_rng(23).uniform(0.0, 0.6 * plain.specs.L, n)
        ld = (n + 63) // 64 * 64
        P, N = engs["arrival"].num_points, engs["arrival"].n_tendons
        x = dict(st=up(np.hstack([st, s[:, None]])), w=up(wrench), d=up(DIST), planes=torch.empty((3, P, ld), dtype=torch.float64, device=dev),
                 Li=torch.empty((N, ld), dtype=torch.float64, device=dev), conv=torch.empty(n, dtype=torch.uint8, device=dev),
                 npts=torch.empty(n, dtype=torch.int32, device=dev))

        def fk(eng):
            t0 = time.perf_counter()
            eng.fk_loaded_batch_dev(x["st"], n, ld, x["planes"][0], x["planes"][1], x["planes"][2], d_wrench=x["w"], wrench_ld=6, d_dist=x["d"],
                                    dist_ld=0, d_Li=x["Li"], d_conv=x["conv"], d_npts=x["npts"])
            torch.cuda.synchronize()
            return time.perf_counter() - t0

        for eng in engs.values():
            fk(eng)
        tt = {k: [] for k in engs}
        for _ in range(args.reps):
            for k, eng in engs.items():
                tt[k].append(fk(eng))
        assert engs["ordered"].loaded_order_last()["ordered"] == n and engs["arrival"].loaded_order_last()["ordered"] == 0
        row = {k: stats(v) for k, v in tt.items()}
        row["gain_ms"] = row["arrival"]["ms_per_call"] - row["ordered"]["ms_per_call"]
        row["spread_ms"] = row["arrival"]["ms_per_call_min_max"][1] - row["arrival"]["ms_per_call_min_max"][0]
        row["converged"] = int(x["conv"].sum().item())
        out["fk"][str(n)] = row
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
