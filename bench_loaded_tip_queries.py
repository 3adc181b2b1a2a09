#!/usr/bin/env python3
"""Tip-goal queries on loaded shapes on one MI355X (VoxelCachedLazyPRM.roadmap_ik_loaded_batch; not part of the driver's bench.py).
bench_loaded_roadmap.py's setup: config 2's robot at dL = L / 40 under the gravity of a 50 g robot (f_e = 2.4525 N/m downwards in the
world frame) among spheres on a 64^3 grid over +-0.25 m, 2^11 vertices, 10 nearest neighbours, built by create_roadmap under that load.
Requests: half near vertex tips (3 mm of noise), half anywhere in the workspace.  Per batch size Q and connection rule (connect_k 0 and
10), k = 5, one process alternates --reps times:
    the loaded call on the loaded roadmap;
    (a) the unloaded roadmap_ik_batch on the unloaded roadmap of the same seed;
    (b) at Q = 64 only: the per-request loop over the single loaded pieces (nearest_tips, ik_loaded_batch, nearest_states,
        validate_edges_loaded with last_valid, the interpolation, fk_loaded_tips), which is what a caller had before this call.
There is no pass mark.  Prints one JSON object and writes it to --out; per (Q, connect_k):
    loaded_ms / unloaded_ms / loop_ms   median, [min, max]
    phases_ms (medians: nearest, ik, edges, select), ik_rounds, integrations_per_request, counts (pairs checked, IK answers without an
    equilibrium, last valid states unconverged, integrations), outcomes (reached, closest, no neighbour) of both calls

    python bench_loaded_tip_queries.py [--reps 5] [--sizes 64,1024,4096] [--out profiles/r25/loaded_tip_queries_v1.json]
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
K = 5


def requests_of(tips, n, seed):
    rng = np.random.default_rng(seed)
    req = tips[rng.integers(0, len(tips), n)] + rng.normal(size=(n, 3)) * 0.003
    req[n // 2:] = rng.uniform(-0.12, 0.12, (n - n // 2, 3)) + np.array([0.0, 0.0, 0.1])
    return np.ascontiguousarray(req)


def piece_loop(irt, prm, mv, requests, kc):
    """(b): one request at a time over the single loaded pieces (no selection: the device work is what is timed)"""
    eng, states = prm.engine, prm.states
    res = dict(min_tension_change=mv.min_tension_change, min_rotation_change=mv.min_rotation_change, min_retraction_change=mv.min_retraction_change)
    for r in requests:
        N, _ = prm.nearest_tips(r, K)
        iv = N[0][N[0] >= 0]
        if len(iv) == 0:
            continue
        ik = eng.ik_loaded_batch(states[iv], r, dist=DIST, frame="world")
        src, slot = list(iv), list(range(len(iv)))
        if kc:
            Cn, _ = prm.nearest_states(ik["state"], kc)
            src, slot = [], []
            for i in range(len(iv)):
                s = [int(v) for v in Cn[i] if v >= 0]
                if iv[i] not in s:
                    s.append(int(iv[i]))
                src += s; slot += [i] * len(s)
        a, b = states[src], ik["state"][slot]
        ev = eng.validate_edges_loaded(a, b, dist=DIST, frame="world", warm_start=False, last_valid=True, **res)
        g = irt.roadmap.interpolate_states(eng, a, b, ev["last_valid_t"])
        eng.fk_loaded_tips(g, dist=DIST, frame="world")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="64,1024,4096")
    ap.add_argument("--connect", default="0,10")
    ap.add_argument("--vertices", type=int, default=1 << 11)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r25", "loaded_tip_queries_v1.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_loaded_tip_queries.py needs a GPU: there is no CPU path to time")
    irt = importlib.import_module("interactive-rate-tendons_amd")
    irt.build()
    W = irt.workloads
    robot = W.robot_config2()
    robot.specs.dL = robot.specs.L / 40
    vox, _ = W.reach_environment(seed=7, n_spheres=48, N=64)
    chk = irt.VoxelBackboneValidityChecker(robot, irt.VoxelEnvironment(), vox)
    mv = irt.VoxelBackboneMotionValidator(chk)
    builder = irt.RoadmapBuilder(chk, mv, seed=0, tau_max=15.0)
    chk.set_loads(dist=DIST, frame="world")
    prm_l, road_l = builder.create_roadmap(args.vertices, k=10, device=True)
    chk.clear_loads()                                                         # (the explicit-load calls do not read the checker's loads)
    prm_u, road_u = builder.create_roadmap(args.vertices, k=10, device=True)
    loads = dict(dist=DIST, frame="world")

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = f()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0), r

    stat = lambda xs: {"median": float(np.median(xs)), "min_max": [float(min(xs)), float(max(xs))]}
    out = {"bench": "loaded_tip_queries", "robot": "config2, dL = L/40", "grid": "64^3 over +-0.25 m, 48 spheres", "vertices": args.vertices,
           "k": K, "reps": args.reps, "loads": "f_e = (0, -2.4525, 0) N/m, world frame, every solve cold", "runs": []}
    for Q in [int(x) for x in args.sizes.split(",")]:
        req_l, req_u = requests_of(road_l["tips"], Q, 5), requests_of(road_u["tips"], Q, 5)
        for kc in [int(x) for x in args.connect.split(",")]:
            call_l = lambda: prm_l.roadmap_ik_loaded_batch(req_l, k=K, motion_validator=mv, connect_k=kc, **loads)
            call_u = lambda: prm_u.roadmap_ik_batch(req_u, k=K, motion_validator=mv, connect_k=kc)
            call_l(); call_u()                                                # warm-up: arenas, workspaces, code objects
            tl, tu, tb, phases, rl, ru = [], [], [], [], None, None
            for _ in range(args.reps):                                        # alternated: all see the same machine
                ms, rl = timed(call_l)
                tl.append(ms); phases.append(prm_l.tip_query_profile())
                ms, ru = timed(call_u)
                tu.append(ms)
                if Q <= 64:
                    ms, _ = timed(lambda: piece_loop(irt, prm_l, mv, req_l, kc))
                    tb.append(ms)
            run = {"Q": Q, "connect_k": kc, "loaded_ms": stat(tl), "unloaded_ms": stat(tu),
                   "ratio_loaded_to_unloaded": float(np.median(tl) / np.median(tu)),
                   "phases_ms": {p: float(np.median([ph[p + "_ms"] for ph in phases])) for p in ("nearest", "ik", "edges", "select")},
                   "ik_rounds": int(phases[-1]["ik_rounds"]), "integrations_per_request": float(rl["counts"][3]) / Q,
                   "counts": [int(x) for x in rl["counts"]],
                   "outcomes_loaded": [int(x) for x in np.bincount(rl["outcome"], minlength=3)],
                   "outcomes_unloaded": [int(x) for x in np.bincount(ru["outcome"], minlength=3)]}
            if tb:
                run["loop_ms"] = stat(tb)
                run["ratio_loop_to_loaded"] = float(np.median(tb) / np.median(tl))
            out["runs"].append(run)
            print(json.dumps(run), file=sys.stderr, flush=True)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
