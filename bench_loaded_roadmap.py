#!/usr/bin/env python3
"""A roadmap built under load on one MI355X (RoadmapBuilder.create_roadmap after set_loads; not part of the driver's bench.py).
Config 2's robot at dL = L / 40, as bench_loaded_edges.py takes it, under the gravity of a 50 g robot (f_e = 2.4525 N/m downwards in
the world frame) among spheres on a 64^3 grid over +-0.25 m; 2^11 vertices, 10 nearest neighbours.  One process alternates, --reps
times: create_roadmap with the loads set, create_roadmap without.  There is no pass mark: the figure is ms per build and its ratio to
the unloaded build of the same run.  Prints one JSON object and writes it to --out:

  loaded / unloaded   ms_per_build (median), ms_per_build_min_max, phases_ms (median per phase: vertices, knn_gpu, connect,
                      vertex_caches), candidates, candidate_edges, edges, vertex_blocks, edge_blocks
  loaded              vertex_phase and edge_phase: samples, levels, rounds (Levenberg-Marquardt rounds = host synchronisations of the
                      shooting), chunks, n_integrations, n_unconverged
  ratio_loaded_to_unloaded, vertices_in_common

    python bench_loaded_roadmap.py [--reps 5] [--vertices 2048] [--k 10] [--out profiles/r16/loaded_roadmap_v1.json]
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

DIST = np.array([0.0, -2.4525, 0.0, 0.0, 0.0, 0.0])
PHASES = ("vertices", "knn_gpu", "connect", "vertex_caches")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--vertices", type=int, default=1 << 11)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16", "loaded_roadmap_v1.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_loaded_roadmap.py needs a GPU: there is no CPU path to time")
    irt = importlib.import_module("interactive-rate-tendons_amd")
    irt.build()
    W = irt.workloads
    robot = W.robot_config2()
    robot.specs.dL = robot.specs.L / 40
    vox, _ = W.reach_environment(seed=7, n_spheres=48, N=64)
    chk = irt.VoxelBackboneValidityChecker(robot, irt.VoxelEnvironment(), vox)
    builder = irt.RoadmapBuilder(chk, irt.VoxelBackboneMotionValidator(chk), seed=0, tau_max=15.0)

    def build(loaded):
        if loaded:
            chk.set_loads(dist=DIST, frame="world")
        else:
            chk.clear_loads()
        builder.timing = {}
        prm, road = builder.create_roadmap(args.vertices, k=args.k, device=True)
        torch.cuda.synchronize()
        t = dict(builder.timing)
        prm.close()
        return t, road

    build(True); build(False)                                                 # warm-up: pools, workspaces, code objects
    runs = {"loaded": [], "unloaded": []}
    roads = {}
    for _ in range(args.reps):                                                # alternated: both see the same machine
        for key in ("loaded", "unloaded"):
            t, road = build(key == "loaded")
            runs[key].append(t); roads[key] = road
    out = {"bench": "loaded_roadmap", "robot": "config2, dL = L/40", "grid": "64^3 over +-0.25 m, 48 spheres", "vertices": args.vertices,
           "k": args.k, "reps": args.reps, "loads": "f_e = (0, -2.4525, 0) N/m, world frame, cold start"}
    for key in ("loaded", "unloaded"):
        tot = [1e3 * t["create_roadmap"]["seconds"] for t in runs[key]]
        last, road = runs[key][-1], roads[key]
        out[key] = {"ms_per_build": float(np.median(tot)), "ms_per_build_min_max": [min(tot), max(tot)],
                    "phases_ms": {p: float(np.median([1e3 * t[p]["seconds"] for t in runs[key]])) for p in PHASES},
                    "candidates": int(last["vertices"]["candidates"]), "candidate_edges": int(last["create_roadmap"]["candidate_edges"]),
                    "edges": int(last["create_roadmap"]["edges"]), "vertex_blocks": int(road["vertex_caches"]["offsets"][-1]),
                    "edge_blocks": int(road["edge_caches"]["offsets"][-1])}
    for name, src in (("vertex_phase", "vertices_loaded"), ("edge_phase", "edges_loaded")):
        out["loaded"][name] = {k: int(v) for k, v in runs["loaded"][-1][src].items()}
    out["ratio_loaded_to_unloaded"] = out["loaded"]["ms_per_build"] / out["unloaded"]["ms_per_build"]
    a, b = roads["loaded"]["states"], roads["unloaded"]["states"]
    out["vertices_in_common"] = int(len(set(map(bytes, a)) & set(map(bytes, b))))
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
