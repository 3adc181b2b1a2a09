"""The accurate connection rule of the tip queries (RMAP_IK_ACCURATE) on bench_tip_queries.py's roadmap (config 3's robot, 10^5
vertices among the spheres of reach_environment): VoxelCachedLazyPRM.roadmap_ik_batch with connect_k = 0 (one edge per IK answer)
and with connect_k = 10 (an edge from every state-space neighbour of the answer), alternated in one process, and nearest_states
alone -- the source search -- on 5 Q query states.

    python bench_tip_connect.py [--vertices 100000] [--k 5] [--connect-k 10] [--reps 5] [--out profiles/r23/tip_connect_v1.json]

Prints one JSON line (and writes it to --out): per batch size and rule the time per call (min / median / max over the repetitions),
the phases of the median call, the pairs checked and the requests reached / moved to another connection vertex / reached only by
the accurate rule.  No ratio is promised: the accurate rule checks up to connect_k + 1 edges where the plain one checks one, and its
cost is reported against the plain call of the same run.  Needs a GPU."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def spread(ts):
    ts = np.sort(np.asarray(ts))
    return dict(min_ms=1e3 * float(ts[0]), median_ms=1e3 * float(ts[len(ts) // 2]), max_ms=1e3 * float(ts[-1]))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--vertices", type=int, default=100000)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--connect-k", type=int, default=10)
    ap.add_argument("--roadmap-k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="*", default=[64, 1024, 16384])
    ap.add_argument("--out", default="")
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_tip_connect.py needs a GPU")
    irt = importlib.import_module("interactive-rate-tendons_amd")
    W = irt.workloads
    robot = W.robot_config3()
    vox, _ = W.reach_environment(seed=7, n_spheres=64)
    new_vox, _ = W.reach_environment(seed=7, n_spheres=72)
    chk = irt.VoxelBackboneValidityChecker(robot, irt.VoxelEnvironment(), vox)
    mv = irt.VoxelBackboneMotionValidator(chk)
    rb = irt.RoadmapBuilder(chk, mv, seed=11)
    chk.engine.reserve(1 << 20)
    t0 = time.perf_counter()
    prm, rm = rb.create_roadmap(args.vertices, k=args.roadmap_k, device=True)
    t_build = time.perf_counter() - t0
    states, tips = rm["states"], rm["tips"]
    V, k, kc, tol = len(states), args.k, args.connect_k, 1e-4
    prm.set_obstacles(new_vox)                                   # the interactive loop: the environment changed after the build
    nv_bad, ne_bad = prm.revalidate()
    rng = np.random.default_rng(17)
    nmax = max(args.sizes)
    requests = tips[rng.integers(0, V, nmax)] + rng.normal(size=(nmax, 3)) * 0.003
    S = states.shape[1]

    def call(n, connect_k):
        return prm.roadmap_ik_batch(requests[:n], tolerance=tol, k=k, motion_validator=mv, connect_k=connect_k)

    sync = lambda: torch.cuda.synchronize()

    def timed(f, *a):
        sync(); t0 = time.perf_counter(); r = f(*a); sync()
        return time.perf_counter() - t0, r

    def median_profile(ts, profs):
        return profs[int(np.argsort(ts)[len(ts) // 2])]

    for n in args.sizes:                                         # warm-up: every shape of the timed window
        call(n, 0); call(n, kc)
    sizes = {}
    for n in args.sizes:
        ts, profs, res = {0: [], kc: []}, {0: [], kc: []}, {}
        for _ in range(args.reps):                               # alternating, same process
            for c in (0, kc):
                dt, res[c] = timed(call, n, c)
                ts[c].append(dt); profs[c].append(prm.tip_query_profile())
        plain, acc = res[0], res[kc]
        row = {}
        for c, name in ((0, "plain"), (kc, "accurate")):
            row[name] = dict(spread(ts[c]), phases_of_median_call=median_profile(ts[c], profs[c]), requests_per_s=n / float(np.median(ts[c])),
                             outcomes=np.bincount(res[c]["outcome"], minlength=3).tolist())
        st = acc["connect_stats"]
        row["accurate"].update(pairs_checked=st["pairs_checked"], reached=st["reached"], moved=st["moved"], gained=st["gained"])
        row["accurate_over_plain"] = row["accurate"]["median_ms"] / row["plain"]["median_ms"]
        row["plain_reached_stays_reached"] = bool(((acc["outcome"] == 0) | (plain["outcome"] != 0)).all())
        sizes[str(n)] = row

    # nearest_states alone, on device tensors: 5 Q query states (the IK answers of Q requests at k = 5), a run of calls each ending in a
    # stream synchronise; the [S][V] copy of the states is read once per group of stateq_q queries
    knn = {}
    q_states = states[rng.integers(0, V, 5 * nmax)] + rng.normal(size=(5 * nmax, S)) * 0.05
    for n in args.sizes:
        m = 5 * n
        d_q = torch.from_numpy(np.ascontiguousarray(q_states[:m])).cuda()
        d_idx = torch.empty((m, kc), dtype=torch.int32, device="cuda")
        prm.nearest_states_dev(d_q, m, kc, d_idx)
        calls = 20
        sync(); t0 = time.perf_counter()
        for _ in range(calls):
            prm.nearest_states_dev(d_q, m, kc, d_idx)
        sync(); dt = (time.perf_counter() - t0) / calls
        groups = (m + 3) // 4
        knn[str(n)] = dict(queries=m, call_ms=1e3 * dt, queries_per_s=m / dt, query_groups=groups, vertices_streamed_per_s=V * groups / dt,
                           bytes_streamed_per_s=8.0 * S * V * groups / dt)
    out = dict(vertices=V, edges=int(len(rm["edges"])), k=k, connect_k=kc, tolerance=tol, reps=args.reps, build_s=t_build,
               invalid_vertices=int(nv_bad), invalid_edges=int(ne_bad), roadmap_ik_batch=sizes, nearest_states=knn,
               source_hash=irt._lib.source_hash())
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    return out


if __name__ == "__main__":
    main()
