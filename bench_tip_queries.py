"""Batched tip-goal queries on config 5's roadmap (10^5 vertices): VoxelCachedLazyPRM.solve_to_tips -- roadmapIk + solveWithRoadmap
for a batch of tip requests in one call -- against the per-request loop over the single pieces (the k nearest tips by a host sort,
one device IK batch of k problems, one validity batch, one solveWithRoadmap), in the same process and alternating.

    python bench_tip_queries.py [--vertices 100000] [--k 5] [--reps 7] [--out profiles/r07/tip_queries.json]

Prints one JSON line (and writes it to --out): per batch size the time per call (min / median / max over the repetitions) and the
phases of the median call (nearest, IK, edges, select, solve; host clocks around work that ends in a device synchronise); the loop
on the same 64 requests and one iteration of it against Q = 1; tip_knn's rate against its floor.  Needs a GPU."""
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

# MI355X, measured chip-wide read rates (float4 copy from HBM; 2 048 rows shared by every workgroup from the XCDs' L2)
HBM_BYTES_PER_S, L2_BYTES_PER_S = 6.29e12, 17e12


def spread(ts):
    ts = np.sort(np.asarray(ts))
    return dict(min_ms=1e3 * float(ts[0]), median_ms=1e3 * float(ts[len(ts) // 2]), max_ms=1e3 * float(ts[-1]))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--vertices", type=int, default=100000)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--roadmap-k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sizes", type=int, nargs="*", default=[1, 64, 2048, 16384])
    ap.add_argument("--out", default="")
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_tip_queries.py needs a GPU")
    irt = importlib.import_module("interactive-rate-tendons_amd")
    W, T = irt.workloads, irt.tip_control
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
    V, k, tol = len(states), args.k, 1e-4
    prm.set_obstacles(new_vox)                                   # the interactive loop: the environment changed after the build
    nv_bad, ne_bad = prm.revalidate()
    rng = np.random.default_rng(17)
    nmax = max(args.sizes + [64])
    requests = tips[rng.integers(0, V, nmax)] + rng.normal(size=(nmax, 3)) * 0.003
    starts = rng.integers(0, V, nmax).astype(np.int32)
    vstat, _ = prm.validity()
    cand = np.flatnonzero(vstat == 1)
    cand_tips = tips[cand]

    def loop_iteration(q):
        """one request through the single pieces"""
        d = cand_tips - requests[q]
        near = cand[np.argsort((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2], kind="stable")[:k]]
        r = T.inverse_kinematics_batch_device(robot, states[near], requests[q], stop_threshold_err=tol)
        ok = chk.is_valid(r["state"])
        hit = np.flatnonzero(ok & (r["error"] < tol))
        i = int(hit[0]) if len(hit) else int(np.argmin(np.where(ok, r["error"], np.inf)))
        s = prm.solveWithRoadmap(starts[q:q + 1], near[i:i + 1])
        return r["state"][i], int(near[i]), int(s["status"][0])

    def loop(n):
        return [loop_iteration(q) for q in range(n)]

    def batch(n):
        return prm.solve_to_tips(starts[:n], requests[:n], tolerance=tol, k=k, motion_validator=mv)

    # warm-up: every shape of the timed window
    loop(4)
    for n in sorted(set(args.sizes + [64])):
        batch(n)
    sync = lambda: torch.cuda.synchronize()

    def timed(f, *a):
        sync(); t0 = time.perf_counter(); r = f(*a); sync()
        return time.perf_counter() - t0, r

    t_loop64, t_batch64, t_loop1, t_batch1, prof64, prof1 = [], [], [], [], [], []
    for _ in range(args.reps):                                   # alternating, same process
        t_loop64.append(timed(loop, 64)[0])
        t_batch64.append(timed(batch, 64)[0]); prof64.append(prm.tip_query_profile())
        t_loop1.append(timed(loop_iteration, 0)[0])
        t_batch1.append(timed(batch, 1)[0]); prof1.append(prm.tip_query_profile())
    res64 = batch(64)
    lp = loop(64)
    agree = int(sum(int(res64["neighbor_vertex"][q] == lp[q][1]) for q in range(64)))

    def median_profile(ts, profs):
        return profs[int(np.argsort(ts)[len(ts) // 2])]

    sizes = {}
    for n in args.sizes:
        ts, profs, res = [], [], None
        for _ in range(args.reps):
            dt, res = timed(batch, n)
            ts.append(dt); profs.append(prm.tip_query_profile())
        sizes[str(n)] = dict(spread(ts), phases_of_median_call=median_profile(ts, profs), requests_per_s=n / float(np.median(ts)),
                             outcomes=np.bincount(res["outcome"], minlength=3).tolist(), solved=int((res["status"] == 0).sum()))

    # tip_knn alone, on device tensors: device events around a run of calls (each call ends in a stream synchronise)
    knn = {}
    for n in sorted(set(args.sizes)):
        d_req = torch.from_numpy(np.ascontiguousarray(requests[:n])).cuda()
        d_idx = torch.empty((n, k), dtype=torch.int32, device="cuda")
        prm.nearest_tips_dev(d_req, n, k, d_idx)
        calls = 20
        sync(); t0 = time.perf_counter()
        for _ in range(calls):
            prm.nearest_tips_dev(d_req, n, k, d_idx)
        sync(); dt = (time.perf_counter() - t0) / calls
        groups = (n + 3) // 4                                    # a wave serves four requests per tile: the tip array is read once per group
        nbytes = 24.0 * V * groups
        knn[str(n)] = dict(call_ms=1e3 * dt, request_groups=groups, tips_streamed_per_s=V * groups / dt, floor_bytes=nbytes,
                           bytes_per_s=nbytes / dt, floor_ms_from_l2=1e3 * nbytes / L2_BYTES_PER_S, floor_ms_from_hbm=1e3 * nbytes / HBM_BYTES_PER_S,
                           fraction_of_l2_floor=(nbytes / L2_BYTES_PER_S) / dt,
                           note="whole call (validity check on the host, launches, synchronise); the %d-byte tip array fits an XCD's 4 MiB L2%s, so "
                                "the L2 rate bounds the stream, not HBM" % (24 * V, "" if 24 * V <= 4 << 20 else " only in part"))
    s_l64, s_b64, s_l1, s_b1 = spread(t_loop64), spread(t_batch64), spread(t_loop1), spread(t_batch1)
    run_spread = max(s_l1["max_ms"] - s_l1["min_ms"], s_b1["max_ms"] - s_b1["min_ms"])
    out = dict(
        vertices=V, edges=int(len(rm["edges"])), k=k, tolerance=tol, reps=args.reps, build_s=t_build, invalid_vertices=int(nv_bad), invalid_edges=int(ne_bad),
        batched=sizes,
        same_64_requests=dict(loop=s_l64, batched=s_b64, batched_phases_of_median_call=median_profile(t_batch64, prof64),
                              loop_ms_per_request=s_l64["median_ms"] / 64, speedup_of_medians=s_l64["median_ms"] / s_b64["median_ms"],
                              same_connection_vertex=agree,
                              note="the loop validates the IK solutions as states (is_valid); the batch checks the edge from the neighbour and steps back "
                                   "along it, so the two may pick different neighbours"),
        one_request=dict(loop_iteration=s_l1, batched_q1=s_b1, batched_phases_of_median_call=median_profile(t_batch1, prof1), run_to_run_spread_ms=run_spread),
        conditions=dict(batched_beats_loop_on_64=bool(s_b64["median_ms"] < s_l64["median_ms"]),
                        q1_not_slower_than_one_iteration_beyond_spread=bool(s_b1["median_ms"] - s_l1["median_ms"] <= run_spread)),
        tip_knn=knn, source_hash=irt._lib.source_hash())
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    return out


if __name__ == "__main__":
    main()
