#!/usr/bin/env python3
"""Host overhead of the launch layer (csrc/launch_host.inc) where it shows: tr_validate_batch (host arrays in, verdict out) at n = 1
and n = 64, tr_validate_batch_dev at n = 64 back to back (one wave per call: the device's time per call) and on an idle device
without the wait (the host's share of a call), and a small indexed edge check through the lanes and through the edge queue.  One JSON line; several blocks per figure, so that one process shows its own spread.

    TENDON_HIP_LIB=<another build> python profiles/probe_launch_latency.py
"""
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BLOCKS, REPS = 7, 300


def blocks(f, reps=REPS, sync=None):
    """median, min and max over BLOCKS blocks of the mean time of `reps` calls, in microseconds"""
    out = []
    for _ in range(BLOCKS):
        t0 = time.perf_counter()
        for _ in range(reps):
            f()
        if sync:
            sync()
        out.append(1e6 * (time.perf_counter() - t0) / reps)
    return {"median_us": float(np.median(out)), "min_us": min(out), "max_us": max(out)}


def host_only(f, sync, calls=12, rounds=200):
    """the host's share of a call: `calls` calls on an idle device (fewer than the argument rings have slots, so none waits for a
    slot), timed without the synchronisation that follows them"""
    out = []
    for _ in range(BLOCKS):
        t = 0.0
        for _ in range(rounds):
            sync()
            t0 = time.perf_counter()
            for _ in range(calls):
                f()
            t += time.perf_counter() - t0
        out.append(1e6 * t / (rounds * calls))
    sync()
    return {"median_us": float(np.median(out)), "min_us": min(out), "max_us": max(out)}


def main():
    import torch
    irt = importlib.import_module("interactive-rate-tendons_amd")
    W = irt.workloads
    robot = W.robot_config2()
    vox, _ = W.reach_environment(seed=7, n_spheres=64)
    res = {}
    for queue in ("1", "0"):
        os.environ["TENDON_HIP_EDGE_QUEUE"] = queue
        chk = irt.VoxelBackboneValidityChecker(robot, irt.VoxelEnvironment(), vox)
        mv = irt.VoxelBackboneMotionValidator(chk)
        eng = chk.engine
        st = W.random_states(robot, 256, seed=5, tau_max=10.0)
        if queue == "1":
            eng.validate_batch(st[:64], False, False)
            for n in (1, 64):
                res["validate_batch_n%d" % n] = blocks(lambda: eng.validate_batch(st[:n], False, False))
            d_st = torch.from_numpy(st[:64]).cuda()
            bits = torch.zeros(1, dtype=torch.int64, device="cuda")
            eng.validate_batch_dev(d_st, 64, bits)
            torch.cuda.synchronize()
            res["validate_batch_dev_n64_enqueue"] = blocks(lambda: eng.validate_batch_dev(d_st, 64, bits), sync=torch.cuda.synchronize)
            res["validate_batch_dev_n64_host"] = host_only(lambda: eng.validate_batch_dev(d_st, 64, bits), torch.cuda.synchronize)
        near = np.argsort(np.linalg.norm(st[:, None] - st[None], axis=2), axis=1)[:, 1:5]
        edges = np.stack([np.repeat(np.arange(256), 4), near.reshape(-1)], 1)
        mv.check_motion_indexed(st, edges)
        res["edges_indexed_1024_%s" % ("queue" if queue == "1" else "lanes")] = blocks(lambda: mv.check_motion_indexed(st, edges), reps=40)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
