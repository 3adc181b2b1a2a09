#!/usr/bin/env python3
"""Tip Jacobian and batched tip IK on one MI355X (tr_tip_jacobian / tr_ik_batch; not part of the driver's bench.py).
Prints one JSON object with a section for config 3 and one for config 2 with rotation + retraction:

  jacobian        Jacobians per second at 2^16 states (host arrays, and device tensors), and the algorithmic fp64 rate of
                  their K1 launches against the vector peak, priced with bench.py's count of an RK4 step
  ik              problems per second at 2^14 reachable goals for the device path (tr_ik_batch) and for the existing Python
                  path (tip_control.inverse_kinematics_batch: one fk_batch per iteration, backbones copied to the host), same
                  process, same starts, goals and thresholds; the speed-up; the rounds each ran
  roadmap_ik_5    latency of a k = 5 batch, the size VoxelCachedLazyPRM::roadmapIk solves

    python bench_ik.py [--reps 5]
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

from bench import FP64_VALU_PEAK_TF, algorithmic_flops_per_rk4_step  # noqa: E402

LM = dict(stop_threshold_err=1e-6, stop_threshold_Dp=1e-12, stop_threshold_JT_err_inf=1e-16, max_iters=60)


def rk4_steps(robot, states):
    """RK4 steps K1 integrates per state: P - 1 on the shared grid; with retraction the lane's own grid from s_start to L"""
    P = len(robot._t(0.0))
    if not robot.enable_retraction:
        return np.full(len(states), P - 1)
    L, dL = robot.specs.L, robot.specs.dL
    s = np.minimum(states[:, -1], L)
    m = np.where(s <= L - dL / 2, np.floor((L - dL / 2 - s) / dL) + 1, 0)
    return np.minimum(m, P - 1)


def median_time(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def section(irt, robot, reps):
    import torch
    W, T = irt.workloads, irt.tip_control
    eng = robot.engine(0)
    S, N = robot.state_size(), len(robot.tendons)
    out = {"state_size": S, "lanes_per_problem": 2 * S + 1}
    # ---- Jacobian at 2^16 states ----
    n = 1 << 16
    st = W.random_states(robot, n, seed=3, tau_max=15.0)
    eng.tip_jacobian(st[:1024])                                           # warm-up: workspace, code objects
    t_host = median_time(lambda: eng.tip_jacobian(st), reps)
    d_st = torch.from_numpy(st).cuda()
    d_J = torch.empty(n * 3 * S, dtype=torch.float64, device="cuda")

    def dev():
        eng.tip_jacobian_dev(d_st, n, d_J)
        torch.cuda.synchronize()
    dev()
    t_dev = median_time(dev, reps)
    eng.profile_begin()
    dev()
    prof = eng.profile_read()["fk_rk4_batch"]
    eng.profile_end()
    lanes = np.repeat(st, 2 * S + 1, axis=0)
    for j in range(S):                                                    # the perturbed coordinate only moves s_start's steps
        d = np.maximum(np.abs(1e-4 * st[:, j]), 1e-6)
        lanes[1 + 2 * j::2 * S + 1, j] -= d
        lanes[2 + 2 * j::2 * S + 1, j] += d
    flops = float(rk4_steps(robot, lanes).sum()) * algorithmic_flops_per_rk4_step(N)
    tf = flops / (prof["total_ms"] * 1e-3) / 1e12 if prof["total_ms"] > 0 else None
    out["jacobian"] = {"states": n, "jacobians_per_s_host": n / t_host, "jacobians_per_s_dev": n / t_dev,
                       "k1_ms": prof["total_ms"], "k1_launches": prof["launches"],
                       "k1_fp64": {"achieved_tflops": tf, "peak_tflops": FP64_VALU_PEAK_TF,
                                   "frac": tf / FP64_VALU_PEAK_TF if tf else None,
                                   "flops_source": "bench.algorithmic_flops_per_rk4_step x RK4 steps of every lane"}}
    # ---- IK at 2^14 reachable goals ----
    m = 1 << 14
    goal_states = W.random_states(robot, m, seed=11, tau_max=12.0)
    if robot.enable_retraction:
        goal_states[:, -1] = np.random.default_rng(1).uniform(0.0, 0.08, m)
    goals, _ = eng.fk_tips(goal_states)
    rng = np.random.default_rng(12)
    start = goal_states + rng.normal(size=goal_states.shape) * np.array([1.5] * N + ([0.3] if robot.enable_rotation else [])
                                                                        + ([0.01] if robot.enable_retraction else []))
    b = T.Bounds.from_robot(robot)
    start = np.clip(start, np.maximum(b.lower, -10), np.minimum(b.upper, 25))
    T.inverse_kinematics_batch_device(robot, start[:64], goals[:64], **LM)  # warm-up
    t0 = time.perf_counter()
    rd = T.inverse_kinematics_batch_device(robot, start, goals, **LM)
    t_d = time.perf_counter() - t0
    # The Python path solves A + mu I with np.linalg.solve, which raises on a numerically singular matrix (S > 3: J^T J has rank
    # 3 at most, and mu shrinks by up to 3x per accepted step).  If the whole batch raises, it is timed in chunks of 2^11 and
    # the chunks that raise are left out (their time is counted, their problems are not).
    py = {}
    t0 = time.perf_counter()
    try:
        rp = T.inverse_kinematics_batch(robot, start, goals, **LM)
        solved = np.arange(m)
        py["launches"] = rp["launches"]
    except np.linalg.LinAlgError as e:
        py["whole_batch_error"] = "%s after %.1f s" % (e, time.perf_counter() - t0)
        t0 = time.perf_counter()
        parts, idx = [], []
        for c in range(0, m, 1 << 11):
            try:
                parts.append(T.inverse_kinematics_batch(robot, start[c:c + (1 << 11)], goals[c:c + (1 << 11)], **LM))
                idx.append(np.arange(c, min(m, c + (1 << 11))))
            except np.linalg.LinAlgError:
                pass
        rp = {k: np.concatenate([p[k] for p in parts]) for k in ("state", "error", "iters")} if parts else None
        solved = np.concatenate(idx) if idx else np.arange(0)
        py["chunks_of_2048_completed"] = len(parts)
    t_p = time.perf_counter() - t0
    py.update({"s": t_p, "problems": int(len(solved)), "problems_per_s": len(solved) / t_p})
    if rp is not None and len(solved):
        py.update({"reached_1e-6": float((rp["error"] <= 1e-6).mean()), "mean_iters": float(rp["iters"].mean())})
        tol = 1e-6 * (1 + np.abs(rp["state"]).max(1))
        py["states_agree_with_device_1e-6_rel"] = float((np.abs(rd["state"][solved] - rp["state"]).max(1) <= tol).mean())
    out["ik"] = {"problems": m, "device": {"s": t_d, "problems_per_s": m / t_d, "rounds": rd["launches"],
                                           "reached_1e-6": float((rd["error"] <= 1e-6).mean()), "mean_iters": float(rd["iters"].mean())},
                 "python": py, "speedup": (m / t_d) / py["problems_per_s"] if py["problems_per_s"] > 0 else None}
    # ---- a roadmapIk-sized batch ----
    k5_s, k5_g = start[:5], goals[0]
    eng.ik_batch(k5_s, k5_g, stop_threshold_err=1e-4)
    lat = [median_time(lambda: eng.ik_batch(k5_s, k5_g, stop_threshold_err=1e-4), 1) for _ in range(max(reps, 20))]
    out["roadmap_ik_5"] = {"median_ms": 1e3 * float(np.median(lat)), "min_ms": 1e3 * float(np.min(lat))}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    irt = importlib.import_module("interactive-rate-tendons_amd")
    irt.build()
    W = irt.workloads
    rot_ret = W.robot_config2()
    rot_ret.enable_rotation = True
    rot_ret.enable_retraction = True
    res = {"bench": "tip_ik", "config3": section(irt, W.robot_config3(), args.reps), "config2_rot_ret": section(irt, rot_ret, args.reps)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
