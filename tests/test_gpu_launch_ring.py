"""The kernel launch layer (csrc/launch_host.inc) under slot reuse: the verdict and fused launches read their arguments from two
rings of 16 device slots, each slot guarded by an event, so more than 16 consecutive calls on one context rewrite slots whose
launches may still be in flight -- on whichever stream they ran.  Many small calls on one engine must equal one large call on a
fresh one, and the launch counts per call are pinned."""
import numpy as np
import pytest

from test_gpu_edges import _with_env

pytestmark = pytest.mark.gpu

PER_CALL = 64
SLOTS = 16


def _many_calls_equal_one(make_checker, states, calls):
    """`calls` consecutive validate_batch_dev calls of 64 states on one engine, alternating between two streams, into disjoint slices
    of one bits / tips / flags buffer, against one call over all states on a fresh engine: bits, flags and tips equal, tips bit for bit."""
    import torch
    n = calls * PER_CALL
    assert len(states) == n
    d_states = torch.from_numpy(states).cuda()

    def buffers():
        return (torch.zeros(calls, dtype=torch.int64, device="cuda"), torch.zeros((n, 3), dtype=torch.float64, device="cuda"),
                torch.zeros(n, dtype=torch.uint8, device="cuda"))

    bits, tips, flags = buffers()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    eng = make_checker().engine
    for i in range(calls):
        lo, hi = i * PER_CALL, (i + 1) * PER_CALL
        eng.validate_batch_dev(d_states[lo:hi], PER_CALL, bits[i:i + 1], tips[lo:hi], flags[lo:hi], stream=streams[i % 2])
    torch.cuda.synchronize()
    want_bits, want_tips, want_flags = buffers()
    torch.cuda.synchronize()
    make_checker().engine.validate_batch_dev(d_states, n, want_bits, want_tips, want_flags)
    torch.cuda.synchronize()
    assert torch.equal(bits, want_bits), torch.nonzero(bits != want_bits).flatten()[:8]
    assert torch.equal(flags, want_flags), torch.nonzero(flags != want_flags).flatten()[:8]
    assert np.array_equal(tips.cpu().numpy().view(np.uint64), want_tips.cpu().numpy().view(np.uint64))
    valid = np.unpackbits(want_bits.cpu().numpy().view(np.uint8), bitorder="little")[:n]
    return valid, want_flags.cpu().numpy()


def _config1(irt):
    W = irt.workloads
    robot = W.robot_config1()
    vox, _ = W.reach_environment(seed=7, n_spheres=64, N=64)
    return robot, vox


def test_ring_wrap_around_on_two_streams(irt):
    """3 x 16 + 1 calls wrap both 16-slot rings three times and cross the stream-switch dependency on every call."""
    W = irt.workloads
    robot, vox = _config1(irt)
    calls = 3 * SLOTS + 1
    states = W.random_states(robot, calls * PER_CALL, seed=42)
    valid, _ = _many_calls_equal_one(lambda: irt.VoxelBackboneValidityChecker(robot, irt.VoxelEnvironment(), vox), states, calls)
    assert 0.05 < valid.mean() < 0.98


def test_ring_wrap_around_retraction_robot(irt):
    """The same on a robot with retraction, every call ordered by backbone length (TENDON_HIP_RETRACT_SORT=64) and the fallback
    pass through a 64-column workspace (TENDON_HIP_FB_CAP=64): the shared ordering helper, the hand-over planes and the fallback
    columns at the size of one wave."""
    from test_gpu_retraction import _robot, _states
    W = irt.workloads
    robot = _robot(irt, "helix")
    for t in robot.tendons:
        t.max_length = 0.02
    vox, _ = W.reach_environment(seed=7, n_spheres=64)
    calls = 3 * SLOTS + 1
    states = _states(irt, robot, calls * PER_CALL, seed=62)

    def run():
        return _many_calls_equal_one(lambda: irt.VoxelBackboneValidityChecker(robot, irt.VoxelEnvironment(), vox), states, calls)

    valid, flags = _with_env(irt, {"TENDON_HIP_RETRACT_SORT": "64", "TENDON_HIP_FB_CAP": "64"}, run)
    hist = np.bincount(flags, minlength=16)
    assert 0.05 < valid.mean() < 0.98 and hist[15] > 0 and hist[7] > 0


def test_ring_slot_reuse_sphere_checker(irt):
    """17 calls against one of 17 x 64 with the sphere-swept checker: the `spheres` fields of a reused slot."""
    W = irt.workloads
    robot, vox = _config1(irt)
    calls = SLOTS + 1
    states = W.random_states(robot, calls * PER_CALL, seed=43)
    valid, _ = _many_calls_equal_one(lambda: irt.VoxelValidityChecker(robot, irt.VoxelEnvironment(), vox), states, calls)
    assert 0.02 < valid.mean() < 0.98


def test_back_to_back_edge_checks_queue_and_lanes(irt):
    """Two indexed edge checks in a row on one engine, as the edge queue's one launch and as the level-synchronous lanes: the same
    verdicts, call after call."""
    W = irt.workloads
    robot, vox = _config1(irt)
    states = W.random_states(robot, PER_CALL, seed=42)
    nt = len(robot.tendons)
    near = np.argsort(np.linalg.norm(states[:, None, :nt] - states[None, :, :nt], axis=2), axis=1)[:, 1:3]
    edges = np.stack([np.repeat(np.arange(PER_CALL), 2), near.reshape(-1)], 1)[:32]

    def run():
        mv = irt.VoxelBackboneMotionValidator(irt.VoxelBackboneValidityChecker(robot, irt.VoxelEnvironment(), vox))
        first, second = mv.check_motion_indexed(states, edges), mv.check_motion_indexed(states, edges)
        return first, second, mv.engine.edge_schedule_last()

    q1, q2, sch_q = _with_env(irt, {"TENDON_HIP_EDGE_QUEUE": "1"}, run)
    l1, l2, sch_l = _with_env(irt, {"TENDON_HIP_EDGE_QUEUE": "0"}, run)
    assert sch_q["samples"] > 0 and sch_q["flags"] == 0 and sch_l["samples"] == 0     # the queue ran, then the lanes
    for got in (q1, q2, l2):
        assert np.array_equal(got["valid"], l1["valid"]) and np.array_equal(got["n_fk"], l1["n_fk"])
    assert 0 < np.asarray(l1["valid"]).sum() < len(edges)


def test_launch_counts_of_one_call(irt):
    """One validate_batch_dev call of 64 states is, on the default schedule, 1 launch of fk_verdict and 1 of fk_sweep_fused (the
    fallback list's), 0 of fk_rk4_batch and backbone_voxel_sweep; with TENDON_HIP_FUSED=0, 1 of fk_rk4_batch and 1 of
    backbone_voxel_sweep, 0 of the other two.  (The counts the code reported before the launch layer moved into its own file.)"""
    import torch
    W = irt.workloads
    robot, vox = _config1(irt)
    d_states = torch.from_numpy(W.random_states(robot, PER_CALL, seed=42)).cuda()
    bits = torch.zeros(1, dtype=torch.int64, device="cuda")

    def run():
        eng = irt.VoxelBackboneValidityChecker(robot, irt.VoxelEnvironment(), vox).engine
        eng.profile_begin()
        eng.validate_batch_dev(d_states, PER_CALL, bits)
        torch.cuda.synchronize()
        prof = eng.profile_read()
        eng.profile_end()
        return {k: v["launches"] for k, v in prof.items()}

    got = run()
    assert (got["fk_verdict"], got["fk_sweep_fused"], got["fk_rk4_batch"], got["backbone_voxel_sweep"]) == (1, 1, 0, 0)
    got = _with_env(irt, {"TENDON_HIP_FUSED": "0"}, run)
    assert (got["fk_verdict"], got["fk_sweep_fused"], got["fk_rk4_batch"], got["backbone_voxel_sweep"]) == (0, 0, 1, 1)
