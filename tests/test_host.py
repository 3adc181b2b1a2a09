"""CPU tests of the host logic: the C-ABI library loads and exports every declared symbol, the
product fails loudly without a GPU, the host mirrors (VoxelOctree, workloads, TendonRobot helpers)
agree with the oracle, and the N>1 sharding + all-gather path works with gloo at world_size 2."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


# ---- C ABI ---------------------------------------------------------------------------------------------
def test_header_declares_exactly_the_bound_symbols(irt):
    text = open(os.path.join(ROOT, "include", "tendon_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(tr_[a-z_]+)\s*\(", text))
    assert declared == set(irt._lib.ABI_SYMBOLS)


def test_shared_library_exports_every_symbol(irt):
    irt.build()                                   # no-op when up to date
    out = subprocess.check_output(["nm", "-D", "--defined-only", irt.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    missing = set(irt._lib.ABI_SYMBOLS) - exported
    assert not missing, missing
    lib = ctypes.CDLL(irt.LIB_PATH)
    for s in irt._lib.ABI_SYMBOLS:
        assert hasattr(lib, s)


def test_environment_switches_are_documented_and_alive():
    """The switch surface stays honest: what csrc/ reads is what the table in include/tendon_hip.h documents, and every switch a
    test or a benchmark sets is still read by the library or the package (a dead one makes an A/B compare a call with itself)."""
    name = re.compile(r"TENDON_HIP_[A-Z0-9_]*[A-Z0-9]")
    pkg = os.path.join(ROOT, "interactive-rate-tendons_amd")
    csrc = os.path.join(pkg, "csrc")
    read_c = set()
    for f in sorted(os.listdir(csrc)):
        if f.endswith((".hip", ".hpp", ".inc")):
            read_c |= set(re.findall(r'getenv\(\s*"(TENDON_HIP_[A-Z0-9_]+)"', open(os.path.join(csrc, f)).read()))
    header = open(os.path.join(ROOT, "include", "tendon_hip.h")).read()
    table = header[header.index("/* Environment switches"):]
    documented = set(name.findall(table[:table.index("*/")]))
    assert read_c == documented, (sorted(read_c - documented), sorted(documented - read_c))
    read_py = set()
    for f in sorted(os.listdir(pkg)):
        if f.endswith(".py"):
            read_py |= set(name.findall(open(os.path.join(pkg, f)).read()))
    tests = os.path.join(ROOT, "tests")
    users = [os.path.join(tests, f) for f in sorted(os.listdir(tests)) if f.endswith(".py")] + \
            [os.path.join(ROOT, f) for f in sorted(os.listdir(ROOT)) if f.startswith("bench") and f.endswith(".py")]
    for f in users:
        dead = set(name.findall(open(f).read())) - read_c - read_py
        assert not dead, (f, sorted(dead))


def test_library_contains_gfx950_code_object(irt):
    data = open(irt.LIB_PATH, "rb").read()
    assert b"gfx950" in data and b"fk_rk4_batch_uniform" in data and b"backbone_voxel_sweep" in data and b"fk_sweep_fused" in data


@pytest.mark.skipif(_has_gpu(), reason="checks the no-GPU failure mode")
def test_product_fails_loudly_without_gpu(irt):
    robot = irt.workloads.robot_config1()
    with pytest.raises(irt.HipError) as e:
        robot.shape_batch(np.zeros((2, 3)))
    assert "no CPU fallback" in str(e.value)


def test_product_never_imports_the_oracle():
    """The product path may not import, include, link or load anything under oracle/."""
    pkg = os.path.join(ROOT, "interactive-rate-tendons_amd")
    bad = re.compile(r"(^\s*(import|from)\s+oracle\b)|(#\s*include\s*[\"<][^\">]*oracle)|liboracle|tendon_oracle|orc_[a-z_]+\(",
                     re.M)
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".inc", ".h")):
                src = open(os.path.join(dirpath, f), errors="ignore").read()
                assert not bad.search(src), (f, bad.search(src).group(0))
    out = subprocess.check_output(["ldd", os.path.join(pkg, "libtendon_hip.so")], text=True)
    assert "oracle" not in out


# ---- host mirrors ----------------------------------------------------------------------------------------
def test_voxel_octree_matches_oracle_grid(irt, orc):
    rng = np.random.default_rng(0)
    v = irt.VoxelOctree(64)
    v.set_xlim(-0.3, 0.5); v.set_ylim((-0.25, 0.25)); v.set_zlim(0.0, 0.4)
    g = orc.Grid(64, (-0.3, 0.5, -0.25, 0.25, 0.0, 0.4))
    assert (v.dx(), v.dy(), v.dz()) == g.cell_size
    for _ in range(12):
        c, r = rng.uniform(-0.3, 0.5, 3), rng.uniform(0.005, 0.08)
        v.add_sphere(c, r); g.add_sphere(c, r)
    for _ in range(10):                                    # add_capsule (VoxelOctree.cpp:471-515), also degenerate and reaching outside
        a, b, r = rng.uniform(-0.35, 0.55, 3), rng.uniform(-0.35, 0.55, 3), rng.uniform(0.004, 0.05)
        if _ == 0:
            b = a.copy()
        v.add_capsule(a, b, r); g.add_capsule(a, b, r)
    for _ in range(50):
        p = rng.uniform(-0.4, 0.6, 3)
        v.add_point(p); g.add_point(p)
        assert v.is_in_domain(*p) == g.is_in_domain(*p)
        assert v.nearest_cell(*p) == g.nearest_cell(*p)
        if v.is_in_domain(*p):
            assert v.find_cell(*p) == g.find_cell(*p)
        else:
            with pytest.raises(irt.DomainError):
                v.find_cell(*p)
    assert np.array_equal(v.blocks, g.blocks())
    assert v.ncells() == g.ncells() and v.nblocks() == g.nblocks()
    ids, masks = v.to_sparse()
    oi, om = g.export_blocks()
    assert np.array_equal(ids, oi) and np.array_equal(masks, om)
    assert irt.VoxelOctree.from_sparse(64, v.limits(), ids, masks) == v
    e = v.empty_copy()
    assert e.is_empty() and e.limits() == v.limits() and not v.collides(e) and v.collides(v)


def test_voxel_octree_file_formats(irt, tmp_path):
    """The reference's obstacle-set files (collision/VoxelOctree.cpp:1357-1497): JSON object layout, TOML with the block
    split into two 32-bit halves, msgpack of the same object, each optionally gzipped; VoxelEnvironment loads by name."""
    import json
    v = irt.VoxelOctree(32)
    v.set_xlim(-0.5, 0.25); v.set_ylim(0.0, 1.0); v.set_zlim(-1.0, 1.0)
    v.add_sphere([0.0, 0.4, 0.1], 0.3)
    v.set_block(7, 0, 5, (1 << 63) | (1 << 32) | 5)              # exercises the upper half and bit 63
    j = v.to_json()
    o = j["VoxelOctree"]
    assert set(o) == {"dimension", "xlimits", "ylimits", "zlimits", "data"} and o["dimension"] == 32 and o["ylimits"] == [0.0, 1.0]
    assert [7, 0, 5, (1 << 63) | (1 << 32) | 5] in o["data"] and len(o["data"]) == v.nblocks()
    assert irt.VoxelOctree.from_json(json.loads(json.dumps(j))) == v
    assert "[7, 0, 5, %d, 5]" % ((1 << 31) | 1) in v.to_toml()
    for name in ("a.json", "b.json.gz", "c.msgpack", "d.toml", "e.toml.gz"):
        path = str(tmp_path / name)
        v.to_file(path)
        w = irt.VoxelOctree.from_file(path)
        assert w == v and w.limits() == v.limits(), name
    env = irt.VoxelEnvironment(filename=str(tmp_path / "a.json"))
    assert env.get_obstacles() == v
    with pytest.raises(irt.Unsupported):
        irt.VoxelOctree.from_file(str(tmp_path / "x.nrrd"))
    with pytest.raises(irt.InvalidArgument):
        irt.VoxelEnvironment().get_obstacles()


def test_robot_toml_roundtrip(irt, tmp_path):
    """tendon::TendonRobot::to_toml / from_toml (tendon/TendonRobot.cpp:1012-1089): table names and keys as the reference
    writes them, defaults for the optional keys."""
    import tomli
    r = irt.workloads.robot_config3()
    r.enable_rotation, r.r, r.residual_threshold = True, 0.0125, 1e-6
    txt = r.to_toml()
    t = tomli.loads(txt)
    assert set(t) == {"tendon_robot", "backbone_specs", "tendons"} and len(t["tendons"]) == 4
    assert t["backbone_specs"]["length_discretization"] == r.specs.dL and t["tendon_robot"]["radius"] == 0.0125
    path = tmp_path / "robot.toml"
    path.write_text(txt)
    q = irt.TendonRobot.from_toml(str(path))
    assert (q.r, q.enable_rotation, q.enable_retraction, q.residual_threshold) == (0.0125, True, False, 1e-6)
    assert q.specs == r.specs and q.tendons == r.tendons
    minimal = tomli.loads("[tendon_robot]\nradius = 0.02\n[backbone_specs]\nlength = 0.1\nlength_discretization = 0.01\nro = 0.01\nri = 0.0\nE = 1e6\nnu = 0.3\n")
    m = irt.TendonRobot.from_toml(minimal)
    assert m.tendons == [] and m.residual_threshold == 5e-6 and not m.enable_rotation
    with pytest.raises(KeyError):
        irt.TendonRobot.from_toml({"backbone_specs": {}})


def test_voxel_octree_errors(irt):
    with pytest.raises(irt.InvalidArgument):
        irt.VoxelOctree(100)
    assert irt.VoxelOctree.to_supported_size(100) == 128
    with pytest.raises(irt.InvalidArgument):
        irt.VoxelOctree.to_supported_size(513)
    v = irt.VoxelOctree(8)
    with pytest.raises(irt.LengthError):
        v.set_ylim(2.0, 1.0)
    with pytest.raises(irt.InvalidArgument):
        v.collides(irt.VoxelOctree(16))
    assert v.bitmask(1, 2, 3) == np.uint64(1) << np.uint64(27)
    assert not v.set_cell(7, 0, 3) and v.cell(7, 0, 3) and v.set_cell(7, 0, 3)
    assert v.set_cell(7, 0, 3, False) is False or True
    assert not v.cell(7, 0, 3)


def test_robot_host_helpers(irt):
    r = irt.workloads.robot_config1()
    assert r.state_size() == 3
    r.enable_rotation = r.enable_retraction = True
    assert r.state_size() == 5
    assert np.array_equal(r.calc_dl([1.0, 2.0, 3.0], [0.5, 2.0, 4.0]), [0.5, 0.0, -1.0])
    with pytest.raises(irt.OutOfRange):
        r.calc_dl([1.0], [1.0, 2.0])
    assert r.is_within_length_limits([0.0, 0.035, -0.015]) and not r.is_within_length_limits([0.0, 0.036, 0.0])
    with pytest.raises(irt.OutOfRange):
        r.is_within_length_limits([0.0, 0.0])
    t = irt.TendonSpecs(C=[1.0, 5.0], D=[0.01])
    assert t.is_helix() and not t.is_straight() and irt.TendonSpecs().is_straight()
    assert irt.TendonSpecs(C=[1.0, 0.0, 2.0], D=[0.01, 0.0]).theta_degree() == 2


def test_workloads_are_deterministic(irt):
    W = irt.workloads
    a, ca = W.reach_environment(seed=7, n_spheres=16)
    b, cb = W.reach_environment(seed=7, n_spheres=16)
    assert a == b and np.array_equal(ca, cb)
    r = W.robot_config2()
    assert np.array_equal(W.random_states(r, 100, 5), W.random_states(r, 100, 5))
    assert len(r._t()) == 129 and len(W.robot_config1()._t()) == 41
    assert W.robot_config3().state_size() == 4


def test_candidate_states_do_not_depend_on_the_split(irt):
    D = irt.distributed
    r = irt.workloads.robot_config3()
    whole = D.candidate_states(r, seed=9, start=0, count=200000)
    for start, count in ((0, 1), (65535, 3), (65536, 70000), (131071, 2), (199000, 1000)):
        assert np.array_equal(D.candidate_states(r, 9, start, count), whole[start:start + count])
    assert whole.min() >= 0 and whole.max() < 20.0
    assert not np.array_equal(D.candidate_states(r, 10, 0, 64), whole[:64])          # the seed is the key
    assert abs(whole.mean() - 10.0) < 0.05 and np.abs(np.corrcoef(whole.T) - np.eye(4)).max() < 0.01


def test_philox_known_answers_and_generator_layout(irt):
    """The candidate generator is Philox-4x32-10 (Salmon et al., SC'11; the Random123 distribution's known-answer vectors
    for philox4x32, 10 rounds) with counter (index lo, index hi, coordinate pair, 0) and key = seed; csrc/sample.hip is the
    same function (compared bit for bit in tests/test_gpu_sampling.py)."""
    D = irt.distributed
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        got = D.philox4x32_10(*[[c] for c in ctr], *key)
        assert tuple(int(g[0]) for g in got) == want
    r = irt.workloads.robot_config3()
    r.enable_rotation = r.enable_retraction = True                 # S = 6: three Philox blocks per candidate
    lo, hi = D.sampling_box(r)
    assert lo.tolist() == [0, 0, 0, 0, -np.pi, 0] and hi.tolist() == [20, 20, 20, 20, np.pi, r.specs.L]
    seed, idx = (5 << 32) | 77, (1 << 33) + 12345
    st = D.candidate_states(r, seed, idx, 1)[0]
    for j in range(3):
        w = [int(x[0]) for x in D.philox4x32_10([idx & 0xffffffff], [idx >> 32], [j], [0], 77, 5)]
        for half in range(2):
            u = (((w[2 * half] << 32) | w[2 * half + 1]) >> 11) * 2.0 ** -53
            d = 2 * j + half
            assert st[d] == lo[d] + u * (hi[d] - lo[d])


def test_shard_bounds(irt):
    D = irt.distributed
    for M in (1, 63, 64, 65, 1000, 1 << 20, (1 << 20) + 1):
        for world in (1, 2, 4, 8):
            spans = [D.shard_bounds(M, world, r) for r in range(world)]
            shard = spans[0][2]
            assert shard % 64 == 0 and all(s[2] == shard for s in spans)
            assert spans[0][0] == 0 and all(spans[i][1] == spans[i + 1][0] for i in range(world - 1))
            assert spans[-1][1] >= M and shard * world - M < 64 * world


def test_unpack_bits(irt):
    w = np.array([0b1011, 1 << 63], dtype=np.uint64)
    b = irt.unpack_bits(w, 128)
    assert b[:4].tolist() == [True, True, False, True] and b[127] and b.sum() == 4


# ---- N > 1: sharding + all-gather over gloo, world_size 2 ---------------------------------------------------
WORKER = r'''
import importlib, os, sys
import numpy as np
sys.path.insert(0, %(root)r)
import torch.distributed as dist
from oracle import oracle as orc
irt = importlib.import_module("interactive-rate-tendons_amd")
W, D = irt.workloads, irt.distributed
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
robot = W.robot_config3()
vox, _ = W.reach_environment(seed=7, n_spheres=32)
s = robot.specs
orb = orc.Robot([t.C for t in robot.tendons], [t.D for t in robot.tendons], dL=s.dL)
og = orc.Grid(256, vox.limits()); og.blocks()[...] = vox.blocks
def validate_local(states):                      # the oracle stands in for the GPU engine on CPU
    v, _, _ = orc.validate_batch(orb, og, states)
    return np.packbits(np.pad(v, (0, -len(v) %% 64)), bitorder="little").view(np.uint64)
M = int(sys.argv[1])
mask = D.ShardedVertexValidator(robot, validate_local, seed=3).run(M)
valid = irt.unpack_bits(mask, M)
# phase 2: every rank connects the same edges from the gathered mask, validates its shard, gathers the verdicts
states = D.candidate_states(robot, 3, 0, M)[valid][:131]
a, b = states[:-1], states[1:]
def edges_local(ea, eb):
    v, _, _ = orc.check_motion_batch(orb, og, ea, eb)
    return D.pack_bits(v)
emask = D.ShardedEdgeValidator(edges_local).run(a, b)
# the roadmap form of the same phase: all vertices on every rank, the rank's shard of the index pairs
eidx = np.stack([np.arange(len(states) - 1), np.arange(1, len(states))], 1)
emask_ix = D.ShardedEdgeValidator(lambda st_, e_: edges_local(st_[e_[:, 0]], st_[e_[:, 1]])).run_indexed(states, eidx)
assert np.array_equal(emask_ix, emask)
# between the two: the connection loop's neighbour table, rows computed per shard and all-gathered (int32)
def knn_local(first, count):                     # numpy brute force stands in for tr_knn_range
    d = np.linalg.norm(states[first:first + count, None, :] - states[None, :, :], axis=2)
    return np.argsort(d, axis=1, kind="stable")[:, :4]
table = D.ShardedNeighbours(knn_local, 4).run(len(states))
# the vertex phase with a row of data per ACCEPTED candidate gathered next to the mask (in production the backbone signatures the edge
# phase would otherwise recompute on every rank): here the row is (candidate index, 7 x index), compacted with numpy
import torch
def validate_with_rows(first, count, n_words):
    words = np.zeros(n_words, dtype=np.uint64)
    if count > 0:
        w = np.asarray(validate_local(D.candidate_states(robot, 3, first, count))).view(np.uint64)
        words[: w.size] = w
        if count %% 64:
            words[count // 64] &= np.uint64((1 << (count %% 64)) - 1)
    idx = np.arange(first, first + count, dtype=np.int32)
    return torch.from_numpy(words.view(np.int64)), torch.from_numpy(np.stack([idx, 7 * idx], 1))
def compact(mask_words, count, rows):
    return rows[torch.from_numpy(irt.unpack_bits(mask_words.numpy().view(np.uint64), count))]
full, rows = D.ShardedVertexValidator(robot, seed=3, validate_candidates=validate_with_rows).run_with_rows(M, compact)
assert np.array_equal(irt.unpack_bits(full.numpy().view(np.uint64), M), valid)
assert np.array_equal(rows.numpy()[:, 0], np.flatnonzero(valid)) and np.array_equal(rows.numpy()[:, 1], 7 * np.flatnonzero(valid))
if rank == 0:
    np.save(sys.argv[2], valid)
    np.save(sys.argv[2] + ".edges.npy", irt.unpack_bits(emask, len(a)))
    np.save(sys.argv[2] + ".knn.npy", table)
    np.save(sys.argv[2] + ".knn_want.npy", knn_local(0, len(states)))
dist.barrier()
dist.destroy_process_group()
'''


def _run_world(world, M, out, tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(WORKER % {"root": ROOT})
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(29500 + world + os.getpid() % 500), OMP_NUM_THREADS="2")
    procs = [subprocess.Popen([sys.executable, str(script), str(M), out],
                              env=dict(env, RANK=str(r), WORLD_SIZE=str(world))) for r in range(world)]
    for p in procs:
        assert p.wait(timeout=600) == 0


def test_sharded_validation_gloo_world2_and_3_match_world1(irt, tmp_path):
    M = 700                                        # not a multiple of 64: exercises padding bits
    _run_world(1, M, str(tmp_path / "w1.npy"), tmp_path)
    _run_world(2, M, str(tmp_path / "w2.npy"), tmp_path)
    _run_world(3, M, str(tmp_path / "w3.npy"), tmp_path)          # shards of 256, 256 and 188 candidates; row blocks of three lengths
    a, b = np.load(tmp_path / "w1.npy"), np.load(tmp_path / "w2.npy")
    assert a.shape == (M,) and np.array_equal(a, b) and np.array_equal(a, np.load(tmp_path / "w3.npy"))
    assert np.array_equal(np.load(tmp_path / "w1.npy.edges.npy"), np.load(tmp_path / "w3.npy.edges.npy"))
    assert 0 < a.sum() < M
    ea, eb = np.load(tmp_path / "w1.npy.edges.npy"), np.load(tmp_path / "w2.npy.edges.npy")
    assert ea.shape == (130,) and np.array_equal(ea, eb) and 0 < ea.sum() < 130      # 130 edges: shards are not whole words
    for w in ("w1", "w2"):                                                           # 131 vertices: shards of 128 and 3 (+ padding rows)
        t, want = np.load(tmp_path / (w + ".npy.knn.npy")), np.load(tmp_path / (w + ".npy.knn_want.npy"))
        assert t.shape == (131, 4) and t.dtype == np.int32 and np.array_equal(t, want)


def test_bench_spawns_its_own_ranks_and_relays_failure():
    """`python bench.py --gpus 2` with no launcher starts two rank processes (before touching torch / the GPU) and
    exits non-zero when a rank fails -- here both do, there is no GPU in this container."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"], env=env, capture_output=True,
                       text=True, timeout=300)
    import torch
    if not torch.cuda.is_available():
        assert p.returncode != 0
        # (the parent terminates the surviving rank as soon as one has failed, so one or two messages arrive)
        assert 1 <= p.stderr.count("needs a GPU") + p.stderr.count("GPU(s)") <= 2, p.stderr[-2000:]


def test_pack_bits_roundtrip(irt):
    rng = np.random.default_rng(1)
    for n in (0, 1, 63, 64, 65, 1000):
        m = rng.random(n) < 0.5
        assert np.array_equal(irt.unpack_bits(irt.distributed.pack_bits(m), n), m)


# ---- .rmp roadmap files <-> CSR voxel caches ------------------------------------------------------------------
def test_rmp_byte_layout_and_roundtrip(irt, tmp_path):
    import struct
    rmp = irt.rmp
    # a file assembled by hand from the layout of RmpStreamer (VoxelCachedLazyPRM.cpp:986-1114)
    blob = struct.pack("<IIB", 2, 1, 1) + struct.pack("<B6d", 64, -0.25, 0.25, -0.25, 0.25, -0.25, 0.25)
    blob += struct.pack("<II3d", 0, 3, 1.0, 2.0, 3.0) + b"\x01" + struct.pack("<3d", 0.1, 0.2, 0.3)
    blob += b"\x01" + struct.pack("<I", 2) + struct.pack("<BBBQ", 1, 2, 3, 0xFF) + struct.pack("<BBBQ", 63, 0, 5, 1 << 63)
    blob += struct.pack("<II3d", 1, 3, 4.0, 5.0, 6.0) + b"\x00" + b"\x00"
    blob += struct.pack("<IId", 0, 1, 5.196) + b"\x01" + struct.pack("<I", 1) + struct.pack("<BBBQ", 0, 0, 0, 7)
    f = tmp_path / "hand.rmp"
    f.write_bytes(blob)
    r = rmp.read_rmp(str(f))
    assert r["N"] == 256 and r["limits"] == (-0.25, 0.25) * 3
    assert np.array_equal(r["states"], [[1, 2, 3], [4, 5, 6]]) and np.array_equal(r["tips"][0], [0.1, 0.2, 0.3])
    assert np.isnan(r["tips"][1]).all() and r["edges"].tolist() == [[0, 1]] and r["weights"][0] == 5.196
    vc = r["vertex_caches"]
    assert vc["offsets"].tolist() == [0, 2, 2] and vc["present"].tolist() == [True, False]
    assert vc["block_ids"].tolist() == [(1 * 64 + 2) * 64 + 3, (63 * 64 + 0) * 64 + 5]
    assert vc["masks"].tolist() == [0xFF, 1 << 63] and r["edge_caches"]["masks"].tolist() == [7]
    # writer reproduces the same bytes
    g = tmp_path / "again.rmp"
    # (a missing tip cannot be expressed per vertex through the array API: write with all tips absent or present)
    rmp.write_rmp(str(g), r["states"], None, r["edges"], r["weights"], vc, r["edge_caches"], N=256, limits=r["limits"])
    r2 = rmp.read_rmp(str(g))
    for k in ("states", "edges", "weights"):
        assert np.array_equal(r[k], r2[k])
    for c in ("vertex_caches", "edge_caches"):
        for k in ("offsets", "block_ids", "masks", "present"):
            assert np.array_equal(r[c][k], r2[c][k])
    # no voxels at all
    h = tmp_path / "plain.rmp"
    rmp.write_rmp(str(h), r["states"], np.array([[0.1, 0.2, 0.3], [0.4, 0.5, 0.6]]), r["edges"], r["weights"])
    r3 = rmp.read_rmp(str(h))
    assert r3["vertex_caches"] is None and np.array_equal(r3["tips"][1], [0.4, 0.5, 0.6])
    assert h.stat().st_size == 9 + 2 * (8 + 24 + 1 + 24) + 16


def test_voxel_octree_set_operations(irt):
    """union / intersect / subtract_block return the old value; remove_point, remove_voxels, intersect_voxels, the leaf and
    occupied-voxel visitors (collision/VoxelOctree.cpp:224-249, 980-1017)."""
    V = irt.VoxelOctree
    a = V(16); a.set_xlim(-1, 1); a.set_ylim(-1, 1); a.set_zlim(-1, 1)
    b = a.empty_copy()
    a.add_sphere([0.1, 0.0, 0.0], 0.4); b.add_sphere([-0.2, 0.1, 0.0], 0.35)
    both = a.empty_copy(); both.add_voxels(a); both.intersect_voxels(b)
    only_a = a.empty_copy(); only_a.add_voxels(a); only_a.remove_voxels(b)
    assert both.ncells() + only_a.ncells() == a.ncells() and 0 < both.ncells() < a.ncells()
    assert not only_a.collides(b) and both.collides(a) and both.collides(b)
    old = a.block(1, 1, 1)
    assert a.union_block(1, 1, 1, 0xF0) == old and a.block(1, 1, 1) == old | 0xF0
    assert a.intersect_block(1, 1, 1, 0xFF) == old | 0xF0 and a.block(1, 1, 1) == (old | 0xF0) & 0xFF
    assert a.subtract_block(1, 1, 1, 0x0F) == (old | 0xF0) & 0xFF and a.block(1, 1, 1) == (old | 0xF0) & 0xF0
    c = a.empty_copy(); c.add_point([0.3, 0.3, 0.3])
    assert c.ncells() == 1
    c.remove_point([5.0, 0.0, 0.0]); assert c.ncells() == 1            # outside the domain: ignored
    c.remove_point([0.3, 0.3, 0.3]); assert c.is_empty()
    seen = []
    both.visit_leaves(lambda bx, by, bz, v: seen.append((bx, by, bz, v)))
    assert len(seen) == both.nblocks() and all(both.block(x, y, z) == v for x, y, z, v in seen)
    occ = both.occupied_voxels()
    assert len(occ) == both.ncells() and all(both.cell(*ix) for ix in occ[:50])
    with pytest.raises(irt.InvalidArgument):
        a.remove_voxels(V(32))


def test_robot_states_from_csv_and_random_state(irt, tmp_path):
    """TendonRobot::read_config_csv / load_config_csv (tendon/TendonRobot.cpp:976-1010): the input of the reference's batch FK
    tools; random_state stays inside the state space; operator==."""
    import io
    robot = irt.workloads.robot_config2()
    robot.enable_rotation = True
    txt = "i,theta,tau_2,extra,tau_1,tau_3\n0,0.5,2.0,x,1.0,3.0\n1,-1.25,5.5,y,4.5,6.5\n\n"
    got = robot.read_config_csv(io.StringIO(txt))
    assert np.array_equal(got, [[1.0, 2.0, 3.0, 0.5], [4.5, 5.5, 6.5, -1.25]])
    p = tmp_path / "configs.csv"
    p.write_text(txt)
    assert np.array_equal(robot.load_config_csv(str(p)), got)
    with pytest.raises(irt.OutOfRange):
        robot.read_config_csv(io.StringIO("tau_1,tau_2\n1,2\n"))
    rng = np.random.default_rng(0)
    robot.enable_retraction = True
    st = np.array([robot.random_state(rng) for _ in range(200)])
    assert st.shape == (200, 5) and (st[:, :3] >= 0).all() and (st[:, :3] <= 20.0).all()
    assert (np.abs(st[:, 3]) <= np.pi).all() and (st[:, 4] >= 0).all() and (st[:, 4] <= robot.specs.L).all()
    same = irt.workloads.robot_config2(); other = irt.workloads.robot_config2()
    assert same == other
    other.tendons[1].max_tension = 7.0
    assert same != other


def test_voxel_environment_table_round_trip(irt, tmp_path):
    """[voxel_environment] of the reference's problem files (motion-planning/VoxelEnvironment.cpp:17-103): rotation as a
    quaternion (w, x, y, z), obstacles by file name or inline."""
    import tomli
    a, b, c = 0.7, -0.4, 1.9
    Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]])
    Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    Ry = np.array([[np.cos(c), 0, np.sin(c)], [0, 1, 0], [-np.sin(c), 0, np.cos(c)]])
    for R in (np.eye(3), Rz, Rz @ Rx, Ry @ Rz @ Rx, np.diag([1.0, -1.0, -1.0]), np.diag([-1.0, -1.0, 1.0])):
        env = irt.VoxelEnvironment(filename="obstacles.msgpack", scaling=1.5, translation=np.array([0.1, -0.2, 0.3]), inv_rotation=R,
                                   interior_fname="inside.nrrd")
        back = irt.VoxelEnvironment.from_toml(tomli.loads(env.to_toml()))
        assert back.filename == "obstacles.msgpack" and back.interior_fname == "inside.nrrd" and back.scaling == 1.5
        assert np.array_equal(back.translation, env.translation) and np.abs(back.inv_rotation - R).max() < 1e-15
        q = irt.VoxelEnvironment._quat_from_matrix(R)
        assert abs(np.linalg.norm(q) - 1) < 1e-15
    vox = irt.VoxelOctree(16)
    vox.set_xlim(-1, 1); vox.set_ylim(-1, 1); vox.set_zlim(-1, 1)
    vox.add_sphere([0.2, 0.1, -0.3], 0.4)
    env = irt.VoxelEnvironment(inv_rotation=Rz)
    env.set_obstacle_cache(vox)
    p = tmp_path / "problem.toml"
    p.write_text(env.to_toml())
    back = irt.VoxelEnvironment.from_toml(str(p))
    assert back.filename == "" and back.get_obstacles() == vox and np.abs(back.inv_rotation - Rz).max() < 1e-15


def test_problem_file_round_trip(irt, tmp_path):
    """motion_planning::Problem::to_toml / from_toml (motion-planning/Problem.cpp:420-560): robot, obstacle primitives, voxel
    environment, start / goal and the validator's resolutions in one flattened file; Environment::voxelize on the host mirror."""
    W = irt.workloads
    robot = W.robot_config3()
    robot.enable_rotation = True
    env = irt.Environment(points=[[0.1, 0.0, 0.05]], spheres=[([0.0, 0.1, 0.1], 0.02), ([0.05, -0.1, 0.12], 0.03)],
                          capsules=[([0.0, 0.0, 0.15], [0.1, 0.05, 0.15], 0.01)])
    a = 0.6
    venv = irt.VoxelEnvironment(filename="env.msgpack", inv_rotation=np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]]))
    pr = irt.Problem(robot=robot, env=env, venv=venv, start=[1, 2, 3, 4], goal=[4, 3, 2, 1], min_tension_change=0.05, min_rotation_change=0.02,
                     start_rotation=0.3, goal_rotation=-0.4)
    path = tmp_path / "problem.toml"
    path.write_text(pr.to_toml())
    back = irt.Problem.from_toml(str(path))
    assert back.robot == robot and back.start == pr.start and back.goal == pr.goal
    assert (back.min_tension_change, back.min_rotation_change, back.min_retraction_change) == (0.05, 0.02, 0.0001)
    assert np.array_equal(back.start_state(), [1, 2, 3, 4, 0.3]) and np.array_equal(back.goal_state(), [4, 3, 2, 1, -0.4])
    assert back.venv.filename == "env.msgpack" and np.abs(back.venv.inv_rotation - venv.inv_rotation).max() < 1e-15
    assert len(back.env.points) == 1 and len(back.env.spheres) == 2 and len(back.env.capsules) == 1
    assert back.env.spheres[1][1] == 0.03 and np.array_equal(back.env.capsules[0][1], [0.1, 0.05, 0.15])
    ref = irt.VoxelOctree(64)
    ref.set_xlim(-0.25, 0.25); ref.set_ylim(-0.25, 0.25); ref.set_zlim(-0.25, 0.25)
    v = back.env.voxelize(ref)
    w = ref.empty_copy()
    w.add_point([0.1, 0.0, 0.05]); w.add_sphere([0.0, 0.1, 0.1], 0.02); w.add_sphere([0.05, -0.1, 0.12], 0.03)
    w.add_capsule([0.0, 0.0, 0.15], [0.1, 0.05, 0.15], 0.01)
    assert v == w and v.ncells() > 50
    # plans (the planners' output CSV)
    plan = np.array([[1, 2, 3, 4, 0.3], [2, 2.5, 3, 3.5, 0.1], [4, 3, 2, 1, -0.4]])
    pfile = tmp_path / "plan.csv"
    back.save_plan(str(pfile), plan)
    assert pfile.read_text().splitlines()[0] == "i,tau_1,tau_2,tau_3,tau_4,theta" and pfile.read_text().splitlines()[1].startswith("1,1.0,2.0")
    assert np.array_equal(irt.Problem.load_plan(str(pfile)), plan)
    assert np.array_equal(back.plan_from_path(plan, [2, 0]), plan[[2, 0]])
    import tomli
    broken = tomli.loads(pr.to_toml())
    del broken["problem"]["goal_rotation"]
    with pytest.raises(irt.OutOfRange):
        irt.Problem.from_toml(broken)


def test_query_paths_are_a_view_on_the_packed_arrays(irt):
    """solveWithRoadmap returns its paths as a sequence over (path_vertices, path_offsets): indexing, negative indices, slices,
    iteration and the empty path of an unsolved query."""
    import importlib
    rm = importlib.import_module("interactive-rate-tendons_amd.roadmap")
    pv, off = np.array([7, 3, 9, 4, 4, 1], dtype=np.int32), np.array([0, 3, 3, 4, 6], dtype=np.int64)
    p = rm._Paths(pv, off)
    assert len(p) == 4 and list(p[0]) == [7, 3, 9] and len(p[1]) == 0 and list(p[2]) == [4] and list(p[-1]) == [4, 1]
    assert [list(x) for x in p] == [[7, 3, 9], [], [4], [4, 1]] and [list(x) for x in p[1:3]] == [[], [4]]
    assert p[0].base is pv or np.shares_memory(p[0], pv)
    with pytest.raises(IndexError):
        p[4]
