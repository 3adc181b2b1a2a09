"""checkMotion on loaded shapes (tr_validate_edges_loaded*, csrc/loaded_edges_host.inc, csrc/loaded_edge_kernel.hpp).

Robots: make_fk_truth's config1 (N = 3), config3_rot (N = 4, rotation) and n8 (N = 8, the one-wave instantiation), on the finest of
the 64^3 / 128^3 / 256^3 grids over +-0.3 m whose voxel the backbone checker accepts for the robot's dL.  32, 32 and 8 seeded edges
with |d tau| <= 1 N and |d theta| <= 0.3; loads: the gravity of a 50 g robot, (0, -2.4525, 0) N/m, plus F_e = (0.05, -0.03, 0.02) N.

 1 composition, exact: the Python bisection of tests/loaded_edges_reference.py (pinned to the C oracle by
   tests/test_loaded_edges_reference.py) driven with device shapes from eng.fk_loaded_batch(state, wrench_s, dist_s, guess) -- the
   per-sample loads (Engine.sample_loads) and the guess rule restated on the host -- and the oracle's predicates on those points.  The
   device call must give the level-order driver's valid, n_fk, last_valid_t, n_unconverged and n_integrations for EVERY edge, and the
   depth-first (reference-order) driver's valid and last_valid_t for every edge and its n_fk for every valid edge (the count of an
   invalid edge belongs to the schedule, as in tests/test_gpu_edges.py).
 2 zero load equals the unloaded check     3 independent of the library's FK (tests/golden/loaded_edges_config3_rot.npz)
 4 indexed equals pairs                    5 schedules do not change a bit
 6 a hopeless load                         7 errors                       8 validators"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.join(HERE, "golden")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import fk_truth_common as ftc                                          # noqa: E402
import loaded_edges_reference as ler                                  # noqa: E402
from loaded_edges_common import DIST, DIST_FULL, FIXTURES, HALF, WRENCH, WRENCH_FULL, grid_dim, make_edges, make_grid      # noqa: E402,F401

pytestmark = pytest.mark.gpu

#         name, frame, warm start, checkMotion(s1, s2, last_valid), sphere checker
CASES = [("config3_rot", "base", False, False, False), ("config3_rot", "world", False, False, False),
         ("config3_rot", "world", True, False, False), ("config3_rot", "world", True, True, False),
         ("config3_rot", "world", False, True, True), ("config3_rot", "base", True, True, True),
         ("config1", "base", False, False, False), ("config1", "world", True, True, False), ("config1", "base", False, True, True),
         ("n8", "world", True, False, False), ("n8", "world", False, True, True)]
# the same under loads with all twelve numbers non-zero (loaded_edges_common: case A's wrench, a distributed row of case D's size): the
# moment row and the z copies of loaded_sample_loads' WORLD frame, and load.l of fk_loaded_uniform, move something
FULL_CASES = [("config3_rot", "world", True, False, False)]
LOADS = {False: (WRENCH, DIST), True: (WRENCH_FULL, DIST_FULL)}
POOL = 512                # TENDON_HIP_EDGE_POOL of test 5: holds the deepest edge alone (7 levels of 64 slots), not the doubled edge list


class MemoJudge(ler.OracleJudge):
    """OracleJudge that remembers what it found for a sample (its key: state, loads and guess as bytes)."""

    def __init__(self, orb, grid):
        super().__init__(orb, grid)
        self.memo = {}

    def _m(self, kind, smp, f):
        k = (kind, smp["key"])
        if k not in self.memo:
            self.memo[k] = f(smp)
        return self.memo[k]

    def shape_valid(self, smp): return self._m("shape", smp, super().shape_valid)
    def backbone_hits(self, smp): return self._m("line", smp, super().backbone_hits)
    def spheres_hit(self, smp): return self._m("sph", smp, super().spheres_hit)


class World:
    """One fixture: robot, oracle robot and grid, edges, the two checkers' engines, and the device FK behind a cache."""

    def __init__(self, irt, orc, helpers, name, env=None):
        import make_fk_truth as mft
        n, eseed, cap, gseed, count, radius = FIXTURES[name]
        self.irt, self.name = irt, name
        self.robot = mft.fixture_robot(irt, name)[0]
        self.a, self.b = make_edges(self.robot, n, eseed, cap)
        self.vox = make_grid(irt, self.robot.specs.dL, gseed, count, radius)
        self.orb, self.og = mft.oracle_robot(self.robot), helpers.oracle_grid(orc, self.vox)
        self.space = ler.Space.of_robot(self.robot)
        self.judge = MemoJudge(self.orb, self.og)
        self._chk = {}
        self.shapes = {}

    def checker(self, spheres=False, **env):
        key = (spheres,) + tuple(sorted(env.items()))
        if key not in self._chk:
            cls = self.irt.VoxelValidityChecker if spheres else self.irt.VoxelBackboneValidityChecker
            with ftc.with_env(**env):
                self._chk[key] = cls(self.robot, self.irt.VoxelEnvironment(), self.vox)
        return self._chk[key]

    def eng(self, spheres=False, **env):
        return self.checker(spheres, **env).engine

    # ---- the device FK of a level, as the edge call evaluates it: per-sample loads, the guess rule ----
    def fk_level(self, frame, warm, loads=(WRENCH, DIST)):
        eng = self.eng()

        def level(states, sa):
            states = np.ascontiguousarray(states)
            w, d = eng.sample_loads(states, loads[0], loads[1], frame)
            g = np.array([s["vu0"] for s in sa]) if (warm and sa is not None) else None
            keys = [states[i].tobytes() + w[i].tobytes() + d[i].tobytes() + (g[i].tobytes() if g is not None else b"") for i in range(len(states))]
            todo = [i for i, k in enumerate(keys) if k not in self.shapes]
            if todo:
                out = eng.fk_loaded_batch(states[todo], wrench=w[todo], dist=d[todo], guess=None if g is None else g[todo])
                for q, i in enumerate(todo):
                    self.shapes[keys[i]] = dict(p=out["p"][q], pts=out["p"][q], converged=bool(out["converged"][q]), L_i=out["L_i"][q],
                                                vu0=out["vu0"][q], calls=int(out["num_fk_calls"][q]), key=keys[i])
            return [self.shapes[k] for k in keys]
        return level

    def python(self, frame, warm, until, spheres, loads=(WRENCH, DIST), edges=None):
        """The level-order driver's result with the totals the device reports."""
        a, b = (self.a, self.b) if edges is None else edges
        r = ler.check_motion_levels(self.space, self.judge, a, b, self.fk_level(frame, warm, loads), until_invalid=until, spheres=spheres)
        r["n_unconverged"] = sum(not s["converged"] for s in r["samples"])
        r["n_integrations"] = sum(s["calls"] for s in r["samples"])
        return r

    def device(self, frame, warm, until, spheres, loads=(WRENCH, DIST), edges=None, **env):
        a, b = (self.a, self.b) if edges is None else edges
        return self.eng(spheres, **env).validate_edges_loaded(a, b, wrench=loads[0], dist=loads[1], frame=frame, warm_start=warm, last_valid=until)


_worlds, _python = {}, {}


@pytest.fixture(scope="module")
def world(irt, orc, helpers):
    def get(name):
        if name not in _worlds:
            _worlds[name] = World(irt, orc, helpers, name)
        return _worlds[name]
    return get


def expected(w, frame, warm, until, spheres, full=False):
    key = (w.name, frame, warm, until, spheres) + (("full",) if full else ())
    if key not in _python:
        _python[key] = w.python(frame, warm, until, spheres, loads=LOADS[full])
    return _python[key]


def same(got, want, until, what=""):
    for k in ("valid", "n_fk") + (("last_valid_t",) if until else ()):
        assert np.array_equal(got[k], want[k]), (what, k, np.flatnonzero(np.asarray(got[k]) != np.asarray(want[k])))
    for k in ("n_domain_errors", "n_unconverged", "n_integrations"):
        assert got[k] == want[k], (what, k, got[k], want[k])


# ---- 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,frame,warm,until,spheres,full", [c + (False,) for c in CASES] + [c + (True,) for c in FULL_CASES],
                         ids=["-".join(str(x) for x in c) for c in CASES] + ["-".join(str(x) for x in c) + "-full" for c in FULL_CASES])
def test_composition_is_exact(world, name, frame, warm, until, spheres, full):
    w = world(name)
    want = expected(w, frame, warm, until, spheres, full)
    got = w.device(frame, warm, until, spheres, loads=LOADS[full])
    print("%s %s %s %s %s%s: %d of %d edges valid, n_fk %d .. %d, levels %s, unconverged %d, %.2f integrations per sample"
          % (name, frame, "warm" if warm else "cold", "until" if until else "plain", "spheres" if spheres else "backbone",
             " under the full load rows" if full else "", want["valid"].sum(),
             len(want["valid"]), want["n_fk"].min(), want["n_fk"].max(), want["levels"], want["n_unconverged"],
             want["n_integrations"] / max(1, len(want["samples"]))))
    same(got, want, until, "level order")
    # the reference's own (depth-first) order on the same device shapes
    level = w.fk_level(frame, warm, LOADS[full])
    fk = lambda state, sa: level(np.asarray(state, float).reshape(1, -1), None if sa is None else [sa])[0]
    for e in range(len(w.a)):
        df = ler.check_motion(w.space, w.judge, w.a[e], w.b[e], fk, until_invalid=until, spheres=spheres)
        ok = df["is_fully_valid"] if until else df["valid"]
        assert bool(got["valid"][e]) == ok, e
        if until:
            assert got["last_valid_t"][e] == df["last_valid_t"], e
        if ok:
            assert got["n_fk"][e] == df["n_fk"], e


def test_the_seeded_set_covers_the_ground(world):
    """On the Python side alone: at least 4 valid and 4 invalid edges, an edge of 9 or more samples, a level of one sample (the
    deepest edge alone, as test 5 runs it) and a level of more than 64 (another launch shape of every kernel of the level), and a
    pool that the small-pool schedule of test 5 overflows with the doubled edge list while it holds the deepest edge alone."""
    n_valid = n_invalid = deepest = 0
    levels = []
    for name in FIXTURES:
        for until in (False, True):
            r = expected(world(name), "world", True, until, False)
            n_valid += int(r["valid"].sum()); n_invalid += int((~r["valid"]).sum())
            deepest = max(deepest, int(r["n_fk"].max()))
            levels += r["levels"]
    w = world("config3_rot")
    need = lambda lv: sum((m + 63) // 64 * 64 for m in lv)
    for until in (False, True):
        r = expected(w, "world", True, until, False)
        deep = int(np.argmax(r["n_fk"]))
        alone = w.python("world", True, until, False, edges=(w.a[deep:deep + 1], w.b[deep:deep + 1]))
        levels += alone["levels"]
        assert need(alone["levels"]) <= POOL < need([2 * m for m in r["levels"]]), (alone["levels"], r["levels"])
    assert n_valid >= 4 and n_invalid >= 4 and deepest >= 9 and 1 in levels and max(levels) > 64, (n_valid, n_invalid, deepest, levels)


# ---- 2 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(FIXTURES))
def test_zero_load_is_the_unloaded_check(world, name):
    """No loads: valid, n_fk and last_valid_t are validate_edges' and validate_edges_last_valid's on every edge (the shapes agree
    with the unloaded kernels' to ~1e-15 m where the start is kept, and a cell flips only for a coordinate that close to a voxel
    face, ~1e-8 expected over the set).  The start of a sample is the unloaded solution of its tensions, which balances the tip
    (round 13: zero iterations), so n_integrations is the number of samples -- on the edges where that premise holds for every t the
    bisection can sample: rows zero_rows_<name> of the golden file (make_loaded_edges.py: solve_initial_bending stops AT
    residual_threshold, and 9 of config3_rot's 32 edges and 1 of n8's 8 hold a state whose start misses it by up to 1.4 % at the tip)."""
    w = world(name)
    rows = np.load(os.path.join(HERE, "golden", "loaded_edges_config3_rot.npz"))["zero_rows_" + name]
    assert len(rows) >= len(w.a) // 2
    for spheres in (False, True):
        eng = w.eng(spheres)
        plain, until = eng.validate_edges(w.a, w.b), eng.validate_edges_last_valid(w.a, w.b)
        for frame in ("base", "world"):
            got = eng.validate_edges_loaded(w.a, w.b, frame=frame, warm_start=False)
            assert np.array_equal(got["valid"], plain["valid"]) and np.array_equal(got["n_fk"], plain["n_fk"])
            assert got["n_unconverged"] == 0 and got["last_valid_t"] is None and got["n_domain_errors"] == 0
            sub = eng.validate_edges_loaded(w.a[rows], w.b[rows], frame=frame, warm_start=False)
            assert np.array_equal(sub["n_fk"], plain["n_fk"][rows]) and sub["n_integrations"] == int(sub["n_fk"].sum())
            got = eng.validate_edges_loaded(w.a, w.b, frame=frame, warm_start=False, last_valid=True)
            for k in ("valid", "n_fk", "last_valid_t"):
                assert np.array_equal(got[k], until[k]), (spheres, frame, k)
            sub = eng.validate_edges_loaded(w.a[rows], w.b[rows], frame=frame, warm_start=False, last_valid=True)
            assert np.array_equal(sub["n_fk"], until["n_fk"][rows]) and sub["n_integrations"] == int(sub["n_fk"].sum())
            print("%s %s %s: %d integrations for %d samples on all edges; %d for %d on the %d rows"
                  % (name, "spheres" if spheres else "backbone", frame, got["n_integrations"], got["n_fk"].sum(), sub["n_integrations"],
                     sub["n_fk"].sum(), len(rows)))
    assert plain["n_fk"].max() >= 3 or name == "config1"


# ---- 3 ------------------------------------------------------------------------------------------------------------------------
def test_verdicts_independent_of_the_librarys_fk(irt):
    """tests/golden/loaded_edges_config3_rot.npz (make_loaded_edges.py): edges whose loaded verdict the numpy shooting decides with
    2 voxels to spare either way -- and at least 3 that are valid loaded and invalid unloaded, 3 the reverse.  The device's and
    the numpy solution of a sample may differ by bound_i <= 1e-5 m, which flips should_subdivide freely: only verdict bits."""
    import make_fk_truth as mft
    fx = dict(np.load(os.path.join(HERE, "golden", "loaded_edges_config3_rot.npz")))
    robot = mft.fixture_robot(irt, "config3_rot")[0]
    vox = irt.VoxelOctree(int(fx["grid"][0]))
    h = float(fx["grid"][1])
    vox.set_xlim(-h, h); vox.set_ylim(-h, h); vox.set_zlim(-h, h)
    eng = irt.VoxelBackboneValidityChecker(robot, irt.VoxelEnvironment(), vox).engine
    eng.grid_add_spheres(fx["spheres"])
    a, b = fx["a"], fx["b"]
    loaded = eng.validate_edges_loaded(a, b, wrench=fx["wrench"], dist=fx["dist"], frame="world", warm_start=False)
    warm = eng.validate_edges_loaded(a, b, wrench=fx["wrench"], dist=fx["dist"], frame="world", warm_start=True)
    unloaded = eng.validate_edges(a, b)
    assert np.array_equal(loaded["valid"], fx["valid_loaded"].astype(bool))
    assert np.array_equal(warm["valid"], fx["valid_loaded"].astype(bool))
    assert np.array_equal(unloaded["valid"], fx["valid_unloaded"].astype(bool))
    assert (loaded["valid"] & ~unloaded["valid"]).sum() >= 3 and (~loaded["valid"] & unloaded["valid"]).sum() >= 3
    assert loaded["n_unconverged"] == 0


# ---- 4 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("warm", [False, True])
def test_indexed_equals_pairs(world, warm):
    w = world("config3_rot")
    eng = w.eng()
    E = len(w.a)
    # every end state a vertex of its own, then edges that share vertices: every edge again, reversed
    states = np.vstack([w.a, w.b])
    edges = np.vstack([np.stack([np.arange(E), E + np.arange(E)], 1), np.stack([E + np.arange(E), np.arange(E)], 1)]).astype(np.int32)
    got = eng.validate_edges_loaded_indexed(states, edges, wrench=WRENCH, dist=DIST, frame="world", warm_start=warm)
    vu = eng.edges_loaded_vertex_strains(len(states))
    pairs = eng.validate_edges_loaded(states[edges[:, 0]], states[edges[:, 1]], wrench=WRENCH, dist=DIST, frame="world", warm_start=warm)
    assert np.array_equal(got["valid"], pairs["valid"])
    assert np.array_equal(got["n_fk"], pairs["n_fk"])              # the unloaded indexed form's convention: 2 ends + the edge's own samples
    assert got["n_domain_errors"] == pairs["n_domain_errors"] == 0
    ws, ds = eng.sample_loads(states, WRENCH, DIST, "world")
    fk = eng.fk_loaded_batch(states, wrench=ws, dist=ds)
    assert np.array_equal(vu, fk["vu0"])
    # every vertex is solved once: the pairs solve each end once per edge
    own = lambda r, ends: int(r["n_integrations"]) - ends
    assert got["n_unconverged"] <= pairs["n_unconverged"]
    assert own(got, int(fk["num_fk_calls"].sum())) == own(pairs, int(fk["num_fk_calls"][edges].sum()))
    same(w.device("world", warm, False, False), expected(w, "world", warm, False, False), False, "pairs after indexed")
    with pytest.raises(irt_error(w, "InvalidArgument")):
        eng.edges_loaded_vertex_strains(len(states))              # a pairwise call since: none resident


def irt_error(w, name):
    return getattr(w.irt, name)


# ---- 5 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("until", [False, True])
def test_schedules_do_not_change_a_bit(world, until):
    w = world("config3_rot")
    want = expected(w, "world", True, until, False)
    same(w.device("world", True, until, False, TENDON_HIP_SHOOT_CHUNK="7"), want, until, "chunks of 7")
    w.device("world", True, until, False)
    how, how7 = w.eng().edges_loaded_last(), w.eng(TENDON_HIP_SHOOT_CHUNK="7").edges_loaded_last()
    assert how7["rounds"] > how["rounds"] and how7["samples"] == how["samples"] == len(want["samples"]) and how["levels"] == len(want["levels"])
    assert how["chunks"] == 1
    keys = ("valid", "n_fk") + (("last_valid_t",) if until else ())
    # a pool that the edge list, taken twice, overflows (test_the_seeded_set_covers_the_ground): retried with fewer edges
    twice = w.device("world", True, until, False, edges=(np.vstack([w.a, w.a]), np.vstack([w.b, w.b])), TENDON_HIP_EDGE_POOL=str(POOL))
    E = len(w.a)
    for k in keys:
        assert np.array_equal(twice[k][:E], want[k]) and np.array_equal(twice[k][E:], want[k]), ("small pool", k)
    assert twice["n_unconverged"] == 2 * want["n_unconverged"] and twice["n_integrations"] == 2 * want["n_integrations"]
    assert w.eng(TENDON_HIP_EDGE_POOL=str(POOL)).edges_loaded_last()["chunks"] >= 3          # the whole list overflowed, its halves ran
    rev = w.device("world", True, until, False, edges=(w.a[::-1], w.b[::-1]))
    for k in keys:
        assert np.array_equal(rev[k][::-1], want[k]), ("reversed", k)
    assert rev["n_unconverged"] == want["n_unconverged"] and rev["n_integrations"] == want["n_integrations"]
    deep = int(np.argmax(want["n_fk"]))
    one = w.device("world", True, until, False, edges=(w.a[deep:deep + 1], w.b[deep:deep + 1]))
    for k in keys:
        assert one[k][0] == want[k][deep], ("alone", k)


# ---- 6 ------------------------------------------------------------------------------------------------------------------------
def test_a_hopeless_load(world):
    w = world("config3_rot")
    heavy = np.array([1e6, 0.0, 0.0, 0.0, 0.0, 0.0])
    for until in (False, True):
        got = w.device("world", True, until, False, loads=(heavy, DIST))
        assert not got["valid"].any() and got["n_unconverged"] > 0
        if until:
            assert (got["last_valid_t"] == 0.0).all()
        same(w.device("world", True, until, False), expected(w, "world", True, until, False), until, "after the hopeless load")


# ---- 7 ------------------------------------------------------------------------------------------------------------------------
def test_errors(world, irt):
    import ctypes as C
    w = world("config1")
    eng = w.eng()
    ret = irt.workloads.robot_config1()
    ret.enable_retraction = True
    reng = irt.Engine(ret, 0)
    with pytest.raises(irt.Unsupported) as e1:
        reng.validate_edges_loaded(np.zeros((2, 4)), np.ones((2, 4)))
    with pytest.raises(irt.Unsupported) as e2:
        reng.fk_loaded_batch(np.zeros((2, 4)))
    assert str(e1.value) == str(e2.value)                              # shoot_check's wording
    with pytest.raises(irt.Unsupported):
        reng.validate_edges_loaded_indexed(np.zeros((2, 4)), [[0, 1]])
    bare = irt.Engine(w.robot, 0)
    with pytest.raises(irt.InvalidArgument):
        bare.validate_edges_loaded(w.a, w.b)                           # no grid
    with pytest.raises(irt.InvalidArgument):
        bare.validate_edges_loaded_indexed(np.vstack([w.a, w.b]), [[0, 1]])
    for kw in (dict(min_tension_change=0.0), dict(min_tension_change=-1.0)):
        with pytest.raises(irt.InvalidArgument):
            eng.validate_edges_loaded(w.a, w.b, **kw)
    rot = world("config3_rot")
    with pytest.raises(irt.InvalidArgument):
        rot.eng().validate_edges_loaded(rot.a, rot.b, min_rotation_change=0.0)
    with pytest.raises(irt.InvalidArgument):
        eng.validate_edges_loaded(w.a, w.b, frame="tool")
    with pytest.raises(irt.InvalidArgument):
        eng.validate_edges_loaded(w.a, w.b, wrench=np.zeros((len(w.a), 6)))
    with pytest.raises(irt.InvalidArgument):
        eng.validate_edges_loaded(w.a, w.b, max_iters=-1)
    with pytest.raises(irt.OutOfRange):
        eng.validate_edges_loaded_indexed(w.a, [[0, len(w.a)]])
    empty = eng.validate_edges_loaded(np.zeros((0, 3)), np.zeros((0, 3)), wrench=WRENCH, dist=DIST)
    assert len(empty["valid"]) == 0 and empty["n_integrations"] == 0
    assert len(bare.validate_edges_loaded(np.zeros((0, 3)), np.zeros((0, 3)))["valid"]) == 0     # n_edges == 0 is TR_OK before the grid is asked for
    assert len(eng.validate_edges_loaded_indexed(w.a, np.zeros((0, 2), dtype=np.int32))["valid"]) == 0
    # the C ABI: a frame that is neither, null loads = no load
    sp, ld = irt._lib.TrSpaceParams(0.02, 0.01, 0.0001), irt._lib.TrEdgeLoads()
    ld.frame = 2
    bits = np.zeros(1, dtype=np.uint64)
    dp = lambda x: x.ctypes.data_as(C.POINTER(C.c_double))
    u64 = bits.ctypes.data_as(C.POINTER(C.c_uint64))
    assert eng.lib.tr_validate_edges_loaded(eng._ctx, C.byref(sp), None, C.byref(ld), dp(w.a), dp(w.b), len(w.a), u64, None, None, None, None,
                                            None) == irt._lib.TR_ERR_INVALID_ARG
    assert eng.lib.tr_validate_edges_loaded(eng._ctx, C.byref(sp), None, None, dp(w.a), dp(w.b), len(w.a), u64, None, None, None, None,
                                            None) == irt._lib.TR_OK
    assert np.array_equal(irt.unpack_bits(bits, len(w.a)), eng.validate_edges(w.a, w.b)["valid"])
    bare.close(); reng.close()


# ---- 8 ------------------------------------------------------------------------------------------------------------------------
def test_validators_follow_set_loads(world, irt):
    w = world("config3_rot")
    for spheres in (False, True):
        chk = w.checker(spheres)
        eng = chk.engine
        mv = irt.VoxelBackboneMotionValidator(chk)
        today = (mv.check_motion_detail(w.a, w.b), mv.check_motion_last_valid(w.a, w.b), chk.is_valid(w.a))
        states = np.vstack([w.a, w.b])
        E = len(w.a)
        edges = np.stack([np.arange(E), E + np.arange(E)], 1).astype(np.int32)
        today_ix = mv.check_motion_indexed(states, edges)
        chk.set_loads(WRENCH, DIST, frame="world", warm_start=True)
        kw = dict(wrench=WRENCH, dist=DIST, frame="world", warm_start=True)
        got, want = mv.check_motion_detail(w.a, w.b), eng.validate_edges_loaded(w.a, w.b, **kw)
        for k in ("valid", "n_fk", "n_unconverged", "n_integrations"):
            assert np.array_equal(got[k], want[k]), k
        assert np.array_equal(mv.check_motion(w.a, w.b), want["valid"]) and mv.checkMotion(w.a[0], w.b[0]) == bool(want["valid"][0])
        ok, t = mv.check_motion_last_valid(w.a, w.b)
        want_u = eng.validate_edges_loaded(w.a, w.b, last_valid=True, **kw)
        assert np.array_equal(ok, want_u["valid"]) and np.array_equal(t, want_u["last_valid_t"])
        ix, want_ix = mv.check_motion_indexed(states, edges), eng.validate_edges_loaded_indexed(states, edges, **kw)
        assert np.array_equal(ix["valid"], want_ix["valid"]) and np.array_equal(ix["n_fk"], want_ix["n_fk"])
        ws, ds = eng.sample_loads(w.a, WRENCH, DIST, "world")
        assert np.array_equal(chk.is_valid(w.a), eng.validate_loaded(w.a, wrench=ws, dist=ds)["valid"])
        with pytest.raises(irt.Unsupported):
            irt.VoxelBackboneDiscreteMotionValidator(chk).check_motion(w.a, w.b)
        chk.clear_loads()
        again = (mv.check_motion_detail(w.a, w.b), mv.check_motion_last_valid(w.a, w.b), chk.is_valid(w.a))
        for k in ("valid", "n_fk"):
            assert np.array_equal(again[0][k], today[0][k])
        assert np.array_equal(again[1][0], today[1][0]) and np.array_equal(again[1][1], today[1][1]) and np.array_equal(again[2], today[2])
        assert np.array_equal(mv.check_motion_indexed(states, edges)["valid"], today_ix["valid"])
        assert irt.VoxelBackboneDiscreteMotionValidator(chk).check_motion(w.a, w.b).shape == (E,)
