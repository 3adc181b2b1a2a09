"""checkMotion on loaded shapes of robots WITH retraction (tr_validate_edges_loaded* on a context opened with
TR_LOADED_RETRACTION_EDGES; csrc/loaded_edges_host.inc), and checker.set_loads on such a robot.

Robots: the loaded-retraction fixtures' config3_ret_edges (N = 4), config2_ret_edges (N = 3), both dL = L / 40 on a 64^3 grid over
+-0.3 m, and config3_rot_ret (rotation, dL = L / 128, 256^3).  Edges and loads: tests/loaded_ret_edges_common.py -- 32 + 2, 32 + 2 and
6 + 2 edges between states of different s_start, one ending at s_start = L, one at s_start < 0; the gravity of a 50 g robot plus
F_e = (0.05, -0.03, 0.02) N.  Every numbered case raises Unsupported without the level-2 opening.

 1 composition, exact: loaded_edges_reference.check_motion_levels driven with device shapes from eng.fk_loaded_batch (World.fk_level
   trims p to n_points and puts s_start into the sample, so the judge takes home_shape(s_start).L_i and the interval test the
   samples' own point counts); the device call gives the level-order driver's valid, n_fk, last_valid_t, n_unconverged and
   n_integrations for EVERY edge, the depth-first driver's valid and last_valid_t for every edge and its n_fk for every valid edge.
 2 the seeded set covers the ground        3 zero load equals the unloaded check
 4 verdicts independent of the library's FK (tests/golden/loaded_ret_edges_config3_ret_edges.npz)
 5 indexed equals pairs, cold and warm     6 schedules do not change a bit
 7 levels and refusals                     8 validators follow set_loads"""
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
import loaded_ret_edges_common as rec                                 # noqa: E402
from loaded_ret_edges_common import WRENCH                            # noqa: E402

pytestmark = pytest.mark.gpu

#         name, frame, warm start, checkMotion(s1, s2, last_valid), sphere checker
CASES = [("config3_ret_edges", "base", False, False, False), ("config3_ret_edges", "world", True, False, False),
         ("config3_ret_edges", "world", True, True, False), ("config3_ret_edges", "world", False, True, True),
         ("config2_ret_edges", "base", False, False, False), ("config2_ret_edges", "world", True, True, True),
         ("config3_rot_ret", "base", False, False, False), ("config3_rot_ret", "world", True, False, False),
         ("config3_rot_ret", "world", False, True, True), ("config3_rot_ret", "world", True, True, False)]
OLD_FK = "loaded FK (general_shape) is not built for robots with retraction"
OLD_EDGES = ("loaded edges (tr_validate_edges_loaded*, tr_*_edges_loaded_indexed): loaded FK (general_shape) is not built for robots with "
             "retraction in this call (tr_fk_loaded_batch*, tr_fk_loaded_tips* and the validity of loaded shapes are)")
OLD_SET_LOADS = ("checker.set_loads: loaded FK (general_shape) is not built for robots with retraction in this call "
                 "(Engine.fk_loaded_batch, fk_loaded_tips and validate_loaded are)")


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
    """One fixture: robot, oracle robot and grid, edges, the two checkers' engines (opened to loaded edges), the device FK behind a cache."""

    def __init__(self, irt, orc, helpers, name):
        import make_fk_truth as mft
        self.irt, self.name = irt, name
        self.robot, self.a, self.b, self.vox = rec.world(irt, name)
        self.dist = rec.dist_of(self.robot)
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
            self._chk[key].engine.set_loaded_retraction(edges=True)
        return self._chk[key]

    def eng(self, spheres=False, **env):
        return self.checker(spheres, **env).engine

    # ---- the device FK of a level, as the edge call evaluates it: per-sample loads (rows under frame WORLD), the guess rule (the
    # accepted base strains of the interval's sample at t_a, unchanged), the state's own points and its s_start ----
    def fk_level(self, frame, warm):
        eng = self.eng()

        def level(states, sa):
            states = np.ascontiguousarray(states)
            w, d = eng.sample_loads(states, WRENCH, self.dist, frame)
            g = np.array([s["vu0"] for s in sa]) if (warm and sa is not None) else None
            keys = [states[i].tobytes() + w[i].tobytes() + d[i].tobytes() + (g[i].tobytes() if g is not None else b"") for i in range(len(states))]
            todo = [i for i, k in enumerate(keys) if k not in self.shapes]
            if todo:
                out = eng.fk_loaded_batch(states[todo], wrench=w[todo], dist=d[todo], guess=None if g is None else g[todo])
                for q, i in enumerate(todo):
                    p = out["p"][q, :int(out["n_points"][q])].copy()
                    self.shapes[keys[i]] = dict(p=p, pts=p, converged=bool(out["converged"][q]), L_i=out["L_i"][q], vu0=out["vu0"][q],
                                                calls=int(out["num_fk_calls"][q]), key=keys[i], s_start=float(states[i, -1]))
            return [self.shapes[k] for k in keys]
        return level

    def python(self, frame, warm, until, spheres, edges=None):
        """The level-order driver's result with the totals the device reports."""
        a, b = (self.a, self.b) if edges is None else edges
        r = ler.check_motion_levels(self.space, self.judge, a, b, self.fk_level(frame, warm), until_invalid=until, spheres=spheres)
        r["n_unconverged"] = sum(not s["converged"] for s in r["samples"])
        r["n_integrations"] = sum(s["calls"] for s in r["samples"])
        return r

    def device(self, frame, warm, until, spheres, edges=None, **env):
        a, b = (self.a, self.b) if edges is None else edges
        return self.eng(spheres, **env).validate_edges_loaded(a, b, wrench=WRENCH, dist=self.dist, frame=frame, warm_start=warm, last_valid=until)


_worlds, _python = {}, {}


@pytest.fixture(scope="module")
def world(irt, orc, helpers):
    def get(name):
        if name not in _worlds:
            _worlds[name] = World(irt, orc, helpers, name)
        return _worlds[name]
    return get


def expected(w, frame, warm, until, spheres):
    key = (w.name, frame, warm, until, spheres)
    if key not in _python:
        _python[key] = w.python(frame, warm, until, spheres)
    return _python[key]


def small_pool(w, until):
    """(deepest edge, TENDON_HIP_EDGE_POOL, copies) of test 6: the smallest pool that holds the deepest edge alone -- every level takes
    whole waves of 64 slots -- and as many copies of that edge as the call puts into its first chunk (9 samples per edge assumed, 13 %
    to spare: edge_plan.hpp), which overflow that pool; test 2 checks that they do, on the Python side."""
    want = expected(w, "world", True, until, False)
    deep = int(np.argmax(want["n_fk"]))
    alone = w.python("world", True, until, False, edges=(w.a[deep:deep + 1], w.b[deep:deep + 1]))
    pool = max(256, need(alone["levels"]))
    return deep, pool, int(0.87 * pool / 9), alone["levels"]


def need(levels):
    return sum((m + 63) // 64 * 64 for m in levels)


def same(got, want, until, what=""):
    for k in ("valid", "n_fk") + (("last_valid_t",) if until else ()):
        assert np.array_equal(got[k], want[k]), (what, k, np.flatnonzero(np.asarray(got[k]) != np.asarray(want[k])))
    for k in ("n_domain_errors", "n_unconverged", "n_integrations"):
        assert got[k] == want[k], (what, k, got[k], want[k])


# ---- 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,frame,warm,until,spheres", CASES, ids=["-".join(str(x) for x in c) for c in CASES])
def test_composition_is_exact(world, name, frame, warm, until, spheres):
    w = world(name)
    want = expected(w, frame, warm, until, spheres)
    got = w.device(frame, warm, until, spheres)
    # (what the warm start does to convergence on these robots is in these lines: compare a warm case with its cold one)
    print("%s %s %s %s %s: %d of %d edges valid, n_fk %d .. %d, levels %s, unconverged %d, %.2f integrations per sample"
          % (name, frame, "warm" if warm else "cold", "until" if until else "plain", "spheres" if spheres else "backbone", want["valid"].sum(),
             len(want["valid"]), want["n_fk"].min(), want["n_fk"].max(), want["levels"], want["n_unconverged"],
             want["n_integrations"] / max(1, len(want["samples"]))))
    same(got, want, until, "level order")
    # the reference's own (depth-first) order on the same device shapes
    level = w.fk_level(frame, warm)
    fk = lambda state, sa: level(np.asarray(state, float).reshape(1, -1), None if sa is None else [sa])[0]
    for e in range(len(w.a)):
        df = ler.check_motion(w.space, w.judge, w.a[e], w.b[e], fk, until_invalid=until, spheres=spheres)
        ok = df["is_fully_valid"] if until else df["valid"]
        assert bool(got["valid"][e]) == ok, e
        if until:
            assert got["last_valid_t"][e] == df["last_valid_t"], e
        if ok:
            assert got["n_fk"][e] == df["n_fk"], e


def test_warm_start_on_retraction_robots_is_reported(world):
    """Nothing is promised about the warm start (the guess holds strains of another arc length): the figures, side by side."""
    for name in rec.FIXTURES:
        w = world(name)
        for warm in (False, True):
            r = w.device("world", warm, False, False)
            how = w.eng().edges_loaded_last()
            print("%s %s: %d unconverged of %d samples, %.2f integrations per sample, %d rounds"
                  % (name, "warm" if warm else "cold", r["n_unconverged"], how["samples"], r["n_integrations"] / how["samples"], how["rounds"]))


# ---- 2 ------------------------------------------------------------------------------------------------------------------------
def test_the_seeded_set_covers_the_ground(world):
    """On the Python side alone (device shapes, the Python bisection)."""
    n_valid = n_invalid = deepest = 0
    levels = []
    for name in rec.FIXTURES:
        for until in (False, True):
            r = expected(world(name), "world", True, until, False)
            n_valid += int(r["valid"].sum()); n_invalid += int((~r["valid"]).sum())
            deepest = max(deepest, int(r["n_fk"].max()))
            levels += r["levels"]
    assert n_valid >= 4 and n_invalid >= 4 and deepest >= 9 and 1 in levels and max(levels) > 64, (n_valid, n_invalid, deepest, levels)
    w = world("config3_ret_edges")
    L, dL = w.robot.specs.L, w.robot.specs.dL
    r = expected(w, "world", True, False, False)
    E = len(w.a)
    ends = r["samples"][:2 * E]                                   # level 0: the end states, a then b of every edge
    na, nb = np.array([len(s["p"]) for s in ends[0::2]]), np.array([len(s["p"]) for s in ends[1::2]])
    assert (np.abs(na - nb) == 1).any()                           # an interval whose two samples differ in point count
    assert (na + 1 < nb).any() and (nb + 1 < na).any()            # ... by more than one point, either way (should_subdivide's first branch)
    near = [s for s in r["samples"] if 0.0 < L - s["s_start"] < dL / 2]
    assert near and all(len(s["p"]) == 1 for s in near)           # a sample within dL / 2 of L: one point, no interval
    at_L = ends[2 * (E + rec.AT_L) + 1]
    assert at_L["s_start"] == L and len(at_L["p"]) == 1 and not at_L["p"].any() and at_L["converged"] and at_L["calls"] == 1
    neg = ends[2 * (E + rec.NEG) + 1]
    assert neg["s_start"] < 0 and not neg["converged"]
    assert not r["valid"][rec.NEG] and r["n_fk"][rec.NEG] == 2    # the negative s_start edge: invalid with its two ends
    # the pool of test 6: holds the deepest edge alone, not the copies of it that make the call's first chunk
    for until in (False, True):
        deep, pool, copies, levels = small_pool(w, until)
        assert need(levels) <= pool < need([copies * m for m in levels]) and need([(copies + 1) // 2 * m for m in levels]) <= pool, (pool, copies, levels)


# ---- 3 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(rec.FIXTURES))
def test_zero_load_is_the_unloaded_check(world, name):
    """No loads: valid, n_fk and last_valid_t are validate_edges' and validate_edges_last_valid's on every seeded edge, with both
    checkers (the shapes agree with the unloaded kernels' to ~1e-15 m where the start is kept; a cell flips only for a coordinate
    that close to a voxel face)."""
    w = world(name)
    for spheres in (False, True):
        eng = w.eng(spheres)
        plain, until = eng.validate_edges(w.a, w.b), eng.validate_edges_last_valid(w.a, w.b)
        for frame in ("base", "world"):
            got = eng.validate_edges_loaded(w.a, w.b, frame=frame, warm_start=False)
            assert np.array_equal(got["valid"], plain["valid"]) and np.array_equal(got["n_fk"], plain["n_fk"]), (spheres, frame)
            assert got["last_valid_t"] is None and got["n_domain_errors"] == 0
            got = eng.validate_edges_loaded(w.a, w.b, frame=frame, warm_start=False, last_valid=True)
            for k in ("valid", "n_fk", "last_valid_t"):
                assert np.array_equal(got[k], until[k]), (spheres, frame, k)
            print("%s %s %s: %d integrations for %d samples, %d unconverged" % (name, "spheres" if spheres else "backbone", frame,
                                                                               got["n_integrations"], got["n_fk"].sum(), got["n_unconverged"]))
    assert plain["n_fk"].max() >= 3 and not plain["valid"][rec.NEG]


# ---- 4 ------------------------------------------------------------------------------------------------------------------------
def test_verdicts_independent_of_the_librarys_fk(irt):
    """tests/golden/loaded_ret_edges_config3_ret_edges.npz (make_loaded_ret_edges.py): edges whose loaded verdict the numpy shooting
    of tests/loaded_ret_reference.py decides with 2 voxels to spare either way -- at least 3 valid loaded and invalid unloaded, 3 the
    reverse.  Only verdict bits are compared."""
    fx = dict(np.load(os.path.join(HERE, "golden", "loaded_ret_edges_config3_ret_edges.npz")))
    robot = rec.robot(irt, "config3_ret_edges")
    vox = irt.VoxelOctree(int(fx["grid"][0]))
    h = float(fx["grid"][1])
    vox.set_xlim(-h, h); vox.set_ylim(-h, h); vox.set_zlim(-h, h)
    eng = irt.VoxelBackboneValidityChecker(robot, irt.VoxelEnvironment(), vox).engine
    eng.set_loaded_retraction(edges=True)
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


# ---- 5 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("warm", [False, True])
def test_indexed_equals_pairs(world, irt, warm):
    w = world("config3_ret_edges")
    eng = w.eng()
    E = len(w.a)
    # every end state a vertex of its own, then edges that share vertices: every edge again, reversed
    states = np.vstack([w.a, w.b])
    edges = np.vstack([np.stack([np.arange(E), E + np.arange(E)], 1), np.stack([E + np.arange(E), np.arange(E)], 1)]).astype(np.int32)
    kw = dict(wrench=WRENCH, dist=w.dist, frame="world", warm_start=warm)
    got = eng.validate_edges_loaded_indexed(states, edges, **kw)
    vu = eng.edges_loaded_vertex_strains(len(states))
    pairs = eng.validate_edges_loaded(states[edges[:, 0]], states[edges[:, 1]], **kw)
    assert np.array_equal(got["valid"], pairs["valid"])
    assert np.array_equal(got["n_fk"], pairs["n_fk"])              # the unloaded indexed form's convention: 2 ends + the edge's own samples
    assert got["n_domain_errors"] == pairs["n_domain_errors"] == 0
    ws, ds = eng.sample_loads(states, WRENCH, w.dist, "world")
    fk = eng.fk_loaded_batch(states, wrench=ws, dist=ds)
    assert np.array_equal(vu, fk["vu0"])
    # every vertex is solved once: the pairs solve each end once per edge
    own = lambda r, ends: int(r["n_integrations"]) - ends
    assert got["n_unconverged"] <= pairs["n_unconverged"]
    assert own(got, int(fk["num_fk_calls"].sum())) == own(pairs, int(fk["num_fk_calls"][edges].sum()))
    same(w.device("world", warm, False, False), expected(w, "world", warm, False, False), False, "pairs after indexed")
    with pytest.raises(irt.InvalidArgument):
        eng.edges_loaded_vertex_strains(len(states))              # a pairwise call since: none resident


# ---- 6 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("until", [False, True])
def test_schedules_do_not_change_a_bit(world, until):
    w = world("config3_ret_edges")
    want = expected(w, "world", True, until, False)
    same(w.device("world", True, until, False, TENDON_HIP_SHOOT_CHUNK="7"), want, until, "chunks of 7")
    w.device("world", True, until, False)
    how, how7 = w.eng().edges_loaded_last(), w.eng(TENDON_HIP_SHOOT_CHUNK="7").edges_loaded_last()
    assert how7["rounds"] > how["rounds"] and how7["samples"] == how["samples"] == len(want["samples"]) and how["levels"] == len(want["levels"])
    assert how["chunks"] == 1
    # the shooting's order: never, always, and always across chunks of 7
    for env in (dict(TENDON_HIP_LOADED_RETRACT_SORT="0"), dict(TENDON_HIP_LOADED_RETRACT_SORT="1"),
                dict(TENDON_HIP_LOADED_RETRACT_SORT="1", TENDON_HIP_SHOOT_CHUNK="7")):
        same(w.device("world", True, until, False, **env), want, until, str(env))
    keys = ("valid", "n_fk") + (("last_valid_t",) if until else ())
    # a pool that the copies of the deepest edge in front of the list overflow (small_pool): retried with fewer edges
    deep, pool, copies, _ = small_pool(w, until)
    rows = np.r_[np.full(copies, deep), np.arange(len(w.a))]
    many = w.device("world", True, until, False, edges=(w.a[rows], w.b[rows]), TENDON_HIP_EDGE_POOL=str(pool))
    for k in keys:
        assert np.array_equal(many[k], want[k][rows]), ("small pool", k)
    assert w.eng(TENDON_HIP_EDGE_POOL=str(pool)).edges_loaded_last()["chunks"] >= 4          # the first chunk overflowed, its halves ran, then the rest
    rev = w.device("world", True, until, False, edges=(w.a[::-1], w.b[::-1]))
    for k in keys:
        assert np.array_equal(rev[k][::-1], want[k]), ("reversed", k)
    assert rev["n_unconverged"] == want["n_unconverged"] and rev["n_integrations"] == want["n_integrations"]
    one = w.device("world", True, until, False, edges=(w.a[deep:deep + 1], w.b[deep:deep + 1]))
    for k in keys:
        assert one[k][0] == want[k][deep], ("alone", k)


# ---- 7 ------------------------------------------------------------------------------------------------------------------------
def test_levels_and_refusals(world, irt):
    w = world("config3_rot_ret")
    a, b = w.a[:2], w.b[:2]
    states, edges = np.vstack([a, b]), np.array([[0, 2], [1, 3]], dtype=np.int32)
    kw = dict(wrench=WRENCH, dist=w.dist)
    chk = irt.VoxelBackboneValidityChecker(w.robot, irt.VoxelEnvironment(), w.vox)
    eng = chk.engine
    edge_calls = dict(pairs=lambda: eng.validate_edges_loaded(a, b, **kw), until=lambda: eng.validate_edges_loaded(a, b, last_valid=True, **kw),
                      indexed=lambda: eng.validate_edges_loaded_indexed(states, edges, **kw))
    voxel_calls = dict(voxelize=lambda: eng.voxelize_edges_loaded_indexed(states, edges, **kw),
                       connect=lambda: eng.voxelize_edges_loaded_indexed(states, edges, validate=True, **kw))

    def messages(calls):
        out = {}
        for name, call in calls.items():
            with pytest.raises(irt.Unsupported) as e:
                call()
            out[name] = str(e.value)
        return out
    # level 0 (never opened) and level 1: the messages the library had before there was a second level, byte for byte
    assert eng.loaded_retraction() == 0
    with pytest.raises(irt.Unsupported) as e0:
        eng.fk_loaded_batch(a)
    assert str(e0.value) == OLD_FK
    assert set(messages(dict(edge_calls, **voxel_calls)).values()) == {OLD_FK}
    eng.set_loaded_retraction()
    assert eng.loaded_retraction() == 1
    assert set(messages(dict(edge_calls, **voxel_calls)).values()) == {OLD_EDGES}
    with pytest.raises(irt.Unsupported) as e1:
        chk.set_loads(**kw)
    assert str(e1.value) == OLD_SET_LOADS
    eng.lib.tr_set_loaded_retraction(eng._ctx, 7)                   # any other non-zero value means 1
    assert eng.loaded_retraction() == 1
    # level 2: the edge calls run, everything above them refuses under its own name
    eng.set_loaded_retraction(edges=True)
    assert eng.loaded_retraction() == 2
    for call in edge_calls.values():
        assert len(call()["valid"]) == 2
    vm = messages(voxel_calls)
    assert all("tr_voxelize_edges_loaded_indexed" in m and "tr_connect_edges_loaded_indexed" in m and "retraction" in m and m != OLD_EDGES
               for m in vm.values()), vm
    rest = messages(dict(sample_valid_vertices_loaded=lambda: eng.sample_valid_vertices_loaded(4, **kw),
                         ik_loaded_batch=lambda: eng.ik_loaded_batch(a, np.zeros(3), **kw),
                         tip_jacobian_loaded=lambda: eng.tip_jacobian_loaded(a, **kw),
                         set_load_profile=lambda: eng.set_load_profile([0.0, 0.1], [1.0, 2.0])))
    assert all("retraction" in m for m in rest.values())
    assert len(set(rest.values()) | set(vm.values())) == len(rest) + 1, (rest, vm)      # each under its own name (the two voxel forms share one)
    with pytest.raises(irt.Unsupported):
        chk.set_loads(profile=([0.0, 0.1], [1.0, 2.0]), **kw)         # through set_load_profile
    assert chk.loads() is None
    # ... and back: closed again
    eng.set_loaded_retraction(False)
    assert eng.loaded_retraction() == 0
    assert set(messages(edge_calls).values()) == {OLD_FK}
    eng.close()


# ---- 8 ------------------------------------------------------------------------------------------------------------------------
def test_validators_follow_set_loads(world, irt):
    w = world("config3_ret_edges")
    for spheres in (False, True):
        chk = w.checker(spheres)
        eng = chk.engine
        mv = irt.VoxelBackboneMotionValidator(chk)
        today = (mv.check_motion_detail(w.a, w.b), mv.check_motion_last_valid(w.a, w.b), chk.is_valid(w.a))
        states = np.vstack([w.a, w.b])
        E = len(w.a)
        edges = np.stack([np.arange(E), E + np.arange(E)], 1).astype(np.int32)
        today_ix = mv.check_motion_indexed(states, edges)
        chk.set_loads(WRENCH, w.dist, frame="world", warm_start=True)
        kw = dict(wrench=WRENCH, dist=w.dist, frame="world", warm_start=True)
        got, want = mv.check_motion_detail(w.a, w.b), eng.validate_edges_loaded(w.a, w.b, **kw)
        for k in ("valid", "n_fk", "n_unconverged", "n_integrations"):
            assert np.array_equal(got[k], want[k]), k
        assert np.array_equal(mv.check_motion(w.a, w.b), want["valid"]) and mv.checkMotion(w.a[0], w.b[0]) == bool(want["valid"][0])
        ok, t = mv.check_motion_last_valid(w.a, w.b)
        want_u = eng.validate_edges_loaded(w.a, w.b, last_valid=True, **kw)
        assert np.array_equal(ok, want_u["valid"]) and np.array_equal(t, want_u["last_valid_t"])
        ix, want_ix = mv.check_motion_indexed(states, edges), eng.validate_edges_loaded_indexed(states, edges, **kw)
        assert np.array_equal(ix["valid"], want_ix["valid"]) and np.array_equal(ix["n_fk"], want_ix["n_fk"])
        ws, ds = eng.sample_loads(w.a, WRENCH, w.dist, "world")
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
    # without the opening set_loads raises the message it always had
    closed = irt.VoxelBackboneValidityChecker(w.robot, irt.VoxelEnvironment(), w.vox)
    with pytest.raises(irt.Unsupported) as e:
        closed.set_loads(WRENCH, w.dist)
    assert str(e.value) == OLD_SET_LOADS and closed.loads() is None
    closed.engine.close()
