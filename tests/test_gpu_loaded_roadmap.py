"""The roadmap build on loaded shapes (tr_sample_valid_vertices_loaded, tr_voxelize_batch_loaded, tr_voxelize_edges_loaded_indexed,
tr_connect_edges_loaded_indexed; csrc/loaded_roadmap_host.inc, csrc/loaded_roadmap_kernel.hpp) and RoadmapBuilder under set_loads.

Worlds, loads and grids: tests/loaded_edges_common.py (config1 -- frame base --, config3_rot and n8 -- frame world).

 1 the vertex phase is the prefix filter of the candidate sequence under the loaded verdict; tips, strains and the two sums are
   fk_loaded_batch's; a continued run and small batches give the same set
 2 independent of the library's FK (tests/golden/loaded_roadmap_config3_rot.npz)        3 zero load is the unloaded vertex phase
 4 vertex voxel sets are the oracle's add_piecewise_line of the loaded points           5 edge voxel sets and connect
 6 one shape per vertex across the phases       7 the builder is the composition of the calls       8 errors

The reference verdict of test 1 is Engine.validate_loaded on the candidates.  tr_validate_shapes_dev, which it ends in, sweeps the
BACKBONE whatever checker is installed; the vertex phase asks the installed checker, as the unloaded vertex phase and the loaded edge
calls do.  Under the sphere checker the reference is therefore validate_loaded without the voxel test (is_valid_shape) and the
oracle's add_sphere / collides on fk_loaded_batch's points -- the predicate tests/test_gpu_loaded_edges.py pins the device's sphere
test to, sample for sample."""
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
from loaded_edges_common import DIST, FIXTURES, WRENCH, make_edges, make_grid      # noqa: E402

pytestmark = pytest.mark.gpu

FRAME = {"config1": "base", "config3_rot": "world", "n8": "world"}
LOADS = dict(wrench=WRENCH, dist=DIST)
MAX_CAND = 256
POOL = 512


def n_want(name):
    return 16 if name == "n8" else 48


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

    def __init__(self, irt, orc, helpers, name):
        import make_fk_truth as mft
        n, eseed, cap, gseed, count, radius = FIXTURES[name]
        self.irt, self.name, self.frame = irt, name, FRAME[name]
        self.robot = mft.fixture_robot(irt, name)[0]
        self.a, self.b = make_edges(self.robot, n, eseed, cap)
        self.vox = make_grid(irt, self.robot.specs.dL, gseed, count, radius)
        self.orb, self.og = mft.oracle_robot(self.robot), helpers.oracle_grid(orc, self.vox)
        self.space = ler.Space.of_robot(self.robot)
        self.judge = MemoJudge(self.orb, self.og)
        self._chk = {}
        self.shapes = {}
        self._phase = {}
        # the gathered pairs: every end state a vertex of its own
        E = len(self.a)
        self.states = np.vstack([self.a, self.b])
        self.edges = np.stack([np.arange(E), E + np.arange(E)], 1).astype(np.int32)

    def checker(self, spheres=False, **env):
        key = (spheres,) + tuple(sorted(env.items()))
        if key not in self._chk:
            cls = self.irt.VoxelValidityChecker if spheres else self.irt.VoxelBackboneValidityChecker
            with ftc.with_env(**env):
                self._chk[key] = cls(self.robot, self.irt.VoxelEnvironment(), self.vox)
        return self._chk[key]

    def eng(self, spheres=False, **env):
        return self.checker(spheres, **env).engine

    # the device FK of a level, as the edge calls evaluate it: per-sample loads, the guess rule (test_gpu_loaded_edges.py's construction)
    def fk_level(self, frame, warm):
        eng = self.eng()

        def level(states, sa):
            states = np.ascontiguousarray(states)
            w, d = eng.sample_loads(states, WRENCH, DIST, frame)
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

    def samples(self, states, frame=None):
        """cold device shapes of `states` under the world's loads, as the judge takes them"""
        return self.fk_level(frame or self.frame, False)(states, None)

    def phase(self, spheres):
        """The vertex phase of test 1 and everything its checks need, computed once: the call, the candidates, their loads, their
        shapes and the reference verdict."""
        if spheres not in self._phase:
            eng = self.eng(spheres)
            out = eng.sample_valid_vertices_loaded(n_want(self.name), frame=self.frame, seed=0, max_candidates=MAX_CAND, want_index=True, **LOADS)
            cand = eng.candidate_states(0, 0, MAX_CAND)
            ws, ds = eng.sample_loads(cand, WRENCH, DIST, self.frame)
            fk = eng.fk_loaded_batch(cand, wrench=ws, dist=ds)
            if spheres:
                valid = eng.validate_loaded(cand, ws, ds, check_voxels=False)["valid"].copy()
                backbone = eng.validate_loaded(cand, ws, ds)["valid"]
                for i in np.flatnonzero(valid):
                    valid[i] = not self.judge.spheres_hit(dict(pts=fk["p"][i], key=("cand", i)))
                print("%s: the sphere test rejects %d candidates the backbone test accepts" % (self.name, int((backbone & ~valid).sum())))
            else:
                valid = eng.validate_loaded(cand, ws, ds)["valid"]
            self._phase[spheres] = dict(out=out, cand=cand, ws=ws, ds=ds, fk=fk, valid=valid)
        return self._phase[spheres]


_worlds = {}


@pytest.fixture(scope="module")
def world(irt, orc, helpers):
    def get(name):
        if name not in _worlds:
            _worlds[name] = World(irt, orc, helpers, name)
        return _worlds[name]
    return get


def _item(out, i):
    a, b = out["offsets"][i], out["offsets"][i + 1]
    ids, masks = np.asarray(out["block_ids"][a:b]), np.asarray(out["masks"][a:b])
    o = np.argsort(ids, kind="stable")
    return ids[o], masks[o]


def _same_lists(x, y):
    return all(np.array_equal(np.asarray(x[k]), np.asarray(y[k])) for k in ("offsets", "block_ids", "masks"))


# ---- 1 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spheres", [False, True])
@pytest.mark.parametrize("name", list(FIXTURES))
def test_vertex_phase_is_the_prefix_filter(world, name, spheres):
    w = world(name)
    ph = w.phase(spheres)
    out, cand, valid, fk = ph["out"], ph["cand"], ph["valid"], ph["fk"]
    nw = n_want(name)
    all_idx = np.flatnonzero(valid)
    idx = all_idx[:nw]
    tried = int(idx[-1]) + 1 if len(all_idx) >= nw else MAX_CAND
    print("%s %s: %d of %d accepted after %d candidates, %d unconverged, %d integrations"
          % (name, "spheres" if spheres else "backbone", out["accepted"], nw, out["tried"], out["n_unconverged"], out["n_integrations"]))
    assert out["accepted"] == len(idx) and out["tried"] == tried
    assert np.array_equal(out["index"], idx)
    assert np.array_equal(out["states"], cand[idx])
    # tips and strains: fk_loaded_batch's, bit for bit (the issue's form of the call: on the accepted states and their rows)
    own = w.eng(spheres).fk_loaded_batch(out["states"], wrench=ph["ws"][idx], dist=ph["ds"][idx])
    assert np.array_equal(out["tips"], own["p"][:, -1]) and np.array_equal(out["vu0"], own["vu0"])
    assert np.array_equal(own["p"], fk["p"][idx]) and np.array_equal(own["vu0"], fk["vu0"][idx])
    assert out["n_unconverged"] == int((~fk["converged"][:tried]).sum())
    assert out["n_integrations"] == int(fk["num_fk_calls"][:tried].sum())
    assert len(idx) == nw or name != "config1"
    assert not valid[:tried].all()                                                   # the filter had something to reject


@pytest.mark.parametrize("spheres", [False, True])
@pytest.mark.parametrize("name", list(FIXTURES))
def test_vertex_phase_continued_and_in_small_batches(world, name, spheres):
    w = world(name)
    want = w.phase(spheres)["out"]
    nw = n_want(name)
    eng = w.eng(spheres)
    kw = dict(frame=w.frame, seed=0, want_index=True, **LOADS)
    head = nw // 3
    a = eng.sample_valid_vertices_loaded(head, max_candidates=MAX_CAND, **kw)
    b = eng.sample_valid_vertices_loaded(nw - head, first_candidate=a["tried"], max_candidates=MAX_CAND - a["tried"], **kw)
    for k in ("states", "tips", "index", "vu0"):
        assert np.array_equal(np.concatenate([a[k], b[k]]), want[k]), k
    assert a["tried"] + b["tried"] == want["tried"]
    assert a["n_integrations"] + b["n_integrations"] == want["n_integrations"]
    assert a["n_unconverged"] + b["n_unconverged"] == want["n_unconverged"]
    small = w.eng(spheres, TENDON_HIP_LOADED_VERTEX_BATCH="64", TENDON_HIP_SHOOT_CHUNK="7")
    got = small.sample_valid_vertices_loaded(nw, max_candidates=MAX_CAND, **kw)
    for k in ("states", "tips", "index", "vu0"):
        assert np.array_equal(got[k], want[k]), k
    for k in ("accepted", "tried", "n_unconverged", "n_integrations"):
        assert got[k] == want[k], k
    batches = small.edges_loaded_last()["levels"]                     # one evaluator call per batch, each in chunks of 7
    assert batches == (want["tried"] + 63) // 64 and (batches > 1 or name != "config1")


def test_the_load_moves_the_accepted_set(world):
    w = world("config1")
    loaded = w.phase(False)["out"]
    unloaded = w.eng().sample_valid_vertices(n_want("config1"), seed=0, max_candidates=MAX_CAND, want_index=True)
    assert unloaded["accepted"] == loaded["accepted"] == n_want("config1")
    assert not np.array_equal(unloaded["index"], loaded["index"])
    gravity = w.eng().sample_valid_vertices_loaded(n_want("config1"), dist=DIST, frame="base", seed=0, max_candidates=MAX_CAND, want_index=True)
    print("config1: 48 accepted within %d candidates unloaded, %d under gravity, %d under gravity and the wrench"
          % (unloaded["tried"], gravity["tried"], loaded["tried"]))
    assert not np.array_equal(unloaded["index"], gravity["index"])


# ---- 2 ------------------------------------------------------------------------------------------------------------------------
def test_accept_flags_independent_of_the_librarys_fk(irt):
    """tests/golden/loaded_roadmap_config3_rot.npz (make_loaded_roadmap.py): the first 128 candidates of seed 0 solved by the numpy
    shooting under WORLD loads; `decided`: the numpy shape is valid and its backbone misses the fixture's spheres grown by 2 voxels
    or hits them shrunk by 2 voxels.  The device's accept flag equals the file's verdict on every decided candidate."""
    import make_fk_truth as mft
    fx = dict(np.load(os.path.join(HERE, "golden", "loaded_roadmap_config3_rot.npz")))
    robot = mft.fixture_robot(irt, "config3_rot")[0]
    vox = irt.VoxelOctree(int(fx["grid"][0]))
    h = float(fx["grid"][1])
    vox.set_xlim(-h, h); vox.set_ylim(-h, h); vox.set_zlim(-h, h)
    eng = irt.VoxelBackboneValidityChecker(robot, irt.VoxelEnvironment(), vox).engine
    eng.grid_add_spheres(fx["spheres"])
    n = len(fx["states"])
    assert np.array_equal(eng.candidate_states(0, 0, n), fx["states"])
    out = eng.sample_valid_vertices_loaded(n, wrench=fx["wrench"], dist=fx["dist"], frame="world", seed=0, max_candidates=n, want_index=True)
    accept = np.zeros(n, dtype=bool)
    accept[out["index"]] = True
    dec = fx["decided"].astype(bool)
    assert dec.sum() >= 100
    assert np.array_equal(accept[dec], fx["valid_loaded"].astype(bool)[dec]), np.flatnonzero(dec & (accept != fx["valid_loaded"].astype(bool)))
    un = eng.sample_valid_vertices(n, seed=0, max_candidates=n, want_index=True)
    unl = np.zeros(n, dtype=bool)
    unl[un["index"]] = True
    assert (accept[dec] != unl[dec]).sum() >= 10
    assert out["n_unconverged"] == 0


# ---- 3 ------------------------------------------------------------------------------------------------------------------------
def test_zero_load_is_the_unloaded_vertex_phase(world):
    w = world("config1")
    for spheres in (False, True):
        eng = w.eng(spheres)
        want = eng.sample_valid_vertices(48, seed=0, max_candidates=MAX_CAND, want_index=True)
        for frame in ("base", "world"):
            got = eng.sample_valid_vertices_loaded(48, frame=frame, seed=0, max_candidates=MAX_CAND, want_index=True)
            assert np.array_equal(got["states"], want["states"]) and np.array_equal(got["index"], want["index"])
            assert got["tried"] == want["tried"] and got["accepted"] == want["accepted"] == 48
            err = np.abs(got["tips"] - want["tips"]).max()
            print("config1 %s %s: zero-load tips within %.3g m of the unloaded ones" % ("spheres" if spheres else "backbone", frame, err))
            assert err <= 1e-9
            assert got["n_unconverged"] == 0


# ---- 4 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(FIXTURES))
def test_vertex_voxel_sets(world, name):
    w = world(name)
    ph = w.phase(False)
    # the accepted states of test 1 and the first 32 candidates (rejected ones among them)
    states = np.vstack([ph["out"]["states"], ph["cand"][:32]])
    eng = w.eng()
    out = eng.voxelize_batch_loaded(states, frame=w.frame, **LOADS)
    smp = w.samples(states)
    want_shape = np.array([w.judge.shape_valid(s) for s in smp])
    assert np.array_equal(out["shape_valid"], want_shape)
    assert want_shape[:len(ph["out"]["states"])].all()
    assert np.array_equal(out["tips"], np.array([s["p"][-1] for s in smp]))
    assert np.array_equal(out["tips"][:len(ph["out"]["tips"])], ph["out"]["tips"])
    assert out["n_unconverged"] == sum(not s["converged"] for s in smp) and out["n_integrations"] == sum(s["calls"] for s in smp)
    for i, s in enumerate(smp):
        ids, masks = _item(out, i)
        if not want_shape[i]:
            assert len(ids) == 0
            continue
        g = w.og.empty_copy()
        g.add_piecewise_line(s["pts"])
        wi, wm = g.export_blocks()
        assert np.array_equal(ids, wi) and np.array_equal(masks, wm), i
    dev = eng.voxelize_batch_loaded(states, frame=w.frame, device=True, **LOADS)
    assert np.array_equal(dev["block_ids"].cpu().numpy().view(np.uint32), out["block_ids"])
    assert np.array_equal(dev["masks"].cpu().numpy().view(np.uint64), out["masks"])


def test_vertex_voxel_sets_follow_the_load(irt, orc):
    """The three verdict states of tests/golden/loaded_fk_config3_rot.npz: the loaded set meets the sphere on the loaded tip and not the
    one on the unloaded tip; voxelize_batch shows the reverse."""
    import make_fk_truth as mft
    fx = dict(np.load(os.path.join(HERE, "golden", "loaded_fk_config3_rot.npz")))
    eng = irt.Engine(mft.fixture_robot(irt, "config3_rot")[0], 0)
    N, half = int(fx["verdict_grid"][0]), float(fx["verdict_grid"][1])
    lim = (-half, half) * 3
    assert len(fx["verdict_states"]) == 3
    for k, i in enumerate(fx["verdict_states"]):
        st, dist = fx["states"][i:i + 1], fx["dist_B"][i]
        for sphere, on_loaded in ((fx["verdict_sphere_loaded"][k], True), (fx["verdict_sphere_unloaded"][k], False)):
            g = orc.Grid(N, lim)
            g.add_sphere(sphere[:3], sphere[3])
            eng.set_grid(N, lim, g.blocks())
            ld = eng.voxelize_batch_loaded(st, dist=dist, frame="base")
            un = eng.voxelize_batch(st)
            assert ld["shape_valid"][0] and un["shape_valid"][0]
            assert bool(eng.check_cached(ld["block_ids"], ld["masks"], ld["offsets"])[0]) == on_loaded
            assert bool(eng.check_cached(un["block_ids"], un["masks"], un["offsets"])[0]) == (not on_loaded)
    eng.close()


# ---- 5 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("warm", [False, True])
@pytest.mark.parametrize("frame", ["base", "world"])
@pytest.mark.parametrize("name", list(FIXTURES))
def test_edge_voxel_sets_and_connect(world, name, frame, warm):
    w = world(name)
    eng = w.eng()
    kw = dict(frame=frame, warm_start=warm, **LOADS)
    vox = eng.voxelize_edges_loaded_indexed(w.states, w.edges, **kw)
    level = w.fk_level(frame, warm)
    fk = lambda state, sa: level(np.asarray(state, float).reshape(1, -1), None if sa is None else [sa])[0]
    n_full = 0
    for e in range(len(w.a)):
        df = ler.check_motion(w.space, w.judge, w.a[e], w.b[e], fk, want_swept=True)
        assert bool(vox["fully_valid"][e]) == df["is_fully_valid"], e
        ids, masks = _item(vox, e)
        if not df["is_fully_valid"]:
            assert len(ids) == 0, e
            continue
        n_full += 1
        wi, wm = df["swept"].export_blocks()
        assert np.array_equal(ids, wi) and np.array_equal(masks, wm), e
        assert vox["n_fk"][e] == df["n_fk"], e
    assert n_full >= 1
    conn = eng.voxelize_edges_loaded_indexed(w.states, w.edges, validate=True, **kw)
    strains = eng.edges_loaded_vertex_strains(len(w.states))
    verdict = eng.validate_edges_loaded_indexed(w.states, w.edges, **kw)
    assert np.array_equal(conn["fully_valid"], verdict["valid"]) and np.array_equal(conn["n_fk"], verdict["n_fk"])
    assert conn["n_unconverged"] == verdict["n_unconverged"] and conn["n_integrations"] == verdict["n_integrations"]
    assert np.array_equal(strains, eng.edges_loaded_vertex_strains(len(w.states)))
    print("%s %s %s: %d of %d edges fully valid, %d valid; %d blocks" % (name, frame, "warm" if warm else "cold", n_full, len(w.a),
                                                                         int(conn["fully_valid"].sum()), int(conn["offsets"][-1])))
    for e in range(len(w.a)):
        ids, masks = _item(conn, e)
        if conn["fully_valid"][e]:
            assert vox["fully_valid"][e]
            vi, vm = _item(vox, e)
            assert np.array_equal(ids, vi) and np.array_equal(masks, vm), e
        else:
            assert len(ids) == 0, e


def test_connect_on_the_golden_edges(irt):
    import make_fk_truth as mft
    fx = dict(np.load(os.path.join(HERE, "golden", "loaded_edges_config3_rot.npz")))
    robot = mft.fixture_robot(irt, "config3_rot")[0]
    vox = irt.VoxelOctree(int(fx["grid"][0]))
    h = float(fx["grid"][1])
    vox.set_xlim(-h, h); vox.set_ylim(-h, h); vox.set_zlim(-h, h)
    eng = irt.VoxelBackboneValidityChecker(robot, irt.VoxelEnvironment(), vox).engine
    eng.grid_add_spheres(fx["spheres"])
    a, b = fx["a"], fx["b"]
    E = len(a)
    states = np.vstack([a, b])
    edges = np.stack([np.arange(E), E + np.arange(E)], 1)
    for warm in (False, True):
        conn = eng.voxelize_edges_loaded_indexed(states, edges, wrench=fx["wrench"], dist=fx["dist"], frame="world", warm_start=warm, validate=True)
        assert np.array_equal(conn["fully_valid"], fx["valid_loaded"].astype(bool))
        assert (np.diff(conn["offsets"]) > 0).tolist() == fx["valid_loaded"].astype(bool).tolist()
    assert np.array_equal(eng.voxelize_edges_indexed(states, edges, validate=True)["fully_valid"], fx["valid_unloaded"].astype(bool))


@pytest.mark.parametrize("validate", [False, True])
def test_a_small_pool_changes_no_bit(world, validate):
    w = world("config3_rot")
    # the edge list taken twice over the same vertices: the pool of 512 overflows with it (tests/test_gpu_loaded_edges.py, test 5)
    edges = np.vstack([w.edges, w.edges])
    kw = dict(frame="world", warm_start=True, validate=validate, **LOADS)
    want = w.eng().voxelize_edges_loaded_indexed(w.states, edges, **kw)
    small = w.eng(TENDON_HIP_EDGE_POOL=str(POOL))
    got = small.voxelize_edges_loaded_indexed(w.states, edges, **kw)
    assert small.edges_loaded_last()["chunks"] >= 2
    assert _same_lists(got, want)
    for k in ("fully_valid", "n_fk"):
        assert np.array_equal(got[k], want[k]), k
    assert got["n_unconverged"] == want["n_unconverged"] and got["n_integrations"] == want["n_integrations"]
    E = len(w.edges)
    for e in range(E):
        x, y = _item(want, e), _item(want, E + e)
        assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1])


# ---- 6 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(FIXTURES))
def test_one_shape_per_vertex_across_the_phases(world, name):
    w = world(name)
    eng = w.eng()
    ph = w.phase(False)
    states, idx = ph["out"]["states"], ph["out"]["index"]
    edges = eng.knn_edges(states, 4)
    eng.voxelize_edges_loaded_indexed(states, edges, frame=w.frame, warm_start=True, validate=True, **LOADS)
    after_connect = eng.edges_loaded_vertex_strains(len(states))
    assert np.array_equal(after_connect, ph["out"]["vu0"])
    assert np.array_equal(after_connect, ph["fk"]["vu0"][idx])
    assert np.array_equal(eng.voxelize_batch_loaded(states, frame=w.frame, **LOADS)["tips"], ph["out"]["tips"])
    with pytest.raises(w.irt.InvalidArgument):
        eng.edges_loaded_vertex_strains(len(states))                   # the vertex pass of voxelize_batch_loaded has taken the rows


# ---- 7 ------------------------------------------------------------------------------------------------------------------------
def _host(c):
    if type(c["block_ids"]).__module__.startswith("torch"):
        return dict(c, block_ids=c["block_ids"].cpu().numpy().view(np.uint32), masks=c["masks"].cpu().numpy().view(np.uint64))
    return c


def _same_roadmap(x, y):
    for k in ("states", "tips", "edges"):
        assert np.array_equal(x[k], y[k]), k
    for k in ("vertex_caches", "edge_caches"):
        assert _same_lists(_host(x[k]), _host(y[k])), k


def test_builder_follows_set_loads(world, irt, orc):
    D = irt.distributed
    w = world("config3_rot")
    chk = w.irt.VoxelBackboneValidityChecker(w.robot, w.irt.VoxelEnvironment(), w.vox)
    eng = chk.engine
    mv = irt.VoxelBackboneMotionValidator(chk)
    builder = irt.RoadmapBuilder(chk, mv, seed=0)
    never = irt.VoxelBackboneValidityChecker(w.robot, w.irt.VoxelEnvironment(), w.vox)
    plain = irt.RoadmapBuilder(never, irt.VoxelBackboneMotionValidator(never), seed=0).create_roadmap(64, k=4, device=False)[1]
    loads = dict(frame="world", warm_start=True, **LOADS)
    chk.set_loads(WRENCH, DIST, frame="world", warm_start=True)
    # the composition of the calls
    sv = eng.sample_valid_vertices_loaded(64, seed=0, box=D.sampling_box(w.robot, None), **loads)
    cand = eng.knn_edges(sv["states"], 5)
    res = dict(min_tension_change=mv.min_tension_change, min_rotation_change=mv.min_rotation_change, min_retraction_change=mv.min_retraction_change)
    conn = eng.voxelize_edges_loaded_indexed(sv["states"], cand, validate=True, **loads, **res)
    kept = cand[conn["fully_valid"]]
    ec = eng.voxelize_edges_loaded_indexed(sv["states"], kept, **loads, **res)
    vc = eng.voxelize_batch_loaded(sv["states"], **loads)
    assert 0 < len(kept) < len(cand)
    assert ec["fully_valid"].all()
    rng = np.random.default_rng(5)
    starts, goals = rng.integers(0, 64, 40), rng.integers(0, 64, 40)
    for device in (False, True):
        prm, road = builder.create_roadmap(64, k=4, device=device)
        assert np.array_equal(road["states"], sv["states"]) and np.array_equal(road["tips"], sv["tips"])
        assert np.array_equal(road["edges"], kept)
        assert builder.timing["create_roadmap"]["candidate_edges"] == len(cand)
        assert _same_lists(_host(road["vertex_caches"]), vc) and _same_lists(_host(road["edge_caches"]), ec)
        assert np.array_equal(road["vertex_caches"]["shape_valid"], vc["shape_valid"])
        assert np.array_equal(builder.validate_edges(road["states"], cand)[0], conn["fully_valid"])
        # the other builder calls follow too
        assert _same_lists(_host(builder.edge_caches(road["states"], kept, device=device)), ec)
        got = prm.solveWithRoadmap(starts, goals)
        orm = orc.Roadmap(w.orb, road["states"], road["edges"], None, vc, _host(road["edge_caches"]))
        code = {-2: 2, -3: 3, 0: 1}
        for q in range(len(starts)):
            r = orm.query(w.og, starts[q], goals[q])
            assert got["status"][q] == (0 if r["n"] > 0 else code[r["n"]]), q
            if r["n"] > 0:
                assert np.array_equal(got["paths"][q], r["path"]) and got["cost"][q] == r["cost"], q
        assert (got["status"] == 0).sum() >= 5
        for call in (lambda: prm.roadmap_ik_batch(road["tips"][:2]), lambda: prm.solve_to_tips([0, 1], road["tips"][:2]),
                     lambda: irt.chained_plan(prm, [0], road["tips"][None, :2]),
                     lambda: builder.build_on_device(64, 5), lambda: builder.validate_edges_sharded(road["states"], cand)):
            with pytest.raises(irt.Unsupported):
                call()
    assert not np.array_equal(plain["states"], sv["states"])                          # the load moved the roadmap
    chk.clear_loads()
    _same_roadmap(builder.create_roadmap(64, k=4, device=False)[1], plain)
    prm, road = builder.create_roadmap(64, k=4, device=True)
    _same_roadmap(road, plain)
    assert len(prm.roadmap_ik_batch(road["tips"][:2])["outcome"]) == 2                   # tip queries answer again


# ---- 8 ------------------------------------------------------------------------------------------------------------------------
def test_errors(world, irt):
    import ctypes as C
    w = world("config1")
    eng = w.eng()
    ret = irt.workloads.robot_config1()
    ret.enable_retraction = True
    reng = irt.Engine(ret, 0)
    with pytest.raises(irt.Unsupported) as e0:
        reng.fk_loaded_batch(np.zeros((2, 4)))                             # shoot_check's wording
    calls = (lambda e, st: e.sample_valid_vertices_loaded(4, **LOADS),
             lambda e, st: e.voxelize_batch_loaded(st, **LOADS),
             lambda e, st: e.voxelize_edges_loaded_indexed(st, [[0, 1]], **LOADS),
             lambda e, st: e.voxelize_edges_loaded_indexed(st, [[0, 1]], validate=True, **LOADS))
    for call in calls:
        with pytest.raises(irt.Unsupported) as e1:
            call(reng, np.zeros((2, 4)))
        assert str(e1.value) == str(e0.value)
    bare = irt.Engine(w.robot, 0)
    for call in calls:
        with pytest.raises(irt.InvalidArgument):
            call(bare, w.states)                                           # no grid
    for kw in (dict(frame="tool"), dict(max_iters=-1)):
        with pytest.raises(irt.InvalidArgument):
            eng.sample_valid_vertices_loaded(4, **kw)
        with pytest.raises(irt.InvalidArgument):
            eng.voxelize_batch_loaded(w.states, **kw)
        for validate in (False, True):
            with pytest.raises(irt.InvalidArgument):
                eng.voxelize_edges_loaded_indexed(w.states, w.edges, validate=validate, **kw)
    with pytest.raises(irt.InvalidArgument):
        eng.voxelize_edges_loaded_indexed(w.states, w.edges, min_tension_change=0.0)
    with pytest.raises(irt.OutOfRange):
        eng.voxelize_edges_loaded_indexed(w.states, [[0, len(w.states)]])
    # empty calls are fine, also before a grid is set
    for e in (eng, bare):
        out = e.sample_valid_vertices_loaded(0, **LOADS)
        assert out["accepted"] == 0 and out["tried"] == 0 and out["states"].shape == (0, 3) and out["n_integrations"] == 0
        out = e.voxelize_batch_loaded(np.zeros((0, 3)), **LOADS)
        assert out["offsets"].tolist() == [0] and out["block_ids"].size == 0
        for validate in (False, True):
            out = e.voxelize_edges_loaded_indexed(w.states, np.zeros((0, 2), dtype=np.int32), validate=validate, **LOADS)
            assert out["offsets"].tolist() == [0] and len(out["fully_valid"]) == 0
    # the C ABI: a frame that is neither; null shoot and null loads = the defaults and no load
    ld = irt._lib.TrEdgeLoads()
    ld.frame = 2
    n = C.c_int64(0)
    st = np.empty((4, 3))
    dp = st.ctypes.data_as(C.POINTER(C.c_double))
    assert eng.lib.tr_sample_valid_vertices_loaded(eng._ctx, None, C.byref(ld), 0, 0, None, None, 4, 64, dp, None, None, None, C.byref(n), None,
                                                   None, None) == irt._lib.TR_ERR_INVALID_ARG
    assert eng.lib.tr_sample_valid_vertices_loaded(eng._ctx, None, None, 0, 0, None, None, 4, 64, dp, None, None, None, C.byref(n), None, None,
                                                   None) == irt._lib.TR_OK
    assert n.value == 4 and np.array_equal(st, eng.sample_valid_vertices(4, seed=0, max_candidates=64)["states"])
    bare.close(); reng.close()


def test_device_outputs_of_the_vertex_phase(world, irt):
    """tr_sample_valid_vertices_loaded_dev: the same rows in the caller's tensors."""
    import ctypes as C
    import torch
    w = world("config3_rot")
    eng = w.eng()
    want = w.phase(False)["out"]
    nw, S = n_want("config3_rot"), eng.state_size
    dev = "cuda:%d" % eng.device
    d_states = torch.zeros(nw * S, dtype=torch.float64, device=dev)
    d_tips = torch.zeros(nw * 3, dtype=torch.float64, device=dev)
    d_index = torch.zeros(nw, dtype=torch.int64, device=dev)
    d_vu = torch.zeros(nw * 6, dtype=torch.float64, device=dev)
    ld = eng._edge_loads(WRENCH, DIST, "world", False)
    acc, tried, nu, ni = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
    vp = lambda t: C.c_void_p(t.data_ptr())
    for with_index in (True, False):
        irt._lib.check(eng._ctx, eng.lib.tr_sample_valid_vertices_loaded_dev(
            eng._ctx, None, C.byref(ld), 0, 0, None, None, nw, MAX_CAND, vp(d_states), vp(d_tips), vp(d_index) if with_index else None, vp(d_vu),
            C.byref(acc), C.byref(tried), C.byref(nu), C.byref(ni), eng._stream_ptr(None)))
        torch.cuda.synchronize()
        k = acc.value
        assert k == want["accepted"] and tried.value == want["tried"] and ni.value == want["n_integrations"]
        assert np.array_equal(d_states.cpu().numpy().reshape(nw, S)[:k], want["states"])
        assert np.array_equal(d_tips.cpu().numpy().reshape(nw, 3)[:k], want["tips"])
        assert np.array_equal(d_index.cpu().numpy()[:k], want["index"])
        assert np.array_equal(d_vu.cpu().numpy().reshape(nw, 6)[:k], want["vu0"])
        d_vu.zero_()
