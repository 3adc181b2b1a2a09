"""Writes tests/golden/loaded_roadmap_config3_rot.npz: the first candidates of the roadmap's vertex phase on config3_rot whose verdict
under load is decided without the library's FK (tests/test_gpu_loaded_roadmap.py, test 2; tests/test_loaded_roadmap_golden.py).

The first 128 candidates of seed 0 in the planner's default box (distributed.candidate_states, the host mirror of the device's
generator), under the loads of loaded_edges_common fixed in the WORLD frame: every candidate's rows are turned by Rz(-theta) with
numpy's own sine and cosine.  Shapes: tests/loaded_fk_reference.py (numpy Newton shooting, |e| <= 1e-11 N).  Grid: the seeded
spheres of loaded_edges_common's config3_rot fixture (make_grid's loop, restated here to keep the centres; the restatement is
checked against make_grid's blocks).
  valid_loaded    the numpy shape is valid (converged, inside the length limits, no self-collision) and its backbone misses the
                  spheres as they are
  decided         the shape is valid -- 1e-4 m inside the length limits -- and the backbone either misses the spheres GROWN by 2
                  voxels or hits them SHRUNK by 2 voxels
  valid_unloaded  the oracle's is_valid_state on the spheres as they are
The device's solution of a candidate may differ from numpy's by bound_i = 1e-9 m + 1.5 C_i (residual_threshold + |e_i|)
(tests/golden/make_loaded_fk.py); the generator fails unless every decided candidate's bound is below a tenth of the 2 voxels, at
least 100 candidates are decided and at least 10 of those differ from the unloaded verdict.

  python tests/golden/make_loaded_roadmap.py          (a second run writes the same bytes)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
for _p in (ROOT, TESTS, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import loaded_edges_common as lec                                    # noqa: E402
import loaded_edges_reference as ler                                  # noqa: E402
import loaded_fk_reference as ref                                    # noqa: E402
import make_fk_truth as mft                                          # noqa: E402
from make_loaded_edges import world_loads                            # noqa: E402

NAME = "config3_rot"
N_CAND, MARGIN_VOXELS, LENGTH_MARGIN, MIN_DECIDED, MIN_MOVED = 128, 2, 1e-4, 100, 10
PATH = os.path.join(HERE, "loaded_roadmap_%s.npz" % NAME)


def seeded_spheres(seed, count, radius):
    """(count, 4) centres and radius of loaded_edges_common.make_grid's spheres"""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < count:
        c = rng.uniform(-0.2, 0.2, 3)
        zc = min(max(c[2], 0.0), 0.2)
        if np.linalg.norm(c) > 0.21 or c[2] < -0.02 or np.sqrt(c[0] ** 2 + c[1] ** 2 + (c[2] - zc) ** 2) < 0.03 + radius:
            continue
        out.append(list(c) + [radius])
    return np.array(out)


def numpy_shapes(rob, states):
    N = rob.n_tendons
    w, d = world_loads(states, N)
    return ref.shoot(rob, states, F_e=w[:, :3], L_e=w[:, 3:], f_e=d[:, :3], l_e=d[:, 3:])


def judge_rows(rob, grids, out, rows, residual_threshold):
    """dict of (len(rows),) arrays for the candidates `rows` of a shooting result: shape, inside (the length limits with
    LENGTH_MARGIN to spare), hit / hit_grown / hit_shrunk, bound"""
    as_is, grown, shrunk = (ler.OracleJudge(rob, g) for g in grids)
    lo = np.array(rob.c.min_length[:rob.n_tendons])
    hi = np.array(rob.c.max_length[:rob.n_tendons])
    r = dict(shape=[], inside=[], hit=[], hit_grown=[], hit_shrunk=[])
    for i in rows:
        smp = dict(p=out["p"][i], pts=out["p"][i], converged=bool(out["converged"][i]), L_i=out["L_i"][i])
        ok = as_is.shape_valid(smp)
        change = as_is.home() - smp["L_i"]
        r["shape"].append(ok)
        r["inside"].append(bool(ok and ((change >= lo + LENGTH_MARGIN) & (change <= hi - LENGTH_MARGIN)).all()))
        for key, j in (("hit", as_is), ("hit_grown", grown), ("hit_shrunk", shrunk)):
            r[key].append(bool(ok and j.backbone_hits(smp)))
    r = {k: np.array(v, dtype=bool) for k, v in r.items()}
    r["bound"] = 1e-9 + 1.5 * out["C"][rows] * (residual_threshold + out["e"][rows])
    return r


def build(rows=None):
    """The file's arrays; rows: only these candidates (tests/test_loaded_roadmap_golden.py reproduces a few), no counts checked."""
    from oracle import oracle as orc
    irt = mft._irt()
    robot = mft.fixture_robot(irt, NAME)[0]
    rob = mft.oracle_robot(robot)
    _, _, _, gseed, count, radius = lec.FIXTURES[NAME]
    grid_n = lec.grid_dim(robot.specs.dL)
    lim = (-lec.HALF, lec.HALF) * 3
    vox = 2 * lec.HALF / grid_n
    spheres = seeded_spheres(gseed, count, radius)
    grids = []
    for grow in (0, MARGIN_VOXELS, -MARGIN_VOXELS):
        g = orc.Grid(grid_n, lim)
        for s in spheres:
            g.add_sphere(s[:3], s[3] + grow * vox)
        grids.append(g)
    if not np.array_equal(grids[0].blocks(), lec.make_grid(irt, robot.specs.dL, gseed, count, radius).blocks):
        raise RuntimeError("the restated spheres are not make_grid's")
    states = irt.distributed.candidate_states(robot, 0, 0, N_CAND)
    sel = np.arange(N_CAND) if rows is None else np.asarray(rows)
    out = numpy_shapes(rob, states[sel])
    j = judge_rows(rob, grids, out, np.arange(len(sel)), robot.residual_threshold)
    valid = j["shape"] & ~j["hit"]
    decided = j["inside"] & (~j["hit_grown"] | j["hit_shrunk"])
    unloaded = np.array([orc.is_valid_state(rob, grids[0], s)[0] for s in states[sel]], dtype=bool)
    if rows is None:
        moved = int((valid[decided] != unloaded[decided]).sum())
        print("%d of %d candidates decided (%d valid, %d invalid), %d of them differ from the unloaded verdict; bound <= %.3g m against %.3g m"
              % (decided.sum(), N_CAND, (valid & decided).sum(), (~valid & decided).sum(), moved, j["bound"][decided].max(), MARGIN_VOXELS * vox))
        if decided.sum() < MIN_DECIDED or moved < MIN_MOVED:
            raise RuntimeError("fewer than %d decided candidates, or fewer than %d that the load moves" % (MIN_DECIDED, MIN_MOVED))
        if not (j["bound"][decided] <= 0.1 * MARGIN_VOXELS * vox).all():
            raise RuntimeError("a decided candidate's displacement bound is not small against the margin")
    return dict(states=states[sel], spheres=spheres, grid=np.array([grid_n, lec.HALF]), wrench=lec.WRENCH, dist=lec.DIST,
                valid_loaded=valid.astype(np.uint8), decided=decided.astype(np.uint8), valid_unloaded=unloaded.astype(np.uint8),
                bound=j["bound"])


if __name__ == "__main__":
    mft.save_npz(PATH, build())
    print("%s: %d bytes" % (PATH, os.path.getsize(PATH)))
