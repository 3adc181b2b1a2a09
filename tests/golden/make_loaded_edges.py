"""Writes tests/golden/loaded_edges_config3_rot.npz: edges of config3_rot whose verdict under load is decided without the library's FK,
and the rows of the seeded edge sets on which zero load costs no iteration (tests/test_gpu_loaded_edges.py, tests 3 and 2).

Test 3.  Twelve edges around the circle (theta_a = -pi + (k + 1/2) pi / 6, d theta = 0.1, seeded tensions in [2, 8] N, |d tau| = 0.5 N)
under the loads of loaded_edges_common, fixed in the world frame: every sample's rows are turned by Rz(-theta) with numpy's own sine
and cosine.  Shapes: tests/loaded_fk_reference.py (numpy Newton shooting, |e| <= 1e-11 N).  One sphere of 4 voxels radius per edge on a
256^3 grid over +-0.3 m, alternately on the LOADED tip of the edge's start state (stops the loaded robot) and on its UNLOADED tip
(stops the unloaded one); every edge is then judged against all spheres:
  valid under load    only if the Python bisection (tests/loaded_edges_reference.py, level order) on numpy shapes finds every sample
                      shape-valid -- 1e-4 m inside the length limits -- and no collision against the spheres GROWN by 2 voxels;
  invalid under load  only if an end state's numpy backbone hits a sphere SHRUNK by 2 voxels;
an edge that is neither is dropped.  The device's solution of a sample may differ from numpy's by bound_i <= 1e-5 m
(tests/golden/make_loaded_fk.py) and its bisection may then sample other t, all on the same sweep, between numpy samples at most
a voxel apart: two voxels cover both.  The unloaded verdicts are the oracle's check_motion on the spheres as they are.  The generator
fails unless at least 3 kept edges are valid loaded and invalid unloaded, and at least 3 the reverse.

Test 2.  zero_rows_<name>: the edges of loaded_edges_common's seeded set of fixture <name> on which the unloaded solution of every
state interpolate(a, b, k / 64), k = 0 .. 64 -- every t the bisection can sample -- balances the tip of the numpy integration to
0.9 residual_threshold.  solve_initial_bending stops its own iteration AT that threshold, so a state whose iteration stops just under
it at the base can sit just over it at the tip (5.00 - 5.07e-6 N against 5e-6 on 9 of config3_rot's 32 edges; the rest stay below
4.5e-6): such a sample takes a Levenberg-Marquardt round at zero load, and the count of integrations of test 2 is asserted on the
rows where none does.

  python tests/golden/make_loaded_edges.py          (a second run writes the same bytes)
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

NAME = "config3_rot"
GRID_N, SPHERE_VOXELS, MARGIN_VOXELS, N_EDGES, LENGTH_MARGIN = 256, 4, 2, 12, 1e-4
PATH = os.path.join(HERE, "loaded_edges_%s.npz" % NAME)


def world_loads(states, N):
    """(n, 6) wrench and dist rows of loads fixed in the world frame: Rz(-theta) applied to all four vectors"""
    c, s = np.cos(states[:, N]), np.sin(states[:, N])
    out = []
    for v in (lec.WRENCH, lec.DIST):
        r = np.empty((len(states), 6))
        for h in (0, 3):
            r[:, h], r[:, h + 1], r[:, h + 2] = c * v[h] + s * v[h + 1], c * v[h + 1] - s * v[h], v[h + 2]
        out.append(r)
    return out


def candidate_edges(N):
    rng = np.random.default_rng(31)
    a = np.zeros((N_EDGES, N + 1))
    a[:, :N] = rng.uniform(2.0, 8.0, (N_EDGES, N))
    a[:, N] = -np.pi + (np.arange(N_EDGES) + 0.5) * np.pi / 6
    d = rng.normal(size=(N_EDGES, N))
    b = a.copy()
    b[:, :N] = a[:, :N] + 0.5 * d / np.linalg.norm(d, axis=1, keepdims=True)
    b[:, N] = a[:, N] + 0.1
    return a, b


class MarginJudge(ler.OracleJudge):
    """shape validity with LENGTH_MARGIN to spare at the length limits (the numpy L_i is not the device's to the last bit)"""

    def shape_valid(self, smp):
        if not super().shape_valid(smp):
            return False
        change = self.home() - smp["L_i"]
        lo = np.array(self.orb.c.min_length[:self.orb.n_tendons])
        hi = np.array(self.orb.c.max_length[:self.orb.n_tendons])
        if not ((change >= lo + LENGTH_MARGIN) & (change <= hi - LENGTH_MARGIN)).all():
            raise RuntimeError("a sample is within %g m of a length limit: choose other tensions" % LENGTH_MARGIN)
        return True


def zero_rows(irt, name):
    robot = mft.fixture_robot(irt, name)[0]
    rob = mft.oracle_robot(robot)
    n, eseed, cap = lec.FIXTURES[name][:3]
    a, b = lec.make_edges(robot, n, eseed, cap)
    N = len(robot.tendons)
    space = ler.Space.of_robot(robot)
    st = np.array([[space.interpolate(a[i], b[i], k / 64) for k in range(65)] for i in range(n)]).reshape(n * 65, -1)
    e = np.linalg.norm(ref.evaluate(rob, st, ref.unloaded_start(rob, st[:, :N]))["e"], axis=1).reshape(n, 65).max(axis=1)
    rows = np.flatnonzero(e <= 0.9 * robot.residual_threshold).astype(np.int32)
    print("%s: zero load costs no iteration on %d of %d edges (start residual of the others: %s N)" % (name, len(rows), n, np.round(np.sort(e[e > 0.9 * robot.residual_threshold]), 8)))
    if len(rows) < n // 2:
        raise RuntimeError("fewer than half of the edges of %s" % name)
    return rows


def build():
    from oracle import oracle as orc
    irt = mft._irt()
    robot = mft.fixture_robot(irt, NAME)[0]
    rob = mft.oracle_robot(robot)
    N = len(robot.tendons)
    lim = (-lec.HALF, lec.HALF) * 3
    vox = 2 * lec.HALF / GRID_N
    a, b = candidate_edges(N)
    space = ler.Space.of_robot(robot)

    def numpy_level(states, sa):
        w, d = world_loads(states, N)
        out = ref.shoot(rob, states, F_e=w[:, :3], L_e=w[:, 3:], f_e=d[:, :3], l_e=d[:, 3:])
        return [dict(p=out["p"][i], pts=out["p"][i], converged=bool(out["converged"][i]), L_i=out["L_i"][i]) for i in range(len(states))]

    ends = numpy_level(np.vstack([a, b]), None)
    spheres = []
    for k in range(N_EDGES):
        tip = ends[k]["p"][-1] if k % 2 == 0 else rob.shape(a[k])["p"][-1]
        spheres.append(list(tip) + [SPHERE_VOXELS * vox])
    spheres = np.array(spheres)
    grids = []
    for grow in (0, MARGIN_VOXELS, -MARGIN_VOXELS):
        g = orc.Grid(GRID_N, lim)
        for s in spheres:
            g.add_sphere(s[:3], s[3] + grow * vox)
        grids.append(g)
    as_is, grown, shrunk = grids
    unloaded = np.array([orc.check_motion(rob, as_is, a[k], b[k])["valid"] for k in range(N_EDGES)])
    lv = ler.check_motion_levels(space, MarginJudge(rob, grown), a, b, numpy_level)
    if lv["n_domain_errors"]:
        raise RuntimeError("a sample left the grid")
    hit_shrunk = MarginJudge(rob, shrunk)
    keep, loaded = [], []
    for k in range(N_EDGES):
        if lv["valid"][k]:
            keep.append(k); loaded.append(True)
        elif hit_shrunk.shape_valid(ends[k]) and hit_shrunk.shape_valid(ends[N_EDGES + k]) and \
                (hit_shrunk.backbone_hits(ends[k]) or hit_shrunk.backbone_hits(ends[N_EDGES + k])):
            keep.append(k); loaded.append(False)
    keep, loaded = np.array(keep), np.array(loaded)
    un = unloaded[keep]
    print("%d of %d edges kept: %d valid loaded and invalid unloaded, %d the reverse, %d valid both, %d invalid both; %d numpy samples, levels %s"
          % (len(keep), N_EDGES, (loaded & ~un).sum(), (~loaded & un).sum(), (loaded & un).sum(), (~loaded & ~un).sum(), len(lv["samples"]), lv["levels"]))
    if (loaded & ~un).sum() < 3 or (~loaded & un).sum() < 3:
        raise RuntimeError("fewer than 3 edges that the load makes valid, or fewer than 3 that it makes invalid")
    arrays = dict(a=a[keep], b=b[keep], spheres=spheres, grid=np.array([GRID_N, lec.HALF]), wrench=lec.WRENCH, dist=lec.DIST,
                  valid_loaded=loaded.astype(np.uint8), valid_unloaded=un.astype(np.uint8))
    for name in lec.FIXTURES:
        arrays["zero_rows_" + name] = zero_rows(irt, name)
    return arrays


if __name__ == "__main__":
    mft.save_npz(PATH, build())
    print("%s: %d bytes" % (PATH, os.path.getsize(PATH)))
