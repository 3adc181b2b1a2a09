"""Writes tests/golden/loaded_ret_edges_config3_ret_edges.npz: edges of config3_ret_edges (a robot WITH retraction, dL = L / 40) whose
verdict under load is decided without the library's FK (tests/test_gpu_loaded_ret_edges.py, test 4).

Twelve edges: eight whose start state pulls one tendon, or two neighbours, with 10 N (tips in eight directions round the axis, far
enough apart for one sphere each) and four that pull one tendon with 5 N, the other tensions seeded in [0.2, 1] N; |d tau| = 0.5 N;
s_start from 0 .. 1.5 dL at the start state to 2.5 dL more at the end state (the ends differ by two or three backbone points), under the loads of tests/loaded_ret_edges_common.py -- the gravity of a 50 g
robot plus the tip force; the robot does not rotate, so WORLD and BASE loads are the same rows.  Shapes: tests/loaded_ret_reference.py
(numpy Newton shooting on the state's own grid, |e| <= 1e-11 N).  A 64^3 grid over +-0.22 m (6.9 mm voxels, the finest the backbone
checker takes for this dL); one sphere per edge, alternately of BIG voxels radius on the LOADED tip of the edge's start state (stops
the loaded robot, the unloaded one passes under it) and of SMALL voxels radius on its UNLOADED tip (the reverse: gravity moves a
full-length backbone's tip by ~5 voxels); every edge is then judged against all spheres:
  valid under load    only if the Python bisection (tests/loaded_edges_reference.py, level order) on numpy shapes finds every sample
                      shape-valid -- 1e-4 m inside the length limits against home_shape(s_start) -- and no collision against the
                      spheres GROWN by 2 voxels;
  invalid under load  only if an end state's numpy backbone hits a sphere SHRUNK by 2 voxels (a sphere that small is left out);
an edge that is neither is dropped (make_loaded_edges.py gives the reason for the two voxels).  The unloaded verdicts are the
oracle's check_motion on the spheres as they are.  The generator fails unless at least 3 kept edges are valid loaded and invalid
unloaded, and at least 3 the reverse.

  python tests/golden/make_loaded_ret_edges.py          (a second run writes the same bytes)
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

import loaded_edges_reference as ler                                  # noqa: E402
import loaded_ret_edges_common as rec                                 # noqa: E402
import loaded_ret_reference as ref                                    # noqa: E402
import make_fk_truth as mft                                          # noqa: E402

NAME = "config3_ret_edges"
GRID_N, HALF, BIG, SMALL, MARGIN_VOXELS, N_EDGES, LENGTH_MARGIN, PULL = 64, 0.22, 3.0, 1.0, 2, 12, 1e-4, 10.0
VOXEL = 2 * HALF / GRID_N
PATH = os.path.join(HERE, "loaded_ret_edges_%s.npz" % NAME)


def candidate_edges(robot):
    N, dL = len(robot.tendons), robot.specs.dL
    rng = np.random.default_rng(31)
    a = np.zeros((N_EDGES, N + 1))
    a[:, :N] = rng.uniform(0.2, 1.0, (N_EDGES, N))
    for k in range(N_EDGES):                                          # eight directions at PULL N, then four single tendons at half of it
        j = (k // 2) % N if k < 2 * N else k % N
        a[k, j] = PULL if k < 2 * N else PULL / 2
        if k < 2 * N and k % 2:
            a[k, (j + 1) % N] = PULL
    a[:, N] = np.arange(N_EDGES) % 4 * dL / 2
    d = rng.normal(size=(N_EDGES, N))
    b = a.copy()
    b[:, :N] = a[:, :N] + 0.5 * d / np.linalg.norm(d, axis=1, keepdims=True)
    b[:, N] = a[:, N] + 2.5 * dL
    return a, b


class MarginJudge(ler.OracleJudge):
    """shape validity with LENGTH_MARGIN to spare at the length limits (the numpy L_i is not the device's to the last bit)"""

    def shape_valid(self, smp):
        if not super().shape_valid(smp):
            return False
        change = self.home(smp["s_start"]) - smp["L_i"]
        lo = np.array(self.orb.c.min_length[:self.orb.n_tendons])
        hi = np.array(self.orb.c.max_length[:self.orb.n_tendons])
        if not ((change >= lo + LENGTH_MARGIN) & (change <= hi - LENGTH_MARGIN)).all():
            raise RuntimeError("a sample is within %g m of a length limit: choose other tensions" % LENGTH_MARGIN)
        return True


def numpy_level(rob, dist):
    """the level evaluator of check_motion_levels on numpy shapes: every sample's own points, its s_start"""
    def level(states, sa):
        states = np.atleast_2d(states)
        out = ref.shoot(rob, states, F_e=rec.WRENCH[:3], L_e=rec.WRENCH[3:], f_e=dist[:3], l_e=dist[3:])
        res = []
        for i in range(len(states)):
            p = out["p"][i, :int(out["n_points"][i])].copy()
            res.append(dict(p=p, pts=p, converged=bool(out["converged"][i]), L_i=out["L_i"][i], s_start=float(states[i, -1])))
        return res
    return level


def grids(orc, spheres):
    """the obstacle grids with the spheres as they are, grown and shrunk by the margin"""
    out = []
    for grow in (0, MARGIN_VOXELS, -MARGIN_VOXELS):
        g = orc.Grid(GRID_N, (-HALF, HALF) * 3)
        for s in spheres:
            if s[3] + grow * VOXEL > 0:
                g.add_sphere(s[:3], s[3] + grow * VOXEL)
        out.append(g)
    return out


def verdicts(robot, a, b, spheres):
    """(decided, loaded, unloaded) per edge against `spheres`: decided = the numpy shapes settle the loaded verdict with the margin"""
    from oracle import oracle as orc
    rob = mft.oracle_robot(robot)
    a, b = np.atleast_2d(a), np.atleast_2d(b)
    E = len(a)
    as_is, grown, shrunk = grids(orc, spheres)
    level = numpy_level(rob, rec.dist_of(robot))
    unloaded = np.array([orc.check_motion(rob, as_is, a[k], b[k])["valid"] for k in range(E)])
    lv = ler.check_motion_levels(ler.Space.of_robot(robot), MarginJudge(rob, grown), a, b, level)
    if lv["n_domain_errors"]:
        raise RuntimeError("a sample left the grid")
    ends = lv["samples"][:2 * E]
    hit = MarginJudge(rob, shrunk)
    decided, loaded = np.zeros(E, bool), np.zeros(E, bool)
    for k in range(E):
        sa, sb = ends[2 * k], ends[2 * k + 1]
        if lv["valid"][k]:
            decided[k] = loaded[k] = True
        elif hit.shape_valid(sa) and hit.shape_valid(sb) and (hit.backbone_hits(sa) or hit.backbone_hits(sb)):
            decided[k] = True
    return decided, loaded, unloaded, lv


def build():
    irt = mft._irt()
    robot = rec.robot(irt, NAME)
    rob = mft.oracle_robot(robot)
    a, b = candidate_edges(robot)
    ends = numpy_level(rob, rec.dist_of(robot))(a, None)
    spheres = []
    for k in range(N_EDGES):
        if k % 2 == 0:
            spheres.append(list(ends[k]["p"][-1]) + [BIG * VOXEL])
        else:
            spheres.append(list(rob.shape(a[k])["p"][-1]) + [SMALL * VOXEL])
    spheres = np.array(spheres)
    decided, loaded, un, lv = verdicts(robot, a, b, spheres)
    keep = np.flatnonzero(decided)
    loaded, un = loaded[keep], un[keep]
    print("%d of %d edges kept: %d valid loaded and invalid unloaded, %d the reverse, %d valid both, %d invalid both; %d numpy samples, levels %s"
          % (len(keep), N_EDGES, (loaded & ~un).sum(), (~loaded & un).sum(), (loaded & un).sum(), (~loaded & ~un).sum(), len(lv["samples"]), lv["levels"]))
    if (loaded & ~un).sum() < 3 or (~loaded & un).sum() < 3:
        raise RuntimeError("fewer than 3 edges that the load makes valid, or fewer than 3 that it makes invalid")
    return dict(a=a[keep], b=b[keep], spheres=spheres, grid=np.array([GRID_N, HALF]), wrench=rec.WRENCH, dist=rec.dist_of(robot),
                valid_loaded=loaded.astype(np.uint8), valid_unloaded=un.astype(np.uint8))


if __name__ == "__main__":
    mft.save_npz(PATH, build())
    print("%s: %d bytes" % (PATH, os.path.getsize(PATH)))
