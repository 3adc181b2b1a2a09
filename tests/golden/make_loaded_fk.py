"""Writes tests/golden/loaded_fk_<name>.npz: loaded shapes of the fixture robots by the numpy reference (tests/loaded_fk_reference.py).

Robots and their 24 states are make_fk_truth's (fixture_robot / fixture_states).  Four load cases per fixture, loads in the robot's
base frame before the state's rotation:
  A  one wrench for all: F_e = (0.05, -0.03, 0.02) N, L_e = (1e-3, -2e-3, 5e-4) N m
  B  gravity per state: f_e = Rz(-theta) (0, -2.4525, 0) N/m (a 50 g robot of 0.2 m), no wrench
  C  B plus a seeded wrench per state, |F| <= 0.1 N, |L| <= 2e-3 N m
  D  C plus a seeded distributed load of its own per state: a force of any direction with 0.3 <= |f| <= 1.0 N/m added to the gravity
     row, and a distributed moment l_e of any direction with 0.003 <= |l| <= 0.01 N (a generator of its own, seeded by the robot's
     position in NAMES).  The only case with a moment per unit length and with a z component in f_e: all twelve numbers of a row are
     non-zero, and the lower limits keep every state's moment large enough to see (tests/test_loaded_fk_truth.py)
Per state and case: the loads, the reference's (v0, u0), points, tip frame, L, L_i, |e_ref|, and
  C_i     the largest 2-norm over the backbone points of dp/d(v0, u0) J^-1 in m/N (from the last Jacobian's integrations)
  bound_i 1e-9 m + 1.5 C_i (residual_threshold + |e_ref,i|): the first-order displacement of a solution whose wrench misses by the
          threshold (1.5 covers the second order; 1e-9 m is the project's interface tolerance)
The generator fails if any (state, case) does not converge.  config3_rot also gets the obstacles of the verdict test: for three
states two spheres, one on the loaded tip (case B) and one on the unloaded tip, each at least 2 voxels clear of the other shape's
backbone on a 256^3 grid over +-0.3 m (checked on the oracle grid).

  python tests/golden/make_loaded_fk.py [name ...]
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

import loaded_fk_reference as ref                                    # noqa: E402
import make_fk_truth as mft                                          # noqa: E402

NAMES = ("config1", "n1", "n8", "config3_rot", "n5", "n6")          # new names go last: case C is seeded by position
CASES = ("A", "B", "C", "D")
WRENCH_A = np.array([0.05, -0.03, 0.02, 1e-3, -2e-3, 5e-4])
GRAVITY = np.array([0.0, -2.4525, 0.0])
GRID_N, GRID_HALF, SPHERE_VOXELS, CLEAR_VOXELS = 256, 0.3, 3, 2


def path(name):
    return os.path.join(HERE, "loaded_fk_%s.npz" % name)


def fixture(name):
    """(robot, oracle robot, states (24, S))"""
    irt = mft._irt()
    robot, st = mft.fixture_states(irt, name)
    return robot, mft.oracle_robot(robot), st


def loads(name, robot, st, case):
    """(wrench (n, 6), dist (n, 6)) of a case"""
    n, N = st.shape[0], len(robot.tendons)
    theta = st[:, N] if robot.enable_rotation else np.zeros(n)
    wrench, dist = np.zeros((n, 6)), np.zeros((n, 6))
    if case == "A":
        wrench[:] = WRENCH_A
        return wrench, dist
    c, s = np.cos(-theta), np.sin(-theta)
    dist[:, 0] = c * GRAVITY[0] - s * GRAVITY[1]
    dist[:, 1] = s * GRAVITY[0] + c * GRAVITY[1]
    if case in ("C", "D"):
        rng = np.random.default_rng(9000 + NAMES.index(name))
        for col, cap in ((0, 0.1), (3, 2e-3)):
            d = rng.normal(size=(n, 3))
            wrench[:, col:col + 3] = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.0, cap, (n, 1))
    if case == "D":
        rng = np.random.default_rng(9500 + NAMES.index(name))
        for col, lo, hi in ((0, 0.3, 1.0), (3, 0.003, 0.01)):
            d = rng.normal(size=(n, 3))
            dist[:, col:col + 3] += d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(lo, hi, (n, 1))
    return wrench, dist


def solve_case(name, robot, rob, st, case, rows=None):
    """The arrays of one case for states `rows` (default: all)."""
    wrench, dist = loads(name, robot, st, case)
    if rows is not None:
        st, wrench, dist = st[rows], wrench[rows], dist[rows]
    out = ref.shoot(rob, st, F_e=wrench[:, :3], L_e=wrench[:, 3:], f_e=dist[:, :3], l_e=dist[:, 3:])
    if not out["converged"].all():
        raise RuntimeError("%s case %s: states %s did not converge (|e| = %s)"
                           % (name, case, np.nonzero(~out["converged"])[0], out["e"][~out["converged"]]))
    bound = 1e-9 + 1.5 * out["C"] * (robot.residual_threshold + out["e"])
    return dict(wrench=wrench, dist=dist, vu0=out["vu0"], p=out["p"], R_tip=out["R"][:, -1], L=out["L"], L_i=out["L_i"],
                e_ref=out["e"], C=out["C"], bound=bound, iters=out["iters"])


def dist_to_polyline(c, pts):
    a, b = pts[:-1], pts[1:]
    ab = b - a
    t = np.clip(((c - a) * ab).sum(1) / np.maximum((ab * ab).sum(1), 1e-300), 0.0, 1.0)
    return np.linalg.norm(a + t[:, None] * ab - c, axis=1).min()


def verdict_obstacles(robot, rob, st, loaded_p, loaded_Li):
    """Three states whose loaded (case B) and unloaded shapes are told apart by a sphere on either tip."""
    from oracle import oracle as orc
    lim = (-GRID_HALF, GRID_HALF) * 3
    vox = 2 * GRID_HALF / GRID_N
    radius = SPHERE_VOXELS * vox
    home = rob.home_shape()["L_i"]
    idx, sph_l, sph_u = [], [], []
    for i in range(st.shape[0]):
        un = rob.shape(st[i])
        pu, pl = un["p"], loaded_p[i]
        empty = orc.Grid(GRID_N, lim)
        if not orc.is_valid_state(rob, empty, st[i]):
            continue
        if rob.collides_self(pl) or not rob.is_within_length_limits(home, loaded_Li[i]):
            continue
        ok = True
        for own, other in ((pl, pu), (pu, pl)):
            if dist_to_polyline(own[-1], other) < radius + (CLEAR_VOXELS + 2) * vox:
                ok = False
                break
            g = orc.Grid(GRID_N, lim)
            g.add_sphere(own[-1], radius)
            line_own, line_other = g.empty_copy(), g.empty_copy()
            line_own.add_piecewise_line(own)
            line_other.add_piecewise_line(other)
            hit_own = g.collides(line_own)
            g.dilate(CLEAR_VOXELS, True)
            if not hit_own or g.collides(line_other):
                ok = False
                break
        if not ok:
            continue
        idx.append(i)
        sph_l.append(list(pl[-1]) + [radius])
        sph_u.append(list(pu[-1]) + [radius])
        if len(idx) == 3:
            break
    if len(idx) < 3:
        raise RuntimeError("fewer than three states separate the loaded and the unloaded shape")
    return dict(verdict_states=np.array(idx, dtype=np.int32), verdict_sphere_loaded=np.array(sph_l), verdict_sphere_unloaded=np.array(sph_u),
                verdict_grid=np.array([GRID_N, GRID_HALF]))


def build(name):
    robot, rob, st = fixture(name)
    arrays = dict(states=st, residual_threshold=np.array(robot.residual_threshold), dL=np.array(robot.specs.dL))
    for case in CASES:
        for k, v in solve_case(name, robot, rob, st, case).items():
            arrays["%s_%s" % (k, case)] = v
    if name == "config3_rot":
        arrays.update(verdict_obstacles(robot, rob, st, arrays["p_B"], arrays["L_i_B"]))
    return arrays


def main(names):
    for name in names or NAMES:
        arrays = build(name)
        mft.save_npz(path(name), arrays)
        print("%s: %d bytes; Newton steps <= %d; C <= %.3g m/N; bound <= %.3g m" % (
            name, os.path.getsize(path(name)), max(int(arrays["iters_%s" % c].max()) for c in CASES),
            max(float(arrays["C_%s" % c].max()) for c in CASES), max(float(arrays["bound_%s" % c].max()) for c in CASES)))


if __name__ == "__main__":
    main(sys.argv[1:])
