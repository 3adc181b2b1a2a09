"""What tests/test_gpu_loaded_edges.py, tests/test_cpp_shim_loaded_edges.py and tests/golden/make_loaded_edges.py share: the loads, the
seeded edges of make_fk_truth's fixture robots and their sphere grids."""
import numpy as np

WRENCH = np.array([0.05, -0.03, 0.02, 0.0, 0.0, 0.0])
DIST = np.array([0.0, -2.4525, 0.0, 0.0, 0.0, 0.0])
# all twelve numbers non-zero: case A's wrench (make_loaded_fk.py) and a row of case D's size -- gravity plus a force of 0.76 N/m with a
# z component, and a distributed moment of 7.8e-3 N
WRENCH_FULL = np.array([0.05, -0.03, 0.02, 1e-3, -2e-3, 5e-4])
DIST_FULL = np.array([0.45, -2.1025, 0.5, 4e-3, -6e-3, 3e-3])
HALF = 0.3
#        edges, seed of the edges, tension cap of the start states, seed and count of the spheres, their radius
FIXTURES = {"config1": (32, 3, 12.0, 5, 40, 0.03), "config3_rot": (32, 3, 18.0, 7, 24, 0.02), "n8": (8, 4, 4.0, 9, 40, 0.03)}


def grid_dim(dL):
    return next(n for n in (256, 128, 64) if 2 * HALF / n >= dL)


def make_edges(robot, n, seed, cap):
    """n edges (a, b): 0.3 <= |d tau| <= 1 N, 0.2 <= |d theta| <= 0.3 (a tip that swings through a dozen voxels: deep levels)"""
    N = len(robot.tendons)
    rng = np.random.default_rng(seed)
    a = np.zeros((n, robot.state_size()))
    a[:, :N] = rng.uniform(0.0, cap, (n, N))
    d = rng.normal(size=(n, N))
    b = a.copy()
    b[:, :N] = np.clip(a[:, :N] + d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.3, 1.0, (n, 1)), 0.0, None)
    if robot.enable_rotation:
        a[:, N] = rng.uniform(-np.pi, np.pi, n)
        b[:, N] = a[:, N] + rng.choice([-1.0, 1.0], n) * rng.uniform(0.2, 0.3, n)
        wrap = b[:, N] > np.pi
        b[wrap, N] -= 2 * np.pi
        wrap = b[:, N] < -np.pi
        b[wrap, N] += 2 * np.pi
    assert (np.linalg.norm(b[:, :N] - a[:, :N], axis=1) <= 1.0).all()
    return np.ascontiguousarray(a), np.ascontiguousarray(b)


def make_grid(irt, dL, seed, count, radius):
    vox = irt.VoxelOctree(grid_dim(dL))
    vox.set_xlim(-HALF, HALF); vox.set_ylim(-HALF, HALF); vox.set_zlim(-HALF, HALF)
    rng = np.random.default_rng(seed)
    k = 0
    while k < count:
        c = rng.uniform(-0.2, 0.2, 3)
        zc = min(max(c[2], 0.0), 0.2)
        if np.linalg.norm(c) > 0.21 or c[2] < -0.02 or np.sqrt(c[0] ** 2 + c[1] ** 2 + (c[2] - zc) ** 2) < 0.03 + radius:
            continue
        vox.add_sphere(c, radius)
        k += 1
    return vox


