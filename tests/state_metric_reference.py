"""The state-space metric of the neighbour searches (knn_kernel.hpp, stateq_kernel.hpp) restated in numpy, the (distance, index)
order built on it, and robots and inputs for every state layout (1 .. 8 tendons, rotation on / off, retraction on / off).

The restatement does what the kernels' headers say, operation for operation, so that a table compared with it needs no tolerance:
the tension differences squared and summed left to right (one product and one sum per column), the root, then + w_rot * arc (the
shortest arc: |d theta|, or 2 pi - |d theta| where |d theta| > pi), then + w_ret * sqrt(d s * d s).  numpy only; checked on the
CPU by tests/test_state_metric_reference.py."""
import numpy as np

K_TABLE = 11                # the k of the whole-table comparisons
CLUSTER = 70                # identical states in the cluster: more than any k the searches take (<= 65)
LATTICE_FRACTION = 0.5      # lattice step = this fraction of each tendon's cap: 3 values per column, 3^8 sites at 8 tendons


def distances(n_tendons, rot, ret, w_rot, w_ret, q, rows):
    """distance(q, rows) over the last axis (the state), the leading axes broadcast: one state (S,) against rows (n, S) -> (n,);
    rows against rows (n, S), (n, S) -> (n,); a block q[:, None, :] (m, 1, S) against rows (n, S) -> (m, n)"""
    q = np.asarray(q, dtype=np.float64)
    rows = np.asarray(rows, dtype=np.float64)
    s2 = np.zeros(np.broadcast_shapes(q.shape[:-1], rows.shape[:-1]))
    for d in range(n_tendons):                                          # left to right, one product and one sum per column
        t = q[..., d] - rows[..., d]
        s2 = s2 + t * t
    dist = np.sqrt(s2)
    c = n_tendons
    if rot:
        arc = np.abs(q[..., c] - rows[..., c])
        arc = np.where(arc > np.pi, 2.0 * np.pi - arc, arc)
        dist = dist + w_rot * arc
        c += 1
    if ret:
        t = q[..., c] - rows[..., c]
        dist = dist + w_ret * np.sqrt(t * t)
    return dist


def nearest(n_tendons, rot, ret, w_rot, w_ret, states, ok, queries, k, max_distance=np.inf, whole_row_sort=False):
    """Per query the first k of the candidates `ok` marks (None: all of `states`) in the order (distance, index): (n, k) int32
    indices padded with -1 and (n, k) distances padded with +inf; an entry farther than max_distance is dropped, one AT it stays.
    The candidates at or below the k-th smallest distance are found by np.partition and only those are stable-sorted;
    whole_row_sort = True stable-sorts the whole row instead (the same result: test_state_metric_reference.py)."""
    states = np.asarray(states, dtype=np.float64)
    queries = np.asarray(queries, dtype=np.float64).reshape(-1, states.shape[1])
    cand = np.arange(len(states)) if ok is None else np.flatnonzero(ok)
    rows = np.ascontiguousarray(states[cand])
    idx = np.full((len(queries), k), -1, dtype=np.int32)
    dist = np.full((len(queries), k), np.inf)
    kk = min(k, len(cand))
    if kk == 0:
        return idx, dist
    for lo in range(0, len(queries), 128):
        D = distances(n_tendons, rot, ret, w_rot, w_ret, queries[lo:lo + 128, None, :], rows)
        kth = None if whole_row_sort else np.partition(D, kk - 1, axis=1)[:, kk - 1]
        for i, d in enumerate(D):
            if whole_row_sort:
                order = np.argsort(d, kind="stable")[:kk]
            else:
                keep = np.flatnonzero(d <= kth[i])                      # (ascending indices: a stable sort by distance is the order (distance, index))
                order = keep[np.argsort(d[keep], kind="stable")][:kk]
            order = order[d[order] <= max_distance]
            idx[lo + i, :len(order)] = cand[order]
            dist[lo + i, :len(order)] = d[order]
    return idx, dist


def same(got, want):
    """indices equal, distances equal as bits"""
    return np.array_equal(got[0], want[0]) and np.array_equal(np.ascontiguousarray(got[1]).view(np.uint64),
                                                              np.ascontiguousarray(want[1]).view(np.uint64))


def exact_bound(dist, column=5):
    """(m, row): a distance bound that is one exact entry of an unbounded table -- the median of `column` over the rows that
    have it -- and a row that holds it there"""
    col = dist[:, column]
    rows = np.flatnonzero(np.isfinite(col))
    row = int(rows[np.argsort(col[rows], kind="stable")[len(rows) // 2]])
    return float(col[row]), row


LAYOUTS = [(nt, rot, ret) for nt in range(1, 9) for rot in (False, True) for ret in (False, True)]


def layout_id(layout):
    return "nt%d%s%s" % (layout[0], "-rot" if layout[1] else "", "-ret" if layout[2] else "")


def layout_robot(irt, n_tendons, rot, ret):
    """n_tendons straight tendons spread round the backbone with UNEQUAL tension caps 8, 11, 14, ... N (the extent of the tension
    space, hence both weights of the metric, is sqrt(sum cap_i^2)); dL = L / 128, which a 256^3 checker accepts"""
    tendons = [irt.TendonSpecs(C=[2.0 * np.pi * i / n_tendons], D=[0.01], max_tension=8.0 + 3.0 * i) for i in range(n_tendons)]
    return irt.TendonRobot(tendons=tendons, specs=irt.BackboneSpecs(dL=0.2 / 128), enable_rotation=bool(rot), enable_retraction=bool(ret))


def layout_rows(n):
    """Where layout_states puts what, whatever the seed: index arrays `lattice` (every third row, outside the cluster), `cluster`
    (identical states), `tension_min` / `tension_max` (first tension 0 / its cap: the first and the last cell of the search's grid),
    `s_zero` / `s_full` (retraction exactly 0 / L), `theta_minus_pi` / `theta_zero` (rotation exactly -pi / 0)."""
    size = min(CLUSTER, n // 4)
    first = n // 2
    cluster = np.arange(first, first + size)
    lattice = np.setdiff1d(np.arange(0, n, 3), cluster)
    pick = lambda *r: np.array([i for i in r if i < n and not first <= i < first + size], dtype=np.int64)
    return dict(lattice=lattice, cluster=cluster, tension_min=pick(1, 2, n - 2), tension_max=pick(4, 5, n - 1),
                s_zero=pick(7, 8, n - 4), s_full=pick(10, 11, n - 5), theta_minus_pi=pick(13, 14), theta_zero=pick(16, 17))


def layout_states(robot, n, seed):
    """n states of the robot's space with what the neighbour searches can get wrong in them (layout_rows says where):
      * uniform states, the bulk;
      * every third row on a lattice of step LATTICE_FRACTION x cap per tendon, its rotation exactly -pi or 0, its retraction exactly
        0, L / 2 or L: coincident states and states at exactly equal distances, at 8 tendons too;
      * a cluster of min(CLUSTER, n / 4) identical states;
      * with rotation: half of the other rotations within 1e-3 of +pi or -pi, inside the interval, so that the shortest arc between
        two of them is tiny where the plain difference is almost 2 pi; a few exactly -pi and exactly 0 (|d theta| = pi exactly: the
        side of the branch that keeps the plain difference);
      * with retraction: a few rows at s = 0 and at s = L exactly;
      * a few rows whose first tension is 0 or its cap, the ends of the column's range."""
    rng = np.random.default_rng(seed)
    caps = np.array([t.max_tension for t in robot.tendons])
    nt = len(caps)
    rot, ret, L = robot.enable_rotation, robot.enable_retraction, robot.specs.L
    S = nt + int(rot) + int(ret)
    where = layout_rows(n)
    lat = where["lattice"]
    st = np.empty((n, S))
    st[:, :nt] = rng.uniform(0.0, 1.0, (n, nt)) * caps
    step = LATTICE_FRACTION * caps
    st[lat, :nt] = np.round(st[lat, :nt] / step) * step
    st[where["tension_min"], 0] = 0.0
    st[where["tension_max"], 0] = caps[0]
    c = nt
    if rot:
        th = rng.uniform(-np.pi, np.pi, n)
        near = rng.random(n) < 0.5
        side = np.where(rng.random(n) < 0.5, 1.0, -1.0)
        th = np.where(near, side * (np.pi - rng.uniform(0.0, 1e-3, n)), th)
        th[lat] = np.where(np.abs(th[lat]) > 0.5 * np.pi, -np.pi, 0.0)
        th[where["theta_minus_pi"]] = -np.pi
        th[where["theta_zero"]] = 0.0
        st[:, c] = th
        c += 1
    if ret:
        s = rng.uniform(0.0, L, n)
        s[lat] = np.round(s[lat] / (0.5 * L)) * (0.5 * L)
        s[where["s_zero"]] = 0.0
        s[where["s_full"]] = L
        st[:, c] = s
    if len(where["cluster"]):
        st[where["cluster"]] = st[where["cluster"][0]]                    # (a uniform state: the lattice leaves the cluster's rows out)
    return np.ascontiguousarray(st)


def sample_rows(n, count=256):
    """A fixed sample of `count` rows of a layout_states set: the whole cluster, every row layout_rows names for a boundary value,
    and rows spread evenly over the rest (a third of them lattice rows)."""
    where = layout_rows(n)
    base = np.unique(np.concatenate([where[key] for key in where if key != "lattice"]))
    rest = np.setdiff1d(np.arange(n), base)
    more = rest[np.linspace(0, len(rest) - 1, max(0, min(count, n) - len(base))).astype(np.int64)]
    return np.union1d(base, more)


# ---- the inputs of tests/test_gpu_neighbour_layouts.py (their adequacy is asserted on the CPU, tests/test_state_metric_reference.py) ----
N_KNN = 4101                # tr_knn: >= 4096 (the lane-per-query form then builds more than one cell), no multiple of 64, 8 or 4
V_ROADMAP = 2051            # tr_roadmap_nearest_states: 32 tiles of 64 vertices and a last one of 3
N_QUERIES = 2049            # one slice of the vertex array whatever Q, and a last wave with a single query


def knn_inputs(robot):
    return layout_states(robot, N_KNN, seed=8100)


def roadmap_inputs(robot):
    """(vertex states, status: about 10 % invalid (2), query states): the queries are another layout_states set; every 37th equals
    a vertex (valid or not), and query 22 is the state of the vertices' cluster"""
    states = layout_states(robot, V_ROADMAP, seed=8200)
    rng = np.random.default_rng(8201)
    status = np.where(rng.random(V_ROADMAP) > 0.1, 1, 2).astype(np.uint8)
    queries = layout_states(robot, N_QUERIES, seed=8300)
    at = np.arange(20, N_QUERIES, 37)
    queries[at] = states[rng.integers(0, V_ROADMAP, len(at))]
    queries[22] = states[layout_rows(V_ROADMAP)["cluster"][0]]
    return states, status, np.ascontiguousarray(queries)
