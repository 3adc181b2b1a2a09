"""A restatement of the seeded search (rule S1 - S4 of include/tendon_hip.h, tr_roadmap_solve_seeded) in numpy / scipy, no GPU:
one scipy.sparse.csgraph.dijkstra per source-seed vertex on the roadmap minus its invalid items, then the brute-force minimum of
c_i + dist(u_i, v_j) + d_j over every pair of seeds, against the direct cost.  Its sums run in Dijkstra's order, not A*'s: costs
agree with the library's to rounding (a path of at most V edges: V 2^-53 relative), picks and statuses exactly unless two
combinations tie that closely.  Edge weights must be > 0 and the edge list free of duplicates (csgraph's sparse input)."""
import numpy as np
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import dijkstra

SOLVED, NO_PATH = 0, 1


def valid_graph(n_vertices, edges, weights, vertex_valid, edge_valid):
    """The undirected roadmap minus the invalid edges and the edges at invalid vertices, as a CSR matrix."""
    e = np.asarray(edges).reshape(-1, 2)
    w = np.asarray(weights, dtype=np.float64)
    vv, ev = np.asarray(vertex_valid, dtype=bool), np.asarray(edge_valid, dtype=bool)
    keep = ev & vv[e[:, 0]] & vv[e[:, 1]] if len(e) else np.zeros(0, dtype=bool)
    e, w = e[keep], w[keep]
    assert (w > 0).all(), "edge weights must be > 0"
    return csr_matrix((np.concatenate([w, w]), (np.concatenate([e[:, 0], e[:, 1]]), np.concatenate([e[:, 1], e[:, 0]]))),
                      shape=(n_vertices, n_vertices))


def solve_seeded(n_vertices, edges, weights, vertex_valid, edge_valid, src, dst, direct_cost=None):
    """src / dst: per query a pair (vertices, costs).  -> dict(status, cost, src_pick, dst_pick, direct): picks index the query's
    lists (-1: direct answer or no path); among equal sums the first (i, j) in lexicographic order; the direct connection wins
    when direct_cost <= the best sum."""
    n = len(src)
    vv = np.asarray(vertex_valid, dtype=bool)
    g = valid_graph(n_vertices, edges, weights, vv, edge_valid)
    roots = np.unique(np.concatenate([np.asarray(v, dtype=np.int64).reshape(-1) for v, _ in src] + [np.zeros(0, np.int64)]))
    roots = roots[vv[roots]] if len(roots) else roots
    dist = dijkstra(g, directed=False, indices=roots) if len(roots) else np.zeros((0, n_vertices))
    row = {int(u): k for k, u in enumerate(roots)}
    out = dict(status=np.full(n, NO_PATH, dtype=np.int32), cost=np.full(n, np.inf), src_pick=np.full(n, -1, dtype=np.int32),
               dst_pick=np.full(n, -1, dtype=np.int32), direct=np.zeros(n, dtype=bool))
    for q in range(n):
        (su, sc), (dv, dd) = src[q], dst[q]
        best, pick = np.inf, (-1, -1)
        for i, (u, c) in enumerate(zip(su, sc)):
            if not vv[u]:
                continue
            for j, (v, d) in enumerate(zip(dv, dd)):
                if not vv[v]:
                    continue
                total = (c + dist[row[int(u)], v]) + d
                if total < best:
                    best, pick = total, (i, j)
        dc = np.inf if direct_cost is None else direct_cost[q]
        if dc < np.inf and dc <= best:
            out["status"][q], out["cost"][q], out["direct"][q] = SOLVED, dc, True
        elif best < np.inf:
            out["status"][q], out["cost"][q] = SOLVED, best
            out["src_pick"][q], out["dst_pick"][q] = pick
    return out


def path_cost(weight_of, c, path, d):
    """((c + w_1) + w_2 ...) + d along a vertex path, left to right from the source: the sum rule S3 states.
    weight_of(u, v) -> the edge's weight."""
    total = np.float64(c)
    for a, b in zip(path[:-1], path[1:]):
        total = total + np.float64(weight_of(int(a), int(b)))
    return total + np.float64(d)
