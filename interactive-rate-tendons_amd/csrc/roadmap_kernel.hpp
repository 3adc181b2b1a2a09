// roadmap_kernel.hpp -- the device code of the roadmap unit apart from the graph search itself (search_kernel.hpp): landmark
// distances, component labels, the single-source sweep.  With the two types the host parts share with it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "search_kernel.hpp"

namespace {

enum : uint8_t { V_UNKNOWN = 0, V_VALID = 1, V_INVALID = 2 };   // VALIDITY_UNKNOWN / VALIDITY_TRUE / removed from the graph

struct Arc { int32_t v, e; double w; };   // one adjacency entry: neighbour, edge id, edge weight (16 B: four per cache line)

// The same distances on the device: every sweep relaxes all arcs for all landmarks at once -- thread (u, l) offers dist[u][l] + w(u, v)
// to every neighbour v (atomicMin on the bit patterns of the non-negative doubles) -- until a sweep changes nothing.  With
// non-negative weights and a monotone rounded addition this fixed point is Dijkstra's result bit for bit: both are the minimum over
// all paths of the left-to-right rounded sums of their weights.  A 100 k-vertex 10-NN roadmap converges in a few dozen sweeps of
// ~30 us; 16 Dijkstras on 16 host threads take 40 - 80 ms.
__global__ __launch_bounds__(256) void landmark_relax(const int64_t *__restrict__ adj_off, const Arc *__restrict__ adj, int64_t V, int L,
                                                      unsigned long long *__restrict__ dist, uint32_t *__restrict__ changed) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= V * L) return;
  const int64_t u = t / L;
  const int l = (int)(t - u * L);
  const double du = __longlong_as_double((long long)dist[u * L + l]);
  if (!(du < 1e300)) return;                                   // not reached yet
  bool any = false;
  for (int64_t k = adj_off[u]; k < adj_off[u + 1]; k++) {
    const Arc a = adj[k];
    const double cand = du + a.w;
    const unsigned long long cb = (unsigned long long)__double_as_longlong(cand);
    unsigned long long *p = &dist[(int64_t)a.v * L + l];
    if (cb < *p) { if (atomicMin(p, cb) > cb) any = true; }
  }
  if (any) *changed = 1u;
}
__global__ __launch_bounds__(256) void landmark_to_float(const unsigned long long *__restrict__ dist, int64_t n, float *__restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t < n) out[t] = (float)__longlong_as_double((long long)dist[t]);
}

__global__ __launch_bounds__(256) void landmark_init(unsigned long long *__restrict__ dist, int64_t n, const int32_t *__restrict__ lm_v, int L) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= n) return;
  const int64_t u = t / L;
  const int l = (int)(t - u * L);
  dist[t] = (lm_v[l] == (int32_t)u) ? 0ull : 0x7FF0000000000000ull;          // 0 at the landmark itself, +inf elsewhere
}

// ---- connected components of the roadmap minus the items known invalid ----
// The reference gives up on a query whose start and goal lie in different components before it searches (solutionComponent /
// sameComponent, VoxelCachedLazyPRM.cpp:2015-2044; LazyPRM renumbers the components when it removes items).  Without that a search
// for an unreachable goal walks the start's whole component before it reports "no path": 10^5 expansions, 37 ms on a core, 250 ms at
// a wave's pace.  Here the labels are recomputed per round on the device: union-find over the edge list with atomic hooks of the
// larger root under the smaller, then one pass that points every vertex at its root.  ~0.1 ms of kernels + the validity bytes up and the labels down.
// (Plain loads and stores except for the hooks: another XCD's L2 may show an older parent, which is an ancestor all the same; a
// vertex passed on the way is pointed at its grandparent -- path halving.  Only the compare-and-swap that turns a root into a
// child has to see the truth, and it does: it is an agent-scope atomic, and its return value is where a failed attempt goes on.)
__device__ __forceinline__ int32_t cc_root(int32_t *parent, int32_t x) {
  int32_t p = parent[x];
  for (int guard = 0; p != x && guard < (1 << 24); guard++) {
    const int32_t gp = parent[p];
    if (gp != p) parent[x] = gp;
    x = p; p = gp;
  }
  return x;
}
__global__ __launch_bounds__(256) void cc_init(int32_t *__restrict__ parent, int64_t V) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v < V) parent[v] = (int32_t)v;
}
// first pass: every vertex under its smallest smaller neighbour (one atomicMin per edge on mostly distinct words) -- a forest of
// short trees whose roots are the local minima, so that the hooks below contend for many words instead of one
__global__ __launch_bounds__(256) void cc_seed(const int32_t *__restrict__ eu, const int32_t *__restrict__ ev, const uint8_t *__restrict__ estat,
                                               const uint8_t *__restrict__ vstat, int64_t E, int32_t *parent) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= E || estat[e] == V_INVALID) return;
  const int32_t a = eu[e], b = ev[e];
  if (a == b || vstat[a] == V_INVALID || vstat[b] == V_INVALID) return;
  atomicMin(&parent[a > b ? a : b], a > b ? b : a);
}
__global__ __launch_bounds__(256) void cc_hook(const int32_t *__restrict__ eu, const int32_t *__restrict__ ev, const uint8_t *__restrict__ estat,
                                               const uint8_t *__restrict__ vstat, int64_t E, int32_t *parent) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= E || estat[e] == V_INVALID) return;
  const int32_t a = eu[e], b = ev[e];
  if (vstat[a] == V_INVALID || vstat[b] == V_INVALID) return;
  int32_t ra = cc_root(parent, a), rb = cc_root(parent, b);
  for (int guard = 0; ra != rb && guard < (1 << 24); guard++) {
    if (ra < rb) { const int32_t t = ra; ra = rb; rb = t; }                 // the larger root goes under the smaller
    const int32_t old = atomicCAS(&parent[ra], ra, rb);
    if (old == ra) break;                                                   // hooked
    ra = cc_root(parent, old);                                              // someone else hooked it first: follow and try again
    rb = cc_root(parent, rb);
  }
}
// (reads only: a halving store of one thread here could replace the root another thread has just written for the same vertex by a
// mere ancestor -- seen as connected pairs with different labels)
__global__ __launch_bounds__(256) void cc_flatten(const int32_t *__restrict__ parent, int32_t *__restrict__ label, int64_t V) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= V) return;
  int32_t x = (int32_t)v, p = parent[x];
  for (int guard = 0; p != x && guard < (1 << 24); guard++) { x = p; p = parent[x]; }
  label[v] = x;
}

// ---- a search as a parallel sweep ----
// A query whose path detours far round new obstacles makes A* expand a large part of the graph (on a 6 x 10^5-vertex roadmap: two of
// 10 000 queries with 3 - 4 x 10^5 expansions each, 200 ms on a core, ten times that on a wave -- they WERE the round).  Such a search
// is answered by relaxing every reached vertex's valid arcs at once, sweep after sweep (the scheme of landmark_relax: atomicMin on the
// bit patterns of the non-negative distances), until a sweep changes nothing; vertices at or beyond the goal's distance are not
// relaxed (weights are non-negative: nothing through them improves the goal).  The fixed point is Dijkstra's -- and A*'s -- cost bit for
// bit: the minimum over all paths of the left-to-right rounded sums of their weights.  The path is walked back on the host from the
// goal along arcs with dist[u] + w == dist[v] exactly (the first such arc of a row: A* keeps the first parent that reaches the
// final cost, so the two can differ only where two routes tie to the last bit).
__global__ __launch_bounds__(256) void sweep_relax(const trk::SArc *__restrict__ rows, int D, const uint8_t *__restrict__ vstat,
                                                   const uint8_t *__restrict__ estat, int64_t V, int32_t goal,
                                                   unsigned long long *__restrict__ dist, uint32_t *__restrict__ changed) {
  const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (u >= V) return;
  const unsigned long long bu = dist[u], bg = dist[goal];
  if (!(bu < bg)) return;                                      // not reached yet (+inf), or no closer than the goal is already
  const double du = __longlong_as_double((long long)bu);
  bool any = false;
  int64_t row = u;
  for (int guard = 0; guard < 4096; guard++) {                 // (a vertex's rows: 16 arcs each, chained through the last slot)
    int64_t next = -1;
    for (int j = 0; j < D; j++) {
      const trk::SArc a = rows[row * D + j];
      if (a.v == trk::SR_ARC_NONE) continue;
      if (a.v == trk::SR_ARC_MORE) { next = a.e; break; }
      const int32_t v = a.v & (int32_t)((1u << trk::SR_VBITS) - 1u);
      if (estat[a.e] == V_INVALID || vstat[v] == V_INVALID) continue;
      const unsigned long long cb = (unsigned long long)__double_as_longlong(du + a.w);
      if (cb < dist[v]) { if (atomicMin(&dist[v], cb) > cb) any = true; }
    }
    if (next < 0) break;
    row = next;
  }
  if (any) *changed = 1u;
}
__global__ __launch_bounds__(256) void sweep_init(unsigned long long *__restrict__ dist, int64_t V, int32_t start) {
  const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (u < V) dist[u] = u == start ? 0ull : 0x7FF0000000000000ull;
}

}  // namespace
