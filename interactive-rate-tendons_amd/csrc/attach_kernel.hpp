// attach_kernel.hpp -- the device glue of the attach phase (tr_roadmap_attach_states / tr_roadmap_solve_states; host side in
// roadmap_attach_host.inc): from the neighbour table of a batch of off-roadmap states to the index pairs tr_validate_edges_indexed_dev
// takes, and from its verdict words back to one byte per slot -- the pairs never leave HBM.
//   attach_mark         per slot of the n x k neighbour table: rows of invalid states become -1 / +inf; the state's validity byte; live byte; the slot's index
//                       pair over the array [roadmap rows | query rows]: (V + i, vertex) when the motion LEAVES state i, (vertex, V + i)
//                       when it ARRIVES there
//   attach_mark_direct  (tr_roadmap_solve_states) the pair (start_q, goal_q) where the direct-edge rule applies, and its distance
//   attach_count / attach_scan / attach_fill   the live slots compacted IN SLOT ORDER: live slots per block of 256 (ballot + popcount
//                       per wave), an exclusive scan of the block counts by one block, then every live slot's position = block offset +
//                       waves before it + lanes before it; no atomics, so the order is the same run after run
//   attach_scatter      verdict bit (and sample count) of every live slot's pair back to its slot; dead slots get 0
// Waves are 64 wide; every __ballot is reached by all lanes of the wave (the bounds test is folded into the predicate, never a branch
// around the cross-lane operation).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace trk {

constexpr int ATTACH_BLOCK = 256;                           // slots per block: four waves

__global__ __launch_bounds__(256) void attach_mark(const uint64_t *__restrict__ valid_bits, int64_t rows, int64_t n_out, int k, int64_t V,
                                                   int32_t *__restrict__ idx, double *__restrict__ dist, uint8_t *__restrict__ valid,
                                                   uint8_t *__restrict__ live, int32_t *__restrict__ pair_all) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= rows * k) return;
  const int64_t i = s / k;
  const bool ok = (valid_bits[i >> 6] >> (i & 63)) & 1;
  if (s == i * k) valid[i] = ok ? 1 : 0;                    // the state's bit as a byte, by the row's first slot
  int32_t v = idx[s];
  if (!ok) { v = -1; idx[s] = -1; dist[s] = __builtin_inf(); }
  live[s] = v >= 0 ? 1 : 0;
  const int32_t me = (int32_t)(V + i);
  pair_all[2 * s] = i < n_out ? me : v;
  pair_all[2 * s + 1] = i < n_out ? v : me;
}

// CompoundStateSpace::distance in stateq_distance's arithmetic for a state layout known at run time
__device__ __forceinline__ double attach_distance(const double *x, const double *c, int NT, bool rot, bool ret, double w_rot, double w_ret) {
#pragma clang fp contract(off)
  double s2 = 0.0;
  for (int d = 0; d < NT; d++) { const double t = x[d] - c[d]; s2 += t * t; }
  double dist = sqrt(s2);
  int R = NT;
  if (rot) {
    double a_ = fabs(x[NT] - c[NT]);
    a_ = (a_ > 3.14159265358979323846) ? 2.0 * 3.14159265358979323846 - a_ : a_;
    dist += w_rot * a_;
    R++;
  }
  if (ret) { const double t = x[R] - c[R]; dist += w_ret * sqrt(t * t); }
  return dist;
}

// query rows [0, n) are the starts, [n, 2 n) the goals; qry = the 2 n rows, dist their neighbour distances (2 n x k, rows of invalid
// states already +inf).  The direct edge of query q is tried when both states are valid and d(start, goal) <= max(dist_s[k-1],
// dist_g[k-1]) and <= max_dist.  live / pair_all: the n slots behind the 2 n k attach slots.
__global__ __launch_bounds__(256) void attach_mark_direct(const uint64_t *__restrict__ valid_bits, int64_t n, int k, int64_t V, int S, int NT,
                                                          int rot, int ret, double w_rot, double w_ret, double max_dist,
                                                          const double *__restrict__ qry, const double *__restrict__ dist,
                                                          uint8_t *__restrict__ live, int32_t *__restrict__ pair_all,
                                                          double *__restrict__ direct_dist) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= n) return;
  const int64_t g = n + q;
  const bool ok = ((valid_bits[q >> 6] >> (q & 63)) & 1) && ((valid_bits[g >> 6] >> (g & 63)) & 1);
  const double d = attach_distance(qry + q * S, qry + g * S, NT, rot != 0, ret != 0, w_rot, w_ret);
  const double ds = dist[q * k + (k - 1)], dg = dist[g * k + (k - 1)];
  const double reach = ds > dg ? ds : dg;
  direct_dist[q] = d;
  live[q] = (ok && d <= reach && d <= max_dist) ? 1 : 0;
  pair_all[2 * q] = (int32_t)(V + q);
  pair_all[2 * q + 1] = (int32_t)(V + g);
}

// live slots of block b -> block_count[b]
__global__ __launch_bounds__(256) void attach_count(const uint8_t *__restrict__ live, int64_t m, uint32_t *__restrict__ block_count) {
  __shared__ uint32_t wave_n[ATTACH_BLOCK / 64];
  const int64_t s = (int64_t)blockIdx.x * ATTACH_BLOCK + threadIdx.x;
  const bool p = s < m && live[s < m ? s : 0] != 0;
  const unsigned long long mk = __ballot(p);
  if ((threadIdx.x & 63) == 0) wave_n[threadIdx.x >> 6] = (uint32_t)__popcll(mk);
  __syncthreads();
  if (threadIdx.x == 0) block_count[blockIdx.x] = wave_n[0] + wave_n[1] + wave_n[2] + wave_n[3];
}

// one block: block_off[b] = live slots before block b, block_off[nb] = all of them (fewer than 2^31: n k <= 2^28)
__global__ __launch_bounds__(256) void attach_scan(const uint32_t *__restrict__ block_count, int64_t nb, uint32_t *__restrict__ block_off) {
  __shared__ uint32_t part[ATTACH_BLOCK];
  const int64_t per = (nb + ATTACH_BLOCK - 1) / ATTACH_BLOCK;
  const int64_t b0 = (int64_t)threadIdx.x * per, b1 = b0 + per < nb ? b0 + per : nb;
  uint32_t sum = 0;
  for (int64_t b = b0; b < b1; b++) sum += block_count[b];
  part[threadIdx.x] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t run = 0;
    for (int t = 0; t < ATTACH_BLOCK; t++) { const uint32_t c = part[t]; part[t] = run; run += c; }
    block_off[nb] = run;
  }
  __syncthreads();
  uint32_t run = part[threadIdx.x];
  for (int64_t b = b0; b < b1; b++) { block_off[b] = run; run += block_count[b]; }
}

// pairs[position of slot s] = pair_all[s] for the live slots; slot_pos[s] = that position, -1 for a dead slot
__global__ __launch_bounds__(256) void attach_fill(const uint8_t *__restrict__ live, int64_t m, const uint32_t *__restrict__ block_off,
                                                   const int32_t *__restrict__ pair_all, int32_t *__restrict__ pairs,
                                                   int32_t *__restrict__ slot_pos) {
  __shared__ uint32_t wave_n[ATTACH_BLOCK / 64];
  const int64_t s = (int64_t)blockIdx.x * ATTACH_BLOCK + threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool p = s < m && live[s < m ? s : 0] != 0;
  const unsigned long long mk = __ballot(p);
  if (lane == 0) wave_n[wave] = (uint32_t)__popcll(mk);
  __syncthreads();
  uint32_t pos = block_off[blockIdx.x];
  for (int w = 0; w < wave; w++) pos += wave_n[w];
  pos += (uint32_t)__popcll(mk & (((unsigned long long)1 << lane) - 1));
  if (s >= m) return;
  slot_pos[s] = p ? (int32_t)pos : -1;
  if (p) { pairs[2 * (int64_t)pos] = pair_all[2 * s]; pairs[2 * (int64_t)pos + 1] = pair_all[2 * s + 1]; }
}

__global__ __launch_bounds__(256) void attach_scatter(const int32_t *__restrict__ slot_pos, int64_t m, const uint64_t *__restrict__ pair_bits,
                                                      const int32_t *__restrict__ pair_nfk, uint8_t *__restrict__ ok, int32_t *__restrict__ nfk) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= m) return;
  const int32_t pos = slot_pos[s];
  ok[s] = pos >= 0 ? (uint8_t)((pair_bits[pos >> 6] >> (pos & 63)) & 1) : 0;
  if (nfk) nfk[s] = pos >= 0 ? pair_nfk[pos] : 0;
}

}  // namespace trk
