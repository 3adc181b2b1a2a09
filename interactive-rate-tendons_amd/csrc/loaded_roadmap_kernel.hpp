// loaded_roadmap_kernel.hpp -- the per-candidate helpers of the roadmap build on loaded shapes (loaded_roadmap_host.inc): createRoadmap's
// vertex phase with every candidate's shape taken from the loaded FK, as the reference's loop does once set_fk_func has put
// TendonRobot::general_shape in the checker's place of fk(state) (motion-planning/VoxelCachedLazyPRM.cpp:1415-1439).
//
//   loaded_tip_rows        the tips of a batch: each workspace column's tip row (no retraction: the last of the P point rows)
//   loaded_gather_strains  the strain rows of the candidates the compaction has just accepted, by their compacted candidate indices:
//                          the order-preserving compaction of vu_pool without a second scan
//   loaded_vertex_tally    unconverged candidates and integrations among the candidates the run has consumed (index < tried): a batch
//                          is solved whole, but what lies behind the candidate that completed the set does not count, so that the two
//                          sums do not depend on the batch size
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace trk {

// tips [m][3] from planes [P][ld], column i, row tip_row
__global__ __launch_bounds__(256) void loaded_tip_rows(const double *__restrict__ px, const double *__restrict__ py, const double *__restrict__ pz,
                                                       int64_t ld, int tip_row, int64_t m, double *__restrict__ tips) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  const int64_t at = (int64_t)tip_row * ld + i;
  tips[3 * i] = px[at]; tips[3 * i + 1] = py[at]; tips[3 * i + 2] = pz[at];
}

// out[pos] = vu[index[pos] - index_base] for the output positions pos in [had, *have) (at most `span` of them): *have is the
// compaction's counter after this batch, `had` what the host read after the batch before
__global__ __launch_bounds__(256) void loaded_gather_strains(const int64_t *__restrict__ index, const unsigned long long *__restrict__ have,
                                                             int64_t had, int64_t span, uint64_t index_base, int64_t m,
                                                             const double *__restrict__ vu, double *__restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= span * 6) return;
  const int64_t pos = had + t / 6, j = t % 6;
  if (pos >= (int64_t)*have) return;
  const int64_t i = index[pos] - (int64_t)index_base;
  if (i < 0 || i >= m) return;
  out[pos * 6 + j] = vu[i * 6 + j];
}

// tally[0] += candidates i < m with index_base + i < *tried that did not converge, tally[1] += the integrations of those candidates
__global__ __launch_bounds__(256) void loaded_vertex_tally(const uint8_t *__restrict__ conv, const int32_t *__restrict__ calls, int64_t m,
                                                           uint64_t index_base, const unsigned long long *__restrict__ tried,
                                                           unsigned long long *__restrict__ tally) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = i < m && index_base + (uint64_t)i < (uint64_t)*tried;
  const unsigned long long bad = __ballot(live && conv[i] == 0);
  long long n = live ? (long long)calls[i] : 0;
  for (int o = 32; o > 0; o >>= 1) n += __shfl_down(n, o);
  if ((threadIdx.x & 63) == 0) {
    if (bad) atomicAdd(&tally[0], (unsigned long long)__popcll(bad));
    if (n) atomicAdd(&tally[1], (unsigned long long)n);
  }
}

}  // namespace trk
