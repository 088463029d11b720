// What the kernels that work on a ligand's bond graph share (k_autos.hip, k_build.hip): the 256 x 256 adjacency bitset (MAX_LIG atoms, 8 words per row,
// 8 KB of LDS) and the ordered compaction of a workgroup: an exclusive scan in thread order, so that what survives is stored in a fixed order with no
// atomic cursor.
#pragma once
#include "model.h"

namespace ddk {

// {a, b} becomes an edge (a != b, both < MAX_LIG; the caller has checked them).  OR: the two directions of a bond and repeated columns are one edge, in
// any arrival order.  Returns whether the bit of the (a, b) direction was set before.
__device__ inline bool adj256_add(uint32_t (*adj)[8], int a, int b) {
  const uint32_t old = atomicOr(&adj[a][b >> 5], 1u << (b & 31));
  atomicOr(&adj[b][a >> 5], 1u << (a & 31));
  return (old >> (b & 31)) & 1u;
}

__device__ inline bool bits256_test(const uint32_t* set, int a) { return (set[a >> 5] >> (a & 31)) & 1u; }

// exclusive scan of one flag per thread over the workgroup in thread order (ballot per wave, the wave totals through LDS); *total: the workgroup's sum.
// Two barriers; wave_sums [blockDim / 64] is free again after the call.
__device__ inline int block_scan_flags(bool flag, int* wave_sums, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
  const unsigned long long b = __ballot(flag);
  const int in_wave = __popcll(b & ((1ull << lane) - 1ull));
  __syncthreads();      // (the previous call's readers are done with wave_sums)
  if (lane == 0) wave_sums[wave] = __popcll(b);
  __syncthreads();
  int before = 0, all = 0;
  for (int w = 0; w < n_waves; ++w) {
    const int s = wave_sums[w];
    all += s;
    if (w < wave) before += s;
  }
  *total = all;
  return before + in_wave;
}

// the same for one int per thread (shuffles inside the wave).  Integer sums: any order gives the same number.
__device__ inline int block_scan_int(int v, int* wave_sums, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
  int incl = v;
  for (int o = 1; o < 64; o <<= 1) {
    const int up = __shfl_up(incl, o, 64);
    if (lane >= o) incl += up;
  }
  __syncthreads();
  if (lane == 63) wave_sums[wave] = incl;
  __syncthreads();
  int before = 0, all = 0;
  for (int w = 0; w < n_waves; ++w) {
    const int s = wave_sums[w];
    all += s;
    if (w < wave) before += s;
  }
  *total = all;
  return before + incl - v;
}

}  // namespace ddk
