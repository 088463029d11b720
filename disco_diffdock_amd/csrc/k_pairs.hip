// Poses in -> distinct binding modes out (see include/ddk.h: ddk_pose_pairwise_rmsd, ddk_pose_cluster):
//   pose_pairs_kernel    the all-pairs symmetry-corrected RMSD matrix of B poses of one ligand in the receptor frame
//                        (the pair form of evaluate.py:308-313; pose j plays the part ref plays in pose_metrics_kernel, k_se3.hip)
//   pose_cluster_kernel  greedy leader clustering by score on such a matrix, one workgroup
// Neither reads anything of a complex, uses a float atomic or synchronises with the host: the matrix is bit-identical run to run.
#include <math.h>

#include "model.h"

namespace ddk {

// pose_pairs_kernel: workgroup (jt, i) owns pose i and the PAIRS_TJ poses j of tile jt; pose i, the j tile (one 16-B word per atom: one ds_read_b128 per
// position) and the mask sit in LDS.  The permutation table is the only large operand (n_perms * n_lig * 4 B): every row is loaded ONCE per workgroup, coalesced,
// and used against all PAIRS_TJ partners.  The PAIRS_WAVES waves stride over the rows, the 64 lanes over the atoms; per row a lane holds PAIRS_TJ partial
// sums of |pos_i[perms[k][a]] - pos_j[a]|^2 (differences first, then squares; fp32, at most MAX_LIG / 64 = 4 terms per lane and 6 levels of the tree below).
// The PAIRS_TJ sums are reduced across the wave by a transposing butterfly: the exchange over lane bit 5 halves the live values (the lower half-wave keeps
// partners 0-3, the upper 4-7), bit 4 halves them again, bit 3 leaves one, bits 2-0 finish it: 4 + 2 + 1 + 3 = 10 cross-lane moves instead of 6 * PAIRS_TJ, and
// lane l ends with the row's sum for partner (l >> 3).  A fixed tree: the same bits every run.  A row with a kept entry outside [0, n_lig) is +inf for every
// partner (its out-of-range entries read atom 0 and are discarded).  Each lane keeps the minimum over its wave's rows, the waves meet through LDS, and the
// square root is taken once per pair.  Tiles that lie wholly at or below i return at once: only i < j is computed, and stored twice.
static_assert(PAIRS_TJ == 8, "the butterfly of pose_pairs_kernel is written for 8 partners");

__global__ __launch_bounds__(PAIRS_WAVES * 64) void pose_pairs_kernel(const float* __restrict__ pos, const uint8_t* __restrict__ mask,
                                                                      const int32_t* __restrict__ perms, int n_perms, int B, int n_lig,
                                                                      float* __restrict__ out) {
  const int i = blockIdx.y, j0 = blockIdx.x * PAIRS_TJ;
  const int j_end = min(j0 + PAIRS_TJ, B);      // (uniform per workgroup)
  if (j_end - 1 < i) return;                    // no j > i and no diagonal entry in this tile
  __shared__ float4 pi[MAX_LIG];
  __shared__ float4 pj[PAIRS_TJ][MAX_LIG];
  __shared__ unsigned char keep[MAX_LIG];
  __shared__ float wave_min[PAIRS_WAVES][PAIRS_TJ];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int a = tid; a < n_lig; a += PAIRS_WAVES * 64) {
    const float* p = pos + ((size_t)i * n_lig + a) * 3;
    pi[a] = make_float4(p[0], p[1], p[2], 0.f);
    keep[a] = mask ? (mask[a] != 0) : 1;
  }
  for (int e = tid; e < PAIRS_TJ * n_lig; e += PAIRS_WAVES * 64) {
    const int t = e / n_lig, a = e - t * n_lig;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);      // (a partner past B: computed like the others, never stored)
    if (j0 + t < B) {
      const float* p = pos + ((size_t)(j0 + t) * n_lig + a) * 3;
      v = make_float4(p[0], p[1], p[2], 0.f);
    }
    pj[t][a] = v;
  }
  // m = the number of kept atoms (n_lig <= the workgroup size: one atom per thread); the barrier also publishes the LDS writes above
  const int m = __syncthreads_count(tid < n_lig && (mask ? mask[tid] != 0 : 1));

  const bool b5 = lane & 32, b4 = lane & 16, b3 = lane & 8;
  float best = INFINITY;
  const int K = perms ? n_perms : 1;
  // a lane's entries of a row (atoms lane, lane + 64, ...; the identity without a table).  The next row is fetched while the current one is worked on, and
  // PAIRS_WAVES = 16 puts four waves on a SIMD: at B = 40 a workgroup is alone on its CU and nothing else covers the load and the LDS round trips
  // (40 x 80 atoms x 1024 rows on an MI355X: 255 us with 4 waves, 108 us with 16; profiles/pairwise_rmsd_timing.md).
  int cur[MAX_LIG / 64], nxt[MAX_LIG / 64];
#pragma unroll
  for (int u = 0; u < MAX_LIG / 64; ++u) {
    const int a = lane + 64 * u;
    cur[u] = nxt[u] = a;
    if (perms && wave < K && a < n_lig) cur[u] = perms[(size_t)wave * n_lig + a];
  }
  for (int k = wave; k < K; k += PAIRS_WAVES) {
    if (perms && k + PAIRS_WAVES < K) {
#pragma unroll
      for (int u = 0; u < MAX_LIG / 64; ++u)
        if (lane + 64 * u < n_lig) nxt[u] = perms[(size_t)(k + PAIRS_WAVES) * n_lig + lane + 64 * u];
    }
    float acc[PAIRS_TJ];
#pragma unroll
    for (int t = 0; t < PAIRS_TJ; ++t) acc[t] = 0.f;
    bool bad = false;
#pragma unroll
    for (int u = 0; u < MAX_LIG / 64; ++u) {
      const int a = lane + 64 * u;
      if (a >= n_lig || !keep[a]) continue;
      int src = cur[u];
      if ((unsigned)src >= (unsigned)n_lig) { bad = true; src = 0; }
      const float4 q = pi[src];
#pragma unroll
      for (int t = 0; t < PAIRS_TJ; ++t) {
        const float4 r = pj[t][a];
        const float dx = q.x - r.x, dy = q.y - r.y, dz = q.z - r.z;
        acc[t] += dx * dx + dy * dy + dz * dz;
      }
    }
#pragma unroll
    for (int u = 0; u < MAX_LIG / 64; ++u) cur[u] = nxt[u];
    float r4[4], r2[2], s;
#pragma unroll
    for (int c = 0; c < 4; ++c) r4[c] = (b5 ? acc[c + 4] : acc[c]) + __shfl_xor(b5 ? acc[c] : acc[c + 4], 32, 64);
#pragma unroll
    for (int c = 0; c < 2; ++c) r2[c] = (b4 ? r4[c + 2] : r4[c]) + __shfl_xor(b4 ? r4[c] : r4[c + 2], 16, 64);
    s = (b3 ? r2[1] : r2[0]) + __shfl_xor(b3 ? r2[0] : r2[1], 8, 64);
    s += __shfl_xor(s, 4, 64);
    s += __shfl_xor(s, 2, 64);
    s += __shfl_xor(s, 1, 64);
    if (__any(bad)) s = INFINITY;      // this table row can never be the minimum (the pair is +inf if no row is valid)
    best = fminf(best, s);
  }
  if ((lane & 7) == 0) wave_min[wave][lane >> 3] = best;
  __syncthreads();
  if (tid < PAIRS_TJ) {
    const int j = j0 + tid;
    if (j < B && j >= i) {
      float v = 0.f;      // the diagonal, and every entry when no atom is kept
      if (j > i && m > 0) {
        float s = wave_min[0][tid];
#pragma unroll
        for (int w = 1; w < PAIRS_WAVES; ++w) s = fminf(s, wave_min[w][tid]);
        v = sqrtf(s / (float)m);
      }
      out[(size_t)i * B + j] = v;
      out[(size_t)j * B + i] = v;
    }
  }
}

hipError_t launch_pose_pairs(const float* pos, const uint8_t* mask, const int32_t* perms, int n_perms, int B, int n_lig, float* out, hipStream_t s) {
  hipLaunchKernelGGL(pose_pairs_kernel, dim3((B + PAIRS_TJ - 1) / PAIRS_TJ, B), dim3(PAIRS_WAVES * 64), 0, s, pos, mask, perms, n_perms, B, n_lig, out);
  return hipGetLastError();
}

// does sample a rank before sample b?  score descending, ties to the lower index, NaN after -inf (NaNs among themselves by index)
__device__ inline bool ranks_before(float sa, int a, float sb, int b) {
  const bool na = sa != sa, nb = sb != sb;
  if (na || nb) return na == nb ? a < b : nb;
  return sa != sb ? sa > sb : a < b;
}

// pose_cluster_kernel: one workgroup, thread c owns sample c and keeps its cluster in a register.  Rank = the number of samples that rank before it (B integer
// compares per thread on scores held in LDS), order[rank] = sample.  Then the walk: ONE barrier per ranked sample - the barrier itself carries the question "is
// order[r] still unassigned" from its owner to everybody (__syncthreads_or), so no thread reads a word that another writes in the same step.  Only the steps
// that found a leader read the matrix (row `leader`, coalesced).  The only float operations are the comparisons with the cutoff and with +inf.
__global__ __launch_bounds__(CLUSTER_MAX_B) void pose_cluster_kernel(const float* __restrict__ rmsd, const float* __restrict__ score, float cutoff, int B,
                                                                     int32_t* __restrict__ cluster, int32_t* __restrict__ leaders,
                                                                     int32_t* __restrict__ n_clusters) {
  __shared__ float sc[CLUSTER_MAX_B];
  __shared__ int order[CLUSTER_MAX_B];
  const int c = threadIdx.x;
  if (score) {
    if (c < B) sc[c] = score[c];
    __syncthreads();
    if (c < B) {
      const float mine = sc[c];
      int rank = 0;
      for (int o = 0; o < B; ++o) rank += ranks_before(sc[o], o, mine, c);
      order[rank] = c;
    }
  } else if (c < B) {
    order[c] = c;
  }
  __syncthreads();
  int mine = -1, n = 0;      // n is uniform: every thread counts the leaders
  for (int r = 0; r < B; ++r) {
    const int leader = order[r];
    if (__syncthreads_or(c == leader && mine < 0)) {
      if (c == leader) {
        mine = n;
        leaders[n] = c;
      } else if (c < B && mine < 0) {
        const float d = rmsd[(size_t)leader * B + c];
        if (d <= cutoff && d != INFINITY) mine = n;      // (a NaN distance compares false: it never joins either)
      }
      ++n;
    }
  }
  if (c < B) {
    cluster[c] = mine;
    if (c >= n) leaders[c] = -1;
  }
  if (c == 0) n_clusters[0] = n;
}

hipError_t launch_pose_cluster(const float* rmsd, const float* score, float cutoff, int B, int32_t* cluster, int32_t* leaders, int32_t* n_clusters,
                               hipStream_t s) {
  hipLaunchKernelGGL(pose_cluster_kernel, dim3(1), dim3((B + 63) / 64 * 64), 0, s, rmsd, score, cutoff, B, cluster, leaders, n_clusters);
  return hipGetLastError();
}

}  // namespace ddk
