// Coordinates and bonds in -> the static graph tables of a complex out (see include/ddk.h: ddk_receptor_knn_graph, ddk_radius_graph,
// ddk_ligand_transformation_mask): rec_edge_index (get_calpha_graph, datasets_utils/process_mols.py:337-353), atom_edge_index (radius_graph,
// process_mols.py:471) and edge_mask / mask_rotate (get_transformation_mask, utils/torsion.py:15-45), which the reference builds on the host with scipy,
// torch_cluster and networkx.
//
// Every distance decision is taken in fp64 on the fp32 coordinates: convert, subtract, d2 = dx*dx + dy*dy + dz*dz, compare with (double)r * (double)r,
// strictly below.  Nothing here accumulates floats across threads and nothing takes a slot from an atomic counter: the edges of a row are stored at the
// row's offset (an exclusive scan of the row counts over the rows) plus the neighbour's rank in the row (a scan over the workgroup or the wave), so the
// output is in a fixed order and the same bits every run.
//
//   knn_rows_kernel     one workgroup per residue i (grid-stride).  Counts the j != i under the cutoff; at most max_neighbor of them: kept in ascending j
//                       (block_scan_flags per 256 points).  More, or none: the max_neighbor (or the one) nearest of all other points by (d2, j).  The
//                       threshold is found by a radix select on the bits of d2 (a non-negative double orders like its bits): eight passes of eight
//                       bits, a 256-bin histogram in LDS per pass (integer counts; a wave whose lanes agree on the bin adds once), so a row with
//                       thousands of points under the cutoff costs nine sweeps over the points and no sort of them.  The selected <= 128 are ranked
//                       against each other in LDS.  Row i's neighbours go to the workspace, its count to cnt[i] (-1: pos[i] is not finite).
//   radius_kernel<0>    one wave per centre i: sweeps j ascending 64 at a time (ballot), stops when max_num_neighbors + 1 in-radius points (self included)
//                       are found, cnt[i] = those without self.
//   build_scan_kernel   one workgroup: exclusive scan of cnt over the rows -> off, E and the status, count_out.
//   knn_write_kernel / radius_kernel<1>   store the columns; the latter repeats the sweep (storing the neighbours of every centre for the second
//                       launch would take n * (max_num_neighbors + 1) words).  Every store is guarded by column < cap.
//   lig_mask_kernel     one workgroup, one thread per bond: checks the columns, builds the adjacency bitset (k_lig_bits.h), walks the side of u without the
//                       bond over the bitset rows (a walk that reaches v is a ring bond; thread 0 also walks the whole graph: connected or not), scans the
//                       rotatable flags over the bonds and stores the rows.
#include "model.h"
#include "k_lig_bits.h"

namespace ddk {

namespace {

// the workspace of calls 1 and 2: this header, cnt [n], off [n], then (call 1) nbr [n, max_neighbor]
struct BuildHeader {
  int32_t status;      // 0 complete, 1 more edges than cap (call 2), 2 a coordinate that is not finite
  int32_t E;
};

inline size_t up256(size_t x) { return (x + 255) / 256 * 256; }

struct BuildLayout {
  size_t cnt, off, nbr, total;
};

inline BuildLayout build_layout(int n, int per_row) {
  BuildLayout L;
  L.cnt = up256(sizeof(BuildHeader));
  L.off = L.cnt + up256((size_t)n * sizeof(int32_t));
  L.nbr = L.off + up256((size_t)n * sizeof(int32_t));
  L.total = L.nbr + up256((size_t)n * per_row * sizeof(int32_t));
  return L;
}

// three products and two sums, each rounded (no fused multiply-add): the bits numpy gives for dx*dx + dy*dy + dz*dz
__device__ inline double dist2(const float* __restrict__ pos, int j, double xi, double yi, double zi) {
#pragma clang fp contract(off)
  const double dx = (double)pos[3 * (size_t)j] - xi, dy = (double)pos[3 * (size_t)j + 1] - yi, dz = (double)pos[3 * (size_t)j + 2] - zi;
  return dx * dx + dy * dy + dz * dz;
}

__device__ inline bool finite3(const float* __restrict__ pos, int i) {
  return isfinite(pos[3 * (size_t)i]) && isfinite(pos[3 * (size_t)i + 1]) && isfinite(pos[3 * (size_t)i + 2]);
}

// vis: the atoms reached from `start` over the adjacency bitset without the bond u - v (u < 0: no bond removed).  A walk that reaches v ends there and
// returns true: the bond closes a ring.  Only u's row is masked: v's row is never read.
__device__ inline bool lig_walk(const uint32_t (*adj)[8], int start, int u, int v, uint32_t* vis) {
  uint32_t pend[8];
#pragma unroll
  for (int w = 0; w < 8; ++w) vis[w] = pend[w] = (w == (start >> 5)) ? 1u << (start & 31) : 0u;
  const int vw = u < 0 ? -1 : v >> 5;
  const uint32_t vbit = u < 0 ? 0u : 1u << (v & 31);
  bool ring = false;
  while (!ring) {
    int a = -1;
#pragma unroll
    for (int w = 0; w < 8; ++w) {
      if (a < 0 && pend[w]) {
        a = w * 32 + __ffs(pend[w]) - 1;
        pend[w] &= pend[w] - 1;
      }
    }
    if (a < 0) break;
#pragma unroll
    for (int w = 0; w < 8; ++w) {
      uint32_t r = adj[a][w];
      if (a == u && w == vw) r &= ~vbit;      // the removed bond
      const uint32_t fresh = r & ~vis[w];
      vis[w] |= fresh;
      pend[w] |= fresh;
      if (w == vw && (fresh & vbit)) ring = true;
    }
  }
  return ring;
}

}  // namespace

__global__ __launch_bounds__(KNN_THREADS) void knn_rows_kernel(int n, const float* __restrict__ pos, double c2, int K, int32_t* __restrict__ cnt,
                                                                int32_t* __restrict__ nbr) {
  __shared__ int hist[256];
  __shared__ int wave_sums[KNN_THREADS / 64];
  __shared__ int s_bin, s_excl;
  __shared__ unsigned long long sel_key[KNN_MAX_NEIGHBOR];
  __shared__ int sel_j[KNN_MAX_NEIGHBOR];
  const int tid = threadIdx.x, lane = tid & 63;
  for (int i = blockIdx.x; i < n; i += gridDim.x) {
    const double xi = pos[3 * (size_t)i], yi = pos[3 * (size_t)i + 1], zi = pos[3 * (size_t)i + 2];
    int32_t* row = nbr + (size_t)i * K;
    int mine = 0;
    for (int j = tid; j < n; j += KNN_THREADS) mine += (j != i && dist2(pos, j, xi, yi, zi) < c2) ? 1 : 0;
    int under;
    block_scan_int(mine, wave_sums, &under);
    int m;
    if (under > 0 && under <= K) {      // all of them, ascending j
      int base = 0;
      for (int j0 = 0; j0 < n; j0 += KNN_THREADS) {
        const int j = j0 + tid;
        int total;
        const bool flag = j < n && j != i && dist2(pos, j, xi, yi, zi) < c2;
        const int p = base + block_scan_flags(flag, wave_sums, &total);
        if (flag && p < K) row[p] = j;
        base += total;
      }
      m = under;
    } else {      // the m nearest of all other points by (d2, j); n - 1 >= m: more than K lie under the cutoff, or m = 1 and n >= 2
      m = under > K ? K : 1;
      unsigned long long prefix = 0;
      int need = m;
      for (int shift = 56; shift >= 0; shift -= 8) {
        const unsigned long long hi = shift == 56 ? 0ull : ~0ull << (shift + 8);
        hist[tid] = 0;      // (KNN_THREADS = 256 bins)
        __syncthreads();
        for (int j0 = 0; j0 < n; j0 += KNN_THREADS) {
          const int j = j0 + tid;
          bool part = j < n && j != i;
          int bin = 0;
          if (part) {
            const unsigned long long key = (unsigned long long)__double_as_longlong(dist2(pos, j, xi, yi, zi));
            part = (key & hi) == prefix;
            bin = (int)((key >> shift) & 255);
          }
          const unsigned long long who = __ballot(part);
          if (who) {      // the lanes that agree with the first one add once (the leading bytes of d2 are the same for most of a row)
            const int leader = __ffsll(who) - 1, b0 = __shfl(bin, leader, 64);
            const unsigned long long same = __ballot(part && bin == b0);
            if (lane == leader) atomicAdd(&hist[b0], __popcll(same));
            if (part && bin != b0) atomicAdd(&hist[bin], 1);
          }
        }
        __syncthreads();
        const int h = hist[tid];
        int total;
        const int excl = block_scan_int(h, wave_sums, &total);
        if (excl < need && need <= excl + h) {      // exactly one bin: need <= the count of the points that share the prefix
          s_bin = tid;
          s_excl = excl;
        }
        __syncthreads();
        prefix |= (unsigned long long)s_bin << shift;
        need -= s_excl;
        __syncthreads();
      }
      // every key below the threshold, and the first `need` of the keys equal to it in ascending j
      int base_lt = 0, base_eq = 0;
      for (int j0 = 0; j0 < n; j0 += KNN_THREADS) {
        const int j = j0 + tid;
        unsigned long long key = 0;
        bool lt = false, eq = false;
        if (j < n && j != i) {
          key = (unsigned long long)__double_as_longlong(dist2(pos, j, xi, yi, zi));
          lt = key < prefix;
          eq = key == prefix;
        }
        int total;
        const int excl = block_scan_int((lt ? 1 : 0) | (eq ? 1 << 16 : 0), wave_sums, &total);      // two counts of at most 256 in one word
        const int lt_before = base_lt + (excl & 0xffff), eq_before = base_eq + (excl >> 16);
        const int p = lt_before + (eq_before < need ? eq_before : need);
        if ((lt || (eq && eq_before < need)) && p < m) {
          sel_key[p] = key;
          sel_j[p] = j;
        }
        base_lt += total & 0xffff;
        base_eq += total >> 16;
      }
      __syncthreads();
      if (tid < m) {      // rank among the selected: nearest first, ties to the lower index
        const unsigned long long key = sel_key[tid];
        const int j = sel_j[tid];
        int rank = 0;
        for (int s = 0; s < m; ++s) rank += (sel_key[s] < key || (sel_key[s] == key && sel_j[s] < j)) ? 1 : 0;
        row[rank] = j;
      }
      __syncthreads();      // sel_* are the next row's
    }
    if (tid == 0) cnt[i] = finite3(pos, i) ? m : -1;
  }
}

__global__ __launch_bounds__(BUILD_SCAN_THREADS) void build_scan_kernel(int n, const int32_t* __restrict__ cnt, int32_t* __restrict__ off, int cap,
                                                                        BuildHeader* __restrict__ H, int32_t* __restrict__ count_out) {
  __shared__ int wave_sums[BUILD_SCAN_THREADS / 64];
  const int per = (n + BUILD_SCAN_THREADS - 1) / BUILD_SCAN_THREADS, first = threadIdx.x * per;      // n <= 65536: at most 64 rows per thread
  int sum = 0, bad = 0;
  for (int k = 0; k < per; ++k) {
    const int i = first + k;
    if (i < n) {
      const int c = cnt[i];
      if (c < 0) bad = 1; else sum += c;
    }
  }
  int total;
  int run = block_scan_int(sum, wave_sums, &total);
  const int any_bad = __syncthreads_or(bad);
  for (int k = 0; k < per; ++k) {
    const int i = first + k;
    if (i < n) {
      off[i] = run;
      const int c = cnt[i];
      run += c < 0 ? 0 : c;
    }
  }
  if (threadIdx.x == 0) {
    const int status = any_bad ? 2 : (total > cap ? 1 : 0);      // total <= 65536 * 1025
    H->status = status;
    H->E = any_bad ? 0 : total;
    count_out[0] = any_bad ? 0 : total;
    count_out[1] = status;
  }
}

__global__ __launch_bounds__(256) void knn_write_kernel(int n, int K, const int32_t* __restrict__ cnt, const int32_t* __restrict__ off,
                                                         const int32_t* __restrict__ nbr, const BuildHeader* __restrict__ H, int32_t* __restrict__ out,
                                                         int cap) {
  if (H->status != 0) return;
  const size_t cells = (size_t)n * K;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < cells; e += (size_t)gridDim.x * 256) {
    const int i = (int)(e / K), k = (int)(e - (size_t)i * K);
    if (k >= cnt[i]) continue;
    const int col = off[i] + k;
    if (col < cap) {
      out[col] = i;
      out[(size_t)cap + col] = nbr[e];
    }
  }
}

// one wave per centre.  FILL = false: cnt[i]; FILL = true: the columns [j; i] at off[i] + the neighbour's rank
template <bool FILL>
__global__ __launch_bounds__(256) void radius_kernel(int n, const float* __restrict__ pos, double r2, int quota, int32_t* __restrict__ cnt,
                                                      const int32_t* __restrict__ off, const BuildHeader* __restrict__ H, int32_t* __restrict__ out, int cap) {
  if (FILL && H->status == 2) return;
  const int lane = threadIdx.x & 63, waves = gridDim.x * 4;
  for (int i = blockIdx.x * 4 + (threadIdx.x >> 6); i < n; i += waves) {      // (i is the same in every lane of the wave)
    const double xi = pos[3 * (size_t)i], yi = pos[3 * (size_t)i + 1], zi = pos[3 * (size_t)i + 2];
    const bool self_in = 0.0 < r2 && finite3(pos, i);      // d2(i, i) = 0: the centre is one of its own in-radius points
    const int base = FILL ? off[i] : 0;
    int c = 0, self_taken = 0;
    for (int j0 = 0; j0 < n && c < quota; j0 += 64) {
      const int j = j0 + lane;
      const bool in = j < n && dist2(pos, j, xi, yi, zi) < r2;
      const unsigned long long b = __ballot(in);
      const int rank = __popcll(b & ((1ull << lane) - 1ull)), room = quota - c, found = __popcll(b);
      const bool taken = in && rank < room;
      if (__ballot(taken && j == i)) self_taken = 1;
      if (FILL && taken && j != i) {
        const int col = base + c + rank - ((j > i && self_in) ? 1 : 0);      // a taken j above i: i was taken before it
        if (col < cap) {
          out[col] = j;
          out[(size_t)cap + col] = i;
        }
      }
      c += found < room ? found : room;
    }
    if (!FILL && lane == 0) cnt[i] = finite3(pos, i) ? c - self_taken : -1;
  }
}

__global__ __launch_bounds__(LIG_MASK_THREADS) void lig_mask_kernel(int n_lig, const int32_t* __restrict__ bond_index, int M, uint8_t* __restrict__ edge_mask,
                                                                     uint8_t* __restrict__ mask_rotate, int cap_rot, int32_t* __restrict__ count_out,
                                                                     uint32_t* __restrict__ rows) {
  __shared__ uint32_t adj[MAX_LIG][8];
  __shared__ int wave_sums[LIG_MASK_THREADS / 64];
  __shared__ int whole[8];
  const int tid = threadIdx.x, nb = M / 2;      // nb <= LIG_MASK_THREADS: bond tid is this thread's
  for (int e = tid; e < MAX_LIG * 8; e += LIG_MASK_THREADS) adj[e >> 3][e & 7] = 0;
  int u = 0, v = 0, bad = 0;
  if (tid < nb) {
    u = bond_index[2 * tid];
    v = bond_index[(size_t)M + 2 * tid];
    bad = ((unsigned)u >= (unsigned)n_lig || (unsigned)v >= (unsigned)n_lig || u == v || bond_index[2 * tid + 1] != v ||
           bond_index[(size_t)M + 2 * tid + 1] != u) ? 1 : 0;
  }
  int any_bad = __syncthreads_or(bad);      // (and adj is zero)
  if (!any_bad) {
    if (tid < nb) bad = adj256_add(adj, u < v ? u : v, u < v ? v : u) ? 1 : 0;      // set before: the same bond twice, in either direction
    any_bad = __syncthreads_or(bad);
  }
  int status = any_bad ? 2 : 0;
  // the side of u without this thread's bond; thread 0 first walks the whole graph from atom 0
  uint32_t vis[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  bool ring = false;
  if (status == 0 && tid == 0) {
    lig_walk(adj, 0, -1, -1, vis);
#pragma unroll
    for (int w = 0; w < 8; ++w) whole[w] = __popc(vis[w]);
  }
  if (status == 0 && tid < nb) ring = lig_walk(adj, u, u, v, vis);
  __syncthreads();
  if (status == 0) {
    int reached = 0;
    for (int w = 0; w < 8; ++w) reached += whole[w];
    if (reached != n_lig) status = 3;
  }
  bool rot = false, u_side = false;
  if (status == 0 && tid < nb && !ring) {
    int size_u = 0;
#pragma unroll
    for (int w = 0; w < 8; ++w) size_u += __popc(vis[w]);
    // l: the smaller side; of two equal sides the one with the lowest atom index, atom 0 (networkx's component order under a stable sort)
    u_side = 2 * size_u < n_lig || (2 * size_u == n_lig && (vis[0] & 1u));
    rot = (u_side ? size_u : n_lig - size_u) > 1;
  }
  int R;
  const int r = block_scan_flags(rot, wave_sums, &R);
  if (status == 0 && R > cap_rot) status = 1;
  if (status == 0 && rot) {
#pragma unroll
    for (int w = 0; w < 8; ++w) {
      const int left = n_lig - 32 * w;
      const uint32_t valid = left >= 32 ? ~0u : (left > 0 ? (1u << left) - 1u : 0u);
      rows[(size_t)r * 8 + w] = u_side ? vis[w] : (~vis[w] & valid);
    }
  }
  if (tid < nb) {      // the marked direction: 2k + 1 (v -> u) if u is on l, else 2k; the head rotates
    const bool on = status == 0 && rot;
    edge_mask[2 * tid] = on && !u_side ? 1 : 0;
    edge_mask[2 * tid + 1] = on && u_side ? 1 : 0;
  }
  if (tid == 0) {
    count_out[0] = (status == 0 || status == 1) ? R : 0;
    count_out[1] = status;
  }
  if (status != 0) return;
  __threadfence_block();
  __syncthreads();      // rows: written by this workgroup, read by it
  const int cells = R * n_lig;      // R <= 1024, n_lig <= 256
  for (int e = tid; e < cells; e += LIG_MASK_THREADS) {
    const int k = e / n_lig, a = e - k * n_lig;
    mask_rotate[e] = (rows[(size_t)k * 8 + (a >> 5)] >> (a & 31)) & 1u;
  }
}

int64_t knn_graph_workspace_bytes(int n, int max_neighbor) { return (int64_t)build_layout(n, max_neighbor).total; }
int64_t radius_graph_workspace_bytes(int n) { return (int64_t)build_layout(n, 0).total; }
int64_t lig_mask_workspace_bytes(int M) { return (int64_t)up256((size_t)(M / 2 > 0 ? M / 2 : 1) * 8 * sizeof(uint32_t)); }

hipError_t launch_receptor_knn_graph(int n, const float* pos, float cutoff, int max_neighbor, int32_t* edge_index_out, int cap, int32_t* count_out,
                                     void* workspace, hipStream_t s) {
  const BuildLayout L = build_layout(n, max_neighbor);
  uint8_t* ws = (uint8_t*)workspace;
  BuildHeader* H = (BuildHeader*)ws;
  int32_t *cnt = (int32_t*)(ws + L.cnt), *off = (int32_t*)(ws + L.off), *nbr = (int32_t*)(ws + L.nbr);
  hipLaunchKernelGGL(knn_rows_kernel, dim3(n < BUILD_GRID ? n : BUILD_GRID), dim3(KNN_THREADS), 0, s, n, pos, (double)cutoff * (double)cutoff, max_neighbor,
                     cnt, nbr);
  hipLaunchKernelGGL(build_scan_kernel, dim3(1), dim3(BUILD_SCAN_THREADS), 0, s, n, cnt, off, cap, H, count_out);
  const size_t blocks = ((size_t)n * max_neighbor + 255) / 256;
  hipLaunchKernelGGL(knn_write_kernel, dim3((unsigned)(blocks < (size_t)BUILD_GRID ? blocks : (size_t)BUILD_GRID)), dim3(256), 0, s, n, max_neighbor, cnt, off,
                     nbr, H, edge_index_out, cap);
  return hipGetLastError();
}

hipError_t launch_radius_graph(int n, const float* pos, float r, int max_num_neighbors, int32_t* edge_index_out, int cap, int32_t* count_out,
                               void* workspace, hipStream_t s) {
  const BuildLayout L = build_layout(n, 0);
  uint8_t* ws = (uint8_t*)workspace;
  BuildHeader* H = (BuildHeader*)ws;
  int32_t *cnt = (int32_t*)(ws + L.cnt), *off = (int32_t*)(ws + L.off);
  const double r2 = (double)r * (double)r;
  const int blocks = (n + 3) / 4, grid = blocks < BUILD_GRID ? blocks : BUILD_GRID;
  hipLaunchKernelGGL(radius_kernel<false>, dim3(grid), dim3(256), 0, s, n, pos, r2, max_num_neighbors + 1, cnt, off, H, edge_index_out, cap);
  hipLaunchKernelGGL(build_scan_kernel, dim3(1), dim3(BUILD_SCAN_THREADS), 0, s, n, cnt, off, cap, H, count_out);
  hipLaunchKernelGGL(radius_kernel<true>, dim3(grid), dim3(256), 0, s, n, pos, r2, max_num_neighbors + 1, cnt, off, H, edge_index_out, cap);
  return hipGetLastError();
}

hipError_t launch_ligand_transformation_mask(int n_lig, const int32_t* bond_index, int M, uint8_t* edge_mask_out, uint8_t* mask_rotate_out, int cap_rot,
                                             int32_t* count_out, void* workspace, hipStream_t s) {
  hipLaunchKernelGGL(lig_mask_kernel, dim3(1), dim3(LIG_MASK_THREADS), 0, s, n_lig, bond_index, M, edge_mask_out, mask_rotate_out, cap_rot, count_out,
                     (uint32_t*)workspace);
  return hipGetLastError();
}

}  // namespace ddk
