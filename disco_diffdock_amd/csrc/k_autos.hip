// Ligand graph in -> its automorphism table out (see include/ddk.h: ddk_ligand_automorphisms): the table perms [K, n_lig] that pose_metrics_kernel
// (k_se3.hip) and pose_pairs_kernel (k_pairs.hip) read, enumerated where they read it instead of by spyrmsd / networkx on another machine
// (evaluate.py:308-313 falls back to the uncorrected RMSD when that search passes the 10 s of utils/utils.py:84-98).
//
// The search is level-synchronous.  The kept atoms are put in a matching order (breadth-first from the lowest unvisited kept atom, component by component,
// neighbours ascending), so every atom but a component's root has an already-ordered neighbour, its parent.  The frontier of level d holds every partial map
// of order[0 .. d) that is still consistent, one row of uint8 per map (row[u] = the image of order[u]; 255 is an atom like any other).  Level d, atom
// v = order[d]: a row's candidates are the kept neighbours of image(parent(v)) (all kept atoms for a root), in ascending order.  The image of the parent has
// the parent's degree (that was checked when it was chosen), so EVERY row of a level has the same number S of candidate slots and the work items of a level
// are the flat pairs t = row * S + slot.  A candidate c survives if it is unused in the row, has v's colour and degree, and is adjacent to the image of u
// exactly when v is adjacent to u, for every mapped u.  The children are the surviving items in flat order: an exclusive scan of the survival flags over t is
// the child's row index, so the table comes out in (parent row, candidate) ascending order, the same bits every run, with no atomic cursor.
//
//   autos_walk_kernel   one workgroup: builds the 256 x 256 adjacency bitset (8 KB of LDS), degrees and the matching order, keeps them in the workspace, and
//                       walks levels with one barrier each while a level has at most AUTOS_WALK_ITEMS items (every level if the host saw that
//                       cap * n_lig <= AUTOS_WALK_ONLY_ITEMS).  The usual molecule never leaves it.
//   autos_count_kernel  + autos_write_kernel: one pending level per pair of launches, over a fixed grid.  count writes the survivors of each chunk of
//                       AUTOS_CHUNK items, write sums the chunks before its own (the scan across workgroups), scans inside the chunk and stores the
//                       children.  The host enqueues n_lig - 1 pairs without knowing how many find work: each reads its level and row count from the
//                       workspace (slot i of the state arrays) and leaves the next state in slot i + 1.  A pair with nothing to do copies the state on.
//   autos_emit_kernel   rows (by matching position, uint8) -> perms_out (by atom, int32), masked-out atoms to themselves, and count_out.
// Nothing spins on a flag and nothing is cooperative: levels are separated by s_barrier inside the one workgroup or by launch boundaries.  A frontier of more
// than cap rows is status 1, a bond index outside [0, n_lig) is status 2 (found before it is used as an address); both emit the identity alone.  Every
// store of a row is guarded by the row index < cap.
#include "model.h"
#include "k_lig_bits.h"

namespace ddk {

namespace {

// the workspace: this header, then AUTOS chunk sums, then the two frontier buffers of cap rows (autos_layout)
struct AutosHeader {
  int32_t status;                         // 0 complete, 1 overflow, 2 bad bond index
  int32_t m;                              // kept atoms = levels
  int32_t level[MAX_LIG + 2];             // state slot i: the first level that is not done yet (m: none), read by launch pair i, written by pair i - 1
  int32_t count[MAX_LIG + 2];             //               the rows of that level's frontier (in buffer level & 1)
  uint32_t adj[MAX_LIG][8];               // adjacency of the kept atoms, bit b of row a: {a, b} is an edge
  uint32_t kept[8];
  int32_t parent[MAX_LIG];                // matching position of order[d]'s parent, -1 for a component's root
  uint8_t order[MAX_LIG];
  uint8_t deg[MAX_LIG];
};

struct AutosLayout {
  int stride;              // bytes per frontier row (a multiple of 4: rows are read and copied as words)
  size_t chunks, sums, buf0, buf1, total;
};

inline AutosLayout autos_layout(int n_lig, int cap) {
  AutosLayout L;
  L.stride = (n_lig + 3) / 4 * 4;
  L.chunks = ((size_t)cap * n_lig + AUTOS_CHUNK - 1) / AUTOS_CHUNK;
  auto up = [](size_t x) { return (x + 255) / 256 * 256; };
  L.sums = up(sizeof(AutosHeader));
  L.buf0 = L.sums + up(L.chunks * sizeof(int32_t));
  L.buf1 = L.buf0 + up((size_t)cap * L.stride);
  L.total = L.buf1 + up((size_t)cap * L.stride);
  return L;
}

// what a workgroup needs of the header, in LDS
struct AutosTables {
  uint32_t adj[MAX_LIG][8];
  uint32_t kept[8];
  int32_t colour[MAX_LIG];
  int32_t parent[MAX_LIG];
  uint8_t order[MAX_LIG];
  uint8_t deg[MAX_LIG];
};

__device__ inline void autos_load_tables(AutosTables& T, const AutosHeader* H, const int32_t* colour, int n_lig) {
  for (int e = threadIdx.x; e < MAX_LIG * 8; e += blockDim.x) T.adj[e >> 3][e & 7] = H->adj[e >> 3][e & 7];
  for (int a = threadIdx.x; a < MAX_LIG; a += blockDim.x) {
    T.colour[a] = a < n_lig ? colour[a] : 0;
    T.parent[a] = H->parent[a];
    T.order[a] = H->order[a];
    T.deg[a] = H->deg[a];
    if (a < 8) T.kept[a] = H->kept[a];
  }
}

// the slot-th set bit of a 256-bit set (slot < its popcount; 0 otherwise, which the checks then refuse or accept like any atom)
__device__ inline int autos_select(const uint32_t* set, int slot) {
  for (int w = 0; w < 8; ++w) {
    uint32_t x = set[w];
    const int n = __popc(x);
    if (slot < n) {
      for (int i = 0; i < slot; ++i) x &= x - 1;
      return w * 32 + __ffs(x) - 1;
    }
    slot -= n;
  }
  return 0;
}

struct AutosLevel {
  int d, v, S;
  bool root;
  int parent;
};

__device__ inline AutosLevel autos_level(const AutosTables& T, int d, int m) {
  AutosLevel L;
  L.d = d;
  L.v = T.order[d];
  L.parent = T.parent[d];
  L.root = L.parent < 0;
  L.S = L.root ? m : T.deg[T.order[L.parent]];
  return L;
}

// item t of a level: does candidate `slot` of row t / S survive?  c_out: the candidate.  The four rules of the header comment, nothing else.
__device__ inline bool autos_item(const AutosTables& T, const AutosLevel& L, const uint8_t* frontier, int stride, int t, int* row_out, int* c_out) {
  const int row = t / L.S, slot = t - row * L.S;
  const uint32_t* R = (const uint32_t*)(frontier + (size_t)row * stride);
  *row_out = row;
  int c;
  if (L.root) {
    c = autos_select(T.kept, slot);
  } else {
    const int pimg = (R[L.parent >> 2] >> (8 * (L.parent & 3))) & 255;
    c = autos_select(T.adj[pimg], slot);
  }
  *c_out = c;
  if (T.colour[c] != T.colour[L.v] || T.deg[c] != T.deg[L.v]) return false;
  uint32_t w = 0;
  for (int u = 0; u < L.d; ++u) {
    if ((u & 3) == 0) w = R[u >> 2];
    const int img = (w >> (8 * (u & 3))) & 255, ou = T.order[u];
    if (img == c) return false;
    if (((T.adj[L.v][ou >> 5] >> (ou & 31)) & 1) != ((T.adj[c][img >> 5] >> (img & 31)) & 1)) return false;
  }
  return true;
}

// child row = the parent row's d bytes and c; whole words (the bytes past d in the last word are never read before they are written)
__device__ inline void autos_store_child(uint8_t* next, const uint8_t* frontier, int stride, int d, int row, int c, int pos) {
  const uint32_t* R = (const uint32_t*)(frontier + (size_t)row * stride);
  uint32_t* W = (uint32_t*)(next + (size_t)pos * stride);
  const int last = d >> 2, sh = 8 * (d & 3);
  for (int k = 0; k < last; ++k) W[k] = R[k];
  const uint32_t keep = sh ? (R[last] & ((1u << sh) - 1u)) : 0u;
  W[last] = keep | ((uint32_t)c << sh);
}

}  // namespace

__global__ __launch_bounds__(AUTOS_WALK_THREADS) void autos_walk_kernel(int n_lig, const int32_t* __restrict__ colour, const int32_t* __restrict__ bond_index,
                                                                        int n_bond_edges, const uint8_t* __restrict__ atom_mask, int cap, int walk_only,
                                                                        AutosHeader* __restrict__ H, uint8_t* buf0, uint8_t* buf1, int stride) {
  __shared__ AutosTables T;
  __shared__ int wave_sums[AUTOS_WALK_THREADS / 64];
  __shared__ int bad, m_s;
  __shared__ uint8_t queue_done[MAX_LIG];
  const int tid = threadIdx.x;
  for (int e = tid; e < MAX_LIG * 8; e += AUTOS_WALK_THREADS) T.adj[e >> 3][e & 7] = 0;
  if (tid < 8) T.kept[tid] = 0;
  if (tid == 0) bad = 0;
  __syncthreads();
  if (tid < MAX_LIG) {
    const bool k = tid < n_lig && (atom_mask ? atom_mask[tid] != 0 : true);
    T.colour[tid] = tid < n_lig ? colour[tid] : 0;
    if (k) atomicOr(&T.kept[tid >> 5], 1u << (tid & 31));
    queue_done[tid] = 0;
  }
  __syncthreads();
  for (int e = tid; e < n_bond_edges; e += AUTOS_WALK_THREADS) {
    const int a = bond_index[e], b = bond_index[(size_t)n_bond_edges + e];
    if ((unsigned)a >= (unsigned)n_lig || (unsigned)b >= (unsigned)n_lig) {
      bad = 1;      // (every writer writes the same value)
    } else if (a != b && ((T.kept[a >> 5] >> (a & 31)) & 1) && ((T.kept[b >> 5] >> (b & 31)) & 1)) {
      adj256_add(T.adj, a, b);      // OR: duplicates and the two directions of a bond are one edge, in any arrival order
    }
  }
  __syncthreads();
  if (tid < MAX_LIG) {
    int dg = 0;
    for (int w = 0; w < 8; ++w) dg += __popc(T.adj[tid][w]);
    T.deg[tid] = (uint8_t)dg;      // at most 255: an atom is not its own neighbour
  }
  if (tid == 0) {
    // the matching order: order[] is its own breadth-first queue
    int m = 0, head = 0;
    for (int r = 0; r < n_lig; ++r) {
      if (!((T.kept[r >> 5] >> (r & 31)) & 1) || queue_done[r]) continue;
      queue_done[r] = 1;
      T.order[m] = (uint8_t)r;
      T.parent[m++] = -1;
      for (; head < m; ++head) {
        const int p = T.order[head];
        for (int w = 0; w < 8; ++w) {
          for (uint32_t x = T.adj[p][w]; x; x &= x - 1) {
            const int q = w * 32 + __ffs(x) - 1;
            if (queue_done[q]) continue;
            queue_done[q] = 1;
            T.order[m] = (uint8_t)q;
            T.parent[m++] = head;
          }
        }
      }
    }
    for (int d = m; d < MAX_LIG; ++d) {
      T.order[d] = 0;
      T.parent[d] = -1;
    }
    m_s = m;
  }
  __syncthreads();
  const int m = m_s;
  // keep the tables for the later launches
  for (int e = tid; e < MAX_LIG * 8; e += AUTOS_WALK_THREADS) H->adj[e >> 3][e & 7] = T.adj[e >> 3][e & 7];
  if (tid < MAX_LIG) {
    H->parent[tid] = T.parent[tid];
    H->order[tid] = T.order[tid];
    H->deg[tid] = T.deg[tid];
    if (tid < 8) H->kept[tid] = T.kept[tid];
  }
  int d = 0, cnt = 1, status = bad ? 2 : 0;      // level 0: one empty row (no byte of it is read)
  if (status == 0) {
    while (d < m) {
      const AutosLevel L = autos_level(T, d, m);
      const int items = cnt * L.S;      // cnt <= cap <= 2^20, S <= 256
      if (!walk_only && items > AUTOS_WALK_ITEMS) break;
      const uint8_t* cur = (d & 1) ? buf1 : buf0;
      uint8_t* nxt = (d & 1) ? buf0 : buf1;
      int base = 0;
      for (int t0 = 0; t0 < items; t0 += AUTOS_WALK_THREADS) {
        const int t = t0 + tid;
        int row = 0, c = 0, total;
        const bool flag = t < items && autos_item(T, L, cur, stride, t, &row, &c);
        const int pos = base + block_scan_flags(flag, wave_sums, &total);
        if (flag && pos < cap) autos_store_child(nxt, cur, stride, d, row, c, pos);
        base += total;
        if (base > cap) break;      // (uniform)
      }
      if (base > cap) {
        status = 1;
        break;
      }
      cnt = base;
      ++d;
      __threadfence_block();
      __syncthreads();      // the children are the next level's rows
    }
  }
  if (tid == 0) {
    H->status = status;
    H->m = m;
    H->level[1] = status ? m : d;
    H->count[1] = status ? 0 : cnt;
  }
}

__global__ __launch_bounds__(AUTOS_CHUNK) void autos_count_kernel(int i, int n_lig, const int32_t* __restrict__ colour, const AutosHeader* __restrict__ H,
                                                                  int32_t* __restrict__ sums, const uint8_t* buf0, const uint8_t* buf1, int stride) {
  const int m = H->m, d = H->level[i], cnt = H->count[i];
  if (d >= m || cnt < 1) return;
  __shared__ AutosTables T;
  autos_load_tables(T, H, colour, n_lig);
  __syncthreads();
  const AutosLevel L = autos_level(T, d, m);
  const int items = cnt * L.S, chunks = (items + AUTOS_CHUNK - 1) / AUTOS_CHUNK;
  const uint8_t* cur = (d & 1) ? buf1 : buf0;
  for (int b = blockIdx.x; b < chunks; b += gridDim.x) {
    const int t = b * AUTOS_CHUNK + threadIdx.x;
    int row, c;
    const int total = __syncthreads_count(t < items && autos_item(T, L, cur, stride, t, &row, &c));
    if (threadIdx.x == 0) sums[b] = total;
  }
}

__global__ __launch_bounds__(AUTOS_CHUNK) void autos_write_kernel(int i, int n_lig, const int32_t* __restrict__ colour, int cap, AutosHeader* __restrict__ H,
                                                                  const int32_t* __restrict__ sums, uint8_t* buf0, uint8_t* buf1, int stride) {
  const int m = H->m, d = H->level[i], cnt = H->count[i];
  if (d >= m || cnt < 1) {      // nothing pending: hand the state on (no row cannot happen, the identity survives every level; emit refuses such a state)
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      H->level[i + 1] = d;
      H->count[i + 1] = cnt;
    }
    return;
  }
  __shared__ AutosTables T;
  __shared__ int wave_sums[AUTOS_CHUNK / 64];
  __shared__ int part[AUTOS_CHUNK / 64];
  autos_load_tables(T, H, colour, n_lig);
  __syncthreads();
  const AutosLevel L = autos_level(T, d, m);
  const int items = cnt * L.S, chunks = (items + AUTOS_CHUNK - 1) / AUTOS_CHUNK;
  const uint8_t* cur = (d & 1) ? buf1 : buf0;
  uint8_t* nxt = (d & 1) ? buf0 : buf1;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int b = blockIdx.x; b < chunks; b += gridDim.x) {
    // the survivors of the chunks before this one: integer sums, any order gives the same number
    int s = 0;
    for (int k = threadIdx.x; k < b; k += AUTOS_CHUNK) s += sums[k];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    __syncthreads();
    if (lane == 0) part[wave] = s;
    __syncthreads();
    int base = 0;
    for (int w = 0; w < AUTOS_CHUNK / 64; ++w) base += part[w];
    const int t = b * AUTOS_CHUNK + threadIdx.x;
    int row = 0, c = 0, total;
    const bool flag = t < items && autos_item(T, L, cur, stride, t, &row, &c);
    const int pos = base + block_scan_flags(flag, wave_sums, &total);
    if (flag && pos < cap) autos_store_child(nxt, cur, stride, d, row, c, pos);
    if (b == chunks - 1 && threadIdx.x == 0) {      // the last chunk knows the next level's row count
      const int next = base + total;
      if (next > cap) {
        H->status = 1;
        H->level[i + 1] = m;
        H->count[i + 1] = 0;
      } else {
        H->level[i + 1] = d + 1;
        H->count[i + 1] = next;
      }
    }
  }
}

__global__ __launch_bounds__(256) void autos_emit_kernel(int fin, int n_lig, int cap, const AutosHeader* __restrict__ H, const uint8_t* buf0,
                                                         const uint8_t* buf1, int stride, int32_t* __restrict__ perms_out, int32_t* __restrict__ count_out) {
  __shared__ int pos_of[MAX_LIG];      // matching position of an atom, -1: masked out
  const int m = H->m;
  int status = H->status, cnt = H->count[fin];
  if (status == 0 && (H->level[fin] != m || cnt < 1 || cnt > cap)) status = 1;      // (cannot happen: n_lig - 1 pairs cover every level; never trust a count)
  for (int a = threadIdx.x; a < MAX_LIG; a += 256) pos_of[a] = -1;
  __syncthreads();
  for (int u = threadIdx.x; u < m; u += 256) pos_of[H->order[u]] = u;
  __syncthreads();
  const int rows = status ? 1 : cnt;
  const uint8_t* fr = (m & 1) ? buf1 : buf0;
  const size_t n = (size_t)rows * n_lig;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256) {
    const int k = (int)(e / n_lig), a = (int)(e - (size_t)k * n_lig), u = pos_of[a];
    perms_out[e] = (status || u < 0) ? a : fr[(size_t)k * stride + u];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    count_out[0] = rows;
    count_out[1] = status;
  }
}

int64_t autos_workspace_bytes(int n_lig, int cap) { return (int64_t)autos_layout(n_lig, cap).total; }

hipError_t launch_ligand_automorphisms(int n_lig, const int32_t* colour, const int32_t* bond_index, int n_bond_edges, const uint8_t* atom_mask,
                                       int32_t* perms_out, int cap, int32_t* count_out, void* workspace, hipStream_t s) {
  const AutosLayout L = autos_layout(n_lig, cap);
  uint8_t* ws = (uint8_t*)workspace;
  AutosHeader* H = (AutosHeader*)ws;
  int32_t* sums = (int32_t*)(ws + L.sums);
  uint8_t *buf0 = ws + L.buf0, *buf1 = ws + L.buf1;
  const bool walk_only = (size_t)cap * n_lig <= (size_t)AUTOS_WALK_ONLY_ITEMS;
  hipLaunchKernelGGL(autos_walk_kernel, dim3(1), dim3(AUTOS_WALK_THREADS), 0, s, n_lig, colour, bond_index, n_bond_edges, atom_mask, cap, (int)walk_only, H,
                     buf0, buf1, L.stride);
  int fin = 1;
  if (!walk_only) {
    const int grid = (int)(L.chunks < (size_t)AUTOS_GRID ? L.chunks : (size_t)AUTOS_GRID);
    for (int i = 1; i < n_lig; ++i) {      // level 0 is the walk's (at most 256 items); a pair per further level, whether it finds one pending or not
      hipLaunchKernelGGL(autos_count_kernel, dim3(grid), dim3(AUTOS_CHUNK), 0, s, i, n_lig, colour, H, sums, buf0, buf1, L.stride);
      hipLaunchKernelGGL(autos_write_kernel, dim3(grid), dim3(AUTOS_CHUNK), 0, s, i, n_lig, colour, cap, H, sums, buf0, buf1, L.stride);
    }
    fin = n_lig;
  }
  const size_t cells = (size_t)cap * n_lig;
  const int egrid = (int)((cells + 255) / 256 < 1024 ? (cells + 255) / 256 : 1024);
  hipLaunchKernelGGL(autos_emit_kernel, dim3(egrid), dim3(256), 0, s, fin, n_lig, cap, H, buf0, buf1, L.stride, perms_out, count_out);
  return hipGetLastError();
}

}  // namespace ddk
