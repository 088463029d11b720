// The ragged class axis of the latent-choice kernels (k_gumbel.hip, k_node_ce.hip): ONE WORKGROUP of RAGGED_T threads walks a graph's ligand nodes, then its
// receptor nodes, as the positions p = 0 .. n_lig_g + n_rec_g - 1, and reduces over them with a fixed halving tree.  Device helpers only; the callers own
// the __shared__ tiles.  Every per-thread partial sum and every first-of-equals rule of those files rests on the order written here: thread t visits the
// quads t, t + RAGGED_T, ... of four positions each, the positions of a quad ascending; the RAGGED_T partials are then combined pairwise, [t] with [t + s]
// for s = RAGGED_T / 2, ..., 1.
#pragma once
#include <cstdint>

namespace ddk {

constexpr int RAGGED_T = 256;

// the graph's nodes on both sides, or n < 0 where a pointer pair is no range of its table (the graph is then left alone)
struct RaggedGraph { int64_t l0, r0, nl, n; };
__device__ __forceinline__ RaggedGraph ragged_graph(const int64_t* lig_ptr, const int64_t* rec_ptr, int64_t n_lig, int64_t n_rec, int g) {
  const int64_t l0 = lig_ptr[g], l1 = lig_ptr[g + 1], r0 = rec_ptr[g], r1 = rec_ptr[g + 1];
  const bool ok = l0 >= 0 && l0 <= l1 && l1 <= n_lig && r0 >= 0 && r0 <= r1 && r1 <= n_rec;
  return RaggedGraph{l0, r0, l1 - l0, ok ? (l1 - l0) + (r1 - r0) : -1};
}
// position p -> its row in the ligand (lig) or the receptor table
__device__ __forceinline__ int64_t ragged_row(const RaggedGraph& G, int64_t p, bool& lig) {
  lig = p < G.nl;
  return lig ? G.l0 + p : G.r0 + (p - G.nl);
}

// f(q, i, p) for every position p = 4 q + i of this thread's quads, in the order above (i = 0 is visited for every quad q the thread owns)
template <class F>
__device__ __forceinline__ void ragged_for_each(const RaggedGraph& G, F f) {
  const int64_t quads = (G.n + 3) >> 2;
  for (int64_t q = threadIdx.x; q < quads; q += RAGGED_T) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t p = 4 * q + i;
      if (p < G.n) f(q, i, p);
    }
  }
}

// red[0] after the halving tree over the RAGGED_T values v with op
template <class T, class Op>
__device__ __forceinline__ T ragged_tree(T* red, T v, Op op) {
  const int t = threadIdx.x;
  __syncthreads();      // (the tile may still be read from the reduction before)
  red[t] = v;
  __syncthreads();
  for (int s = RAGGED_T / 2; s > 0; s >>= 1) {
    if (t < s) red[t] = op(red[t], red[t + s]);
    __syncthreads();
  }
  return red[0];
}
template <class T>
__device__ __forceinline__ T ragged_tree_sum(T* red, T v) { return ragged_tree(red, v, [](T a, T b) { return a + b; }); }
__device__ __forceinline__ double ragged_tree_fmax(double* red, double v) { return ragged_tree(red, v, [](double a, double b) { return fmax(a, b); }); }

// the maximum over the workgroup and into ``where`` the lowest position that holds it: the larger value wins, among equals the lower position.  A thread
// that compared nothing passes where = INT64_MAX; that is also the answer when no thread did
template <class T>
__device__ __forceinline__ T ragged_tree_argmax(T* red, int64_t* redi, T v, int64_t& where) {
  const int t = threadIdx.x;
  __syncthreads();
  red[t] = v; redi[t] = where;
  __syncthreads();
  for (int s = RAGGED_T / 2; s > 0; s >>= 1) {
    if (t < s) {
      const T o = red[t + s];
      const int64_t oi = redi[t + s];
      if (o > red[t] || (o == red[t] && oi < redi[t])) { red[t] = o; redi[t] = oi; }
    }
    __syncthreads();
  }
  where = redi[0];
  return red[0];
}

}  // namespace ddk
